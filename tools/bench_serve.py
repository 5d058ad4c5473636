#!/usr/bin/env python
"""Batch-1 serving latency on a stream of DISTINCT utterances (BC2013_GST, synthetic weights as in bench.py).

The bench's ``synth_rtf_b1`` repeats one utterance, which the exact-key graphs replay.  A stream of requests almost
never repeats a tuple of mel lengths; this tool times what such a stream gets, three ways in one process:

  eager     FastSpeech2.infer_packed + Generator.infer_packed, every launch from Python
  exact     SynthGraphs()               -- graph 2 keyed on the exact mel lengths
  bucketed  SynthGraphs(bucketed=True)  -- graph 2 keyed on the capacity bucket

Each way is warmed on 30 utterances and timed on 30 OTHER ones (distinct texts, phoneme counts spread over 8..60),
idle GPU -> int16 waveform on the host per utterance; plus the repeat-one replay latency (one utterance, warmed,
through the exact-key graphs: what ``synth_rtf_b1`` measures) for comparison.

  python tools/bench_serve.py [--out profiles/serve_b1_distinct.txt]
"""
import argparse
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report to this file")
    ap.add_argument("--n", type=int, default=30, help="utterances per set (warm set and timed set)")
    ap.add_argument("--frames-per-phone", type=float, default=8.1)
    ap.add_argument("--ladder", default=None, help="capacity ladder to try instead of hip._CAP_LADDER: "
                    "top:step,... with '-' for the open last range, e.g. --ladder=512:32,1024:64,-:128")
    args = ap.parse_args(argv)

    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.infer.graphs import SynthGraphs
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.ops import hip
    from speakingstyle_amd.utils.model import get_vocoder

    if args.ladder:
        hip._CAP_LADDER = tuple((None if t == "-" else int(t), int(st)) for t, st in
                                (part.split(":") for part in args.ladder.split(",")))
    dev = torch.device("cuda", 0)
    pp, mc, tc = load_named("BC2013_GST")
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc).to(dev)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(args.frames_per_phone + 1.0))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    voc = get_vocoder(mc, dev)
    mx = float(pp["preprocessing"]["audio"]["max_wav_value"])
    ref = SyntheticBatches(1, device=dev, seed=17, max_seq_len=mc["max_seq_len"],
                           phone_counts=np.array([14])).make_batch()
    rng = np.random.default_rng(123)

    def utt(T):
        ids = torch.from_numpy(rng.integers(1, 300, size=(1, T))).to(dev)
        return (ref[2][:1], ids, torch.tensor([T], device=dev), T, ref[6][:1], ref[7][:1], ref[8])

    # two sets of new texts from the same distribution: phoneme counts drawn from 8..60, distinct inside each set
    warm_set = [utt(int(t)) for t in rng.permutation(np.arange(8, 61))[: args.n]]
    timed_set = [utt(int(t)) for t in rng.permutation(np.arange(8, 61))[: args.n]]

    def eager(a):
        rows, lens, _ = model.infer_packed(*a)
        return voc.infer_packed(rows, lens, int16_scale=mx), lens

    ways = [("eager", eager, None)]
    for name, kw in (("exact", {}), ("bucketed", {"bucketed": True})):
        sg = SynthGraphs(model, voc, int16_scale=mx, **kw)
        ways.append((name, sg, sg))

    lines = [f"batch-1 text -> int16 wav on the host, BC2013_GST, {args.n} warm-up utterances then {args.n} OTHER "
             f"utterances (distinct texts, phoneme counts {min(int(a[3]) for a in timed_set)}.."
             f"{max(int(a[3]) for a in timed_set)}), ms per utterance",
             f"{'path':10s} {'median':>8s} {'p90':>8s} {'min':>8s} {'max':>8s}   captures replays eager (timed set only)"]
    res = {}
    for name, fn, sg in ways:
        call = (lambda a, f=fn: f(*a)) if sg is not None else fn
        for a in warm_set:
            call(a)[0].cpu()
        before = dict(sg.stats) if sg is not None else None
        ts, pure = [], []
        for a in timed_set:
            seen = None if sg is None else (sg.stats["captures"], sg.stats["eager"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            wav, _ = call(a)
            wav.cpu()
            ts.append(1e3 * (time.perf_counter() - t0))
            pure.append(sg is not None and seen == (sg.stats["captures"], sg.stats["eager"]))
        ts = np.asarray(ts)
        res[name] = float(np.median(ts))
        extra = ""
        if sg is not None:
            d = {k: sg.stats[k] - before[k] for k in ("captures", "replays", "eager")}
            extra = f"   {d['captures']:8d} {d['replays']:7d} {d['eager']:5d}"
            po = ts[np.asarray(pure)]
            if len(po):  # where the time goes: calls that only replayed vs calls that still opened a bucket
                extra += f"   replay-only calls: {len(po)} of {len(ts)}, median {np.median(po):.3f}"
                if len(po) < len(ts):
                    extra += f"; bucket-opening calls: median {np.median(ts[~np.asarray(pure)]):.3f}"
        lines.append(f"{name:10s} {np.median(ts):8.3f} {np.percentile(ts, 90):8.3f} {ts.min():8.3f} {ts.max():8.3f}{extra}")
    # repeat-one: the utterance of synth_rtf_b1 (14 phonemes) replayed through the exact-key graphs
    sg = SynthGraphs(model, voc, int16_scale=mx)
    a = utt(14)
    for _ in range(5):
        sg(*a)[0].cpu()
    ts = []
    for _ in range(args.n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sg(*a)[0].cpu()
        ts.append(1e3 * (time.perf_counter() - t0))
    rep = float(np.median(ts))
    lines.append(f"{'repeat-one':10s} {rep:8.3f} {np.percentile(ts, 90):8.3f} {min(ts):8.3f} {max(ts):8.3f}"
                 f"   (one 14-phoneme utterance, exact-key replay)")
    b = res["bucketed"]
    lines.append(f"bucketed median {b:.3f} ms = {b / rep:.2f} x the repeat-one replay; "
                 f"{res['exact'] / b:.2f} x faster than exact keys, {res['eager'] / b:.2f} x faster than eager; "
                 f"aim <= 2.0 ms: {'met' if b <= 2.0 else 'MISSED'}; "
                 f"below both baselines: {'yes' if b < min(res['exact'], res['eager']) else 'NO'}")
    lines.append(f"ladder {hip._CAP_LADDER}; text bucket 16 phonemes")
    report = "\n".join(lines)
    print(report)
    if args.out:
        with open(args.out, "w") as f:
            f.write(report + "\n")


if __name__ == "__main__":
    main()
