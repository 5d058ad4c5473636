#!/usr/bin/env python
"""Micro-benchmarks of the hot HIP kernels at the headline model's shapes.

Reports achieved TFLOP/s (GEMM-shaped) or GB/s (memory-bound) per kernel, and
the hipBLASLt number for the plain-GEMM equivalent (torch.matmul) as a yardstick.
Usage (GPU box): python tools/bench_kernels.py [--rows 160000] [--iters 20] | --griffin-lim | --dtw | --align | --yin
       | --pyin | --k256 | --prosody | --tsne | --features | --istftnet
"""
import argparse
import functools
import json
import math
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from speakingstyle_amd.ops import hip  # noqa: E402


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters  # ms


def bench_griffin_lim(out_path, rounds=7, n_iters=60):
    """60 Griffin-Lim iterations: the HIP kernels (csrc/k_griffin.hip, one launch per iteration, packed batch)
    against the torch.stft / torch.istft loop of ``audio/stft.py`` (padded batch) on the same GPU.  The two
    alternate in one process, each call timed with device events; the table reports the median and the spread."""
    import numpy as np

    from speakingstyle_amd import ops
    from speakingstyle_amd.audio.stft import TacotronSTFT, griffin_lim

    dev = torch.device("cuda")
    stft = TacotronSTFT().to(dev)
    win = stft.fft_window(dev)
    rng = np.random.default_rng(0)
    workloads = [("1 utterance x 800 frames", [800]),
                 ("16 utterances, 300-850 frames", [int(v) for v in rng.integers(300, 851, size=16)])]

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e)

    lines = [f"Griffin-Lim, {n_iters} iterations, n_fft 1024 / hop 256, fp32, {torch.cuda.get_device_name(0)}",
             f"{rounds} alternating rounds per arm after 2 warm-up rounds; device-event time per call (ms)", "",
             f"{'workload':32s} {'momentum':>8s} {'arm':>22s} {'median':>9s} {'min':>9s} {'max':>9s} {'us/iter':>9s}"]
    for name, lens in workloads:
        B, Tm = len(lens), max(lens)
        g = torch.Generator(device="cpu").manual_seed(1)
        y = (0.5 * torch.sin(2 * math.pi * 220 * torch.arange(256 * (Tm - 1)) / 22050.0)
             + 0.1 * torch.randn(B, 256 * (Tm - 1), generator=g)).clamp(-1, 1).to(dev)
        mag = stft.magnitudes(y)  # [B, 513, Tm]
        for b, n in enumerate(lens):
            mag[b, :, n:] = 0
        ph = 2 * math.pi * torch.rand(mag.shape, generator=g).to(dev)
        rows = torch.cat([mag[b, :, :n].t() for b, n in enumerate(lens)], 0).contiguous()
        ph_rows = torch.cat([ph[b, :, :n].t() for b, n in enumerate(lens)], 0).contiguous()
        for momentum in (0.0, 0.99):
            def run_hip():
                return hip.griffin_lim(rows, 1024, 256, win, n_iters, momentum, init_phase=ph_rows, lengths=lens)

            def run_torch():
                ops.set_backend("reference")  # the torch loop on the GPU tensors
                try:
                    return griffin_lim(mag, stft, n_iters, momentum, init_phase=ph)
                finally:
                    ops.set_backend(None)

            t = {"hip packed (1 launch/iter)": [], "torch.stft/istft loop": []}
            for r in range(rounds + 2):
                for arm, fn in (("hip packed (1 launch/iter)", run_hip), ("torch.stft/istft loop", run_torch)):
                    ms = timed(fn)
                    if r >= 2:
                        t[arm].append(ms)
            for arm, v in t.items():
                v.sort()
                med = v[len(v) // 2]
                lines.append(f"{name:32s} {momentum:8.2f} {arm:>22s} {med:9.3f} {v[0]:9.3f} {v[-1]:9.3f} "
                             f"{1e3 * med / n_iters:9.1f}")
            a, b = t["hip packed (1 launch/iter)"], t["torch.stft/istft loop"]
            lines.append(f"{'':32s} {'':8s} {'torch / hip (medians)':>22s} {b[len(b) // 2] / a[len(a) // 2]:9.2f}")
        lines.append(f"{'':32s} frames: {sum(lens)} packed, {B * Tm} padded")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def dtw_workloads():
    """(name, x, y, x_lens, y_lens) on the CPU: 64 pairs with the LJSpeech ``val.txt`` frame-count distribution
    (phoneme counts x 8.1 frames, as data/synthetic.py draws them) and a +-10 % length mismatch, and one 800 x 850
    pair; D = 13, y a time-warped copy of x plus 0.3 x noise."""
    import numpy as np

    from speakingstyle_amd.data import synthetic

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    counts = synthetic.ljspeech_phone_counts(os.path.join(root, "preprocessed_data", "LJSpeech", "val.txt"))
    rng = np.random.default_rng(0)
    tx = np.clip(np.round(rng.choice(counts, size=64) * 8.1), 16, 1000).astype(np.int64)
    ty = np.maximum(1, np.round(tx * rng.uniform(0.9, 1.1, size=64))).astype(np.int64)
    out = []
    for name, xl, yl in (("64 pairs, LJSpeech val lengths +-10 %", tx.tolist(), ty.tolist()), ("1 pair, 800 x 850", [800], [850])):
        g = torch.Generator().manual_seed(len(xl))
        xs, ys = [], []
        for a, b in zip(xl, yl):
            x = torch.randn(a, 13, generator=g)
            src = torch.round(torch.arange(b, dtype=torch.float64) * ((a - 1) / max(b - 1, 1))).long()
            xs.append(x)
            ys.append(x[src] + 0.3 * torch.randn(b, 13, generator=g))
        out.append((name, torch.cat(xs), torch.cat(ys), xl, yl))
    return out


def bench_dtw(out_path, rounds=3):
    """``ops.dtw`` (csrc/k_dtw.hip: one fwd + one path launch) against the torch wavefront of ``ops/reference.py``
    on the same GPU tensors.  The two arms alternate in one process; every call is timed wall-clock between two device
    synchronisations (the torch arm walks its paths on the host).  The fwd and path kernels are also timed on
    their own with device events."""
    import time

    from speakingstyle_amd import ops
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    lines = [f"Batched DTW, D = 13, fp32, {torch.cuda.get_device_name(0)}",
             f"{rounds} alternating rounds per arm after 1 warm-up round; wall time per call between device syncs (ms);",
             "kernel rows: device-event time of one launch (3 warm-up launches before each), 20 samples", "",
             f"{'workload':40s} {'arm':>24s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    for name, x, y, xl, yl in dtw_workloads():
        x, y = x.to(dev), y.to(dev)
        t = {"hip ops.dtw": [], "torch wavefront": []}
        for r in range(rounds + 1):
            for arm, fn in (("hip ops.dtw", lambda: ops.dtw(x, y, xl, yl)), ("torch wavefront", lambda: ref.dtw(x, y, xl, yl))):
                ms = wall(fn)
                if r >= 1:
                    t[arm].append(ms)
        for arm, v in t.items():
            v.sort()
            lines.append(f"{name:40s} {arm:>24s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}")
        a, b = t["hip ops.dtw"], t["torch wavefront"]
        lines.append(f"{'':40s} {'torch / hip (medians)':>24s} {b[len(b) // 2] / a[len(a) // 2]:10.1f}")
        lines.append(f"{'':40s} {'slowest hip < fastest torch':>24s} {str(a[-1] < b[0]):>10s}")
        plan = hip.DTWPlan(xl, yl, dev)
        ws = hip._workspace(dev, plan.ws_floats)
        cost = torch.empty(plan.P, device=dev)
        path = torch.empty(plan.P, plan.Lmax, 2, device=dev, dtype=torch.int32)
        plen = torch.empty(plan.P, device=dev, dtype=torch.int32)
        assert len(plan.chunks) == 1
        for arm, fn in (("dtw_fwd kernel", lambda: hip.dtw_fwd_raw(x, y, plan, plan.chunks[0], ws, cost)),
                        ("dtw_path kernel", lambda: hip.dtw_path_raw(plan, plan.chunks[0], ws, path, plen))):
            v = sorted(timeit(fn, 1) for _ in range(20))
            lines.append(f"{name:40s} {arm:>24s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}")
        lines.append(f"{'':40s} cells: {sum(a * b for a, b in zip(xl, yl))}, plane bytes: {plan.chunks[0][2]}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def align_workload(batch=200):
    """(lp [B, Tmax, Nmax] on the CPU, t_lens, n_lens): ``batch`` utterances with the LJSpeech ``val.txt`` phoneme
    counts and 8.1 frames per phoneme on average (as data/synthetic.py draws them); lp = log_softmax(3 randn) over
    each utterance's own tokens."""
    import numpy as np

    from speakingstyle_amd.data import synthetic

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    counts = synthetic.ljspeech_phone_counts(os.path.join(root, "preprocessed_data", "LJSpeech", "val.txt"))
    rng = np.random.default_rng(0)
    nl = rng.choice(counts, size=batch).astype(np.int64)
    tl = np.clip(np.round(nl * rng.normal(8.1, 0.8, size=batch)), nl, 1000).astype(np.int64)
    g = torch.Generator().manual_seed(batch)
    lp = 3.0 * torch.randn(batch, int(tl.max()), int(nl.max()), generator=g)
    pad = torch.arange(int(nl.max())).view(1, 1, -1) >= torch.from_numpy(nl).view(-1, 1, 1)
    return torch.log_softmax(lp.masked_fill(pad, float("-inf")), -1), tl.tolist(), nl.tolist()


def bench_align(out_path, rounds=3):
    """``ops.align_forward_sum`` forward + backward and ``ops.align_mas`` (csrc/k_align.hip) against the torch
    reference loop of ``ops/reference.py`` and, for the forward-sum, ``F.ctc_loss`` forward + backward on the same
    lattice size, all on the same GPU tensors.  The arms alternate in one process; every call is timed wall-clock
    between two device synchronisations.  The kernels are also timed on their own with device events."""
    import time

    import torch.nn.functional as F

    from speakingstyle_amd import ops
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")
    lp, tl, nl = align_workload()
    lp = lp.to(dev)
    B, Tmax, Nmax = lp.shape
    cells = sum(a * b for a, b in zip(tl, nl))

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def fsum(fn):
        x = lp.detach().requires_grad_(True)
        fn(x, tl, nl).sum().backward()
        return x.grad

    # the CTC yardstick: same [T, B, N + 1] lattice size, targets 1..N_b (blank 0 unused by the labels)
    ctc_lp = torch.log_softmax(torch.randn(Tmax, B, Nmax + 1, device=dev), -1)
    ctc_tg = torch.arange(1, Nmax + 1, device=dev).unsqueeze(0).repeat(B, 1)
    ctc_tl, ctc_nl = torch.tensor(tl, device=dev), torch.tensor(nl, device=dev)

    def ctc():
        x = ctc_lp.detach().requires_grad_(True)
        F.ctc_loss(x, ctc_tg, ctc_tl, ctc_nl, reduction="sum").backward()

    arms = [("forward-sum fwd + bwd", "hip ops.align_forward_sum", lambda: fsum(ops.align_forward_sum)),
            ("forward-sum fwd + bwd", "torch reference loop", lambda: fsum(ref.align_forward_sum)),
            ("forward-sum fwd + bwd", "F.ctc_loss fwd + bwd", ctc),
            ("MAS durations", "hip ops.align_mas", lambda: ops.align_mas(lp, tl, nl)),
            ("MAS durations", "torch reference loop", lambda: ref.align_mas(lp, tl, nl))]
    t = {a[:2]: [] for a in arms}
    for r in range(rounds + 1):
        for what, arm, fn in arms:
            ms = wall(fn)
            if r >= 1:
                t[(what, arm)].append(ms)
    lines = [f"Alignment learning kernels, fp32, {torch.cuda.get_device_name(0)}",
             f"batch {B}, LJSpeech val.txt phoneme counts (mean {sum(nl) / B:.0f}, max {max(nl)}), "
             f"{sum(tl) / sum(nl):.1f} frames per phoneme: lattice [{B}, {Tmax}, {Nmax}], {cells} cells inside "
             f"({cells * 4 / 1e6:.1f} MB of lp)",
             f"{rounds} alternating rounds per arm after 1 warm-up round; wall time per call between device syncs (ms);",
             "kernel rows: device-event time of one launch (3 warm-up launches before each), 20 samples", "",
             f"{'workload':24s} {'arm':>28s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    med = {}
    for (what, arm), v in t.items():
        v.sort()
        med[(what, arm)] = v[len(v) // 2]
        lines.append(f"{what:24s} {arm:>28s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}")
    f_hip = med[("forward-sum fwd + bwd", "hip ops.align_forward_sum")]
    lines.append(f"{'':24s} {'torch loop / hip (medians)':>28s} "
                 f"{med[('forward-sum fwd + bwd', 'torch reference loop')] / f_hip:10.1f}")
    lines.append(f"{'':24s} {'ctc_loss / hip (medians)':>28s} "
                 f"{med[('forward-sum fwd + bwd', 'F.ctc_loss fwd + bwd')] / f_hip:10.1f}")
    lines.append(f"{'':24s} {'MAS torch loop / hip':>28s} "
                 f"{med[('MAS durations', 'torch reference loop')] / med[('MAS durations', 'hip ops.align_mas')]:10.1f}")
    # the kernels alone
    td, nd, W = hip._align_plan(lp, tl, nl, "bench")
    alpha, grad = torch.empty_like(lp), torch.empty_like(lp)
    nll, gn = torch.empty(B, device=dev), torch.ones(B, device=dev)
    dur = torch.empty(B, Nmax, device=dev, dtype=torch.int32)
    ws = hip._workspace(dev, 2 * int(hip.lib().ssamd_align_mas_plane_words(B, Tmax, W)))
    L, P, S = hip.lib(), hip._ptr, hip._stream
    kernels = [("align_fwd (sum) kernel", 2, lambda: L.ssamd_align_fsum_fwd(P(lp), P(td), P(nd), B, Tmax, Nmax, W, P(alpha), P(nll), S())),
               ("align_fsum_bwd kernel", 3, lambda: L.ssamd_align_fsum_bwd(P(lp), P(alpha), P(nll), P(gn), P(td), P(nd), B, Tmax, Nmax, W, P(grad), S())),
               ("align_fwd (max) + path", 1, lambda: L.ssamd_align_mas(P(lp), P(td), P(nd), B, Tmax, Nmax, W, P(ws), P(nll), P(dur), S()))]
    lines += ["", f"{'kernel':24s} {'':>28s} {'median':>10s} {'min':>10s} {'max':>10s} {'GB/s':>8s} {'% of 8 TB/s':>12s}"]
    for name, planes, fn in kernels:
        v = sorted(timeit(fn, 1) for _ in range(20))
        # traffic that has to move: `planes` fp32 planes over the cells inside the lattices (the backward also zeroes
        # the padding of its slab, counted with the full slab)
        moved = (planes - 1) * cells * 4 + (B * Tmax * Nmax * 4 if "bwd" in name else cells * 4)
        gbs = moved / (v[len(v) // 2] * 1e-3) / 1e9
        lines.append(f"{name:24s} {'':>28s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f} {gbs:8.0f} {100 * gbs / 8000:11.1f}%")
    lines += ["", "The recurrences are latency-bound, not bandwidth-bound: a wave advances one frame per ~2 transcendental",
              "round trips and an utterance occupies ceil(N / 64) waves, so the batch keeps a few hundred waves of the",
              "chip busy; the last column says how far that is from moving the same planes at HBM speed."]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def yin_workloads(sr=22050, hop=256):
    """(name, packed wav on the CPU, sample counts): 64 utterances with the LJSpeech ``val.txt`` frame-count
    distribution (as ``dtw_workloads``) and one utterance of 800 frames.  The signal is six harmonics of an F0 that
    wanders over 90 .. 250 Hz under a 3 Hz envelope, with noise-only stretches and 1 % noise: voiced, unvoiced and
    quiet frames, as speech has them."""
    import numpy as np

    from speakingstyle_amd.data import synthetic

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    counts = synthetic.ljspeech_phone_counts(os.path.join(root, "preprocessed_data", "LJSpeech", "val.txt"))
    rng = np.random.default_rng(0)
    frames = np.clip(np.round(rng.choice(counts, size=64) * 8.1), 16, 1000).astype(np.int64)
    out = []
    for name, fr in (("64 utterances, LJSpeech val lengths", frames.tolist()), ("1 utterance, 800 frames", [800])):
        wavs = []
        for T in fr:
            n = hop * (T - 1)
            t = np.arange(n) / sr
            f0 = 170 + 80 * np.sin(2 * np.pi * 1.1 * t + rng.uniform(0, 6.28))
            ph = 2 * np.pi * np.cumsum(f0) / sr
            s = sum(0.6 ** k * np.sin((k + 1) * ph + rng.uniform(0, 6.28)) for k in range(6))
            voiced = np.sin(2 * np.pi * 0.8 * t + rng.uniform(0, 6.28)) > -0.4
            x = np.where(voiced, 0.3 * (0.55 + 0.45 * np.sin(2 * np.pi * 3 * t)) * s, 0.0) + 0.01 * rng.standard_normal(n)
            wavs.append(0.5 * x / np.abs(x).max())
        out.append((name, torch.from_numpy(np.concatenate(wavs)).float(), [len(w) for w in wavs]))
    return out


def bench_yin(out_path, rounds=5, sr=22050, hop=256):
    """``ops.yin`` (csrc/k_pitch.hip: one launch) against the torch reference ``ops.reference.yin`` on the same GPU
    tensors and against numpy ``data.preprocess.yin_f0`` on the host.  The arms alternate in one process; every call is
    timed wall-clock between two device synchronisations; the kernel alone is also timed with device events.  The
    deviations of the kernel and of the float32 torch reference from the float64 torch reference on the same
    workloads go to ``yin_numerics.txt`` beside the table."""
    import time

    import numpy as np

    from speakingstyle_amd import ops
    from speakingstyle_amd.data.preprocess import yin_f0
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    lines = [f"Batched YIN, sr {sr} / hop {hop} / frame 1024 (lags 1 .. 311), fp32, {torch.cuda.get_device_name(0)}",
             f"{rounds} alternating rounds per arm after 1 warm-up round; wall time per call between device syncs (ms);",
             "kernel row: device-event time of one launch (3 warm-up launches before each), 20 samples", "",
             f"{'workload':38s} {'arm':>28s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    num = [f"YIN kernel (csrc/k_pitch.hip) against the float64 torch reference, {torch.cuda.get_device_name(0)}; the "
           "workloads of profiles/yin.txt", "",
           "ref32 = the float32 torch reference on the same GPU, hip = the kernel; cmnd: maximum absolute deviation of the",
           "plane from float64; disagree: frames whose voicing differs from float64 or whose F0 differs by more than 1e-3",
           "relative; f0: maximum relative F0 error over the other voiced frames", "",
           f"{'workload':38s} {'frames':>7s} {'voiced':>7s} {'max cmnd':>10s} {'cmnd ref32':>11s} {'cmnd hip':>10s} "
           f"{'dis ref32':>9s} {'dis hip':>8s} {'f0 ref32':>10s} {'f0 hip':>10s}"]
    for name, wav_h, lens in yin_workloads(sr, hop):
        wav = wav_h.to(dev)
        host = np.split(wav_h.numpy(), np.cumsum(lens)[:-1])
        arms = (("hip ops.yin", lambda: ops.yin(wav, lens, sr, hop)),
                ("torch reference, same GPU", lambda: ref.yin(wav, lens, sr, hop)),
                ("numpy yin_f0, host", lambda: [yin_f0(w, sr, hop) for w in host]))
        t = {a: [] for a, _ in arms}
        for r in range(rounds + 1):
            for arm, fn in arms:
                ms = wall(fn)
                if r >= 1:
                    t[arm].append(ms)
        for arm, v in t.items():
            v.sort()
            lines.append(f"{name:38s} {arm:>28s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}")
        a = t["hip ops.yin"]
        for arm in ("torch reference, same GPU", "numpy yin_f0, host"):
            b = t[arm]
            lines.append(f"{'':38s} {arm + ' / hip':>28s} {b[len(b) // 2] / a[len(a) // 2]:10.1f}")
        _, frames, tau_min, tau_max = ref.yin_plan(wav, lens, sr, hop)
        pack = hip.YinPack(lens, frames, dev)
        f0 = torch.empty(pack.R, device=dev)

        def launch():
            hip._check(hip.lib().ssamd_yin(hip._ptr(wav), hip._ptr(pack.off), hip._ptr(pack.n), hip._ptr(pack.rows), pack.R,
                                           hop, 1024, tau_min, tau_max, float(sr), 0.15, hip._ptr(f0), None, hip._stream()),
                       "ssamd_yin")

        v = sorted(timeit(launch, 1) for _ in range(20))
        lines.append(f"{name:38s} {'yin_kernel':>28s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}")
        flop = 3.0 * pack.R * tau_max * 512
        lines.append(f"{'':38s} frames: {pack.R}, samples: {sum(lens)}, {flop / 1e9:.2f} GFLOP in the difference "
                     f"function -> {flop / (v[len(v) // 2] * 1e-3) / 1e12:.2f} TFLOP/s at the median")
        f64, _, c64 = ref.yin(wav.double(), lens, sr, hop, return_cmnd=True)
        row = [f"{name:38s} {pack.R:7d} {int((f64 > 0).sum()):7d} {float(c64.max()):10.3e}"]
        got = {"ref32": ref.yin(wav, lens, sr, hop, return_cmnd=True), "hip": ops.yin(wav, lens, sr, hop, return_cmnd=True)}
        dev_c, dis, err = {}, {}, {}
        for k, (f, _, c) in got.items():
            f = f.double()
            dev_c[k] = float((c.double() - c64).abs().max())
            both = (f > 0) & (f64 > 0)
            rel = (f - f64).abs() / f64.clamp(min=1.0)
            bad = ((f > 0) != (f64 > 0)) | (both & (rel > 1e-3))
            dis[k] = int(bad.sum())
            err[k] = float(rel[both & ~bad].max()) if (both & ~bad).any() else 0.0
        row.append(f"{dev_c['ref32']:11.3e} {dev_c['hip']:10.3e} {dis['ref32']:9d} {dis['hip']:8d} {err['ref32']:10.3e} "
                   f"{err['hip']:10.3e}")
        num.append(" ".join(row))
    for text, path in (("\n".join(lines) + "\n", out_path),
                       ("\n".join(num) + "\n", out_path and os.path.join(os.path.dirname(os.path.abspath(out_path)),
                                                                         "yin_numerics.txt"))):
        print(text, end="", flush=True)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


def bench_pyin(out_path, rounds=3, sr=22050, hop=256):
    """``ops.pyin`` (csrc/k_pitch.hip's cmnd plane, then csrc/k_pyin.hip: candidates and Viterbi decode) against the
    torch reference ``ops.reference.pyin`` on the same GPU tensors and on the host, on the workloads of ``--yin``.  The
    arms alternate in one process; every call is timed wall-clock between two device synchronisations; the three
    kernels alone are timed with device events.  The cost of the waveform-level metrics with either tracker is timed
    on the batch against a noisy copy of itself.  The deviations of the kernels and of the float32 torch reference from
    the float64 torch reference on the same workloads go to ``pyin_numerics.txt`` beside the table."""
    import time

    from speakingstyle_amd import ops
    from speakingstyle_amd.analysis.objective import wave_metrics
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")
    pp = load_named("LJSpeech")[0]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def med(v):
        v = sorted(v)
        return f"{v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}"

    B = hip.PYIN_BINS_PER_THREAD
    lines = [f"Probabilistic YIN, sr {sr} / hop {hop} / frame 1024 (lags 1 .. 311, 839 bins, band of 101), fp32, "
             f"{torch.cuda.get_device_name(0)}",
             f"{rounds} alternating rounds per arm after 1 warm-up round; wall time per call between device syncs (ms);",
             "kernel rows: device-event time of one launch (3 warm-up launches before each), 20 samples;",
             f"pyin_viterbi_kernel: {1024 // B} threads per utterance, {B} bins per thread on a sliding window of the "
             "log-triangle table,", "forward pass and back-trace in one launch", "",
             f"{'workload':38s} {'arm':>30s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    num = [f"pYIN kernels (csrc/k_pyin.hip) against the float64 torch reference, {torch.cuda.get_device_name(0)}; the "
           "workloads of profiles/pyin.txt", "",
           "ref32 = the float32 torch reference on the same GPU, hip = the kernels; obs dis: frames whose set of non-zero",
           "bins differs from float64; obs / vp: maximum absolute deviation of the candidate plane / of voiced_prob from",
           "float64 over the other frames; track dis: frames whose voicing or decoded bin differs from float64", "",
           f"{'workload':38s} {'frames':>7s} {'voiced':>7s} {'obs dis ref32':>13s} {'obs dis hip':>11s} {'obs ref32':>10s} "
           f"{'obs hip':>10s} {'vp ref32':>10s} {'vp hip':>10s} {'track dis ref32':>15s} {'track dis hip':>13s}"]
    for name, wav_h, lens in yin_workloads(sr, hop):
        wav = wav_h.to(dev)
        arms = (("hip ops.pyin", lambda: ops.pyin(wav, lens, sr, hop)),
                ("hip ops.yin", lambda: ops.yin(wav, lens, sr, hop)),
                ("torch reference, same GPU", lambda: ref.pyin(wav, lens, sr, hop)),
                ("torch reference, host", lambda: ref.pyin(wav_h, lens, sr, hop)))
        t = {a: [] for a, _ in arms}
        for r in range(rounds + 1):
            for arm, fn in arms:
                ms = wall(fn)
                if r >= 1:
                    t[arm].append(ms)
        for arm, v in t.items():
            lines.append(f"{name:38s} {arm:>30s} {med(v)}")
        a = sorted(t["hip ops.pyin"])
        for arm in ("torch reference, same GPU", "torch reference, host"):
            b = sorted(t[arm])
            lines.append(f"{'':38s} {arm + ' / hip':>30s} {b[len(b) // 2] / a[len(a) // 2]:10.1f}")
        _, frames, tau_min, tau_max, NB, h = ref.pyin_plan(wav, lens, sr, hop)
        pack = hip.YinPack(lens, frames, dev)
        f0 = torch.empty(pack.R, device=dev)
        cm = torch.empty(pack.R, tau_max + 1, device=dev)

        def launch_yin():
            hip._check(hip.lib().ssamd_yin(hip._ptr(wav), hip._ptr(pack.off), hip._ptr(pack.n), hip._ptr(pack.rows), pack.R,
                                           hop, 1024, tau_min, tau_max, float(sr), 0.15, hip._ptr(f0), hip._ptr(cm),
                                           hip._stream()), "ssamd_yin")

        launch_yin()
        obs, vp = hip.pyin_obs(cm, sr, tau_min, tau_max)
        plans = {b: hip.PyinPlan(frames, NB, h, dev, bins_per_thread=b) for b in (2, 4)}
        plan = plans[B]
        ws = hip._workspace(dev, plan.ws_floats)

        def launch_obs():
            hip._check(hip.lib().ssamd_pyin_obs(hip._ptr(cm), pack.R, tau_min, tau_max, float(sr), 71.0, 240.0, NB, 0.01,
                                                hip._ptr(obs), hip._ptr(vp), hip._stream()), "ssamd_pyin_obs")

        def launch_viterbi(pl=plan):
            for c0, c1, _ in pl.chunks:
                hip._check(hip.lib().ssamd_pyin_viterbi(hip._ptr(obs), hip._ptr(vp), hip._ptr(pl.meta[4 * c0:]), c1 - c0,
                                                        NB, h, pl.bins_per_thread, hip._ptr(pl.tab), math.log(0.99),
                                                        math.log(0.01), 71.0, 240.0, hip._ptr(ws), hip._ptr(f0),
                                                        hip._stream()), "ssamd_pyin_viterbi")

        tracks = {}
        for b, pl in plans.items():  # both forms of the decoder, alternating; they must decode the same track
            launch_viterbi(pl)
            tracks[b] = f0.clone()
        same = torch.equal(tracks[2], tracks[4])
        tv = {b: [] for b in plans}
        for _ in range(20):
            for b, pl in plans.items():
                tv[b].append(timeit(lambda: launch_viterbi(pl), 1))
        for kname, fn in (("yin_kernel (with the plane)", launch_yin), ("pyin_obs_kernel", launch_obs)):
            lines.append(f"{name:38s} {kname:>30s} {med([timeit(fn, 1) for _ in range(20)])}")
        for b in plans:
            kname = f"pyin_viterbi_kernel<{b}>" + (" (used)" if b == B else "")
            lines.append(f"{name:38s} {kname:>30s} {med(tv[b])}")
        lines.append(f"{'':38s} the two forms decode {'the same track, bitwise' if same else 'DIFFERENT tracks'}")
        v = sorted(tv[B])
        lines.append(f"{'':38s} frames: {pack.R} (longest utterance {max(frames)}), back-pointer planes "
                     f"{sum(c[2] for c in plan.chunks) / 2 ** 20:.1f} MiB in {len(plan.chunks)} launch(es) -> "
                     f"{1e3 * v[len(v) // 2] / max(frames):.2f} us per frame of the longest utterance at the median")
        if len(lens) > 1:
            noisy = (wav + 0.02 * torch.randn(wav.shape, device=dev, generator=torch.Generator(dev).manual_seed(0))).clamp(-1, 1)
            tw = {k: [] for k in ("yin", "pyin")}
            for r in range(rounds + 1):
                for k in tw:
                    ms = wall(lambda: wave_metrics(noisy, lens, wav, lens, pp, tracker=k))
                    if r >= 1:
                        tw[k].append(ms)
            for k, v in tw.items():
                lines.append(f"{name:38s} {'wave_metrics, tracker=' + k:>30s} {med(v)}")
        ref64 = ref.pyin(wav.double(), lens, sr, hop, return_obs=True)
        got = {"ref32": ref.pyin(wav, lens, sr, hop, return_obs=True), "hip": ops.pyin(wav, lens, sr, hop, return_obs=True)}
        st = {}
        for k, (f, _, p, o) in got.items():
            bad = ((o > 0) != (ref64[3] > 0)).any(1)
            state = [torch.where(x > 0, torch.round(240 * torch.log2(x.double().clamp(min=1.0) / 71.0)), -torch.ones_like(x.double()))
                     for x in (f, ref64[0])]
            st[k] = (int(bad.sum()), float((o.double() - ref64[3])[~bad].abs().max()),
                     float((p.double() - ref64[2])[~bad].abs().max()), int((state[0] != state[1]).sum()))
        num.append(f"{name:38s} {pack.R:7d} {int((ref64[0] > 0).sum()):7d} {st['ref32'][0]:13d} {st['hip'][0]:11d} "
                   f"{st['ref32'][1]:10.3e} {st['hip'][1]:10.3e} {st['ref32'][2]:10.3e} {st['hip'][2]:10.3e} "
                   f"{st['ref32'][3]:15d} {st['hip'][3]:13d}")
    for text, path in (("\n".join(lines) + "\n", out_path),
                       ("\n".join(num) + "\n", out_path and os.path.join(os.path.dirname(os.path.abspath(out_path)),
                                                                         "pyin_numerics.txt"))):
        print(text, end="", flush=True)
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


def bench_k256(out_path, rounds=5, iters=20):
    """The K = 256 Linear GEMMs of the training step (QKV forward, attention fc forward / data gradient, the w_2
    data gradient with its ReLU bitmask): the tile kernels (gemm_k256 = 0) against the weight-stationary
    streaming kernel (= 1) in one process, arms interleaved, `rounds` rounds of `iters` launches each.  Decoder
    rows (100 352), encoder rows (14 336) and a row sweep for the crossover.  The inputs rotate over four
    copies so that a launch does not find its rows in the Infinity Cache from the launch before."""
    dev = "cuda"
    lib = hip.lib()
    lines = ["K = 256 GEMMs, us per launch: tile kernels (old) vs weight-stationary streaming kernel (new); "
             f"{rounds} interleaved rounds x {iters} launches; floor = bytes / 6.2 TB/s",
             f"{'rows':>7} {'N':>5} {'epilogue':>8} {'old min..max':>15} {'new min..max':>15} {'new/old':>8} "
             f"{'floor':>6}  verdict"]
    print(lines[0] + "\n" + lines[1], flush=True)
    torch.manual_seed(0)
    for M in (100352, 14336, 81920, 69632, 50176, 28672, 20480, 8192, 4096, 2048):
        xs = [(torch.randn(1, M, 256, device=dev) / 16).to(torch.bfloat16) for _ in range(4)]
        for N, epi in ((256, "-"), (768, "bias"), (1024, "mask")):
            w = (torch.randn(N, 1, 256, device=dev) / 16).to(torch.bfloat16)
            b = torch.randn(N, device=dev) if epi == "bias" else None
            mk = torch.randint(0, 256, (M, N // 8), device=dev, dtype=torch.uint8) if epi == "mask" else None
            it = [0]

            def run():
                it[0] += 1
                x = xs[it[0] & 3]
                if mk is not None:
                    return hip.conv_gemm_mask_raw(x, w, None, 1, M, 256, 1, 0, N, 0, mask_in=mk)
                return hip.conv_gemm_raw(x, w, b, 1, M, 256, 1, 1, 0, N, 0)

            t = {0: [], 1: []}
            try:
                for _ in range(rounds):
                    for arm in (0, 1):
                        lib.ssamd_gemm_set_k256(arm)
                        t[arm].append(timeit(run, iters) * 1e3)
            finally:
                lib.ssamd_gemm_set_k256(-1)
            floor = (M * 512 + M * N * 2 + N * 512 + (M * N // 8 if mk is not None else 0)) / 6.2e6
            wins = max(t[1]) < min(t[0])
            line = (f"{M:7d} {N:5d} {epi:>8} {min(t[0]):7.1f}..{max(t[0]):<6.1f} {min(t[1]):7.1f}..{max(t[1]):<6.1f} "
                    f"{sorted(t[1])[rounds // 2] / sorted(t[0])[rounds // 2]:8.3f} {floor:6.1f}  "
                    f"{'new wins every round' if wins else 'no clear win'}")
            lines.append(line)
            print(line, flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def prosody_workload():
    """The 64 pairs of ``dtw_workloads`` (LJSpeech ``val.txt`` lengths) with what a transfer needs on top, on the CPU:
    phoneme durations that sum to every x length (the pair's phoneme count, at least one frame each), an F0 track with
    unvoiced stretches, an energy track and normalised pitch predictions.
    -> (x, y, x_lens, y_lens, src_dur [64, Nmax] int32, src_lens, f0, energy, pred_pitch)"""
    import numpy as np

    from speakingstyle_amd.data import synthetic

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    counts = synthetic.ljspeech_phone_counts(os.path.join(root, "preprocessed_data", "LJSpeech", "val.txt"))
    n = np.random.default_rng(0).choice(counts, size=64)  # the draw of dtw_workloads
    _, x, y, xl, yl = dtw_workloads()[0]
    rng = np.random.default_rng(1)
    n = np.minimum(n, np.asarray(xl))
    dur = np.zeros((64, int(n.max())), dtype=np.int32)
    for p in range(64):
        dur[p, :n[p]] = 1 + rng.multinomial(xl[p] - n[p], np.ones(n[p]) / n[p])
    ry = sum(yl)
    f0 = 180.0 + 60.0 * np.sin(np.arange(ry) / 23.0) + rng.normal(0, 5, ry)
    f0 = np.where(np.convolve(rng.standard_normal(ry + 8), np.ones(9) / 9, "valid") > -0.05, f0, 0.0)
    return (x, y, xl, yl, torch.from_numpy(dur), torch.from_numpy(n.astype(np.int32)), torch.from_numpy(f0).float(),
            torch.from_numpy(rng.uniform(1, 60, ry)).float(), torch.from_numpy(rng.standard_normal(dur.shape)).float())


@functools.lru_cache(maxsize=None)
def _resource_remarks(src):
    """The compiler's remarks for one compile of ``src`` (a file with many kernels is compiled once)."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-c", os.path.join(csrc, src), "--offload-arch=gfx950",
           "-std=c++17", "-O3", "-I", csrc, "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull]
    return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600).stdout


def _kernel_resources(src, name):
    """Register / scratch / LDS figures of kernel ``name`` from a compile of ``src`` for gfx950 (remarks of
    ``-Rpass-analysis=kernel-resource-usage``)."""
    try:
        remarks = _resource_remarks(src)
    except (OSError, subprocess.TimeoutExpired) as e:
        return [f"compile figures not available: {e}"]
    keep, on = [], False
    for line in remarks.splitlines():
        if "remark:" not in line:
            continue
        text = line.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if text.startswith("Function Name:"):
            on = name in text
        if on and text.split(":")[0] in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill",
                                         "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"):
            keep.append(text)
    return keep or ["compile figures not available: no remarks for " + name]


STYLEMAP_KERNELS = ("tsne_pairdist_kernel", "tsne_perplexity_kernel", "tsne_planesum_kernel", "tsne_symmetrise_kernel",
                    "tsne_grad_kernel", "tsne_update_kernel", "kmeans_far_kernel", "kmeans_pick_kernel",
                    "kmeans_assign_kernel", "kmeans_finish_kernel")


def bench_tsne(out_path, sizes=(1024, 4096, 13100), dim=512, n_iter=750, rounds=3):
    """The style-map ops (csrc/k_stylemap.hip) against the torch references of ``ops/reference.py`` on the same GPU
    tensors (float32), arms alternating in one process, wall time between device synchronisations: affinities, one
    gradient evaluation, the whole descent, k-means (k = 10).  Where the reference's descent would run for minutes it is
    timed over 20 iterations and scaled, and the row says so.  scikit-learn's TSNE on the host, where it imports:
    ``exact`` at N = 1024, ``barnes_hut`` above."""
    import time

    from speakingstyle_amd import ops
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def row(name, arm, v, note=""):
        v = sorted(v)
        return f"{name:34s} {arm:>24s} {v[len(v) // 2]:12.3f} {v[0]:12.3f} {v[-1]:12.3f}  {note}"

    lines = [f"Style map: exact t-SNE and k-means, fp32, D = {dim}, {torch.cuda.get_device_name(0)}",
             "kernels of csrc/k_stylemap.hip, compiled for gfx950:"]
    for k in STYLEMAP_KERNELS:
        lines.append(f"  {k}: " + "; ".join(_kernel_resources("k_stylemap.hip", k)))
    lines += [f"{rounds} alternating rounds per arm after 1 warm-up round (the {n_iter}-iteration rows: 1 round); wall "
              "time per call between device syncs (ms)", "",
              f"{'workload':34s} {'arm':>24s} {'median':>12s} {'min':>12s} {'max':>12s}"]
    for n in sizes:
        g = torch.Generator().manual_seed(n)
        centres = torch.randn(10, dim, generator=g) * 3.0
        x = (centres[torch.randint(0, 10, (n,), generator=g)] + torch.randn(n, dim, generator=g)).to(dev)
        perp = 30.0
        P = ops.tsne_affinities(x, perp)
        y = (torch.randn(n, 2, generator=g) * 5.0).to(dev)
        arms = [("affinities", lambda: ops.tsne_affinities(x, perp), lambda: ref.tsne_affinities(x, perp)),
                ("one gradient", lambda: ops.tsne_gradient(P, y, 1.0), lambda: ref.tsne_gradient(P, y, 1.0)),
                ("k-means k=10", lambda: ops.kmeans(x, 10), lambda: ref.kmeans(x, 10))]
        for what, hip_fn, ref_fn in arms:
            t = {"hip": [], "torch reference": []}
            for r in range(rounds + 1):
                for arm, fn in (("hip", hip_fn), ("torch reference", ref_fn)):
                    ms = wall(fn)
                    if r >= 1:
                        t[arm].append(ms)
            name = f"N = {n}: {what}"
            for arm, v in t.items():
                lines.append(row(name, arm, v))
            h, q = sorted(t["hip"]), sorted(t["torch reference"])
            lines.append(f"{'':34s} {'torch / hip (medians)':>24s} {q[len(q) // 2] / h[len(h) // 2]:12.1f}")
            print(lines[-3] + "\n" + lines[-2] + "\n" + lines[-1], flush=True)
        name = f"N = {n}: {n_iter} iterations"
        wall(lambda: hip.tsne(x, perp, 20, 10, P=P))
        out = {}
        lines.append(row(name, "hip", [wall(lambda: out.update(r=hip.tsne(x, perp, n_iter, 250, P=P)))],
                     f"final KL {out['r'][1][-1]:.4f}"))
        short = n_iter if n <= 4096 else 20
        wall(lambda: ref.tsne(x, perp, 3, 1, P=P))
        ms = wall(lambda: out.update(q=ref.tsne(x, perp, short, min(250, short // 2), P=P)))
        note = f"final KL {out['q'][1][-1]:.4f}" if short == n_iter else f"{short} iterations timed, scaled to {n_iter}"
        lines.append(row(name, "torch reference", [ms * n_iter / short], note))
        print(lines[-2] + "\n" + lines[-1], flush=True)
        try:
            from sklearn.manifold import TSNE
        except ImportError:
            lines.append(f"{name:34s} {'scikit-learn (host)':>24s} not installed")
            continue
        method = "exact" if n <= 1024 else "barnes_hut"
        xs = x.cpu().numpy()
        t0 = time.perf_counter()
        sk = TSNE(perplexity=perp, max_iter=n_iter, method=method, init="pca", random_state=0,
                  n_iter_without_progress=n_iter).fit(xs)
        lines.append(row(name, f"scikit-learn {method}", [1e3 * (time.perf_counter() - t0)],
                         f"host, {os.cpu_count()} logical CPUs seen; KL {sk.kl_divergence_:.4f}"))
        print(lines[-1], flush=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


def bench_prosody(out_path, rounds=5):
    """``ops.prosody_transfer`` (csrc/k_prosody.hip: one launch) against the torch reference of ``ops/reference.py`` on
    the same GPU tensors, arms alternating in one process, wall time between device synchronisations; the kernel on its
    own with device events; and ``infer.transfer.synthesize_like`` against the plain packed synthesis of one
    utterance (LJSpeech model and HiFi-GAN V1 with random weights, ~8 frames per phoneme)."""
    import time

    from speakingstyle_amd import ops
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def row(name, arm, v):
        v = sorted(v)
        return f"{name:40s} {arm:>28s} {v[len(v) // 2]:10.3f} {v[0]:10.3f} {v[-1]:10.3f}"

    x, y, xl, yl, dur, nl, f0, en, pred = prosody_workload()
    _, path, plen = ops.dtw(x.to(dev), y.to(dev), xl, yl)
    a = (path, plen, dur.to(dev), nl.to(dev), xl, yl, f0.to(dev), en.to(dev), pred.to(dev), (180.0, 45.0), (20.0, 12.0),
         "relative")
    lines = [f"Prosody transfer, fp32, {torch.cuda.get_device_name(0)}",
             "prosody_transfer_kernel, compiled for gfx950: " + "; ".join(_kernel_resources("k_prosody.hip",
                                                                                           "prosody_transfer_kernel")),
             f"{rounds} alternating rounds per arm after 1 warm-up round; wall time per call between device syncs (ms);",
             "device-event row: one call of the op, the kernel and the upload of its offset table (3 warm-up calls before each), 20 samples", "",
             f"{'workload':40s} {'arm':>28s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    name = "64 utterances, LJSpeech val lengths"
    t = {"hip ops.prosody_transfer": [], "torch reference": []}
    for r in range(rounds + 1):
        for arm, fn in (("hip ops.prosody_transfer", lambda: ops.prosody_transfer(*a)),
                        ("torch reference", lambda: ref.prosody_transfer(*a))):
            ms = wall(fn)
            if r >= 1:
                t[arm].append(ms)
    for arm, v in t.items():
        lines.append(row(name, arm, v))
    h, q = sorted(t["hip ops.prosody_transfer"]), sorted(t["torch reference"])
    lines.append(f"{'':40s} {'torch / hip (medians)':>28s} {q[len(q) // 2] / h[len(h) // 2]:10.1f}")
    lines.append(row(name, "op, device events", [timeit(lambda: ops.prosody_transfer(*a), 1) for _ in range(20)]))
    got, want = ops.prosody_transfer(*a), ref.prosody_transfer(*a)
    lines.append(f"{'':40s} frames: {sum(yl)} recorded / {sum(xl)} synthesized, tokens: {int(nl.sum())}; rec_dur equal: "
                 f"{torch.equal(got[0], want[0])}, largest pitch difference {float((got[1] - want[1]).abs().max()):.2e}")

    # one utterance end to end
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.infer.transfer import recording_features, synthesize_like
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.models.hifigan import Generator, default_config

    configs = load_named("LJSpeech")
    pp, mc = configs[0], configs[1]
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc).to(dev)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(9.1))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    torch.manual_seed(1)
    voc = Generator(default_config()).eval().fold_weight_norm().to(dev)
    b = SyntheticBatches(1, device=dev, seed=3, max_seq_len=mc["max_seq_len"]).make_batch()[:9]
    sr, hop = pp["preprocessing"]["audio"]["sampling_rate"], pp["preprocessing"]["stft"]["hop_length"]
    ts = torch.arange(int(5.0 * sr), dtype=torch.float64) / sr
    ph = 2 * math.pi * torch.cumsum(170 + 40 * torch.sin(2 * math.pi * 0.8 * ts), 0) / sr
    rec = (0.2 * sum(0.6 ** k * torch.sin((k + 1) * ph) for k in range(6)) * (torch.sin(2 * math.pi * 0.5 * ts) > -0.6)
           + 0.002 * torch.randn(ts.shape[0], dtype=torch.float64)).float().to(dev)
    stats = {"pitch": (180.0, 45.0), "energy": (20.0, 12.0)}
    feats = recording_features(rec, [rec.shape[0]], pp)
    mx = pp["preprocessing"]["audio"]["max_wav_value"]

    def plain():
        rows, lens, _ = model.infer_packed(*b[2:9])
        return voc.infer_packed(rows.to(torch.bfloat16), lens, int16_scale=mx).cpu()

    arms = (("plain packed synthesis", plain),
            ("synthesize_like (features)", lambda: synthesize_like(model, configs, b, vocoder=voc, features=feats,
                                                                          stats=stats)),
            ("synthesize_like (samples)", lambda: synthesize_like(model, configs, b, [rec], vocoder=voc,
                                                                           stats=stats)))
    t = {k: [] for k, _ in arms}
    for r in range(rounds + 1):
        for arm, fn in arms:
            ms = wall(fn)
            if r >= 1:
                t[arm].append(ms)
    out = synthesize_like(model, configs, b, vocoder=voc, features=feats, stats=stats)
    name = f"1 utterance, {int(b[4][0])} phonemes"
    lines += ["", f"{'workload':40s} {'arm':>28s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    for arm, v in t.items():
        lines.append(row(name, arm, v))
    lines.append(f"{'':40s} first pass {out['first_pass']['mel_lens'][0]} frames, recording {feats[3][0]} frames, second "
                 f"pass {out['mel_lens'][0]} frames")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def _median_spread(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def bench_features(out_path, rounds=9, iters=20, sr=22050, n_fft=1024, hop=256, n_mel=80):
    """``ops.frame_features`` (csrc/k_features.hip: one packed launch) on the 64-utterance workload of ``--yin``
    against (a) the per-utterance loop over ``hip.logmel`` (csrc/k_audio.hip) and (b) ``torch.stft`` + matmul per
    utterance on the same GPU.  Device events around ``iters`` calls, 3 warm-up calls before each window, the arms
    interleaved round by round in one process.  The outputs of the three arms are compared at the sizes timed."""
    from speakingstyle_amd import ops
    from speakingstyle_amd.audio.stft import TacotronSTFT
    from speakingstyle_amd.ops import reference as ref

    dev = torch.device("cuda")
    stft = TacotronSTFT(n_fft, hop, n_fft, n_mel, sr, 0.0, 8000.0)
    window, basis = stft.fft_window(dev), stft.mel_basis.to(dev).contiguous()
    name, wav_h, lens = yin_workloads(sr, hop)[0]
    wav = wav_h.to(dev)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    utts = [wav[a:b].unsqueeze(0) for a, b in zip(offs[:-1], offs[1:])]
    frames = [1 + n // hop for n in lens]
    R = sum(frames)

    def packed():
        return ops.frame_features(wav, lens, n_fft, hop, window, basis)

    def loop():
        return [hip.logmel(u, n_fft, hop, window, basis) for u in utts]

    def torch_arm():
        return ref.frame_features(wav, lens, n_fft, hop, window, basis)

    supp = hip._mel_support(basis)
    tab = ref.frame_pairs(lens, frames).to(dev)
    mel, energy = torch.empty(R, n_mel, device=dev), torch.empty(R, device=dev)
    log_clip = float(torch.log(torch.tensor([1e-5]))[0])

    def launch():
        hip._check(hip.lib().ssamd_frame_features(hip._ptr(wav), hip._ptr(tab), tab.shape[0], n_fft, hop, hip._ptr(window),
                                                  hip._ptr(basis), hip._ptr(supp), n_mel, 1e-5, log_clip, 0, hip._ptr(mel),
                                                  hip._ptr(energy), hip._stream()), "ssamd_frame_features")

    arms = (("packed ops.frame_features", packed), ("(a) loop over hip.logmel", loop),
            ("(b) torch.stft + matmul, same GPU", torch_arm), ("frame_features_kernel alone", launch))
    t = {a: [] for a, _ in arms}
    for r in range(rounds):
        for arm, fn in arms:
            t[arm].append(timeit(fn, iters))
    nz = int((basis != 0).sum())
    lines = [f"Packed log-mel / energy front-end, sr {sr} / n_fft {n_fft} / hop {hop} / {n_mel} mels, fp32, "
             f"{torch.cuda.get_device_name(0)}",
             f"workload: {name}: {len(lens)} utterances, {sum(lens)} samples, {R} frame rows "
             f"({sum((f + 1) // 2 for f in frames)} workgroups of two rows)",
             f"device events around {iters} calls after 3 warm-up calls; {rounds} rounds, the arms interleaved in one "
             "process; ms per call", "",
             f"{'arm':>36s} {'median':>10s} {'min':>10s} {'max':>10s}"]
    for arm, v in t.items():
        lines.append(f"{arm:>36s} {'%10.4f %10.4f %10.4f' % _median_spread(v)}")
    pm, plo, phi = _median_spread(t["packed ops.frame_features"])
    lm, llo, lhi = _median_spread(t["(a) loop over hip.logmel"])
    tm = _median_spread(t["(b) torch.stft + matmul, same GPU"])[0]
    lines += ["", f"(a) / packed: {lm / pm:.2f} at the medians; slowest packed round {phi:.4f} ms against the fastest loop "
                  f"round {llo:.4f} ms: the packed launch {'beats' if phi < llo else 'does NOT beat'} the loop by more than "
                  "the spread of the repeats",
              f"(b) / packed: {tm / pm:.2f} at the medians"]
    km = _median_spread(t["frame_features_kernel alone"])[0]
    flop = (R / 2) * (5.0 * n_fft * math.log2(n_fft)) + R * 2.0 * nz
    lines += [f"kernel alone: {flop / 1e9:.3f} GFLOP (5 n log2 n per complex transform of two rows + 2 per non-zero of "
              f"the basis, {nz} of {basis.numel()}) -> {flop / (km * 1e-3) / 1e12:.3f} TFLOP/s; it reads "
              f"{4.0 * sum(lens) / 1e6:.1f} MB of samples once from memory ({n_fft // hop} times through the caches) and "
              f"writes {4.0 * R * (n_mel + 1) / 1e6:.1f} MB -> {(4.0 * sum(lens) + 4.0 * R * (n_mel + 1)) / (km * 1e-3) / 1e9:.1f}"
              " GB/s: neither the vector rate nor the memory rate binds; the radix-2 stages go through LDS with a barrier "
              "each (not measured further: no counter run)"]
    a, b, c = packed(), loop(), torch_arm()
    mel_a = torch.cat([m[0].t() for m, _ in b])
    en_a = torch.cat([e[0] for _, e in b])
    lines += ["", f"outputs at the sizes timed: max |log-mel packed - loop| {float((a[0] - mel_a).abs().max()):.3e}, "
                  f"packed - torch {float((a[0] - c[0]).abs().max()):.3e}; max rel energy packed - loop "
                  f"{float(((a[1] - en_a).abs() / en_a.clamp(min=1e-30)).max()):.3e}, packed - torch "
                  f"{float(((a[1] - c[1]).abs() / c[1].clamp(min=1e-30)).max()):.3e}"]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def _v1_tail_packed(g, x, vp, out, int16_scale):
    """The part of HiFi-GAN V1's ``infer_packed`` that the iSTFT head stands in for: the stage 3 and 4 upsamplers and
    MRFs and conv_post, on the packed rows x [R * 64, 128] after stage 2 (the launches ``Generator.infer_packed``
    issues for i = 2, 3, copied from it)."""
    from speakingstyle_amd.models import hifigan as H

    nk, rate = g.num_kernels, 64
    for i in (2, 3):
        up = g.ups[i]
        s = up.stride[0]
        blocks = [g.resblocks[i * nk + j] for j in range(nk)]
        wu, wimg, bt = g._ups_image(i)
        cout = wu.shape[0] // s
        fused = all(b.fusable(cout, vp.R * rate * s) for b in blocks)
        x_act = None
        if fused and H._CONV3_SQ[0] and bt is not None and wu.shape[0] == wu.shape[1] in (64, 128):
            y = hip.conv3_sq_packed(x, vp, rate, wimg, bt)
        else:
            ks_ = (s // 2) * cout if (H._CONVT_KSPLIT[0] and up.kernel_size[0] == 2 * s
                                      and up.padding[0] * 2 == s) else 0
            if fused:
                y = hip.conv1d_infer_packed(x, vp, rate, wu, bt, 1, 1, None, wimg=wimg, ksplit=ks_)
            else:
                y, x_act = hip.conv1d_infer_packed(x, vp, rate, wu, bt, 1, 1, None, wimg=wimg, dual_lrelu=True,
                                                   ksplit=ks_)
        rate *= s
        y = y.view(vp.R * rate, cout)
        if x_act is not None:
            x_act = x_act.view(vp.R * rate, cout)
        xs = None
        for j, blk in enumerate(blocks):
            last = j == nk - 1
            xs = blk.forward_packed(y, vp, rate, acc=xs, out_scale=(1.0 / nk) if last else 1.0, x_act=x_act,
                                    post_lrelu=(i < 3) and last)
        x = xs
    return hip.conv_post_packed(x, vp, rate, g.conv_post.weight, g.conv_post.bias, out, 0.01, int16_scale)


def bench_istftnet(out_path, rounds=7, iters=10):
    """iSTFTNet (C8C8I) against HiFi-GAN V1, random init, throughput at equal output length (not quality).
    (1) The head kernel alone (csrc/k_istft.hip) on the last-stage rows of the 64-utterance LJSpeech-length batch,
    padded and packed form, against its byte floor and against the V1 launches it stands in for (stage 3 / 4
    upsamplers and ResBlocks + conv_post) on the same batch.  (2) ``Generator.infer_packed`` of both configs on the
    same mel batches (256 utterances of LJSpeech lengths; 1 utterance of 113 frames), eager, and batch 1 through
    the bucketed serving graphs.  Device events around ``iters`` calls after 3 warm-up calls, the arms alternating
    round by round in one process; the ratios are taken per interleaved pair."""
    import json as _json

    import numpy as np

    from speakingstyle_amd.data import synthetic
    from speakingstyle_amd.models import hifigan as H

    dev = torch.device("cuda")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    counts = synthetic.ljspeech_phone_counts(os.path.join(root, "preprocessed_data", "LJSpeech", "val.txt"))
    rng = np.random.default_rng(0)
    lens64 = np.clip(np.round(rng.choice(counts, size=64) * 8.1), 16, 1000).astype(np.int64).tolist()
    lens256 = np.clip(np.round(rng.choice(counts, size=256) * 8.1), 16, 1000).astype(np.int64).tolist()
    with open(os.path.join(root, "config", "hifigan", "config_istft.json")) as f:
        hi = H.AttrDict(_json.load(f))
    torch.manual_seed(0)
    g1 = H.Generator(H.default_config()).eval().fold_weight_norm().to(dev).requires_grad_(False)
    gi = H.Generator(hi).eval().fold_weight_norm().to(dev).requires_grad_(False)
    HBM = 6.29e12  # measured streaming rate (8.0 TB/s spec)
    lines = [f"iSTFTNet C8C8I vs HiFi-GAN V1, random init, bf16, {torch.cuda.get_device_name(0)}",
             "throughput at equal output length (256 samples per mel frame); random weights say nothing about quality",
             f"device events around {iters} calls after 3 warm-up calls; {rounds} rounds, the arms alternating in one "
             "process; ms per call", ""]

    def table(arms, title):
        t = {a: [] for a, _ in arms}
        for r in range(rounds):
            for arm, fn in arms:
                t[arm].append(timeit(fn, iters))
        lines.append(title)
        lines.append(f"{'arm':>52s} {'median':>10s} {'min':>10s} {'max':>10s}")
        for arm, v in t.items():
            lines.append(f"{arm:>52s} {'%10.4f %10.4f %10.4f' % _median_spread(v)}")
        return t

    def pairs(t, a, b, what):
        r = sorted(x / y for x, y in zip(t[a], t[b]))
        lines.append(f"{what}: {r[len(r) // 2]:.3f} at the median pair, {r[0]:.3f} .. {r[-1]:.3f} over the {len(r)} "
                     f"interleaved pairs ({'above 1 in every pair' if r[0] > 1 else 'NOT above 1 in every pair'})")
        return r

    # ---- (1) the head kernel alone
    C, rate = 128, 64
    bm = hip.voc_tile_rows("istft", C)
    R = sum(lens64)
    rows = R * rate
    torch.manual_seed(1)
    x = torch.randn(rows, C, device=dev).to(torch.bfloat16)
    w, b = gi.conv_post.weight, gi.conv_post.bias
    vp = hip.voc_pack_for(lens64, dev, gi._packed_geoms(lens64))
    vp1 = hip.voc_pack_for(lens64, dev, g1._packed_geoms(lens64))
    Tm = max(lens64) * rate
    xpad = torch.zeros(len(lens64), Tm, C, device=dev, dtype=torch.bfloat16)
    o = 0
    for u, n in enumerate(lens64):
        xpad[u, : n * rate] = x[o * rate:(o + n) * rate]
        o += n
    out = torch.zeros(len(lens64), max(lens64) * 256, device=dev, dtype=torch.int16)
    out1 = torch.zeros_like(out)
    arms = (("istft_head_kernel, packed (int16 out)", lambda: hip.istft_head_packed(x, vp, rate, w, b, out, 32768.0)),
            ("istft_head_kernel, padded (int16 out)", lambda: hip.istft_head(xpad, w, b, 32768.0)),
            ("V1 stage 3 + 4 + conv_post, packed (int16 out)", lambda: _v1_tail_packed(g1, x, vp1, out1, 32768.0)))
    t = table(arms, f"(1) head alone: 64 utterances, LJSpeech val lengths, {R} frames = {rows} last-stage rows x {C} "
                    f"channels; tile {bm} rows, {sum(-(-n * rate // bm) for n in lens64)} workgroups packed, "
                    f"{len(lens64) * -(-Tm // bm)} padded ({len(lens64) * Tm} padded rows)")
    km = _median_spread(t["istft_head_kernel, packed (int16 out)"])[0]
    kp = _median_spread(t["istft_head_kernel, padded (int16 out)"])[0]
    byts = rows * C * 2 + 4 * rows * 2
    floor_ms = byts / HBM * 1e3
    flop = 2.0 * rows * (7 * C) * 18
    lines += [f"byte floor: {rows} x {C} x 2 B read + 4 x {rows} x 2 B written = {byts / 1e6:.1f} MB at {HBM / 1e12:.2f} "
              f"TB/s (measured streaming rate; 8.0 TB/s spec) = {floor_ms:.4f} ms; packed kernel {km:.4f} ms = "
              f"{km / floor_ms:.2f} x the floor ({byts / (km * 1e-3) / 1e12:.2f} TB/s); padded {kp:.4f} ms for "
              f"{len(lens64) * Tm * C * 2 / 1e6:.1f} MB of padded rows",
              f"conv work: {flop / 1e9:.2f} GFLOP useful (N = 18), {flop * 32 / 18 * 2 / 1e9:.2f} GFLOP issued (N padded "
              f"to 32, two sign halves) -> {flop * 32 / 18 * 2 / (km * 1e-3) / 1e12:.1f} TFLOP/s issued"]
    pairs(t, "V1 stage 3 + 4 + conv_post, packed (int16 out)", "istft_head_kernel, packed (int16 out)",
          "V1 stage 3 + 4 + conv_post / istft head (packed)")
    lines += ["compile figures (gfx950) of istft_head_kernel<128, 16, 4>:"] + \
             ["    " + s for s in _kernel_resources("k_istft.hip", "istft_head_kernelILi128E")] + [""]

    # ---- (2) the generators, eager
    torch.manual_seed(2)
    mel256 = torch.randn(sum(lens256), 80, device=dev).to(torch.bfloat16)
    mel1 = torch.randn(113, 80, device=dev).to(torch.bfloat16)
    speed = {}
    for name, mel, lens in (("batch 256, LJSpeech val lengths", mel256, lens256), ("batch 1, 113 frames", mel1, [113])):
        arms = (("HiFi-GAN V1 infer_packed", lambda: g1.infer_packed(mel, lens, 32768.0)),
                ("iSTFTNet C8C8I infer_packed", lambda: gi.infer_packed(mel, lens, 32768.0)))
        t = table(arms, f"(2) Generator.infer_packed, eager, {name} ({sum(lens)} frames, {sum(lens) * 256 / 22050:.1f} s "
                        "of audio)")
        speed[name] = pairs(t, "HiFi-GAN V1 infer_packed", "iSTFTNet C8C8I infer_packed", "V1 / C8C8I")
        mi = _median_spread(t["iSTFTNet C8C8I infer_packed"])[0]
        m1 = _median_spread(t["HiFi-GAN V1 infer_packed"])[0]
        lines += [f"RTF (vocoder only): V1 {m1 * 1e-3 / (sum(lens) * 256 / 22050):.3e}, C8C8I "
                  f"{mi * 1e-3 / (sum(lens) * 256 / 22050):.3e}", ""]

    # ---- (2b) batch 1 through the bucketed serving graphs (FastSpeech2 BC2013_GST + vocoder: the whole synthesis)
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.infer.graphs import SynthGraphs
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2

    pp, mc, tc = load_named("BC2013_GST")
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc).to(dev)
    with torch.no_grad():  # a duration head that speaks: ~8.1 frames per phoneme, 14 phonemes -> ~113 frames
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(9.1))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    ref = SyntheticBatches(1, device=dev, seed=12, max_seq_len=mc["max_seq_len"],
                           phone_counts=np.array([14])).make_batch()
    ids = torch.from_numpy(np.random.default_rng(5).integers(1, 300, size=(1, 14)).astype(np.int64)).to(dev)
    a = (ref[2][:1].contiguous(), ids, torch.tensor([14], device=dev), 14, ref[6][:1].contiguous(),
         ref[7][:1].contiguous(), ref[8])
    sgs = {"HiFi-GAN V1, graphs": SynthGraphs(model, g1, int16_scale=32768.0, warm=1, bucketed=True),
           "iSTFTNet C8C8I, graphs": SynthGraphs(model, gi, int16_scale=32768.0, warm=1, bucketed=True)}
    frames = {}
    for k, sg in sgs.items():
        for _ in range(4):  # warm, capture graph 1, capture graph 2, replay
            frames[k] = sg(*a)[1]
    arms = tuple((k, (lambda sg=sg: sg(*a))) for k, sg in sgs.items())
    t = table(arms, f"(2b) text -> int16 wav through the bucketed graphs, batch 1, {sorted(set(sum(frames.values(), [])))} frames (FastSpeech2 "
                    "BC2013_GST + vocoder, replays only)")
    speed["graphs b1"] = pairs(t, "HiFi-GAN V1, graphs", "iSTFTNet C8C8I, graphs", "V1 / C8C8I (whole synthesis)")
    lines += [f"graph statistics: {dict((k, dict(sg.stats)) for k, sg in sgs.items())}", ""]
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def write_feature_corpus(root, n_utts=256, sr=22050, seed=0):
    """A synthetic raw corpus for the end-to-end preprocessing figure: ``n_utts`` int16 wavs with the LJSpeech
    ``val.txt`` length distribution (the signal of ``yin_workloads``) and a transcript each -> the config
    (``source: learned``, ``pyin``) without its preprocessed_path."""
    import numpy as np

    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.config import config_dir_triplet, load_yaml, normalize_preprocess_config
    from speakingstyle_amd.data import synthetic

    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    counts = synthetic.ljspeech_phone_counts(os.path.join(here, "preprocessed_data", "LJSpeech", "val.txt"))
    rng = np.random.default_rng(seed)
    frames = np.clip(np.round(rng.choice(counts, size=n_utts) * 8.1), 100, 1000).astype(np.int64)
    raw = os.path.join(root, "raw", "LJSpeech")
    os.makedirs(raw, exist_ok=True)
    for i, T in enumerate(frames):
        n = 256 * (int(T) - 1)
        t = np.arange(n) / sr
        f0 = 170 + 80 * np.sin(2 * np.pi * 1.1 * t + rng.uniform(0, 6.28))
        ph = 2 * np.pi * np.cumsum(f0) / sr
        s = sum(0.6 ** k * np.sin((k + 1) * ph + rng.uniform(0, 6.28)) for k in range(6))
        voiced = np.sin(2 * np.pi * 0.8 * t + rng.uniform(0, 6.28)) > -0.4
        x = np.where(voiced, 0.3 * (0.55 + 0.45 * np.sin(2 * np.pi * 3 * t)) * s, 0.0) + 0.01 * rng.standard_normal(n)
        write_wav(os.path.join(raw, f"S{i:04d}.wav"), sr, (0.5 * x / np.abs(x).max() * 32767).astype(np.int16))
        with open(os.path.join(raw, f"S{i:04d}.lab"), "w") as f:
            f.write("printing in the only sense with which we are at present concerned")
    p = load_yaml(config_dir_triplet("LJSpeech_unaligned")[0])
    p["path"]["raw_path"] = os.path.join(root, "raw")
    p["preprocessing"]["val_size"] = 16
    p["preprocessing"]["pitch"]["extractor"] = "pyin"
    return normalize_preprocess_config(p), int(frames.sum())


def preprocess_host_arm(cfg_path):
    """The per-utterance host path of ``bench_preprocess`` in a process that never opens the GPU -> one JSON line."""
    import time

    from speakingstyle_amd.data.preprocess import Preprocessor

    with open(cfg_path) as f:
        job = json.load(f)
    t0 = time.perf_counter()
    out = Preprocessor(job["config"]).build_from_path(workers=job["workers"])
    print(json.dumps({"seconds": time.perf_counter() - t0, "utterances": len(out)}))


def bench_preprocess(out_path, n_utts=256, workers=16):
    """End to end: ``Preprocessor.build_from_path`` on a synthetic corpus, the per-utterance host path with
    ``workers`` pool workers against ``device="cuda"`` (``workers`` loaders), wall clock, the two alternating."""
    import copy
    import subprocess
    import tempfile
    import time

    from speakingstyle_amd.data.preprocess import Preprocessor

    lines = []
    with tempfile.TemporaryDirectory() as root:
        config, total = write_feature_corpus(root, n_utts)
        runs = {"host": [], "cuda": []}
        split = []
        for r in range(2):
            for arm in ("cuda", "host")[:2 - r]:  # the host path takes minutes: one run of it
                cfg = copy.deepcopy(config)
                cfg["path"]["preprocessed_path"] = os.path.join(root, f"pre_{arm}_{r}")
                if arm == "host":  # its forked workers must not inherit this process's open GPU: a process of its own
                    cfg_path = os.path.join(root, f"host_{r}.json")
                    with open(cfg_path, "w") as f:
                        json.dump({"config": cfg, "workers": workers}, f)
                    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--preprocess-host-arm", cfg_path],
                                         check=True, stdout=subprocess.PIPE, text=True)
                    got = json.loads(res.stdout.strip().split("\n")[-1])
                    runs[arm].append(got["seconds"])
                    assert got["utterances"] == n_utts, got
                    continue
                pre = Preprocessor(cfg, device="cuda")
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = pre.build_from_path(workers=workers)
                torch.cuda.synchronize()
                runs[arm].append(time.perf_counter() - t0)
                assert len(out) == n_utts, (arm, len(out))
                split.append(dict(pre.timings))
    sec = total * 256 / 22050
    lines += [f"Preprocessor.build_from_path end to end, {torch.cuda.get_device_name(0)}: {n_utts} synthetic utterances "
              f"({total} frames, {sec / 60:.1f} min of audio at 22050 Hz, LJSpeech val.txt lengths), source: learned, "
              f"extractor: pyin, {workers} pool workers in either arm; wall clock of the whole call, three "
              "runs (cuda, host, cuda; the first cuda run also loads the kernel library; every run starts its pool)", "",
              f"{'arm':>28s} {'run 1 (s)':>10s} {'run 2 (s)':>10s}"]
    lines.append(f"{'per-utterance host path':>28s} {runs['host'][0]:10.2f} {'-':>10s}")
    lines.append(f"{'device=cuda':>28s} {runs['cuda'][0]:10.2f} {runs['cuda'][1]:10.2f}")
    lines += ["", f"host / cuda: {runs['host'][0] / runs['cuda'][0]:.2f} against the first cuda run, "
                  f"{runs['host'][0] / runs['cuda'][1]:.2f} against the second",
              "", "main-process split of the cuda runs (s): load = waiting for the loader pool (process start, wav "
              "decoding, text frontend), kernels = H2D + pyin + frame_features + interp_unvoiced + the D2H that ends the "
              "batch, write = per-utterance rules, statistics and .npy files"]
    for r, s in enumerate(split, 1):
        lines.append(f"  run {r}: load {s['load']:.2f}  kernels {s['kernels']:.2f}  write {s['write']:.2f}")
    bound = max(split[-1], key=split[-1].get)
    lines.append(f"the second cuda run is bound by: {bound}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=160000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-attn", action="store_true")
    ap.add_argument("--griffin-lim", action="store_true",
                    help="only the Griffin-Lim arm: HIP kernels vs the torch loop, table written to --out")
    ap.add_argument("--dtw", action="store_true",
                    help="only the DTW arm: HIP kernels vs the torch wavefront, table written to --out")
    ap.add_argument("--align", action="store_true",
                    help="only the alignment arm: forward-sum / MAS kernels vs the torch loop and F.ctc_loss")
    ap.add_argument("--yin", action="store_true",
                    help="only the pitch arm: the YIN kernel vs the torch reference on the GPU and numpy on the host "
                         "(yin_numerics.txt is written beside --out)")
    ap.add_argument("--pyin", action="store_true",
                    help="only the probabilistic-YIN arm: ops.pyin vs the torch reference on the GPU and on the host, "
                         "kernel-only times, wave_metrics with either tracker (pyin_numerics.txt is written beside --out)")
    ap.add_argument("--k256", action="store_true",
                    help="only the K = 256 Linear GEMMs: tile kernels vs the weight-stationary streaming kernel")
    ap.add_argument("--prosody", action="store_true",
                    help="only the prosody-transfer arm: the kernel vs the torch reference on the GPU, and "
                         "synthesize_like vs plain synthesis for one utterance")
    ap.add_argument("--tsne", action="store_true",
                    help="only the style-map arm: t-SNE affinities, gradient, 750 iterations and k-means at N = 1024, "
                         "4096, 13100 (D = 512), kernels vs the torch reference on the GPU, scikit-learn on the host "
                         "(profiles/style_map.txt)")
    ap.add_argument("--features", action="store_true",
                    help="only the feature front-end: the packed ops.frame_features launch vs the per-utterance loop over "
                         "hip.logmel and torch.stft + matmul (profiles/features.txt), then Preprocessor end to end, host "
                         "path vs device=\"cuda\" (profiles/preprocess_gpu.txt beside --out)")
    ap.add_argument("--istftnet", action="store_true",
                    help="iSTFTNet: the head kernel alone against its byte floor and the HiFi-GAN V1 launches it stands "
                         "in for, then Generator.infer_packed V1 vs C8C8I, eager and through the bucketed graphs "
                         "(profiles/istftnet.txt)")
    ap.add_argument("--preprocess-host-arm", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None,
                    help="default: profiles/griffin_lim.txt, profiles/dtw.txt, profiles/align.txt, profiles/yin.txt, "
                         "profiles/pyin.txt, profiles/k256_shapes.txt, profiles/prosody_transfer.txt")
    args = ap.parse_args()
    prof = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")
    if args.preprocess_host_arm:
        return preprocess_host_arm(args.preprocess_host_arm)
    if args.istftnet:
        return bench_istftnet(args.out or os.path.join(prof, "istftnet.txt"))
    if args.features:
        out = args.out or os.path.join(prof, "features.txt")
        bench_features(out)
        return bench_preprocess(os.path.join(os.path.dirname(os.path.abspath(out)), "preprocess_gpu.txt"))
    if args.prosody:
        return bench_prosody(args.out or os.path.join(prof, "prosody_transfer.txt"))
    if args.tsne:
        return bench_tsne(args.out or os.path.join(prof, "style_map.txt"))
    if args.k256:
        return bench_k256(args.out or os.path.join(prof, "k256_shapes.txt"), iters=args.iters)
    if args.pyin:
        return bench_pyin(args.out or os.path.join(prof, "pyin.txt"))
    if args.yin:
        return bench_yin(args.out or os.path.join(prof, "yin.txt"))
    if args.align:
        return bench_align(args.out or os.path.join(prof, "align.txt"))
    if args.dtw:
        return bench_dtw(args.out or os.path.join(prof, "dtw.txt"))
    args.out = args.out or os.path.join(prof, "griffin_lim.txt")
    if args.griffin_lim:
        return bench_griffin_lim(args.out)
    dev = "cuda"
    B = 200
    L = args.rows // B
    R = B * L
    res = []
    shapes = [  # name, Cin, N, ks
        ("ffn.w1 (k9 256->1024)", 256, 1024, 9),
        ("ffn.w2 (k1 1024->256)", 1024, 256, 1),
        ("ffn.w1 dgrad (k9 1024->256)", 1024, 256, 9),
        ("ffn.w2 dgrad (k1 256->1024)", 256, 1024, 1),
        ("qkv (256->768)", 256, 768, 1),
        ("attn fc (256->256)", 256, 256, 1),
        ("postnet (k5 512->512)", 512, 512, 5),
        ("postnet in (k5 80->512)", 80, 512, 5),
    ]
    for name, Cin, N, ks in ([] if args.only_attn else shapes):
        x = torch.randn(B, L, Cin, device=dev).to(torch.bfloat16)
        w = torch.randn(N, ks, Cin, device=dev).to(torch.bfloat16)
        bias = torch.randn(N, device=dev)
        pad = (ks - 1) // 2
        flops = 2.0 * R * N * ks * Cin
        hip.lib().ssamd_gemm_set_variant(0)
        t_lds = timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), args.iters)
        hip.lib().ssamd_gemm_set_variant(2)
        t_ring = timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), args.iters)
        hip.lib().ssamd_gemm_set_variant(3)
        t_big = timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), args.iters)
        hip.lib().ssamd_gemm_set_variant(4)
        t_b64 = timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), args.iters)
        hip.lib().ssamd_gemm_set_variant(5)
        t_pers = timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), args.iters)
        hip.lib().ssamd_gemm_set_variant(-1)
        t = timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), args.iters)
        t_lds = min(t_lds, timeit(lambda: hip.conv_gemm_raw(x, w, bias, B, L, Cin, ks, 1, pad, N, 1), 1) * 0 + t_lds)
        dy = torch.randn(B, L, N, device=dev).to(torch.bfloat16)
        tw = timeit(lambda: hip.conv_wgrad_raw(x, dy, B, L, Cin, ks, 1, pad, N, with_bias=True), args.iters)
        hip.lib().ssamd_wgrad_set_variant(0)
        tw_old = timeit(lambda: hip.conv_wgrad_raw(x, dy, B, L, Cin, ks, 1, pad, N, with_bias=True), args.iters)
        hip.lib().ssamd_wgrad_set_variant(1)
        tw_r = timeit(lambda: hip.conv_wgrad_raw(x, dy, B, L, Cin, ks, 1, pad, N, with_bias=True), args.iters)
        hip.lib().ssamd_wgrad_set_variant(2)
        tw_32 = timeit(lambda: hip.conv_wgrad_raw(x, dy, B, L, Cin, ks, 1, pad, N, with_bias=True), args.iters)
        hip.lib().ssamd_wgrad_set_variant(-1)
        hip.lib().ssamd_wgrad_set_blocks(256)
        tw_256 = timeit(lambda: hip.conv_wgrad_raw(x, dy, B, L, Cin, ks, 1, pad, N, with_bias=True), args.iters)
        hip.lib().ssamd_wgrad_set_blocks(0)
        row = {"op": name, "fwd_ms": round(t, 3), "fwd_TF": round(flops / t / 1e9, 1),
               "fwd_regstage_TF": round(flops / t_lds / 1e9, 1), "fwd_ring256_TF": round(flops / t_ring / 1e9, 1),
               "fwd_big256x256_TF": round(flops / t_big / 1e9, 1),
               "fwd_big_bk64_TF": round(flops / t_b64 / 1e9, 1),
               "fwd_persistent_TF": round(flops / t_pers / 1e9, 1), "wgrad_ms": round(tw, 3),
               "wgrad_TF": round(flops / tw / 1e9, 1), "wgrad_128x128_TF": round(flops / tw_old / 1e9, 1),
               "wgrad_256x128_TF": round(flops / tw_r / 1e9, 1), "wgrad_bk32_TF": round(flops / tw_32 / 1e9, 1),
               "wgrad_256blocks_TF": round(flops / tw_256 / 1e9, 1)}
        if ks > 1:  # packed-sequence geometry (rinfo table), same data
            from speakingstyle_amd.ops.packing import PackInfo

            ri = PackInfo.build(torch.full((B,), L, device=dev), L, R).rinfo
            tpf = timeit(lambda: hip.conv_gemm_raw(x, w, bias, 1, R, Cin, ks, 1, pad, N, 1, rinfo=ri), args.iters)
            tpw = timeit(lambda: hip.conv_wgrad_raw(x, dy, 1, R, Cin, ks, 1, pad, N, with_bias=True, rinfo=ri),
                         args.iters)
            row["fwd_packed_TF"] = round(flops / tpf / 1e9, 1)
            row["wgrad_packed_TF"] = round(flops / tpw / 1e9, 1)
        if ks == 1:
            a2 = x.view(R, Cin)
            w2 = w.view(N, Cin)
            tb = timeit(lambda: torch.matmul(a2, w2.t()), args.iters)
            row["hipblaslt_ms"] = round(tb, 3)
            row["hipblaslt_TF"] = round(flops / tb / 1e9, 1)
        res.append(row)
        print(json.dumps(row), flush=True)
    # attention
    for H, D in ((2, 128), (8, 32)):
        Lq = 800
        qkv = torch.randn(B, Lq, 3 * H * D, device=dev).to(torch.bfloat16)
        lens = torch.randint(Lq // 2, Lq + 1, (B,), device=dev)
        lens[0] = Lq
        fl = 4.0 * B * H * Lq * Lq * D * (lens.float().mean().item() / Lq)
        qh = qkv.clone().requires_grad_(True)
        tf = timeit(lambda: hip.attention(qh, lens, H), args.iters)
        o = hip.attention(qh, lens, H)
        g = torch.randn_like(o)
        tb = timeit(lambda: torch.autograd.grad(o, qh, g, retain_graph=True), args.iters)
        row = {"op": f"attention H{H} D{D} L{Lq}", "fwd_ms": round(tf, 3), "fwd_TF": round(fl / tf / 1e9, 1),
               "bwd_ms": round(tb, 3), "bwd_TF": round(2.5 * fl / tb / 1e9, 1)}
        if D == 128:  # forward variants: register-staged (NF=1) / LDS-DMA NF=1 / NF=2
            for dma, nf in ((0, 1), (1, 1), (1, 2)):
                hip.lib().ssamd_attn_set_fwd(dma, nf)
                row[f"fwd_ms_dma{dma}_nf{nf}"] = round(timeit(lambda: hip.attention(qh, lens, H), args.iters), 3)
            hip.lib().ssamd_attn_set_fwd(1, 2)
        if D == 128:  # dK/dV kernel (register-staged / LDS-DMA) x fragments per wave; dQ NF = 1
            for dma, nkv in ((0, 2), (1, 1), (1, 2)):
                hip.lib().ssamd_attn_set_kv_dma(dma)
                hip.lib().ssamd_attn_set_nf(nkv, 1)
                t2 = timeit(lambda: torch.autograd.grad(o, qh, g, retain_graph=True), args.iters)
                row[f"bwd_ms_kvdma{dma}_nf{nkv}"] = round(t2, 3)
            hip.lib().ssamd_attn_set_kv_dma(1)
            hip.lib().ssamd_attn_set_nf(1, 2)
            for qd, nq in ((0, 1), (1, 1), (1, 2)):  # dQ kernel variants
                hip.lib().ssamd_attn_set_q_dma(qd, nq)
                t2 = timeit(lambda: torch.autograd.grad(o, qh, g, retain_graph=True), args.iters)
                row[f"bwd_ms_qdma{qd}_nf{nq}"] = round(t2, 3)
            hip.lib().ssamd_attn_set_q_dma(1, 2)
            for xcd in (0, 1):  # plain block order / all blocks of a sequence on one XCD
                hip.lib().ssamd_attn_set_xcd(xcd)
                row[f"fwd_ms_xcd{xcd}"] = round(timeit(lambda: hip.attention(qh, lens, H), args.iters), 3)
                t2 = timeit(lambda: torch.autograd.grad(o, qh, g, retain_graph=True), args.iters)
                row[f"bwd_ms_xcd{xcd}"] = round(t2, 3)
            hip.lib().ssamd_attn_set_xcd(1)
        if D == 32:  # query / key fragments per wave of the D = 32 kernels
            for nf in (1, 2, 4):
                hip.lib().ssamd_attn_set_nf32(nf, nf)
                row[f"fwd_ms_nf{nf}"] = round(timeit(lambda: hip.attention(qh, lens, H), args.iters), 3)
                o2 = hip.attention(qh, lens, H)
                row[f"bwd_ms_nf{nf}"] = round(timeit(lambda: torch.autograd.grad(o2, qh, g, retain_graph=True),
                                                     args.iters), 3)
            hip.lib().ssamd_attn_set_nf32(2, 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
