"""Bucketed synthesis graphs (``SynthGraphs(bucketed=True)``, ``hip.VocPackCap``, ``ssamd_voc_cap_tables``): one
captured graph per capacity bucket serves utterances it has never seen -- bit for bit the eager bucketed run, and
(one GEMM kernel family pinned) each utterance's synthesis alone; plus the two lifetime fixes of the exact-key mode
and the serving entry / CLI."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HOP = 256


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


# ------------------------------------------------------------------------------------------------ table kernel
CASES = [[37], [64], [1], [5, 9, 1], [63]]  # the CPU cases ([63]: F = 1)
RATE_TILES = [(rate, bm) for rate in (1, 8, 256) for bm in (64, 128, 256)]


@pytest.mark.parametrize("lens", CASES)
def test_cap_tables_kernel_equals_host_reference(lens):
    from speakingstyle_amd.ops import hip

    dev = torch.device("cuda", 0)
    rcap, mcap = hip.cap_bucket(lens)
    pack = hip.VocPackCap(len(lens), rcap, mcap, dev, RATE_TILES)
    Tb = 16
    mel_len = torch.tensor(lens + [123], device=dev, dtype=torch.int64)  # the filler's own prediction: overwritten
    dur = torch.full((len(lens) + 1, Tb), 7, device=dev, dtype=torch.int64)
    pack.buf.fill_(-1)  # every word of every table must be written
    pack.update(mel_len, dur)
    h_lens, h_cu, h_tabs = hip.cap_tables_host(lens, rcap, pack.geoms, mcap)
    F = rcap - sum(lens)
    assert mel_len.tolist() == h_lens.tolist() == lens + [F]
    assert dur[-1].tolist() == [F] + [0] * (Tb - 1) and bool((dur[:-1] == 7).all())  # the filler rewrite only
    assert pack.cu.tolist() == h_cu.tolist()
    for rate, bm, n_cap, _ in pack.geoms:
        tt, n = pack.tiles(rate, bm)
        assert n == n_cap and np.array_equal(tt.cpu().numpy().reshape(n, 4), h_tabs[(rate, bm)]), (rate, bm)
    # rinfo is rebuilt from cu on every update (here: another length set in the same capacity)
    r1 = pack.rinfo(8).clone()
    assert r1[:, 1].tolist() == sum(([8 * n] * (8 * n) for n in lens + [F]), [])
    if lens[0] > 1:
        mel_len2 = torch.tensor([lens[0] - 1] + lens[1:] + [0], device=dev, dtype=torch.int64)
        pack.update(mel_len2, dur)
        want = hip.cap_tables_host([lens[0] - 1] + lens[1:], rcap, pack.geoms, mcap)[0].tolist()
        assert mel_len2.tolist() == want and want[-1] == min(F + 1, mcap)  # (the filler too is clamped to Mcap)
        r2 = pack.rinfo(8)[: 8 * sum(want)]
        assert r2[:, 1].tolist() == sum(([8 * n] * (8 * n) for n in want), [])


def test_cap_tables_kernel_clamps_a_wrong_bucket():
    """Lengths that do not fit the capacity: cu and the tiles stay inside Rcap rows / Mcap frames."""
    from speakingstyle_amd.ops import hip

    dev = torch.device("cuda", 0)
    pack = hip.VocPackCap(3, 64, 32, dev, [(1, 64), (256, 128)])
    for lens in ([100, 50, 7], [-5, 70, 0], [63, 63, 63]):
        mel_len = torch.tensor(lens + [0], device=dev, dtype=torch.int64)
        dur = torch.zeros(4, 16, device=dev, dtype=torch.int64)
        pack.update(mel_len, dur)
        h_lens, h_cu, h_tabs = hip.cap_tables_host(lens, 64, pack.geoms, 32)
        assert mel_len.tolist() == h_lens.tolist() and pack.cu.tolist() == h_cu.tolist() and h_cu[-1] <= 64
        for rate, bm, n_cap, _ in pack.geoms:
            tt, n = pack.tiles(rate, bm)
            assert np.array_equal(tt.cpu().numpy().reshape(n, 4), h_tabs[(rate, bm)])


# ------------------------------------------------------------------------------------------------ null tiles
class _WithNullTiles:
    """A VocPack whose tile tables carry ``extra`` null tiles {0, 0, 0, 0} at the end."""

    def __init__(self, vp, extra=3):
        self.vp, self.extra = vp, extra
        self.lens, self.R, self.B, self.cu = vp.lens, vp.R, vp.B, vp.cu

    def tiles(self, rate, bm):
        tt, n = self.vp.tiles(rate, bm)
        return torch.cat([tt, torch.zeros(4 * self.extra, device=tt.device, dtype=tt.dtype)]), n + self.extra

    def rinfo(self, rate):
        return self.vp.rinfo(rate)


RATE = 8
SEQ = [37, 1]  # rows = [37 * rate, 1 * rate]: several tiles and a partial one, then a sequence shorter than any tile
GUARD = 64
SENTINEL = -7.0


def _convs(C, K, n, dev):
    torch.manual_seed(C + K)
    cs = [torch.nn.Conv1d(C, C, K).to(dev).requires_grad_(False) for _ in range(n)]
    for c in cs:
        c.weight.mul_(0.5)
    return cs


def _null_tile_check(run, C, dev, rate_tiles):
    """``run(vp, out)`` writes its packed result into ``out`` ([R*rate, C], first holding the accumulator input):
    once on the exact tables, once with 3 null tiles appended -- bitwise equal, guard rows untouched."""
    from speakingstyle_amd.ops import hip

    vp = hip.VocPack(SEQ, dev, rate_tiles)
    rows = vp.R * RATE
    torch.manual_seed(1)
    acc0 = torch.randn(rows, C, device=dev).to(torch.bfloat16)
    bufs = []
    for pk in (vp, _WithNullTiles(vp)):
        big = torch.full((rows + 2 * GUARD, C), SENTINEL, device=dev, dtype=torch.bfloat16)
        out = big[GUARD: GUARD + rows]
        out.copy_(acc0)
        run(pk, out)
        bufs.append(big)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])
    for big in bufs:
        assert bool((big[:GUARD] == SENTINEL).all()) and bool((big[GUARD + rows:] == SENTINEL).all())
    assert not torch.equal(bufs[0][GUARD: GUARD + rows], acc0)  # the kernel did run


@pytest.mark.parametrize("mode,C,K", [
    # the tall tile exists from K = 7 (C = 64 / 128) and K = 11 (C = 32): the smallest K that has it
    ("tall", 32, 11), ("tall", 64, 7), ("tall", 128, 7),
    ("r128", 32, 3), ("r128", 64, 3), ("r128", 128, 3),
    ("r64", 32, 3), ("r64", 64, 3), ("r64", 128, 3)])
def test_null_tiles_resblock_layer(mode, C, K):
    from speakingstyle_amd.ops import hip

    dev = torch.device("cuda", 0)
    saved = hip._TALL_MIN_TILES[0], hip._SMALL_MAX_TILES[0]
    # tile choice forced through its thresholds (tall: from 0 tiles; 128-row: tall never, 64-row never; 64-row: always)
    hip._TALL_MIN_TILES[0], hip._SMALL_MAX_TILES[0] = {"tall": (0, 0), "r128": (1 << 30, 0), "r64": (1 << 30, 1 << 30)}[mode]
    try:
        want, bm = hip.rb_layer_tile(C, K, SEQ, RATE)
        assert want == {"tall": 1, "r128": 0, "r64": -1}[mode] and bm > 0
        c1, c2 = _convs(C, K, 2, dev)
        torch.manual_seed(2)
        x = torch.randn((37 + 1) * RATE, C, device=dev).to(torch.bfloat16)

        def run(vp, out):
            hip.resblock_layer_packed(x, vp, RATE, c1, c2, 3, 0.1, acc=out, out_scale=0.5, post_lrelu=True)

        _null_tile_check(run, C, dev, [(RATE, bm)])
    finally:
        hip._TALL_MIN_TILES[0], hip._SMALL_MAX_TILES[0] = saved


@pytest.mark.parametrize("short", [False, True])
@pytest.mark.parametrize("C", [32, 64, 128])
def test_null_tiles_resblock_fused(C, short):
    from speakingstyle_amd.ops import hip

    dev = torch.device("cuda", 0)
    K, dil = 3, (1, 3, 5)
    assert hip.resblock_fusable(C, K)
    saved = hip._RF_SHORT_MAX_TILES[0]
    hip._RF_SHORT_MAX_TILES[0] = (1 << 30) if short else 0
    try:
        got, bm = hip.rf_tile(C, K, dil, SEQ, RATE)
        assert got == short and bm > 0
        cs = _convs(C, K, 6, dev)
        torch.manual_seed(2)
        x = torch.randn((37 + 1) * RATE, C, device=dev).to(torch.bfloat16)

        def run(vp, out):
            hip.resblock_fused_packed(x, vp, RATE, cs[0::2], cs[1::2], dil, 0.1, acc=out, out_scale=0.5,
                                      post_lrelu=True)

        _null_tile_check(run, C, dev, [(RATE, bm)])
    finally:
        hip._RF_SHORT_MAX_TILES[0] = saved


@pytest.mark.parametrize("C", [64, 128])
def test_null_tiles_conv3_sq(C):
    from speakingstyle_amd.ops import hip

    dev = torch.device("cuda", 0)
    torch.manual_seed(3)
    wimg = (torch.randn(C, 3, C, device=dev) * 0.05).to(torch.bfloat16)
    bias = torch.randn(C, device=dev)
    x = torch.randn((37 + 1) * RATE, C, device=dev).to(torch.bfloat16)

    def run(vp, out):
        hip.conv3_sq_packed(x, vp, RATE, wimg, bias, out=out)

    _null_tile_check(run, C, dev, [(RATE, hip.voc_tile_rows(2, C))])


def test_null_tiles_conv_post():
    from speakingstyle_amd.ops import hip

    dev = torch.device("cuda", 0)
    C = 32
    torch.manual_seed(4)
    w = torch.randn(1, C, 7, device=dev) * 0.05
    b = torch.randn(1, device=dev)
    x = torch.randn((37 + 1) * RATE, C, device=dev).to(torch.bfloat16)
    vp = hip.VocPack(SEQ, dev, [(RATE, hip.voc_tile_rows("post", C))])
    W = 37 * RATE
    bufs = []
    for pk in (vp, _WithNullTiles(vp)):
        big = torch.full((2 + 2, W), 12345, device=dev, dtype=torch.int16)  # a guard row before and after
        hip.conv_post_packed(x, pk, RATE, w, b, big[1:3], 0.01, 32768.0)
        bufs.append(big)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])
    for big in bufs:
        assert bool((big[0] == 12345).all()) and bool((big[3] == 12345).all())
        assert bool((big[2, 1 * RATE:] == 12345).all()) and not bool((big[1] == 12345).all())


# ------------------------------------------------------------------------------------------------ synthesis
@pytest.fixture(scope="module")
def tts():
    """BC2013_GST model (the bench's duration head: ~8 frames per phoneme), HiFi-GAN V1, one reference mel."""
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.models.hifigan import Generator, default_config

    dev = torch.device("cuda", 0)
    pp, mc, tc = load_named("BC2013_GST")
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc).to(dev)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(9.1))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    torch.manual_seed(1)
    g = Generator(default_config()).eval().fold_weight_norm().to(dev)
    ref = SyntheticBatches(1, device=dev, seed=12, max_seq_len=mc["max_seq_len"],
                           phone_counts=np.array([14])).make_batch()
    rng = np.random.default_rng(5)

    def utt(T, B=1):
        """B texts of T random phonemes (a list: one count per row, padded by the caller's convention)."""
        Ts = [T] * B if isinstance(T, int) else list(T)
        B, Tm = len(Ts), max(Ts)
        ids = np.zeros((B, Tm), dtype=np.int64)
        for i, n in enumerate(Ts):
            ids[i, :n] = rng.integers(1, 300, size=n)
        return (ref[2][:1].expand(B).contiguous(), torch.from_numpy(ids).to(dev), torch.tensor(Ts, device=dev), Tm,
                ref[6][:1].expand(B, -1, -1).contiguous(), ref[7][:1].expand(B).contiguous(), ref[8])

    return model, g, utt


def _graphs(tts, **kw):
    from speakingstyle_amd.infer.graphs import SynthGraphs

    return SynthGraphs(tts[0], tts[1], int16_scale=32768.0, warm=1, **kw)


def test_unseen_utterances_replay(tts):
    """Twelve utterances, distinct texts and phoneme counts, in two text buckets (Tb = 16 / 32) and two capacities
    (d_control 0.5: ~4 frames per phoneme, so Rcap = 64 / 128).  Per bucket: one warm run, one run that captures
    graph 1 and warms graph 2, one that captures graph 2 -- everything after that only replays."""
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.ops import hip

    model, g, utt = tts
    sg = _graphs(tts, bucketed=True)
    Ts = [5, 6, 8, 9, 11, 12, 17, 19, 21, 23, 25, 27]
    seen_tb, seen_cap = set(), set()
    for k, T in enumerate(Ts):
        a = utt(T)
        before = dict(sg.stats)
        wav, lens = sg(*a, d_control=0.5)
        wav_e, lens_e = sg.eager(*a, d_control=0.5)
        assert lens == lens_e and wav.shape == (1, lens[0] * HOP) and torch.equal(wav, wav_e), (T, lens, lens_e)
        assert wav.any()
        seen_tb.add(FastSpeech2.pad_text_bucket(T))
        seen_cap.add(hip.cap_bucket(lens))
        if k % 6 >= 3:  # the bucket is open: replays only (graph 1 + graph 2)
            assert (sg.stats["captures"], sg.stats["eager"]) == (before["captures"], before["eager"]), (T, sg.stats)
            assert sg.stats["replays"] == before["replays"] + 2
    assert seen_tb == {16, 32} and seen_cap == {(64, 64), (128, 128)}, (seen_tb, seen_cap)
    st = sg.stats
    assert (st["captures"], st["eager"], st["replays"]) == (4, 4, 18), st


def test_bucketed_equals_each_utterance_alone(tts):
    """The existing packed path as oracle, under the pinning of ``tests/test_synth_packed_gpu.py::pinned_gemm`` (one
    GEMM kernel family: skinny off, split-K off, no fused GEMM + LayerNorm).  Observed on MI355X: every mel length
    equal; _rel 0.0 wherever the capacity picks the kernels the utterance alone picks (the padded rows, the filler
    and the null tiles change no bit of a real utterance), at most 2.6e-3 where the row count moves the C = 256 MRF
    across ``hifigan._RB256_MIN_ROWS`` (a capacity above 128 frames runs the ResBlock kernel, an utterance of up to
    128 frames alone the GEMMs)."""
    from speakingstyle_amd.ops import hip

    model, g, utt = tts
    hip.lib().ssamd_gemm_set_skinny(0)
    hip.lib().ssamd_gemm_set_splitk(0)
    rows_saved = hip.GEMM_ADDLN_MAX_ROWS
    hip.GEMM_ADDLN_MAX_ROWS = 0
    try:
        sg = _graphs(tts, bucketed=True)
        worst = 0.0
        jobs = [[T] for T in (9, 14, 11, 20, 27, 8, 13, 16, 30, 22, 17, 25)] + [[5, 12, 9], [16, 3, 10], [7, 7, 12]]
        for Ts in jobs:
            a = utt(Ts)
            wav, lens = sg(*a)
            assert wav.shape == (len(Ts), max(lens) * HOP)
            for i, T in enumerate(Ts):
                one = tuple(t[i:i + 1] if isinstance(t, torch.Tensor) else t for t in a)
                one = (one[0], one[1][:, :T].contiguous(), one[2], T) + one[4:]  # this utterance alone, unpadded
                rows, lens_o, _ = model.infer_packed(*one)
                ref = g.infer_packed(rows, lens_o, int16_scale=32768.0)
                assert [lens[i]] == lens_o, (Ts, i, lens, lens_o)
                n = lens[i] * HOP
                e = _rel(wav[i, :n], ref[0, :n])
                worst = max(worst, e)
                print(f"bucketed vs alone: T={Ts} row {i} frames {lens[i]} _rel {e:.3e}")
                assert e < 5e-2, (Ts, i, e)
                assert not wav[i, n:].any()
        print(f"largest _rel: {worst:.3e}; stats {sg.stats}")
        assert sg.stats["replays"] > 0
    finally:
        hip.lib().ssamd_gemm_set_skinny(1)
        hip.lib().ssamd_gemm_set_splitk(-1)
        hip.GEMM_ADDLN_MAX_ROWS = rows_saved


def test_batch_of_three_and_stale_tail(tts):
    """B = 3 with mixed lengths replays bitwise; a short text after a long one in the same Tb bucket does not see
    the long one's tail in the static inputs."""
    model, g, utt = tts
    sg, fresh = _graphs(tts, bucketed=True), _graphs(tts, bucketed=True)
    for Ts in ([5, 12, 9], [11, 4, 8], [12, 12, 3], [6, 9, 10]):
        a = utt(Ts)
        wav, lens = sg(*a)
        wav_e, lens_e = fresh.eager(*a)
        assert lens == lens_e and torch.equal(wav, wav_e) and wav.shape == (3, max(lens) * HOP)
        for i, n in enumerate(lens):
            assert not wav[i, n * HOP:].any()
    assert sg.stats["replays"] >= 3 and sg.stats["captures"] >= 2, sg.stats  # the later batches did replay
    sg = _graphs(tts, bucketed=True)
    for T in (15, 14, 13, 15, 6, 16, 3):  # opened by long texts; then long -> short -> long -> short
        a = utt(T)
        wav, lens = sg(*a)
        wav_e, lens_e = fresh.eager(*a)
        assert lens == lens_e and torch.equal(wav, wav_e), T


def test_same_utterance_after_forty_others(tts):
    model, g, utt = tts
    sg = _graphs(tts, bucketed=True)
    A = utt(13)
    first, lens_first = sg(*A, d_control=0.5)
    rng = np.random.default_rng(9)
    for T in rng.integers(4, 32, size=40):
        sg(*utt(int(T)), d_control=0.5)
    again, lens_again = sg(*A, d_control=0.5)
    assert lens_again == lens_first and torch.equal(again, first)
    assert sg.stats["replays"] > 60, sg.stats


def test_exact_key_graph_keeps_its_vocoder_tables(tts):
    """``bucketed=False``: the graph-2 entry owns the VocPack its graph reads -- more other length sets than the
    kernel library's LRU holds (32) go through ``Generator.infer_packed``, then the first utterance replays."""
    model, g, utt = tts
    sg = _graphs(tts)
    A = utt(14)
    for _ in range(3):
        wav, lens = sg(*A)
    assert sg.stats["captures"] == 2
    e2 = next(iter(sg.g2.values()))
    assert e2["graph"] is not None and e2["pack"].lens.tolist() == lens
    torch.manual_seed(3)
    for n in range(40, 40 + 36):
        if [n] != lens:
            g.infer_packed(torch.randn(n, 80, device=wav.device), [n], int16_scale=32768.0)
    before = dict(sg.stats)
    wav2, lens2 = sg(*A)
    assert sg.stats["captures"] == before["captures"] and sg.stats["replays"] == before["replays"] + 2
    rows, lens_e, _ = model.infer_packed(*A)
    ref = g.infer_packed(rows, lens_e, int16_scale=32768.0)
    assert lens2 == lens_e and torch.equal(wav2, ref) and torch.equal(wav2, wav)


@pytest.mark.parametrize("bucketed", [False, True])
def test_weight_generation_drops_the_graphs(tts, bucketed):
    from speakingstyle_amd.ops import hip

    model, g, utt = tts
    sg = _graphs(tts, bucketed=bucketed)
    A = utt(12)
    for _ in range(3):
        wav, lens = sg(*A)
    assert sg.stats["captures"] == 2 and len(sg.g1) == 1 and len(sg.g2) == 1
    hip.bump_weight_generation()
    w1, l1 = sg(*A)  # the graphs are gone: this call warms again ...
    assert sg.stats["captures"] == 2 and sg.g1 and next(iter(sg.g1.values()))["graph"] is None
    w2, l2 = sg(*A)
    w3, l3 = sg(*A)  # ... and the next two recapture graph 1 and graph 2
    assert sg.stats["captures"] == 4 and sg.wgen == hip.generation()
    ref, lens_e = sg.eager(*A)
    for w, l_ in ((w1, l1), (w2, l2), (w3, l3)):
        assert l_ == lens_e == lens and torch.equal(w, ref) and torch.equal(w, wav)


def test_serve_cli_equals_synthesizer(tmp_path):
    """``synthesize.py --mode serve``: three lines -> three wavs, the samples ``Synthesizer.tts`` returns."""
    import sys

    import yaml
    from scipy.io import wavfile

    from speakingstyle_amd.config import config_dir_triplet, load_configs, load_yaml
    from speakingstyle_amd.infer.serve import Synthesizer
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.utils.model import ROOT, save_checkpoint

    sys.path.insert(0, ROOT)
    import synthesize as cli

    p_path, m_path, t_path = config_dir_triplet("BC2013_GST")
    pp, tc = load_yaml(p_path), load_yaml(t_path)
    for k, v in pp["path"].items():  # the repository's relative paths, from wherever the test runs
        if isinstance(v, str) and not os.path.isabs(v):
            pp["path"][k] = os.path.join(ROOT, v)
    tc["path"]["ckpt_path"] = str(tmp_path / "ckpt")
    tc["path"]["result_path"] = str(tmp_path / "out")
    files = []
    for name, cfg in (("p.yaml", pp), ("t.yaml", tc)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as f:
            yaml.safe_dump(cfg, f)
    configs = load_configs(files[0], m_path, files[1])
    torch.manual_seed(0)
    model = FastSpeech2(configs[0], configs[1])
    with torch.no_grad():  # a duration head that speaks: ~8 frames per phoneme
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(9.1))
    save_checkpoint(os.path.join(tc["path"]["ckpt_path"], "1.pth.tar"), model)
    lines = ["Hello there.", "The quick brown fox jumps over the lazy dog.", "Graphs replay."]
    src = tmp_path / "lines.txt"
    src.write_text("\n".join(lines) + "\n")
    torch.manual_seed(7)  # the vocoder has no checkpoint here: the same random one on both sides
    cli.main(["--mode", "serve", "--source", str(src), "--restore_step", "1", "-p", files[0], "-m", m_path,
              "-t", files[1]])
    torch.manual_seed(7)
    s = Synthesizer(configs, 1)
    for i, line in enumerate(lines):
        sr, got = wavfile.read(os.path.join(tc["path"]["result_path"], f"serve_{i:04d}.wav"))
        want = s.tts(line)
        assert sr == s.sampling_rate and want.dtype == np.int16 and want.size > 20 * HOP
        assert np.array_equal(got, want), i
    assert s.stats["eager"] + s.stats["replays"] > 0
