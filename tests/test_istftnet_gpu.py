"""iSTFTNet on the GPU: the head kernel (``csrc/k_istft.hip``) alone against the float64 reference op, padded and
packed; the C8C8I generator's packed path against each utterance alone and against the fp32 torch forward; and the
bucketed serving graphs with the iSTFT generator.  The numerics tests print their figures (``ISTFTNUM`` lines:
profiles/istftnet_numerics.txt is made from them)."""
import contextlib
import functools
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
HOP = 256
MARGIN = 8  # kernel deviation allowed, in units of the float32 reference op's own deviation from float64


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


def _operands(T, C=128, B=2, seed=0):
    """x ~ N(0, 1) in bf16, w ~ N(0, 0.02^2) and b ~ N(0, 0.1^2) rounded to bf16 (kernel and oracle see identical
    operands; |z| stays within about +-2), all on the CPU."""
    g = torch.Generator().manual_seed(1000 * seed + T + C)
    x = torch.randn(B, T, C, generator=g).to(torch.bfloat16)
    w = (torch.randn(18, C, 7, generator=g) * 0.02).to(torch.bfloat16).float()
    b = (torch.randn(18, generator=g) * 0.1).to(torch.bfloat16).float()
    return x, w, b


@functools.lru_cache(maxsize=None)
def _oracle(T, C=128):
    """(float64 result, float32 CPU result) of the reference op on the case's operands; computed once, never written."""
    from speakingstyle_amd.ops import reference as ref

    x, w, b = _operands(T, C)
    r64 = ref.istft_head(x.double(), w.double(), b.double(), 16, 4)
    r32 = ref.istft_head(x.float(), w, b, 16, 4)
    return r64, r32


def _head_case(T, C):
    from speakingstyle_amd.ops import hip

    x, w, b = _operands(T, C)
    r64, r32 = _oracle(T, C)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = hip.istft_head(xd, wd, bd)
    assert y.shape == (2, 4 * T) and y.dtype == torch.float32
    peak = float(r64.abs().max())
    d_t = float((r32.double() - r64).abs().max()) / peak
    d_k = float((y.double().cpu() - r64).abs().max()) / peak
    print(f"ISTFTNUM head C={C} T={T} cpu_fp32={d_t:.3e} hip={d_k:.3e} ratio={d_k / max(d_t, 1e-30):.2f} "
          f"bound={MARGIN * d_t:.3e}")
    assert d_t > 0 and d_t < 1e-4, d_t  # the yardstick itself is a rounding-level figure
    assert d_k <= MARGIN * d_t, (T, d_k, d_t)
    # int16 form: clamp and convert of the fp32 form, bitwise (scale chosen so that some samples clamp)
    scale = 32768.0 * 0.9 / float(y.abs().max()) * 1.5
    yi = hip.istft_head(xd, wd, bd, int16_scale=scale)
    want = (y * scale).clamp(-32768, 32767).to(torch.int16)
    assert yi.dtype == torch.int16 and torch.equal(yi, want)
    assert bool((want == 32767).any() or (want == -32768).any())
    # two runs are bitwise equal
    assert torch.equal(hip.istft_head(xd, wd, bd), y)


@pytest.mark.parametrize("T", [2, 7, 63, 64, 65, 130, 257])
def test_head_padded_vs_float64(T):
    _head_case(T, 128)


@pytest.mark.parametrize("T", [2, 130])
def test_head_padded_vs_float64_c64(T):
    """The C = 64 instantiation (two K steps per tap): one tile and a tile boundary."""
    _head_case(T, 64)


def test_head_rejects_what_it_cannot_run():
    from speakingstyle_amd.ops import hip

    x, w, b = (t.to(DEV) for t in _operands(1))
    with pytest.raises(ValueError):
        hip.istft_head(x, w, b)
    x, w, b = _operands(4, C=32)
    with pytest.raises(ValueError):
        hip.istft_head(x.to(DEV), w.to(DEV), b.to(DEV))
    assert hip.istft_head_has(128) and not hip.istft_head_has(128, 32, 8) and not hip.istft_head_has(32)
    assert hip.voc_tile_rows("istft", 128) in (32, 64, 128)


class _WithNullTiles:
    """A VocPack whose tile tables carry ``extra`` null tiles {0, 0, 0, 0} at the end."""

    def __init__(self, vp, extra=3):
        self.vp, self.extra = vp, extra
        self.lens, self.R, self.B, self.cu = vp.lens, vp.R, vp.B, vp.cu

    def tiles(self, rate, bm):
        tt, n = self.vp.tiles(rate, bm)
        return torch.cat([tt, torch.zeros(4 * self.extra, device=tt.device, dtype=tt.dtype)]), n + self.extra


def test_head_packed_equals_each_utterance_alone():
    from speakingstyle_amd.ops import hip

    dev = torch.device(DEV, 0)
    C, rate, lens = 128, 64, [1, 3, 2, 8, 1]
    vp = hip.VocPack(lens, dev, [(rate, hip.voc_tile_rows("istft", C))])
    _, w, b = _operands(5)
    w, b = w.to(dev), b.to(dev)
    torch.manual_seed(11)
    x = torch.randn(sum(lens) * rate, C, device=dev).to(torch.bfloat16)
    W = max(lens) * rate * 4
    SENT = 12345.0
    bufs = []
    for pk in (vp, vp, _WithNullTiles(vp)):
        big = torch.full((len(lens) + 2, W), SENT, device=dev)  # a guard row before and after
        big[1:-1].zero_()  # the caller zero-fills
        hip.istft_head_packed(x, pk, rate, w, b, big[1:-1])
        bufs.append(big)
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[1])  # two runs
    assert torch.equal(bufs[0], bufs[2])  # null tiles change nothing
    out = bufs[0][1:-1]
    for big in bufs:
        assert bool((big[0] == SENT).all()) and bool((big[-1] == SENT).all())
    o = 0
    for u, L in enumerate(lens):
        alone = hip.istft_head(x[o * rate:(o + L) * rate].unsqueeze(0).contiguous(), w, b)[0]
        n = L * rate * 4
        assert alone.shape == (n,) and torch.equal(out[u, :n], alone), u
        assert not out[u, n:].any()
        assert out[u, :n].any()
        o += L
    # int16, packed: clamp and convert of the fp32 form
    scale = 32768.0 / float(out.abs().max()) * 1.5
    oi = torch.zeros(len(lens), W, device=dev, dtype=torch.int16)
    hip.istft_head_packed(x, vp, rate, w, b, oi, int16_scale=scale)
    assert torch.equal(oi, (out * scale).clamp(-32768, 32767).to(torch.int16))


# ------------------------------------------------------------------------------------------------ generator
@contextlib.contextmanager
def torch_fp32_only():
    """Force the torch reference ops and make the HIP kernel library unreachable (as the fp32 oracles of
    tests/test_vocoder_oracle_gpu.py do): the oracle provably runs no ``ssamd_`` kernel."""
    from speakingstyle_amd import ops
    from speakingstyle_amd.models import hifigan as H
    from speakingstyle_amd.ops import hip

    saved = (hip.lib, H._hip_train, ops._FORCED)

    def _no_kernels(*a, **k):
        raise AssertionError("an ssamd_ kernel was reached inside the fp32 oracle")

    hip.lib = _no_kernels
    H._hip_train = lambda: False
    ops.set_backend("reference")
    try:
        yield
    finally:
        hip.lib = saved[0]
        H._hip_train = saved[1]
        ops.set_backend(saved[2])


def _istft_generator(seed):
    from speakingstyle_amd.models import hifigan as H

    with open(os.path.join(ROOT, "config", "hifigan", "config_istft.json")) as f:
        h = H.AttrDict(json.load(f))
    torch.manual_seed(seed)
    return H.Generator(h).eval().fold_weight_norm().to(DEV)


def test_generator_packed_vs_alone_and_fp32_forward():
    """``infer_packed`` of the C8C8I generator (random init) against each utterance alone on ``_infer_hip`` (1e-2
    relative L2, the bound of test_packed_vocoding_equals_each_utterance_alone; zeros past each length), and against
    the fp32 torch ``forward`` per utterance for lengths >= 8 (5e-2, the generator budget of the fp32 oracle test).
    exp() multiplies the trunk's bf16 error, so the trunk-output error (lrelu of the last stage, HIP bf16 against
    fp32 torch) and the total are printed per utterance."""
    from speakingstyle_amd import ops

    g = _istft_generator(9)
    assert g.packable() and g.hop == HOP
    lengths = [40, 1, 17, 9, 33]
    B, T = len(lengths), max(lengths) + 3
    torch.manual_seed(5)
    mel = torch.randn(B, T, 80, device=DEV) * 2 - 5
    trunk = {}
    real_head = ops.istft_head

    def spy(x, *a, **k):
        trunk["hip"] = F.leaky_relu(x.float(), 0.01)
        return real_head(x, *a, **k)

    with torch.no_grad():
        pk = g.infer(mel, int16_scale=32768.0, lengths=lengths)
        pkf = g.infer_packed(mel, lengths)
        assert pk.shape == (B, T * HOP) and pk.dtype == torch.int16 and pkf.shape == (B, max(lengths) * HOP)
        trunks = []
        for i, n in enumerate(lengths):
            one = mel[i:i + 1, :n].to(torch.bfloat16).contiguous()
            alone = g.infer(one, int16_scale=32768.0)[0]
            assert _rel(pk[i, : n * HOP], alone) < 1e-2, (i, _rel(pk[i, : n * HOP], alone))
            assert not pk[i, n * HOP:].any()
            ops.istft_head = spy
            try:
                alone_f = g.infer(one)[0]
            finally:
                ops.istft_head = real_head
            trunks.append(trunk.pop("hip")[0])
            assert _rel(pkf[i, : n * HOP], alone_f) < 1e-2, (i, _rel(pkf[i, : n * HOP], alone_f))
            assert not pkf[i, n * HOP:].any()
    seen = {}
    hook = g.conv_post.register_forward_pre_hook(lambda m, a: seen.__setitem__("x", a[0]))
    try:
        worst = 0.0
        for i, n in enumerate(lengths):
            if n < 8:
                continue
            with torch_fp32_only(), torch.no_grad():
                ref = g(mel[i:i + 1, :n].transpose(1, 2)).reshape(-1)
            t_ref = seen.pop("x")[0, :, 1:].t()  # without the reflected column: lrelu of the last stage, [T, C]
            e_trunk, e_total = _rel(trunks[i], t_ref), _rel(pkf[i, : n * HOP], ref)
            worst = max(worst, e_total)
            print(f"ISTFTNUM generator frames={n} trunk={e_trunk:.3e} total={e_total:.3e} "
                  f"gain={e_total / max(e_trunk, 1e-30):.2f} bound=5.000e-02")
            assert e_total < 5e-2, (i, e_total, e_trunk)
        print(f"ISTFTNUM generator worst_total={worst:.3e}")
    finally:
        hook.remove()


# ------------------------------------------------------------------------------------------------ serving
@pytest.fixture(scope="module")
def tts():
    """BC2013_GST model with a duration head that speaks (the fixture of tests/test_serve_buckets_gpu.py), the
    iSTFTNet generator, one reference mel."""
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2

    dev = torch.device(DEV, 0)
    pp, mc, tc = load_named("BC2013_GST")
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc).to(dev)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(9.1))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    g = _istft_generator(1)
    g.requires_grad_(False)
    ref = SyntheticBatches(1, device=dev, seed=12, max_seq_len=mc["max_seq_len"],
                           phone_counts=np.array([14])).make_batch()
    rng = np.random.default_rng(5)

    def utt(T):
        ids = torch.from_numpy(rng.integers(1, 300, size=(1, T)).astype(np.int64)).to(dev)
        return (ref[2][:1].contiguous(), ids, torch.tensor([T], device=dev), T, ref[6][:1].contiguous(),
                ref[7][:1].contiguous(), ref[8])

    return model, g, utt


def test_bucketed_graphs_replay_with_the_istft_generator(tts):
    """One text bucket and one capacity: a warm run, one that captures graph 1, one that captures graph 2; then three
    unseen texts only replay, each bit for bit the eager ``infer_packed`` run.  No table, graph or hop edit was
    needed for the head: the capacity tables are generic and the graphs take the hop from the output shape."""
    from speakingstyle_amd.infer.graphs import SynthGraphs

    model, g, utt = tts
    sg = SynthGraphs(model, g, int16_scale=32768.0, warm=1, bucketed=True)
    for T in (5, 6, 8):
        sg(*utt(T), d_control=0.5)
    for T in (9, 11, 12):
        a = utt(T)
        before = dict(sg.stats)
        wav, lens = sg(*a, d_control=0.5)
        wav_e, lens_e = sg.eager(*a, d_control=0.5)
        assert lens == lens_e and wav.shape == (1, lens[0] * HOP) and wav.dtype == torch.int16
        assert torch.equal(wav, wav_e), (T, lens)
        assert wav.any()
        assert (sg.stats["captures"], sg.stats["eager"]) == (before["captures"], before["eager"]), (T, sg.stats)
        assert sg.stats["replays"] == before["replays"] + 2
