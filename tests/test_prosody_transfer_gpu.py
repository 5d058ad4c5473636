"""csrc/k_prosody.hip against ``ops.reference.prosody_transfer`` in float64, and the second synthesis pass of
``infer/transfer.py`` on the GPU.

Numerics convention (as for tests/test_align_gpu.py): the yardstick of a case is the float32 torch reference's own
deviation from the float64 reference on the same inputs, the maximum over 8 seeds; the kernel may deviate from float64
by up to 8 times that (hardware log2 / exp2 are about 1 ulp against libm's 0.5), with a floor of 2^-20 max(1,
max |oracle|).  Every comparison prints its figures (``PROSNUM`` lines) before it asserts.  The references of a case are
computed once and shared."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from prosody_signals import cast, pack_case, random_utterance, recover, rendered_pair
from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SEEDS = 8
MARGIN = 8.0
P_STATS, E_STATS = (180.0, 45.0), (20.0, 12.0)
NS = (1, 2, 63, 64, 65, 129, 300)
YS = (1, 2, 63, 64, 65, 255, 256, 257, 1100)
VOICING = ("mixed",) * 6 + ("first", "last")  # seeds 6 / 7: one voiced frame, at the first / the last frame


@functools.lru_cache(maxsize=None)
def references(n, ty, mode):
    """The 8 seeds of a case as one batch (x_len from ty / 2 to 2 ty, durations with zeros): inputs, the float64
    reference and the float32 reference's deviation from it per output."""
    utts = [random_utterance(100003 * s + 1009 * n + ty, n, ty, VOICING[s]) for s in range(SEEDS)]
    args = pack_case(utts)
    r64 = ref.prosody_transfer(*args, P_STATS, E_STATS, mode)
    r32 = ref.prosody_transfer(*cast(args, torch.float32), P_STATS, E_STATS, mode)
    assert torch.equal(r32[0], r64[0]) and torch.equal(r32[4], r64[4])
    dev = [float((r32[k].double() - r64[k]).abs().max()) for k in (1, 2, 3)]
    return args, r64, dev


@pytest.mark.parametrize("ty", YS)
@pytest.mark.parametrize("n", NS)
def test_kernel_against_float64(n, ty):
    for mode in ("relative", "absolute"):
        args, r64, dev = references(n, ty, mode)
        out = ops.prosody_transfer(*cast(args, torch.float32, "cuda"), P_STATS, E_STATS, mode)
        assert out[0].dtype == torch.int32 and out[4].dtype == torch.bool and out[1].dtype == torch.float32
        assert torch.equal(out[0].cpu(), r64[0]) and torch.equal(out[4].cpu(), r64[4])
        for k, name in ((1, "pitch"), (2, "energy"), (3, "voiced")):
            err = float((out[k].cpu().double() - r64[k]).abs().max())
            floor = 2.0 ** -20 * max(1.0, float(r64[k].abs().max()))
            print(f"PROSNUM {mode} N={n} y_len={ty} {name}: |oracle| {float(r64[k].abs().max()):.2f} ref32 "
                  f"{dev[k - 1]:.3e} hip {err:.3e} floor {floor:.3e}")
            assert torch.isfinite(out[k]).all()
            assert err <= max(MARGIN * dev[k - 1], floor), (mode, name)


def test_more_than_1024_tokens_is_refused_on_the_gpu():
    path = torch.zeros(1, 1, 2, dtype=torch.int32, device="cuda")
    one = torch.ones(1, device="cuda")
    with pytest.raises(ValueError, match="1025"):
        ops.prosody_transfer(path, torch.ones(1, dtype=torch.int32, device="cuda"),
                             torch.ones(1, 1025, dtype=torch.int32, device="cuda"), [1025], [1], [1], one, one,
                             torch.zeros(1, 1025, device="cuda"))


def test_1024_tokens_and_a_long_recording():
    """The token limit itself, and a recording far longer than anything LDS could hold."""
    u = random_utterance(7, 1024, 9000, tx=6000)
    args = pack_case([u])
    r64 = ref.prosody_transfer(*args, P_STATS, E_STATS, "relative")
    r32 = ref.prosody_transfer(*cast(args, torch.float32), P_STATS, E_STATS, "relative")
    gpu = list(cast(args, torch.float32, "cuda"))
    gpu[3] = [1024]  # the token counts as a host list
    out = ops.prosody_transfer(*gpu, P_STATS, E_STATS, "relative")
    assert torch.equal(out[0].cpu(), r64[0]) and int(out[0].sum()) == 9000
    for k in (1, 2, 3):
        dev = float((r32[k].double() - r64[k]).abs().max())
        err = float((out[k].cpu().double() - r64[k]).abs().max())
        print(f"PROSNUM relative N=1024 y_len=9000 output {k}: ref32 {dev:.3e} hip {err:.3e}")
        assert err <= max(MARGIN * dev, 2.0 ** -20 * max(1.0, float(r64[k].abs().max())))


BATCH = [(300, 1100), (1, 1), (64, 257), (129, 63), (2, 256)]  # (N, y_len)


def test_batch_is_each_utterance_alone_bitwise():
    utts = [random_utterance(900 + k, n, ty) for k, (n, ty) in enumerate(BATCH)]
    both = ops.prosody_transfer(*cast(pack_case(utts), torch.float32, "cuda"), P_STATS, E_STATS, "relative")
    again = ops.prosody_transfer(*cast(pack_case(utts), torch.float32, "cuda"), P_STATS, E_STATS, "relative")
    for a, b in zip(both, again):
        assert torch.equal(a, b)
    for p, u in enumerate(utts):
        n = len(u["src_dur"])
        alone = ops.prosody_transfer(*cast(pack_case([u]), torch.float32, "cuda"), P_STATS, E_STATS, "relative")
        for k in range(4):
            assert torch.equal(both[k][p, :n], alone[k][0]), (p, k)
            assert not both[k][p, n:].any()
        assert bool(both[4][p]) == bool(alone[4][0])


def test_recovery_on_rendered_audio_on_the_gpu():
    """The rendered pairs through the GPU log-mel, ``ops.pyin``, ``ops.dtw`` and the kernel: the caps of the CPU test."""
    pairs = [rendered_pair(seed) for seed in range(100, 106)]
    d_err, p_err, e_err = recover(pairs, torch.device("cuda"))
    print(f"PROSREC gpu duration {d_err:.0f} frames, pitch {100 * p_err:.2f} %, energy {100 * e_err:.2f} %")
    assert d_err <= 2 and p_err <= 0.05 and e_err <= 0.03


# ---------------------------------------------------------------------------- the second pass
def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp(min=1e-12)).item()


@pytest.fixture
def pinned_gemm():
    """One GEMM kernel family for the packed batch and the batch-1 runs (tests/test_synth_packed_gpu.py)."""
    from speakingstyle_amd.ops import hip

    hip.lib().ssamd_gemm_set_skinny(0)
    hip.lib().ssamd_gemm_set_splitk(0)
    rows = hip.GEMM_ADDLN_MAX_ROWS
    hip.GEMM_ADDLN_MAX_ROWS = 0
    yield
    hip.lib().ssamd_gemm_set_skinny(1)
    hip.lib().ssamd_gemm_set_splitk(-1)
    hip.GEMM_ADDLN_MAX_ROWS = rows


def _lj_model(dev):
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2

    configs = load_named("LJSpeech")
    torch.manual_seed(0)
    model = FastSpeech2(configs[0], configs[1]).to(dev)
    with torch.no_grad():  # ~8 frames per phoneme (the bench's duration head)
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(9.1))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    return configs, model


def test_packed_second_pass_equals_forward_with_the_targets(pinned_gemm):
    from speakingstyle_amd.data.synthetic import SyntheticBatches

    dev = torch.device("cuda", 0)
    (pp, mc, tc), model = _lj_model(dev)
    b = SyntheticBatches(4, device=dev, seed=3, max_seq_len=mc["max_seq_len"]).make_batch()
    args = (b[2], b[3], b[4], b[5], b[6], b[7], b[8])
    assert model.packed_inference_ok(b[3])
    g = torch.Generator().manual_seed(4)
    T = b[3].shape[1]
    inside = torch.arange(T, device=dev).unsqueeze(0) < b[4].unsqueeze(1)
    d_t = (torch.randint(0, 13, (4, T), generator=g).to(dev) * inside).long()
    p_t, e_t = torch.randn(4, T, generator=g).to(dev), torch.randn(4, T, generator=g).to(dev)
    front = model.infer_front(*args, p_targets=p_t, e_targets=e_t, d_targets=d_t)
    lens = front[2].tolist()
    assert lens == d_t.sum(1).tolist() and torch.equal(front[1], d_t)
    rows = model.infer_back(front, lens)
    assert rows.shape == (sum(lens), 80)
    cu = np.concatenate([[0], np.cumsum(lens)])
    for i, n in enumerate(lens):
        one = tuple(a[i:i + 1] if isinstance(a, torch.Tensor) else a for a in args)
        with torch.no_grad():  # the style reference (b[6], another length) must not size the result
            alone = model(*one, p_targets=p_t[i:i + 1], e_targets=e_t[i:i + 1], d_targets=d_t[i:i + 1],
                          mels_style_only=True)
        assert alone[9].tolist() == [n] and alone[1].shape[1] == n
        e = _rel(rows[cu[i]:cu[i + 1]], alone[1][0, :n])
        assert e < 2e-2, (i, e)
    # and without targets the front is what it was
    plain = model.infer_front(*args)
    assert len(plain) == 4 and plain[2].tolist() != lens


def test_tts_with_a_prosody_reference_leaves_the_graphs_alone(tmp_path):
    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.infer.serve import Synthesizer
    from speakingstyle_amd.models.hifigan import Generator, default_config
    from speakingstyle_amd.utils.model import ROOT

    dev = torch.device("cuda", 0)
    configs, model = _lj_model(dev)
    for k, v in configs[0]["path"].items():
        if isinstance(v, str) and not os.path.isabs(v):
            configs[0]["path"][k] = os.path.join(ROOT, v)
    torch.manual_seed(1)
    voc = Generator(default_config()).eval().fold_weight_norm().to(dev)
    s = Synthesizer(configs, device=dev, model=model, vocoder=voc)
    rec = rendered_pair(100)["y"]
    wav_path = str(tmp_path / "rec.wav")
    write_wav(wav_path, s.sampling_rate, (rec["wav"] * 32767.0).astype(np.int16))
    text = "The quick brown fox jumps over the lazy dog."
    plain = [s.tts(text) for _ in range(3)]  # warm, capture, replay
    assert np.array_equal(plain[0], plain[2])
    before = s.stats
    stats = {"pitch": P_STATS, "energy": E_STATS}
    import speakingstyle_amd.infer.transfer as transfer

    saved = transfer.normalisation
    transfer.normalisation = lambda pp: stats  # no stats.json of a training run here
    try:
        like = s.tts(text, prosody_ref=wav_path)
        half = s.tts(text, prosody_ref=wav_path, transfer=("duration",), transfer_strength=0.5)
    finally:
        transfer.normalisation = saved
    from speakingstyle_amd.infer.synthesis import single_batch

    frames = int(rec["dur"].sum())
    phones = int(single_batch(text, configs[0], 0, None, s.lexicon)[0][4][0])
    # strength 1: the recording's frames, plus one for every phoneme the recording gave none (min_frames)
    assert like.dtype == np.int16 and like.size % s.hop == 0
    assert frames <= like.size // s.hop <= frames + phones
    assert abs(half.size - (plain[0].size + like.size) // 2) <= s.hop * 40 and half.size != like.size
    assert s.stats == before and list(s._prosody) == [wav_path]
    again = s.tts(text)
    assert np.array_equal(again, plain[0])
    assert s.stats["replays"] == before["replays"] + 2 and s.stats["captures"] == before["captures"]
