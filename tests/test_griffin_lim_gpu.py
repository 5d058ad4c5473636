"""Griffin-Lim kernels (csrc/k_griffin.hip) against the torch reference op in float64.

Tolerance of the sample comparisons, relative to the peak of the float64 result: 32 x the deviation of the SAME
computation in torch float32 on the CPU from float64, measured inside the test (a radix-2 LDS FFT with computed
twiddles is a few times worse than pocketfft and the phase projection amplifies rounding; a wrong index, window
or normalisation is wrong at the 1e-1 level).  Samples are compared after at most 3 iterations -- float32 and
float64 drift apart after that -- and 30 iterations are judged by their spectral convergence.  Every comparison
prints its figures (``GLNUM`` lines: profiles/griffin_lim_numerics.txt is made from them)."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from speakingstyle_amd import ops  # noqa: E402
from speakingstyle_amd.audio.stft import TacotronSTFT  # noqa: E402
from speakingstyle_amd.ops import hip, reference as ref  # noqa: E402

SR = 22050
MARGIN = 32.0
# the geometries of test_audio_gpu.py at their minimum frame counts, plus one longer utterance
CASES = [(1024, 256, 1024, 4), (1024, 256, 800, 5), (512, 128, 512, 4), (2048, 300, 1200, 5), (1024, 256, 1024, 37)]


@functools.lru_cache(maxsize=None)
def _case(n_fft, hop, win, T):
    """B = 2 utterances of T frames: (stft, window [n_fft], mag [2, T, NB], phase [2, T, NB], log-mel [2, T, 80])."""
    assert T >= ref.gl_min_frames(n_fft, hop)
    stft = TacotronSTFT(n_fft, hop, win, 80, SR, 0.0, 8000.0)
    g = torch.Generator().manual_seed(n_fft + hop + T)
    t = torch.arange(hop * (T - 1)) / SR
    y = (0.5 * torch.sin(2 * torch.pi * 220 * t) + 0.1 * torch.randn(2, t.numel(), generator=g)).clamp(-1, 1)
    mag = stft.magnitudes(y).transpose(1, 2).contiguous()
    assert mag.shape == (2, T, n_fft // 2 + 1)
    ph = (2 * math.pi * torch.rand(mag.shape, generator=g)).contiguous()
    mel = torch.log(torch.clamp(mag @ stft.mel_basis.t(), min=1e-5)).contiguous()
    return stft, stft.fft_window("cpu"), mag, ph, mel


@functools.lru_cache(maxsize=None)
def _oracle(n_fft, hop, win, T, n_iters, momentum):
    """(float64 result, float32 CPU result) of the reference op on the case's magnitudes and phases."""
    _, w, mag, ph, _ = _case(n_fft, hop, win, T)
    r64 = ref.griffin_lim(mag.double(), n_fft, hop, w.double(), n_iters, momentum, init_phase=ph.double())
    r32 = ref.griffin_lim(mag, n_fft, hop, w, n_iters, momentum, init_phase=ph)
    return r64, r32


def _judge(what, case, got, r64, r32):
    """got (HIP, fp32) vs the float64 oracle, bound = MARGIN x the CPU-float32 deviation, all relative to the peak."""
    peak = float(r64.abs().max())
    cpu = float((r32.double() - r64).abs().max()) / peak
    dev = float((got.double().cpu() - r64).abs().max()) / peak
    print(f"GLNUM {what} n_fft={case[0]} hop={case[1]} win={case[2]} T={case[3]} cpu_fp32={cpu:.3e} hip={dev:.3e} "
          f"ratio={dev / max(cpu, 1e-30):.2f} bound={MARGIN * cpu:.3e}")
    # the yardstick itself must be a rounding-level figure: 32 x 1e-3 stays below the 1e-1 of a wrong index / window
    assert cpu > 0 and cpu < 1e-3, cpu
    assert dev <= MARGIN * cpu, (what, case, dev, cpu)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_istft_matches_torch_float64(case):
    n_fft, hop, win, T = case
    stft, w, mag, ph, _ = _case(*case)
    spec = torch.polar(mag, ph)  # complex64 [2, T, NB]
    s_t = spec.transpose(1, 2)
    r64 = torch.istft(s_t.to(torch.complex128), n_fft, hop, win, window=stft.window.double())
    r32 = torch.istft(s_t, n_fft, hop, win, window=stft.window)
    got = ops.istft(spec.cuda(), n_fft, hop, w.cuda())
    assert got.shape == r64.shape == (2, hop * (T - 1)) and got.dtype == torch.float32
    _judge("istft", case, got, r64, r32)


@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("n_iters", [1, 3])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_griffin_lim_matches_reference_float64(case, n_iters, momentum):
    n_fft, hop, win, T = case
    _, w, mag, ph, _ = _case(*case)
    r64, r32 = _oracle(*case, n_iters, momentum)
    got = ops.griffin_lim(mag.cuda(), n_fft, hop, w.cuda(), n_iters, momentum, init_phase=ph.cuda())
    assert got.shape == r64.shape == (2, hop * (T - 1))
    _judge(f"griffin_lim iters={n_iters} momentum={momentum}", case, got, r64, r32)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_mel_inversion_matches_pinv_float64(case):
    n_fft, hop, win, T = case
    stft, w, _, ph, mel = _case(*case)
    pinv = torch.linalg.pinv(stft.mel_basis).contiguous()
    r64 = torch.clamp(torch.exp(mel.double()) @ pinv.double().t(), min=0.0)
    r32 = torch.clamp(torch.exp(mel) @ pinv.t(), min=0.0)
    _, mag = ops.griffin_lim(mel.cuda(), n_fft, hop, w.cuda(), 0, 0.0, init_phase=ph.cuda(), mel_pinv=pinv.cuda(),
                             return_mag=True)
    assert mag.shape == (2 * T, n_fft // 2 + 1) and float(mag.min()) >= 0
    _judge("mel_inversion", case, mag.view(2, T, -1), r64, r32)


def _convergence(stft, wav, mag):
    """||STFT(y)| - mag| / |mag| in float64 on the CPU (wav [B, N], mag [B, T, NB])."""
    s = torch.stft(wav.double().cpu(), stft.n_fft, stft.hop, stft.win, window=stft.window.double(), center=True,
                   pad_mode="reflect", return_complex=True).abs().transpose(1, 2)
    return float((s - mag.double()).norm() / mag.double().norm())


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_thirty_iterations_converge_like_float64(momentum):
    case = CASES[-1]
    n_fft, hop, win, T = case
    stft, w, mag, ph, _ = _case(*case)
    r64, _ = _oracle(*case, 30, momentum)
    got0 = ops.griffin_lim(mag.cuda(), n_fft, hop, w.cuda(), 0, momentum, init_phase=ph.cuda())
    got = ops.griffin_lim(mag.cuda(), n_fft, hop, w.cuda(), 30, momentum, init_phase=ph.cuda())
    c0, c_hip, c_ref = _convergence(stft, got0, mag), _convergence(stft, got, mag), _convergence(stft, r64, mag)
    print(f"GLNUM convergence momentum={momentum} T={T} iter0={c0:.4f} hip30={c_hip:.4f} float64_30={c_ref:.4f} "
          f"rel={abs(c_hip - c_ref) / c_ref:.4f}")
    assert abs(c_hip - c_ref) <= 0.02 * c_ref, (c_hip, c_ref)
    assert c_hip < c0, (c_hip, c0)


LENS = [4, 9, 37, 2, 1]


@functools.lru_cache(maxsize=None)
def _packed():
    """Packed magnitude rows of LENS at 1024 / 256 on the GPU (rows of the T = 37 case), and the window."""
    _, w, mag, _, _ = _case(*CASES[-1])
    rows = torch.cat([mag[b % 2, :n] for b, n in enumerate(LENS)], 0).contiguous().cuda()
    return rows, w.cuda()


def test_packed_batch_is_bitwise_each_utterance_alone():
    rows, w = _packed()
    for scale in (None, 32768.0):
        out = hip.griffin_lim(rows, 1024, 256, w, 3, 0.99, seed=11, lengths=LENS, int16_scale=scale)
        assert out.shape == (5, 256 * 36) and out.dtype == (torch.float32 if scale is None else torch.int16)
        o = 0
        for b, n in enumerate(LENS):
            alone = hip.griffin_lim(rows[o:o + n].contiguous(), 1024, 256, w, 3, 0.99, seed=11, int16_scale=scale)
            o += n
            N = 256 * (n - 1)
            assert alone.shape == (1, N)
            assert torch.equal(out[b, :N], alone[0]) and not out[b, N:].any(), (b, n)
            assert n < 2 or alone.any()
    # the 2-frame utterance is the iSTFT of its magnitude with the seeded phase: no iteration touched it (fp32
    # rounding is ~1e-6 of the peak; a wrong phase or an iteration is wrong at the 1e-1 level)
    two = rows[50:52].cpu()
    want = ref.istft(torch.polar(two.double(), ref.gl_seed_phase(11, 2, 513, dtype=torch.float64)), 1024, 256, w.cpu())
    got = hip.griffin_lim(rows, 1024, 256, w, 3, 0.99, seed=11, lengths=LENS)[3, :256].cpu()
    assert float((got.double() - want[0]).abs().max()) < 1e-4 * float(want.abs().max())


def test_seed_reproduces_and_matters():
    rows, w = _packed()
    a = hip.griffin_lim(rows, 1024, 256, w, 3, 0.99, seed=1, lengths=LENS)
    b = hip.griffin_lim(rows, 1024, 256, w, 3, 0.99, seed=1, lengths=LENS)
    c = hip.griffin_lim(rows, 1024, 256, w, 3, 0.99, seed=2, lengths=LENS)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert bool(torch.isfinite(a).all())


def test_outputs_are_zero_past_each_length_and_int16_is_the_conversion():
    rows, w = _packed()
    W = 256 * 37 + 77  # wider than the longest utterance, not a multiple of the block
    f = hip.griffin_lim(rows, 1024, 256, w, 2, 0.99, seed=3, lengths=LENS, width=W)
    i = hip.griffin_lim(rows, 1024, 256, w, 2, 0.99, seed=3, lengths=LENS, width=W, int16_scale=20000.0)
    assert f.shape == i.shape == (5, W) and i.dtype == torch.int16
    for b, n in enumerate(LENS):
        N = 256 * (n - 1)
        assert not f[b, N:].any() and not i[b, N:].any()
        assert n < 2 or (f[b, :N].any() and i[b, :N].any())
    assert torch.equal(i, (f * 20000.0).clamp(-32768, 32767).to(torch.int16))
    loud = hip.griffin_lim(rows, 1024, 256, w, 2, 0.99, seed=3, lengths=LENS, width=W, int16_scale=1e7)
    assert int(loud.max()) == 32767 and int(loud.min()) == -32768  # clamped, not wrapped
    assert torch.equal(loud, (f * 1e7).clamp(-32768, 32767).to(torch.int16))


def test_unsupported_geometry_is_an_error():
    rows, w = _packed()
    with pytest.raises(ValueError):
        hip.griffin_lim(rows[:, :385].contiguous(), 768, 192, w[:768].contiguous(), 1, lengths=LENS)
    # the entry points check the geometry before anything else (nothing is launched, no pointer is read)
    assert hip.lib().ssamd_gl_iter(None, None, None, None, 0.0, 1, None, None, 1, 768, 192, None, hip._stream()) == -2


def _preprocess():
    from speakingstyle_amd.config import normalize_preprocess_config

    return normalize_preprocess_config(None)


def test_vocoder_runs_the_kernel():
    """``GriffinLim.infer`` / ``infer_packed`` with lengths == ``hip.griffin_lim`` on the same rows, bitwise."""
    from speakingstyle_amd.models.griffinlim import GriffinLim

    stft, w, _, _, mel = _case(*CASES[-1])
    voc = GriffinLim(_preprocess(), n_iters=3, momentum=0.99, seed=4)
    x = mel.cuda()  # [2, 37, 80]
    lens = [37, 20]
    pinv = torch.linalg.pinv(stft.mel_basis).contiguous().cuda()
    rows = torch.cat([x[0, :37], x[1, :20]], 0).contiguous()
    for scale in (None, 32768.0):
        want = hip.griffin_lim(rows, 1024, 256, w.cuda(), 3, 0.99, seed=4, lengths=lens, int16_scale=scale,
                               mel_pinv=pinv, width=37 * 256)
        got = voc.infer(x, int16_scale=scale, lengths=lens)
        assert got.shape == (2, 37 * 256) and torch.equal(got, want)
        assert torch.equal(voc.infer_packed(rows, lens, int16_scale=scale), want)
        assert torch.equal(voc.infer_packed(x, lens, int16_scale=scale), want)
    assert not got[0, 36 * 256:].any() and not got[1, 19 * 256:].any() and got[1, : 19 * 256].any()
    full = voc.infer(x)
    assert full.dtype == torch.float32 and torch.equal(voc(x.transpose(1, 2)), full.unsqueeze(1))


def test_vocoder_infer_keeps_the_mel_in_fp32():
    from speakingstyle_amd.config import normalize_model_config
    from speakingstyle_amd.models.griffinlim import GriffinLim
    from speakingstyle_amd.utils.model import vocoder_infer

    _, _, _, _, mel = _case(*CASES[-1])
    pp = _preprocess()
    voc = GriffinLim(pp, n_iters=2, seed=4)
    x = mel.cuda()
    wavs = vocoder_infer(x, voc, normalize_model_config(None), pp, lengths=[37 * 256, 20 * 256 - 5], channel_last=True)
    want = voc.infer(x, int16_scale=32768.0, lengths=[37, 20]).cpu().numpy()
    assert wavs[0].dtype == np.int16 and wavs[0].shape == (37 * 256,) and wavs[1].shape == (20 * 256 - 5,)
    assert np.array_equal(wavs[0], want[0]) and np.array_equal(wavs[1], want[1, : 20 * 256 - 5])


def test_synthesizer_on_gpu_runs_eagerly():
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.infer.serve import Synthesizer
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.models.griffinlim import GriffinLim
    from speakingstyle_amd.utils.model import ROOT

    dev = torch.device("cuda", 0)
    pp, mc, tc = load_named("BC2013_GST")
    mc["transformer"]["encoder_layer"] = 2
    mc["transformer"]["decoder_layer"] = 2
    for k, v in pp["path"].items():
        if isinstance(v, str) and not os.path.isabs(v):
            pp["path"][k] = os.path.join(ROOT, v)
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc).to(dev)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(4.0))
    model.eval().set_compute_dtype(torch.bfloat16)
    model.requires_grad_(False)
    s = Synthesizer((pp, mc, tc), device=dev, model=model, vocoder=GriffinLim(pp, n_iters=4))
    wav = s.tts("Hi.")
    assert wav.dtype == np.int16 and wav.ndim == 1 and wav.size > s.hop and wav.size % s.hop == 0
    assert wav[: -s.hop].any() and not wav[-s.hop:].any()  # frames * hop samples, the last hop zero
    again = s.tts("Hi.")
    assert np.array_equal(wav, again)
    st = s.stats
    assert st["eager"] == 2 and st["captures"] == 0 and st["replays"] == 0, st
