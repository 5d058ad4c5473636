"""Griffin-Lim vocoder, host side: the torch reference op (``ops.reference.griffin_lim`` / ``istft``) against the
torch.stft / torch.istft loop it is defined by, packed batches against single utterances, convergence, and the
``GriffinLim`` vocoder behind ``get_vocoder`` / ``vocoder_infer`` / ``Synthesizer``."""
import math
import os

import numpy as np
import pytest
import torch

from speakingstyle_amd import ops
from speakingstyle_amd.audio.stft import TacotronSTFT
from speakingstyle_amd.config import load_named, normalize_model_config, normalize_preprocess_config
from speakingstyle_amd.ops import reference as ref

SR = 22050


def _signal(N, B=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(N) / SR
    return (0.5 * torch.sin(2 * torch.pi * 220 * t) + 0.1 * torch.randn(B, N, generator=g)).clamp(-1, 1)


def _mag_rows(stft, T, B=1, seed=0):
    """|STFT| of the test signal as channel-last rows [B, T, NB] plus a fixed random phase of the same shape."""
    mag = stft.magnitudes(_signal(stft.hop * (T - 1), B, seed)).transpose(1, 2).contiguous()
    assert mag.shape[1] == T
    ph = 2 * math.pi * torch.rand(mag.shape, generator=torch.Generator().manual_seed(seed + 100))
    return mag, ph


def _convergence(stft, wav, mag):
    """||STFT(y)| - mag| / |mag| over one utterance (mag [T, NB])."""
    got = stft.magnitudes(wav[None].to(torch.float32))[0].t()
    return float((got - mag).norm() / mag.norm())


def test_get_vocoder_builds_griffin_lim():
    from speakingstyle_amd.models.griffinlim import GriffinLim
    from speakingstyle_amd.utils.model import get_vocoder

    mc = normalize_model_config({"vocoder": {"model": "GriffinLim", "speaker": "LJSpeech", "n_iters": 7,
                                             "momentum": 0.5}})
    voc = get_vocoder(mc, torch.device("cpu"), preprocess_config=normalize_preprocess_config(None))
    assert isinstance(voc, GriffinLim) and voc.n_iters == 7 and voc.momentum == 0.5 and not voc.packable()
    assert voc.eval() is voc and voc.to("cpu") is voc and voc.requires_grad_(False) is voc
    d = get_vocoder(normalize_model_config({"vocoder": {"model": "GriffinLim"}}), torch.device("cpu"))
    assert (d.n_iters, d.momentum, d.hop, d.n_fft) == (60, 0.99, 256, 1024)
    with pytest.raises(ValueError):
        get_vocoder(normalize_model_config({"vocoder": {"model": "MelGAN"}}), torch.device("cpu"))


def test_vocoder_infer_on_cpu_trims_by_lengths():
    from speakingstyle_amd.models.griffinlim import GriffinLim
    from speakingstyle_amd.utils.model import vocoder_infer

    pp = normalize_preprocess_config(None)
    mc = normalize_model_config(None)
    voc = GriffinLim(pp, n_iters=2)
    stft = voc.stft
    mel, _ = stft.mel_spectrogram(_signal(256 * 8, B=2))  # [2, 80, 9]
    T = mel.shape[2]
    wavs = vocoder_infer(mel, voc, mc, pp)
    assert len(wavs) == 2 and all(w.dtype == np.int16 and w.shape == (T * 256,) for w in wavs)
    assert wavs[0].any() and not wavs[0][(T - 1) * 256:].any()  # N = hop * (T - 1): the last hop is zero
    cut = vocoder_infer(mel, voc, mc, pp, lengths=[T * 256, 5 * 256 - 3])
    assert cut[0].shape == (T * 256,) and cut[1].shape == (5 * 256 - 3,)
    assert np.array_equal(cut[0], wavs[0]) and np.array_equal(cut[1], wavs[1][: 5 * 256 - 3])
    y = voc(mel)  # the generator's call convention
    assert y.shape == (2, 1, T * 256) and y.dtype == torch.float32


def test_synthesizer_with_griffin_lim_on_cpu():
    from speakingstyle_amd.infer.serve import Synthesizer
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.models.griffinlim import GriffinLim
    from speakingstyle_amd.utils.model import ROOT

    pp, mc, tc = load_named("BC2013_GST")
    mc["transformer"]["encoder_layer"] = 2
    mc["transformer"]["decoder_layer"] = 2
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(4.0))
    model.eval().requires_grad_(False)
    for k, v in pp["path"].items():
        if isinstance(v, str) and not os.path.isabs(v):
            pp["path"][k] = os.path.join(ROOT, v)
    s = Synthesizer((pp, mc, tc), device="cpu", model=model, vocoder=GriffinLim(pp, n_iters=2))
    wav = s.tts("Hi.")
    assert wav.dtype == np.int16 and wav.ndim == 1 and wav.size > 0 and wav.size % s.hop == 0
    assert wav.any() and not wav[-s.hop:].any()


@pytest.mark.parametrize("n_fft,hop,win,T", [(1024, 256, 1024, 11), (1024, 256, 800, 5), (2048, 300, 1200, 9)])
def test_reference_op_equals_the_torch_loop(n_fft, hop, win, T):
    """Given phase, momentum 0, 3 iterations: the op equals the torch.stft / torch.istft loop it replaces (the body
    of ``audio/stft.py::griffin_lim`` before it took a phase), to fp32 rounding."""
    stft = TacotronSTFT(n_fft, hop, win, 80, SR, 0.0, 8000.0)
    mag, ph = _mag_rows(stft, T, B=2)
    m, p = mag.transpose(1, 2), ph.transpose(1, 2)  # the loop's [B, NB, T]
    spec = m * torch.exp(1j * p)
    y = torch.istft(spec, n_fft, hop, win, window=stft.window)
    for _ in range(3):
        s = torch.stft(y, n_fft, hop, win, window=stft.window, return_complex=True)
        y = torch.istft(m * torch.exp(1j * torch.angle(s)), n_fft, hop, win, window=stft.window)
    got = ops.griffin_lim(mag, n_fft, hop, stft.fft_window("cpu"), 3, 0.0, init_phase=ph)
    assert got.shape == y.shape == (2, hop * (T - 1))
    assert float((got - y).abs().max()) < 2e-5 * float(y.abs().max())
    # the module-level functions kept their CPU results and gained the phase argument
    from speakingstyle_amd.audio.stft import griffin_lim

    assert torch.equal(griffin_lim(m, stft, 3, init_phase=p), y)
    # the iSTFT front alone
    w0 = ops.istft(torch.polar(mag, ph), n_fft, hop, stft.fft_window("cpu"))
    assert float((w0 - torch.istft(spec, n_fft, hop, win, window=stft.window)).abs().max()) < 1e-6


def test_packed_batch_equals_each_utterance_alone():
    """Lengths [4, 9, 37, 2, 1] at 1024 / 256, seeded phase: exact.  2 frames: the zero-iteration iSTFT; 1: empty."""
    stft = TacotronSTFT()
    lens = [4, 9, 37, 2, 1]
    mags = [_mag_rows(stft, max(n, 4), seed=i)[0][0][:n] for i, n in enumerate(lens)]
    win = stft.fft_window("cpu")
    assert ref.gl_min_frames(1024, 256) == 4
    for momentum in (0.0, 0.99):
        out = ops.griffin_lim(torch.cat(mags, 0), 1024, 256, win, 3, momentum, seed=5, lengths=lens)
        assert out.shape == (5, 256 * 36)
        padded = torch.zeros(5, 37, 513)
        for b, m in enumerate(mags):
            padded[b, : lens[b]] = m
        assert torch.equal(ops.griffin_lim(padded, 1024, 256, win, 3, momentum, seed=5, lengths=lens), out)
        for b, (n, m) in enumerate(zip(lens, mags)):
            alone = ops.griffin_lim(m, 1024, 256, win, 3, momentum, seed=5)
            assert alone.shape == (1, 256 * (n - 1))
            assert torch.equal(out[b, : alone.shape[1]], alone[0]) and not out[b, alone.shape[1]:].any()
    two = ops.istft(torch.polar(mags[3], ref.gl_seed_phase(5, 2, 513)), 1024, 256, win)
    assert torch.equal(out[3, :256], two[0]) and two.any()
    i16 = ops.griffin_lim(torch.cat(mags, 0), 1024, 256, win, 3, 0.99, seed=5, lengths=lens, int16_scale=32768.0)
    assert i16.dtype == torch.int16 and torch.equal(i16, (out * 32768.0).clamp(-32768, 32767).to(torch.int16))
    assert not torch.equal(ops.griffin_lim(mags[1], 1024, 256, win, 3, seed=6), ops.griffin_lim(mags[1], 1024, 256, win, 3, seed=5))


@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_spectral_convergence_falls(momentum):
    stft = TacotronSTFT()
    mag, ph = _mag_rows(stft, 37)
    win = stft.fft_window("cpu")
    c0 = _convergence(stft, ops.griffin_lim(mag, 1024, 256, win, 0, momentum, init_phase=ph)[0], mag[0])
    c30 = _convergence(stft, ops.griffin_lim(mag, 1024, 256, win, 30, momentum, init_phase=ph)[0], mag[0])
    assert c30 < c0 and c30 < 0.5 and c0 > 0.5, (c0, c30)


def test_mel_inversion_is_inv_mel_spec():
    """Log-mel rows with the pseudo-inverse: the magnitudes ``inv_mel_spec`` builds, and its waveform."""
    from speakingstyle_amd.audio.stft import inv_mel_spec

    stft = TacotronSTFT()
    mel, _ = stft.mel_spectrogram(_signal(256 * 10))
    pinv = torch.linalg.pinv(stft.mel_basis)
    ph = 2 * math.pi * torch.rand(513, 11, generator=torch.Generator().manual_seed(3))
    want = inv_mel_spec(mel[0], stft, 2, init_phase=ph)
    got, mag = ops.griffin_lim(mel[0].t().contiguous(), 1024, 256, stft.fft_window("cpu"), 2, 0.0,
                               init_phase=ph.t().contiguous(), mel_pinv=pinv, return_mag=True)
    ref_mag = torch.clamp(pinv @ torch.exp(mel[0]), min=0.0).t()
    assert float((mag - ref_mag).abs().max()) < 1e-5 * float(ref_mag.abs().max()) and float(mag.min()) >= 0
    assert float((got[0] - want).abs().max()) < 1e-4 * float(want.abs().max())


def test_clis_write_wavs_without_a_checkpoint(tmp_path):
    """``hifigan_inference_e2e.py --griffin_lim`` and ``synthesize.py --vocoder griffin_lim``: no HiFi-GAN weights."""
    import importlib
    import sys

    from speakingstyle_amd.audio.io import read_wav
    from speakingstyle_amd.utils.model import ROOT

    sys.path.insert(0, ROOT)
    stft = TacotronSTFT()
    mels = tmp_path / "mels"
    mels.mkdir()
    for i, n in enumerate((12, 7)):
        mel, _ = stft.mel_spectrogram(_signal(256 * n, seed=i))
        np.save(mels / f"u{i}.npy", mel[0].numpy())
    e2e = importlib.import_module("hifigan_inference_e2e")
    e2e.main(["--griffin_lim", "--input_mels_dir", str(mels), "--output_dir", str(tmp_path / "out"), "--n_iters", "3"])
    for i, n in enumerate((12, 7)):
        wav, sr = read_wav(str(tmp_path / "out" / f"u{i}_generated_e2e.wav"))
        assert sr == SR and wav.shape[-1] == (n + 1) * 256 and np.abs(wav).max() > 0
    with pytest.raises(SystemExit):
        e2e.main(["--input_mels_dir", str(mels)])  # neither a checkpoint nor --griffin_lim
    # synthesize.py: a checkpoint of a model whose duration head speaks (~4 frames per phoneme), no vocoder weights
    import yaml

    from speakingstyle_amd.config import config_dir_triplet, load_configs, load_yaml
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.utils.model import save_checkpoint

    cli = importlib.import_module("synthesize")
    p_path, m_path, t_path = config_dir_triplet("LJSpeech")
    pp, tc = load_yaml(p_path), load_yaml(t_path)
    for k, v in pp["path"].items():  # the repository's relative paths, from wherever the test runs
        if isinstance(v, str) and not os.path.isabs(v):
            pp["path"][k] = os.path.join(ROOT, v)
    tc["path"]["ckpt_path"] = str(tmp_path / "ckpt")
    files = []
    for name, cfg in (("p.yaml", pp), ("t.yaml", tc)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as f:
            yaml.safe_dump(cfg, f)
    configs = load_configs(files[0], m_path, files[1])
    torch.manual_seed(0)
    model = FastSpeech2(configs[0], configs[1])
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(4.0))
    save_checkpoint(os.path.join(tc["path"]["ckpt_path"], "1.pth.tar"), model)
    cli.main(["--mode", "single", "--text", "Hi.", "--vocoder", "griffin_lim", "--restore_step", "1",
              "-p", files[0], "-m", m_path, "-t", files[1], "--result_path", str(tmp_path / "synth")])
    out = [f for f in os.listdir(tmp_path / "synth") if f.endswith(".wav")]
    assert len(out) == 1
    wav, sr = read_wav(str(tmp_path / "synth" / out[0]))
    assert sr == SR and wav.shape[-1] > 0 and wav.shape[-1] % 256 == 0
