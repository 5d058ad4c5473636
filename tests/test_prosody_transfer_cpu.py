"""Prosody transfer on the CPU: ``ops.reference.prosody_transfer`` (float64 = the oracle of csrc/k_prosody.hip) against
constructions whose answer is known, ``data/preprocess.py``'s phoneme averages, and the second synthesis pass of
``infer/transfer.py`` on a small random-weight model."""
import functools
import math

import numpy as np
import pytest
import torch

from prosody_signals import cast, pack_case, random_utterance, recover, rendered_pair
from speakingstyle_amd.data.preprocess import interpolate_unvoiced, phoneme_average
from speakingstyle_amd.ops import reference as ref

P_STATS, E_STATS = (180.0, 45.0), (20.0, 12.0)


def _block_case(seed, n):
    """Tokens with distinct random 13-vectors, repeated src_dur times on the x side and true_dur times on the y."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 12, n)
    if not src.any():
        src[int(rng.integers(n))] = int(rng.integers(1, 12))
    true = np.where(src > 0, rng.integers(1, 12, n), 0)
    vec = rng.standard_normal((n, 13))
    return src, true, np.repeat(vec, src, 0), np.repeat(vec, true, 0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_blocks_come_back_exactly(dtype):
    cases = [_block_case(1000 + n, n) for n in range(1, 41)]
    x = torch.from_numpy(np.concatenate([c[2] for c in cases])).to(dtype)
    y = torch.from_numpy(np.concatenate([c[3] for c in cases])).to(dtype)
    xl, yl = [int(c[0].sum()) for c in cases], [int(c[1].sum()) for c in cases]
    _, path, plen = ref.dtw(x, y, xl, yl)
    dur = torch.zeros(40, 40, dtype=torch.int32)
    for p, c in enumerate(cases):
        dur[p, :len(c[0])] = torch.from_numpy(c[0]).int()
    f0 = torch.full((sum(yl),), 150.0, dtype=dtype)
    rec = ref.prosody_transfer(path, plen, dur, list(range(1, 41)), xl, yl, f0, f0.clone(), torch.zeros(40, 40, dtype=dtype),
                               pitch_mode="absolute")[0]
    assert rec.dtype == torch.int32
    for p, c in enumerate(cases):
        assert rec[p, :len(c[1])].tolist() == c[1].tolist(), p
        assert not rec[p, len(c[1]):].any()


CASES = [(1, 1), (2, 2), (7, 1), (5, 40), (40, 130), (63, 64), (64, 255), (65, 300), (129, 257)]  # (N, y_len)


@functools.lru_cache(maxsize=None)
def _random_batch(voicing="mixed"):
    utts = [random_utterance(31 * n + ty, n, ty, voicing) for n, ty in CASES]
    return utts, pack_case(utts)


def test_absolute_targets_are_the_preprocess_averages():
    utts, args = _random_batch()
    rec, pitch, en, voiced, ok = ref.prosody_transfer(*args, P_STATS, E_STATS, "absolute")
    assert pitch.dtype == torch.float64 and ok.dtype == torch.bool
    for p, u in enumerate(utts):
        n = len(u["src_dur"])
        d = rec[p, :n].numpy()
        want_p = (phoneme_average(interpolate_unvoiced(u["f0"]), list(d)) - P_STATS[0]) / P_STATS[1]
        want_e = (phoneme_average(u["energy"], list(d)) - E_STATS[0]) / E_STATS[1]
        # a token without frames is 0 in the preprocessing before the normalisation; here the target itself is 0
        want_p, want_e = np.where(d > 0, want_p, 0.0), np.where(d > 0, want_e, 0.0)
        assert np.abs(pitch[p, :n].numpy() - want_p).max() <= 1e-12
        assert np.abs(en[p, :n].numpy() - want_e).max() <= 1e-12
        want_v = phoneme_average((u["f0"] > 0).astype(np.float64), list(d))
        assert np.abs(voiced[p, :n].numpy() - want_v).max() <= 1e-12
        assert bool(ok[p]) == bool((u["f0"] > 0).any())
        assert not pitch[p, n:].any() and not en[p, n:].any() and not rec[p, n:].any()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_durations_cover_the_recording(dtype):
    utts, args = _random_batch()
    rec = ref.prosody_transfer(*cast(args, dtype), P_STATS, E_STATS, "relative")[0]
    for p, u in enumerate(utts):
        n = len(u["src_dur"])
        assert int(rec[p].sum()) == u["ty"]
        assert not rec[p, :n][torch.from_numpy(u["src_dur"] == 0)].any()
    # token(j) is non-decreasing: a long vertical run gives its one recorded frame to the run's middle token
    path = torch.tensor([[[i, 0] for i in range(9)] + [[8, 1]]], dtype=torch.int32)
    rec = ref.prosody_transfer(path, torch.tensor([10]), torch.tensor([[3, 3, 3]]), [3], [9], [2],
                               torch.tensor([100.0, 0.0], dtype=dtype), torch.ones(2, dtype=dtype),
                               torch.zeros(1, 3, dtype=dtype), pitch_mode="absolute")[0]
    assert rec.tolist() == [[0, 1, 1]]


def test_more_than_1024_tokens_is_refused():
    path = torch.zeros(1, 1, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match="1025"):
        ref.prosody_transfer(path, torch.tensor([1]), torch.ones(1, 1025, dtype=torch.int32), [1025], [1], [1],
                             torch.ones(1), torch.ones(1), torch.zeros(1, 1025))
    with pytest.raises(ValueError, match="sideways"):
        ref.prosody_transfer(path, torch.tensor([1]), torch.ones(1, 1, dtype=torch.int32), [1], [1], [1], torch.ones(1),
                             torch.ones(1), torch.zeros(1, 1), pitch_mode="sideways")


def test_one_voiced_frame_holds_and_none_keeps_the_prediction():
    for voicing in ("first", "last"):
        utts, args = _random_batch(voicing)
        rec, pitch, _, voiced, ok = ref.prosody_transfer(*args, P_STATS, E_STATS, "absolute")
        for p, u in enumerate(utts):
            hz = u["f0"][u["f0"] > 0][0]
            has = rec[p] > 0
            assert bool(ok[p])
            assert (pitch[p][has] * P_STATS[1] + P_STATS[0] - hz).abs().max() <= 1e-9  # a constant contour
            assert int((voiced[p] > 0).sum()) == 1
    utts, args = _random_batch("none")
    for mode in ("absolute", "relative"):
        out = ref.prosody_transfer(*args, P_STATS, E_STATS, mode)
        assert not out[4].any() and torch.isfinite(out[1]).all() and not out[3].any()


def test_blend_keeps_the_prediction_without_voicing():
    """``transfer_targets`` end to end on block features: durations are the recording's, the energy is transferred, and
    with no voiced frame the pitch target is the first pass's prediction."""
    from speakingstyle_amd.infer.transfer import transfer_targets

    rng = np.random.default_rng(5)
    src, true = np.asarray([3, 0, 4, 2, 5]), np.asarray([5, 0, 2, 4, 3])
    vec = rng.standard_normal((5, 20)).astype(np.float32)
    pred_p, pred_e = torch.randn(1, 5), torch.randn(1, 5)
    first = {"mel": torch.from_numpy(np.repeat(vec, src, 0)), "mel_lens": [int(src.sum())],
             "durations": torch.from_numpy(src)[None], "src_lens": torch.tensor([5]), "pitch": pred_p, "energy": pred_e}
    en = torch.from_numpy(rng.uniform(1, 30, int(true.sum())).astype(np.float32))
    feats = (torch.from_numpy(np.repeat(vec, true, 0)), en, torch.zeros(int(true.sum())), [int(true.sum())])
    stats = {"pitch": P_STATS, "energy": E_STATS}
    t = transfer_targets(first, feats, stats)
    assert t["d_targets"].tolist() == [true.tolist()] and not bool(t["pitch_ok"][0])
    assert torch.equal(t["p_targets"], pred_p)
    want_e = (torch.from_numpy(phoneme_average(en.double().numpy(), list(true))) - E_STATS[0]) / E_STATS[1]
    got = t["e_targets"][0]
    assert (got[true > 0].double() - want_e[true > 0]).abs().max() < 1e-5 and got[1] == pred_e[0, 1]
    half = transfer_targets(first, feats, stats, what=("duration",), strength=0.5, min_frames=2)
    assert half["d_targets"].tolist() == [[4, 0, 3, 3, 4]] and torch.equal(half["e_targets"], pred_e)
    feats_v = feats[:2] + (torch.full_like(feats[2], 200.0),) + feats[3:]
    voiced = transfer_targets(first, feats_v, stats, what="pitch", pitch_mode="absolute")
    assert voiced["d_targets"].tolist() == [src.tolist()]
    assert (voiced["p_targets"][0][true > 0] - (200.0 - P_STATS[0]) / P_STATS[1]).abs().max() < 1e-5
    with pytest.raises(ValueError, match="1.5"):
        transfer_targets(first, feats, stats, strength=1.5)


def test_relative_mode_carries_the_shape_to_the_predicted_level():
    utts, args = _random_batch()
    base = ref.prosody_transfer(*args, P_STATS, E_STATS, "relative", return_contour=True)
    for factor in (0.5, 1.7):
        scaled = args[:6] + (args[6] * factor,) + args[7:]
        out = ref.prosody_transfer(*scaled, P_STATS, E_STATS, "relative")
        assert torch.equal(out[0], base[0])
        assert (out[1] - base[1]).abs().max() <= 1e-9
    g = base[5]
    for p, u in enumerate(utts):
        n, ty = len(u["src_dur"]), u["ty"]
        hz = np.maximum(u["pred"] * P_STATS[1] + P_STATS[0], 1.0)
        l_pred = float((u["src_dur"] * np.log(hz)).sum() / u["src_dur"].sum())
        if (u["f0"] > 0).any():  # every recorded frame once = every token weighted by its rec_dur
            assert abs(float(torch.log(g[p, :ty]).mean()) - l_pred) <= 1e-9
    absolute = ref.prosody_transfer(*args, P_STATS, E_STATS, "absolute")
    assert not torch.allclose(absolute[1], base[1])


# ---------------------------------------------------------------------------- recovery on rendered audio
RECOVERY_SEEDS = range(100, 106)
CAP_FRAMES, CAP_PITCH, CAP_ENERGY = 2, 0.05, 0.03


def test_recovery_on_rendered_audio():
    """Measured with the float32 torch references: durations exact, token pitch within 4.4 %, energy within 2.1 % (a
    prototype of the rules: 1 frame, 3.4 %, 1.8 %); the caps leave one frame for the boundary frames (they sit in a
    glide) and the float64 run."""
    pairs = [rendered_pair(seed) for seed in RECOVERY_SEEDS]
    d_err, p_err, e_err = recover(pairs, torch.device("cpu"))
    print(f"PROSREC cpu duration {d_err:.0f} frames, pitch {100 * p_err:.2f} %, energy {100 * e_err:.2f} %")
    assert d_err <= CAP_FRAMES and p_err <= CAP_PITCH and e_err <= CAP_ENERGY


# ---------------------------------------------------------------------------- the second pass
def _small_model(config="BC2013_GST"):
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2

    pp, mc, tc = load_named(config)
    mc["transformer"]["encoder_layer"] = 2
    mc["transformer"]["decoder_layer"] = 2
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(4.0))
    model.eval().requires_grad_(False)
    return (pp, mc, tc), model


def _batch(ref_frames):
    rng = np.random.default_rng(2)
    Ts = [9, 6]
    texts = np.zeros((2, 9), dtype=np.int64)
    for i, n in enumerate(Ts):
        texts[i, :n] = rng.integers(1, 300, size=n)
    mels = rng.standard_normal((2, ref_frames, 80)).astype(np.float32)
    return (["a", "b"], ["", ""], np.zeros(2, dtype=np.int64), texts, np.asarray(Ts), 9, mels,
            np.asarray([ref_frames, ref_frames - 3]), ref_frames)


@pytest.mark.parametrize("ref_frames", [7, 200])
def test_second_pass_has_the_targets_length(ref_frames):
    """The mel length is sum(durations), whatever the length of the style reference."""
    from speakingstyle_amd.infer.transfer import synthesize_like

    configs, model = _small_model()
    rng = np.random.default_rng(3)
    frames = [61, 37]
    feats = (torch.from_numpy(rng.standard_normal((sum(frames), 80)).astype(np.float32)),
             torch.from_numpy(rng.uniform(1, 30, sum(frames)).astype(np.float32)),
             torch.from_numpy(np.where(rng.random(sum(frames)) > 0.3, rng.uniform(90, 300, sum(frames)), 0.0).astype(np.float32)),
             frames)
    out = synthesize_like(model, configs, _batch(ref_frames), features=feats,
                          stats={"pitch": P_STATS, "energy": E_STATS})
    d = out["targets"]["d_targets"]
    assert d.sum(1).tolist() == out["mel_lens"] == [m.shape[0] for m in out["mel"]]
    assert out["targets"]["rec_dur"].sum(1).tolist() == frames  # strength 1: the recording's frames, all of them
    assert out["mel_lens"] == frames
    assert all(torch.isfinite(m).all() for m in out["mel"])
    # the hazard: without mels_style_only the style reference sizes the result
    b = _batch(ref_frames)
    args = [torch.from_numpy(np.asarray(a)) for a in b[2:5]]
    plain = model(*args, 9, mels=torch.from_numpy(b[6]), mel_lens=torch.from_numpy(b[7]), max_mel_len=b[8], d_targets=d)
    assert plain[1].shape[1] == ref_frames and plain[9].tolist() == list(b[7])
    only = model(*args, 9, mels=torch.from_numpy(b[6]), mel_lens=torch.from_numpy(b[7]), max_mel_len=b[8], d_targets=d,
                 mels_style_only=True)
    assert only[9].tolist() == frames and only[1].shape[1] == max(frames)


def test_frame_level_config_is_refused():
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.infer.transfer import synthesize_like

    configs = load_named("LJSpeech_paper")
    with pytest.raises(ValueError, match="preprocessing.pitch.feature"):
        synthesize_like(None, configs, _batch(7), features=None)


def test_cli_batch_mode_with_each_utterances_own_recording(tmp_path):
    """``synthesize.py --mode batch --prosody_ref recording``: every listed utterance takes the timing of its own
    ``<raw_path>/<speaker>/<basename>.wav``; single mode takes a given wav.  Griffin-Lim, a two-layer model."""
    import os
    import sys

    import yaml
    from scipy.io import wavfile

    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.config import config_dir_triplet, load_configs, load_yaml
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.utils.model import ROOT, save_checkpoint

    sys.path.insert(0, ROOT)
    import synthesize as cli

    p_path, m_path, t_path = config_dir_triplet("LJSpeech")
    pp, mc, tc = load_yaml(p_path), load_yaml(m_path), load_yaml(t_path)
    for k, v in pp["path"].items():
        if isinstance(v, str) and not os.path.isabs(v):
            pp["path"][k] = os.path.join(ROOT, v)
    pp["path"]["raw_path"] = str(tmp_path / "raw")
    mc["transformer"]["encoder_layer"] = mc["transformer"]["decoder_layer"] = 2
    tc["path"]["ckpt_path"], tc["path"]["result_path"] = str(tmp_path / "ckpt"), str(tmp_path / "out")
    files = []
    for name, cfg in (("p.yaml", pp), ("m.yaml", mc), ("t.yaml", tc)):
        files.append(str(tmp_path / name))
        with open(files[-1], "w") as f:
            yaml.safe_dump(cfg, f)
    configs = load_configs(*files)
    torch.manual_seed(0)
    model = FastSpeech2(configs[0], configs[1])
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(4.0))
    save_checkpoint(os.path.join(tc["path"]["ckpt_path"], "1.pth.tar"), model)
    with open(os.path.join(pp["path"]["preprocessed_path"], "val.txt"), encoding="utf-8") as f:
        lines = [next(f) for _ in range(2)]
    (tmp_path / "val2.txt").write_text("".join(lines))
    os.makedirs(tmp_path / "raw" / "LJSpeech")
    frames = {}
    for k, line in enumerate(lines):
        base = line.split("|")[0]
        rec = rendered_pair(100 + k)["y"]
        frames[base] = (int(rec["dur"].sum()), len(line.split("|")[2].split()))
        write_wav(str(tmp_path / "raw" / "LJSpeech" / f"{base}.wav"), 22050, (rec["wav"] * 32767.0).astype(np.int16))
    common = ["--restore_step", "1", "-p", files[0], "-m", files[1], "-t", files[2], "--vocoder", "griffin_lim"]
    cli.main(["--mode", "batch", "--source", str(tmp_path / "val2.txt"), "--prosody_ref", "recording"] + common)
    for base, (n, phones) in frames.items():
        sr, wav = wavfile.read(os.path.join(tc["path"]["result_path"], f"{base}.wav"))
        # the recording's frames, plus one for every phoneme it gave none
        assert sr == 22050 and wav.dtype == np.int16 and n <= wav.size // 256 <= n + phones
    base, (n, _) = next(iter(frames.items()))
    cli.main(["--mode", "single", "--text", "Hello there.", "--prosody_ref", str(tmp_path / "raw" / "LJSpeech" / f"{base}.wav"),
              "--transfer", "pitch,energy", "--result_path", str(tmp_path / "single")] + common)
    cli.main(["--mode", "single", "--text", "Hello there.", "--result_path", str(tmp_path / "plain")] + common)
    a = wavfile.read(str(tmp_path / "single" / "Hello there..wav"))[1]
    b = wavfile.read(str(tmp_path / "plain" / "Hello there..wav"))[1]
    assert a.size == b.size and not np.array_equal(a, b)  # the first pass's timing, another pitch and energy
    with pytest.raises(ValueError, match="batch"):
        cli.main(["--mode", "single", "--text", "Hello there.", "--prosody_ref", "recording"] + common)
