"""The YIN pitch tracker (``ops.yin`` / ``ops.reference.yin``) and the waveform-level prosody metrics
(speakingstyle_amd/analysis/objective.py) on the CPU: the float64 reference against ``data.preprocess.yin_f0``, steady
tones against their true frequency, silent / constant / zero-headed input, the argument errors, VDE / GPE / FFE /
cents against their closed forms, and ``analyze.py objective --wave`` on a small synthetic corpus with recordings."""
import csv
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from pitch_signals import short, speechlike, tone, zero_headed

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))


@pytest.mark.parametrize("n", [513, 1024, 1786])
def test_float64_reference_is_yin_f0_on_zero_free_signals(n):
    from speakingstyle_amd.data.preprocess import yin_f0

    x = short(n, n)
    want = yin_f0(x, 22050, 256)
    got, frames = ref.yin(t64(x), [n], 22050, 256)
    assert frames == [1 + n // 256] and got.dtype == torch.float64 and got.shape == want.shape
    got = got.numpy()
    assert np.array_equal(got > 0, want > 0)
    v = want > 0
    assert v.any() or n == 513  # three frames around a reflection: none is periodic
    assert np.all(np.abs(got[v] / want[v] - 1) <= 1e-9)


def test_packed_batch_is_the_utterances_one_by_one():
    xs = [short(1, 1786), short(2, 513), short(3, 1024)]
    lens = [len(x) for x in xs]
    f0, frames, cm = ops.yin(torch.from_numpy(np.concatenate(xs)).float(), lens, 22050, 256, return_cmnd=True)
    assert f0.dtype == torch.float32 and frames == [1 + n // 256 for n in lens]
    assert cm.shape == (sum(frames), 311 + 1) and torch.all(cm[:, 0] == 1)
    at = 0
    for x, T in zip(xs, frames):
        one, _, cm1 = ops.yin(torch.from_numpy(x).float(), [len(x)], 22050, 256, return_cmnd=True)
        assert torch.equal(f0[at:at + T], one) and torch.equal(cm[at:at + T], cm1)
        at += T


@pytest.mark.parametrize("sr,hop,f", [(22050, 256, 97.3), (22050, 256, 220.0), (22050, 256, 523.25), (16000, 200, 150.0)])
def test_steady_tones(sr, hop, f):
    x = tone(f, sr // 2, sr)
    for dtype in (torch.float64, torch.float32):
        f0, _ = ops.yin(torch.from_numpy(x).to(dtype), [len(x)], sr, hop)
        inner = f0[3:-3].double().numpy()
        assert inner.size > 10 and np.all(inner > 0)
        assert np.abs(inner / f - 1).max() <= 1e-3, (dtype, np.abs(inner / f - 1).max())


def test_silence_constant_and_zero_headed_frames_are_unvoiced():
    for x in (np.zeros(3000), np.full(3000, 0.25)):
        for dtype in (torch.float64, torch.float32):
            f0, _, cm = ops.yin(torch.from_numpy(x).to(dtype), [3000], 22050, 256, return_cmnd=True)
            assert torch.all(f0 == 0) and torch.isfinite(cm).all()
    x = zero_headed()
    for dtype in (torch.float64, torch.float32):
        f0, _, cm = ops.yin(torch.from_numpy(x).to(dtype), [len(x)], 22050, 256, return_cmnd=True)
        assert torch.isfinite(f0).all() and torch.isfinite(cm).all()
        # frame t holds the samples 256 t - 512 .. 256 t + 511 and the zeros end at sample 2205: frames 0 .. 6 are
        # all zero; in frames 7 and 8 every difference of the lags 1 .. 311 / 1 .. 157 lies inside the zeros, so the
        # running sum is exactly 0 there and cmnd is 1 (data.preprocess.yin_f0 answers 755 Hz and 524 Hz)
        assert torch.all(f0[:9] == 0) and torch.all(cm[:8] == 1) and torch.all(cm[8, :158] == 1)
        assert torch.any(cm[8, 158:] != 1) and (f0 > 0).any()


def test_value_errors():
    x = torch.zeros(4000)
    for kw, word in ((dict(frame=1000), "1000"), (dict(hop=0), "hop 0"), (dict(hop=1025), "1025"),
                     (dict(frame=512, hop=513), "513")):
        args = dict(sr=22050, hop=256)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.yin(x, [4000], **args)
    with pytest.raises(ValueError, match="512 samples"):
        ops.yin(torch.zeros(3512), [3000, 512], 22050, 256)
    with pytest.raises(ValueError, match="1024 samples"):
        ops.yin(torch.zeros(1024), [1024], 22050, 256, frame=2048)
    with pytest.raises(ValueError, match="3999"):
        ops.yin(x, [3999], 22050, 256)
    f0, frames = ops.yin(torch.zeros(513), [513], 22050, 256)  # the shortest utterance that is accepted
    assert frames == [3] and f0.shape == (3,)


def test_prosody_errors_closed_forms():
    from speakingstyle_amd.analysis.objective import prosody_errors

    #          both ok  gross(+25%)  a only  b only  neither  both ok(-10%)  gross(-30%)   pad
    fa = [[100.0, 250.0, 120.0, 0.0, 0.0, 180.0, 70.0, 999.0]]
    fb = [[100.0, 200.0, 0.0, 130.0, 0.0, 200.0, 100.0, 0.0]]
    mask = torch.tensor([[True] * 7 + [False]])
    e = prosody_errors(torch.tensor(fa), torch.tensor(fb), mask)
    assert float(e["vde"][0]) == 2 / 7
    assert float(e["gpe"][0]) == 2 / 4
    assert float(e["ffe"][0]) == 4 / 7
    cents = [0.0, 1200 * math.log2(1.25), 1200 * math.log2(0.9), 1200 * math.log2(0.7)]
    assert abs(float(e["f0_rmse_cents"][0]) - math.sqrt(sum(c * c for c in cents) / 4)) <= 1e-9
    # exactly 20 % off is not gross; no cell voiced on both sides: gpe and cents are nan, ffe is vde
    e = prosody_errors(torch.tensor([[120.0, 80.0]], dtype=torch.float64),
                       torch.tensor([[100.0, 100.0]], dtype=torch.float64), torch.ones(1, 2, dtype=torch.bool))
    assert float(e["gpe"][0]) == 0.0 and float(e["ffe"][0]) == 0.0
    e = prosody_errors(torch.tensor([[120.0, 0.0]]), torch.tensor([[0.0, 0.0]]), torch.ones(1, 2, dtype=torch.bool))
    assert float(e["vde"][0]) == 0.5 and float(e["ffe"][0]) == 0.5
    assert math.isnan(float(e["gpe"][0])) and math.isnan(float(e["f0_rmse_cents"][0]))


def test_wave_metrics_identity_path():
    """A batch against itself: the path is the diagonal, so the figures are those of the F0 tracks index by index."""
    from speakingstyle_amd.analysis.objective import WAVE_METRICS, wave_metrics
    from speakingstyle_amd.config import load_named

    pp = load_named("LJSpeech")[0]
    xs = [speechlike(5, 9000, 22050), short(6, 1786), short(7, 4000)]
    lens = [len(x) for x in xs]
    wav = torch.from_numpy(np.concatenate(xs)).float()
    m = wave_metrics(wav, lens, wav.clone(), lens, pp)
    assert set(WAVE_METRICS) <= set(m)
    assert m["path_len"].tolist() == [1 + n // 256 for n in lens]
    for k in WAVE_METRICS:
        assert m[k].shape == (3,) and np.all(m[k] == 0.0), (k, m[k])


def make_corpus(tmp_path, n=4, sr=22050):
    from speakingstyle_amd.audio.io import write_wav

    pre, raw = tmp_path / "pre", tmp_path / "raw"
    for k in ("mel", "pitch", "energy", "duration"):
        (pre / k).mkdir(parents=True)
    (raw / "LJ").mkdir(parents=True)
    (pre / "speakers.json").write_text(json.dumps({"LJ": 0}))
    (pre / "stats.json").write_text(json.dumps({"pitch": [-2.0, 8.0, 200.0, 40.0], "energy": [-1.5, 7.0, 30.0, 20.0]}))
    rng = np.random.default_rng(1)
    lines = []
    for i in range(n):
        phones = rng.choice(["HH", "AH0", "L", "OW1", "W", "ER1", "D", "sp"], size=rng.integers(5, 12)).tolist()
        d = rng.integers(1, 9, len(phones))
        base = f"LJ002-{i:04d}"
        np.save(pre / "duration" / f"LJ-duration-{base}.npy", d)
        np.save(pre / "pitch" / f"LJ-pitch-{base}.npy", rng.standard_normal(len(phones)).astype(np.float32))
        np.save(pre / "energy" / f"LJ-energy-{base}.npy", rng.standard_normal(len(phones)).astype(np.float32))
        np.save(pre / "mel" / f"LJ-mel-{base}.npy", (rng.random((int(d.sum()), 80)) * 10 - 10).astype(np.float32))
        write_wav(str(raw / "LJ" / f"{base}.wav"), sr, (speechlike(10 + i, 256 * int(d.sum()), sr) * 32767).astype(np.int16))
        lines.append(f"{base}|LJ|{{{' '.join(phones)}}}|text {i}")
    (pre / "val.txt").write_text("\n".join(lines) + "\n")
    (pre / "train.txt").write_text("\n".join(lines * 3) + "\n")
    return pre, raw


def make_configs(tmp_path, pre, raw):
    from speakingstyle_amd.config import config_dir_triplet, load_yaml

    p, m, t = (load_yaml(x) for x in config_dir_triplet("BC2013"))
    p["path"]["preprocessed_path"] = str(pre)
    p["path"]["raw_path"] = str(raw)
    m["transformer"].update(encoder_layer=1, decoder_layer=1, conv_filter_size=64, encoder_hidden=32,
                            decoder_hidden=32, encoder_head=2, decoder_head=2)
    m["variance_predictor"]["filter_size"] = 32
    m["reference_encoder"].update(encoder_layer=1, encoder_head=2, encoder_hidden=32, conv_layer=1,
                                  conv_filter_size=32)
    m["multi_speaker"] = False
    t["optimizer"]["batch_size"] = 2
    paths = []
    for nm, obj in (("preprocess", p), ("model", m), ("train", t)):
        f = tmp_path / f"{nm}.yaml"
        f.write_text(yaml.safe_dump(obj))
        paths.append(str(f))
    return paths


OLD_HEADER = ["basename", "pred_frames", "true_frames", "mcd_db", "logmel_l1", "pitch_rmse", "energy_rmse", "pitch_corr",
              "dur_mae_frames", "len_ratio", "path_len"]


def test_objective_cli_wave(tmp_path):
    from speakingstyle_amd.analysis.objective import METRICS, WAVE_METRICS

    pre, raw = make_corpus(tmp_path)
    p, m, t = make_configs(tmp_path, pre, raw)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    base = [sys.executable, "analyze.py", "objective", "-p", p, "-m", m, "-t", t, "--batch_size", "4", "--cpu"]
    r = subprocess.run(base + ["--out_dir", str(tmp_path / "wave"), "--wave", "--vocoder", "griffin_lim"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    summ = json.loads(r.stdout)
    assert summ["n"] == 4
    for stat in ("mean", "median"):
        assert list(summ[stat]) == list(METRICS + WAVE_METRICS)
    with open(tmp_path / "wave" / "objective.csv") as f:
        rd = csv.DictReader(f)
        rows = list(rd)
        assert rd.fieldnames == OLD_HEADER + list(WAVE_METRICS)
    assert len(rows) == 4
    for row in rows:
        if int(row["pred_frames"]) >= 4:  # long enough for the pitch tracker's frame
            assert math.isfinite(float(row["wave_mcd_db"])) and 0.0 <= float(row["wave_vde"]) <= 1.0
            assert float(row["wave_vde"]) <= float(row["wave_ffe"]) <= 1.0
    assert any(int(row["pred_frames"]) >= 4 for row in rows)
    r = subprocess.run(base + ["--out_dir", str(tmp_path / "plain")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(tmp_path / "plain" / "objective.csv") as f:
        assert f.readline().strip().split(",") == OLD_HEADER
    assert list(json.loads(r.stdout)["mean"]) == list(METRICS)


def test_missing_recording_names_the_file(tmp_path):
    from speakingstyle_amd.analysis.objective import evaluate_objective
    from speakingstyle_amd.config import load_configs
    from speakingstyle_amd.utils.model import get_model

    pre, raw = make_corpus(tmp_path, n=2)
    configs = load_configs(*make_configs(tmp_path, pre, raw))
    torch.manual_seed(0)
    model = get_model(0, configs, torch.device("cpu"), train=False)
    (raw / "LJ" / "LJ002-0001.wav").unlink()
    ran = []
    model.register_forward_pre_hook(lambda *a: ran.append(1))
    with pytest.raises(FileNotFoundError, match="LJ002-0001.wav"):
        evaluate_objective(model, configs, str(pre / "val.txt"), "cpu", wave=True, vocoder="griffin_lim")
    assert not ran  # raised before the model ran
