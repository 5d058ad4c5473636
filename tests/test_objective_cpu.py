"""Objective synthesis metrics (speakingstyle_amd/analysis/objective.py) on the CPU: identity, a known time warp,
a known cepstral offset, the DCT against its formula, and the ``analyze.py objective`` command on a small synthetic
preprocessed corpus."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = {"pitch": [-2.0, 8.0, 200.0, 40.0], "energy": [-1.5, 7.0, 30.0, 20.0]}


def make_corpus(tmp_path, n=6):
    pre = tmp_path / "pre"
    for k in ("mel", "pitch", "energy", "duration"):
        (pre / k).mkdir(parents=True)
    (pre / "speakers.json").write_text(json.dumps({"LJ": 0}))
    (pre / "stats.json").write_text(json.dumps(STATS))
    rng = np.random.default_rng(1)
    lines = []
    for i in range(n):
        phones = rng.choice(["HH", "AH0", "L", "OW1", "W", "ER1", "D", "sp"], size=rng.integers(5, 12)).tolist()
        T = len(phones)
        d = rng.integers(1, 9, T)
        base = f"LJ002-{i:04d}"
        np.save(pre / "duration" / f"LJ-duration-{base}.npy", d)
        np.save(pre / "pitch" / f"LJ-pitch-{base}.npy", rng.standard_normal(T).astype(np.float32))
        np.save(pre / "energy" / f"LJ-energy-{base}.npy", rng.standard_normal(T).astype(np.float32))
        np.save(pre / "mel" / f"LJ-mel-{base}.npy", (rng.random((int(d.sum()), 80)) * 10 - 10).astype(np.float32))
        lines.append(f"{base}|LJ|{{{' '.join(phones)}}}|text {i}")
    (pre / "val.txt").write_text("\n".join(lines) + "\n")
    (pre / "train.txt").write_text("\n".join(lines * 3) + "\n")
    return pre


def make_configs(tmp_path, pre):
    from speakingstyle_amd.config import config_dir_triplet, load_yaml

    p, m, t = (load_yaml(x) for x in config_dir_triplet("BC2013"))
    p["path"]["preprocessed_path"] = str(pre)
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


def utterances(lens=(9, 31, 70), seed=0):
    """Packed log-mel rows and frame-level pitch / energy contours of a few utterances."""
    g = torch.Generator().manual_seed(seed)
    R = sum(lens)
    mel = torch.rand(R, 80, generator=g) * 10 - 10
    pitch = 200 + 40 * torch.randn(R, generator=g, dtype=torch.float64)
    energy = 30 + 20 * torch.randn(R, generator=g, dtype=torch.float64)
    return mel, pitch, energy, list(lens)


def split(t, lens):
    return list(torch.split(t, lens))


def test_identity():
    from speakingstyle_amd.analysis.objective import utterance_metrics

    mel, pitch, energy, lens = utterances()
    durs = [np.arange(1, 4)] * len(lens)
    m = utterance_metrics(mel, lens, mel.clone(), lens, pitch, pitch.clone(), energy, energy.clone(), durs, durs)
    for k in ("mcd_db", "logmel_l1", "pitch_rmse", "energy_rmse", "dur_mae_frames"):
        assert np.all(m[k] == 0.0), k
    assert np.all(m["len_ratio"] == 1.0)
    assert np.allclose(m["pitch_corr"], 1.0, atol=1e-12)
    assert m["path_len"].tolist() == lens
    for p, n in enumerate(lens):
        assert np.array_equal(m["path"][p, :n, 0], np.arange(n)) and np.array_equal(m["path"][p, :n, 1], np.arange(n))
        assert np.all(m["path"][p, n:] == -1)


def test_known_warp_gathers_through_the_path():
    from speakingstyle_amd.analysis.objective import utterance_metrics

    mel, pitch, energy, lens = utterances()
    rep = lambda t: torch.cat([u.repeat_interleave(2, 0) for u in split(t, lens)])  # noqa: E731
    lens2 = [2 * n for n in lens]
    m = utterance_metrics(rep(mel), lens2, mel, lens, rep(pitch), pitch, rep(energy), energy)
    assert np.all(m["mcd_db"] == 0.0) and np.all(m["logmel_l1"] == 0.0)
    assert m["path_len"].tolist() == lens2
    # index by index the contours differ; through the path every doubled frame meets its original
    assert np.all(m["pitch_rmse"] == 0.0) and np.all(m["energy_rmse"] == 0.0)
    assert np.all(m["len_ratio"] == 2.0)
    for p, n in enumerate(lens):
        assert np.array_equal(m["path"][p, :2 * n, 1], np.arange(2 * n) // 2)


def test_known_offset_gives_the_closed_form_mcd():
    from speakingstyle_amd.analysis.objective import MCD_SCALE, dct_matrix, mel_cepstra, utterance_metrics

    mel, _, _, lens = utterances()
    # adding delta * (DCT basis vector k) to every log-mel frame moves cepstral coefficient k by delta and no other
    # (the basis is orthonormal), so every local cost is delta, the path is the diagonal, MCD = scale * delta
    delta, k = 0.75, 4
    basis = dct_matrix(80, 13, dtype=torch.float64)[:, k - 1]
    shifted = (mel.double() + delta * basis).float()
    m = utterance_metrics(shifted, lens, mel, lens)
    assert m["path_len"].tolist() == lens
    assert np.allclose(m["mcd_db"], MCD_SCALE * delta, rtol=1e-5)
    c = mel_cepstra(shifted.double()) - mel_cepstra(mel.double())
    want = torch.zeros(13, dtype=torch.float64)
    want[k - 1] = delta
    assert torch.allclose(c, want.expand_as(c), atol=1e-5)
    assert set(m) >= {"mcd_db", "logmel_l1", "len_ratio"} and "pitch_rmse" not in m


def test_mel_cepstra_matches_the_dct_formula():
    from speakingstyle_amd.analysis.objective import mel_cepstra

    mel = utterances()[0][:11]
    N = 80
    want = np.zeros((11, 13))
    for k in range(1, 14):
        w = math.sqrt(2.0 / N) * np.cos(math.pi / N * (np.arange(N) + 0.5) * k)
        want[:, k - 1] = mel.double().numpy() @ w
    got = mel_cepstra(mel)
    assert got.dtype == torch.float32 and got.shape == (11, 13)
    assert np.abs(got.double().numpy() - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert np.abs(mel_cepstra(mel.double()).numpy() - want).max() <= 1e-12 * np.abs(want).max()


def test_pitch_corr_is_nan_for_a_constant_contour():
    from speakingstyle_amd.analysis.objective import utterance_metrics

    mel, pitch, energy, lens = utterances((12,))
    m = utterance_metrics(mel, lens, mel, lens, torch.full_like(pitch, 180.0), pitch, energy, energy)
    assert math.isnan(m["pitch_corr"][0]) and m["pitch_rmse"][0] > 0


def test_missing_ground_truth_and_empty_list_name_the_file(tmp_path):
    from speakingstyle_amd.analysis.objective import evaluate_objective
    from speakingstyle_amd.config import load_configs
    from speakingstyle_amd.utils.model import get_model

    pre = make_corpus(tmp_path, n=2)
    configs = load_configs(*make_configs(tmp_path, pre))
    torch.manual_seed(0)
    model = get_model(0, configs, torch.device("cpu"), train=False)
    gone = pre / "pitch" / "LJ-pitch-LJ002-0001.npy"
    gone.unlink()
    with pytest.raises(FileNotFoundError, match="LJ-pitch-LJ002-0001.npy"):
        evaluate_objective(model, configs, str(pre / "val.txt"), "cpu")
    empty = tmp_path / "empty.txt"
    empty.write_text("")
    with pytest.raises(ValueError, match="empty.txt"):
        evaluate_objective(model, configs, str(empty), "cpu")


def test_objective_cli(tmp_path):
    pre = make_corpus(tmp_path)
    p, m, t = make_configs(tmp_path, pre)
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out_dir = tmp_path / "obj"
    r = subprocess.run([sys.executable, "analyze.py", "objective", "-p", p, "-m", m, "-t", t, "--out_dir", str(out_dir),
                        "--batch_size", "4", "--cpu"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    summ = json.loads(r.stdout)
    on_disk = json.loads((out_dir / "objective_summary.json").read_text())
    assert on_disk["n"] == summ["n"] and on_disk["mean"]["mcd_db"] == summ["mean"]["mcd_db"]
    assert summ["n"] == 6
    for stat in ("mean", "median"):
        for k, v in summ[stat].items():
            assert math.isfinite(v) or (k == "pitch_corr" and math.isnan(v)), (stat, k, v)
        assert set(summ[stat]) == {"mcd_db", "logmel_l1", "pitch_rmse", "energy_rmse", "pitch_corr", "dur_mae_frames",
                                   "len_ratio"}
    with open(out_dir / "objective.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 6 and rows[0]["basename"] == "LJ002-0000"
