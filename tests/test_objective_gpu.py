"""The whole objective-metrics path on the GPU: ``evaluate_objective`` on a six-utterance synthetic corpus with a tiny
model, HIP DTW kernels against the torch reference.

Every summary figure must agree within the DTW cost bound (Tx + Ty + D + 8) * 2^-23 (tests/test_dtw_gpu.py) scaled
by the metric's constant: the MCD is (10 sqrt(2) / ln 10) * cost / path length, so its bound is that relative bound
times the figure itself; the other figures depend on the DTW only through the path, which must be the same, so they
are held to the same relative bound (their own arithmetic is float64 on both sides).

Both runs synthesize with the HIP model kernels (bitwise repeatable) and differ only in the DTW: the second run
routes ``ops.dtw`` to ``ops.reference.dtw`` on the same device tensors.  Switching the whole call with
``ops.set_backend("reference")`` also swaps the model's bf16 kernels for torch ops, which moves the synthesized
mels themselves (measured on an MI355X: mean mcd_db 62.802 against 63.011, 3.3e-3 relative, with synthesized
lengths of 0-4 frames from the untrained model) -- a difference of the synthesis, not of the alignment, and far
above the DTW bound of 8e-6.  The duration head's bias is set so that the untrained model speaks about four frames
per phoneme, as the recordings do."""
import csv
import json
import math

import numpy as np
import pytest
import torch

from speakingstyle_amd import ops

pytestmark = pytest.mark.gpu


def make_corpus(tmp_path, n=6):
    pre = tmp_path / "pre"
    for k in ("mel", "pitch", "energy", "duration"):
        (pre / k).mkdir(parents=True)
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
        lines.append(f"{base}|LJ|{{{' '.join(phones)}}}|text {i}")
    (pre / "val.txt").write_text("\n".join(lines) + "\n")
    (pre / "train.txt").write_text("\n".join(lines * 3) + "\n")
    return pre


def make_configs(pre):
    """The LJSpeech model at its real widths (the HIP kernels cover those) with one layer each way."""
    from speakingstyle_amd.config import load_named

    pp, mc, tc = load_named("LJSpeech")
    pp["path"]["preprocessed_path"] = str(pre)
    mc["transformer"]["encoder_layer"] = mc["transformer"]["decoder_layer"] = 1
    return pp, mc, tc


def agree(a, b, rel, what):
    for stat in ("mean", "median"):
        for k in a[stat]:
            u, v = a[stat][k], b[stat][k]
            print(f"DTWNUM objective {what} {stat}.{k} hip={u!r} reference={v!r}")
            if math.isnan(u) or math.isnan(v):
                assert math.isnan(u) and math.isnan(v), (stat, k)
            else:
                assert abs(u - v) <= rel * max(abs(u), abs(v)), (stat, k, u, v)


def test_evaluate_objective_hip_against_reference(tmp_path, monkeypatch):
    from speakingstyle_amd.analysis import objective
    from speakingstyle_amd.ops import hip, reference as ref
    from speakingstyle_amd.utils.model import get_model

    pre = make_corpus(tmp_path)
    configs = make_configs(pre)
    dev = torch.device("cuda")
    torch.manual_seed(1234)
    model = get_model(0, configs, dev, train=False)
    with torch.no_grad():  # exp(1.6) - 1 ~ 4 frames per phoneme
        model.variance_adaptor.duration_predictor.linear_layer.bias.fill_(1.6)
    hip.bump_weight_generation()
    src = str(pre / "val.txt")
    calls = []
    hip_dtw = hip.dtw
    monkeypatch.setattr(hip, "dtw", lambda *a, **k: calls.append(1) or hip_dtw(*a, **k))
    got = objective.evaluate_objective(model, configs, src, dev, batch_size=4, out_dir=str(tmp_path / "hip"))
    assert got["n"] == 6 and got["n_empty"] == 0 and len(calls) == 2  # two batches through the kernels
    with open(tmp_path / "hip" / "objective.csv") as f:
        frames = [(int(r["pred_frames"]), int(r["true_frames"])) for r in csv.DictReader(f)]
    print(f"DTWNUM objective frames (pred, true) = {frames}")
    assert all(a >= 8 for a, _ in frames)
    rel = max(a + b + 13 + 8 for a, b in frames) * 2.0 ** -23
    monkeypatch.setattr(ops, "dtw", lambda x, y, xl, yl, plane_budget=None: ref.dtw(x, y, xl, yl))
    want = objective.evaluate_objective(model, configs, src, dev, batch_size=4)
    assert want["n"] == 6 and len(calls) == 2
    agree(got, want, rel, "dtw=reference")
