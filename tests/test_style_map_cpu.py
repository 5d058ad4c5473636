"""The style map on the CPU: the float64 torch references of exact t-SNE and k-means (``ops.reference``), which are
the oracle of csrc/k_stylemap.hip, and ``analysis/style_map.py`` with the ``analyze.py style`` command on a small
synthetic corpus."""
import csv
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

from stylemap_signals import blob_set, gaussian_blobs, grid_points, knn_purity, points, row_perplexity
from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ affinities
@pytest.mark.parametrize("n,dim,perp", [(7, 3, 2.0), (65, 1, 2.0), (65, 80, 21.0), (300, 32, 30.0)])
def test_conditional_rows_meet_the_perplexity(n, dim, perp):
    x = points(11 * n + dim, n, dim)
    pc, beta = ref.tsne_conditional(x, perp)
    h = row_perplexity(pc).log()
    assert float((h - math.log(perp)).abs().max()) <= ref.TSNE_ENTROPY_TOL * (1 + 1e-6)
    assert float(pc.diagonal().abs().max()) == 0.0
    assert torch.allclose(pc.sum(1), torch.ones(n, dtype=pc.dtype), atol=1e-12)
    assert bool((beta > 0).all())


def test_joint_p_is_symmetric_sums_to_one_and_has_a_zero_diagonal():
    x, _ = blob_set(0)
    P = ref.tsne_affinities(x, 30.0)
    assert P.dtype == torch.float64 and P.shape == (300, 300)
    assert torch.equal(P, P.t())
    assert abs(float(P.sum()) - 1.0) <= 1e-12
    assert float(P.diagonal().abs().max()) == 0.0 and float(P.min()) >= 0.0
    assert ops.tsne_affinities(x, 30.0).equal(P)  # CPU tensors take the reference


def test_affinities_survive_a_scale_where_unshifted_float32_underflows():
    # |x| ~ 30 in 32 dimensions: squared distances of several 1e4, exp(-d) is 0 in any format without the row shift
    x = points(5, 100, 32, scale=30.0)
    p64 = ref.tsne_affinities(x, 10.0)
    p32 = ref.tsne_affinities(x.float(), 10.0)
    assert torch.isfinite(p32).all() and abs(float(p32.sum()) - 1.0) < 1e-5
    assert float((p32.double() - p64).abs().max()) <= 1e-4 * float(p64.max())


def test_duplicated_points():
    x = points(6, 40, 8)
    x = torch.cat([x, x[:24]])
    P = ref.tsne_affinities(x, 5.0)
    assert torch.isfinite(P).all() and torch.equal(P, P.t()) and abs(float(P.sum()) - 1.0) <= 1e-12


@pytest.mark.parametrize("n,perp,word", [(6, 2.0, "N = 6"), (30, 1.5, "perplexity"), (30, 10.0, "perplexity"),
                                         (ref.TSNE_MAX_N + 1, 30.0, "TSNE_MAX_N")])
def test_affinity_limits(n, perp, word):
    with pytest.raises(ValueError, match=word):
        ref.tsne_affinities(torch.zeros(n, 2, dtype=torch.float64), perp)
    with pytest.raises(ValueError, match=word):
        ops.tsne(torch.zeros(n, 2, dtype=torch.float64), perp)


def test_against_scikit_learn_internals():
    """An extra: acceptance rests on the float64 reference.  scikit-learn bisects on float32 distances without the row
    shift, to the same 1e-5 entropy tolerance: P agrees to 1e-4 of its maximum, gradient and KL (same P) to rounding."""
    pytest.importorskip("sklearn")
    from scipy.spatial.distance import pdist, squareform
    from sklearn.manifold import _t_sne

    x, _ = blob_set(0)
    P = ref.tsne_affinities(x, 30.0)
    sk = squareform(_t_sne._joint_probabilities(squareform(pdist(x.numpy(), "sqeuclidean")), 30.0, 0))
    assert float(np.abs(sk - P.numpy()).max()) <= 1e-4 * float(P.max())
    y = points(3, 300, 2)
    kl, grad = _t_sne._kl_divergence(y.numpy().ravel(), squareform(P.numpy(), checks=False), 1.0, 300, 2)
    assert abs(kl - float(ref.tsne_kl(P, y))) <= 1e-11
    assert float(np.abs(grad.reshape(300, 2) - ref.tsne_gradient(P, y, 1.0)[3].numpy()).max()) <= 1e-14


# ------------------------------------------------------------------ gradient, KL, step
@pytest.mark.parametrize("scale", [1e-4, 1.0, 10.0])
def test_analytic_gradient_is_autograd_of_the_kl(scale):
    x = points(2, 63, 8)
    P = ref.tsne_affinities(x, 10.0)
    y = (points(4, 63, 2) * scale).requires_grad_(True)
    (auto,) = torch.autograd.grad(ref.tsne_kl(P, y), y)
    attr, rep, zrow, grad = ref.tsne_gradient(P, y.detach(), 1.0)
    assert float((grad - auto).abs().max()) <= 1e-12 * max(1.0, float(auto.abs().max()))
    g12 = ref.tsne_gradient(P, y.detach(), 12.0)[3]
    assert torch.allclose(g12, 4.0 * (12.0 * attr - rep / zrow.sum()), rtol=0, atol=1e-15)


def test_step_gains_rule():
    grad = torch.tensor([[1.0, -1.0], [1.0, -1.0]], dtype=torch.float64)
    upd = torch.tensor([[1.0, 1.0], [-1.0, 0.0]], dtype=torch.float64)
    gains = torch.tensor([[1.0, 1.0], [0.0125, 1.0]], dtype=torch.float64)
    y, u, g = ref.tsne_step(grad, torch.zeros(2, 2, dtype=torch.float64), upd, gains, 0.5, 10.0)
    assert g.flatten().tolist() == pytest.approx([0.8, 1.2, 0.2125, 0.8], rel=1e-15)  # same sign x 0.8, opposite + 0.2, zero product x 0.8
    assert torch.equal(u, 0.5 * upd - 10.0 * (g * grad)) and torch.equal(y, u)
    assert float(ref.tsne_step(grad, y, upd, gains * 0.001, 0.5, 10.0)[2].min()) == 0.01


@functools.lru_cache(maxsize=None)
def blob_runs():
    """The blob set at perplexity 30, 500 iterations, 250 exaggerated: float64, float32 and float64 from a start
    perturbed by 1e-9 -> [(y, trace)]."""
    x, labels = blob_set(0)
    y0 = ref.tsne_init(x, "pca")
    g = torch.Generator().manual_seed(1)
    jog = y0 + 1e-9 * torch.randn(y0.shape, generator=g, dtype=torch.float64)
    kw = dict(perplexity=30.0, n_iter=500, exag_iter=250, kl_every=50)
    return labels, [ref.tsne(x, **kw), ref.tsne(x.float(), **kw), ref.tsne(x, init=jog, **kw)]


def test_tsne_separates_the_blobs():
    labels, runs = blob_runs()
    for (y, trace), dt in zip(runs, (torch.float64, torch.float32, torch.float64)):
        assert y.dtype == dt and y.shape == (300, 2) and len(trace) == 10
        after = trace[4:]  # 250 updates onwards: no exaggeration
        print("TSNEREF purity", knn_purity(y, labels), "trace", [round(v, 4) for v in trace])
        assert all(b <= a for a, b in zip(after, after[1:]))
        assert knn_purity(y, labels) >= 0.99
        assert trace[-1] == pytest.approx(float(ref.tsne_kl(ref.tsne_affinities(blob_set(0)[0].to(dt), 30.0), y)),
                                          rel=1e-5)


def test_tsne_inits():
    x, _ = blob_set(1)
    y = ref.tsne_init(x, "pca")
    assert float(y[:, 0].std()) == pytest.approx(1e-4, rel=1e-9) and float(y[:, 1].std()) <= 1e-4
    assert torch.equal(ref.tsne_init(x, "pca"), y) and ref.tsne_init(x.float(), "pca").dtype == torch.float32
    # the sign rule sits on the eigenvectors: mirrored data gives the mirrored map, not the same one
    assert torch.allclose(ref.tsne_init(-x, "pca"), -y, rtol=1e-9, atol=1e-15)
    r = ref.tsne_init(x, "random", seed=3)
    assert torch.equal(r, ref.tsne_init(x, "random", seed=3)) and not torch.equal(r, ref.tsne_init(x, "random", seed=4))
    assert 0.5e-4 < float(r.std()) < 2e-4
    with pytest.raises(ValueError, match="init"):
        ref.tsne_init(x, "spectral")
    with pytest.raises(ValueError, match="init"):
        ref.tsne_init(x, torch.zeros(5, 2))
    assert ref.tsne_plan(120, 50, 12.0, 50)[1] == [50, 100, 120]
    assert ref.tsne_learning_rate(13100) == pytest.approx(13100 / 48) and ref.tsne_learning_rate(300) == 50.0


# ------------------------------------------------------------------ k-means
def test_kmeans_recovers_the_blobs():
    x, truth = gaussian_blobs(3, 6, 50, 32)
    for dt in (torch.float64, torch.float32):
        labels, cent, its = ref.kmeans(x.to(dt), 6)
        assert labels.dtype == torch.int32 and cent.dtype == dt and cent.shape == (6, 32) and 1 <= its < 100
        owners = [set(labels[truth == b].tolist()) for b in range(6)]
        assert all(len(o) == 1 for o in owners) and len(set.union(*owners)) == 6
        for c in range(6):
            assert torch.allclose(cent[c], x.to(dt)[labels == c].mean(0), atol=1e-5)
    assert ops.kmeans(x, 6)[0].equal(ref.kmeans(x, 6)[0])


def test_kmeans_start_ties_and_empty_clusters():
    # 4 distinct points, each twice: the farthest-point start takes the lowest index of every tie
    x = torch.tensor([[0.0], [0.0], [4.0], [4.0], [1.0], [1.0], [3.0], [3.0]], dtype=torch.float64)
    labels, cent, its = ref.kmeans(x, 2, seed=8)  # seed % N = 0
    assert cent[:, 0].tolist() == [0.5, 3.5] and labels.tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    # the point in the middle is equally far from both centroids: the lower index wins
    mid = torch.tensor([[0.0], [2.0], [1.0]], dtype=torch.float64)
    assert ref.kmeans(mid, 2, n_iter=1)[0].tolist() == [0, 1, 0]
    # k = 3 on two distinct values: the third centre duplicates one (index 0 on the all-zero tie), gets no point
    # (ties go to the lower index) and keeps its centroid
    two = torch.tensor([[0.0], [0.0], [5.0], [5.0]], dtype=torch.float64)
    labels, cent, its = ref.kmeans(two, 3)
    assert labels.tolist() == [0, 0, 1, 1] and cent[:, 0].tolist() == [0.0, 5.0, 0.0] and its == 2
    assert ref.kmeans(x, 1)[1][0, 0] == 2.0


def test_kmeans_stops():
    x = grid_points(2, 200, 5)
    full = ref.kmeans(x, 7)
    assert full[2] < 100
    one = ref.kmeans(x, 7, n_iter=1)
    assert one[2] == 1 and not torch.equal(one[1], full[1])
    again = ref.kmeans(x, 7, n_iter=full[2])  # the iteration that changes nothing is the last one counted
    assert again[2] == full[2] and torch.equal(again[0], full[0]) and torch.equal(again[1], full[1])


@pytest.mark.parametrize("shape,k,word", [((10, 4), 0, "k = 0"), ((10, 4), 65, "k = 65"), ((10, 4), 11, "exceeds N"),
                                          ((10, 513), 2, "D = 513"), ((10,), 2, r"\[N, D\]")])
def test_kmeans_limits(shape, k, word):
    with pytest.raises(ValueError, match=word):
        ref.kmeans(torch.zeros(*shape, dtype=torch.float64), k)
    with pytest.raises(ValueError, match=word):
        ops.kmeans(torch.zeros(*shape, dtype=torch.float64), k)


# ------------------------------------------------------------------ analysis/style_map.py, analyze.py style
N_UTTS = 24


def make_corpus(tmp_path):
    pre = tmp_path / "pre"
    (pre / "mel").mkdir(parents=True)
    (pre / "speakers.json").write_text(json.dumps({"LJ": 0}))
    (pre / "stats.json").write_text(json.dumps({"pitch": [-2.0, 8.0, 200.0, 40.0], "energy": [-1.5, 7.0, 30.0, 20.0]}))
    rng = np.random.default_rng(1)
    lines = []
    for i in range(N_UTTS):
        base = f"LJ003-{i:04d}"
        mel = rng.random((int(rng.integers(20, 60)), 80)) * 4 - 8 + (i % 3) * 2.0
        np.save(pre / "mel" / f"LJ-mel-{base}.npy", mel.astype(np.float32))
        lines.append(f"{base}|LJ|{{HH AH0 L OW1}}|text {i}")
    (pre / "train.txt").write_text("\n".join(lines) + "\n")
    return pre


def make_configs(tmp_path, pre, style):
    from speakingstyle_amd.config import config_dir_triplet, load_yaml

    p, m, t = (load_yaml(x) for x in config_dir_triplet("BC2013"))
    p["path"]["preprocessed_path"] = str(pre)
    m["transformer"].update(encoder_layer=1, decoder_layer=1, conv_filter_size=64, encoder_hidden=32,
                            decoder_hidden=32, encoder_head=2, decoder_head=2)
    m["variance_predictor"]["filter_size"] = 32
    m["multi_speaker"] = False
    if style == "gst":
        m["reference_encoder"] = None
        m["gst"] = {"use_gst": True, "conv_filters": [4, 4, 8, 8, 16, 16], "gru_hidden": 16, "token_size": 16,
                    "n_style_token": 4, "attn_head": 2}
    elif style == "film":
        m["reference_encoder"].update(encoder_layer=1, encoder_head=2, encoder_hidden=32, conv_layer=1,
                                      conv_filter_size=32)
    else:
        m["reference_encoder"] = None
    for k in ("ckpt_path", "log_path", "result_path"):
        t["path"][k] = str(tmp_path / k)
    paths = []
    for nm, obj in (("preprocess", p), ("model", m), ("train", t)):
        f = tmp_path / f"{nm}.yaml"
        f.write_text(yaml.safe_dump(obj))
        paths.append(str(f))
    return paths


def load_model(paths):
    from speakingstyle_amd.config import load_configs
    from speakingstyle_amd.utils.model import get_model

    configs = load_configs(*paths)
    torch.manual_seed(7)
    return get_model(0, configs, torch.device("cpu"), train=False), configs


@pytest.mark.parametrize("style", ["gst", "film"])
def test_style_map_end_to_end(tmp_path, style):
    from speakingstyle_amd.analysis.style_map import style_map
    from speakingstyle_amd.train.style_tuning import parse_annotations

    pre = make_corpus(tmp_path)
    model, configs = load_model(make_configs(tmp_path, pre, style))
    out = tmp_path / "map"
    rep = style_map(model, configs, str(pre / "train.txt"), torch.device("cpu"), str(out), clusters=3, iters=60, seed=0)
    tokens = 4 if style == "gst" else 0
    assert rep["N"] == N_UTTS + tokens and rep["utterances"] == N_UTTS and rep["tokens"] == tokens
    assert rep["perplexity"] == pytest.approx((rep["N"] - 1) / 3) and rep["space"] == "film" and rep["dim"] == 64
    assert sum(rep["cluster_sizes"]) == N_UTTS and len(rep["exemplars"]) == 3
    assert math.isfinite(rep["final_kl"]) and rep["final_kl"] == rep["kl_trace"][-1]
    assert json.load(open(out / "style_map.json"))["N"] == rep["N"]
    rows = list(csv.DictReader(open(out / "style_map.csv")))
    assert len(rows) == N_UTTS + tokens
    assert [r["kind"] for r in rows].count("token") == tokens
    assert all(math.isfinite(float(r["x"])) and math.isfinite(float(r["y"])) and 0 <= int(r["cluster"]) < 3
               for r in rows)
    assert rep["png"] == (out / "style_map.png").exists()
    draft = out / "annotations_draft.txt"
    assert draft.exists() == (style == "gst") == rep["annotations_draft"]
    if style == "gst":
        assert all(r["top_token"] != "" for r in rows)
        names, mels, targets = parse_annotations(str(draft), str(pre), 4)
        assert len(names) == sum(len(e) for e in rep["exemplars"]) and targets.shape == (len(names), 4)
        assert mels[0].shape[1] == 80
        for space, dim in (("query", 16), ("weights", 4)):
            r2 = style_map(model, configs, str(pre / "train.txt"), torch.device("cpu"), str(tmp_path / space),
                           space=space, clusters=2, iters=20)
            assert r2["N"] == N_UTTS and r2["dim"] == dim and r2["tokens"] == 0
        sub = style_map(model, configs, str(pre / "train.txt"), torch.device("cpu"), str(tmp_path / "sub"), clusters=2,
                        iters=20, max_utts=16)
        assert sub["N"] == 16 and sub["utterances"] == 12 and sub["subsampled_from"] == N_UTTS and "note" in sub
    else:
        with pytest.raises(ValueError, match="use_gst"):
            style_map(model, configs, str(pre / "train.txt"), torch.device("cpu"), str(out), space="weights")


def test_style_map_needs_a_style_encoder(tmp_path):
    from speakingstyle_amd.analysis.style_map import embed_corpus

    pre = make_corpus(tmp_path)
    model, configs = load_model(make_configs(tmp_path, pre, None))
    with pytest.raises(ValueError, match="reference_encoder"):
        embed_corpus(model, configs, str(pre / "train.txt"), torch.device("cpu"))


def test_analyze_style_command(tmp_path):
    pre = make_corpus(tmp_path)
    p, m, t = make_configs(tmp_path, pre, "gst")
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    out = tmp_path / "cli"
    r = subprocess.run([sys.executable, "analyze.py", "style", "--restore_step", "0", "-p", p, "-m", m, "-t", t, "--cpu",
                        "--out_dir", str(out), "--iters", "40", "--perplexity", "30"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rep = json.loads(r.stdout[r.stdout.index("{"):])
    assert rep["N"] == N_UTTS + 4 and rep["clusters"] == 4 and rep["perplexity"] == pytest.approx(9.0)
    assert (out / "style_map.csv").exists() and (out / "annotations_draft.txt").exists()
