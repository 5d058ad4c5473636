"""Style map: where a corpus's utterances (and a GST model's tokens) lie in the style space.

The frozen style encoder embeds every utterance of a metadata list; the columns are standardised; ``ops.kmeans``
clusters the utterances and ``ops.tsne`` lays them out in the plane (exact t-SNE: on the GPU the kernels of
``csrc/k_stylemap.hip``, on the CPU the torch references).  The outputs tell a researcher which utterances to
annotate for ``tune_style.py`` and with which label:

  style_map.csv          basename, speaker, kind (utt | token), x, y, cluster, distance to the centroid, top token
  style_map.json         N, space, the perplexity used, KL trace, cluster sizes, the 5 utterances nearest each centroid,
                         the neighbours of ``--like``
  style_map.png          scatter coloured by cluster, tokens marked
  annotations_draft.txt  (GST, clusters <= n_style_token) each cluster's exemplars as ``basename|speaker|cluster``:
                         to be corrected by a person, then read by ``train.style_tuning.parse_annotations``

Spaces: ``film`` (gamma || beta of ``model.compute_style``; any style encoder), ``query`` (``w_query`` of the GST
reference embedding) and ``weights`` (head-averaged token attention weights), the last two for GST only.
"""
from __future__ import annotations

import csv
import json
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..ops import reference as ref
from ..utils.tools import pad_2d

SPACES = ("film", "query", "weights")
EXEMPLARS = 5


def read_metadata(source: str):
    """``basename|speaker|...`` lines -> [(basename, speaker)]."""
    rows = []
    with open(source, encoding="utf-8") as f:
        for line in f:
            parts = line.strip().split("|")
            if len(parts) >= 2 and parts[0]:
                rows.append((parts[0], parts[1]))
    if not rows:
        raise ValueError(f"{source}: no utterances")
    return rows


def _check_space(model, space):
    if space not in SPACES:
        raise ValueError(f"space must be one of {SPACES}, got {space!r}")
    if model.style_encoder() is None:
        raise ValueError("the style map needs a style encoder: set `reference_encoder:` or `gst: use_gst: true` in "
                         "model.yaml")
    if space != "film" and getattr(model, "gst", None) is None:
        raise ValueError(f"space {space!r} exists for GST models only (model.yaml `gst: use_gst: true`)")


@torch.no_grad()
def embed_mels(model, mels: Sequence[np.ndarray], device, space="film", batch_size=32):
    """Style embeddings of mels ([T, n_mel] each) by the frozen encoder in eval mode -> (X [M, E] fp32 on ``device``,
    top token per row as an int64 tensor, or None without GST)."""
    _check_space(model, space)
    enc, gst = model.style_encoder(), getattr(model, "gst", None)
    was = enc.training
    enc.eval()
    cd = model.compute_dtype
    out, tops = [], []
    try:
        for i in range(0, len(mels), batch_size):
            chunk = list(mels[i:i + batch_size])
            lens = torch.tensor([m.shape[0] for m in chunk], device=device)
            x = torch.from_numpy(pad_2d(chunk)).to(device, cd)
            if gst is None:
                g, b = model.compute_style(x, lens, x.shape[1], len(chunk), device)
                out.append(torch.cat([g.float(), b.float()], 1))
                continue
            q = ops.linear(gst.reference_embedding(x, lens).to(cd), gst.w_query.weight, None)
            style, w = gst.token_attention(q)
            w = w.float().mean(1)
            tops.append(w.argmax(1))
            if space == "film":
                g, b = gst._film(style.to(cd))
                out.append(torch.cat([g.float(), b.float()], 1))
            else:
                out.append(q.float() if space == "query" else w)
    finally:
        enc.train(was)
    return torch.cat(out), (torch.cat(tops) if tops else None)


@torch.no_grad()
def embed_corpus(model, configs, source, device, space="film", batch_size=32):
    """Every utterance of the metadata list ``source`` (``{preprocessed_path}/mel/{speaker}-mel-{basename}.npy``, the
    files ``parse_annotations`` reads) -> dict(names, speakers, kinds, X [M, E], top_token).  For a GST model in the
    ``film`` space the pure-token styles follow the utterances as rows of kind ``token``."""
    _check_space(model, space)
    pre = configs[0]["path"]["preprocessed_path"]
    meta = read_metadata(source)
    mels = [np.load(os.path.join(pre, "mel", f"{spk}-mel-{base}.npy")).astype(np.float32) for base, spk in meta]
    X, top = embed_mels(model, mels, device, space, batch_size)
    names, speakers = [b for b, _ in meta], [s for _, s in meta]
    kinds = ["utt"] * len(meta)
    gst = getattr(model, "gst", None)
    if gst is not None and space == "film":
        n_tok = gst.embed.shape[0]
        g, b = gst.from_token_weights(torch.eye(n_tok, device=device))
        X = torch.cat([X, torch.cat([g.float(), b.float()], 1)])
        top = torch.cat([top, torch.arange(n_tok, device=device)])
        names += [f"token_{k}" for k in range(n_tok)]
        speakers += ["-"] * n_tok
        kinds += ["token"] * n_tok
    return {"names": names, "speakers": speakers, "kinds": kinds, "X": X.contiguous(), "top_token": top}


def _subsample(n_utts, cap, seed):
    if n_utts <= cap:
        return None
    g = torch.Generator().manual_seed(int(seed))
    return torch.randperm(n_utts, generator=g)[:cap].sort().values


def _plot(path, y, cluster, is_tok, names):
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        return None
    fig, ax = plt.subplots(figsize=(8, 8))
    u = ~is_tok
    ax.scatter(y[u, 0], y[u, 1], c=cluster[u], cmap="tab20", s=6, linewidths=0)
    if is_tok.any():
        ax.scatter(y[is_tok, 0], y[is_tok, 1], c="black", marker="*", s=120)
        for i in np.nonzero(is_tok)[0]:
            ax.annotate(names[i], (y[i, 0], y[i, 1]), fontsize=8)
    ax.set_xticks([])
    ax.set_yticks([])
    fig.tight_layout()
    fig.savefig(path, dpi=120)
    plt.close(fig)
    return path


@torch.no_grad()
def style_map(model, configs, source, device, out_dir, space="film", clusters: Optional[int] = None,
              perplexity=30.0, iters=750, max_utts=16384, like: Optional[str] = None, top=10, seed=0,
              batch_size=32) -> dict:
    """Embed, subsample, standardise, cluster, lay out, write the files -> the summary (also ``style_map.json``)."""
    emb = embed_corpus(model, configs, source, device, space, batch_size)
    gst = getattr(model, "gst", None)
    n_tok_bank = int(gst.embed.shape[0]) if gst is not None else 0
    if clusters is None:
        clusters = n_tok_bank if gst is not None else 10
    kinds = np.asarray(emb["kinds"])
    n_utts_all = int((kinds == "utt").sum())
    n_tok = len(kinds) - n_utts_all
    keep = _subsample(n_utts_all, min(int(max_utts), ref.TSNE_MAX_N) - n_tok, seed)
    rows = list(range(len(kinds)))
    if keep is not None:
        rows = keep.tolist() + list(range(n_utts_all, len(kinds)))
    idx = torch.tensor(rows, device=emb["X"].device)
    X = emb["X"][idx].float()
    names = [emb["names"][r] for r in rows]
    speakers = [emb["speakers"][r] for r in rows]
    kinds = kinds[rows]
    tops = emb["top_token"][idx].tolist() if emb["top_token"] is not None else [None] * len(rows)
    n_utts = len(rows) - n_tok
    N = len(rows)
    if N < 7:
        raise ValueError(f"the style map needs at least 7 rows, {source} gives {N}")
    mean = X[:n_utts].mean(0, keepdim=True)
    std = X[:n_utts].std(0, unbiased=False, keepdim=True)
    std = torch.where(std > 0, std, torch.ones_like(std))
    Z = ((X - mean) / std).contiguous()

    k = max(1, min(int(clusters), n_utts))
    labels_u, cent, km_iters = ops.kmeans(Z[:n_utts].contiguous(), k, seed=seed)
    dist = torch.cdist(Z.double(), cent.double())          # tokens take the nearest utterance cluster
    cluster = torch.cat([labels_u.long(), dist[n_utts:].argmin(1)])
    d_cent = dist.gather(1, cluster[:, None])[:, 0]
    used = float(min(float(perplexity), (N - 1) / 3))
    y, trace = ops.tsne(Z, used, n_iter=int(iters), exag_iter=min(250, int(iters) // 2), seed=seed)

    exemplars = []
    for c in range(k):
        members = torch.nonzero(cluster[:n_utts] == c)[:, 0]
        order = members[d_cent[members].argsort()][:EXEMPLARS].tolist()
        exemplars.append([{"basename": names[i], "speaker": speakers[i], "distance": float(d_cent[i])} for i in order])
    neighbours = None
    if like:
        from ..infer.synthesis import reference_mel

        q, _ = embed_mels(model, [reference_mel(configs[0], like)], device, space, 1)
        dq = torch.cdist(((q.float() - mean) / std).double(), Z[:n_utts].double())[0]
        near = dq.argsort()[:int(top)].tolist()
        neighbours = [{"basename": names[i], "speaker": speakers[i], "distance": float(dq[i]),
                       "cluster": int(cluster[i])} for i in near]

    os.makedirs(out_dir, exist_ok=True)
    yc, cl, dc = y.detach().cpu().double().numpy(), cluster.cpu().numpy(), d_cent.cpu().numpy()
    with open(os.path.join(out_dir, "style_map.csv"), "w", newline="", encoding="utf-8") as f:
        wr = csv.writer(f)
        wr.writerow(["basename", "speaker", "kind", "x", "y", "cluster", "dist_to_centroid", "top_token"])
        for i in range(N):
            wr.writerow([names[i], speakers[i], kinds[i], f"{yc[i, 0]:.6g}", f"{yc[i, 1]:.6g}", int(cl[i]),
                         f"{dc[i]:.6g}", "" if tops[i] is None else int(tops[i])])
    png = _plot(os.path.join(out_dir, "style_map.png"), yc, cl, kinds == "token", names)
    draft = None
    if gst is not None and k <= n_tok_bank:
        draft = os.path.join(out_dir, "annotations_draft.txt")
        with open(draft, "w", encoding="utf-8") as f:
            f.write("# exemplars of every cluster: correct the label (a token index), then tune_style.py\n")
            for c, ex in enumerate(exemplars):
                for e in ex:
                    f.write(f"{e['basename']}|{e['speaker']}|{c}\n")
    rep = {"N": N, "utterances": n_utts, "tokens": n_tok, "space": space, "dim": int(Z.shape[1]),
           "subsampled_from": n_utts_all if keep is not None else None,
           "perplexity": used, "iters": int(iters), "kl_trace": [float(v) for v in trace],
           "final_kl": float(trace[-1]), "clusters": k, "kmeans_iterations": int(km_iters),
           "cluster_sizes": torch.bincount(cluster[:n_utts], minlength=k).tolist(), "exemplars": exemplars,
           "like": like, "neighbours": neighbours, "png": png is not None, "annotations_draft": draft is not None}
    if keep is not None:
        rep["note"] = f"{n_utts_all} utterances subsampled to {n_utts} (seed {seed})"
    with open(os.path.join(out_dir, "style_map.json"), "w", encoding="utf-8") as f:
        json.dump(rep, f, indent=2)
    return rep
