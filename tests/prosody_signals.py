"""Deterministic inputs of the prosody-transfer tests (tests/test_prosody_transfer_cpu.py, ..._gpu.py): functions of
their arguments alone."""
import numpy as np
import torch

SR, HOP = 22050, 256


def random_path(rng, tx, ty, stick=0.6):
    """A monotone warping path from (0, 0) to (tx - 1, ty - 1): diagonal / up (i + 1) / left (j + 1) steps, the
    previous step repeated with probability ``stick`` (long vertical and horizontal runs).  -> int32 [L, 2]."""
    i = j = 0
    cells, last = [(0, 0)], None
    while (i, j) != (tx - 1, ty - 1):
        moves = [m for m, ok in ((0, i < tx - 1 and j < ty - 1), (1, i < tx - 1), (2, j < ty - 1)) if ok]
        m = last if last in moves and rng.random() < stick else moves[int(rng.integers(len(moves)))]
        i, j = i + (m != 2), j + (m != 1)
        cells.append((i, j))
        last = m
    return np.asarray(cells, dtype=np.int32)


def durations_for(rng, n, total, zeros=0.2):
    """n integer durations >= 0 summing to ``total`` (>= 1), about ``zeros`` of them 0."""
    w = rng.random(n) * (rng.random(n) >= zeros)
    if w.sum() == 0:
        w[int(rng.integers(n))] = 1.0
    d = np.floor(w / w.sum() * total).astype(np.int64)
    nz = np.nonzero(w)[0]
    d[nz[int(rng.integers(len(nz)))]] += total - d.sum()
    return d


def f0_track(rng, ty, voicing="mixed"):
    """F0 in Hz over ty frames: 80 .. 400 with unvoiced stretches; ``voicing``: "mixed", "first" / "last" (one voiced
    frame, at that end), "none"."""
    f = rng.uniform(80.0, 400.0, ty)
    if voicing == "mixed":
        f = np.where(np.convolve(rng.standard_normal(ty + 4), np.ones(5) / 5, "valid") > -0.1, f, 0.0)
    elif voicing in ("first", "last"):
        keep = 0 if voicing == "first" else ty - 1
        f = np.where(np.arange(ty) == keep, f, 0.0)
    else:
        f = np.zeros(ty)
    return f


def pack_case(utts, nmax=None, dtype=torch.float64):
    """utts: dicts {"path" [L, 2], "src_dur" [N], "f0" [Ty], "energy" [Ty], "pred" [N], "tx", "ty"} -> the arguments
    of ``prosody_transfer`` up to ``pred_pitch`` (padding: -1 cells, durations 7 and predictions 9 past N, which must
    not matter)."""
    P = len(utts)
    lmax = max(u["tx"] for u in utts) + max(u["ty"] for u in utts) - 1
    nmax = nmax or max(len(u["src_dur"]) for u in utts)
    path = np.full((P, lmax, 2), -1, dtype=np.int32)
    dur = np.full((P, nmax), 7, dtype=np.int32)
    pred = np.full((P, nmax), 9.0)
    for p, u in enumerate(utts):
        n = len(u["src_dur"])
        path[p, :len(u["path"])] = u["path"]
        dur[p, :n] = u["src_dur"]
        pred[p, :n] = u["pred"]
    return (torch.from_numpy(path), torch.tensor([len(u["path"]) for u in utts], dtype=torch.int32),
            torch.from_numpy(dur), torch.tensor([len(u["src_dur"]) for u in utts], dtype=torch.int32),
            [u["tx"] for u in utts], [u["ty"] for u in utts],
            torch.from_numpy(np.concatenate([u["f0"] for u in utts])).to(dtype),
            torch.from_numpy(np.concatenate([u["energy"] for u in utts])).to(dtype), torch.from_numpy(pred).to(dtype))


def random_utterance(seed, n, ty, voicing="mixed", tx=None):
    """One utterance on a random path: tx between ty / 2 and 2 ty, durations with zeros summing to tx."""
    rng = np.random.default_rng(seed)
    tx = int(tx if tx is not None else rng.integers(max(1, ty // 2), 2 * ty + 1))
    return {"path": random_path(rng, tx, ty), "src_dur": durations_for(rng, n, tx), "f0": f0_track(rng, ty, voicing),
            "energy": rng.uniform(0.5, 60.0, ty), "pred": rng.standard_normal(n), "tx": tx, "ty": ty}


def cast(args, dtype, device=None):
    """The floating arguments of ``pack_case`` in ``dtype``, everything on ``device``."""
    out = []
    for a in args:
        if isinstance(a, torch.Tensor):
            a = a.to(dtype) if a.is_floating_point() else a
            a = a.to(device) if device is not None else a
        out.append(a)
    return tuple(out)


def _box(v, width=1025):
    pad = width // 2
    return np.convolve(np.pad(v, pad, mode="edge"), np.ones(width) / width, "valid")


def rendered_pair(seed, n_tok=10):
    """Two renderings of one token sequence with different timing.  Tokens: 6-harmonic tones (amplitudes 0.6^h,
    phase-continuous), F0 a permutation of linspace(110, 220, n_tok), amplitude uniform in 0.3 .. 1.0; F0 and amplitude
    smoothed with a 1025-sample box; white noise 0.002.  The x side has 10 .. 15 frames per token, the y side 8 .. 23;
    an utterance of N = hop sum(dur) samples has 1 + N // hop frames, the extra one belongs to the last token.
    -> {"x" / "y": {"wav" float32, "dur" int64 [n_tok] (frames, the extra one counted), "f0" / "amp" per sample}}"""
    rng = np.random.default_rng(seed)
    f0_tok = rng.permutation(np.linspace(110.0, 220.0, n_tok))
    amp_tok = rng.uniform(0.3, 1.0, n_tok)
    out = {}
    for side, (lo, hi) in (("x", (10, 15)), ("y", (8, 23))):
        dur = rng.integers(lo, hi + 1, n_tok)
        f0 = _box(np.repeat(f0_tok, dur * HOP))
        amp = _box(np.repeat(amp_tok, dur * HOP))
        ph = 2 * np.pi * np.cumsum(f0) / SR
        s = sum(0.6 ** h * np.sin((h + 1) * ph) for h in range(6))
        wav = 0.25 * amp * s + 0.002 * rng.standard_normal(len(ph))
        d = dur.astype(np.int64)
        d[-1] += 1
        out[side] = {"wav": np.clip(wav, -1, 1).astype(np.float32), "dur": d, "f0": f0, "amp": amp}
    return out


def token_means(per_frame, dur):
    """Mean of a per-frame contour over each token's frames."""
    ends = np.cumsum(dur)
    return np.asarray([per_frame[e - d:e].mean() for d, e in zip(dur, ends)])


def recovery_figures(pairs, rec_dur, pitch_hz, energy, y_energy_frames):
    """(largest duration error in frames, largest relative token-pitch error against the true contour's token means,
    largest relative token-energy error against the true amplitude contour's token means).  The front end's energy
    of a harmonic tone is proportional to its amplitude; the one constant of a recording is the ratio of its summed
    frame energies (``y_energy_frames``) to its summed amplitudes."""
    d_err = p_err = e_err = 0.0
    for k, pr in enumerate(pairs):
        dur = pr["y"]["dur"]
        n = len(dur)
        d_err = max(d_err, float(np.abs(rec_dur[k][:n] - dur).max()))
        centres = np.minimum(np.arange(int(dur.sum())) * HOP, len(pr["y"]["f0"]) - 1)
        p_true = token_means(pr["y"]["f0"][centres], dur)
        p_err = max(p_err, float(np.abs(pitch_hz[k][:n] / p_true - 1.0).max()))
        amp = pr["y"]["amp"][centres]
        e_true = token_means(amp, dur) * (y_energy_frames[k].sum() / amp.sum())
        e_err = max(e_err, float(np.abs(energy[k][:n] / e_true - 1.0).max()))
    return d_err, p_err, e_err


def recover(pairs, device):
    """Both renderings through ``recording_features``, the alignment and ``ops.prosody_transfer`` on ``device``."""
    from speakingstyle_amd import ops
    from speakingstyle_amd.analysis.objective import align
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.infer.transfer import recording_features

    pp = load_named("LJSpeech")[0]
    assert pp["preprocessing"]["audio"]["sampling_rate"] == SR and pp["preprocessing"]["stft"]["hop_length"] == HOP
    feats = {}
    for side in ("x", "y"):
        wavs = [torch.from_numpy(pr[side]["wav"]) for pr in pairs]
        feats[side] = recording_features(torch.cat(wavs).to(device), [len(w) for w in wavs], pp)
    xmel, _, _, xframes = feats["x"]
    ymel, yen, yf0, yframes = feats["y"]
    assert xframes == [int(pr["x"]["dur"].sum()) for pr in pairs]
    assert yframes == [int(pr["y"]["dur"].sum()) for pr in pairs]
    _, path, plen = align(xmel, xframes, ymel, yframes)
    n = len(pairs[0]["x"]["dur"])
    dur = torch.tensor(np.stack([pr["x"]["dur"] for pr in pairs]), dtype=torch.int32, device=device)
    rec, pitch, en, _, ok = ops.prosody_transfer(path, plen, dur, torch.full((len(pairs),), n, device=device), xframes,
                                                 yframes, yf0, yen, torch.zeros(len(pairs), n, device=device),
                                                 pitch_mode="absolute")
    assert bool(ok.all())
    cu = np.concatenate([[0], np.cumsum(yframes)])
    y_en = [yen.cpu().numpy()[cu[k]:cu[k + 1]] for k in range(len(pairs))]
    return recovery_figures(pairs, rec.cpu().numpy(), pitch.cpu().numpy(), en.cpu().numpy(), y_en)
