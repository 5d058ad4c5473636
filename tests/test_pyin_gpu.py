"""csrc/k_pyin.hip (``ops.pyin`` / ``ops.pyin_obs`` / ``ops.pyin_decode`` on the GPU) against ``ops.reference`` in
float64, and the waveform-level metrics with ``tracker="pyin"`` on the GPU against the CPU path.

Numerics convention (as for tests/test_pitch_gpu.py): the yardstick of a case is the float32 torch reference's own
deviation from the float64 reference on the same inputs; the kernels may deviate from float64 by up to MARGIN = 8 times
that, with a floor of 4 * 2^-23 for the probabilities.  A case is one (sr, hop, frame) setting with all its utterances.
Every figure is printed on a ``PYINNUM`` line before it is asserted.  The references of a case are computed once and
shared.

A frame *disagrees* with float64 at the candidate level when its set of non-zero bins differs (a candidate within
rounding of a bin edge, a trough on a near-equality, or a trough so close to cmnd 1 that its weight, 1e-60 say, is
below float32's range), and at the track level when its voicing or its decoded bin differs.  At most 0.5 % of all frames of the set (rounded up) may disagree at either level; the float32 CPU reference
itself must disagree on none (a condition of the inputs: the seeds below were chosen for it)."""
import functools
import math

import numpy as np
import pytest
import torch

from pitch_signals import short, speechlike, zero_headed

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

MARGIN = 8.0
PROB_FLOOR = 4 * 2.0 ** -23
FMIN, BPS = 71.0, 20
# (sr, hop, frame) -> (samples, seed) of every utterance: the cases and sample counts of tests/test_pitch_gpu.py (3 to
# 36 frames at 22050 Hz, a hop that is no power of two, tau_max = 113 and 622) and (22050, 64, 512): h = 10 instead
# of 50, 47 frames.  839 bins cross the wave boundaries of the decoder in every case.
CASES = {(22050, 256, 1024): ((513, 513), (1024, 1024), (1786, 1786), (9000, 9000 % 97)),
         (16000, 200, 1024): ((9000, 3),), (8000, 100, 512): ((4000, 4000),),
         (44100, 512, 2048): ((20000, 1),), (22050, 64, 512): ((3000, 3000),)}


def signal(n, seed, sr):
    return short(seed, n, sr) if n < 5000 else speechlike(seed, n, sr)


def bins_of(f0):
    """Decoded state per frame: the bin of a voiced frame, -1 for an unvoiced one."""
    f = f0.double()
    b = torch.round(12 * BPS * torch.log2(f.clamp(min=1.0) / FMIN)).long()
    return torch.where(f > 0, b, torch.full_like(b, -1))


def pyin_all(x, case, dtype, device="cpu"):
    sr, hop, frame = case
    return ops.pyin(torch.from_numpy(x).to(dtype).to(device), [len(x)], sr, hop, frame, return_obs=True)


@functools.lru_cache(maxsize=None)
def references(case):
    """Inputs, float64 and float32 CPU references of a case, concatenated over its utterances."""
    sr = case[0]
    xs = [signal(n, seed, sr) for n, seed in CASES[case]]
    r = {"xs": xs}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        outs = [pyin_all(x, case, dtype) for x in xs]
        r["f" + tag], r["p" + tag], r["o" + tag] = (torch.cat([o[i] for o in outs]) for i in (0, 2, 3))
        r["frames"] = [o[1][0] for o in outs]
    return r


@functools.lru_cache(maxsize=None)
def hip_singles(case):
    outs = [pyin_all(x, case, torch.float32, "cuda") for x in references(case)["xs"]]
    return tuple(torch.cat([o[i] for o in outs]).cpu() for i in (0, 2, 3)) + ([o[1][0] for o in outs],)


def obs_disagreeing(o, o64):
    return torch.nonzero(((o > 0) != (o64 > 0)).any(1)).flatten().tolist()


def track_disagreeing(f, f64):
    return torch.nonzero(bins_of(f) != bins_of(f64)).flatten().tolist()


def deviation(a, a64, skip):
    keep = torch.ones(a64.shape[0], dtype=torch.bool)
    keep[skip] = False
    return float((a.double() - a64)[keep].abs().max()) if keep.any() else 0.0


@pytest.mark.parametrize("case", list(CASES))
def test_obs_voiced_prob_and_track_against_float64(case):
    r = references(case)
    f, p, o, frames = hip_singles(case)
    sr, hop, _ = case
    assert frames == r["frames"] == [1 + n // hop for n, _ in CASES[case]]
    assert f.dtype == p.dtype == o.dtype == torch.float32 and o.shape == r["o64"].shape and o.shape[1] == 839
    assert torch.isfinite(f).all() and torch.isfinite(p).all() and torch.isfinite(o).all()
    assert torch.all(o >= 0) and torch.all((p >= 0) & (p <= 1))
    bad_ref, bad = obs_disagreeing(r["o32"], r["o64"]), obs_disagreeing(o, r["o64"])
    for i in bad:
        print(f"PYINNUM obs disagree case={case} frame={i} f64 bins={torch.nonzero(r['o64'][i]).flatten().tolist()} "
              f"hip bins={torch.nonzero(o[i]).flatten().tolist()}")
    ref_o, hip_o = deviation(r["o32"], r["o64"], bad_ref), deviation(o, r["o64"], bad)
    ref_p, hip_p = deviation(r["p32"], r["p64"], bad_ref), deviation(p, r["p64"], bad)
    print(f"PYINNUM obs case={case} frames={len(f)} candidates={int((r['o64'] > 0).sum())} disagree: ref32 {len(bad_ref)} "
          f"hip {len(bad)}  max|obs - f64|: ref32 {ref_o:.3e} hip {hip_o:.3e}  max|voiced_prob - f64|: ref32 {ref_p:.3e} "
          f"hip {hip_p:.3e}")
    tbad_ref, tbad = track_disagreeing(r["f32"], r["f64"]), track_disagreeing(f, r["f64"])
    for i in tbad:
        print(f"PYINNUM track disagree case={case} frame={i} f64={float(r['f64'][i])!r} hip={float(f[i])!r}")
    voiced = r["f64"] > 0
    cents = float((1200 * torch.log2(f.double()[voiced] / r["f64"][voiced])).abs().max()) if voiced.any() else 0.0
    print(f"PYINNUM track case={case} voiced={int(voiced.sum())} disagree: ref32 {len(tbad_ref)} hip {len(tbad)}  "
          f"max |cents| of the bin centres on voiced frames {cents:.3e}")
    assert bad_ref == [] and tbad_ref == []
    assert hip_o <= max(MARGIN * ref_o, PROB_FLOOR)
    assert hip_p <= max(MARGIN * ref_p, PROB_FLOOR)


def test_disagreeing_frames_of_the_whole_set():
    total, bad, tbad = 0, 0, 0
    for case in CASES:
        r = references(case)
        f, _, o, _ = hip_singles(case)
        total += len(f)
        bad += len(obs_disagreeing(o, r["o64"]))
        tbad += len(track_disagreeing(f, r["f64"]))
    allowed = math.ceil(0.005 * total)
    print(f"PYINNUM set frames={total} disagreeing: obs {bad} track {tbad} allowed={allowed}")
    assert bad <= allowed and tbad <= allowed


def plane(seed, T, NB, h):
    """A sparse candidate plane: 1-3 candidates per frame around a random walk of 0 .. h bins per frame that starts at
    an edge of the grid, now and then a jump beyond h, and empty stretches.  fp32, voiced_prob = the row sums."""
    rng = np.random.default_rng(seed)
    obs = np.zeros((T, NB), np.float32)
    b = 0 if seed % 2 else NB - 1
    for t in range(T):
        if rng.random() < 0.08:
            b = int(rng.integers(0, NB))  # a jump
        else:
            b = int(np.clip(b + rng.integers(-h, h + 1), 0, NB - 1))
        if 20 <= t % 35 < 20 + seed % 7:
            continue  # an empty stretch
        w = rng.dirichlet(np.ones(3)) * rng.uniform(0.3, 1.0)
        for k in range(int(rng.integers(1, 4))):
            c = b if k == 0 else int(np.clip(b + rng.integers(-2 * h, 2 * h + 1), 0, NB - 1))
            obs[t, c] += np.float32(w[k])
    vp = np.minimum(obs.sum(1, dtype=np.float32), np.float32(1))
    return torch.from_numpy(obs), torch.from_numpy(vp)


DECODER_CASES = [(839, 256, 1), (839, 64, 11), (65, 256, 21), (65, 64, 31)]  # (NB, hop, seed): h = 50 / 10


@functools.lru_cache(maxsize=None)
def decoder_references(case):
    NB, hop, seed = case
    fmax = FMIN * 2.0 ** ((NB - 1 + 0.5) / (12 * BPS))
    assert ref.pyin_bins(22050, hop, FMIN, fmax) == (NB, 50 if hop == 256 else 10)
    T = 70
    planes = [plane(seed + k, T, NB, 50 if hop == 256 else 10) for k in range(2)]
    obs, vp = torch.cat([p[0] for p in planes]), torch.cat([p[1] for p in planes])
    f64 = ref.pyin_decode(obs.double(), vp.double(), [T, T], 22050, hop)
    f32 = ref.pyin_decode(obs, vp, [T, T], 22050, hop)
    return obs, vp, f64, f32


@functools.lru_cache(maxsize=None)
def decoder_hip(case):
    obs, vp, _, _ = decoder_references(case)
    return ops.pyin_decode(obs.cuda(), vp.cuda(), [70, 70], 22050, case[1]).cpu()


def test_decoder_alone_on_constructed_planes():
    total, bad_all = 0, 0
    for case in DECODER_CASES:
        obs, vp, f64, f32 = decoder_references(case)
        f = decoder_hip(case)
        bad_ref, bad = track_disagreeing(f32, f64), track_disagreeing(f, f64)
        s = bins_of(f64)
        print(f"PYINNUM decode NB={case[0]} hop={case[1]} frames={len(f)} voiced={int((s >= 0).sum())} switches="
              f"{int(((s[1:] >= 0) != (s[:-1] >= 0)).sum())} bins {int(s[s >= 0].min())} .. {int(s.max())} disagree: "
              f"ref32 {len(bad_ref)} hip {len(bad)}")
        assert f.dtype == torch.float32 and torch.isfinite(f).all()
        assert bad_ref == []
        from speakingstyle_amd.ops import hip

        other = hip.pyin_decode(obs.cuda(), vp.cuda(), [70, 70], 22050, case[1], bins_per_thread=4)
        assert torch.equal(other.cpu(), f)  # four bins per thread: the same track
        total += len(f)
        bad_all += len(bad)
    allowed = math.ceil(0.005 * total)
    print(f"PYINNUM decode set frames={total} disagreeing={bad_all} allowed={allowed}")
    assert bad_all <= allowed


@pytest.mark.parametrize("NB,hop", [(839, 256), (65, 64)])
def test_decoder_on_empty_and_constant_planes(NB, hop):
    T = 70
    z = torch.zeros(T, NB, device="cuda")
    assert torch.all(ops.pyin_decode(z, torch.zeros(T, device="cuda"), [T], 22050, hop) == 0)
    for b in (0, NB // 2, NB - 1):  # the band's edges at bins 0 and NB - 1
        obs = z.clone()
        obs[:, b] = 0.9
        f0 = ops.pyin_decode(obs, torch.full((T,), 0.9, device="cuda"), [40, 30], 22050, hop).cpu()
        assert torch.all(bins_of(f0) == b), (b, bins_of(f0))
    # voiced, 30 empty frames, voiced again: the switch bit both ways
    obs = z.clone()
    obs[:20, 7] = 0.9
    obs[50:, NB - 3] = 0.9
    vp = obs.sum(1)
    got = bins_of(ops.pyin_decode(obs, vp, [T], 22050, hop).cpu())
    want = bins_of(ref.pyin_decode(obs.cpu().double(), vp.cpu().double(), [T], 22050, hop))
    assert torch.equal(got, want) and torch.all(want[:20] == 7) and torch.all(want[50:] == NB - 3)
    assert torch.all(want[25:45] == -1)


def test_mixed_batch_is_each_utterance_alone_and_repeatable():
    case = (22050, 256, 1024)
    xs = references(case)["xs"]
    f1, p1, o1, frames = hip_singles(case)
    order = [3, 0, 2, 1]
    wav = torch.from_numpy(np.concatenate([xs[i] for i in order])).float().cuda()
    lens = [len(xs[i]) for i in order]
    f, fr, p, o = ops.pyin(wav, lens, *case, return_obs=True)
    assert fr == [frames[i] for i in order]
    starts = np.concatenate([[0], np.cumsum(frames)])
    rows = torch.cat([torch.arange(starts[i], starts[i + 1]) for i in order])
    assert torch.equal(f.cpu(), f1[rows]) and torch.equal(p.cpu(), p1[rows]) and torch.equal(o.cpu(), o1[rows])
    f2, _, p2, o2 = ops.pyin(wav, lens, *case, return_obs=True)
    assert torch.equal(f, f2) and torch.equal(p, p2) and torch.equal(o, o2)
    f3, _, p3 = ops.pyin(wav, lens, *case)  # without the plane: the same track
    assert torch.equal(f, f3) and torch.equal(p, p3)
    # the back-pointer planes in chunks of one utterance: the same track
    obs, vp = o.contiguous(), p.contiguous()
    from speakingstyle_amd.ops import hip

    f4 = hip.pyin_decode(obs, vp, fr, 22050, 256, plane_budget=1)
    assert torch.equal(f, f4)
    # the decoder's other form (four bins per thread): the same track
    assert torch.equal(f, hip.pyin_decode(obs, vp, fr, 22050, 256, bins_per_thread=4))


def test_silence_constant_and_zero_headed_frames():
    for x in (np.zeros(3000), np.full(3000, 0.25)):
        f0, _, vp, obs = ops.pyin(torch.from_numpy(x).float().cuda(), [3000], 22050, 256, return_obs=True)
        assert torch.all(f0 == 0) and torch.all(vp == 0) and torch.all(obs == 0)
    x = torch.from_numpy(zero_headed()).float()
    f0, _, vp, obs = ops.pyin(x.cuda(), [len(x)], 22050, 256, return_obs=True)
    want = ref.pyin(x, [len(x)], 22050, 256)[0]
    f0, vp, obs = f0.cpu(), vp.cpu(), obs.cpu()
    assert torch.isfinite(f0).all() and torch.isfinite(vp).all() and torch.isfinite(obs).all()
    assert torch.all(f0[:9] == 0) and torch.all(vp[:8] == 0) and torch.all(obs[:8] == 0)
    assert (f0 > 0).any() and torch.equal(f0 > 0, want > 0)


def test_value_errors_are_those_of_the_cpu():
    x = torch.zeros(4000, device="cuda")
    with pytest.raises(ValueError, match="h = 200"):
        ops.pyin(x, [4000], 22050, 1024)
    with pytest.raises(ValueError, match="NB = 1678"):
        ops.pyin(x, [4000], 22050, 256, bins_per_semitone=40)
    with pytest.raises(ValueError, match="1000"):
        ops.pyin(x, [4000], 22050, 256, frame=1000)
    with pytest.raises(ValueError, match="3999"):
        ops.pyin(x, [3999], 22050, 256)
    with pytest.raises(ValueError, match="frames"):
        ops.pyin_decode(torch.zeros(5, 839, device="cuda"), torch.zeros(5, device="cuda"), [4], 22050, 256)


def test_wave_metrics_against_the_cpu_path():
    from speakingstyle_amd.analysis.objective import wave_metrics
    from speakingstyle_amd.config import load_named

    pp = load_named("LJSpeech")[0]
    rng = np.random.default_rng(11)
    a, b = [], []
    for seed, n in ((21, 9000), (22, 7000), (23, 8000)):  # the three pairs of tests/test_pitch_gpu.py
        x = speechlike(seed, n, 22050)
        m = int(n / 1.05)
        a.append(x)
        b.append(np.interp(np.arange(m) * 1.05, np.arange(n), x) + 1e-3 * rng.standard_normal(m))
    la, lb = [len(x) for x in a], [len(x) for x in b]
    wa, wb = (torch.from_numpy(np.concatenate(v)).float() for v in (a, b))
    got = wave_metrics(wa.cuda(), la, wb.cuda(), lb, pp, tracker="pyin")
    want = wave_metrics(wa, la, wb, lb, pp, tracker="pyin")
    clean = []
    for w, lens in ((wa, la), (wb, lb)):  # the two F0 tracks of every side, frame by frame
        fg, frames, _ = ops.pyin(w.cuda(), lens, 22050, 256)
        fc = ops.pyin(w, lens, 22050, 256)[0]
        at, side = 0, []
        for T in frames:
            side.append(track_disagreeing(fg.cpu()[at:at + T], fc[at:at + T]) == [])
            at += T
        clean.append(side)
    for p in range(3):
        Tx, Ty = 1 + la[p] // 256, 1 + lb[p] // 256
        bound = (Tx + Ty + 13 + 8) * 2.0 ** -23
        ok = clean[0][p] and clean[1][p]
        print(f"PYINNUM wave pair={p} frames=({Tx}, {Ty}) tracks_agree={ok} path_len hip={int(got['path_len'][p])} "
              f"cpu={int(want['path_len'][p])} bound={bound:.3e} " +
              " ".join(f"{k}: hip={got[k][p]!r} cpu={want[k][p]!r}" for k in sorted(want) if k != "path_len"))
    for p in range(3):
        Tx, Ty = 1 + la[p] // 256, 1 + lb[p] // 256
        u, v = float(got["wave_mcd_db"][p]), float(want["wave_mcd_db"][p])
        assert abs(u - v) <= (Tx + Ty + 13 + 8) * 2.0 ** -23 * max(abs(u), abs(v))
        if clean[0][p] and clean[1][p]:
            for k in ("wave_vde", "wave_gpe", "wave_ffe"):
                assert got[k][p] == want[k][p] or (math.isnan(got[k][p]) and math.isnan(want[k][p])), (p, k)
