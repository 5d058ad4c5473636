"""csrc/k_pitch.hip (``ops.yin`` on the GPU) against ``ops.reference.yin`` in float64, and the waveform-level metrics
on the GPU against the CPU path.

Numerics convention (as for tests/test_align_gpu.py): the yardstick of a case is the float32 torch reference's own
deviation from the float64 reference on the same inputs; the kernel may deviate from float64 by up to MARGIN = 8 times
that.  A case is one (sr, hop, frame) setting with all its utterances.  Every figure is printed on a ``YINNUM`` line
before it is asserted.  The references of a case are computed once and shared.

A frame *disagrees* with float64 when its voicing differs or its F0 differs by more than 1e-3 relative: neighbouring
integer lags differ by at least 1 / tau_max >= 1.6e-3, so this separates a lag jump from rounding.  At most 0.5 % of
all frames of the set (rounded up) may disagree; the float32 CPU reference itself must disagree on none (a condition
of the inputs)."""
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
F0_FLOOR = 4 * 2.0 ** -23
LAG_JUMP = 1e-3
# (sr, hop, frame) -> sample counts; 22050 Hz: three slices past the zero head and the full signal; 16000 Hz: a hop
# that is no power of two; 8000 Hz / 512: tau_max = 113; 44100 Hz / 2048: tau_max = 622, more than two lags per lane
CASES = {(22050, 256, 1024): (513, 1024, 1786, 9000), (16000, 200, 1024): (9000,), (8000, 100, 512): (4000,),
         (44100, 512, 2048): (20000,)}


def signal(n, sr):
    return short(n, n, sr) if n < 5000 else speechlike(n % 97, n, sr)


@functools.lru_cache(maxsize=None)
def references(case):
    """Inputs, float64 and float32 CPU references of a case, utterance by utterance and concatenated."""
    sr, hop, frame = case
    xs = [signal(n, sr) for n in CASES[case]]
    r = {"xs": xs, "f64": [], "c64": [], "f32": [], "c32": []}
    for x in xs:
        f, _, c = ref.yin(torch.from_numpy(x), [len(x)], sr, hop, frame, return_cmnd=True)
        g, _, d = ref.yin(torch.from_numpy(x).float(), [len(x)], sr, hop, frame, return_cmnd=True)
        r["f64"].append(f), r["c64"].append(c), r["f32"].append(g), r["c32"].append(d)
    for k in ("f64", "c64", "f32", "c32"):
        r[k] = torch.cat(r[k])
    return r


def disagreeing(f, f64):
    """Indices of the frames of ``f`` that disagree with the float64 track."""
    f = f.double()
    v, v64 = f > 0, f64 > 0
    jump = v & v64 & ((f - f64).abs() > LAG_JUMP * f64)
    return torch.nonzero((v != v64) | jump).flatten().tolist()


def f0_error(f, f64, skip):
    """Maximum relative F0 error over the voiced frames outside ``skip``."""
    keep = (f64 > 0) & (f > 0)
    keep[skip] = False
    return float(((f.double() - f64).abs() / f64.clamp(min=1.0))[keep].max()) if keep.any() else 0.0


@functools.lru_cache(maxsize=None)
def hip_singles(case):
    sr, hop, frame = case
    out = [ops.yin(torch.from_numpy(x).float().cuda(), [len(x)], sr, hop, frame, return_cmnd=True) for x in references(case)["xs"]]
    return torch.cat([o[0] for o in out]).cpu(), torch.cat([o[2] for o in out]).cpu(), [o[1][0] for o in out]


@pytest.mark.parametrize("case", list(CASES))
def test_cmnd_and_f0_against_float64(case):
    r = references(case)
    f, c, frames = hip_singles(case)
    sr, hop, _ = case
    assert frames == [1 + n // hop for n in CASES[case]] and f.dtype == torch.float32 and c.dtype == torch.float32
    assert c.shape == r["c64"].shape and torch.isfinite(c).all() and torch.isfinite(f).all()
    ref_dev = float((r["c32"].double() - r["c64"]).abs().max())
    hip_dev = float((c.double() - r["c64"]).abs().max())
    print(f"YINNUM cmnd case={case} frames={len(f)} lags={c.shape[1] - 1} max|cmnd|={float(r['c64'].abs().max()):.3e} "
          f"ref32 {ref_dev:.3e} hip {hip_dev:.3e}")
    bad_ref, bad = disagreeing(r["f32"], r["f64"]), disagreeing(f, r["f64"])
    for i in bad:
        print(f"YINNUM disagree case={case} frame={i} f64={float(r['f64'][i])!r} hip={float(f[i])!r}")
    ref_err, hip_err = f0_error(r["f32"], r["f64"], bad_ref), f0_error(f, r["f64"], bad)
    print(f"YINNUM f0 case={case} voiced={int((r['f64'] > 0).sum())} disagree: ref32 {len(bad_ref)} hip {len(bad)}  "
          f"relative error: ref32 {ref_err:.3e} hip {hip_err:.3e}")
    assert hip_dev <= MARGIN * ref_dev
    assert bad_ref == []
    assert hip_err <= max(MARGIN * ref_err, F0_FLOOR)


def test_disagreeing_frames_of_the_whole_set():
    total, bad = 0, 0
    for case in CASES:
        r = references(case)
        total += len(r["f64"])
        bad += len(disagreeing(hip_singles(case)[0], r["f64"]))
    allowed = math.ceil(0.005 * total)
    print(f"YINNUM set frames={total} disagreeing={bad} allowed={allowed}")
    assert bad <= allowed


def test_mixed_batch_is_each_utterance_alone_and_repeatable():
    case = (22050, 256, 1024)
    xs = references(case)["xs"]
    f1, c1, frames = hip_singles(case)
    order = [3, 0, 2, 1]
    wav = torch.from_numpy(np.concatenate([xs[i] for i in order])).float().cuda()
    lens = [len(xs[i]) for i in order]
    f, fr, c = ops.yin(wav, lens, *case, return_cmnd=True)
    assert fr == [frames[i] for i in order]
    starts = np.concatenate([[0], np.cumsum(frames)])
    rows = torch.cat([torch.arange(starts[i], starts[i + 1]) for i in order])
    assert torch.equal(f.cpu(), f1[rows]) and torch.equal(c.cpu(), c1[rows])
    f2, _, c2 = ops.yin(wav, lens, *case, return_cmnd=True)
    assert torch.equal(f, f2) and torch.equal(c, c2)
    f3, _ = ops.yin(wav, lens, *case)  # without the plane: the same track
    assert torch.equal(f, f3)


def test_silence_constant_and_zero_headed_frames():
    for x in (np.zeros(3000), np.full(3000, 0.25)):
        f0, _, cm = ops.yin(torch.from_numpy(x).float().cuda(), [3000], 22050, 256, return_cmnd=True)
        assert torch.all(f0 == 0) and torch.isfinite(cm).all()
    x = torch.from_numpy(zero_headed()).float()
    f0, _, cm = ops.yin(x.cuda(), [len(x)], 22050, 256, return_cmnd=True)
    want, _, _ = ref.yin(x, [len(x)], 22050, 256, return_cmnd=True)
    f0, cm = f0.cpu(), cm.cpu()
    assert torch.isfinite(f0).all() and torch.isfinite(cm).all()
    assert torch.all(f0[:9] == 0) and torch.all(cm[:8] == 1) and torch.all(cm[8, :158] == 1)
    assert torch.any(cm[8, 158:] != 1) and torch.equal(f0 > 0, want > 0)


def test_value_errors_are_those_of_the_cpu():
    x = torch.zeros(4000, device="cuda")
    for kw, word in ((dict(frame=1000), "1000"), (dict(hop=0), "hop 0"), (dict(hop=1025), "1025")):
        args = dict(sr=22050, hop=256)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.yin(x, [4000], **args)
    with pytest.raises(ValueError, match="512 samples"):
        ops.yin(x[:3512], [3000, 512], 22050, 256)


def test_wave_metrics_against_the_cpu_path():
    from speakingstyle_amd.analysis.objective import wave_metrics
    from speakingstyle_amd.config import load_named

    pp = load_named("LJSpeech")[0]
    rng = np.random.default_rng(11)
    a, b = [], []
    for seed, n in ((21, 9000), (22, 7000), (23, 8000)):
        x = speechlike(seed, n, 22050)
        m = int(n / 1.05)
        a.append(x)
        b.append(np.interp(np.arange(m) * 1.05, np.arange(n), x) + 1e-3 * rng.standard_normal(m))
    la, lb = [len(x) for x in a], [len(x) for x in b]
    wa, wb = (torch.from_numpy(np.concatenate(v)).float() for v in (a, b))
    got = wave_metrics(wa.cuda(), la, wb.cuda(), lb, pp)
    want = wave_metrics(wa, la, wb, lb, pp)
    clean = []
    for w, lens in ((wa, la), (wb, lb)):  # the two F0 tracks of every side, frame by frame
        fg, frames = ops.yin(w.cuda(), lens, 22050, 256)
        fc, _ = ops.yin(w, lens, 22050, 256)
        at, side = 0, []
        for T in frames:
            side.append(disagreeing(fg.cpu()[at:at + T], fc[at:at + T].double()) == [])
            at += T
        clean.append(side)
    for p in range(3):
        Tx, Ty = 1 + la[p] // 256, 1 + lb[p] // 256
        bound = (Tx + Ty + 13 + 8) * 2.0 ** -23
        ok = clean[0][p] and clean[1][p]
        print(f"YINNUM wave pair={p} frames=({Tx}, {Ty}) tracks_agree={ok} path_len hip={int(got['path_len'][p])} "
              f"cpu={int(want['path_len'][p])} bound={bound:.3e} " +
              " ".join(f"{k}: hip={got[k][p]!r} cpu={want[k][p]!r}" for k in sorted(want) if k != "path_len"))
    for p in range(3):
        Tx, Ty = 1 + la[p] // 256, 1 + lb[p] // 256
        u, v = float(got["wave_mcd_db"][p]), float(want["wave_mcd_db"][p])
        assert abs(u - v) <= (Tx + Ty + 13 + 8) * 2.0 ** -23 * max(abs(u), abs(v))
        if clean[0][p] and clean[1][p]:
            for k in ("wave_vde", "wave_gpe", "wave_ffe"):
                assert got[k][p] == want[k][p] or (math.isnan(got[k][p]) and math.isnan(want[k][p])), (p, k)
