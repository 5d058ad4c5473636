"""``ops.reference.pyin`` (probabilistic YIN: the CPU path of ``ops.pyin`` and the oracle of csrc/k_pyin.hip) and its
plumbing: steady tones, silent / constant / zero-headed input, packing, the robustness against noise that is the reason
for the tracker (against ``ops.yin`` on the same input), the argument errors, ``wave_metrics(tracker=...)``, the
``analyze.py`` flag and the config enum."""
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

from pitch_signals import short, speechlike, tone, zero_headed
from pyin_signals import noisy_voice

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMIN, BINS = 71.0, 12 * 20  # the default grid: bin b is FMIN 2^(b / BINS)


def bins_of(f0):
    return BINS * np.log2(np.asarray(f0, np.float64) / FMIN)


def test_plan_and_grid():
    x = torch.zeros(4000)
    lens, frames, tau_min, tau_max, NB, h = ref.pyin_plan(x, [4000], 22050, 256)
    assert (lens, frames, tau_min, tau_max) == ref.yin_plan(x, [4000], 22050, 256)
    assert (NB, h) == (839, 50)
    assert ref.pyin_bins(22050, 64) == (839, 10)
    assert ref.pyin_bins(16000, 200) == (839, 50) and ref.pyin_bins(44100, 512) == (839, 50)


def test_value_errors():
    x = torch.zeros(4000)
    with pytest.raises(ValueError, match="h = 200"):
        ops.pyin(x, [4000], 22050, 1024)
    with pytest.raises(ValueError, match="NB = 1678"):
        ops.pyin(x, [4000], 22050, 256, bins_per_semitone=40)
    with pytest.raises(ValueError, match="1000"):  # those of yin
        ops.pyin(x, [4000], 22050, 256, frame=1000)
    with pytest.raises(ValueError, match="3999"):
        ops.pyin(x, [3999], 22050, 256)
    with pytest.raises(ValueError, match="frames"):
        ops.pyin_decode(torch.zeros(5, 839), torch.zeros(5), [4], 22050, 256)


@pytest.mark.parametrize("f", [110.0, 220.0, 440.0])
def test_steady_tones(f):
    x = tone(f, 22050 // 2, 22050)
    for dtype in (torch.float64, torch.float32):
        f0, frames, vp = ops.pyin(torch.from_numpy(x).to(dtype), [len(x)], 22050, 256)
        assert frames == [1 + len(x) // 256] and f0.dtype == dtype and vp.dtype == dtype
        # as for yin: the three frames at either end straddle the reflection
        inner, p = f0[3:-3].double().numpy(), vp[3:-3].double().numpy()
        assert inner.size > 10 and np.all(inner > 0)
        assert np.abs(bins_of(inner) - bins_of(f)).max() <= 1.0, (dtype, inner)
        assert np.all(np.abs(bins_of(inner) - np.round(bins_of(inner))) < 1e-3)  # bin centres
        assert p.min() > 0.9, (dtype, p.min())


def test_silence_constant_and_zero_headed_frames_are_unvoiced():
    for x in (np.zeros(3000), np.full(3000, 0.25)):
        for dtype in (torch.float64, torch.float32):
            f0, _, vp, obs = ops.pyin(torch.from_numpy(x).to(dtype), [3000], 22050, 256, return_obs=True)
            assert torch.all(f0 == 0) and torch.all(vp == 0) and torch.all(obs == 0)
            assert obs.shape == (12, 839)
    x = zero_headed()
    for dtype in (torch.float64, torch.float32):
        f0, _, vp, obs = ops.pyin(torch.from_numpy(x).to(dtype), [len(x)], 22050, 256, return_obs=True)
        assert torch.isfinite(f0).all() and torch.isfinite(vp).all() and torch.isfinite(obs).all()
        assert torch.all((vp >= 0) & (vp <= 1)) and torch.all(obs >= 0)
        # frames 0 .. 8 begin in the zeros (tests/test_pitch_cpu.py): cmnd is 1 over all of frames 0 .. 7
        assert torch.all(f0[:9] == 0) and torch.all(vp[:8] == 0) and torch.all(obs[:8] == 0)
        assert (f0 > 0).any()


def test_obs_of_a_hand_made_plane():
    """Three troughs at lags 50 / 100 / 150 with cmnd 0.3 / 0.1 / 0.2: the first takes the thresholds above 0.3, the
    second those in (0.1, 0.3] and the mass no trough is below, the third nothing."""
    tau_min, tau_max = 27, 311
    cm = torch.ones(2, tau_max + 1, dtype=torch.float64)
    for lag, v in ((50, 0.3), (100, 0.1), (150, 0.2)):
        cm[0, lag - 1:lag + 2] = torch.tensor([0.9, v, 0.9], dtype=torch.float64)
    obs, vp = ops.pyin_obs(cm, 22050, tau_min, tau_max)
    F = lambda x: 1 - (1 - x) ** 18 * (1 + 18 * x)  # noqa: E731
    want = {round(float(bins_of(22050 / 50))): 1 - F(0.3), round(float(bins_of(22050 / 100))): F(0.3) - 0.99 * F(0.1)}
    assert sorted(torch.nonzero(obs[0]).flatten().tolist()) == sorted(want)
    for b, w in want.items():
        assert abs(float(obs[0, b]) - w) <= 1e-12
    assert abs(float(vp[0]) - (1 - 0.99 * F(0.1))) <= 1e-12
    assert torch.all(obs[1] == 0) and float(vp[1]) == 0.0


def test_decode_of_hand_made_planes():
    NB = 839
    z = torch.zeros(6, NB, dtype=torch.float64)
    assert torch.all(ops.pyin_decode(z, torch.zeros(6, dtype=torch.float64), [6], 22050, 256) == 0)
    for b in (0, 400, NB - 1):  # a constant bin, the band's edges included
        obs = z.clone()
        obs[:, b] = 0.9
        f0 = ops.pyin_decode(obs, torch.full((6,), 0.9, dtype=torch.float64), [4, 2], 22050, 256)
        assert np.abs(bins_of(f0.numpy()) - b).max() < 1e-6
    # a candidate further than h = 50 bins from the track cannot be reached in one frame: the track stays, the
    # outlier frame goes through a neighbouring state
    obs = z.clone()
    obs[:, 300] = 0.9
    obs[3] = 0
    obs[3, 500] = 0.9
    f0 = ops.pyin_decode(obs, torch.full((6,), 0.9, dtype=torch.float64), [6], 22050, 256)
    got = bins_of(np.where(f0.numpy() > 0, f0.numpy(), FMIN))
    assert np.abs(got[[0, 1, 2, 4, 5]] - 300).max() < 1e-6 and abs(got[3] - 500) > 100


def test_packed_batch_is_the_utterances_one_by_one():
    xs = [short(1, 1786), speechlike(4, 6000, 22050), short(3, 1024)]
    lens = [len(x) for x in xs]
    f0, frames, vp, obs = ops.pyin(torch.from_numpy(np.concatenate(xs)).float(), lens, 22050, 256, return_obs=True)
    assert f0.dtype == torch.float32 and frames == [1 + n // 256 for n in lens] and obs.shape == (sum(frames), 839)
    at = 0
    for x, T in zip(xs, frames):
        one = ops.pyin(torch.from_numpy(x).float(), [len(x)], 22050, 256, return_obs=True)
        assert torch.equal(f0[at:at + T], one[0]) and torch.equal(vp[at:at + T], one[2])
        assert torch.equal(obs[at:at + T], one[3])
        at += T
    assert (f0 > 0).any() and (f0 == 0).any()
    assert torch.equal(ops.pyin(torch.from_numpy(np.concatenate(xs)).float(), lens, 22050, 256)[0], f0)


@functools.lru_cache(maxsize=None)
def noisy_tracks():
    """Voicing errors and gross errors of both trackers on 3 seeds x 3 s of ``noisy_voice`` with noise 0.10."""
    sr, hop = 22050, 256
    sig = [noisy_voice(seed, 3 * sr, sr, 0.10, 1.0) for seed in (1, 2, 3)]
    wav = torch.from_numpy(np.concatenate([s[0] for s in sig])).float()
    lens = [len(s[0]) for s in sig]
    fy, frames = ops.yin(wav, lens, sr, hop)
    fp = ops.pyin(wav, lens, sr, hop)[0]
    centre = np.concatenate([np.minimum(np.arange(T) * hop, n - 1) for T, n in zip(frames, lens)])  # frame t is around t hop
    truth = np.concatenate([s[1] for s in sig]), np.concatenate([s[2] for s in sig])
    at = np.concatenate([[0], np.cumsum(lens)[:-1]]).repeat(frames) + centre
    tf, tv = truth[0][at], truth[1][at]
    out = {"frames": sum(frames), "voiced": int(tv.sum())}
    for name, f in (("yin", fy.numpy()), ("pyin", fp.numpy())):
        both = (f > 0) & tv
        out[name] = (int(((f > 0) != tv).sum()), int((np.abs(f - tf)[both] > 0.2 * tf[both]).sum()), int(both.sum()))
    return out


def test_noise_robustness_against_yin():
    r = noisy_tracks()
    print(f"PYINNUM noisy frames={r['frames']} voiced={r['voiced']} (voicing errors, gross errors, voiced in both): "
          f"yin {r['yin']} pyin {r['pyin']}")
    assert r["frames"] == 777 and r["voiced"] > 300
    assert r["pyin"][0] <= 0.5 * r["yin"][0]
    assert r["pyin"][1] == 0 and r["pyin"][2] > 300


def test_wave_metrics_tracker():
    from speakingstyle_amd.analysis.objective import WAVE_METRICS, wave_metrics
    from speakingstyle_amd.config import load_named

    pp = load_named("LJSpeech")[0]
    rng = np.random.default_rng(5)
    a = [speechlike(5, 9000, 22050), short(6, 1786)]
    b = [x + 0.02 * rng.standard_normal(len(x)) for x in a]
    lens = [len(x) for x in a]
    wa, wb = (torch.from_numpy(np.concatenate(v)).float() for v in (a, b))
    plain = wave_metrics(wa, lens, wb, lens, pp)
    named = wave_metrics(wa, lens, wb, lens, pp, tracker="yin")
    assert list(plain) == list(named)
    for k in plain:
        assert np.array_equal(plain[k], named[k], equal_nan=True), k
    got = wave_metrics(wa, lens, wb, lens, pp, tracker="pyin")
    assert list(got) == list(plain) and set(WAVE_METRICS) <= set(got)
    assert np.array_equal(got["wave_mcd_db"], plain["wave_mcd_db"]) and np.array_equal(got["path_len"], plain["path_len"])
    for k in ("wave_vde", "wave_ffe"):
        assert got[k].shape == (2,) and np.all((got[k] >= 0) & (got[k] <= 1))
    # the figures are those of the pyin tracks along the same path: a batch against itself has no error
    same = wave_metrics(wa, lens, wa.clone(), lens, pp, tracker="pyin")
    for k in WAVE_METRICS:
        assert np.all(same[k] == 0.0), (k, same[k])
    with pytest.raises(ValueError, match="foo"):
        wave_metrics(wa, lens, wb, lens, pp, tracker="foo")


def test_analyze_flag_and_config_enum():
    spec = importlib.util.spec_from_file_location("analyze_cli", os.path.join(ROOT, "analyze.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["objective", "-p", "p", "-m", "m", "-t", "t", "--wave"]
    assert cli.build_parser().parse_args(base).pitch_tracker == "yin"
    assert cli.build_parser().parse_args(base + ["--pitch_tracker", "pyin"]).pitch_tracker == "pyin"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(base + ["--pitch_tracker", "foo"])

    from speakingstyle_amd.config import config_dir_triplet, load_yaml, normalize_preprocess_config

    p = load_yaml(config_dir_triplet("LJSpeech")[0])
    p["preprocessing"]["pitch"]["extractor"] = "pyin"
    assert normalize_preprocess_config(p)["preprocessing"]["pitch"]["extractor"] == "pyin"
    p["preprocessing"]["pitch"]["extractor"] = "foo"
    with pytest.raises(ValueError, match="foo"):
        normalize_preprocess_config(p)


def test_preprocess_extractor_runs_on_the_host():
    from speakingstyle_amd.data.preprocess import extract_f0

    x = tone(220.0, 6000, 22050).astype(np.float32)
    f0 = extract_f0(x, 22050, 256, "pyin")
    assert f0.dtype == np.float64 and f0.shape == (1 + 6000 // 256,)
    assert np.abs(bins_of(f0[3:-3]) - bins_of(220.0)).max() <= 1.0
    assert np.all(extract_f0(np.zeros(3000, np.float32), 22050, 256, "pyin") == 0)
