"""csrc/k_features.hip (``ops.frame_features`` / ``ops.interp_unvoiced`` on the GPU) against ``ops.reference`` in
float64, and ``Preprocessor(device="cuda")`` against ``device="cpu"`` on the tiny corpus of tests/feature_corpus.py.

Numerics convention (as for tests/test_pyin_gpu.py): the yardstick of a case is the float32 CPU reference's own
deviation from the float64 reference on the same input; the kernel may deviate from float64 by up to MARGIN = 8 times
that, with floors of 4 * 2^-20 absolute on log-mel (4 ulps at |log 1e-5| = 11.5) and 4 * 2^-23 relative on energy.  A
frame whose float64 energy is exactly 0 (digital silence under the whole window) must come out as exactly 0.  A case is
one (sr, n_fft, hop, n_mel) setting with all its utterances: n_fft / 2 + 1 samples (the shortest legal length), 1024,
1786 and 9000 (1024 is no legal length at n_fft = 2048 and is left out there).  Every figure is printed on a ``FEATNUM``
line before it is asserted.  The references of a case are computed once and shared.

The pipeline test reads the files of the two runs.  Pitch: the two pYIN runs decode the same bins on this corpus
(asserted).  The kernel and the float32 host reference round a bin's centre fmin * 2^(b / 240) differently in the last
place on some bins (tests/test_pyin_gpu.py compares bins for that reason), which moves the statistics and with them
every normalised entry, so the files cannot be bit-equal.  Instead: each run's files must hold exactly what the
pipeline's own steps give from that run's F0 track (cut, filled in, averaged; (x - mean) / std undone in float64); the
interpolation kernel on the host's track is bit for bit the host's contour; and the two contours are bit-equal on
every voiced frame whose two F0 values are bit-equal, within 3 ulps on the other voiced frames (two exp2
implementations of 1 ulp each, two products) and within 5 ulps of the largest value on the filled-in frames.  The statistics are compared in Hz within 4 * 2^-23 relative.
Mel and energy: the oracle is the float64 reference
on the samples ``load_utterance`` returns, cut and averaged as the pipeline does; a float32 energy file holds
(e - mean) / std rounded to float32, which de-normalised is off by up to 2^-23 (|e| + |mean|) on top of the
allowance."""
import functools
import json

import numpy as np
import pytest
import torch

from feature_corpus import (CASES, SPEAKER, config_for, interp_cases, np_interp, read_tree, signals, stft_of,
                            write_raw)
from pitch_signals import speechlike

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

MARGIN = 8.0
MEL_FLOOR = 4 * 2.0 ** -20
ENERGY_FLOOR = 4 * 2.0 ** -23
PITCH_RTOL = 4 * 2.0 ** -23


def features(xs, case, dtype, device="cpu", **kw):
    sr, n_fft, hop, n_mel = case
    stft = stft_of(case)
    wav = torch.cat([torch.from_numpy(x) for x in xs]).to(dtype).to(device)
    return ops.frame_features(wav, [len(x) for x in xs], n_fft, hop, stft.fft_window(device),
                              stft.mel_basis.to(device), **kw)


@functools.lru_cache(maxsize=None)
def references(case):
    xs = signals(case)
    r = {"xs": xs}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        r["m" + tag], r["e" + tag], r["frames"] = features(xs, case, dtype)
    return r


@functools.lru_cache(maxsize=None)
def hip_singles(case):
    outs = [features([x], case, torch.float32, "cuda") for x in references(case)["xs"]]
    return torch.cat([o[0] for o in outs]).cpu(), torch.cat([o[1] for o in outs]).cpu(), [o[2][0] for o in outs]


def rel_energy(e, e64):
    live = e64 > 0
    return float(((e.double() - e64)[live].abs() / e64[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("case", CASES)
def test_log_mel_and_energy_against_float64(case):
    sr, n_fft, hop, n_mel = case
    r = references(case)
    mel, energy, frames = hip_singles(case)
    assert frames == r["frames"] == [1 + len(x) // hop for x in r["xs"]]
    assert (n_fft // 2 + 1) in [len(x) for x in r["xs"]] and 9000 in [len(x) for x in r["xs"]]
    assert mel.dtype == energy.dtype == torch.float32 and mel.shape == r["m64"].shape == (sum(frames), n_mel)
    assert torch.isfinite(mel).all() and torch.isfinite(energy).all()
    ref_m, hip_m = float((r["m32"].double() - r["m64"]).abs().max()), float((mel.double() - r["m64"]).abs().max())
    ref_e, hip_e = rel_energy(r["e32"], r["e64"]), rel_energy(energy, r["e64"])
    dead = r["e64"] == 0
    print(f"FEATNUM case={case} frames={sum(frames)} silent_frames={int(dead.sum())}  max|log-mel - f64|: ref32 "
          f"{ref_m:.3e} hip {hip_m:.3e} allowed {max(MARGIN * ref_m, MEL_FLOOR):.3e}  max rel energy: ref32 {ref_e:.3e} "
          f"hip {hip_e:.3e} allowed {max(MARGIN * ref_e, ENERGY_FLOOR):.3e}")
    assert hip_m <= max(MARGIN * ref_m, MEL_FLOOR)
    assert hip_e <= max(MARGIN * ref_e, ENERGY_FLOOR)
    assert torch.all(energy[dead] == 0)


@pytest.mark.parametrize("case", CASES)
def test_packed_batch_is_bitwise_the_singles(case):
    xs = references(case)["xs"]
    mel1, energy1, frames1 = hip_singles(case)
    order = list(range(len(xs)))[::-1]
    mel, energy, frames = features([xs[i] for i in order], case, torch.float32, "cuda")
    assert frames == [frames1[i] for i in order]
    starts = np.concatenate([[0], np.cumsum(frames1)])
    rows = torch.cat([torch.arange(starts[i], starts[i + 1]) for i in order])
    assert torch.equal(mel.cpu(), mel1[rows]) and torch.equal(energy.cpu(), energy1[rows])
    again = features([xs[i] for i in order], case, torch.float32, "cuda")
    assert torch.equal(mel, again[0]) and torch.equal(energy, again[1])


@pytest.mark.parametrize("case", CASES)
def test_silence_and_clip_wave(case):
    sr, n_fft, hop, n_mel = case
    mel, energy, frames = features([np.zeros(1786), np.zeros(n_fft // 2 + 1)], case, torch.float32, "cuda")
    log_clip = torch.log(torch.tensor([1e-5], dtype=torch.float32))
    assert mel.shape[0] == sum(frames) and torch.all(mel.cpu() == log_clip) and torch.all(energy == 0)
    # the lengths of the case past speechlike's zero head (at 44100 Hz the short signals lie inside it), peak 1.5
    xs = [speechlike(5 + i, len(x) + sr // 10, sr)[sr // 10:] for i, x in enumerate(references(case)["xs"])]
    xs = [x * (1.5 / np.abs(x).max()) for x in xs]
    assert all(np.abs(x).max() > 1.4 for x in xs)
    a = features(xs, case, torch.float32, "cuda", clip_wave=True)
    b = features([np.clip(x.astype(np.float32), -1, 1) for x in xs], case, torch.float32, "cuda")
    c = features(xs, case, torch.float32, "cuda")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[1], c[1])


def test_value_errors_and_a_hand_made_basis():
    case = CASES[0]
    stft = stft_of(case)
    w, fb = stft.fft_window("cuda"), stft.mel_basis.cuda()
    x = torch.zeros(3000, device="cuda")
    with pytest.raises(ValueError, match="512"):
        ops.frame_features(x[:512], [512], 1024, 256, w, fb)  # N = n_fft / 2
    with pytest.raises(ValueError, match="hop"):
        ops.frame_features(x, [3000], 1024, 0, w, fb)
    with pytest.raises(ValueError, match="2999"):
        ops.frame_features(x, [2999], 1024, 256, w, fb)
    with pytest.raises(ValueError, match="1000"):
        ops.frame_features(x, [3000], 1000, 256, w, fb)
    # an all-zero row, a row with a hole and the last bin: the support table against the dense float64 projection
    hand = torch.zeros(4, 513)
    hand[0, 3:9] = 1.0
    hand[2, 100], hand[2, 200] = 0.5, 0.25
    hand[3, 512] = 1.0
    sig = torch.from_numpy(speechlike(7, 9000, 22050))
    mel, _, _ = ops.frame_features(sig.float().cuda(), [9000], 1024, 256, w, hand.cuda())
    want, _, _ = ops.frame_features(sig, [9000], 1024, 256, w.cpu(), hand)
    want32, _, _ = ops.frame_features(sig.float(), [9000], 1024, 256, w.cpu(), hand)
    ref_m, hip_m = float((want32.double() - want).abs().max()), float((mel.cpu().double() - want).abs().max())
    print(f"FEATNUM hand-made basis max|log-mel - f64|: ref32 {ref_m:.3e} hip {hip_m:.3e}")
    assert hip_m <= max(MARGIN * ref_m, MEL_FLOOR)
    assert torch.all(mel[:, 1].cpu() == torch.log(torch.tensor([1e-5], dtype=torch.float32)))


def test_interp_unvoiced_against_float64():
    cases = dict(interp_cases())
    rng = np.random.default_rng(9)
    gap = rng.uniform(80.0, 400.0, 700) * (rng.random(700) > 0.3)
    gap[150:450] = 0.0  # 300 unvoiced frames across two chunk carries, voiced on both sides
    gap[149], gap[450] = 111.1, 333.3
    cases["700 frames, a gap of 300"] = gap
    singles = {}
    for name, f0 in cases.items():
        got, nv = ops.interp_unvoiced(torch.from_numpy(f0).float().cuda(), [len(f0)])
        x32 = f0.astype(np.float32).astype(np.float64)
        want = np_interp(x32)
        got = got.cpu()
        singles[name] = got
        err = float(np.max(np.abs(got.double().numpy() - want) / np.maximum(np.abs(want), 1e-30))) if len(f0) else 0.0
        print(f"FEATNUM interp case={name!r} frames={len(f0)} voiced={int(nv[0])} max rel error {err:.3e}")
        assert got.dtype == torch.float32 and nv.dtype == torch.int32
        assert nv.tolist() == [int(np.count_nonzero(f0))], name
        assert np.all(np.abs(got.double().numpy() - want) <= PITCH_RTOL * np.abs(want)), name
        # and bit for bit the float32 host reference
        assert torch.equal(got, ops.interp_unvoiced(torch.from_numpy(f0).float(), [len(f0)])[0]), name
    names = ["700 frames, a gap of 300", "none", "leading and trailing runs"]
    packed = torch.from_numpy(np.concatenate([cases[n] for n in names])).float().cuda()
    got, nv = ops.interp_unvoiced(packed, [len(cases[n]) for n in names])
    assert torch.equal(got.cpu(), torch.cat([singles[n] for n in names]))
    assert nv.tolist() == [int(np.count_nonzero(cases[n])) for n in names]


def hz_stats(st):
    """[min, max, mean, std] of a normalised contour -> min and max in Hz, mean, std."""
    return [st[0] * st[3] + st[2], st[1] * st[3] + st[2], st[2], st[3]]


def bins_of(f0):
    f = f0.double()
    b = torch.round(12 * 20 * torch.log2(f.clamp(min=1.0) / 71.0)).long()
    return torch.where(f > 0, b, torch.full_like(b, -1))


@pytest.mark.parametrize("source", ["learned", "textgrid"])
def test_pipeline_on_the_gpu_against_the_cpu_device(source, tmp_path):
    from speakingstyle_amd.data.preprocess import Preprocessor, phoneme_average

    config, n = write_raw(tmp_path, source)
    trees, cfgs = {}, {}
    for device in ("cpu", "cuda"):
        cfgs[device] = config_for(config, n, tmp_path / device)
        assert len(Preprocessor(cfgs[device], device=device).build_from_path(workers=1)) == 6
        trees[device] = read_tree(tmp_path / device)
    cpu, gpu = trees["cpu"], trees["cuda"]
    assert sorted(cpu) == sorted(gpu)
    for name in ("train.txt", "val.txt", "speakers.json"):
        assert cpu[name] == gpu[name], name
    sc, sg = json.loads(cpu["stats.json"]), json.loads(gpu["stats.json"])
    pre = Preprocessor(cfgs["cuda"])
    pp = config["preprocessing"]
    hop, sr = pp["stft"]["hop_length"], pp["audio"]["sampling_rate"]
    window, basis = pre.stft.fft_window("cpu"), pre.stft.mel_basis
    kept = [line.split("|")[0] for line in (cpu["train.txt"] + cpu["val.txt"]).strip().split("\n")]
    assert len(kept) == 6
    fig = {"ref_m": 0.0, "hip_m": 0.0, "ref_e": 0.0, "hip_e": 0.0, "fmt": 0.0, "pitch": 0.0, "same": 0, "voiced": 0}
    e_ok = True
    for base in sorted(kept):
        _, wav, duration, _ = pre.load_utterance(SPEAKER, base)
        x = torch.from_numpy(wav)
        # the two pYIN runs decode the same bins on this corpus
        f_cpu = ops.pyin(x, [len(x)], sr, hop)[0]
        f_gpu = ops.pyin(x.cuda(), [len(x)], sr, hop)[0].cpu()
        assert torch.equal(bins_of(f_cpu), bins_of(f_gpu)), base
        # What each run must have written, from its own F0 track with the pipeline's own steps: cut to T, fill the
        # unvoiced frames (the kernel on the GPU side), average per phoneme where the config says so.
        T = len(f_cpu) if duration is None else sum(duration)
        want = {}
        for side, f in (("cpu", f_cpu[:T].contiguous()), ("cuda", f_gpu[:T].contiguous().cuda())):
            g = ops.interp_unvoiced(f, [T])[0].cpu()
            want[side] = g if duration is None or pre.pitch_phoneme else f.cpu()
        # the interpolation kernel on the host's own track: bit for bit the host's contour
        assert torch.equal(ops.interp_unvoiced(f_cpu[:T].contiguous().cuda(), [T])[0].cpu(),
                           ops.interp_unvoiced(f_cpu[:T].contiguous(), [T])[0])
        # the two contours: bit-equal on every voiced frame whose two F0 values are bit-equal; within 3 ulps (3 * 2^-23
        # relative) on the other voiced frames -- a bin centre is fmin * exp2(b / 240): the device's exp2f and the
        # host's exp2 are each good to 1 ulp and each product rounds by half an ulp --; and within 5 ulps of the
        # largest value on the filled-in frames (two such end points, three roundings of half an ulp)
        gc, gg = want["cpu"].double().numpy(), want["cuda"].double().numpy()
        fc, fg = f_cpu[:T].numpy(), f_gpu[:T].numpy()
        same = (fc == fg) & (fc > 0)
        fig["same"] += int(same.sum())
        fig["voiced"] += int((fc > 0).sum())
        assert np.array_equal(gc[same], gg[same]), base
        voiced = fc > 0
        assert np.all(np.abs(gc - gg)[voiced] <= 3 * 2.0 ** -23 * gc[voiced]), base
        assert np.all(np.abs(gc - gg) <= 5 * 2.0 ** -23 * gc.max()), base
        fig["pitch"] = max(fig["pitch"], float(np.max(np.abs(gc - gg) / np.maximum(gc, 1e-30))))
        # the files hold exactly these values: (x - mean) / std in float64, undone here (a few 2^-53 of |x| + |mean|)
        for side, tree, st in (("cpu", cpu, sc), ("cuda", gpu, sg)):
            px = want[side].double().numpy()
            if duration is not None and pre.pitch_phoneme:
                px = phoneme_average(px, duration)
            got = tree[f"pitch/{SPEAKER}-pitch-{base}.npy"]
            assert got.dtype == np.float64 and got.shape == px.shape, (base, side)
            assert np.all(np.abs(got * st["pitch"][3] + st["pitch"][2] - px)
                          <= 2.0 ** -48 * (np.abs(px) + st["pitch"][2])), (base, side)
        if duration is not None:
            assert np.array_equal(cpu[f"duration/{SPEAKER}-duration-{base}.npy"],
                                  gpu[f"duration/{SPEAKER}-duration-{base}.npy"])
        m64, e64, _ = ref.frame_features(x.double(), [len(x)], pre.stft.n_fft, hop, window, basis, clip_wave=True)
        m32, e32, _ = ref.frame_features(x, [len(x)], pre.stft.n_fft, hop, window, basis, clip_wave=True)
        T = m64.shape[0] if duration is None else sum(duration)
        mel = gpu[f"mel/{SPEAKER}-mel-{base}.npy"]
        assert mel.shape == (T, 80) and mel.dtype == np.float32
        fig["ref_m"] = max(fig["ref_m"], float((m32[:T].double() - m64[:T]).abs().max()))
        fig["hip_m"] = max(fig["hip_m"], float(np.abs(mel.astype(np.float64) - m64[:T].numpy()).max()))
        e64, e32 = e64[:T].numpy(), e32[:T].numpy()
        if pre.energy_phoneme and duration is not None:
            e64, e32 = phoneme_average(e64, duration), phoneme_average(e32, duration)
        file = gpu[f"energy/{SPEAKER}-energy-{base}.npy"]
        e = file.astype(np.float64) * sg["energy"][3] + sg["energy"][2]
        fmt = 2.0 ** -23 * (np.abs(e64) + abs(sg["energy"][2])) if file.dtype == np.float32 else 0.0 * e64
        live = e64 > 0
        ref_e = float(np.max(np.abs(e32 - e64)[live] / e64[live]))
        fig["ref_e"] = max(fig["ref_e"], ref_e)
        fig["hip_e"] = max(fig["hip_e"], float(np.max(np.abs(e - e64)[live] / e64[live])))
        fig["fmt"] = max(fig["fmt"], float(np.max((fmt / np.maximum(e64, 1e-30))[live])))
        e_ok &= bool(np.all(np.abs(e - e64) <= max(MARGIN * ref_e, ENERGY_FLOOR) * e64 + fmt + 1e-300))
    stat_p = max(abs(a - b) / abs(a) for a, b in zip(hz_stats(sc["pitch"]), hz_stats(sg["pitch"])))
    print(f"FEATNUM pipeline source={source}  voiced frames {fig['voiced']}, F0 bit-equal on {fig['same']}; max rel pitch "
          f"contour (Hz) cuda - cpu {fig['pitch']:.3e} stats {stat_p:.3e}  "
          f"max|log-mel - f64|: ref32 {fig['ref_m']:.3e} hip {fig['hip_m']:.3e}  "
          f"max rel energy: ref32 {fig['ref_e']:.3e} hip {fig['hip_e']:.3e} (of which the float32 file's rounding up to "
          f"{fig['fmt']:.3e})  stats cpu {sc} gpu {sg}")
    assert stat_p <= PITCH_RTOL
    assert fig["hip_m"] <= max(MARGIN * fig["ref_m"], MEL_FLOOR)
    assert e_ok
