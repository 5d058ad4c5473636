"""The packed feature ops on host tensors (``ops.frame_features`` / ``ops.interp_unvoiced`` = ``ops.reference``), the
host tables of their kernels (csrc/k_features.hip) and the batched ``Preprocessor(device="cpu")`` against the
per-utterance path on a tiny corpus.

Pitch files and ``stats.json`` of the two paths differ by one float32 interpolation against float64 ``np.interp``:
4 * 2^-23 relative on the contour in Hz.  A normalised file holds (g - mean) / std, where that error is no longer
relative to the value (it is arbitrarily large relative to an entry near 0), so the files and the min / max entries are
compared in Hz, each side de-normalised with its own mean / std; mean and std themselves are compared directly."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from feature_corpus import CASES, config_for, interp_cases, np_interp, read_tree, signals, stft_of, write_raw

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PITCH_RTOL = 4 * 2.0 ** -23
@pytest.mark.parametrize("case", CASES)
def test_frame_features_is_tacotron_stft_per_utterance(case):
    sr, n_fft, hop, n_mel = case
    stft = stft_of(case)
    xs = [torch.from_numpy(x).float() for x in signals(case)]
    lens = [len(x) for x in xs]
    window, basis = stft.fft_window("cpu"), stft.mel_basis
    mel, energy, frames = ops.frame_features(torch.cat(xs), lens, n_fft, hop, window, basis)
    assert frames == [1 + n // hop for n in lens] and mel.shape == (sum(frames), n_mel) and mel.is_contiguous()
    want = [stft.mel_spectrogram(x.unsqueeze(0)) for x in xs]
    assert torch.equal(mel, torch.cat([m[0].t() for m, _ in want]))
    assert torch.equal(energy, torch.cat([e[0] for _, e in want]))
    # clip_wave is the host clip
    loud = torch.cat(xs) * 3.0
    a = ops.frame_features(loud, lens, n_fft, hop, window, basis, clip_wave=True)
    b = ops.frame_features(loud.clamp(-1, 1), lens, n_fft, hop, window, basis)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # float32 against its own float64 run.  A transform of n points in a format of unit roundoff u has
    # ||dX||_2 <= c log2(n) u ||X||_2; c = 4 covers the window product, |.| and the projection's sums.  The energy is
    # ||X||_2 of the one-sided spectrum (||X||_2 of the whole one is at most sqrt(2) of it), a mel entry moves by at
    # most its filter's row sum times ||dX||_2, and log / exp move it by a few u of itself.
    mel64, energy64, _ = ops.frame_features(torch.cat(xs).double(), lens, n_fft, hop, window, basis)
    assert mel64.dtype == energy64.dtype == torch.float64
    u = 2.0 ** -24
    dx = 4 * np.log2(n_fft) * u * np.sqrt(2.0) * energy64
    assert torch.all((energy.double() - energy64).abs() <= dx)
    lin, lin64 = torch.exp(mel.double()), torch.exp(mel64)
    bound = basis.double().sum(1).unsqueeze(0) * dx.unsqueeze(1) + 32 * u * lin64
    assert torch.all((lin - lin64).abs() <= bound)


def test_frame_features_value_errors():
    stft = stft_of(CASES[0])
    w, fb = stft.fft_window("cpu"), stft.mel_basis
    x = torch.zeros(3000)
    with pytest.raises(ValueError, match="512"):
        ops.frame_features(x[:512], [512], 1024, 256, w, fb)
    with pytest.raises(ValueError, match="hop"):
        ops.frame_features(x, [3000], 1024, 0, w, fb)
    with pytest.raises(ValueError, match="2999"):
        ops.frame_features(x, [2999], 1024, 256, w, fb)
    with pytest.raises(ValueError, match="1000"):
        ops.frame_features(x, [3000], 1000, 256, w, fb)


def test_interp_unvoiced_is_np_interp_in_float64():
    cases = interp_cases()
    for name, f0 in cases.items():
        got, nv = ops.interp_unvoiced(torch.from_numpy(f0), [len(f0)])
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), np_interp(f0)), name
        assert nv.dtype == torch.int32 and nv.tolist() == [int(np.count_nonzero(f0))], name
    packed = np.concatenate(list(cases.values()))
    got, nv = ops.interp_unvoiced(torch.from_numpy(packed), [len(v) for v in cases.values()])
    assert np.array_equal(got.numpy(), np.concatenate([np_interp(v) for v in cases.values()]))
    assert nv.tolist() == [int(np.count_nonzero(v)) for v in cases.values()]
    with pytest.raises(ValueError, match="frames"):
        ops.interp_unvoiced(torch.zeros(5), [4])


def check_support(basis):
    supp = ref.mel_support(basis)
    assert supp.dtype == torch.int32 and supp.shape == (basis.shape[0], 2)
    for m, (lo, hi) in enumerate(supp.tolist()):
        nz = torch.nonzero(basis[m]).flatten().tolist()
        if nz:
            assert (lo, hi) == (nz[0], nz[-1] + 1), m  # every non-zero inside, and no wider than that
        else:
            assert lo == hi, m
    return supp


def test_support_table_covers_every_shipped_basis_and_hand_made_ones():
    from speakingstyle_amd.audio.stft import TacotronSTFT
    from speakingstyle_amd.config import load_yaml, normalize_preprocess_config

    paths = sorted(glob.glob(os.path.join(ROOT, "config", "*", "preprocess.yaml")))
    assert len(paths) >= 7
    seen = set()
    for p in paths:
        pp = normalize_preprocess_config(load_yaml(p))["preprocessing"]
        key = (pp["stft"]["filter_length"], pp["stft"]["hop_length"], pp["stft"]["win_length"],
               pp["mel"]["n_mel_channels"], pp["audio"]["sampling_rate"], pp["mel"]["mel_fmin"], pp["mel"]["mel_fmax"])
        if key in seen:
            continue
        seen.add(key)
        basis = TacotronSTFT(*key).mel_basis
        supp = check_support(basis)
        contiguous = all(bool((basis[m, lo:hi] != 0).all()) for m, (lo, hi) in enumerate(supp.tolist()))
        assert contiguous, key  # the slaney triangles have no hole
    for case in CASES:
        check_support(stft_of(case).mel_basis)
    hand = torch.zeros(4, 513)
    hand[0, 3:9] = 1.0
    hand[2, 100] = 0.5   # row 2: a hole between 100 and 200
    hand[2, 200] = 0.25
    hand[3, 512] = 1.0   # the last bin; row 1 stays all zero
    assert check_support(hand).tolist() == [[3, 9], [0, 0], [100, 201], [512, 513]]
    # the projection over the supports alone is the dense one
    mag = torch.rand(513, dtype=torch.float64)
    dense = hand.double() @ mag
    sparse = torch.stack([(hand[m, lo:hi].double() * mag[lo:hi]).sum() for m, (lo, hi) in
                          enumerate(ref.mel_support(hand).tolist())])
    assert torch.allclose(dense, sparse, rtol=1e-15, atol=0)


def test_pair_table_gives_each_frame_row_once():
    hop = 256
    lens = [513, 1024, 1786, 9000, 256 * 7]  # 3, 5, 7, 36 and 8 frame rows: odd tails and an even one
    frames = [1 + n // hop for n in lens]
    assert frames == [3, 5, 7, 36, 8]
    tab = ref.frame_pairs(lens, frames)
    assert tab.dtype == torch.int32 and tab.shape == (sum((f + 1) // 2 for f in frames), 6)
    off = np.concatenate([[0], np.cumsum(lens)])
    cu = np.concatenate([[0], np.cumsum(frames)])
    rows_seen, tails = [], 0
    for lo, hi, n, first, row, rows in tab.tolist():
        b = int(np.searchsorted(off, lo + (hi << 32), side="right")) - 1
        assert (lo + (hi << 32), n) == (off[b], lens[b])
        assert first % 2 == 0 and rows in (1, 2) and row == cu[b] + first
        assert first + rows <= frames[b]  # never pairs across utterances
        assert rows == 2 or first == frames[b] - 1  # only a last odd row stands alone
        tails += rows == 1
        rows_seen += list(range(row, row + rows))
    assert rows_seen == list(range(sum(frames))) and tails == 3
    # offsets past 2^32 samples keep both words
    big = ref.frame_pairs([3_000_000_000, 600], [1, 3])
    assert [(int(e[0]) & 0xFFFFFFFF) + (int(e[1]) << 32) for e in big] == [0, 3_000_000_000, 3_000_000_000]


@pytest.fixture(scope="module", params=["learned", "textgrid"])
def runs(request, tmp_path_factory):
    """The per-utterance path and ``device="cpu"`` on the same raw corpus -> (source, config, host tree, cpu tree)."""
    from speakingstyle_amd.data.preprocess import Preprocessor

    root = tmp_path_factory.mktemp("features_" + request.param)
    config, n = write_raw(root, request.param)
    trees = []
    for name, device in (("host", None), ("cpu", "cpu")):
        cfg = config_for(config, n, root / name)
        out = Preprocessor(cfg, device=device).build_from_path(workers=1)
        assert len(out) == 6
        trees.append(read_tree(root / name))
    return request.param, config, trees[0], trees[1]


def hz(v, stats):
    return np.asarray(v, dtype=np.float64) * stats[3] + stats[2]


def assert_pitch_close(a, b, sa, sb, what):
    a, b = hz(a, sa), hz(b, sb)
    assert a.shape == b.shape and np.all(np.abs(a - b) <= PITCH_RTOL * np.abs(a)), what


def test_batched_cpu_pipeline_against_the_per_utterance_path(runs):
    source, config, host, cpu = runs
    assert sorted(host) == sorted(cpu)
    kinds = {os.path.dirname(k) for k in host}
    assert kinds == {"", "mel", "pitch", "energy"} | (set() if source == "learned" else {"duration"})
    assert sum(k.startswith("mel") for k in host) == 6
    for name in ("train.txt", "val.txt", "speakers.json"):
        assert host[name] == cpu[name], name
    sh, sc = json.loads(host["stats.json"]), json.loads(cpu["stats.json"])
    assert sh["energy"] == sc["energy"]
    for k in (2, 3):
        assert abs(sh["pitch"][k] - sc["pitch"][k]) <= PITCH_RTOL * abs(sh["pitch"][k])
    assert_pitch_close(sh["pitch"][:2], sc["pitch"][:2], sh["pitch"], sc["pitch"], "stats min / max")
    for rel, a in host.items():
        b = cpu[rel]
        if rel.startswith(("mel", "energy", "duration")):
            assert a.dtype == b.dtype and np.array_equal(a, b), rel
        elif rel.startswith("pitch"):
            assert a.dtype == b.dtype == np.float64
            assert_pitch_close(a, b, sh["pitch"], sc["pitch"], rel)


def test_batched_pipeline_in_small_batches_is_the_same(tmp_path, monkeypatch):
    """Batches of 4 utterances instead of one batch: the same files bit for bit (an utterance does not depend on its
    batch)."""
    from speakingstyle_amd.data.preprocess import Preprocessor

    config, n = write_raw(tmp_path, "learned")
    trees = []
    for name, size in (("one", 64), ("split", 4)):
        monkeypatch.setattr(Preprocessor, "BATCH_UTTERANCES", size)
        pre = Preprocessor(config_for(config, n, tmp_path / name), device="cpu")
        assert len(pre.build_from_path(workers=1)) == 6
        assert all(v >= 0 for v in pre.timings.values()) and pre.timings["kernels"] > 0
        trees.append(read_tree(tmp_path / name))
    assert sorted(trees[0]) == sorted(trees[1])
    for rel, a in trees[0].items():
        assert np.array_equal(a, trees[1][rel]) if isinstance(a, np.ndarray) else a == trees[1][rel], rel


def test_dio_with_a_device_names_the_key(tmp_path):
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.preprocess import Preprocessor

    pp = load_named("LJSpeech")[0]
    assert pp["preprocessing"]["pitch"].get("extractor", "dio") == "dio"
    pp["path"]["raw_path"] = str(tmp_path / "does_not_exist")  # nothing is read before the error
    with pytest.raises(ValueError, match=r"preprocessing\.pitch\.extractor"):
        Preprocessor(pp, device="cpu")
    Preprocessor(pp)  # the host path takes dio as before
