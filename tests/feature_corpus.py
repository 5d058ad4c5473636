"""Cases, signals and a tiny raw corpus for the feature tests (tests/test_features_cpu.py, ..._gpu.py): six tone sequences
under 1 s (``prosody_signals.rendered_pair``), with learned durations also an utterance shorter than its transcript and
a silent one (both dropped).  Functions of their arguments alone."""
import json
import os

import numpy as np

from pitch_signals import short, speechlike
from prosody_signals import rendered_pair

SR = 22050
SPEAKER = "LJSpeech"
PHONES = ["HH", "AH0", "L", "OW1", "W", "ER1", "L", "D"]


def _textgrid(path, phones, dur_s, lead=0.05):
    t = lead
    ivs = [(0.0, lead, "sil")]
    for p in phones:
        ivs.append((t, t + dur_s, p))
        t += dur_s
    ivs.append((t, t + 0.02, "sp"))
    xmax = t + 0.02
    lines = ['File type = "ooTextFile"', 'Object class = "TextGrid"', "", "xmin = 0", f"xmax = {xmax}", "tiers? <exists>",
             "size = 1", "item []:", "    item [1]:", '        class = "IntervalTier"', '        name = "phones"',
             "        xmin = 0", f"        xmax = {xmax}", f"        intervals: size = {len(ivs)}"]
    for i, (a, b, p) in enumerate(ivs, 1):
        lines += [f"        intervals [{i}]:", f"            xmin = {a}", f"            xmax = {b}", f'            text = "{p}"']
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def write_raw(root, source):
    """raw/<speaker>/U00i.wav + .lab under ``root`` -> the normalised preprocess config (pyin; ``source``: "learned" |
    "textgrid"), its preprocessed_path still to be set by ``config_for``."""
    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.config import config_dir_triplet, load_yaml, normalize_preprocess_config

    raw = os.path.join(str(root), "raw", SPEAKER)
    os.makedirs(raw, exist_ok=True)
    wavs = [rendered_pair(40 + i, n_tok=5)["x"]["wav"] for i in range(6)]
    assert all(0.5 * SR < len(w) < SR for w in wavs)
    if source == "learned":
        wavs.append(wavs[0][:SR // 20])           # 5 frames for a transcript of more phones: "short"
        wavs.append(np.zeros(SR // 2, np.float32))  # no voiced frame
    for i, w in enumerate(wavs):
        write_wav(os.path.join(raw, f"U{i:03d}.wav"), SR, (w * 32767).astype(np.int16))
        with open(os.path.join(raw, f"U{i:03d}.lab"), "w") as f:
            f.write(f"hello world {i}")
    p = load_yaml(config_dir_triplet("LJSpeech_unaligned" if source == "learned" else "LJSpeech")[0])
    p["path"]["raw_path"] = os.path.join(str(root), "raw")
    p["preprocessing"]["val_size"] = 2
    p["preprocessing"]["pitch"]["extractor"] = "pyin"
    return normalize_preprocess_config(p), len(wavs)


def config_for(config, n_utts, out_dir):
    """A copy of ``config`` that writes to ``out_dir`` (with the TextGrids a TextGrid config reads from there)."""
    cfg = json.loads(json.dumps(config))
    cfg["path"]["preprocessed_path"] = str(out_dir)
    if cfg["preprocessing"]["duration"]["source"] != "learned":
        d = os.path.join(str(out_dir), "TextGrid", SPEAKER)
        os.makedirs(d, exist_ok=True)
        for i in range(n_utts):
            _textgrid(os.path.join(d, f"U{i:03d}.TextGrid"), PHONES, 0.055 + 0.001 * i)
    return cfg


def read_tree(out_dir):
    """{relative path: array | text} of everything a run wrote (the TextGrids aside)."""
    tree = {}
    for d, _, files in os.walk(str(out_dir)):
        if os.path.basename(os.path.dirname(d)) == "TextGrid" or os.path.basename(d) == "TextGrid":
            continue
        for fn in files:
            p = os.path.join(d, fn)
            rel = os.path.relpath(p, str(out_dir))
            tree[rel] = np.load(p) if fn.endswith(".npy") else open(p, encoding="utf-8").read()
    return tree


# ------------------------------------------------------------------ kernel cases (sr, n_fft, hop, n_mel) and signals
CASES = [(22050, 1024, 256, 80), (16000, 1024, 200, 80), (8000, 512, 100, 40), (44100, 2048, 512, 80)]


def stft_of(case):
    from speakingstyle_amd.audio.stft import TacotronSTFT

    sr, n_fft, hop, n_mel = case
    return TacotronSTFT(n_fft, hop, n_fft, n_mel, sr, 0.0, min(8000.0, sr / 2))


def signals(case):
    sr, n_fft = case[0], case[1]
    return [(short(n, n, sr) if n < 5000 else speechlike(n % 97, n, sr)) for n in (n_fft // 2 + 1, 1024, 1786, 9000)
            if n > n_fft // 2]


def np_interp(f0):
    from speakingstyle_amd.data.preprocess import interpolate_unvoiced

    return interpolate_unvoiced(np.asarray(f0, dtype=np.float64))


def interp_cases():
    rng = np.random.default_rng(5)
    mixed = rng.uniform(80.0, 400.0, 90) * (rng.random(90) > 0.5)
    mixed[:7] = 0.0
    mixed[-9:] = 0.0
    ends = np.zeros(40)
    ends[0], ends[-1] = 123.4, 321.7
    one = np.zeros(33)
    one[11] = 200.3
    return {"none": np.zeros(25), "one voiced": one, "ends only": ends, "leading and trailing runs": mixed,
            "one frame": np.array([150.2]), "one unvoiced frame": np.array([0.0])}
