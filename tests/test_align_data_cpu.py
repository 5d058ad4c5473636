"""``preprocessing.duration.source: learned`` from wavs and transcripts alone, on a tiny generated corpus:
prepare_align -> Preprocessor.build_from_path (no TextGrids) -> Dataset / collate / to_device (no durations) ->
a real-data training step and a validation pass through the alignment learner."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name):  # by path: the session-scoped reference fixture may shadow same-named top-level modules
    spec = importlib.util.spec_from_file_location("ssamd_cli_" + name, os.path.join(ROOT, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.config import config_dir_triplet, load_yaml

    root = tmp_path_factory.mktemp("unaligned")
    src = root / "LJ"
    (src / "wavs").mkdir(parents=True)
    sr = 22050
    meta = []
    for i in range(7):
        # utterance 6 is 0.05 s (5 frames) for a transcript of more phones than that: it must be dropped
        t = np.arange(int(sr * (0.05 if i == 6 else 0.9 + 0.05 * i))) / sr
        wav = 0.4 * np.sin(2 * np.pi * (110 + 10 * i) * t) * (1 + 0.3 * np.sin(2 * np.pi * 3 * t))
        write_wav(str(src / "wavs" / f"LJ{i:03d}.wav"), sr, (wav * 32767).astype(np.int16))
        meta.append(f"LJ{i:03d}|Hello world {i}.|Hello world {i}.")
    (src / "metadata.csv").write_text("\n".join(meta) + "\n")
    p = load_yaml(config_dir_triplet("LJSpeech_unaligned")[0])
    assert p["preprocessing"]["duration"]["source"] == "learned"
    p["dataset"] = "LJSpeech"  # the corpus layout prepare_align reads
    p["path"].update(corpus_path=str(src), raw_path=str(root / "raw"), preprocessed_path=str(root / "pre"))
    p["preprocessing"]["val_size"] = 2
    pf = root / "preprocess.yaml"
    pf.write_text(yaml.safe_dump(p))
    assert _load("prepare_align").main([str(pf)]) == 7
    out = _load("preprocess").main(["--preprocess_config", str(pf), "--workers", "1"])
    return root, pf, out


def test_preprocess_without_textgrids(corpus, capsys):
    from speakingstyle_amd.text import text_to_sequence

    root, pf, out = corpus
    assert len(out) == 6  # the 5-frame utterance has fewer frames than phones
    assert not (root / "pre" / "duration").exists() and not (root / "pre" / "TextGrid").exists()
    stats = json.load(open(root / "pre" / "stats.json"))
    assert len(stats["pitch"]) == 4 and stats["pitch"][0] < stats["pitch"][1]
    lines = (root / "pre" / "train.txt").read_text().strip().split("\n")
    assert len(lines) == 4 and len((root / "pre" / "val.txt").read_text().strip().split("\n")) == 2
    base, spk, text, raw = lines[0].split("|", 3)
    # the phones are the text frontend's, i.e. what synthesis feeds the model for the same transcript
    from speakingstyle_amd.text import g2p

    lexicon = g2p.load_lexicon(yaml.safe_load(pf.read_text())["path"]["lexicon_path"], "en")
    assert text == "{" + " ".join(g2p.english_to_phones(raw, lexicon)) + "}" and raw.startswith("hello world")
    assert text.startswith("{HH ") and " W ER1 L D " in text
    mel = np.load(root / "pre" / "mel" / f"{spk}-mel-{base}.npy")
    pitch = np.load(root / "pre" / "pitch" / f"{spk}-pitch-{base}.npy")
    energy = np.load(root / "pre" / "energy" / f"{spk}-energy-{base}.npy")
    # whole utterance, frame-level contours
    assert mel.shape[1] == 80 and pitch.shape == energy.shape == (mel.shape[0],)
    assert mel.shape[0] >= len(text_to_sequence(text, ["english_cleaners"]))
    assert not any("LJ006" in x for x in out)


def test_config_enum():
    from speakingstyle_amd.config import ConfigError, normalize_preprocess_config

    assert normalize_preprocess_config({})["preprocessing"]["duration"]["source"] == "textgrid"
    with pytest.raises(ConfigError):
        normalize_preprocess_config({"preprocessing": {"duration": {"source": "mfa"}}})


def test_dataset_step_and_validation_without_durations(corpus):
    from speakingstyle_amd.benchmark import tiny_overrides
    from speakingstyle_amd.config import load_configs, load_named
    from speakingstyle_amd.data.dataset import Dataset, to_device
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.train.evaluate import evaluate
    from speakingstyle_amd.train.trainer import Trainer

    root, pf, _ = corpus
    _, mc, tc = load_named("LJSpeech_unaligned")
    pp = load_configs(str(pf), mc, tc)[0]
    tiny_overrides(mc)
    tc["optimizer"]["batch_size"] = 2
    ds = Dataset("train.txt", pp, tc, sort=True, drop_last=True)
    batches = ds.collate_fn([ds[i] for i in range(4)])
    assert len(batches) == 2 and all(len(b) == 12 and b[11] is None for b in batches)
    b = to_device(batches[0], "cpu")
    assert b[11] is None and b[9].shape == b[6].shape[:2] and b[10].dtype == torch.float32
    assert list(b[4].host_lengths) == b[4].tolist() and list(b[7].host_lengths) == b[7].tolist()
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc)
    tr = Trainer(model, (pp, mc, tc))
    losses, output, _ = tr.train_step(b)
    assert len(losses) == 8 and all(torch.isfinite(torch.as_tensor(v)).all() for v in losses)
    assert torch.equal(output[5].sum(1).long(), b[7])
    vals = tr.reduce_losses(losses)
    assert len(vals) == 7 and vals[6] == pytest.approx(float(losses[7].detach()), rel=1e-6)
    assert vals[0] == pytest.approx(float(losses[0].detach()), rel=1e-5)
    model.eval()
    msg = evaluate(model, 1, (pp, mc, tc))
    assert "Align Loss" in msg
