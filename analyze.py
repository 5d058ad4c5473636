#!/usr/bin/env python
"""Research tooling CLI (the reference's notebooks as commands).

  variance distributions, ground truth vs predictions (notebooks/variance_control_distbn.ipynb):
    python analyze.py variance --restore_step 900000 -p P -m M -t T [--source val.txt] [--out_dir analysis]
        [--pitch_control 1.2 --energy_control 1 --duration_control 1] [--outlier_k 3]
  one-batch forward / style-encoder inspection (notebooks/ref_encoder.ipynb):
    python analyze.py inspect --restore_step 0 -p P -m M -t T [--synthetic]
  objective metrics of free-running synthesis against the recordings (MCD, F0 / energy error along a DTW path):
    python analyze.py objective --restore_step 900000 -p P -m M -t T [--source val.txt] [--out_dir analysis]
        [--pitch_control 1 --energy_control 1 --duration_control 1] [--n_ceps 13] [--batch_size 32] [--cpu]
        [--wave [--vocoder griffin_lim] [--pitch_tracker pyin]]   (pitch and MCD of the vocoded audio against the
                                                                   recordings)
  style map of a corpus (exact t-SNE + k-means of the style embeddings; exemplars to annotate for tune_style.py):
    python analyze.py style --restore_step 900000 -p P -m M -t T [--source train.txt] [--out_dir analysis]
        [--space film|query|weights] [--clusters K] [--perplexity 30] [--iters 750] [--max_utts 16384]
        [--like x.wav --top 10] [--seed 1234] [--cpu]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("command", choices=["variance", "inspect", "objective", "style"])
    ap.add_argument("--restore_step", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1234, help="parameter init seed (restore_step 0: reproducible runs)")
    ap.add_argument("-p", "--preprocess_config", required=True)
    ap.add_argument("-m", "--model_config", required=True)
    ap.add_argument("-t", "--train_config", required=True)
    ap.add_argument("--source", default=None, help="metadata list (default: <preprocessed_path>/val.txt)")
    ap.add_argument("--out_dir", default=None)
    ap.add_argument("--pitch_control", type=float, default=1.0)
    ap.add_argument("--energy_control", type=float, default=1.0)
    ap.add_argument("--duration_control", type=float, default=1.0)
    ap.add_argument("--outlier_k", type=float, default=3.0)
    ap.add_argument("--batch_size", type=int, default=None, help="default: 8 (variance), 32 (objective)")
    ap.add_argument("--n_ceps", type=int, default=13, help="objective: mel cepstra 1 .. n_ceps enter the MCD")
    ap.add_argument("--wave", action="store_true",
                    help="objective: also vocode every synthesis and compare it with the recording "
                         "(<raw_path>/<speaker>/<basename>.wav): wave_mcd_db, wave_vde, wave_gpe, wave_ffe, "
                         "wave_f0_rmse_cents")
    ap.add_argument("--vocoder", choices=["griffin_lim", "hifigan"], default=None,
                    help="objective --wave: the vocoder (default: the model config's; griffin_lim needs no checkpoint)")
    ap.add_argument("--pitch_tracker", choices=["yin", "pyin"], default="yin",
                    help="objective --wave: the F0 tracker of both waveforms (pyin: probabilistic YIN, one smooth "
                         "track per utterance; keeps the voiced frames of noisy vocoded audio that yin drops)")
    ap.add_argument("--space", choices=["film", "query", "weights"], default="film",
                    help="style: the embedding (film: gamma || beta; query / weights: GST only)")
    ap.add_argument("--clusters", type=int, default=None,
                    help="style: k of k-means (default: the model's n_style_token with GST, else 10)")
    ap.add_argument("--perplexity", type=float, default=30.0,
                    help="style: t-SNE perplexity, clamped to (N - 1) / 3; the value used is reported")
    ap.add_argument("--iters", type=int, default=750, help="style: t-SNE iterations")
    ap.add_argument("--max_utts", type=int, default=16384,
                    help="style: a larger corpus is subsampled with --seed (exact t-SNE holds 16384 points)")
    ap.add_argument("--like", default=None, help="style: a wav whose nearest utterances in the style space are listed")
    ap.add_argument("--top", type=int, default=10, help="style: neighbours of --like to list")
    ap.add_argument("--synthetic", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    return ap


def main(argv=None):
    a = build_parser().parse_args(argv)

    import torch

    from speakingstyle_amd.config import load_configs
    from speakingstyle_amd.utils.model import get_model

    configs = load_configs(a.preprocess_config, a.model_config, a.train_config)
    dev = torch.device("cuda" if torch.cuda.is_available() and not a.cpu else "cpu")
    torch.manual_seed(a.seed)
    model = get_model(a.restore_step, configs, dev, train=False, ignore_layers=configs[2].get("ignore_layers", []))
    if a.command == "variance":
        from speakingstyle_amd.analysis.variance import analyze

        src = a.source or os.path.join(configs[0]["path"]["preprocessed_path"], "val.txt")
        rep = analyze(model, configs, src, dev, (a.pitch_control, a.energy_control, a.duration_control), a.out_dir,
                      a.batch_size or 8, a.outlier_k)
    elif a.command == "objective":
        from speakingstyle_amd.analysis.objective import evaluate_objective

        src = a.source or os.path.join(configs[0]["path"]["preprocessed_path"], "val.txt")
        rep = evaluate_objective(model, configs, src, dev, (a.pitch_control, a.energy_control, a.duration_control),
                                 a.batch_size or 32, a.out_dir, a.n_ceps, wave=a.wave, vocoder=a.vocoder,
                                 pitch_tracker=a.pitch_tracker)
    elif a.command == "style":
        from speakingstyle_amd.analysis.style_map import style_map

        src = a.source or os.path.join(configs[0]["path"]["preprocessed_path"], "train.txt")
        rep = style_map(model, configs, src, dev, a.out_dir or "analysis", a.space, a.clusters, a.perplexity, a.iters,
                        a.max_utts, a.like, a.top, a.seed, a.batch_size or 32)
    else:
        from speakingstyle_amd.analysis.inspect import inspect_batch

        rep = inspect_batch(model, configs, dev, synthetic=a.synthetic)
    print(json.dumps(rep, indent=2))
    return rep


if __name__ == "__main__":
    main()
