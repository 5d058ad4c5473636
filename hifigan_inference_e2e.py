#!/usr/bin/env python
"""HiFi-GAN end-to-end CLI (reference ``hifigan/inference_e2e.py``): every ``.npy`` mel in
--input_mels_dir (e.g. FastSpeech2 output, [n_mels, T]) -> ``{name}_generated_e2e.wav``.

  python hifigan_inference_e2e.py --checkpoint_file cp_hifigan/g_02500000 [--input_mels_dir test_mel_files]
  python hifigan_inference_e2e.py --griffin_lim [--input_mels_dir test_mel_files]     (no checkpoint)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--input_mels_dir", default="test_mel_files")
    ap.add_argument("--output_dir", default="generated_files_from_mel")
    ap.add_argument("--checkpoint_file", default=None)
    ap.add_argument("--config", default=None, help="default: config.json next to the checkpoint")
    ap.add_argument("--batch_size", type=int, default=16)
    ap.add_argument("--griffin_lim", action="store_true",
                    help="vocode with Griffin-Lim instead of a generator: no checkpoint needed")
    ap.add_argument("--preprocess_config", default=None, help="--griffin_lim: preprocess.yaml with the STFT / mel "
                    "settings of the mels (default: 22.05 kHz, 1024 / 256, 80 mels)")
    ap.add_argument("--n_iters", type=int, default=60, help="--griffin_lim: iterations")
    a = ap.parse_args(argv)
    from speakingstyle_amd.vocoder.infer import from_mels, from_mels_griffin_lim

    if a.griffin_lim:
        pp = None
        if a.preprocess_config:
            from speakingstyle_amd.config import load_yaml, normalize_preprocess_config

            pp = normalize_preprocess_config(load_yaml(a.preprocess_config))
        paths = from_mels_griffin_lim(a.input_mels_dir, a.output_dir, pp, batch_size=a.batch_size, n_iters=a.n_iters)
    else:
        if a.checkpoint_file is None:
            ap.error("--checkpoint_file is required (or pass --griffin_lim)")
        paths = from_mels(a.input_mels_dir, a.output_dir, a.checkpoint_file, config=a.config, batch_size=a.batch_size)
    for p in paths:
        print(p)


if __name__ == "__main__":
    main()
