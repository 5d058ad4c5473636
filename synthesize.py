#!/usr/bin/env python
"""Synthesis CLI -- reference flags (``synthesize.py:153-225``) plus word-level
prosody control and GST style weights.

  single:  python synthesize.py --mode single --text "..." [--ref_audio x.wav] --restore_step N -p -m -t
  batch:   python synthesize.py --mode batch --source val.txt --restore_step N -p -m -t
  word-level control: --word_pitch 1,1.3,0.8 --word_energy ... --word_duration ... (one factor per word)
  GST:     --style_weights 0.5,0,0,...   (one weight per style token)
  Griffin-Lim instead of HiFi-GAN (no vocoder checkpoint): --vocoder griffin_lim   (all modes)
  iSTFTNet generator instead of HiFi-GAN (generator_istft_{speaker}.pth.tar): --vocoder istftnet   (all modes)
  serve:   python synthesize.py --mode serve [--source lines.txt] --restore_step N -p -m -t
           one text per line (from --source or stdin) -> {result_path}/serve_{line:04d}.wav, through the serving
           entry (infer/serve.py: bucketed HIP graphs on the GPU); prints the graph statistics at the end
  prosody transfer (all modes): --prosody_ref x.wav [--transfer pitch,energy,duration] [--transfer_strength 0..1]
           [--transfer_pitch relative|absolute]: say the text the way the recording says it (infer/transfer.py);
           --prosody_ref recording: every utterance's own <raw_path>/<speaker>/<basename>.wav (batch mode)
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

from speakingstyle_amd.config import load_configs  # noqa: E402
from speakingstyle_amd.data.dataset import TextDataset  # noqa: E402
from speakingstyle_amd.infer.synthesis import single_batch, synthesize, word_level_controls  # noqa: E402
from speakingstyle_amd.text import g2p  # noqa: E402
from speakingstyle_amd.utils.model import get_model, get_vocoder  # noqa: E402


def _floats(s):
    return None if s is None else [float(x) for x in s.split(",") if x.strip()]


def _choose_vocoder(model_config, choice):
    """--vocoder griffin_lim: the checkpoint-free Griffin-Lim vocoder instead of the model config's;
    --vocoder istftnet: the iSTFTNet generator (``generator_istft_{speaker}.pth.tar``, random init without one)."""
    if choice == "griffin_lim":
        model_config["vocoder"] = dict(model_config["vocoder"], model="GriffinLim")
    elif choice == "istftnet":
        model_config["vocoder"] = dict(model_config["vocoder"], model="iSTFTNet")


def _transfer_args(args):
    """The validated --transfer* flags as ``synthesize_like`` keywords."""
    from speakingstyle_amd.infer.transfer import check_transfer

    what = check_transfer(args.transfer, args.transfer_strength, args.transfer_pitch)
    return {"what": what, "strength": args.transfer_strength, "pitch_mode": args.transfer_pitch}


def synthesize_with_prosody(model, configs, vocoder, batchs, controls, result_path, args, use_ref, style_weights,
                            speaker_of=None):
    """The batches through ``infer.transfer.synthesize_like`` -> ``{result_path}/{basename}.wav``."""
    from speakingstyle_amd.analysis.objective import _recording
    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.infer.transfer import synthesize_like

    pp = configs[0]
    kw = _transfer_args(args)
    for batch in batchs:
        names = batch[0]
        if args.prosody_ref == "recording":
            if speaker_of is None:
                raise ValueError("--prosody_ref recording needs --mode batch: the recordings are the listed utterances'")
            recs = [_recording(pp, speaker_of[base], base) for base in names]
        else:
            recs = [args.prosody_ref] * len(names)
        out = synthesize_like(model, configs, batch, recs, vocoder=vocoder, controls=controls, use_ref=use_ref,
                              style_weights=style_weights, **kw)
        for wav, name in zip(out["wav"], names):
            write_wav(os.path.join(result_path, f"{name}.wav"), pp["preprocessing"]["audio"]["sampling_rate"], wav)


def serve(args):
    """One wav per input line through ``infer.serve.Synthesizer``."""
    from speakingstyle_amd.audio.io import write_wav
    from speakingstyle_amd.infer.serve import Synthesizer

    configs = load_configs(args.preprocess_config, args.model_config, args.train_config)
    _choose_vocoder(configs[1], args.vocoder)
    tts = Synthesizer(configs, args.restore_step)
    result_path = args.result_path or configs[2]["path"]["result_path"]
    os.makedirs(result_path, exist_ok=True)
    if args.source is not None:
        with open(args.source, encoding="utf-8") as f:
            lines = f.read().splitlines()
    else:
        lines = sys.stdin.read().splitlines()
    extra = {}
    if args.prosody_ref is not None:
        if args.prosody_ref == "recording":
            raise ValueError("--prosody_ref recording needs --mode batch: the recordings are the listed utterances'")
        kw = _transfer_args(args)
        extra = {"prosody_ref": args.prosody_ref, "transfer": kw["what"], "transfer_strength": kw["strength"],
                 "pitch_mode": kw["pitch_mode"]}
    n = 0
    for line in lines:
        if not line.strip():
            continue
        wav = tts.tts(line.strip(), speaker_id=args.speaker_id, ref_audio=args.ref_audio,
                      style_weights=_floats(args.style_weights), pitch_control=args.pitch_control,
                      energy_control=args.energy_control, duration_control=args.duration_control, **extra)
        write_wav(os.path.join(result_path, f"serve_{n:04d}.wav"), tts.sampling_rate, wav)
        n += 1
    print(f"wrote {n} wavs to {result_path}; graphs: {tts.stats}")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--restore_step", type=int, required=True)
    ap.add_argument("--mode", type=str, choices=["batch", "single", "serve"], required=True)
    ap.add_argument("--source", type=str, default=None)
    ap.add_argument("--text", type=str, default=None)
    ap.add_argument("--ref_audio", type=str, default=None)
    ap.add_argument("--speaker_id", type=int, default=0, help="speaker id (multi-speaker models)")
    ap.add_argument("-p", "--preprocess_config", type=str, required=True)
    ap.add_argument("-m", "--model_config", type=str, required=True)
    ap.add_argument("-t", "--train_config", type=str, required=True)
    ap.add_argument("--pitch_control", type=float, default=1.0)
    ap.add_argument("--energy_control", type=float, default=1.0)
    ap.add_argument("--duration_control", type=float, default=1.0)
    ap.add_argument("--word_pitch", type=str, default=None)
    ap.add_argument("--word_energy", type=str, default=None)
    ap.add_argument("--word_duration", type=str, default=None)
    ap.add_argument("--style_weights", type=str, default=None)
    ap.add_argument("--batch_size", type=int, default=8)
    ap.add_argument("--plot", action="store_true", help="also write mel/pitch/energy PNGs")
    ap.add_argument("--result_path", type=str, default=None)
    ap.add_argument("--vocoder", type=str, choices=["config", "griffin_lim", "istftnet"], default="config",
                    help="config: the model config's vocoder (HiFi-GAN); griffin_lim: no checkpoint needed; "
                         "istftnet: the iSTFTNet generator (config/hifigan/config_istft.json)")
    ap.add_argument("--prosody_ref", type=str, default=None,
                    help="a wav whose pitch / energy / timing the synthesis takes over; 'recording': each utterance's "
                         "own recording under raw_path (batch mode)")
    ap.add_argument("--transfer", type=str, default="pitch,energy,duration", help="what --prosody_ref transfers")
    ap.add_argument("--transfer_strength", type=float, default=1.0, help="0 = the model's prediction, 1 = the recording's")
    ap.add_argument("--transfer_pitch", type=str, choices=["relative", "absolute"], default="relative",
                    help="relative: the recording's contour at the voice's own level; absolute: its Hz")
    args = ap.parse_args(argv)
    if args.mode == "serve":
        assert args.text is None
        return serve(args)
    if args.mode == "batch":
        assert args.source is not None and args.text is None
    else:
        assert args.source is None and args.text is not None

    configs = load_configs(args.preprocess_config, args.model_config, args.train_config)
    pp, mc, tc = configs
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model = get_model(args.restore_step, configs, device, train=False, ignore_layers=tc.get("ignore_layers", []))
    _choose_vocoder(mc, args.vocoder)
    vocoder = get_vocoder(mc, device, preprocess_config=pp)
    result_path = args.result_path or tc["path"]["result_path"]
    os.makedirs(result_path, exist_ok=True)
    controls = [args.pitch_control, args.energy_control, args.duration_control]
    use_ref = True
    speaker_of = None
    if args.mode == "batch":
        ds = TextDataset(args.source, pp, tc)
        speaker_of = dict(zip(ds.basename, ds.speaker))
        batchs = list(DataLoader(ds, batch_size=args.batch_size, collate_fn=ds.collate_fn))
    else:
        lexicon = g2p.load_lexicon(pp["path"]["lexicon_path"], pp["preprocessing"]["text"].get("language", "en"))
        batch, phones, use_ref = single_batch(args.text, pp, args.speaker_id, args.ref_audio, lexicon)
        batchs = [batch]
        if any(v is not None for v in (args.word_pitch, args.word_energy, args.word_duration)):
            groups = g2p.word_groups(args.text, lexicon)
            for i, wv in enumerate((args.word_pitch, args.word_energy, args.word_duration)):
                if wv is not None:
                    controls[i] = word_level_controls(groups, _floats(wv), controls[i])
    sw = _floats(args.style_weights)
    if args.prosody_ref is not None:
        synthesize_with_prosody(model, configs, vocoder, batchs, controls, result_path, args, use_ref, sw, speaker_of)
        print("wrote results to", result_path)
        return
    synthesize(model, configs, vocoder, batchs, controls, result_path, plot=args.plot, use_ref=use_ref,
               style_weights=sw)
    print("wrote results to", result_path)


if __name__ == "__main__":
    main()
