"""Typed configuration loading for the three-YAML config scheme.

The reference passes three plain dicts ``(preprocess_config, model_config,
train_config)`` everywhere (``train.py:195-200`` of the reference).  We keep that
exact external contract -- the same YAML files and keys load unchanged -- but the
loader here

* uses ``yaml.safe_load`` (the reference uses ``FullLoader``),
* fills defaults for keys that only the BC2013 config carries, so that the
  LJSpeech / LibriTTS / AISHELL3 configs run (the reference crashes with
  ``KeyError: 'reference_encoder'`` at ``model/modules.py:314`` and in
  ``model/optimizer.py:16-21``),
* validates the enumerations the reference asserts at runtime
  (``model/modules.py:36-43``),
* adds an optional ``mi355x:`` block in the train config for the MI355X-native
  knobs (compute dtype, DDP bucket size, kernel toggles, frame budget).
"""
from __future__ import annotations

import copy
import os
from typing import Any, Dict, Tuple

import yaml

Config = Dict[str, Any]

# --------------------------------------------------------------------------- defaults
_MODEL_DEFAULTS: Config = {
    "transformer": {
        "encoder_layer": 4,
        "encoder_head": 2,
        "encoder_hidden": 256,
        "decoder_layer": 6,
        "decoder_head": 2,
        "decoder_hidden": 256,
        "conv_filter_size": 1024,
        "conv_kernel_size": [9, 1],
        "encoder_dropout": 0.2,
        "decoder_dropout": 0.2,
    },
    "variance_predictor": {"filter_size": 256, "kernel_size": 3, "dropout": 0.5},
    "variance_embedding": {
        "pitch_quantization": "linear",
        "energy_quantization": "linear",
        "n_bins": 256,
    },
    # None => style conditioning disabled (LJSpeech / LibriTTS / AISHELL3 configs)
    "reference_encoder": None,
    # Global Style Tokens (Wang et al. 2018).  Only a commented-out block exists in
    # the reference (config/BC2013/model.yaml:33-39); we implement it.
    "gst": None,
    "multi_speaker": False,
    # condition on preprocessing.speaker_embedder vectors through a learned projection (not in the
    # reference model: its checkpoints lack the projection, so this is opt-in)
    "speaker_embed_proj": False,
    # alignment learner (models/aligner.py): {hidden, temperature, prior_scaling}; None => durations come with the
    # data (no extra parameters: reference checkpoints load as before)
    "aligner": None,
    "max_seq_len": 1000,
    "vocoder": {"model": "HiFi-GAN", "speaker": "LJSpeech"},
}

_GST_DEFAULTS: Config = {
    "use_gst": False,
    "conv_filters": [32, 32, 64, 64, 128, 128],
    "gru_hidden": 128,
    "token_size": 128,
    "n_style_token": 10,
    "attn_head": 4,
}

_REF_ENC_DEFAULTS: Config = {
    "encoder_layer": 4,
    "encoder_head": 8,
    "encoder_hidden": 256,
    "conv_layer": 3,
    "conv_filter_size": 1024,
    "conv_kernel_size": 3,
    "dropout": 0.1,
}

_TRAIN_DEFAULTS: Config = {
    "ignore_layers": [],
    "path": {"ckpt_path": "./output/ckpt", "log_path": "./output/log", "result_path": "./output/result"},
    "optimizer": {
        "batch_size": 16,
        "betas": [0.9, 0.98],
        "eps": 1e-9,
        "weight_decay": 0.0,
        "grad_clip_thresh": 1.0,
        "grad_acc_step": 1,
        "warm_up_step": 4000,
        "anneal_steps": [300000, 400000, 500000],
        "anneal_rate": 0.3,
        # init_lr / anneal_lr absent => Noam warm-up schedule (upstream FastSpeech2)
    },
    "step": {"total_step": 900000, "log_step": 100, "synth_step": 1000, "val_step": 1000, "save_step": 10000},
    "mi355x": {
        # activation / GEMM operand dtype on the GPU: bf16 (HIP kernels, fp32 master weights + Adam
        # state) or fp32 (torch reference ops in fp32 -- a numerics oracle, not a fast path)
        "dtype": "bf16",
        "bucket_mb": 32,          # DDP gradient bucket size (fp32 MiB)
        "seed": 1234,
        "num_workers": 4,
        # per-rank frame budget: each GPU trains on its own batch of <= this many PADDED mel frames
        # (data/dataset.py FrameBudgetSampler) instead of batch_size / world utterances of a global batch
        "frames_per_gpu": None,
        "max_batch_per_gpu": None,  # optional utterance cap of a frame-budget batch
        "phase_timing": False,    # per-phase host / device step timing (Perf/phase_* TB scalars)
        "preempt_check_steps": 10,  # DP: steps between cross-rank SIGTERM agreements
        "hip_kernels": True,      # False => torch reference ops even on GPU (debug / A-B only)
        # "high": the step's main chain on a high-priority HIP stream (weight gradients on a normal-
        # priority side stream fill the idle CUs); "normal": one priority for both (A/B)
        "stream_priority": "high",
        # run backward on the calling thread (no autograd device worker thread): less host time per step
        "backward_same_thread": True,
        # (non-finite steps are always skipped on the device by the fused clip+Adam kernel: no knob)
        # validated experiment / diagnostic switches (speakingstyle_amd/experimental.py); empty = production
        "experimental": {},
    },
}

_PREPROCESS_DEFAULTS: Config = {
    "dataset": "LJSpeech",
    "path": {
        "corpus_path": "./data/corpus",
        "lexicon_path": "lexicon/librispeech-lexicon.txt",
        "raw_path": "./raw_data",
        "preprocessed_path": "./preprocessed_data/LJSpeech",
    },
    "preprocessing": {
        "val_size": 512,
        "text": {"text_cleaners": ["english_cleaners"], "language": "en"},
        "audio": {"sampling_rate": 22050, "max_wav_value": 32768.0},
        "stft": {"filter_length": 1024, "hop_length": 256, "win_length": 1024},
        "mel": {"n_mel_channels": 80, "mel_fmin": 0, "mel_fmax": 8000},
        "pitch": {"feature": "phoneme_level", "normalization": True, "extractor": "dio"},
        "energy": {"feature": "phoneme_level", "normalization": True},
        # textgrid: phoneme durations from Montreal-Forced-Aligner TextGrids; learned: no TextGrids -- phones from
        # the transcript, frame-level contours, durations from the model's alignment learner
        "duration": {"source": "textgrid"},
        "speaker_embedder": "none",
    },
}


def _merge(defaults: Config, user: Config | None) -> Config:
    """Recursive dict merge; ``user`` wins.  ``None``-valued defaults are replaced wholesale."""
    out = copy.deepcopy(defaults)
    if not user:
        return out
    for k, v in user.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict):
            out[k] = _merge(out[k], v)
        else:
            out[k] = copy.deepcopy(v)
    return out


class ConfigError(ValueError):
    pass


def _check_enum(value, allowed, where):
    if value not in allowed:
        raise ConfigError(f"{where} = {value!r}; expected one of {allowed}")


def normalize_preprocess_config(cfg: Config | None) -> Config:
    out = _merge(_PREPROCESS_DEFAULTS, cfg)
    pp = out["preprocessing"]
    _check_enum(pp["pitch"]["feature"], ["phoneme_level", "frame_level"], "preprocessing.pitch.feature")
    _check_enum(pp["pitch"].get("extractor", "dio"), ["dio", "yin", "pyin"], "preprocessing.pitch.extractor")
    _check_enum(pp["energy"]["feature"], ["phoneme_level", "frame_level"], "preprocessing.energy.feature")
    _check_enum(pp["duration"]["source"], ["textgrid", "learned"], "preprocessing.duration.source")
    return out


def normalize_model_config(cfg: Config | None) -> Config:
    out = _merge(_MODEL_DEFAULTS, cfg)
    ve = out["variance_embedding"]
    _check_enum(ve["pitch_quantization"], ["linear", "log"], "variance_embedding.pitch_quantization")
    _check_enum(ve["energy_quantization"], ["linear", "log"], "variance_embedding.energy_quantization")
    if out.get("reference_encoder"):
        out["reference_encoder"] = _merge(_REF_ENC_DEFAULTS, out["reference_encoder"])
    gst = out.get("gst")
    if gst:
        out["gst"] = _merge(_GST_DEFAULTS, gst)
        if not out["gst"].get("use_gst", False):
            out["gst"] = None
    if out.get("aligner"):
        missing = [k for k in ("hidden", "temperature", "prior_scaling") if k not in out["aligner"]]
        if missing:
            raise ConfigError(f"aligner block lacks {missing}")
        if int(out["aligner"]["hidden"]) % 8:
            raise ConfigError("aligner.hidden must be a multiple of 8")
    tr = out["transformer"]
    for side in ("encoder", "decoder"):
        if tr[f"{side}_hidden"] % tr[f"{side}_head"]:
            raise ConfigError(f"transformer.{side}_hidden must be divisible by {side}_head")
    if len(tr["conv_kernel_size"]) != 2:
        raise ConfigError("transformer.conv_kernel_size must have two entries")
    return out


def normalize_train_config(cfg: Config | None) -> Config:
    out = _merge(_TRAIN_DEFAULTS, cfg)
    # loss.anneal_steps is what the reference's LR warm-up actually reads
    # (model/optimizer.py:16); without a loss block fall back to warm_up_step.
    loss = out.get("loss") or {}
    loss.setdefault("lambda_f", 0.0)
    loss.setdefault("lambda_align", 1.0)  # weight of the forward-sum alignment loss (learned durations only)
    loss.setdefault("anneal_steps", out["optimizer"]["warm_up_step"])
    out["loss"] = loss
    if out["optimizer"]["grad_acc_step"] < 1:
        raise ConfigError("optimizer.grad_acc_step must be >= 1")
    mi = out["mi355x"]
    _check_enum(mi["dtype"], ["bf16", "fp32"], "mi355x.dtype")
    _check_enum(mi.get("stream_priority", "high"), ["high", "normal"], "mi355x.stream_priority")
    for k in ("graph_steps", "graph_t_quant", "graph_m_quant"):  # removed knobs (round 6: training graphs lost)
        mi.pop(k, None)
    if mi.get("frames_per_gpu") is not None and int(mi["frames_per_gpu"]) <= 0:
        raise ConfigError("mi355x.frames_per_gpu must be a positive frame count (or null)")
    if "nan_guard" in mi:  # removed knob: the device-side non-finite skip is unconditional
        mi.pop("nan_guard")
    return out


def learned_durations(preprocess_config: Config) -> bool:
    """``preprocessing.duration.source: learned``: no TextGrids and no ``duration/`` arrays; the model's alignment
    learner supplies the durations (``models/aligner.py``)."""
    return ((preprocess_config.get("preprocessing") or {}).get("duration") or {}).get("source", "textgrid") == "learned"


def style_mode(model_config: Config) -> str:
    """'film' (reference encoder -> FiLM), 'gst' (style tokens -> FiLM), or 'none'."""
    if model_config.get("gst"):
        return "gst"
    if model_config.get("reference_encoder"):
        return "film"
    return "none"


def load_yaml(path: str) -> Config:
    with open(path, "r") as f:
        return yaml.safe_load(f) or {}


def load_configs(preprocess: str | Config, model: str | Config, train: str | Config | None = None) -> Tuple[Config, Config, Config]:
    """Load + normalize the three configs (paths or already-loaded dicts)."""
    p = load_yaml(preprocess) if isinstance(preprocess, str) else preprocess
    m = load_yaml(model) if isinstance(model, str) else model
    t = load_yaml(train) if isinstance(train, str) else (train or {})
    return normalize_preprocess_config(p), normalize_model_config(m), normalize_train_config(t)


def config_dir_triplet(name: str, root: str | None = None) -> Tuple[str, str, str]:
    """``config/<name>/{preprocess,model,train}.yaml`` paths."""
    root = root or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config")
    d = os.path.join(root, name)
    return tuple(os.path.join(d, f"{k}.yaml") for k in ("preprocess", "model", "train"))  # type: ignore


def load_named(name: str) -> Tuple[Config, Config, Config]:
    return load_configs(*config_dir_triplet(name))
