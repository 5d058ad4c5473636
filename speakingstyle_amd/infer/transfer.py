"""Prosody transfer: speak a text with a recording's pitch, energy and timing.

Two synthesis passes.  The first is the ordinary one (the model's own durations, pitch and energy, under whatever
style and controls the caller gives).  Its mel is aligned with the recording's (``analysis.objective.align``: DTW on
mel cepstra), ``ops.prosody_transfer`` turns the path and the recording's F0 / energy contours into the per-phoneme
targets the variance adaptor was trained on, and the second pass synthesizes with those targets in place of the
predictions.  Only phoneme-level pitch / energy configs are covered; the alignment is always the DTW one (a model's
own aligner is not used).

  recording_features   packed samples -> log-mel rows, energy, F0 (``ops.pyin`` / ``ops.yin``), frame counts
  transfer_targets     first pass + features -> p / e / d targets, blended with a strength in [0, 1]
  synthesize_like      both passes; on the GPU the packed path (``infer_front`` / ``infer_back`` / the vocoder's
                       ``infer_packed``) run eagerly, elsewhere ``FastSpeech2.forward``
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import ops
from ..analysis.objective import PITCH_TRACKERS, _front_end, align

FEATURES = ("pitch", "energy", "duration")
PITCH_FRAME = 1024  # samples per analysis frame of the pitch tracker


def check_transfer(what, strength, pitch_mode) -> tuple:
    """The validated ``what`` as a tuple; ``ValueError`` with the offending value."""
    what = tuple(what.split(",")) if isinstance(what, str) else tuple(what)
    bad = [w for w in what if w not in FEATURES]
    if bad or not what:
        raise ValueError(f"transfer {what!r}: a non-empty subset of {', '.join(FEATURES)}")
    if not 0.0 <= float(strength) <= 1.0:
        raise ValueError(f"transfer_strength {strength} outside 0 .. 1")
    if pitch_mode not in ops.ref.PROSODY_PITCH_MODES:
        raise ValueError(f"pitch_mode {pitch_mode!r} not supported ({', '.join(ops.ref.PROSODY_PITCH_MODES)})")
    return what


def check_levels(pp):
    """Frame-level pitch / energy have no per-phoneme targets to transfer to."""
    for k in ("pitch", "energy"):
        if pp["preprocessing"][k]["feature"] != "phoneme_level":
            raise ValueError(f"prosody transfer needs phoneme-level features: preprocessing.{k}.feature is "
                             f"{pp['preprocessing'][k]['feature']!r}")


def normalisation(pp) -> Dict[str, tuple]:
    """(mean, std) of the stored pitch / energy: ``stats.json`` where the config normalises, (0, 1) where not."""
    out, st = {}, None
    for k in ("pitch", "energy"):
        if pp["preprocessing"][k].get("normalization", True):
            if st is None:
                fn = os.path.join(pp["path"]["preprocessed_path"], "stats.json")
                if not os.path.exists(fn):
                    raise FileNotFoundError(f"prosody transfer needs the {k} normalisation of the training data: {fn} "
                                            "is missing")
                with open(fn) as f:
                    st = json.load(f)
            out[k] = (float(st[k][2]), float(st[k][3]))
        else:
            out[k] = (0.0, 1.0)
    return out


@torch.no_grad()
def recording_features(wav, lens, pp, tracker: str = "pyin"):
    """Packed fp32 samples in [-1, 1] (all utterances back to back, host sample counts ``lens``) -> (log-mel rows
    [R, n_mel], energy [R], F0 [R] in Hz (0 = unvoiced), host frame counts): 1 + N // hop frames per utterance.  The
    mel front end of the preprocess config (on the GPU the fused log-mel kernel, which also gives the energy) and
    ``ops.pyin`` (``tracker="yin"``: ``ops.yin``)."""
    if tracker not in PITCH_TRACKERS:
        raise ValueError(f"pitch tracker {tracker!r} not supported ({', '.join(PITCH_TRACKERS)})")
    lens = [int(v) for v in lens]
    pre = pp["preprocessing"]
    wav = wav.float().contiguous()
    track = ops.yin if tracker == "yin" else ops.pyin
    f0, frames = track(wav, lens, pre["audio"]["sampling_rate"], pre["stft"]["hop_length"], PITCH_FRAME)[:2]
    stft = _front_end(pp)
    rows, en, at = [], [], 0
    for n in lens:
        mel, e = stft.mel_spectrogram(wav[at:at + n].unsqueeze(0))
        rows.append(mel[0].transpose(0, 1))
        en.append(e[0])
        at += n
    return torch.cat(rows).float().contiguous(), torch.cat(en).float().contiguous(), f0, [int(v) for v in frames]


@torch.no_grad()
def transfer_targets(first_pass, features, stats, what=FEATURES, strength: float = 1.0, pitch_mode: str = "relative",
                     min_frames: int = 1, n_ceps: int = 13):
    """The second pass's targets.  ``first_pass``: {"mel": packed post-net rows [R, n_mel], "mel_lens": host frame
    counts, "durations" [B, T] integers, "src_lens" [B], "pitch" / "energy" [B, T] the normalised predictions};
    ``features``: ``recording_features``' tuple for the B recordings; ``stats``: {"pitch": (mean, std), "energy":
    (mean, std)} (``normalisation``).  For each feature of ``what`` with strength s:

      pitch, energy   pred + s (transferred - pred); the prediction stays where the recording gave the token no frame
                      and (pitch) where the recording has no voiced frame
      duration        floor((1 - s) src_dur + s rec_dur + 0.5), then at least ``min_frames`` where src_dur > 0

    A feature not in ``what`` keeps the first pass's values.
    -> {"p_targets", "e_targets" [B, T] fp32, "d_targets" [B, T] int64, "rec_dur", "voiced", "pitch_ok", "path_len"}"""
    what = check_transfer(what, strength, pitch_mode)
    s = float(strength)
    rmel, ren, rf0, rframes = features
    lens = [int(v) for v in first_pass["mel_lens"]]
    for b, n in enumerate(lens):
        if n < 1:
            raise ValueError(f"prosody transfer: the first pass gave utterance {b} no frames; nothing to align")
    src_dur = first_pass["durations"]
    pred_p, pred_e = first_pass["pitch"].float(), first_pass["energy"].float()
    _, path, plen = align(first_pass["mel"], lens, rmel.to(first_pass["mel"].device), rframes, n_ceps)
    rec_dur, tp, te, voiced, ok = ops.prosody_transfer(path, plen, src_dur, first_pass["src_lens"], lens, rframes, rf0,
                                                       ren, pred_p, stats["pitch"], stats["energy"], pitch_mode)
    has = rec_dur > 0
    tp, te = tp.to(pred_p.dtype), te.to(pred_e.dtype)
    p_t, e_t, d_t = pred_p, pred_e, src_dur.long()
    if "pitch" in what:
        p_t = torch.where(has & ok.unsqueeze(1), pred_p + s * (tp - pred_p), pred_p)
    if "energy" in what:
        e_t = torch.where(has, pred_e + s * (te - pred_e), pred_e)
    if "duration" in what:
        d_t = torch.floor((1.0 - s) * src_dur.double() + s * rec_dur.double() + 0.5).long()
        d_t = torch.where(src_dur > 0, d_t.clamp(min=int(min_frames)), d_t)
    return {"p_targets": p_t, "e_targets": e_t, "d_targets": d_t, "rec_dur": rec_dur, "voiced": voiced,
            "pitch_ok": ok, "path_len": plen}


def _load_recordings(recordings, pp, device):
    """Wav paths or sample arrays -> (packed fp32 samples on ``device``, host sample counts)."""
    from ..audio.io import read_wav

    sr = pp["preprocessing"]["audio"]["sampling_rate"]
    wavs = []
    for r in recordings:
        if isinstance(r, (str, os.PathLike)):
            r = read_wav(os.fspath(r), sr)[0]
        w = torch.as_tensor(np.asarray(r) if not isinstance(r, torch.Tensor) else r).float().reshape(-1).clamp(-1.0, 1.0)
        if w.shape[0] <= PITCH_FRAME // 2:
            raise ValueError(f"prosody transfer: a recording of {w.shape[0]} samples is too short for the pitch "
                             f"tracker's frame of {PITCH_FRAME}")
        wavs.append(w.to(device))
    return torch.cat(wavs), [int(w.shape[0]) for w in wavs]


@torch.no_grad()
def synthesize_like(model, configs, batch, recordings=None, vocoder=None, controls=(1.0, 1.0, 1.0), use_ref=True,
                    style_weights=None, what=FEATURES, strength: float = 1.0, pitch_mode: str = "relative",
                    tracker: str = "pyin", stats=None, features=None, min_frames: int = 1):
    """Synthesize the texts of ``batch`` (a ``single_batch`` / ``TextDataset.collate_fn`` tuple, host arrays or device
    tensors) the way ``recordings`` (one wav path or sample array per utterance; or their ``recording_features`` as
    ``features``) say them.  Pass 1 is the plain synthesis -- style reference (``use_ref``: the batch's mels), GST
    ``style_weights`` and ``controls`` as in ``synthesize`` -- pass 2 takes ``transfer_targets``.

    On the GPU with the packed inference path both passes run ``infer_front`` / ``infer_back`` and the vocoder's
    ``infer_packed`` eagerly; elsewhere ``FastSpeech2.forward`` (``mels_style_only``: the style reference does not
    size the result).  -> {"mel": one [T_b, n_mel] fp32 tensor per utterance, "mel_lens": host list, "wav": one
    int16 array per utterance (None without ``vocoder``), "targets": ``transfer_targets``' dict, "first_pass"}."""
    from ..data.dataset import to_device

    pp, mc = configs[0], configs[1]
    check_levels(pp)
    what = check_transfer(what, strength, pitch_mode)
    dev = next(model.parameters()).device
    batch = to_device(batch, dev)
    speakers, texts, src_lens, max_src = batch[2], batch[3], batch[4], int(batch[5])
    mels, mel_lens, max_mel = (batch[6], batch[7], batch[8]) if use_ref else (None, None, None)
    B = texts.shape[0]
    sw = None if style_weights is None else torch.as_tensor(style_weights, device=dev).float().view(1, -1).expand(B, -1)
    ctl = [torch.as_tensor(c, device=dev).float().view(1, -1) if isinstance(c, (list, np.ndarray)) else c for c in controls]
    if features is None:
        if recordings is None or len(recordings) != B:
            raise ValueError(f"prosody transfer: {B} utterances need {B} recordings")
        features = recording_features(*_load_recordings(recordings, pp, dev), pp, tracker)
    stats = normalisation(pp) if stats is None else stats
    packed = model.packed_inference_ok(texts)

    def run(p_t=None, e_t=None, d_t=None):
        """One pass -> (packed post-net rows [R, n_mel], host mel lengths, durations, p_pred, e_pred)."""
        if packed:
            front = model.infer_front(speakers, texts, src_lens, max_src, mels, mel_lens, max_mel, ctl[0], ctl[1], ctl[2],
                                      sw, p_targets=p_t, e_targets=e_t, d_targets=d_t, return_preds=True)
            lens = [int(v) for v in front[2].cpu().tolist()]
            return model.infer_back(front[:4], lens), lens, front[1], front[4][0], front[4][1]
        out = model(speakers, texts, src_lens, max_src, mels=mels, mel_lens=mel_lens, max_mel_len=max_mel, p_targets=p_t,
                    e_targets=e_t, d_targets=d_t, p_control=ctl[0], e_control=ctl[1], d_control=ctl[2], style_weights=sw,
                    mels_style_only=True)
        lens = [int(v) for v in out[9].cpu().tolist()]
        rows = torch.cat([out[1][b, :n].float() for b, n in enumerate(lens)]) if B else out[1].reshape(0, out[1].shape[-1])
        return rows.contiguous(), lens, out[5], out[2], out[3]

    rows, lens, dur, p_pred, e_pred = run()
    first = {"mel": rows, "mel_lens": lens, "durations": dur, "src_lens": src_lens, "pitch": p_pred, "energy": e_pred}
    targets = transfer_targets(first, features, stats, what, strength, pitch_mode, min_frames)
    rows2, lens2, _, _, _ = run(targets["p_targets"], targets["e_targets"], targets["d_targets"])
    wav = None
    if vocoder is not None:
        wav = _vocode(vocoder, rows2, lens2, configs)
    cu = np.concatenate([[0], np.cumsum(lens2)]).astype(np.int64)
    return {"mel": [rows2[cu[b]:cu[b + 1]] for b in range(B)], "mel_lens": lens2, "wav": wav, "targets": targets,
            "first_pass": first}


def _vocode(vocoder, rows, lens, configs):
    """Packed post-net rows -> one int16 array of lens[b] * hop samples per utterance."""
    pp, mc = configs[0], configs[1]
    hop = pp["preprocessing"]["stft"]["hop_length"]
    mx = pp["preprocessing"]["audio"]["max_wav_value"]
    if rows.is_cuda and hasattr(vocoder, "infer_packed"):
        x = rows.to(getattr(vocoder, "mel_dtype", torch.bfloat16)).contiguous()
        wav = vocoder.infer_packed(x, lens, int16_scale=mx).cpu().numpy()
        return [wav[b, : n * hop] for b, n in enumerate(lens)]
    from ..utils.model import vocoder_infer

    M = max(lens + [1])
    pad = rows.new_zeros(len(lens), M, rows.shape[1])
    at = 0
    for b, n in enumerate(lens):
        pad[b, :n] = rows[at:at + n]
        at += n
    return vocoder_infer(pad, vocoder, mc, pp, lengths=[n * hop for n in lens], channel_last=True)
