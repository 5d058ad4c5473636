"""Objective synthesis metrics: how far is a free-running synthesis from the recording of the same utterance?

The synthesized and the recorded utterance differ in length, so every per-utterance figure is taken along a dynamic
time warping path between their mel cepstra (``ops.dtw``: one HIP workgroup per pair on the GPU, the torch
wavefront of ``ops.reference`` on the CPU):

  mcd_db          mel-cepstral distortion, (10 sqrt(2) / ln 10) * DTW cost / path length, over cepstra 1..n_ceps
                  of the stored natural-log mel (orthonormal DCT-II, c0 dropped)
  logmel_l1       mean |log-mel difference| along the path, all mel channels
  pitch_rmse      RMSE of the frame-level pitch / energy contours gathered along the path (de-normalised with
  energy_rmse     ``stats.json``; phoneme-level features are expanded to frames with the predicted / stored durations)
  pitch_corr      Pearson correlation of the two pitch contours along the path (nan when one is constant)
  dur_mae_frames  mean |predicted - stored| phoneme duration in frames (no alignment involved)
  len_ratio       synthesized frames / recorded frames

The x side of every alignment is the synthesis, the y side the recording.  A synthesis of zero frames has no
alignment: its path metrics are nan, it is counted in ``n_empty`` and left out of the means and medians.

Waveform-level figures (``wave_metrics``, ``evaluate_objective(wave=True)``): the figures above compare what the model
predicts; these compare what is heard.  Both waveforms -- the vocoded synthesis and the recording -- go through the
same front end (log-mel -> cepstra -> ``ops.dtw``) and the same pitch tracker (``ops.yin``: one HIP workgroup per
frame on the GPU; or ``ops.pyin``, probabilistic YIN, which decodes one smooth track per utterance and keeps the
voiced frames of noisy vocoded audio that a fixed threshold drops), and the F0 tracks are gathered along the path
(Skerry-Ryan et al. 2018, after Chu & Alwan 2009):

  wave_mcd_db         ``mcd_db`` of the audio
  wave_vde            voicing decision error: share of path cells voiced on one side only
  wave_gpe            gross pitch error: among cells voiced on both sides, the share with |fa - fb| > 0.2 fb (nan
                      when there are none)
  wave_ffe            F0 frame error: share of cells with either error
  wave_f0_rmse_cents  RMSE of 1200 log2(fa / fb) over the cells voiced on both sides (nan when there are none)
"""
from __future__ import annotations

import csv
import json
import math
import os
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import ops
from .variance import _stats

MCD_SCALE = 10.0 * math.sqrt(2.0) / math.log(10.0)
METRICS = ("mcd_db", "logmel_l1", "pitch_rmse", "energy_rmse", "pitch_corr", "dur_mae_frames", "len_ratio")
WAVE_METRICS = ("wave_mcd_db", "wave_vde", "wave_gpe", "wave_ffe", "wave_f0_rmse_cents")
GROSS_PITCH_ERROR = 0.2  # relative F0 deviation from the y side that counts as gross
PITCH_TRACKERS = ("yin", "pyin")


def dct_matrix(n_mel: int, n_ceps: int, device=None, dtype=torch.float32) -> torch.Tensor:
    """[n_mel, n_ceps]: columns k = 1 .. n_ceps of the orthonormal DCT-II, sqrt(2/N) cos(pi (n + 1/2) k / N)."""
    if not 1 <= n_ceps < n_mel:
        raise ValueError(f"n_ceps {n_ceps} must lie in 1 .. n_mel - 1 = {n_mel - 1}")
    n = torch.arange(n_mel, dtype=torch.float64).unsqueeze(1)
    k = torch.arange(1, n_ceps + 1, dtype=torch.float64).unsqueeze(0)
    return (math.sqrt(2.0 / n_mel) * torch.cos(math.pi / n_mel * (n + 0.5) * k)).to(device=device, dtype=dtype)


def mel_cepstra(logmel: torch.Tensor, n_ceps: int = 13) -> torch.Tensor:
    """Natural-log mel rows [..., n_mel] -> mel cepstra 1 .. n_ceps [..., n_ceps] (fp32, or float64 for float64 rows):
    one small full-precision matmul."""
    x = logmel if logmel.dtype == torch.float64 else logmel.float()
    return x @ dct_matrix(x.shape[-1], n_ceps, x.device, x.dtype)


def align(pred_mel, pred_lens, true_mel, true_lens, n_ceps: int = 13):
    """DTW of packed log-mel rows [R, n_mel] on their cepstra -> ``ops.dtw``'s (cost [P], path [P, Lmax, 2], path_len
    [P]); path[..., 0] indexes the synthesized frames, path[..., 1] the recorded ones."""
    return ops.dtw(mel_cepstra(pred_mel, n_ceps).contiguous(), mel_cepstra(true_mel, n_ceps).contiguous(),
                   list(pred_lens), list(true_lens))


def _starts(lens, device):
    cu = np.zeros(len(lens), dtype=np.int64)
    cu[1:] = np.cumsum(lens)[:-1]
    return torch.from_numpy(cu).to(device)


def _along(path, plen, pred_lens, true_lens):
    """Global row indices of the path cells in the packed pred / true rows and the mask of real cells."""
    dev = path.device
    mask = torch.arange(path.shape[1], device=dev).unsqueeze(0) < plen.unsqueeze(1)
    ip = (path[..., 0].long() + _starts(pred_lens, dev).unsqueeze(1)).masked_fill(~mask, 0)
    it = (path[..., 1].long() + _starts(true_lens, dev).unsqueeze(1)).masked_fill(~mask, 0)
    return ip, it, mask


def _rmse(a, b, mask, n):
    d = (a - b).masked_fill(~mask, 0.0)
    return torch.sqrt((d * d).sum(1) / n)


def _pearson(a, b, mask, n):
    a, b = a.masked_fill(~mask, 0.0), b.masked_fill(~mask, 0.0)
    da = (a - (a.sum(1) / n).unsqueeze(1)).masked_fill(~mask, 0.0)
    db = (b - (b.sum(1) / n).unsqueeze(1)).masked_fill(~mask, 0.0)
    den = torch.sqrt((da * da).sum(1) * (db * db).sum(1))
    return torch.where(den > 0, (da * db).sum(1) / den, torch.full_like(den, float("nan")))


def utterance_metrics(pred_mel, pred_lens, true_mel, true_lens, pred_pitch=None, true_pitch=None, pred_energy=None,
                      true_energy=None, pred_dur: Optional[Sequence] = None, true_dur: Optional[Sequence] = None,
                      n_ceps: int = 13) -> Dict[str, np.ndarray]:
    """Per-pair metrics of P utterances.  ``pred_mel`` [Rp, n_mel] / ``true_mel`` [Rt, n_mel]: packed log-mel rows with
    host frame counts ``pred_lens`` / ``true_lens``; ``*_pitch`` / ``*_energy``: packed frame-level contours [Rp] / [Rt]
    in physical units; ``*_dur``: one integer array of phoneme durations per utterance.  -> {metric: float64 [P]} plus
    ``path_len`` (int) and ``path`` / the DTW ``cost`` as returned by ``align``.  Metrics whose inputs are missing are
    left out."""
    pred_lens, true_lens = [int(v) for v in pred_lens], [int(v) for v in true_lens]
    cost, path, plen = align(pred_mel, pred_lens, true_mel, true_lens, n_ceps)
    ip, it, mask = _along(path, plen, pred_lens, true_lens)
    n = plen.double()
    out = {"mcd_db": MCD_SCALE * cost.double() / n}
    dm = (pred_mel.double()[ip] - true_mel.double()[it]).abs().sum(-1).masked_fill(~mask, 0.0)
    out["logmel_l1"] = dm.sum(1) / (n * pred_mel.shape[1])
    if pred_pitch is not None and true_pitch is not None:
        a, b = pred_pitch.double()[ip], true_pitch.double()[it]
        out["pitch_rmse"] = _rmse(a, b, mask, n)
        out["pitch_corr"] = _pearson(a, b, mask, n)
    if pred_energy is not None and true_energy is not None:
        out["energy_rmse"] = _rmse(pred_energy.double()[ip], true_energy.double()[it], mask, n)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if pred_dur is not None and true_dur is not None:
        res["dur_mae_frames"] = np.asarray([np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).mean()
                                            for a, b in zip(pred_dur, true_dur)])
    res["len_ratio"] = np.asarray(pred_lens, np.float64) / np.asarray(true_lens, np.float64)
    res["path_len"] = plen.cpu().numpy()
    res["cost"] = cost.cpu().numpy()
    res["path"] = path.cpu().numpy()
    return res


def prosody_errors(fa, fb, mask) -> Dict[str, torch.Tensor]:
    """Voicing / pitch errors of F0 tracks gathered along alignment paths: ``fa`` / ``fb`` [P, L] in Hz (0 =
    unvoiced; b is the side the deviation is relative to), ``mask`` [P, L] the real cells.  -> float64 [P] each of
    ``vde``, ``gpe``, ``ffe`` and ``f0_rmse_cents``."""
    fa, fb = fa.double(), fb.double()
    n = mask.sum(1).double()
    va, vb = (fa > 0) & mask, (fb > 0) & mask
    voicing = va != vb
    both = va & vb
    gross = both & ((fa - fb).abs() > GROSS_PITCH_ERROR * fb)
    nb = both.sum(1).double()
    nan = torch.full_like(n, float("nan"))
    one = torch.ones_like(fa)
    cents = (1200.0 * torch.log2(torch.where(both, fa, one) / torch.where(both, fb, one)))
    some = nb > 0
    nb1 = torch.where(some, nb, torch.ones_like(nb))
    return {"vde": voicing.sum(1).double() / n,
            "gpe": torch.where(some, gross.sum(1).double() / nb1, nan),
            "ffe": (voicing | gross).sum(1).double() / n,
            "f0_rmse_cents": torch.where(some, torch.sqrt((cents * cents).sum(1) / nb1), nan)}


_front_ends = {}


def _front_end(pp):
    """The mel front end of a preprocess config (one ``TacotronSTFT`` per setting)."""
    from ..audio.stft import TacotronSTFT

    pre = pp["preprocessing"]
    s, m = pre["stft"], pre["mel"]
    key = (s["filter_length"], s["hop_length"], s["win_length"], m["n_mel_channels"], pre["audio"]["sampling_rate"],
           m["mel_fmin"], m["mel_fmax"])
    if key not in _front_ends:
        _front_ends[key] = TacotronSTFT(*key)
    return _front_ends[key]


def _logmel_rows(wav, lens, stft):
    """Packed waveforms -> packed log-mel rows [R, n_mel] (1 + N // hop per utterance), one front-end call per
    utterance (on the GPU the fused log-mel kernel)."""
    rows, at = [], 0
    for n in lens:
        mel, _ = stft.mel_spectrogram(wav[at:at + n].unsqueeze(0))
        rows.append(mel[0].transpose(0, 1))
        at += n
    return torch.cat(rows).contiguous()


@torch.no_grad()
def wave_metrics(wav_a, lens_a, wav_b, lens_b, pp, n_ceps: int = 13, frame: int = 1024,
                 tracker: str = "yin") -> Dict[str, np.ndarray]:
    """Waveform-level metrics of P pairs of utterances: ``wav_a`` / ``wav_b`` packed fp32 samples in [-1, 1] on one
    device (all utterances back to back) with host sample counts ``lens_a`` / ``lens_b``; ``pp`` the preprocess
    config (sampling rate, STFT, mel).  Log-mel of both sides -> cepstra -> ``ops.dtw``; ``ops.yin`` (``frame``
    samples per analysis frame; ``tracker="pyin"``: ``ops.pyin``) on both sides; F0 gathered along the path.  a is the
    x side of the alignment, b the y side and the pitch reference.  -> {metric of ``WAVE_METRICS``: float64 [P]} plus
    ``path_len``."""
    if tracker not in PITCH_TRACKERS:
        raise ValueError(f"pitch tracker {tracker!r} not supported ({', '.join(PITCH_TRACKERS)})")
    track = ops.yin if tracker == "yin" else ops.pyin
    lens_a, lens_b = [int(v) for v in lens_a], [int(v) for v in lens_b]
    pre = pp["preprocessing"]
    sr, hop = pre["audio"]["sampling_rate"], pre["stft"]["hop_length"]
    wav_a, wav_b = wav_a.float().contiguous(), wav_b.float().contiguous()
    fa, frames_a = track(wav_a, lens_a, sr, hop, frame)[:2]  # also checks the lengths before anything else runs
    fb, frames_b = track(wav_b, lens_b, sr, hop, frame)[:2]
    stft = _front_end(pp)
    mel_a, mel_b = _logmel_rows(wav_a, lens_a, stft), _logmel_rows(wav_b, lens_b, stft)
    cost, path, plen = align(mel_a, frames_a, mel_b, frames_b, n_ceps)
    ia, ib, mask = _along(path, plen, frames_a, frames_b)
    err = prosody_errors(fa[ia], fb[ib], mask)
    out = {"wave_mcd_db": MCD_SCALE * cost.double() / plen.double(), "wave_vde": err["vde"], "wave_gpe": err["gpe"],
           "wave_ffe": err["ffe"], "wave_f0_rmse_cents": err["f0_rmse_cents"]}
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["path_len"] = plen.cpu().numpy()
    return res


def _recording(pp, spk: str, base: str) -> str:
    fn = os.path.join(pp["path"]["raw_path"], spk, f"{base}.wav")
    if not os.path.exists(fn):
        raise FileNotFoundError(f"waveform-level objective evaluation needs the recording of every listed utterance: "
                                f"{fn} is missing")
    return fn


def _get_vocoder(vocoder, configs, device):
    """``vocoder``: None = the configured one, "griffin_lim" / "hifigan" = that one, or a vocoder object."""
    if vocoder is not None and not isinstance(vocoder, str):
        return vocoder
    from ..utils.model import get_vocoder

    mc = configs[1]
    if vocoder is not None:
        names = {"griffin_lim": "GriffinLim", "hifigan": "HiFi-GAN"}
        if vocoder not in names:
            raise ValueError(f"vocoder {vocoder!r} not supported ({', '.join(names)})")
        mc = dict(mc, vocoder=dict(mc["vocoder"], model=names[vocoder]))
    return get_vocoder(mc, device, preprocess_config=configs[0])


def _vocode(vocoder, mel, frames, hop):
    """Synthesized mels [B, Tmax, n_mel] with host frame counts -> one fp32 waveform per utterance, on the mels'
    device.  Griffin-Lim returns hop * (T - 1) samples of an utterance of T frames, a generator T * hop."""
    from ..models.griffinlim import GriffinLim

    x = mel.to(getattr(vocoder, "mel_dtype", torch.bfloat16) if mel.is_cuda else torch.float32).contiguous()
    wav = vocoder.infer(x, lengths=frames).float().clamp(-1.0, 1.0)  # as written to a file
    short = hop if isinstance(vocoder, GriffinLim) else 0
    return [wav[i, :max(0, hop * T - short)] for i, T in enumerate(frames)]


def _load(root: str, kind: str, spk: str, base: str) -> np.ndarray:
    fn = os.path.join(root, kind, f"{spk}-{kind}-{base}.npy")
    if not os.path.exists(fn):
        raise FileNotFoundError(f"objective evaluation needs the ground truth of every listed utterance: {fn} is missing")
    return np.load(fn, allow_pickle=False)


def _frames(values: np.ndarray, durations: np.ndarray, level: str, T: int, what: str) -> np.ndarray:
    """A stored / predicted contour as T frame values: phoneme-level values repeated over their durations."""
    v = np.asarray(values, np.float64).reshape(-1)
    if level == "phoneme_level":
        if v.shape[0] != durations.shape[0]:
            raise ValueError(f"{what}: {v.shape[0]} phoneme values but {durations.shape[0]} durations")
        v = np.repeat(v, durations)
    if v.shape[0] < T:
        raise ValueError(f"{what}: {v.shape[0]} frame values for {T} mel frames")
    return v[:T]


def _summary(rows: List[dict], metrics=METRICS) -> Dict:
    out = {"n": len(rows), "n_empty": sum(1 for r in rows if r["pred_frames"] == 0), "mean": {}, "median": {}}
    for m in metrics:
        v = np.asarray([r[m] for r in rows], np.float64)
        v = v[~np.isnan(v)]
        out["mean"][m] = float(v.mean()) if v.size else float("nan")
        out["median"][m] = float(np.median(v)) if v.size else float("nan")
    return out


@torch.no_grad()
def evaluate_objective(model, configs, source: str, device, controls=(1.0, 1.0, 1.0), batch_size: int = 32,
                       out_dir: Optional[str] = None, n_ceps: int = 13, wave: bool = False, vocoder=None,
                       pitch_tracker: str = "yin") -> Dict:
    """Free-running synthesis (no targets, predicted durations) of every utterance of ``source`` (a ``val.txt``-style
    list) against its stored mel / pitch / energy / duration; one ``ops.dtw`` call per batch of pairs.
    -> {"n", "n_empty", "mean": {metric: value}, "median": {...}}; with ``out_dir`` also ``objective_summary.json``
    and the per-utterance ``objective.csv``.

    ``wave``: also the waveform-level ``WAVE_METRICS`` -- every synthesized mel is vocoded (``vocoder``: None = the
    configured one, ``"griffin_lim"`` needs no checkpoint, ``"hifigan"``, or a vocoder object) and compared with the
    recording ``<raw_path>/<speaker>/<basename>.wav`` at the configured rate (``wave_metrics``, F0 of both sides by
    ``pitch_tracker``; the summary names a tracker other than ``yin`` as ``"pitch_tracker"``).  A synthesis too short
    for the pitch tracker's frame has nan there."""
    from torch.utils.data import DataLoader

    from ..data.dataset import TextDataset, to_device

    pp = configs[0]
    root = pp["path"]["preprocessed_path"]
    st = _stats(root)
    levels = {"pitch": pp["preprocessing"]["pitch"]["feature"], "energy": pp["preprocessing"]["energy"]["feature"]}
    ds = TextDataset(source, pp)
    if len(ds) == 0:
        raise ValueError(f"objective evaluation: {source} lists no utterances")
    speaker_of = dict(zip(ds.basename, ds.speaker))
    dev = torch.device(device)
    model.eval()
    if pitch_tracker not in PITCH_TRACKERS:
        raise ValueError(f"pitch tracker {pitch_tracker!r} not supported ({', '.join(PITCH_TRACKERS)})")
    if wave:
        from ..audio.io import read_wav

        voc = _get_vocoder(vocoder, configs, dev)
        sr, hop = pp["preprocessing"]["audio"]["sampling_rate"], pp["preprocessing"]["stft"]["hop_length"]
        yin_frame = 1024
    rows: List[dict] = []
    for batch in DataLoader(ds, batch_size=batch_size, collate_fn=ds.collate_fn):
        names = batch[0]
        truth = []
        recs = [_recording(pp, speaker_of[base], base) for base in names] if wave else []
        for base in names:  # fail on a missing file before the model runs
            spk = speaker_of[base]
            dur = _load(root, "duration", spk, base).astype(np.int64).reshape(-1)
            mel = _load(root, "mel", spk, base).astype(np.float32)
            T = min(mel.shape[0], int(dur.sum()))
            if T < 1:
                raise ValueError(f"objective evaluation: {base} has no frames in its stored mel / durations")
            con = {k: _frames(_load(root, k, spk, base) * st[k][3] + st[k][2], dur, levels[k], T, f"{k} of {base}")
                   for k in ("pitch", "energy")}
            truth.append((mel[:T], con["pitch"], con["energy"], dur))
        b = to_device(batch, dev)
        out = model(*b[2:], p_control=controls[0], e_control=controls[1], d_control=controls[2])
        post, p, e, d = out[1].float(), out[2].float().cpu().numpy(), out[3].float().cpu().numpy(), out[5].cpu().numpy()
        src_lens, mel_lens = out[8].cpu().numpy(), out[9].cpu().numpy()
        keep = [i for i in range(len(names)) if int(mel_lens[i]) > 0]
        pred_con = {"pitch": [], "energy": []}
        pred_dur = [d[i, :int(src_lens[i])].astype(np.int64) for i in range(len(names))]
        for i, base in enumerate(names):
            if pred_dur[i].shape != truth[i][3].shape:
                raise ValueError(f"objective evaluation: {base} has {pred_dur[i].shape[0]} phonemes in {source} but "
                                 f"{truth[i][3].shape[0]} stored durations")
        for i in keep:
            n, T = int(src_lens[i]), int(mel_lens[i])
            for k, v in (("pitch", p), ("energy", e)):
                vals = v[i, :n] if levels[k] == "phoneme_level" else v[i, :T]
                pred_con[k].append(_frames(vals * st[k][3] + st[k][2], pred_dur[i], levels[k], T, f"predicted {k}"))
        res = {}
        if keep:
            f64 = lambda xs: torch.from_numpy(np.concatenate(xs)).to(dev)  # noqa: E731
            res = utterance_metrics(
                torch.cat([post[i, :int(mel_lens[i])] for i in keep]).contiguous(), [int(mel_lens[i]) for i in keep],
                torch.from_numpy(np.concatenate([truth[i][0] for i in keep])).to(dev), [truth[i][0].shape[0] for i in keep],
                f64(pred_con["pitch"]), f64([truth[i][1] for i in keep]), f64(pred_con["energy"]),
                f64([truth[i][2] for i in keep]), [pred_dur[i] for i in keep], [truth[i][3] for i in keep], n_ceps)
        wres, wat = {}, {}
        if wave:
            syn = dict(zip(keep, _vocode(voc, post[keep], [int(mel_lens[i]) for i in keep], hop))) if keep else {}
            rec = {}
            for i in keep:
                y = np.clip(read_wav(recs[i], sr)[0], -1.0, 1.0)
                if syn[i].shape[0] > yin_frame // 2 and y.shape[0] > yin_frame // 2:
                    rec[i] = torch.from_numpy(y).to(dev)
            wkeep = list(rec)
            wat = {i: k for k, i in enumerate(wkeep)}
            if wkeep:
                wres = wave_metrics(torch.cat([syn[i] for i in wkeep]), [syn[i].shape[0] for i in wkeep],
                                    torch.cat([rec[i] for i in wkeep]), [rec[i].shape[0] for i in wkeep], pp, n_ceps,
                                    yin_frame, pitch_tracker)
        at = {i: k for k, i in enumerate(keep)}
        for i, base in enumerate(names):
            row = {"basename": base, "pred_frames": int(mel_lens[i]), "true_frames": int(truth[i][0].shape[0])}
            for m in METRICS:
                row[m] = float(res[m][at[i]]) if i in at else float("nan")
            if i not in at:  # no alignment, but the duration figures stand
                row["dur_mae_frames"] = float(np.abs(pred_dur[i] - truth[i][3]).mean())
                row["len_ratio"] = 0.0
            row["path_len"] = int(res["path_len"][at[i]]) if i in at else 0
            for m in WAVE_METRICS if wave else ():
                row[m] = float(wres[m][wat[i]]) if i in wat else float("nan")
            rows.append(row)
    summary = _summary(rows, METRICS + WAVE_METRICS if wave else METRICS)
    if wave and pitch_tracker != "yin":
        summary["pitch_tracker"] = pitch_tracker
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, "objective_summary.json"), "w") as f:
            json.dump(summary, f, indent=2)
        with open(os.path.join(out_dir, "objective.csv"), "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(rows[0].keys()))
            w.writeheader()
            w.writerows(rows)
    return summary
