"""Offline feature extraction (reference ``preprocessor/preprocessor.py``,
``preprocessor/{ljspeech,libritts,aishell3,bc_2013}.py``, ``prepare_align.py``).

Pipeline: ``prepare_align`` (resample + peak-normalise wavs, write ``.lab``
transcripts) -> Montreal Forced Aligner (external) -> ``Preprocessor.build_from_path``:
TextGrid phones + frame durations (leading/trailing silence trimmed), F0,
mel + energy (TacotronSTFT), optional phoneme-level averaging, outlier-robust
z-normalisation, ``stats.json`` / ``speakers.json`` / ``train.txt`` / ``val.txt``.
Output layout is the reference's.

Offline-image substitutions: TextGrids are parsed here (no ``tgt``); F0 is
pyworld's algorithm pair DIO + StoneMask re-implemented in the native host
runtime (``csrc/host_f0.cpp``, ``utils/native.dio/stonemask``), same frame period
(hop / sr) and 0 = unvoiced convention; numerical parity with pyworld itself is
unpinned (the library is not installable here).  ``preprocessing.pitch.extractor:
yin`` selects the vectorised YIN tracker below instead, ``pyin`` probabilistic YIN (``ops.pyin`` on a host tensor:
one smooth track per utterance, F0 quantised to bins of 2.5 cents).
Utterances are processed by a multiprocessing pool (the reference uses
joblib+dask, ``preprocessor/bc_2013.py:62-73``).

``preprocessing.duration.source: learned`` needs no aligner run and no TextGrids: the phones come from the
transcript through the text frontend (what ``synthesize.py`` feeds the model), the whole utterance's mel is
stored with frame-level energy and interpolated-F0 contours under ``energy/`` and ``pitch/``, and there is no
``duration/``: the model's alignment learner finds the durations in training (``models/aligner.py``).

``Preprocessor(config, device=...)`` (``preprocess.py --device cpu|cuda``) is the batched pipeline: the pool only
loads (wav, transcript / TextGrid slice), the main process packs about 64 utterances into one vector and runs
``ops.pyin`` / ``ops.yin``, ``ops.frame_features`` and ``ops.interp_unvoiced`` on it (HIP kernels on ``cuda``, the
torch references on ``cpu``), and the pitch / energy contours are normalised in memory and written once.  Drop rules,
statistics and metadata go through the same functions as the per-utterance path.
"""
from __future__ import annotations

import json
import os
import random
import re
import time
from multiprocessing import Pool
from typing import List, Optional, Tuple

import numpy as np

from ..audio.io import read_wav, write_wav
from ..audio.stft import TacotronSTFT, get_mel_from_wav
from ..text import cleaners as _cleaners

SIL_PHONES = ("sil", "sp", "spn", "")


# ------------------------------------------------------------------ TextGrid
def parse_textgrid(path: str):
    """-> {tier_name: [(start, end, text), ...]} for interval tiers.

    Both Praat formats reduce to the same value sequence -- long format: the values
    right of every ``=``; short format: every quoted string / number -- namely
    file-type, object-class, xmin, xmax, n_tiers, then per tier: class, name, xmin,
    xmax, n, and n (xmin, xmax, text) triples (point tiers: n (time, mark) pairs).
    """
    with open(path, encoding="utf-8") as f:
        raw = f.read()
    tok_re = r'"(?:[^"]|"")*"|[-+]?\d*\.?\d+(?:[eE][-+]?\d+)?'
    if re.search(r"^\s*xmin\s*=", raw, re.M):
        vals = re.findall(r"=\s*(" + tok_re + ")", raw)
    else:
        vals = re.findall(tok_re, raw)

    def unq(t):
        return t[1:-1].replace('""', '"') if t.startswith('"') else t

    vals = [unq(v) if v.startswith('"') else v for v in vals]
    i = 5  # skip header: type, class, xmin, xmax, n_tiers
    n_tiers = int(float(vals[4])) if len(vals) > 4 else 0
    tiers = {}
    for _ in range(n_tiers):
        cls, name = vals[i], vals[i + 1]
        n = int(float(vals[i + 4]))
        i += 5
        if cls == "IntervalTier":
            tiers[name] = [(float(vals[i + 3 * k]), float(vals[i + 3 * k + 1]), vals[i + 3 * k + 2]) for k in range(n)]
            i += 3 * n
        else:
            i += 2 * n
    return tiers


def get_alignment(intervals, sampling_rate: int, hop_length: int):
    """Phones + frame durations, trimming leading/trailing silences (``preprocessor.py:253-291``)."""
    phones: List[str] = []
    durations: List[int] = []
    start_time = end_time = 0.0
    end_idx = 0
    for s, e, p in intervals:
        if not phones:
            if p in SIL_PHONES:
                continue
            start_time = s
        if p not in SIL_PHONES:
            phones.append(p)
            end_time = e
            end_idx = len(phones)
        else:
            phones.append(p if p else "sp")
        durations.append(int(np.round(e * sampling_rate / hop_length) - np.round(s * sampling_rate / hop_length)))
    return phones[:end_idx], durations[:end_idx], start_time, end_time


# ------------------------------------------------------------------ F0 (YIN)
def yin_f0(wav: np.ndarray, sr: int, hop: int, fmin: float = 71.0, fmax: float = 800.0, frame: int = 1024,
           threshold: float = 0.15) -> np.ndarray:
    """Frame-synchronous F0 (Hz, 0 = unvoiced) with center padding like the STFT."""
    x = np.pad(wav.astype(np.float64), (frame // 2, frame // 2), mode="reflect")
    n_frames = 1 + (len(x) - frame) // hop
    tau_min = max(2, int(sr / fmax))
    tau_max = min(frame // 2, int(sr / fmin) + 1)
    idx = np.arange(frame)[None, :] + hop * np.arange(n_frames)[:, None]
    frames = x[idx]
    frames = frames - frames.mean(axis=1, keepdims=True)
    W = frame // 2
    # difference function via FFT autocorrelation: d(tau) = r(0)_t + r(0)_{t+tau} - 2 r(tau)
    fft_n = 1 << int(np.ceil(np.log2(2 * frame)))
    F = np.fft.rfft(frames, fft_n, axis=1)
    acf = np.fft.irfft(F * np.conj(np.fft.rfft(frames[:, :W], fft_n, axis=1)), fft_n, axis=1)[:, : W + 1]
    sq = np.cumsum(frames ** 2, axis=1)
    e0 = sq[:, W - 1:W]
    taus = np.arange(1, W + 1)
    e_tau = sq[:, taus + W - 1] - sq[:, taus - 1]
    d = np.concatenate([np.zeros((n_frames, 1)), e0 + e_tau - 2 * acf[:, 1:]], axis=1)
    cmnd = d.copy()
    csum = np.cumsum(d[:, 1:], axis=1)
    cmnd[:, 1:] = d[:, 1:] * taus[None, :] / np.maximum(csum, 1e-12)
    cmnd[:, 0] = 1.0
    f0 = np.zeros(n_frames)
    region = cmnd[:, tau_min:tau_max]
    below = region < threshold
    has = below.any(axis=1)
    first = np.argmax(below, axis=1)
    for i in np.nonzero(has)[0]:
        t = first[i] + tau_min
        while t + 1 < tau_max and cmnd[i, t + 1] < cmnd[i, t]:
            t += 1
        if 1 <= t < W:  # parabolic interpolation
            a, b, c = cmnd[i, t - 1], cmnd[i, t], cmnd[i, t + 1]
            den = a - 2 * b + c
            t = t + (0.5 * (a - c) / den if abs(den) > 1e-12 else 0.0)
        f0[i] = sr / t
    energy_gate = np.sqrt(e0[:, 0] / W) > 1e-4
    return (f0 * energy_gate).astype(np.float64)


def extract_f0(wav: np.ndarray, sr: int, hop: int, method: str = "dio") -> np.ndarray:
    """Frame F0 (Hz, 0 = unvoiced) on the hop grid.  ``dio``: DIO + StoneMask exactly as
    the reference calls pyworld (``preprocessor/preprocessor.py:182-187``: float64 wav,
    frame_period = hop / sr * 1000 ms, default floor/ceil 71/800 Hz)."""
    if method == "dio":
        from ..utils import native

        x = wav.astype(np.float64)
        f0, t = native.dio(x, sr, frame_period=hop / sr * 1000)
        return native.stonemask(x, f0, t, sr)
    if method == "yin":
        return yin_f0(wav, sr, hop)
    if method == "pyin":
        import torch

        from .. import ops

        # a host tensor: the workers of the preprocessing pool never open the GPU
        x = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32))
        return ops.pyin(x, [x.shape[0]], sr, hop)[0].double().numpy()
    raise ValueError(f"unknown pitch extractor {method!r} (dio | yin | pyin)")


def interpolate_unvoiced(pitch: np.ndarray) -> np.ndarray:
    nz = np.nonzero(pitch)[0]
    if len(nz) == 0:
        return pitch
    return np.interp(np.arange(len(pitch)), nz, pitch[nz])


def phoneme_average(values: np.ndarray, durations: List[int]) -> np.ndarray:
    out = np.zeros(len(durations))
    pos = 0
    for i, d in enumerate(durations):
        out[i] = np.mean(values[pos:pos + d]) if d > 0 else 0.0
        pos += d
    return out


def remove_outlier(values: np.ndarray) -> np.ndarray:
    values = np.asarray(values)
    if values.size == 0:
        return values
    p25, p75 = np.percentile(values, [25, 75])
    lo, hi = p25 - 1.5 * (p75 - p25), p75 + 1.5 * (p75 - p25)
    return values[(values > lo) & (values < hi)]


class RunningMoments:
    """StandardScaler.partial_fit equivalent (Chan's parallel update)."""

    def __init__(self):
        self.n, self.mean, self.m2 = 0, 0.0, 0.0

    def update(self, x):
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        if x.size == 0:
            return
        n_b, mean_b = x.size, float(x.mean())
        m2_b = float(((x - mean_b) ** 2).sum())
        n = self.n + n_b
        delta = mean_b - self.mean
        self.mean += delta * n_b / n
        self.m2 += m2_b + delta * delta * self.n * n_b / n
        self.n = n

    @property
    def std(self):
        return float(np.sqrt(self.m2 / self.n)) if self.n else 1.0


# ------------------------------------------------------------------ Preprocessor
class Preprocessor:
    BATCH_UTTERANCES = 64         # utterances per packed batch of the device pipeline ...
    BATCH_SAMPLES = 64 * 12 * 22050  # ... and its cap on packed samples (a batch always holds one utterance)
    DEVICE_EXTRACTORS = ("pyin", "yin")

    def __init__(self, config, model_config=None, device=None):  # second arg accepted for CLI compatibility
        """``device``: None = the per-utterance host pipeline; "cpu" / "cuda" (or a ``torch.device``) = the batched
        pipeline with the packed ops on that device."""
        self.config = config
        pp = config["preprocessing"]
        self.in_dir = config["path"]["raw_path"]
        self.out_dir = config["path"]["preprocessed_path"]
        self.val_size = pp["val_size"]
        self.sampling_rate = pp["audio"]["sampling_rate"]
        self.hop_length = pp["stft"]["hop_length"]
        self.pitch_phoneme = pp["pitch"]["feature"] == "phoneme_level"
        self.energy_phoneme = pp["energy"]["feature"] == "phoneme_level"
        self.pitch_norm = pp["pitch"]["normalization"]
        self.energy_norm = pp["energy"]["normalization"]
        self.f0_method = pp["pitch"].get("extractor", "dio")
        self.device = None
        if device is not None:
            import torch

            if self.f0_method not in self.DEVICE_EXTRACTORS:
                raise ValueError(f"preprocessing.pitch.extractor: {self.f0_method!r} has no packed kernel; with a device "
                                 f"it must be one of {' | '.join(self.DEVICE_EXTRACTORS)}")
            self.device = torch.device(device)
        self.timings = {"load": 0.0, "kernels": 0.0, "write": 0.0}  # seconds of the batched pipeline's main process
        self.learned = (pp.get("duration") or {}).get("source", "textgrid") == "learned"
        self.language = pp["text"].get("language", "en")
        self.cleaners = pp["text"]["text_cleaners"]
        self._lexicon = None
        self.stft = TacotronSTFT(pp["stft"]["filter_length"], self.hop_length, pp["stft"]["win_length"],
                                 pp["mel"]["n_mel_channels"], self.sampling_rate, pp["mel"]["mel_fmin"],
                                 pp["mel"]["mel_fmax"])

    def process_utterance(self, speaker: str, basename: str):
        wav_path = os.path.join(self.in_dir, speaker, f"{basename}.wav")
        lab_path = os.path.join(self.in_dir, speaker, f"{basename}.lab")
        tg_path = os.path.join(self.out_dir, "TextGrid", speaker, f"{basename}.TextGrid")
        tiers = parse_textgrid(tg_path)
        phone, duration, start, end = get_alignment(tiers.get("phones", []), self.sampling_rate, self.hop_length)
        if start >= end or not phone:
            return None
        text = "{" + " ".join(phone) + "}"
        wav, _ = read_wav(wav_path, self.sampling_rate)
        wav = wav[int(self.sampling_rate * start): int(self.sampling_rate * end)].astype(np.float32)
        with open(lab_path, encoding="utf-8") as f:
            raw_text = f.readline().strip("\n")
        pitch = extract_f0(wav, self.sampling_rate, self.hop_length, self.f0_method)
        mel, energy = get_mel_from_wav(np.clip(wav, -1, 1), self.stft)
        T = sum(duration)
        pitch, mel, energy = pitch[:T], mel[:, :T], energy[:T]
        if pitch.shape[0] < T or np.sum(pitch != 0) <= 1:
            return None
        if self.pitch_phoneme:
            pitch = phoneme_average(interpolate_unvoiced(pitch), duration)
        if self.energy_phoneme:
            energy = phoneme_average(energy, duration)
        for kind, arr in (("duration", np.asarray(duration)), ("pitch", pitch), ("energy", energy), ("mel", mel.T)):
            np.save(os.path.join(self.out_dir, kind, f"{speaker}-{kind}-{basename}.npy"), arr)
        return "|".join([basename, speaker, text, raw_text]), remove_outlier(pitch), remove_outlier(energy), mel.shape[1]

    def transcript_phones(self, raw_text: str) -> List[str]:
        """Phones of a transcript through the text frontend, as synthesis produces them (lexicon + letter-to-sound
        for English, the pinyin lexicon for Mandarin)."""
        from ..text import g2p

        if self._lexicon is None:
            self._lexicon = g2p.load_lexicon(self.config["path"]["lexicon_path"], self.language)
        if self.language == "zh":
            return g2p.mandarin_phones(raw_text.split(), self._lexicon)
        return g2p.english_to_phones(raw_text, self._lexicon)

    def process_utterance_unaligned(self, speaker: str, basename: str):
        """``duration.source: learned``: phones from the transcript, the whole utterance's mel, frame-level energy
        and interpolated F0.  -> the ``process_utterance`` tuple, None (no usable pitch / no phones), or
        ``"short"`` for an utterance with fewer frames than phones (no monotone alignment exists)."""
        from ..text import text_to_sequence

        wav_path = os.path.join(self.in_dir, speaker, f"{basename}.wav")
        lab_path = os.path.join(self.in_dir, speaker, f"{basename}.lab")
        with open(lab_path, encoding="utf-8") as f:
            raw_text = f.readline().strip("\n")
        phone = self.transcript_phones(raw_text)
        text = "{" + " ".join(phone) + "}"
        n_phone = len(text_to_sequence(text, self.cleaners))
        if n_phone == 0:
            return None
        wav, _ = read_wav(wav_path, self.sampling_rate)
        wav = wav.astype(np.float32)
        pitch = extract_f0(wav, self.sampling_rate, self.hop_length, self.f0_method)
        mel, energy = get_mel_from_wav(np.clip(wav, -1, 1), self.stft)
        T = min(mel.shape[1], pitch.shape[0])
        pitch, mel, energy = pitch[:T], mel[:, :T], energy[:T]
        if T < n_phone:
            return "short"
        if np.sum(pitch != 0) <= 1:
            return None
        pitch = interpolate_unvoiced(pitch)
        for kind, arr in (("pitch", pitch), ("energy", energy), ("mel", mel.T)):
            np.save(os.path.join(self.out_dir, kind, f"{speaker}-{kind}-{basename}.npy"), arr)
        return "|".join([basename, speaker, text, raw_text]), remove_outlier(pitch), remove_outlier(energy), mel.shape[1]

    # ------------------------------------------------------------ batched pipeline (device is not None)
    def load_utterance(self, speaker: str, basename: str):
        """The host half of an utterance, as the per-utterance path does it up to the features (runs in the pool and
        never touches a device): transcript / phones, the wav (resampled; the TextGrid slice [start, end)) and the
        durations.  -> None (no phones) or (info line, wav float32 [N], durations | None, phones)."""
        wav_path = os.path.join(self.in_dir, speaker, f"{basename}.wav")
        lab_path = os.path.join(self.in_dir, speaker, f"{basename}.lab")
        if self.learned:
            from ..text import text_to_sequence

            with open(lab_path, encoding="utf-8") as f:
                raw_text = f.readline().strip("\n")
            phone = self.transcript_phones(raw_text)
            text = "{" + " ".join(phone) + "}"
            n_phone = len(text_to_sequence(text, self.cleaners))
            if n_phone == 0:
                return None
            wav, _ = read_wav(wav_path, self.sampling_rate)
            return "|".join([basename, speaker, text, raw_text]), wav.astype(np.float32), None, n_phone
        tg_path = os.path.join(self.out_dir, "TextGrid", speaker, f"{basename}.TextGrid")
        tiers = parse_textgrid(tg_path)
        phone, duration, start, end = get_alignment(tiers.get("phones", []), self.sampling_rate, self.hop_length)
        if start >= end or not phone:
            return None
        text = "{" + " ".join(phone) + "}"
        wav, _ = read_wav(wav_path, self.sampling_rate)
        wav = wav[int(self.sampling_rate * start): int(self.sampling_rate * end)].astype(np.float32)
        with open(lab_path, encoding="utf-8") as f:
            raw_text = f.readline().strip("\n")
        return "|".join([basename, speaker, text, raw_text]), wav, duration, len(duration)

    def _batch_features(self, batch, window, basis):
        """One packed batch on the device: a single H2D of the samples, F0 on the unclipped samples, log-mel / energy
        on the clipped ones, the contours over the frames every utterance keeps, and a single D2H.
        -> per utterance (mel [T, n_mel], energy [T], f0 [T], contour [T], n_voiced) as host arrays, T = the frames
        kept (all of them with learned durations, min(frames, sum(durations)) with TextGrids)."""
        import torch

        from .. import ops

        dev = self.device
        lens = [len(b[1]) for b in batch]
        x = torch.from_numpy(np.ascontiguousarray(np.concatenate([b[1] for b in batch]), dtype=np.float32))
        if dev.type == "cuda":
            x = x.pin_memory().to(dev, non_blocking=True)
        if self.f0_method == "pyin":
            f0, frames, _ = ops.pyin(x, lens, self.sampling_rate, self.hop_length)
        else:
            f0, frames = ops.yin(x, lens, self.sampling_rate, self.hop_length)
        mel, energy, _ = ops.frame_features(x, lens, self.stft.n_fft, self.hop_length, window, basis, 1e-5,
                                            clip_wave=True)
        keep = [T if b[2] is None else min(T, sum(b[2])) for b, T in zip(batch, frames)]
        starts = np.concatenate([[0], np.cumsum(frames)])
        if keep != frames:  # interpolate_unvoiced sees the truncated contour: its held ends depend on the cut
            rows = np.concatenate([np.arange(a, a + k) for a, k in zip(starts[:-1], keep)])
            f0 = f0[torch.from_numpy(rows).to(dev)]
        contour, n_voiced = ops.interp_unvoiced(f0, keep)
        n_mel, R, Rk = mel.shape[1], mel.shape[0], f0.shape[0]
        flat = torch.cat([mel.reshape(-1), energy, f0, contour, n_voiced.to(torch.float32)]).cpu().numpy()
        mel, energy = flat[:R * n_mel].reshape(R, n_mel), flat[R * n_mel:R * n_mel + R]
        f0, contour = flat[R * n_mel + R:][:Rk], flat[R * n_mel + R + Rk:][:Rk]
        n_voiced = flat[R * n_mel + R + 2 * Rk:]
        out, at = [], 0
        for a, k, nv in zip(starts[:-1], keep, n_voiced):
            out.append((mel[a:a + k], energy[a:a + k], f0[at:at + k], contour[at:at + k], int(nv)))
            at += k
        return out, frames

    def _finish_utterance(self, item, feats, frames):
        """The per-utterance rules of ``process_utterance`` / ``process_utterance_unaligned`` on a batch's features:
        -> None / "short" (dropped) or (info, pitch float64, energy, mel [T, n_mel])."""
        info, _, duration, n_phone = item
        mel, energy, f0, contour, n_voiced = feats
        if self.learned:
            if mel.shape[0] < n_phone:
                return "short"
            if n_voiced <= 1:
                return None
            return info, contour.astype(np.float64), energy.copy(), mel
        T = sum(duration)
        if frames < T or n_voiced <= 1:
            return None
        pitch = f0.astype(np.float64)
        if self.pitch_phoneme:
            pitch = phoneme_average(contour.astype(np.float64), duration)
        energy = phoneme_average(energy, duration) if self.energy_phoneme else energy.copy()
        return info, pitch, energy, mel

    def _build_batched(self, speakers, jobs, workers: int):
        import multiprocessing

        dev = self.device
        window = self.stft.fft_window(dev)
        basis = self.stft.mel_basis.to(device=dev, dtype=window.dtype).contiguous()
        shortest = max(self.stft.n_fft, 1024) // 2  # reflect padding of the STFT and of the pitch tracker's frame
        self.timings = {"load": 0.0, "kernels": 0.0, "write": 0.0}
        out, held, pm, em = [], [], RunningMoments(), RunningMoments()
        n_frames = n_short = 0

        def flush(batch):
            nonlocal n_frames, n_short
            t0 = time.perf_counter()
            feats, frames = self._batch_features(batch, window, basis)
            t1 = time.perf_counter()
            for item, ft, T in zip(batch, feats, frames):
                r = self._finish_utterance(item, ft, T)
                if isinstance(r, str):
                    n_short += 1
                if r is None or isinstance(r, str):
                    continue
                info, pitch, energy, mel = r
                basename, speaker = info.split("|")[:2]
                if not self.learned:
                    np.save(os.path.join(self.out_dir, "duration", f"{speaker}-duration-{basename}.npy"),
                            np.asarray(item[2]))
                np.save(os.path.join(self.out_dir, "mel", f"{speaker}-mel-{basename}.npy"), mel)
                held.append((f"{speaker}-{{}}-{basename}.npy", pitch, energy))
                out.append(info)
                pm.update(remove_outlier(pitch))
                em.update(remove_outlier(energy))
                n_frames += mel.shape[0]
            self.timings["kernels"] += t1 - t0
            self.timings["write"] += time.perf_counter() - t1

        pool = None
        if workers > 1:  # fresh processes: the workers only load, and never inherit an open GPU from this one
            pool = multiprocessing.get_context("spawn").Pool(min(workers, 16), initializer=_init_loader,
                                                             initargs=(self.config,))
            items = pool.imap(_load_job, jobs, chunksize=4)
        else:
            items = (self.load_utterance(s, b) for s, b in jobs)
        try:
            batch, samples = [], 0
            t0 = time.perf_counter()
            for (speaker, basename), item in zip(jobs, items):
                if item is None:
                    continue
                if len(item[1]) <= shortest:
                    raise ValueError(f"{speaker}/{basename}: {len(item[1])} samples; the features need more than "
                                     f"{shortest}")
                if batch and (len(batch) >= self.BATCH_UTTERANCES or samples + len(item[1]) > self.BATCH_SAMPLES):
                    self.timings["load"] += time.perf_counter() - t0
                    flush(batch)
                    batch, samples = [], 0
                    t0 = time.perf_counter()
                batch.append(item)
                samples += len(item[1])
            self.timings["load"] += time.perf_counter() - t0
            if batch:
                flush(batch)
        finally:
            if pool is not None:
                pool.terminate()
                pool.join()
        if n_short:
            print(f"Dropped {n_short} utterances with fewer mel frames than phones")
        t0 = time.perf_counter()
        p_mean, p_std = (pm.mean, pm.std) if self.pitch_norm else (0.0, 1.0)
        e_mean, e_std = (em.mean, em.std) if self.energy_norm else (0.0, 1.0)
        p_min, p_max = self._write_normalized("pitch", [(h[0], h[1]) for h in held], p_mean, p_std)
        e_min, e_max = self._write_normalized("energy", [(h[0], h[2]) for h in held], e_mean, e_std)
        self.timings["write"] += time.perf_counter() - t0
        return self.write_metadata(speakers, out, (p_min, p_max, p_mean, p_std), (e_min, e_max, e_mean, e_std), n_frames)

    def _write_normalized(self, kind, held, mean, std):
        """``normalize`` on the contours still in memory: each is normalised and written once -> (min, max)."""
        lo, hi = np.finfo(np.float64).max, np.finfo(np.float64).min
        for name, v in held:
            v = self.normalized(v, mean, std)
            np.save(os.path.join(self.out_dir, kind, name.format(kind)), v)
            if v.size:
                lo, hi = min(lo, float(v.min())), max(hi, float(v.max()))
        return lo, hi

    def list_jobs(self):
        """-> ({speaker: id}, [(speaker, basename)]) in sorted order: every wav with a transcript (learned durations)
        or a TextGrid."""
        speakers = {}
        jobs: List[Tuple[str, str]] = []
        for i, spk in enumerate(sorted(os.listdir(self.in_dir))):
            spk_dir = os.path.join(self.in_dir, spk)
            if not os.path.isdir(spk_dir):
                continue
            speakers[spk] = len(speakers)
            for fn in sorted(os.listdir(spk_dir)):
                if fn.endswith(".wav"):
                    base = fn[:-4]
                    if self.learned:
                        if os.path.exists(os.path.join(spk_dir, f"{base}.lab")):
                            jobs.append((spk, base))
                    elif os.path.exists(os.path.join(self.out_dir, "TextGrid", spk, f"{base}.TextGrid")):
                        jobs.append((spk, base))
        return speakers, jobs

    def write_metadata(self, speakers, out, pitch_stats, energy_stats, n_frames):
        """``speakers.json``, ``stats.json`` ([min, max, mean, std] each), the 1234-seeded shuffle and ``train.txt`` /
        ``val.txt``."""
        with open(os.path.join(self.out_dir, "speakers.json"), "w") as f:
            json.dump(speakers, f)
        with open(os.path.join(self.out_dir, "stats.json"), "w") as f:
            json.dump({"pitch": list(pitch_stats), "energy": list(energy_stats)}, f)
        random.Random(1234).shuffle(out)
        val = out[: self.val_size]
        train = out[self.val_size:]
        with open(os.path.join(self.out_dir, "train.txt"), "w", encoding="utf-8") as f:
            f.write("".join(x + "\n" for x in train))
        with open(os.path.join(self.out_dir, "val.txt"), "w", encoding="utf-8") as f:
            f.write("".join(x + "\n" for x in val))
        print("Total time: {:.2f} hours".format(n_frames * self.hop_length / self.sampling_rate / 3600))
        return out

    def build_from_path(self, workers: int = 4):
        for kind in ("mel", "pitch", "energy") + (() if self.learned else ("duration",)):
            os.makedirs(os.path.join(self.out_dir, kind), exist_ok=True)
        speakers, jobs = self.list_jobs()
        if self.device is not None:
            return self._build_batched(speakers, jobs, workers)
        one = self.process_utterance_unaligned if self.learned else self.process_utterance
        if workers > 1:
            with Pool(workers) as pool:
                results = pool.starmap(one, jobs)
        else:
            results = [one(s, b) for s, b in jobs]
        out, pm, em = [], RunningMoments(), RunningMoments()
        n_frames = 0
        n_short = sum(1 for r in results if isinstance(r, str))
        if n_short:
            print(f"Dropped {n_short} utterances with fewer mel frames than phones")
        for r in results:
            if r is None or isinstance(r, str):
                continue
            info, p, e, n = r
            out.append(info)
            pm.update(p)
            em.update(e)
            n_frames += n
        p_mean, p_std = (pm.mean, pm.std) if self.pitch_norm else (0.0, 1.0)
        e_mean, e_std = (em.mean, em.std) if self.energy_norm else (0.0, 1.0)
        p_min, p_max = self.normalize(os.path.join(self.out_dir, "pitch"), p_mean, p_std)
        e_min, e_max = self.normalize(os.path.join(self.out_dir, "energy"), e_mean, e_std)
        return self.write_metadata(speakers, out, (p_min, p_max, p_mean, p_std), (e_min, e_max, e_mean, e_std), n_frames)

    @staticmethod
    def normalized(v, mean, std):
        return (v - mean) / std

    @staticmethod
    def normalize(in_dir, mean, std):
        lo, hi = np.finfo(np.float64).max, np.finfo(np.float64).min
        for fn in os.listdir(in_dir):
            p = os.path.join(in_dir, fn)
            v = Preprocessor.normalized(np.load(p), mean, std)
            np.save(p, v)
            if v.size:
                lo, hi = min(lo, float(v.min())), max(hi, float(v.max()))
        return lo, hi


# ------------------------------------------------------------------ loader pool of the batched pipeline
_loader = None


def _init_loader(config):
    global _loader
    _loader = Preprocessor(config)


def _load_job(job):
    return _loader.load_utterance(*job)


# ------------------------------------------------------------------ prepare_align
def _write_pair(out_dir, speaker, base, wav, sr_in, sr, max_wav_value, text):
    os.makedirs(os.path.join(out_dir, speaker), exist_ok=True)
    wav = np.asarray(wav, dtype=np.float64)
    if sr_in != sr:
        from math import gcd

        from scipy.signal import resample_poly

        g = gcd(sr_in, sr)
        wav = resample_poly(wav, sr // g, sr_in // g)
    wav = wav / max(np.abs(wav).max(), 1e-8) * max_wav_value
    write_wav(os.path.join(out_dir, speaker, f"{base}.wav"), sr, wav.astype(np.int16))
    with open(os.path.join(out_dir, speaker, f"{base}.lab"), "w", encoding="utf-8") as f:
        f.write(text)


def _clean(text, names):
    for n in names:
        text = getattr(_cleaners, n)(text)
    return text


def prepare_align(config):
    """Dataset dispatcher (reference ``prepare_align.py:8-17``)."""
    ds = config["dataset"]
    in_dir = config["path"]["corpus_path"]
    out_dir = config["path"]["raw_path"]
    sr = config["preprocessing"]["audio"]["sampling_rate"]
    mx = config["preprocessing"]["audio"]["max_wav_value"] - 1  # stay inside int16
    names = config["preprocessing"]["text"]["text_cleaners"]
    n = 0
    if ds in ("LJSpeech", "BC2013"):
        meta = os.path.join(in_dir, "metadata.csv")
        spk = ds
        with open(meta, encoding="utf-8") as f:
            for line in f:
                parts = line.strip().split("|")
                if len(parts) < 2:
                    continue
                base, text = parts[0], parts[-1]
                wp = os.path.join(in_dir, "wavs", f"{base}.wav")
                if os.path.exists(wp):
                    wav, sr_in = read_wav(wp)
                    _write_pair(out_dir, spk, base, wav, sr_in, sr, mx, _clean(text, names))
                    n += 1
    elif ds == "LibriTTS":
        for spk in sorted(os.listdir(in_dir)):
            for chap in sorted(os.listdir(os.path.join(in_dir, spk))):
                d = os.path.join(in_dir, spk, chap)
                for fn in sorted(os.listdir(d)):
                    if not fn.endswith(".wav"):
                        continue
                    base = fn[:-4]
                    tp = os.path.join(d, f"{base}.normalized.txt")
                    if not os.path.exists(tp):
                        continue
                    with open(tp, encoding="utf-8") as f:
                        text = _clean(f.readline().strip(), names)
                    wav, sr_in = read_wav(os.path.join(d, fn))
                    _write_pair(out_dir, spk, base, wav, sr_in, sr, mx, text)
                    n += 1
    elif ds == "AISHELL3":
        for split in ("train", "test"):
            content = os.path.join(in_dir, split, "content.txt")
            if not os.path.exists(content):
                continue
            with open(content, encoding="utf-8") as f:
                for line in f:
                    wav_name, text = line.strip("\n").split("\t")
                    spk = wav_name[:7]
                    text = " ".join(text.split(" ")[1::2])  # pinyin tokens
                    wp = os.path.join(in_dir, split, "wav", spk, wav_name)
                    if os.path.exists(wp):
                        wav, sr_in = read_wav(wp)
                        _write_pair(out_dir, spk, wav_name[:-4], wav, sr_in, sr, mx, text)
                        n += 1
    else:
        raise ValueError(f"unknown dataset {ds!r}")
    return n
