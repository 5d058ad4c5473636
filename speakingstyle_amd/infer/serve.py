"""Serving entry: one loaded model + vocoder, one call per utterance (``Synthesizer.tts`` -> int16 samples).

On the GPU every call goes through ``SynthGraphs(bucketed=True)`` (``infer/graphs.py``): after the first few
utterances have opened their buckets, an unseen text replays two captured HIP graphs.  On the CPU it is the ``synthesize``
path of the single mode (``infer/synthesis.py``) with the waveform returned instead of written.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from ..text import g2p
from .synthesis import reference_mel, single_batch, synthesize, word_level_controls


class Synthesizer:
    def __init__(self, configs, restore_step: int = 0, device=None, model=None, vocoder=None, warm: int = 1):
        """``configs``: (preprocess, model, train) dicts.  ``model`` / ``vocoder``: already built ones (eval, on
        ``device``); otherwise they are loaded as ``synthesize.py`` loads them."""
        from ..utils.model import get_model, get_vocoder

        self.configs = configs
        pp, mc, tc = configs
        self.device = torch.device(device if device is not None else ("cuda" if torch.cuda.is_available() else "cpu"))
        self.model = model if model is not None else get_model(restore_step, configs, self.device, train=False,
                                                               ignore_layers=tc.get("ignore_layers", []))
        self.vocoder = vocoder if vocoder is not None else get_vocoder(mc, self.device, preprocess_config=pp)
        pre = pp["preprocessing"]
        self.hop = pre["stft"]["hop_length"]
        self.sampling_rate = pre["audio"]["sampling_rate"]
        self.max_wav = pre["audio"]["max_wav_value"]
        self.lexicon = g2p.load_lexicon(pp["path"]["lexicon_path"], pre["text"].get("language", "en"))
        self._refs = {}  # reference wav path -> (mel [1, T, n_mel], mel_lens [1]) on the device
        self._prosody = {}  # prosody recording path -> ``transfer.recording_features`` on the device
        self.graphs = None
        if self.device.type == "cuda":
            from .graphs import SynthGraphs

            self.graphs = SynthGraphs(self.model, self.vocoder, int16_scale=self.max_wav, warm=warm, bucketed=True)

    @property
    def stats(self) -> Optional[dict]:
        """Capture / replay / eager counters of the graphs (None on the CPU)."""
        return None if self.graphs is None else dict(self.graphs.stats)

    def _reference(self, ref_audio):
        hit = self._refs.get(ref_audio)
        if hit is None:
            mel = torch.from_numpy(reference_mel(self.configs[0], ref_audio)[None]).to(self.device)
            hit = self._refs[ref_audio] = (mel, torch.tensor([mel.shape[1]], device=self.device))
        return hit

    def _prosody_features(self, path):
        hit = self._prosody.get(path)
        if hit is None:
            from .transfer import _load_recordings, recording_features

            hit = self._prosody[path] = recording_features(*_load_recordings([path], self.configs[0], self.device),
                                                            self.configs[0])
        return hit

    def _control(self, text, scalar, per_word):
        if per_word is None:
            return float(scalar)
        groups = g2p.word_groups(text, self.lexicon)
        return word_level_controls(groups, [float(v) for v in per_word], float(scalar))

    @torch.no_grad()
    def tts(self, text: str, speaker_id: int = 0, ref_audio: Optional[str] = None,
            style_weights: Optional[Sequence[float]] = None, pitch_control: float = 1.0, energy_control: float = 1.0,
            duration_control: float = 1.0, word_pitch=None, word_energy=None, word_duration=None,
            prosody_ref: Optional[str] = None, transfer=("pitch", "energy", "duration"), transfer_strength: float = 1.0,
            pitch_mode: str = "relative") -> np.ndarray:
        """One utterance -> int16 samples [mel frames * hop].  Style: ``ref_audio`` (a wav path; featurized once
        per path), else GST ``style_weights``, else neutral.  ``word_*``: one factor per word (scaled by the scalar
        control), as in the single mode.

        ``prosody_ref`` (a wav path; featurized once per path): say the text the way that recording says it --
        ``transfer`` names what is taken from it, ``transfer_strength`` in [0, 1] blends it with the model's own
        prediction, ``pitch_mode`` "relative" keeps the voice's own pitch level (``infer/transfer.py``).  Two eager
        passes; the captured graphs are neither used nor touched."""
        ctl = [self._control(text, s, w) for s, w in ((pitch_control, word_pitch), (energy_control, word_energy),
                                                      (duration_control, word_duration))]
        if prosody_ref:
            from .transfer import synthesize_like

            batch, _, use_ref = single_batch(text, self.configs[0], speaker_id, ref_audio, self.lexicon)
            out = synthesize_like(self.model, self.configs, batch, vocoder=self.vocoder, controls=ctl, use_ref=use_ref,
                                  style_weights=style_weights, what=transfer, strength=transfer_strength,
                                  pitch_mode=pitch_mode, features=self._prosody_features(prosody_ref))
            return out["wav"][0]
        batch, _, use_ref = single_batch(text, self.configs[0], speaker_id, None, self.lexicon)
        if self.graphs is None:
            if ref_audio:
                batch, _, use_ref = single_batch(text, self.configs[0], speaker_id, ref_audio, self.lexicon)
            out = synthesize(self.model, self.configs, None, [batch], ctl, None, use_ref=use_ref,
                             style_weights=style_weights)[0]
            from ..utils.model import vocoder_infer

            n = int(out[9][0])
            return vocoder_infer(out[1][:, :n].float(), self.vocoder, self.configs[1], self.configs[0],
                                 lengths=[n * self.hop], channel_last=True)[0]
        dev = self.device
        texts = torch.from_numpy(batch[3]).to(dev)
        src_lens = torch.from_numpy(batch[4]).to(dev)
        speakers = torch.from_numpy(batch[2]).to(dev)
        mels = mel_lens = max_mel = None
        if ref_audio:
            mels, mel_lens = self._reference(ref_audio)
            max_mel = mels.shape[1]
        sw = None if style_weights is None else torch.as_tensor(style_weights, device=dev).float().view(1, -1)
        ctl = [torch.as_tensor(c, device=dev).float().view(1, -1) if isinstance(c, np.ndarray) else c for c in ctl]
        wav, lens = self.graphs(speakers, texts, src_lens, int(batch[5]), mels, mel_lens, max_mel,
                                p_control=ctl[0], e_control=ctl[1], d_control=ctl[2], style_weights=sw)
        return wav[0, : lens[0] * self.hop].cpu().numpy()
