"""Griffin-Lim vocoder: log-mel -> waveform with no trained weights (reference ``audio/audio_processing.py:66-82``,
``audio/tools.py:18-34``: pseudo-inverse mel basis, then phase reconstruction).

It offers the inference surface of ``hifigan.Generator`` so it can stand in wherever ``get_vocoder``'s result is
used (``vocoder_infer``, ``infer/serve.py::Synthesizer``, ``SynthGraphs``' eager branch).  On the GPU a batch is
one packed run of the kernels in ``csrc/k_griffin.hip`` (``ops.griffin_lim``): one launch per iteration for all
utterances, each reconstructed exactly as if alone; on the CPU it is the torch loop of ``ops.reference``.  The
mel is consumed in fp32.  An utterance of T frames has hop * (T - 1) samples (torch.istft), so the last ``hop``
samples of its T * hop slot are zero.  The initial phase is a hash of (seed, frame, bin): the same text gives the
same samples on every call.
"""
from __future__ import annotations

import torch

from .. import ops
from ..audio.stft import TacotronSTFT


class GriffinLim:
    mel_dtype = torch.float32  # what ``vocoder_infer`` hands over on the GPU (the generator takes bf16)

    def __init__(self, preprocess_config, n_iters: int = 60, momentum: float = 0.99, seed: int = 0):
        pre = preprocess_config["preprocessing"]
        s, m = pre["stft"], pre["mel"]
        self.stft = TacotronSTFT(s["filter_length"], s["hop_length"], s["win_length"], m["n_mel_channels"],
                                 pre["audio"]["sampling_rate"], m["mel_fmin"], m["mel_fmax"])
        self.n_fft, self.hop = self.stft.n_fft, self.stft.hop
        self.n_iters, self.momentum, self.seed = int(n_iters), float(momentum), int(seed)
        self._pinv = torch.linalg.pinv(self.stft.mel_basis).contiguous()  # [n_fft/2+1, n_mel], as inv_mel_spec
        self._dev = {}  # device -> (window, pinv)

    # ------------------------------------------------------------------ nn.Module-like surface (no parameters)
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        return self

    def requires_grad_(self, flag: bool = False):
        return self

    def packable(self) -> bool:
        """No capacity form: ``SynthGraphs`` runs this vocoder eagerly."""
        return False

    def _consts(self, device):
        c = self._dev.get(device)
        if c is None:
            c = self._dev[device] = (self.stft.fft_window(device), self._pinv.to(device))
        return c

    def _run(self, mel, lengths, int16_scale, width):
        window, pinv = self._consts(mel.device)
        return ops.griffin_lim(mel.float(), self.n_fft, self.hop, window, self.n_iters, self.momentum, seed=self.seed,
                               lengths=lengths, int16_scale=int16_scale, mel_pinv=pinv, width=width)

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def infer(self, mel_cl: torch.Tensor, int16_scale=None, lengths=None) -> torch.Tensor:
        """mel [B, T, n_mel] (channel-last log-mel) -> wav [B, T * hop] in [-1, 1], or int16 samples scaled by
        ``int16_scale``.  ``lengths``: host frame counts; samples from hop * (lengths[b] - 1) on are zero."""
        return self._run(mel_cl, lengths, int16_scale, mel_cl.shape[1] * self.hop)

    @torch.no_grad()
    def infer_packed(self, mel: torch.Tensor, lengths, int16_scale=None, width=None) -> torch.Tensor:
        """mel padded [B, M, n_mel] or packed [R, n_mel] rows + host frame ``lengths`` -> wav [B, W]
        (W = ``width`` or max(lengths) * hop)."""
        lens = [max(0, int(v)) for v in lengths]
        if mel.dim() == 3:
            lens = [min(n, mel.shape[1]) for n in lens]
        W = int(width) if width is not None else max(lens + [0]) * self.hop
        return self._run(mel, lens, int16_scale, W)

    @torch.no_grad()
    def __call__(self, mel: torch.Tensor) -> torch.Tensor:
        """mel [B, n_mel, T] (the generator's training layout) -> wav [B, 1, T * hop]."""
        return self.infer(mel.transpose(1, 2)).unsqueeze(1)
