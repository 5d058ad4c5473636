"""Alignment learner: durations learned jointly with the model instead of read from forced-alignment TextGrids
(Badlani et al., "One TTS Alignment To Rule Them All", 2021).

A small text / mel attention gives lp [B, T, N], the log-probability of token n at mel frame t:

    keys    = conv k1(ReLU(conv k3(phoneme embeddings)))                     [B, N, hidden]
    queries = conv k1(ReLU(conv k1(ReLU(conv k3(target mel)))))              [B, T, hidden]
    score(t, n) = -temperature * |q_t - k_n|^2
    lp = log_softmax_n(score + log prior),   padded tokens masked to -inf before the softmax

trained with ``ops.align_forward_sum`` (the total probability of all monotone alignments); its Viterbi path
(``ops.align_mas``) gives the hard durations that the length regulator and the duration predictor use.  The prior is
the paper's beta-binomial prior along the diagonal, computed on the device from the lengths (``torch.lgamma``);
``prior_scaling`` multiplies its two shape parameters (larger: narrower around the diagonal; 0: no prior).
The convolutions go through ``ops.conv1d``; the score is one fp32 ``baddbmm`` plus the two squared norms.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from .layers import ConvHolder


def beta_binomial_log_prior(t_lens: torch.Tensor, n_lens: torch.Tensor, Tmax: int, Nmax: int,
                            scaling: float = 1.0) -> torch.Tensor:
    """log pmf of BetaBinomial(N_b, a = scaling (t + 1), b = scaling (T_b - t)) at token n, for frame t of utterance
    b -> [B, Tmax, Nmax] fp32: frame t of T expects token ~ N t / T, wide in the middle and narrow at both ends
    (the paper's prior, which scipy.stats.betabinom tabulates per utterance).  Cells outside an
    utterance's lattice hold finite filler values (they are masked or never read)."""
    dev = t_lens.device
    T = t_lens.to(torch.float32).view(-1, 1, 1)
    N = n_lens.to(torch.float32).view(-1, 1, 1)
    t = torch.minimum(torch.arange(Tmax, device=dev, dtype=torch.float32).view(1, -1, 1), T - 1)
    k = torch.minimum(torch.arange(Nmax, device=dev, dtype=torch.float32).view(1, 1, -1), N)
    a, b = scaling * (t + 1.0), scaling * (T - t)
    lg = torch.lgamma
    log_comb = lg(N + 1.0) - lg(k + 1.0) - lg(N - k + 1.0)
    return log_comb + lg(k + a) + lg(N - k + b) - lg(N + a + b) - (lg(a) + lg(b) - lg(a + b))


class AlignmentEncoder(nn.Module):
    def __init__(self, n_mel: int, d_text: int, cfg):
        super().__init__()
        h = int(cfg["hidden"])
        self.temperature = float(cfg["temperature"])
        self.prior_scaling = float(cfg["prior_scaling"])
        self.key_proj = nn.ModuleList([ConvHolder(d_text, 2 * h, 3), ConvHolder(2 * h, h, 1)])
        self.query_proj = nn.ModuleList([ConvHolder(n_mel, 2 * h, 3), ConvHolder(2 * h, h, 1), ConvHolder(h, h, 1)])

    def forward(self, mels, mel_lens, text_emb, src_lens):
        """mels [B, T, n_mel] and text_emb [B, N, d_text] in the compute dtype -> lp [B, T, N] fp32."""
        k = self.key_proj[1](self.key_proj[0](text_emb, "relu")).float()
        q = self.query_proj[2](self.query_proj[1](self.query_proj[0](mels, "relu"), "relu")).float()
        # -temperature * (|q|^2 + |k|^2 - 2 q.k)
        norms = (q * q).sum(-1, keepdim=True) + (k * k).sum(-1).unsqueeze(1)
        score = torch.baddbmm(norms, q, k.transpose(1, 2), beta=-self.temperature, alpha=2.0 * self.temperature)
        if self.prior_scaling:
            with torch.no_grad():
                prior = beta_binomial_log_prior(mel_lens, src_lens, score.shape[1], score.shape[2], self.prior_scaling)
            score = score + prior
        pad = ops.lengths_to_mask(src_lens, score.shape[2]).unsqueeze(1)
        return torch.log_softmax(score.masked_fill(pad, float("-inf")), dim=-1)
