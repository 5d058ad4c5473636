"""Plain-PyTorch implementations of every fused op (channel-last ``[B, L, C]``).

These are (a) the CPU execution path (BASELINE config #1: "tiny on CPU,
plumbing") and (b) the fp32 numerics oracle the HIP kernels are tested against
(``tests/test_kernels_gpu.py``).  They intentionally mirror the *math* of the
reference modules, cited per function, not their code structure: the reference
works in ``[B, C, L]`` for convolutions with transposes around every conv
(``model/modules.py:300-305``), we stay channel-last.
"""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch
import torch.nn.functional as F


def lengths_to_mask(lengths: torch.Tensor, max_len: int) -> torch.Tensor:
    """True = padding (reference ``utils/tools.py:110-118`` semantics)."""
    ids = torch.arange(max_len, device=lengths.device)
    return ids.unsqueeze(0) >= lengths.unsqueeze(1)


def sinusoid_table(n_position: int, d_hid: int, device=None, dtype=torch.float32) -> torch.Tensor:
    """Sinusoid PE, dim 2i -> sin, 2i+1 -> cos, angle = pos / 10000^(2*(i//2)/d)
    (reference ``transformer/Models.py:10-30``), computed in float64 like numpy."""
    pos = torch.arange(n_position, dtype=torch.float64, device=device).unsqueeze(1)
    idx = torch.arange(d_hid, dtype=torch.float64, device=device)
    angle = pos / torch.pow(10000.0, 2.0 * torch.div(idx, 2, rounding_mode="floor") / d_hid)
    out = torch.empty_like(angle)
    out[:, 0::2] = torch.sin(angle[:, 0::2])
    out[:, 1::2] = torch.cos(angle[:, 1::2])
    return out.to(dtype)


def linear(x, w, b=None, act: Optional[str] = None):
    y = F.linear(x, w.to(x.dtype), None if b is None else b.to(x.dtype))
    return _act(y, act)


def _act(y, act):
    if act is None:
        return y
    if act == "relu":
        return F.relu(y)
    if act == "lrelu":
        return F.leaky_relu(y, 0.1)
    if act == "tanh":
        return torch.tanh(y)
    raise ValueError(act)


def conv1d(x, w, b=None, pad: int = 0, dil: int = 1, act: Optional[str] = None):
    """Channel-last Conv1d: x [B, L, Cin], w [Cout, Cin, K] (PyTorch layout) -> [B, L', Cout]."""
    y = F.conv1d(x.transpose(1, 2), w.to(x.dtype), None if b is None else b.to(x.dtype), padding=pad, dilation=dil)
    return _act(y.transpose(1, 2), act)


def conv_transpose1d(x, w, b, stride: int, pad: int):
    """Channel-last ConvTranspose1d: w [Cin, Cout, K]."""
    y = F.conv_transpose1d(x.transpose(1, 2), w.to(x.dtype), None if b is None else b.to(x.dtype), stride=stride, padding=pad)
    return y.transpose(1, 2)


def attention(qkv: torch.Tensor, lengths: torch.Tensor, n_head: int) -> torch.Tensor:
    """Scaled dot-product MHA core with key-padding mask.

    qkv: [B, L, 3*H*dk] = [q | k | v] with head-major channels (h*dk + d), exactly
    the reference's ``view(sz_b, len, n_head, d_k)`` split (``transformer/SubLayers.py:39-44``).
    Softmax over keys with keys >= length masked to -inf (``transformer/Modules.py:14-21``).
    Returns [B, L, H*dk].  Query rows >= length are zero: the reference computes them and
    masks them after the block (``transformer/Layers.py:27``); every consumer here masks
    them too, so defining them as 0 lets the kernels skip padded query tiles entirely.
    """
    B, L, C3 = qkv.shape
    D = C3 // (3 * n_head)
    q, k, v = qkv.view(B, L, 3, n_head, D).permute(2, 0, 3, 1, 4).unbind(0)  # [B,H,L,D]
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) / math.sqrt(D)
    key_pad = lengths_to_mask(lengths, L)[:, None, None, :]
    s = s.masked_fill(key_pad, float("-inf"))
    p = torch.softmax(s, dim=-1)
    o = torch.matmul(p, v.float()).masked_fill(lengths_to_mask(lengths, L)[:, None, :, None], 0.0).to(qkv.dtype)
    return o.permute(0, 2, 1, 3).reshape(B, L, n_head * D)


def film(x, gamma, beta, s_gamma, s_beta):
    """(s_g*g + 1) * x + s_b*b, gamma/beta [B, C] broadcast over L (``model/blocks.py:54-62``)."""
    g = (s_gamma * gamma).unsqueeze(1)
    bb = (s_beta * beta).unsqueeze(1)
    return ((g + 1.0) * x.float() + bb).to(x.dtype)


def add_layernorm(
    a: torch.Tensor,
    residual: Optional[torch.Tensor],
    ln_w: torch.Tensor,
    ln_b: torch.Tensor,
    *,
    pre_drop: float = 0.0,
    post_drop: float = 0.0,
    training: bool = False,
    film_params: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]] = None,
    lengths: Optional[torch.Tensor] = None,
    eps: float = 1e-5,
) -> torch.Tensor:
    """out = rowmask( FiLM( post_drop( LN( pre_drop(a) + residual ) ) ) ).

    Covers: MHA tail (``SubLayers.py:54-55`` + ``Layers.py:27-28``), FFN tail +
    FiLM + mask (``SubLayers.py:89-91``, ``Layers.py:31-35``), variance-predictor
    ReLU->LN->Dropout (``model/modules.py:216-245``) and the ref-encoder conv stack.
    """
    h = F.dropout(a, pre_drop, training) if pre_drop > 0 else a
    if residual is not None:
        h = h + residual
    y = F.layer_norm(h.float(), (h.shape[-1],), ln_w.float(), ln_b.float(), eps)
    if post_drop > 0:
        y = F.dropout(y, post_drop, training)
    if film_params is not None:
        g, b, sg, sb = film_params
        y = (sg * g.float()).unsqueeze(1).add(1.0) * y + (sb * b.float()).unsqueeze(1)
    y = y.to(a.dtype)
    if lengths is not None:
        y = y.masked_fill(lengths_to_mask(lengths, y.shape[1]).unsqueeze(-1), 0.0)
    return y


def length_regulate(x: torch.Tensor, durations: torch.Tensor, max_len: Optional[int]):
    """Expand phoneme i of item b ``durations[b, i]`` times and pad to ``max_len``.

    Equivalent to the reference's per-phoneme ``.item()`` loop
    (``model/modules.py:168-201``) but sync-free when ``max_len`` is given.
    Returns (out [B, M, C], mel_len [B] int64).
    """
    d = durations.long().clamp(min=0)
    mel_len = d.sum(1)
    B, T, C = x.shape
    if max_len is None:
        max_len = int(mel_len.max().item()) if B > 0 else 0
    cum = torch.cumsum(d, dim=1)  # [B, T]
    frames = torch.arange(max_len, device=x.device).unsqueeze(0).expand(B, -1)
    idx = torch.searchsorted(cum, frames.contiguous(), right=True)  # phoneme index per frame
    valid = frames < mel_len.unsqueeze(1)
    idx = idx.clamp(max=max(T - 1, 0))
    out = torch.gather(x, 1, idx.unsqueeze(-1).expand(-1, -1, C))
    out = out.masked_fill(~valid.unsqueeze(-1), 0.0)
    return out, mel_len


def bucketize_embed(values, bins, table):
    """torch.bucketize(values, bins) -> embedding rows (``model/modules.py:83-101``)."""
    return F.embedding(torch.bucketize(values.float(), bins.float()), table)


def masked_mean_mse(pred, target, mask_valid):
    diff = (pred.float() - target.float()) * mask_valid
    n = mask_valid.sum().clamp(min=1)
    return (diff * diff).sum() / n


def fastspeech2_loss_terms(
    mel_pred, postnet_pred, mel_target, mel_valid, p_pred, p_target, p_valid,
    e_pred, e_target, e_valid, logd_pred, d_target, src_valid,
):
    """The five masked terms of ``model/loss.py:43-82`` without ``masked_select``
    compaction: L1(mel), L1(postnet), MSE(pitch), MSE(energy), MSE(log(d+1))."""
    mv = mel_valid.unsqueeze(-1).float()
    nmel = (mv.sum() * mel_target.shape[-1]).clamp(min=1)
    mel_l = ((mel_pred.float() - mel_target.float()).abs() * mv).sum() / nmel
    post_l = ((postnet_pred.float() - mel_target.float()).abs() * mv).sum() / nmel
    pitch_l = masked_mean_mse(p_pred, p_target, p_valid.float())
    energy_l = masked_mean_mse(e_pred, e_target, e_valid.float())
    logd_t = torch.log(d_target.float() + 1.0)
    dur_l = masked_mean_mse(logd_pred, logd_t, src_valid.float())
    return mel_l, post_l, pitch_l, energy_l, dur_l


# ------------------------------------------------------------------ iSTFT / Griffin-Lim (audio/stft.py semantics)
def gl_min_frames(n_fft: int, hop: int) -> int:
    """Fewest frames at which reflect padding is defined (hop * (T - 1) > n_fft / 2); csrc/gl_frames.h."""
    return n_fft // (2 * hop) + 2


def gl_rows(x, lengths=None):
    """Frame rows of a batch -> (packed rows [R, C], host frame counts).  ``x``: padded ``[B, T, C]`` (``lengths``
    optional, clipped to T), packed ``[R, C]`` rows with ``lengths``, or one utterance ``[T, C]`` without."""
    if x.dim() == 2:
        lens = [x.shape[0]] if lengths is None else [max(0, int(v)) for v in lengths]
        assert sum(lens) == x.shape[0], "packed rows vs lengths"
        return x, lens
    assert x.dim() == 3, "frame rows: [B, T, C] or [R, C]"
    B, T, _ = x.shape
    lens = [T] * B if lengths is None else [max(0, min(int(v), T)) for v in lengths]
    if all(n == T for n in lens):
        return x.reshape(B * T, x.shape[2]), lens
    return torch.cat([x[b, :n] for b, n in enumerate(lens)], 0), lens


def _hash_u32(x):
    """csrc/common.h hash_u32 on int64 tensors holding uint32 values."""
    m = 0xFFFFFFFF
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & m
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & m
    return x ^ (x >> 16)


def gl_seed_phase(seed: int, T: int, NB: int, device=None, dtype=torch.float32):
    """The kernels' seeded initial phase of one utterance: 2 pi * hash(seed, local frame, bin) / 2^32 -> [T, NB]."""
    f = torch.arange(T, dtype=torch.int64, device=device).unsqueeze(1)
    k = torch.arange(NB, dtype=torch.int64, device=device).unsqueeze(0)
    h = _hash_u32(_hash_u32((int(seed) & 0xFFFFFFFF) ^ ((f * 0x9E3779B9) & 0xFFFFFFFF)) ^ k)
    return (h.to(torch.float32) * (2.0 / 4294967296.0)).to(dtype) * math.pi


def _istft_one(spec, n_fft, hop, window):
    """spec [T, NB] complex -> hop * (T - 1) samples (torch.istft, centred)."""
    if spec.shape[0] <= 1:
        return torch.zeros(0, dtype=window.dtype, device=spec.device)
    return torch.istft(spec.transpose(0, 1).unsqueeze(0), n_fft, hop, n_fft, window=window, center=True)[0]


def _wav_batch(wavs, width, int16_scale, dtype, device):
    W = int(width) if width is not None else max([w.shape[0] for w in wavs] + [0])
    out = torch.zeros(len(wavs), W, dtype=dtype, device=device)
    for b, w in enumerate(wavs):
        n = min(W, w.shape[0])
        out[b, :n] = w[:n]
    if int16_scale is not None:
        out = (out * int16_scale).clamp(-32768, 32767).to(torch.int16)
    return out


def istft(spec, n_fft, hop, window, lengths=None, width=None):
    """Complex spectrum rows (``gl_rows`` layouts, C = n_fft/2 + 1) -> wav [B, W]: utterance b's hop * (T_b - 1)
    samples, zeros after (W = ``width`` or the longest).  ``window``: the [n_fft] analysis window."""
    rows, lens = gl_rows(spec, lengths)
    window = window.to(rows.real.dtype)
    wavs, o = [], 0
    for n in lens:
        wavs.append(_istft_one(rows[o:o + n], n_fft, hop, window))
        o += n
    return _wav_batch(wavs, width, None, window.dtype, rows.device)


def griffin_lim(x, n_fft, hop, window, n_iters, momentum=0.99, init_phase=None, seed=0, lengths=None,
                int16_scale=None, mel_pinv=None, width=None, return_mag=False):
    """Griffin-Lim on magnitude rows, or log-mel rows when ``mel_pinv`` [n_fft/2+1, n_mel] is given
    (mag = clamp(pinv @ exp(mel), 0)); row layouts as ``gl_rows``.  Every utterance on its own:
    S = mag * exp(i phase) -> y = istft(S); per iteration c = stft(y), t = c + momentum * (c - c_prev)
    (t = c on the first), S = mag * t / |t| (mag where t = 0), y = istft(S).  ``momentum = 0`` is the classic
    algorithm, 0.99 the fast variant.  Utterances below ``gl_min_frames`` get no iteration.  ``init_phase``:
    radians in x's layout, else ``gl_seed_phase(seed)``.  Computes in x's dtype (float64 = the oracle).
    -> wav [B, W] (int16 = (wav * int16_scale).clamp.to(int16)); with ``return_mag`` also the packed mag rows."""
    rows, lens = gl_rows(x, lengths)
    window = window.to(rows.dtype)
    mag = torch.clamp(torch.exp(rows) @ mel_pinv.to(rows.dtype).t(), min=0.0) if mel_pinv is not None else rows
    NB = n_fft // 2 + 1
    assert mag.shape[1] == NB, "griffin_lim: rows are not [*, n_fft/2+1] magnitudes (mel_pinv missing?)"
    ph_rows = None if init_phase is None else gl_rows(init_phase, lengths)[0].to(rows.dtype)
    wavs, o = [], 0
    for n in lens:
        m = mag[o:o + n]
        ph = ph_rows[o:o + n] if ph_rows is not None else gl_seed_phase(seed, n, NB, rows.device, rows.dtype)
        o += n
        y = _istft_one(torch.polar(m, ph), n_fft, hop, window)
        prev = None
        for _ in range(n_iters if n >= gl_min_frames(n_fft, hop) else 0):
            c = torch.stft(y.unsqueeze(0), n_fft, hop, n_fft, window=window, center=True, pad_mode="reflect",
                           return_complex=True)[0].transpose(0, 1)
            t = c if (prev is None or momentum == 0) else c + momentum * (c - prev)
            prev = c
            a = t.abs()
            s = torch.where(a > 0, m * (t / torch.where(a > 0, a, torch.ones_like(a))), m.to(t.dtype))
            y = _istft_one(s, n_fft, hop, window)
        wavs.append(y)
    out = _wav_batch(wavs, width, int16_scale, rows.dtype, rows.device)
    return (out, mag) if return_mag else out


# ------------------------------------------------------------------ dynamic time warping (csrc/k_dtw.hip semantics)
def dtw_lens(x, y, x_lens, y_lens):
    """Host row counts of a packed DTW batch, validated: x [Rx, D] / y [Ry, D] with one (x_len, y_len) per pair.
    A pair without rows on either side has no warping path: ``ValueError`` before anything runs."""
    xl = [int(v) for v in (x_lens.tolist() if isinstance(x_lens, torch.Tensor) else x_lens)]
    yl = [int(v) for v in (y_lens.tolist() if isinstance(y_lens, torch.Tensor) else y_lens)]
    if x.dim() != 2 or y.dim() != 2 or x.shape[1] != y.shape[1]:
        raise ValueError(f"dtw: x / y must be packed rows [R, D] of one D, got {tuple(x.shape)} / {tuple(y.shape)}")
    if len(xl) != len(yl):
        raise ValueError(f"dtw: {len(xl)} x lengths but {len(yl)} y lengths")
    for p, (a, b) in enumerate(zip(xl, yl)):
        if a < 1 or b < 1:
            raise ValueError(f"dtw: pair {p} has lengths ({a}, {b}); every pair needs at least one row on each side")
    if sum(xl) != x.shape[0] or sum(yl) != y.shape[0]:
        raise ValueError(f"dtw: lengths sum to ({sum(xl)}, {sum(yl)}) but x / y have ({x.shape[0]}, {y.shape[0]}) rows")
    return xl, yl


def _dtw_one(x, y):
    """One pair: (A(Tx-1, Ty-1) as a 0-d tensor, directions [Tx, Ty] uint8) by a wavefront over the anti-diagonals
    (one batch of elementwise ops per diagonal)."""
    Tx, Ty, W = x.shape[0], y.shape[0], y.shape[0] + 1
    c = torch.zeros(Tx, Ty, dtype=x.dtype, device=x.device)
    for d in range(x.shape[1]):  # from the differences, d in index order
        df = x[:, d].unsqueeze(1) - y[:, d].unsqueeze(0)
        c = c + df * df
    c = torch.sqrt(c).reshape(-1)
    A = torch.full(((Tx + 1) * W,), float("inf"), dtype=x.dtype, device=x.device)  # cell (i, j) at (i+1) W + j + 1
    A[0] = 0.0  # the diagonal predecessor of (0, 0)
    dirs = torch.zeros(Tx * Ty, dtype=torch.uint8, device=x.device)
    two = torch.full((), 2, dtype=torch.uint8, device=x.device)
    for k in range(Tx + Ty - 1):
        lo, hi = max(0, k - Ty + 1), min(k, Tx - 1)
        n = hi - lo + 1
        at = (lo + 1) * W + (k - lo) + 1  # cells of diagonal k: stride W - 1 in A, Ty - 1 in c / dirs
        diag = torch.as_strided(A, (n,), (W - 1,), at - W - 1)
        up = torch.as_strided(A, (n,), (W - 1,), at - W)
        left = torch.as_strided(A, (n,), (W - 1,), at - 1)
        # tie rule: diagonal, then (i-1, j), then (i, j-1); a later candidate wins only on strict <
        m1 = up < diag
        best = torch.where(m1, up, diag)
        m2 = left < best
        best = torch.where(m2, left, best)
        ck = torch.as_strided(c, (n,), (Ty - 1,), lo * Ty + k - lo)
        torch.as_strided(A, (n,), (W - 1,), at).copy_(ck + best)
        torch.as_strided(dirs, (n,), (Ty - 1,), lo * Ty + k - lo).copy_(torch.where(m2, two, m1.to(torch.uint8)))
    return A[-1], dirs.view(Tx, Ty)


def dtw(x, y, x_lens, y_lens):
    """Dynamic time warping of P packed pairs: x [Rx, D] / y [Ry, D] rows, ``x_lens`` / ``y_lens`` the P row counts
    (host sequences).  Local cost c(i, j) = sqrt(sum_d (x[i, d] - y[j, d])^2) from the differences; A(i, j) =
    c(i, j) + min(A(i-1, j-1), A(i-1, j), A(i, j-1)) with ties to the diagonal, then (i-1, j), then (i, j-1).
    Computes in x's dtype (float64 = the oracle) on x's device.
    -> cost [P] = A(Tx-1, Ty-1), path [P, Lmax, 2] int32 ((i, j) cells in increasing order, -1 past the length,
    Lmax = max Tx + max Ty - 1), path_len [P] int32."""
    import numpy as np

    xl, yl = dtw_lens(x, y, x_lens, y_lens)
    P = len(xl)
    Lmax = (max(xl) + max(yl) - 1) if P else 0
    path = np.full((P, Lmax, 2), -1, dtype=np.int32)
    plen = np.zeros(P, dtype=np.int32)
    costs, ox, oy = [], 0, 0
    for p, (tx, ty) in enumerate(zip(xl, yl)):
        total, dirs = _dtw_one(x[ox:ox + tx], y[oy:oy + ty].to(x.dtype))
        ox, oy = ox + tx, oy + ty
        costs.append(total)
        dr = dirs.cpu().numpy()
        i, j, cells = tx - 1, ty - 1, []
        while True:
            cells.append((i, j))
            if i == 0 and j == 0:
                break
            d = dr[i, j]
            i, j = (i - 1 if d != 2 else i), (j - 1 if d != 1 else j)
        plen[p] = len(cells)
        path[p, :len(cells)] = np.asarray(cells[::-1], dtype=np.int32)
    cost = torch.stack(costs) if P else torch.zeros(0, dtype=x.dtype, device=x.device)
    return cost, torch.from_numpy(path).to(x.device), torch.from_numpy(plen).to(x.device)


# ------------------------------------------------- alignment learning (csrc/k_align.hip semantics)
ALIGN_MAX_N = 1024  # tokens per utterance the kernels cover (16 waves of 64 lanes)


def _host_lens(v):
    if isinstance(v, torch.Tensor):
        h = getattr(v, "host_lengths", None)
        v = h if h is not None else v.tolist()
    return [int(x) for x in v]


def align_lens(lp, t_lens, n_lens, what="align"):
    """Host lengths of a padded alignment batch, validated: lp [B, Tmax, Nmax] with T_b mel frames and N_b tokens per
    utterance (host sequences, or tensors -- a tensor with a ``host_lengths`` attribute is not read back).  A
    monotone alignment that visits every token needs 1 <= N_b <= T_b: ``ValueError`` before anything runs."""
    if lp.dim() != 3:
        raise ValueError(f"{what}: lp must be [B, Tmax, Nmax], got {tuple(lp.shape)}")
    tl, nl = _host_lens(t_lens), _host_lens(n_lens)
    B, Tmax, Nmax = lp.shape
    if len(tl) != B or len(nl) != B:
        raise ValueError(f"{what}: {len(tl)} frame lengths / {len(nl)} token lengths for a batch of {B}")
    if Nmax > ALIGN_MAX_N:
        raise ValueError(f"{what}: Nmax = {Nmax} exceeds {ALIGN_MAX_N} tokens")
    for b, (t, n) in enumerate(zip(tl, nl)):
        if not 1 <= n <= t or t > Tmax or n > Nmax:
            raise ValueError(f"{what}: utterance {b} has (T, N) = ({t}, {n}) in a [{Tmax}, {Nmax}] lattice; "
                             "every utterance needs 1 <= N <= T")
    return tl, nl


def _lens_on(v, host, device):
    if isinstance(v, torch.Tensor) and v.device == device:
        return v.to(torch.long)
    return torch.tensor(host, dtype=torch.long, device=device)


def _logaddexp(a, b):
    """max + log1p(exp(-|d|)), -inf where both are -inf (torch.logaddexp's gradient is NaN there; the value is not)."""
    m = torch.maximum(a, b)
    r = m + torch.log1p(torch.exp(-(a - b).abs()))
    return torch.where(m == float("-inf"), m, r)


def _shift_tokens(x, fill, back=False):
    """x[..., n - 1] at n (``back``: x[..., n + 1]), ``fill`` at the open end."""
    pad = torch.full_like(x[..., :1], fill)
    return torch.cat([x[..., 1:], pad], -1) if back else torch.cat([pad, x[..., :-1]], -1)


def _align_alpha(lp, tl, nl, hard):
    """alpha [B, Tmax, Nmax] of the lattice (max in place of logaddexp when ``hard``; then also the advance plane
    [B, Tmax, Nmax] bool: advance only on strict >).  Cells n >= N_b are -inf; rows t >= T_b are not meaningful."""
    B, Tmax, Nmax = lp.shape
    ninf = float("-inf")
    n_idx = torch.arange(Nmax, device=lp.device)
    lpm = lp.masked_fill((n_idx.unsqueeze(0) >= nl.unsqueeze(1)).unsqueeze(1), ninf)
    first = torch.full((B, Nmax), ninf, dtype=lp.dtype, device=lp.device)
    first[:, 0] = 0.0
    rows, adv = [lpm[:, 0] + first], [torch.zeros(B, Nmax, dtype=torch.bool, device=lp.device)]
    for t in range(1, Tmax):
        stay = rows[-1]
        move = _shift_tokens(stay, ninf)
        if hard:
            go = move > stay
            adv.append(go)
            rows.append(lpm[:, t] + torch.where(go, move, stay))
        else:
            rows.append(lpm[:, t] + _logaddexp(stay, move))
    return torch.stack(rows, 1), (torch.stack(adv, 1) if hard else None)


class _AlignForwardSum(torch.autograd.Function):
    """The closed-form gradient (the path posterior): autograd through logaddexp is NaN at the -inf cells."""

    @staticmethod
    def forward(ctx, lp, tl, nl):
        B = lp.shape[0]
        alpha, _ = _align_alpha(lp, tl, nl, hard=False)
        end = alpha[torch.arange(B, device=lp.device), tl - 1, nl - 1]
        ctx.save_for_backward(lp, alpha, end, tl, nl)
        return -end

    @staticmethod
    def backward(ctx, g):
        lp, alpha, end, tl, nl = ctx.saved_tensors
        B, Tmax, Nmax = lp.shape
        ninf = float("-inf")
        n_idx = torch.arange(Nmax, device=lp.device).unsqueeze(0)
        lpm = lp.masked_fill((n_idx >= nl.unsqueeze(1)).unsqueeze(1), ninf)
        last = torch.where(n_idx == (nl - 1).unsqueeze(1), 0.0, ninf).to(lp.dtype)  # beta(T_b - 1, .)
        none = torch.full_like(last, ninf)
        rows = [None] * Tmax
        nxt = none  # lp + beta of frame t + 1
        for t in range(Tmax - 1, -1, -1):
            beta = _logaddexp(nxt, _shift_tokens(nxt, ninf, back=True))
            at = (tl - 1).unsqueeze(1)
            beta = torch.where(at == t, last, torch.where(at < t, none, beta))
            rows[t] = beta
            nxt = lpm[:, t] + beta
        beta = torch.stack(rows, 1)
        x = alpha + beta - end.view(B, 1, 1)
        t_idx = torch.arange(Tmax, device=lp.device).view(1, Tmax, 1)
        inside = (t_idx < tl.view(B, 1, 1)) & (n_idx.unsqueeze(1) < nl.view(B, 1, 1)) & (x > ninf)
        post = torch.where(inside, torch.exp(torch.where(inside, x, torch.zeros_like(x))), torch.zeros_like(x))
        return -post * g.to(lp.dtype).view(B, 1, 1), None, None


def align_forward_sum(lp, t_lens, n_lens):
    """Negative total log-probability of all monotone alignments of T_b frames to N_b tokens: paths start at token 0,
    end at token N_b - 1 and at each frame stay or advance by one.  This is the CTC forward-sum without blanks.

        alpha(0, 0) = lp(0, 0), alpha(0, n > 0) = -inf
        alpha(t, n) = lp(t, n) + logaddexp(alpha(t-1, n), alpha(t-1, n-1)),     nll_b = -alpha(T_b - 1, N_b - 1)

    lp [B, Tmax, Nmax] (only cells t < T_b, n < N_b are read) -> nll [B] in lp's dtype (float64 = the oracle),
    differentiable in lp: the gradient is minus the path posterior exp(alpha + beta - alpha_end), exactly 0 on
    unreachable cells and on padding."""
    tl, nl = align_lens(lp, t_lens, n_lens, "align_forward_sum")
    return _AlignForwardSum.apply(lp, _lens_on(t_lens, tl, lp.device), _lens_on(n_lens, nl, lp.device))


@torch.no_grad()
def align_mas(lp, t_lens, n_lens):
    """Monotonic alignment search: the best path of the ``align_forward_sum`` lattice (max in place of logaddexp;
    on a tie stay wins, advance only on strict >), walked back from (T_b - 1, N_b - 1).
    -> durations [B, Nmax] int32: frames on each token, >= 1 for n < N_b, 0 beyond, summing to T_b."""
    import numpy as np

    tl, nl = align_lens(lp, t_lens, n_lens, "align_mas")
    B, Tmax, Nmax = lp.shape
    _, adv = _align_alpha(lp.detach(), _lens_on(t_lens, tl, lp.device), _lens_on(n_lens, nl, lp.device), hard=True)
    adv = adv.cpu().numpy()
    dur = np.zeros((B, Nmax), dtype=np.int32)
    for b in range(B):
        n = nl[b] - 1
        for t in range(tl[b] - 1, -1, -1):
            dur[b, n] += 1
            if t > 0 and adv[b, t, n]:
                n -= 1
    return torch.from_numpy(dur).to(lp.device)


def segment_mean(values, durations):
    """Mean of each token's run of frames: values [B, Tmax], durations [B, Nmax] (token n of utterance b owns the
    frames sum(d[:n]) .. sum(d[:n + 1]) - 1) -> [B, Nmax] fp32, 0 for a zero duration
    (``data/preprocess.py::phoneme_average`` on the device; frames added in order)."""
    B, Tmax = values.shape
    Nmax = durations.shape[1]
    d = durations.to(torch.long).clamp(min=0)
    ends = torch.cumsum(d, 1)
    t_idx = torch.arange(Tmax, device=values.device).unsqueeze(0).expand(B, Tmax).contiguous()
    tok = torch.searchsorted(ends, t_idx, right=True)  # frames past the last run fall into slot Nmax
    sums = torch.zeros(B, Nmax + 1, dtype=torch.float32, device=values.device)
    sums.scatter_add_(1, tok, values.float())
    return torch.where(d > 0, sums[:, :Nmax] / d.clamp(min=1).float(), torch.zeros_like(sums[:, :Nmax]))


# ------------------------------------------------------------------ YIN pitch tracker (csrc/k_pitch.hip semantics)
def yin_plan(wav, lengths, sr, hop, frame=1024, fmin=71.0, fmax=800.0):
    """Host side of a packed YIN batch, validated: -> (sample counts, frame counts 1 + N // hop, tau_min, tau_max).
    ``ValueError`` with the offending value for a frame size the kernel does not cover, a hop outside 1 .. frame,
    an utterance too short for the reflect padding (N <= frame / 2) or lengths that do not add up."""
    frame, hop = int(frame), int(hop)
    if frame not in (512, 1024, 2048):
        raise ValueError(f"yin: frame {frame} not covered (512, 1024 or 2048)")
    if not 0 < hop <= frame:
        raise ValueError(f"yin: hop {hop} must lie in 1 .. frame = {frame}")
    lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if wav.dim() != 1:
        raise ValueError(f"yin: wav must be one packed vector of samples, got shape {tuple(wav.shape)}")
    for b, n in enumerate(lens):
        if n <= frame // 2:
            raise ValueError(f"yin: utterance {b} has {n} samples; reflect padding needs more than frame / 2 = "
                             f"{frame // 2}")
        if n + frame >= 2 ** 31:
            raise ValueError(f"yin: utterance {b} has {n} samples; positions inside an utterance are 32-bit")
    if sum(lens) != wav.shape[0]:
        raise ValueError(f"yin: lengths sum to {sum(lens)} but wav has {wav.shape[0]} samples")
    tau_min = max(2, int(sr / fmax))
    tau_max = min(frame // 2, int(sr / fmin) + 1)
    if tau_min >= tau_max:
        raise ValueError(f"yin: no lag between fmax {fmax} and fmin {fmin} at sr {sr} (tau {tau_min} .. {tau_max})")
    return lens, [1 + n // hop for n in lens], tau_min, tau_max


def _yin_one(x, sr, hop, frame, tau_min, tau_max, threshold):
    """One utterance: (f0 [T], cmnd [T, tau_max + 1]) in x's dtype."""
    W = frame // 2
    pad = torch.nn.functional.pad(x.view(1, 1, -1), (W, W), mode="reflect").view(-1)
    fr = pad.unfold(0, frame, hop)  # [T, frame], T = 1 + N // hop
    fr = fr - fr.mean(1, keepdim=True)
    head = fr[:, :W]
    T = fr.shape[0]
    d = torch.empty(T, tau_max, dtype=x.dtype, device=x.device)  # column tau - 1
    shifted = fr.unfold(1, W, 1)  # [T, W + 1, W] view: row tau = fr[:, tau : tau + W]
    step = max(1, (1 << 24) // max(1, T * W))  # lags per batch of elementwise ops
    for a in range(1, tau_max + 1, step):
        b = min(tau_max + 1, a + step)
        df = head.unsqueeze(1) - shifted[:, a:b]
        d[:, a - 1:b - 1] = (df * df).sum(-1)
    taus = torch.arange(1, tau_max + 1, dtype=x.dtype, device=x.device)
    run = torch.cumsum(d, 1)
    live = run > 0
    cm = torch.where(live, d * taus / torch.where(live, run, torch.ones_like(run)), torch.ones_like(d))
    cm = torch.cat([torch.ones(T, 1, dtype=x.dtype, device=x.device), cm], 1)  # [T, tau_max + 1], cmnd(0) = 1
    idx = torch.arange(tau_max, device=x.device).unsqueeze(0)  # lags 0 .. tau_max - 1
    below = (cm[:, :tau_max] < threshold) & (idx >= tau_min)
    has = below.any(1)
    first = torch.argmax(below.to(torch.uint8), 1, keepdim=True)
    # walk down: the first lag t >= first at which t + 1 == tau_max or cmnd(t + 1) >= cmnd(t)
    stop = ~(cm[:, 1:] < cm[:, :-1])
    stop[:, -1] = True
    t = torch.argmax((stop & (idx >= first)).to(torch.uint8), 1, keepdim=True)
    t = torch.where(has.unsqueeze(1), t, torch.full_like(t, tau_min))  # any valid lag: the frame is zeroed below
    # tau_min >= 2 and t < tau_max <= W: cmnd(t - 1) and cmnd(t + 1) always exist, so every lag is interpolated
    a, b, c = cm.gather(1, t - 1), cm.gather(1, t), cm.gather(1, t + 1)
    den = a - 2 * b + c
    ok = den.abs() > 1e-12
    lag = t.to(x.dtype) + torch.where(ok, 0.5 * (a - c) / torch.where(ok, den, torch.ones_like(den)),
                                      torch.zeros_like(den))
    f0 = (float(sr) / lag).squeeze(1)
    voiced = has & (torch.sqrt((head * head).sum(1) / W) > 1e-4)
    return torch.where(voiced, f0, torch.zeros_like(f0)), cm


def yin(wav, lengths, sr, hop, frame=1024, fmin=71.0, fmax=800.0, threshold=0.15, return_cmnd=False):
    """YIN fundamental frequency of packed utterances: ``wav`` one vector of all samples back to back, ``lengths``
    the host sample counts.  Semantics of ``data.preprocess.yin_f0`` (centre reflect padding by frame / 2, 1 + N //
    hop frames, frame mean removed, W = frame / 2) with the difference function accumulated from the squared
    differences, d(tau) = sum_{j<W} (x[j] - x[j + tau])^2 (no cancellation: fp32 is enough), and cmnd(tau) = 1 where
    the running sum of d is 0 (a frame that begins in digital silence has no pitch; ``yin_f0`` answers with rounding
    noise there).  Lag: the first tau in [tau_min, tau_max) with cmnd < threshold, walked on while cmnd falls,
    parabolic interpolation; a frame without a crossing or with rms(x[:W]) <= 1e-4 is unvoiced (0).
    Computes in wav's dtype (float64 = the oracle) on wav's device.
    -> f0 [R] over the packed frame rows (R = sum of 1 + N_b // hop), the per-utterance frame counts (host list) and,
    with ``return_cmnd``, the plane [R, tau_max + 1]."""
    lens, frames, tau_min, tau_max = yin_plan(wav, lengths, sr, hop, frame, fmin, fmax)
    f0s, cms, at = [], [], 0
    for n in lens:
        f0, cm = _yin_one(wav[at:at + n], sr, int(hop), int(frame), tau_min, tau_max, threshold)
        at += n
        f0s.append(f0)
        cms.append(cm)
    f0 = torch.cat(f0s) if f0s else wav.new_zeros(0)
    if return_cmnd:
        return f0, frames, (torch.cat(cms) if cms else wav.new_zeros(0, tau_max + 1))
    return f0, frames


# --------------------------------------------------------- probabilistic YIN (csrc/k_pyin.hip semantics)
PYIN_MAX_HALF = 63    # the kernel keeps a band offset 0 .. 2 h and a switch bit in one byte
PYIN_MAX_BINS = 1024  # ... and four bins per lane of a 256-thread workgroup
PYIN_LOG_FLOOR = 1e-30


def pyin_bins(sr, hop, fmin=71.0, fmax=800.0, bins_per_semitone=20, max_transition_rate=35.92):
    """Pitch grid of the pYIN decoder -> (NB bins of 1 / bins_per_semitone semitones from fmin up to fmax, band
    half-width h in bins a track may move per frame).  ``ValueError`` with the value when h > 63 or NB > 1024."""
    bps = int(bins_per_semitone)
    if bps < 1 or not 0 < fmin < fmax:
        raise ValueError(f"pyin: bins_per_semitone {bins_per_semitone} / fmin {fmin} / fmax {fmax} give no pitch grid")
    NB = int(math.floor(12 * bps * math.log2(fmax / fmin))) + 1
    st = max(1, int(round(max_transition_rate * 12 * int(hop) / sr)))
    h = st * bps // 2
    if NB > PYIN_MAX_BINS:
        raise ValueError(f"pyin: {bps} bins per semitone between {fmin} and {fmax} Hz are NB = {NB} bins; the decoder "
                         f"covers NB <= {PYIN_MAX_BINS}")
    if h > PYIN_MAX_HALF:
        raise ValueError(f"pyin: hop {hop} at sr {sr} lets a track move h = {h} bins per frame; the decoder covers "
                         f"h <= {PYIN_MAX_HALF}")
    return NB, h


def pyin_plan(wav, lengths, sr, hop, frame=1024, fmin=71.0, fmax=800.0, bins_per_semitone=20,
              max_transition_rate=35.92):
    """Host side of a packed pYIN batch, validated: ``yin_plan``'s (sample counts, frame counts, tau_min, tau_max)
    followed by ``pyin_bins``' (NB, h)."""
    plan = yin_plan(wav, lengths, sr, hop, frame, fmin, fmax)
    return plan + pyin_bins(sr, hop, fmin, fmax, bins_per_semitone, max_transition_rate)


def _beta_2_18_tail(x):
    """1 - F(x) of Beta(2, 18), the prior of the YIN threshold: (1 - x)^18 (1 + 18 x), x clamped to [0, 1].  The
    weights below are differences of F; taken between the tails they keep their relative precision where F is
    within rounding of 1 (a trough at cmnd 0.8 weighs 4e-12: float32 holds that as a tail, not as 1 - F)."""
    x = x.clamp(0.0, 1.0)
    y = 1.0 - x
    y2 = y * y
    y4 = y2 * y2
    y8 = y4 * y4
    return (y8 * y8 * y2) * (1.0 + 18.0 * x)


def pyin_obs(cm, sr, tau_min, tau_max, fmin=71.0, fmax=800.0, bins_per_semitone=20, no_trough_prob=0.01):
    """Stage 1 of pYIN, every frame row alone: the cmnd plane ``cm`` [R, tau_max + 1] of ``yin`` -> (obs [R, NB]
    probability of every pitch bin, voiced_prob [R]) in cm's dtype.

    Troughs are the lags t in [tau_min, tau_max - 1] with cm[t] < cm[t - 1] and cm[t] <= cm[t + 1].  With the YIN
    threshold distributed as Beta(2, 18) (CDF F), a trough below every earlier trough (m = the smallest cmnd of the
    earlier ones, 2 at the start) is YIN's pick for the thresholds in (cm[t], m] and weighs F(m) - F(cm[t]); the
    lowest trough (the first of equals) also takes no_trough_prob * F(cm[t]), the thresholds no trough is below.
    Every weighted trough is interpolated as in ``yin`` and lands in bin round(12 bps log2(sr / lag / fmin)),
    clamped to the grid; weights of one bin are added in increasing lag order; voiced_prob is their clamped sum."""
    bps = int(bins_per_semitone)
    NB = int(math.floor(12 * bps * math.log2(fmax / fmin))) + 1
    R = cm.shape[0]
    dt, dev = cm.dtype, cm.device
    obs = torch.zeros(R, NB, dtype=dt, device=dev)
    vp = torch.zeros(R, dtype=dt, device=dev)
    if R == 0:
        return obs, vp
    a, b, c = cm[:, tau_min - 1:tau_max - 1], cm[:, tau_min:tau_max], cm[:, tau_min + 1:tau_max + 1]
    trough = (b < a) & (b <= c)
    two = torch.full_like(b, 2.0)
    low = torch.cummin(torch.where(trough, b, two), 1).values
    m = torch.cat([two[:, :1], low[:, :-1]], 1)  # the smallest cmnd of the earlier troughs
    rec = trough & (b < m)
    K = int(rec.sum(1).max())
    if K == 0:
        return obs, vp
    Sb = _beta_2_18_tail(b)
    w = Sb - _beta_2_18_tail(m)  # F(m) - F(cm[t])
    lags = torch.arange(tau_min, tau_max, device=dev)
    last = torch.where(rec, lags, torch.zeros_like(lags)).argmax(1, keepdim=True)  # the lowest trough
    w = w.scatter_add(1, last, no_trough_prob * (1.0 - Sb.gather(1, last)))
    den = a - 2 * b + c
    ok = den.abs() > 1e-12
    lag = lags.to(dt) + torch.where(ok, 0.5 * (a - c) / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))
    bins = torch.round(12 * bps * torch.log2(float(sr) / lag / float(fmin))).clamp(0, NB - 1)
    bins = torch.where(rec, bins, torch.zeros_like(bins)).to(torch.long)  # elsewhere the parabola means nothing
    # the record troughs of every row, compacted in lag order: one add per row and step keeps the order on any device
    order = torch.where(rec, lags, torch.full_like(lags, tau_max)).sort(1).values[:, :K]
    live = order < tau_max
    col = (order - tau_min).clamp(max=tau_max - tau_min - 1)
    wk = torch.where(live, w.gather(1, col), torch.zeros_like(vp).unsqueeze(1))
    bk = bins.gather(1, col)
    for k in range(K):
        obs.scatter_add_(1, bk[:, k:k + 1], wk[:, k:k + 1])
        vp = vp + wk[:, k]
    return obs, vp.clamp(0.0, 1.0)


def pyin_decode(obs, voiced_prob, frames, sr, hop, fmin=71.0, bins_per_semitone=20, max_transition_rate=35.92,
                switch_prob=0.01):
    """Stage 2 of pYIN, every utterance alone: Viterbi over 2 NB states (voiced bin b, unvoiced bin b) of the planes
    of ``pyin_obs`` (packed rows, ``frames`` the host frame counts) -> f0 [R]: the centre fmin 2^(b / (12 bps)) of
    the decoded bin on voiced frames, 0 on unvoiced ones.

    Log observation log(max(obs, 1e-30)) for a voiced state, log(max((1 - voiced_prob) / NB, 1e-30)) for an unvoiced
    one; uniform start; a bin moves by d in [-h, h] with weight (h + 1 - |d|) / (h + 1)^2 (moves off the grid do not
    exist), keeping the voicing costs log(1 - switch_prob), switching log(switch_prob).  After every frame the
    maximum over all states is subtracted.  Ties: the lowest predecessor bin, then staying over switching; at the
    last frame voiced over unvoiced, then the lowest bin."""
    bps = int(bins_per_semitone)
    NB = obs.shape[1]
    frames = [int(v) for v in frames]
    if obs.dim() != 2 or voiced_prob.shape != obs.shape[:1] or sum(frames) != obs.shape[0]:
        raise ValueError(f"pyin_decode: obs {tuple(obs.shape)} / voiced_prob {tuple(voiced_prob.shape)} do not hold the "
                         f"{sum(frames)} frames of the utterances")
    st = max(1, int(round(max_transition_rate * 12 * int(hop) / sr)))
    h = st * bps // 2
    if h > PYIN_MAX_HALF or not 1 <= NB <= PYIN_MAX_BINS:
        raise ValueError(f"pyin_decode: h = {h} / NB = {NB} outside the decoder's h <= {PYIN_MAX_HALF}, NB <= "
                         f"{PYIN_MAX_BINS}")
    dt, dev = obs.dtype, obs.device
    d = torch.arange(-h, h + 1, dtype=dt, device=dev)
    ltri = torch.log((h + 1 - d.abs()) / float((h + 1) ** 2))
    stay = torch.tensor(math.log(1.0 - switch_prob), dtype=dt, device=dev)
    swap = torch.tensor(math.log(switch_prob), dtype=dt, device=dev)
    centres = float(fmin) * torch.exp2(torch.arange(NB, dtype=dt, device=dev) / (12 * bps))
    pad = torch.full((2, h), float("-inf"), dtype=dt, device=dev)
    out, at = [], 0
    for T in frames:
        if T == 0:
            continue
        lo = torch.stack([torch.log(obs[at:at + T].clamp(min=PYIN_LOG_FLOOR)),
                          torch.log(((1.0 - voiced_prob[at:at + T]) / NB).clamp(min=PYIN_LOG_FLOOR)).unsqueeze(1)
                          .expand(T, NB)], 1)  # [T, 2, NB]
        at += T
        delta = lo[0] - lo[0].max()
        back = torch.empty(T, 2, NB, dtype=torch.long, device=dev)  # predecessor: voicing * NB + bin
        base = torch.arange(NB, device=dev) - h
        for t in range(1, T):
            win = torch.cat([pad, delta, pad], 1).unfold(1, 2 * h + 1, 1) + ltri  # [2, NB, 2 h + 1]
            best, off = win.max(2)  # the first of equal maxima: the lowest bin
            keep, move = best + stay, best.flip(0) + swap
            sw = move > keep
            back[t] = torch.where(sw, 1 - torch.arange(2, device=dev).unsqueeze(1), torch.arange(2, device=dev).unsqueeze(1)) * NB \
                + base + torch.where(sw, off.flip(0), off)
            delta = torch.where(sw, move, keep) + lo[t]
            delta = delta - delta.max()
        state = int(delta.reshape(-1).argmax())  # the first of equal maxima: voiced, the lowest bin
        walk = back.reshape(T, 2 * NB).cpu().numpy()  # one copy: the walk itself runs on the host
        path = [state]
        for t in range(T - 1, 0, -1):
            state = int(walk[t, state])
            path.append(state)
        s = torch.tensor(path[::-1], device=dev)
        out.append(torch.where(s < NB, centres[s % NB], torch.zeros_like(centres[:1])))
    return torch.cat(out) if out else obs.new_zeros(0)


def pyin(wav, lengths, sr, hop, frame=1024, fmin=71.0, fmax=800.0, bins_per_semitone=20, max_transition_rate=35.92,
         switch_prob=0.01, no_trough_prob=0.01, return_obs=False):
    """Probabilistic YIN (Mauch & Dixon 2014) of packed utterances, layout and frame counts of ``yin``: the cmnd plane
    of ``yin`` -> ``pyin_obs`` (pitch candidates of every frame for all YIN thresholds at once, weighted by a Beta(2,
    18) prior in closed form) -> ``pyin_decode`` (one smooth track per utterance).  Computes in wav's dtype (float64 =
    the oracle) on wav's device.  -> f0 [R] (bin centres: quantised to 1 / bins_per_semitone semitones, 2.5 cents at
    the default; 0 = unvoiced), the per-utterance frame counts (host list), voiced_prob [R] and, with
    ``return_obs``, the plane [R, NB]."""
    _, frames, tau_min, tau_max, NB, h = pyin_plan(wav, lengths, sr, hop, frame, fmin, fmax, bins_per_semitone,
                                                   max_transition_rate)
    _, _, cm = yin(wav, lengths, sr, hop, frame, fmin, fmax, return_cmnd=True)
    obs, vp = pyin_obs(cm, sr, tau_min, tau_max, fmin, fmax, bins_per_semitone, no_trough_prob)
    f0 = pyin_decode(obs, vp, frames, sr, hop, fmin, bins_per_semitone, max_transition_rate, switch_prob)
    return (f0, frames, vp, obs) if return_obs else (f0, frames, vp)


# --------------------------------------------------------- prosody transfer (csrc/k_prosody.hip semantics)
PROSODY_MAX_N = 1024  # tokens per utterance the kernel covers (4 per thread of a 256-thread workgroup)
PROSODY_PITCH_MODES = ("relative", "absolute")


def prosody_lens(path, path_len, src_dur, src_lens, x_lens, y_lens, f0, energy, pred_pitch, pitch_stats, energy_stats,
                 pitch_mode):
    """Host side of a prosody-transfer batch, validated -> (x_lens, y_lens) as int lists.  ``ValueError`` with the
    offending value before anything runs."""
    if pitch_mode not in PROSODY_PITCH_MODES:
        raise ValueError(f"prosody_transfer: pitch_mode {pitch_mode!r} not supported ({', '.join(PROSODY_PITCH_MODES)})")
    if path.dim() != 3 or path.shape[2] != 2 or src_dur.dim() != 2 or pred_pitch.shape != src_dur.shape:
        raise ValueError(f"prosody_transfer: path [P, Lmax, 2] / src_dur, pred_pitch [P, Nmax], got {tuple(path.shape)} / "
                         f"{tuple(src_dur.shape)} / {tuple(pred_pitch.shape)}")
    xl, yl = _host_lens(x_lens), _host_lens(y_lens)
    P, Nmax = src_dur.shape
    if not (path.shape[0] == path_len.shape[0] == len(xl) == len(yl) == len(src_lens) == P):
        raise ValueError(f"prosody_transfer: {path.shape[0]} paths / {path_len.shape[0]} path lengths / {len(xl)} x "
                         f"lengths / {len(yl)} y lengths / {len(src_lens)} token counts for {P} utterances")
    if Nmax > PROSODY_MAX_N:
        raise ValueError(f"prosody_transfer: Nmax = {Nmax} exceeds {PROSODY_MAX_N} tokens")
    for p, (a, b) in enumerate(zip(xl, yl)):
        if a < 1 or b < 1:
            raise ValueError(f"prosody_transfer: utterance {p} has lengths ({a}, {b}); an alignment has at least one "
                             "frame on each side")
    if f0.dim() != 1 or f0.shape != energy.shape or sum(yl) != f0.shape[0]:
        raise ValueError(f"prosody_transfer: y lengths sum to {sum(yl)} but f0 / energy are {tuple(f0.shape)} / "
                         f"{tuple(energy.shape)}")
    for name, st in (("pitch", pitch_stats), ("energy", energy_stats)):
        if len(st) != 2 or not float(st[1]) > 0.0:
            raise ValueError(f"prosody_transfer: {name} statistics must be (mean, std > 0), got {tuple(st)}")
    return xl, yl


def _pad_frames(v, yl):
    """Packed frames [Ry] -> ([P, Ymax] zero-padded, valid [P, Ymax])."""
    P, Ymax, dev = len(yl), max(yl), v.device
    lens = torch.tensor(yl, dtype=torch.long, device=dev)
    starts = torch.cumsum(lens, 0) - lens
    j = torch.arange(Ymax, device=dev).unsqueeze(0)
    valid = j < lens.unsqueeze(1)
    rows = v[(starts.unsqueeze(1) + j).clamp(max=v.shape[0] - 1)]
    return torch.where(valid, rows, torch.zeros_like(rows)), valid


def prosody_contour(f0, y_lens):
    """``data.preprocess.interpolate_unvoiced`` of packed F0 tracks [Ry] (Hz, 0 = unvoiced): unvoiced frames take the
    line between the neighbouring voiced frames, the ends hold the first / last voiced value.
    -> (g [P, Ymax] zero-padded, valid [P, Ymax], voiced [P, Ymax], ok [P] = the utterance has a voiced frame;
    without one g is all zero)."""
    yl = _host_lens(y_lens)
    f0p, valid = _pad_frames(f0, yl)
    Ymax, big = f0p.shape[1], f0p.shape[1] + 1
    v = valid & (f0p > 0)
    j = torch.arange(Ymax, device=f0.device).unsqueeze(0).expand_as(f0p)
    a = torch.where(v, j, torch.full_like(j, -1)).cummax(1).values
    b = torch.where(v, j, torch.full_like(j, big)).flip(1).cummin(1).values.flip(1)
    has_a, has_b = a >= 0, b < big
    fa = torch.gather(f0p, 1, a.clamp(min=0))
    fb = torch.gather(f0p, 1, b.clamp(max=Ymax - 1))
    line = (fb - fa) / (b - a).clamp(min=1).to(f0.dtype) * (j - a).to(f0.dtype) + fa
    zero = torch.zeros_like(f0p)
    g = torch.where(v, f0p, torch.where(has_a & has_b, line, torch.where(has_a, fa, torch.where(has_b, fb, zero))))
    return torch.where(valid, g, zero), valid, v, v.any(1)


@torch.no_grad()
def prosody_transfer(path, path_len, src_dur, src_lens, x_lens, y_lens, f0, energy, pred_pitch, pitch_stats=(0.0, 1.0),
                     energy_stats=(0.0, 1.0), pitch_mode="relative", return_contour=False):
    """A recording's prosody as the per-token targets of the variance adaptor.  ``path`` [P, Lmax, 2] int32 /
    ``path_len`` [P]: ``dtw``'s alignment of P syntheses (index 0: frame i) with their recordings (index 1: frame j);
    ``src_dur`` [P, Nmax] the integer token durations of the syntheses, ``src_lens`` [P] their token counts;
    ``x_lens`` / ``y_lens`` host frame counts; ``f0`` [Ry] (Hz, 0 = unvoiced) / ``energy`` [Ry] the recordings' packed
    contours; ``pred_pitch`` [P, Nmax] the syntheses' normalised pitch (relative mode only); ``*_stats`` (mean, std)
    of the normalisation.

      owner(j) = (i_lo + i_hi) >> 1 over the run of path cells of recorded frame j
      token(j) = #{n : cumsum(src_dur)[n] <= min(owner(j), sum(src_dur) - 1)}: the token whose frames hold owner(j);
                 frames past the synthesis go to the last token with a duration.  Non-decreasing in j.
      rec_dur[n] = #{j : token(j) = n}: sums to y_len, 0 where src_dur is 0 (all 0 when every src_dur is)
      g = ``prosody_contour``; ``pitch_mode="relative"``: g <- g exp(L_pred - L_ref) with L_ref = mean_j ln g[j] and
          L_pred = the src_dur-weighted mean of ln max(pred_pitch std + mean, 1) -- the recording's contour at the
          synthesis' own level; ``"absolute"`` and utterances without a voiced frame: g as it is
      pitch[n] = (mean of g over the token's frames - mean) / std, energy[n] likewise (frames added in increasing j
          into one accumulator per token), voiced[n] = share of the token's frames with f0 > 0; 0 where rec_dur is 0

    Computes in f0's dtype (float64 = the oracle) on its device.
    -> rec_dur [P, Nmax] int32, pitch / energy / voiced [P, Nmax], pitch_ok [P] bool[, g [P, Ymax] as used]."""
    xl, yl = prosody_lens(path, path_len, src_dur, src_lens, x_lens, y_lens, f0, energy, pred_pitch, pitch_stats,
                          energy_stats, pitch_mode)
    dev, dt = f0.device, f0.dtype
    P, Nmax = src_dur.shape
    Ymax = max(yl) if P else 0
    if P == 0:
        z = torch.zeros(0, Nmax, dtype=dt, device=dev)
        out = (z.to(torch.int32), z, z.clone(), z.clone(), torch.zeros(0, dtype=torch.bool, device=dev))
        return out + (torch.zeros(0, 0, dtype=dt, device=dev),) if return_contour else out
    p_mean, p_std = float(pitch_stats[0]), float(pitch_stats[1])
    e_mean, e_std = float(energy_stats[0]), float(energy_stats[1])
    nl = _lens_on(src_lens, _host_lens(src_lens), dev)
    n_idx = torch.arange(Nmax, device=dev).unsqueeze(0)
    dur = torch.where(n_idx < nl.unsqueeze(1), src_dur.to(dev).long().clamp(min=0), torch.zeros((), dtype=torch.long, device=dev))
    ends = torch.cumsum(dur, 1)
    total = ends[:, -1]
    # runs of equal j: neighbouring cells compared
    L = path.shape[1]
    i, j = path[..., 0].long(), path[..., 1].long()
    ylens = torch.tensor(yl, dtype=torch.long, device=dev)
    cell = (torch.arange(L, device=dev).unsqueeze(0) < path_len.long().unsqueeze(1)) & (j >= 0) & (j < ylens.unsqueeze(1))
    jm = torch.where(cell, j, torch.full_like(j, -1))
    neg = torch.full_like(jm[:, :1], -1)
    first = cell & (jm != torch.cat([neg, jm[:, :-1]], 1))
    last = cell & (jm != torch.cat([jm[:, 1:], neg], 1))
    lo = torch.zeros(P, Ymax + 1, dtype=torch.long, device=dev)
    hi = torch.zeros(P, Ymax + 1, dtype=torch.long, device=dev)
    lo.scatter_(1, torch.where(first, j, torch.full_like(j, Ymax)), i)
    hi.scatter_(1, torch.where(last, j, torch.full_like(j, Ymax)), i)
    owner = (lo[:, :Ymax] + hi[:, :Ymax]) >> 1
    key = torch.minimum(owner, (total - 1).unsqueeze(1)).clamp(min=0)
    tok = torch.searchsorted(ends, key, right=True).clamp(max=Nmax)
    g, valid, v, ok = prosody_contour(f0, yl)
    tok = torch.where(valid & (total > 0).unsqueeze(1), tok, torch.full_like(tok, Nmax))  # slot Nmax: no token
    if pitch_mode == "relative":
        one = torch.ones_like(g)
        l_ref = torch.log(torch.where(g > 0, g, one)).sum(1) / ylens.to(dt)
        hz = (pred_pitch.to(dev, dt) * p_std + p_mean).clamp(min=1.0)
        l_pred = (dur.to(dt) * torch.log(hz)).sum(1) / total.clamp(min=1).to(dt)
        scale = torch.where(ok & (total > 0), torch.exp(l_pred - l_ref), torch.ones_like(l_ref))
        g = g * scale.unsqueeze(1)

    def sums(values):
        s = torch.zeros(P, Nmax + 1, dtype=dt, device=dev)
        s.scatter_add_(1, tok, values)
        return s[:, :Nmax]

    cnt = sums(valid.to(dt))
    some = cnt > 0
    c1 = torch.where(some, cnt, torch.ones_like(cnt))
    zero = torch.zeros_like(cnt)
    pitch = torch.where(some, (sums(g) / c1 - p_mean) / p_std, zero)
    en = torch.where(some, (sums(_pad_frames(energy.to(dt), yl)[0]) / c1 - e_mean) / e_std, zero)
    voiced = torch.where(some, sums(v.to(dt)) / c1, zero)
    out = (cnt.to(torch.int32), pitch, en, voiced, ok)
    return out + (g,) if return_contour else out


# --------------------------------------------------------- packed feature front-end (csrc/k_features.hip semantics)
FEATURE_NFFT = (512, 1024, 2048)


def feature_plan(wav, lengths, n_fft, hop, window, basis):
    """Host side of a packed ``frame_features`` batch, validated -> (sample counts, frame counts 1 + N // hop).
    ``ValueError`` with the offending value for a transform size the kernel does not cover, a hop <= 0, an utterance
    too short for the reflect padding (N <= n_fft / 2), lengths that do not add up, or a window / basis of the wrong
    shape."""
    n_fft, hop = int(n_fft), int(hop)
    if n_fft not in FEATURE_NFFT:
        raise ValueError(f"frame_features: n_fft {n_fft} not covered (512, 1024 or 2048)")
    if hop <= 0:
        raise ValueError(f"frame_features: hop {hop} must be positive")
    if wav.dim() != 1:
        raise ValueError(f"frame_features: wav must be one packed vector of samples, got shape {tuple(wav.shape)}")
    if window.dim() != 1 or window.shape[0] != n_fft or basis.dim() != 2 or basis.shape[1] != n_fft // 2 + 1:
        raise ValueError(f"frame_features: window [n_fft] / basis [n_mel, n_fft / 2 + 1] for n_fft {n_fft}, got "
                         f"{tuple(window.shape)} / {tuple(basis.shape)}")
    lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    for b, n in enumerate(lens):
        if n <= n_fft // 2:
            raise ValueError(f"frame_features: utterance {b} has {n} samples; reflect padding needs more than "
                             f"n_fft / 2 = {n_fft // 2}")
        if 2 * n + n_fft >= 2 ** 31:
            raise ValueError(f"frame_features: utterance {b} has {n} samples; positions inside an utterance are 32-bit")
    if sum(lens) != wav.shape[0]:
        raise ValueError(f"frame_features: lengths sum to {sum(lens)} but wav has {wav.shape[0]} samples")
    frames = [1 + n // hop for n in lens]
    if sum(frames) >= 2 ** 31 // max(1, basis.shape[0]):
        raise ValueError(f"frame_features: {sum(frames)} frame rows of {basis.shape[0]} mels; packed offsets are 32-bit")
    return lens, frames


def mel_support(basis):
    """[first non-zero, last non-zero + 1) of every row of a mel basis -> int32 [n_mel, 2] on the host; (0, 0) for an
    all-zero row.  Zeros inside the range contribute nothing to the projection, so this is right for any basis."""
    nz = (basis.detach().cpu() != 0)
    K = nz.shape[1]
    any_ = nz.any(1)
    idx = torch.arange(K)
    lo = torch.where(nz, idx, torch.full_like(idx, K)).min(1).values
    hi = torch.where(nz, idx + 1, torch.zeros_like(idx)).max(1).values
    lo = torch.where(any_, lo, torch.zeros_like(lo))
    return torch.stack([lo, hi], 1).to(torch.int32)


def frame_pairs(lens, frames):
    """Workgroup table of ``frame_features_kernel``: one entry per pair of consecutive frame rows 2p, 2p + 1 of one
    utterance (a last odd row stands alone) -> int32 [G, 6] on the host: {sample offset of the utterance, low and high
    word; N; first frame index inside the utterance; output row; rows in this pair (1 | 2)}."""
    import numpy as np

    lens, frames = np.asarray(lens, dtype=np.int64), np.asarray(frames, dtype=np.int64)
    off = np.zeros(len(lens), dtype=np.int64)
    off[1:] = np.cumsum(lens)[:-1]
    cu = np.zeros(len(lens), dtype=np.int64)
    cu[1:] = np.cumsum(frames)[:-1]
    groups = (frames + 1) // 2
    u = np.repeat(np.arange(len(lens)), groups)
    cg = np.zeros(len(lens), dtype=np.int64)
    cg[1:] = np.cumsum(groups)[:-1]
    first = 2 * (np.arange(int(groups.sum())) - cg[u])
    tab = np.stack([off[u] & 0xFFFFFFFF, off[u] >> 32, lens[u], first, cu[u] + first,
                    np.minimum(2, frames[u] - first)], axis=1)
    return torch.from_numpy(tab.astype(np.uint32).view(np.int32).reshape(-1, 6))


def frame_features(wav, lengths, n_fft, hop, window, basis, clip=1e-5, clip_wave=False):
    """Log-mel and energy of packed utterances (``wav`` one vector of all samples back to back, host sample counts
    ``lengths``): per utterance ``torch.stft(center=True, pad_mode="reflect")`` with the n_fft-point ``window`` ->
    |X| -> log(max(basis @ |X|, clip)) and energy = ||X||_2 over frequency, as ``TacotronSTFT.mel_spectrogram``;
    ``clip_wave`` clamps the samples to [-1, 1] first.  Computes in wav's dtype (float64 = the oracle) on wav's device.
    -> (mel [R, n_mel] row-major per frame row, energy [R], the frame counts 1 + N // hop as a host list)."""
    lens, frames = feature_plan(wav, lengths, n_fft, hop, window, basis)
    win, fb = window.to(wav.dtype), basis.to(wav.dtype)
    mels, ens, at = [], [], 0
    for n in lens:
        x = wav[at:at + n].unsqueeze(0)
        at += n
        if clip_wave:
            x = x.clamp(-1, 1)
        mag = torch.stft(x, int(n_fft), int(hop), int(n_fft), window=win, center=True, pad_mode="reflect",
                         return_complex=True).abs()  # [1, n_fft / 2 + 1, T]
        mels.append(torch.log(torch.clamp(torch.matmul(fb, mag), min=clip))[0].t())
        ens.append(torch.norm(mag, dim=1)[0])
    if not mels:
        return wav.new_zeros(0, basis.shape[0]), wav.new_zeros(0), frames
    return torch.cat(mels).contiguous(), torch.cat(ens), frames


def interp_plan(f0, frames):
    """Host frame counts of a packed contour batch, validated -> list[int]."""
    fr = [int(v) for v in (frames.tolist() if isinstance(frames, torch.Tensor) else frames)]
    if f0.dim() != 1 or any(t < 0 for t in fr) or sum(fr) != f0.shape[0]:
        raise ValueError(f"interp_unvoiced: frames sum to {sum(fr)} but f0 has shape {tuple(f0.shape)}")
    if f0.shape[0] >= 2 ** 31:
        raise ValueError("interp_unvoiced: packed row counts are 32-bit")
    return fr


def interp_unvoiced(f0, frames):
    """``data.preprocess.interpolate_unvoiced`` of every utterance of a packed F0 batch (host frame counts
    ``frames``): the zero frames filled linearly in Hz between the nearest non-zero frames (``np.interp``'s
    slope * (x - xa) + fa), the ends held; an utterance without a non-zero frame stays as it is.  Computes in f0's
    dtype.  -> (contour [R], n_voiced [P] int32: the non-zero frames per utterance)."""
    fr = interp_plan(f0, frames)
    outs, counts, at = [], [], 0
    for T in fr:
        y = f0[at:at + T]
        at += T
        v = y != 0
        nv = int(v.sum())
        counts.append(nv)
        if nv == 0 or T == 0:
            outs.append(y.clone())
            continue
        j = torch.arange(T, device=y.device)
        a = torch.cummax(torch.where(v, j, torch.full_like(j, -1)), 0).values
        b = torch.flip(torch.cummin(torch.flip(torch.where(v, j, torch.full_like(j, T)), [0]), 0).values, [0])
        ya, yb = y[a.clamp(min=0)], y[b.clamp(max=T - 1)]
        mid = (yb - ya) / (b - a).clamp(min=1).to(y.dtype) * (j - a).to(y.dtype) + ya
        g = torch.where(a < 0, yb, torch.where(b >= T, ya, mid))
        outs.append(torch.where(v, y, g))
    out = torch.cat(outs) if outs else f0.new_zeros(0)
    return out, torch.tensor(counts, dtype=torch.int32, device=f0.device)


# ------------------------------------------------------------------------ style map: exact t-SNE and k-means
TSNE_MAX_N = 16384        # a distance row of the perplexity kernel lives in LDS
TSNE_ENTROPY_TOL = 1e-5   # scikit-learn's exact method: |H - log perplexity| of a row
TSNE_BISECT_STEPS = 100
KMEANS_MAX_K = 64
KMEANS_MAX_D = 512


def tsne_check(x, perplexity):
    """Argument rules of ``tsne_affinities`` / ``tsne`` (the same on both paths) -> (N, D)."""
    if x.dim() != 2:
        raise ValueError(f"tsne: x must be [N, D], got shape {tuple(x.shape)}")
    N, D = x.shape
    if N < 7:
        raise ValueError(f"tsne: x has N = {N} points, at least 7 are needed")
    if N > TSNE_MAX_N:
        raise ValueError(f"tsne: x has N = {N} points, more than TSNE_MAX_N = {TSNE_MAX_N}; subsample first")
    if D < 1:
        raise ValueError("tsne: x has no columns")
    if not perplexity >= 2:
        raise ValueError(f"tsne: perplexity = {perplexity} is below 2")
    if perplexity > (N - 1) / 3:
        raise ValueError(f"tsne: perplexity = {perplexity} exceeds (N - 1) / 3 = {(N - 1) / 3:g}")
    return N, D


def pairwise_sqdist(x, chunk_elems=1 << 24):
    """Squared Euclidean distances [N, N], summed from the differences (never from norms) in row chunks, so that no
    N x N x D temporary exists."""
    N, D = x.shape
    out = x.new_empty(N, N)
    rows = max(1, min(N, chunk_elems // max(1, N * D)))
    for r0 in range(0, N, rows):
        d = x[r0:r0 + rows, None, :] - x[None, :, :]
        out[r0:r0 + rows] = (d * d).sum(-1)
    return out


def tsne_conditional(x, perplexity):
    """The row-normalised affinities of t-SNE -> (P_cond [N, N] with a zero diagonal, beta [N] as last evaluated).
    Per row: the smallest off-diagonal distance is subtracted before the exponential (P is unchanged, the row sum is
    >= 1 and fp32 stays in range), then beta is bisected as scikit-learn's exact method does it: beta = 1, at most 100
    steps, a row stops at |H - log perplexity| <= 1e-5 and keeps the P of that evaluation, beta doubles / halves while
    a bound is infinite and takes the midpoint otherwise."""
    N, _ = tsne_check(x, perplexity)
    dt, dev = x.dtype, x.device
    dist = pairwise_sqdist(x)
    eye = torch.eye(N, dtype=torch.bool, device=dev)
    dmin = dist.masked_fill(eye, float("inf")).min(dim=1, keepdim=True).values
    dist = dist - dmin
    target = math.log(perplexity)
    beta = torch.ones(N, 1, dtype=dt, device=dev)
    lo = torch.full_like(beta, -float("inf"))
    hi = torch.full_like(beta, float("inf"))
    active = torch.ones(N, 1, dtype=torch.bool, device=dev)
    P = torch.zeros_like(dist)
    beta_used = beta.clone()
    for _ in range(TSNE_BISECT_STEPS):
        p = torch.exp(-dist * beta).masked_fill(eye, 0.0)
        s = p.sum(1, keepdim=True)
        H = torch.log(s) + beta * (dist * p).sum(1, keepdim=True) / s
        P = torch.where(active, p / s, P)
        beta_used = torch.where(active, beta, beta_used)
        diff = H - target
        active = active & ~(diff.abs() <= TSNE_ENTROPY_TOL)
        if not bool(active.any()):
            break
        up = active & (diff > 0)   # entropy too high: raise beta
        dn = active & ~(diff > 0)
        lo = torch.where(up, beta, lo)
        hi = torch.where(dn, beta, hi)
        nb_up = torch.where(torch.isinf(hi), beta * 2, (beta + hi) / 2)
        nb_dn = torch.where(torch.isinf(lo), beta / 2, (beta + lo) / 2)
        beta = torch.where(up, nb_up, torch.where(dn, nb_dn, beta))
    return P, beta_used.reshape(N)


def tsne_affinities(x, perplexity):
    """Joint affinities of exact t-SNE: x [N, D] -> P [N, N] = (P_cond + P_cond^T) / sum, symmetric, zero diagonal,
    sums to 1 (``tsne_conditional``).  Computes in x's dtype; float64 is the oracle."""
    pc, _ = tsne_conditional(x, perplexity)
    s = pc + pc.t()
    return s / s.sum()


def _tsne_w(y):
    d = y[:, None, :] - y[None, :, :]
    w = 1.0 / (1.0 + (d * d).sum(-1))
    return d, w.masked_fill(torch.eye(y.shape[0], dtype=torch.bool, device=y.device), 0.0)


def tsne_gradient(P, y, exaggeration=1.0):
    """Gradient of KL(exaggeration * P || Q) for the Student-t map y [N, 2] -> (attr [N, 2], rep [N, 2], zrow [N],
    grad [N, 2]): w_ij = 1 / (1 + |y_i - y_j|^2), attr_i = sum_j P_ij w_ij (y_i - y_j), rep_i = sum_j w_ij^2
    (y_i - y_j), zrow_i = sum_j w_ij, grad = 4 (exaggeration attr - rep / sum zrow)."""
    d, w = _tsne_w(y)
    attr = ((P * w).unsqueeze(-1) * d).sum(1)
    rep = ((w * w).unsqueeze(-1) * d).sum(1)
    zrow = w.sum(1)
    grad = 4.0 * (exaggeration * attr - rep / zrow.sum())
    return attr, rep, zrow, grad


def tsne_kl(P, y):
    """KL(P || Q) of the map: sum_{P > 0} P (log P - log w) + log Z."""
    _, w = _tsne_w(y)
    pos = P > 0
    eye = torch.eye(y.shape[0], dtype=torch.bool, device=y.device)
    lw = torch.log(torch.where(eye, torch.ones_like(w), w))
    lp = torch.log(torch.where(pos, P, torch.ones_like(P)))
    return (torch.where(pos, P * (lp - lw), torch.zeros_like(P))).sum() + torch.log(w.sum())


def tsne_step(grad, y, update, gains, momentum, lr):
    """One descent step with per-element gains -> (y, update, gains): gains + 0.2 where update and gradient disagree
    in sign (update * grad < 0), x 0.8 otherwise, floor 0.01; update = momentum update - lr gains grad."""
    inc = update * grad < 0
    gains = torch.where(inc, gains + 0.2, gains * 0.8).clamp(min=0.01)
    update = momentum * update - lr * (gains * grad)
    return y + update, update, gains


def tsne_learning_rate(N, early_exaggeration=12.0):
    return max(N / early_exaggeration / 4.0, 50.0)


def tsne_init(x, init="pca", seed=0):
    """The start of the map, [N, 2] in x's dtype on x's device, made on the host so that every path starts from the
    same y0.  "pca": the top two eigenvectors of the D x D covariance in float64, each sign fixed so that the entry of
    largest magnitude is positive, scaled so that the first component has standard deviation 1e-4.  "random":
    N(0, 1e-4^2) from a seeded CPU generator.  A tensor is taken as it is."""
    N = x.shape[0]
    if isinstance(init, torch.Tensor):
        if tuple(init.shape) != (N, 2):
            raise ValueError(f"tsne: init must be [{N}, 2], got shape {tuple(init.shape)}")
        return init.detach().to(device=x.device, dtype=x.dtype).clone()
    if init == "random":
        g = torch.Generator().manual_seed(int(seed))
        y = torch.randn(N, 2, generator=g, dtype=torch.float64) * 1e-4
    elif init == "pca":
        xc = x.detach().to("cpu", torch.float64)
        xc = xc - xc.mean(0, keepdim=True)
        cov = xc.t() @ xc / max(N - 1, 1)
        _, vec = torch.linalg.eigh(cov)
        comp = vec[:, -2:].flip(1) if vec.shape[1] >= 2 else torch.cat([vec, torch.zeros_like(vec)], 1)
        big = comp.abs().argmax(0)
        sign = torch.sign(comp[big, torch.arange(comp.shape[1])])
        comp = comp * torch.where(sign == 0, torch.ones_like(sign), sign)
        y = xc @ comp
        sd = y[:, 0].std()
        y = y / sd * 1e-4 if sd > 0 else y
    else:
        raise ValueError(f"tsne: init must be 'pca', 'random' or a tensor, got {init!r}")
    return y.to(device=x.device, dtype=x.dtype)


def tsne_plan(n_iter, exag_iter, early_exaggeration, kl_every):
    """Per iteration (exaggeration, momentum, record KL before this step?) and the iteration counts the KL trace
    reports: every ``kl_every`` updates and after the last one."""
    if n_iter < 1 or exag_iter < 0 or kl_every < 1:
        raise ValueError("tsne: n_iter >= 1, exag_iter >= 0 and kl_every >= 1 are needed")
    steps = [(float(early_exaggeration) if it < exag_iter else 1.0, 0.5 if it < exag_iter else 0.8,
              it > 0 and it % kl_every == 0) for it in range(n_iter)]
    at = [it for it in range(kl_every, n_iter, kl_every)] + [n_iter]
    return steps, at


def tsne(x, perplexity=30.0, n_iter=750, exag_iter=250, early_exaggeration=12.0, init="pca", seed=0, kl_every=50,
         P=None):
    """Exact t-SNE of x [N, D] -> (y [N, 2], kl_trace): gradient descent with momentum 0.5 during the ``exag_iter``
    exaggerated iterations and 0.8 after, learning rate max(N / early_exaggeration / 4, 50), per-element gains, a
    fixed iteration count.  kl_trace[i] is KL(P || Q) (never exaggerated) after ``tsne_plan``'s i-th count of updates;
    its last entry is the final map's.  Computes in x's dtype."""
    N, _ = tsne_check(x, perplexity)
    steps, _ = tsne_plan(n_iter, exag_iter, early_exaggeration, kl_every)
    if P is None:
        P = tsne_affinities(x, perplexity)
    y = tsne_init(x, init, seed)
    lr = tsne_learning_rate(N, early_exaggeration)
    update, gains = torch.zeros_like(y), torch.ones_like(y)
    trace = []
    for ex, mom, rec in steps:
        if rec:
            trace.append(float(tsne_kl(P, y)))
        grad = tsne_gradient(P, y, ex)[3]
        y, update, gains = tsne_step(grad, y, update, gains, mom, lr)
    trace.append(float(tsne_kl(P, y)))
    return y, trace


def kmeans_check(x, k):
    if x.dim() != 2:
        raise ValueError(f"kmeans: x must be [N, D], got shape {tuple(x.shape)}")
    N, D = x.shape
    if not 1 <= k <= KMEANS_MAX_K:
        raise ValueError(f"kmeans: k = {k} is outside 1 .. {KMEANS_MAX_K}")
    if k > N:
        raise ValueError(f"kmeans: k = {k} exceeds N = {N}")
    if not 1 <= D <= KMEANS_MAX_D:
        raise ValueError(f"kmeans: D = {D} is outside 1 .. {KMEANS_MAX_D}")
    return N, D


def _sqdist_ordered(x, c):
    """[N, k] squared distances, summed over the columns in increasing order, every product and sum rounded on its
    own: what one accumulator per pair gives."""
    acc = x.new_zeros(x.shape[0], c.shape[0])
    for d in range(x.shape[1]):
        df = x[:, d:d + 1] - c[None, :, d]
        acc = acc + df * df
    return acc


def kmeans(x, k, n_iter=100, seed=0):
    """Lloyd's k-means with a farthest-point start -> (labels int32 [N], centroids [k, D], iterations).  The first
    centre is point ``seed % N``; each next one is the point farthest from its nearest chosen centre (lowest index on
    ties).  A step assigns every point to its nearest centroid (lowest index on ties; distances summed from the
    differences in column order) and sets each centroid to sum / count of its points in index order; an empty cluster
    keeps its centroid.  Stops when no label changes, or after ``n_iter`` steps."""
    N, D = kmeans_check(x, k)
    if n_iter < 1:
        raise ValueError("kmeans: n_iter must be at least 1")
    idx = int(seed) % N
    cent = x.new_empty(k, D)
    mind = x.new_full((N,), float("inf"))
    for c in range(k):
        cent[c] = x[idx]
        mind = torch.minimum(mind, _sqdist_ordered(x, cent[c:c + 1])[:, 0])
        idx = int(torch.nonzero(mind == mind.max())[0])
    labels = torch.full((N,), -1, dtype=torch.int64, device=x.device)
    iterations = 0
    for it in range(n_iter):
        dist = _sqdist_ordered(x, cent)
        best = dist.min(1, keepdim=True).values
        ids = torch.arange(k, device=x.device).expand(N, k)
        new = torch.where(dist == best, ids, torch.full_like(ids, k)).min(1).values  # first index of the minimum
        changed = int((new != labels).sum())
        labels = new
        iterations = it + 1
        if changed == 0:
            break
        sums = x.new_zeros(k, D).index_add_(0, labels, x)
        cnt = torch.bincount(labels, minlength=k)
        has = cnt > 0
        cent = torch.where(has[:, None], sums / cnt.clamp(min=1).to(x.dtype)[:, None], cent)
    return labels.to(torch.int32), cent, iterations


# ------------------------------------------------------------------------ iSTFTNet head
def istft_head_check(x, w, n_fft: int, hop: int):
    """Shape rules of the iSTFTNet head; -> (x as [B, T, C], whether x came without a batch axis)."""
    single = x.dim() == 2
    xb = x.unsqueeze(0) if single else x
    if xb.dim() != 3:
        raise ValueError("istft_head: x must be [B, T, C] or [T, C]")
    if n_fft < 2 or n_fft % 2 or hop < 1 or hop > n_fft:
        raise ValueError(f"istft_head: n_fft {n_fft} / hop {hop}")
    if w.dim() != 3 or tuple(w.shape) != (n_fft + 2, xb.shape[2], 7):
        raise ValueError(f"istft_head: weight {tuple(w.shape)}, expected {(n_fft + 2, xb.shape[2], 7)}")
    if xb.shape[1] < 2:
        raise ValueError("istft_head: the reflection pad needs at least 2 rows per utterance")
    return xb, single


def istft_head(x, w, b, n_fft: int, hop: int, slope: float = 0.01):
    """iSTFTNet head on last-stage rows x [B, T, C] (or [T, C]): leaky_relu(slope) -> one reflected row on the
    left -> Conv1d(C, n_fft + 2, 7, padding 3) (w [n_fft + 2, C, 7], b [n_fft + 2]) -> mag = exp(first n_fft/2 + 1
    channels), phase = sin(the others) -> inverse real DFT of each of the T + 1 frames, periodic Hann window ->
    overlap-add at ``hop`` over the window envelope, the centred hop * T samples kept -> [B, hop * T] (or
    [hop * T]).  The direct formula (a DFT-basis matmul and ``F.fold``, no FFT) in the dtype of x: in float64 it is
    the oracle of the HIP kernel, and it equals ``torch.istft(mag * exp(i phase), n_fft, hop, n_fft, hann,
    center=True)``.  Differentiable."""
    xb, single = istft_head_check(x, w, n_fft, hop)
    dt, dev = xb.dtype, xb.device
    B, T, _ = xb.shape
    N, H, nb = int(n_fft), int(hop), n_fft // 2 + 1
    a = F.leaky_relu(xb, slope)
    p = torch.cat([a[:, 1:2], a], 1)
    z = F.conv1d(p.transpose(1, 2), w.to(dt), None if b is None else b.to(dt), padding=3)  # [B, N + 2, T + 1]
    mag, phi = torch.exp(z[:, :nb]), torch.sin(z[:, nb:])
    k = torch.arange(nb, device=dev, dtype=torch.float64)[:, None]
    n = torch.arange(N, device=dev, dtype=torch.float64)[None, :]
    ck = torch.full((nb, 1), 2.0, device=dev, dtype=torch.float64)
    ck[0] = ck[nb - 1] = 1.0
    ang = 2.0 * math.pi * k * n / N
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / N)  # periodic Hann [1, N]
    bc = (ck * torch.cos(ang) * win / N).to(dt)  # [nb, N]
    bs = (ck * torch.sin(ang) * win / N).to(dt)
    re, im = mag * torch.cos(phi), mag * torch.sin(phi)  # [B, nb, F]
    frames = torch.einsum("bkf,kn->bnf", re, bc) - torch.einsum("bkf,kn->bnf", im, bs)  # [B, N, F]
    full = H * T + N  # H * (F - 1) + N
    y = F.fold(frames, (1, full), (1, N), stride=(1, H)).reshape(B, full)
    env = F.fold((win.to(dt) ** 2).reshape(1, N, 1).expand(1, N, T + 1), (1, full), (1, N),
                 stride=(1, H)).reshape(1, full)
    y = y[:, N // 2: N // 2 + H * T] / env[:, N // 2: N // 2 + H * T]
    return y[0] if single else y
