"""FastSpeech2 with optional speaking-style conditioning (FiLM reference encoder or GST).

Forward order and outputs follow the reference's ``model/fastspeech2.py:44-120``:
masks -> style encoder (gamma, beta) -> encoder (FiLM) -> + speaker embedding ->
VarianceAdaptor -> decoder (FiLM) -> mel_linear -> PostNet residual, returning
the same 10-tuple.  Activations are channel-last in the compute dtype (bf16 on
MI355X, fp32 on CPU); mel outputs are fp32.

Fixed reference bugs: no per-forward debug prints (D3),
style encoder optional (D2), consistent rounding of controlled durations (D11),
device derived from tensors (D19), synthesis without a reference mel uses a
neutral style.
"""
from __future__ import annotations

import json
import math
import os
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..ops.weights import DerivedCache
from ..config import style_mode
from ..text.symbols import symbols
from .layers import FFTBlock, FiLM, LinearNorm, PostNet, fused_param_groups
from .style import GlobalStyleTokens, ReferenceEncoder


def _pe_param(n_position: int, d: int) -> nn.Parameter:
    return nn.Parameter(ops.sinusoid_table(n_position, d).unsqueeze(0), requires_grad=False)


_pe_cast = DerivedCache()  # positional table -> its copy in the dtype last asked for


def positional_rows(pe_param: torch.Tensor, length: int, d: int, device, dtype=None) -> torch.Tensor:
    """First ``length`` sinusoid rows; beyond the stored table (eval on long
    inputs, reference ``transformer/Models.py:82-87``) they are generated.  ``dtype``: the rows in that dtype,
    from a copy of the (constant, non-trainable) table in that dtype, cached per version and weight generation."""
    if length <= pe_param.shape[1]:
        if dtype is None or dtype == pe_param.dtype:
            return pe_param[0, :length]
        return _pe_cast.get(pe_param, (pe_param,), lambda: pe_param[0].to(dtype).contiguous(), extra=dtype)[:length]
    t = ops.sinusoid_table(length, d, device=device)
    return t if dtype is None else t.to(dtype)


class Encoder(nn.Module):
    """Phoneme embedding + PE + N FFT blocks (``transformer/Models.py:33-101``)."""

    def __init__(self, config, film=False):
        super().__init__()
        tr = config["transformer"]
        d = tr["encoder_hidden"]
        self.max_seq_len = config["max_seq_len"]
        self.d_model = d
        self.src_word_emb = nn.Embedding(len(symbols) + 1, d, padding_idx=0)
        self.position_enc = _pe_param(self.max_seq_len + 1, d)
        nh = tr["encoder_head"]
        self.layer_stack = nn.ModuleList(
            FFTBlock(d, nh, d // nh, d // nh, tr["conv_filter_size"], tr["conv_kernel_size"], tr["encoder_dropout"], film=film)
            for _ in range(tr["encoder_layer"])
        )

    def forward(self, texts, src_lens, style=None, compute_dtype=torch.float32):
        T = texts.shape[1]
        pe = positional_rows(self.position_enc, T, self.d_model, texts.device, compute_dtype)
        # the fp32 table itself: the HIP op reads its cached bf16 image and writes the gradient slot
        tab = self.src_word_emb.weight if ops.use_hip(texts) else self.src_word_emb.weight.to(compute_dtype)
        x = ops.embed_add_pe(texts, tab, pe)
        for layer in self.layer_stack:
            x = layer(x, src_lens, style)
        return x


class Decoder(nn.Module):
    """PE + N FFT blocks; training truncates to ``max_seq_len`` frames
    (``transformer/Models.py:104-170``)."""

    def __init__(self, config, film=False):
        super().__init__()
        tr = config["transformer"]
        d = tr["decoder_hidden"]
        self.max_seq_len = config["max_seq_len"]
        self.d_model = d
        self.position_enc = _pe_param(self.max_seq_len + 1, d)
        nh = tr["decoder_head"]
        self.layer_stack = nn.ModuleList(
            FFTBlock(d, nh, d // nh, d // nh, tr["conv_filter_size"], tr["conv_kernel_size"], tr["decoder_dropout"], film=film)
            for _ in range(tr["decoder_layer"])
        )

    def forward(self, x, mel_lens, style=None):
        M = x.shape[1]
        if self.training and M > self.max_seq_len:
            M = self.max_seq_len
            x = x[:, :M]
            mel_lens = mel_lens.clamp(max=M)
        pe = positional_rows(self.position_enc, M, self.d_model, x.device, x.dtype)
        x = x + pe.unsqueeze(0)
        for layer in self.layer_stack:
            x = layer(x, mel_lens, style)
        return x, mel_lens

    def forward_packed(self, x_phone, durations, mel_lens, M, R, style=None):
        """Length regulation + decoder over the valid frames only (``ops/packing.py``).

        Same result as ``forward(LR(x_phone))`` on every valid frame; returns the packed
        ``[1, R, C]`` output, the (truncated) lengths and the PackInfo."""
        if self.training and M > self.max_seq_len:
            M = self.max_seq_len
        dec_lens = mel_lens.clamp(max=M)
        pk = ops.PackInfo.build(dec_lens, M, R)
        pe = positional_rows(self.position_enc, M, self.d_model, x_phone.device, x_phone.dtype)
        x = ops.length_regulate_packed(x_phone, durations, pk, pe)
        for layer in self.layer_stack:
            x = layer(x, dec_lens, style, pack=pk)
        return x, dec_lens, pk


class VariancePredictor(nn.Module):
    """[Conv1d k3 -> ReLU -> LN -> Dropout] x2 -> [FiLM] -> Linear(1) -> mask
    (``model/modules.py:204-259``)."""

    def __init__(self, model_config, film=False):
        super().__init__()
        d_in = model_config["transformer"]["encoder_hidden"]
        vp = model_config["variance_predictor"]
        fs, k, self.dropout = vp["filter_size"], vp["kernel_size"], vp["dropout"]
        from collections import OrderedDict

        from .layers import ConvHolder

        self.conv_layer = nn.Sequential(OrderedDict([
            ("conv1d_1", ConvHolder(d_in, fs, k)),
            ("relu_1", nn.ReLU()),
            ("layer_norm_1", nn.LayerNorm(fs)),
            ("dropout_1", nn.Dropout(self.dropout)),
            ("conv1d_2", ConvHolder(fs, fs, k)),
            ("relu_2", nn.ReLU()),
            ("layer_norm_2", nn.LayerNorm(fs)),
            ("dropout_2", nn.Dropout(self.dropout)),
        ]))
        if film:
            self.film = FiLM()
        self.linear_layer = nn.Linear(fs, 1)

    def forward(self, x, lengths, style=None):
        return self.rest(self.first(x), lengths, style)

    def first(self, x):
        """The first block: conv 1 -> ReLU -> LN -> dropout."""
        cl = self.conv_layer
        c1 = cl.conv1d_1
        return ops.conv_relu_layernorm(x, c1.conv.weight, c1.conv.bias, c1.pad, c1.dil, cl.layer_norm_1.weight,
                                       cl.layer_norm_1.bias, post_drop=self.dropout, training=self.training)

    def first_block(self):
        """(conv weight, conv bias, (LN weight, LN bias)) of the first conv block (fused with another
        predictor's on a shared input: ``ops.dual_conv_relu_layernorm``)."""
        cl = self.conv_layer
        return cl.conv1d_1.conv.weight, cl.conv1d_1.conv.bias, (cl.layer_norm_1.weight, cl.layer_norm_1.bias)

    def rest(self, h, lengths, style=None):
        """Everything after the first block: conv 2 -> ReLU -> LN -> dropout -> [FiLM] -> Linear -> mask."""
        cl = self.conv_layer
        c2 = cl.conv1d_2
        fp = self.film.pack(style) if (style is not None and hasattr(self, "film")) else None
        h = ops.conv_relu_layernorm(h, c2.conv.weight, c2.conv.bias, c2.pad, c2.dil, cl.layer_norm_2.weight,
                                    cl.layer_norm_2.bias, post_drop=self.dropout, training=self.training,
                                    film_params=fp)
        return ops.predictor_head(h, self.linear_layer.weight, self.linear_layer.bias, lengths)


def _apply_control(pred, control):
    if isinstance(control, torch.Tensor):
        control = control.to(pred.device, pred.dtype)
        if control.dim() == 2 and control.shape[1] != pred.shape[1]:
            control = F.pad(control, (0, pred.shape[1] - control.shape[1]), value=1.0)[:, : pred.shape[1]]
        return pred * control
    return pred * control if control != 1.0 else pred


class VarianceAdaptor(nn.Module):
    """Duration / pitch / energy predictors, bucketized embeddings and the
    length regulator (``model/modules.py:20-165``).  Only the duration predictor
    receives the style FiLM (``modules.py:121``; D7 preserved).  Controls may be
    scalars or per-phoneme ``[B, T]`` tensors (word-level control, the reference
    ``notebooks/control.ipynb`` cells 17-23)."""

    def __init__(self, preprocess_config, model_config, film=False):
        super().__init__()
        self.duration_predictor = VariancePredictor(model_config, film)
        self.pitch_predictor = VariancePredictor(model_config, film)
        self.energy_predictor = VariancePredictor(model_config, film)
        pp = preprocess_config["preprocessing"]
        self.pitch_feature_level = pp["pitch"]["feature"]
        self.energy_feature_level = pp["energy"]["feature"]
        ve = model_config["variance_embedding"]
        n_bins = ve["n_bins"]
        stats = _load_stats(preprocess_config)
        p_min, p_max = stats["pitch"][:2]
        e_min, e_max = stats["energy"][:2]
        self.pitch_bins = nn.Parameter(_bins(p_min, p_max, n_bins, ve["pitch_quantization"]), requires_grad=False)
        self.energy_bins = nn.Parameter(_bins(e_min, e_max, n_bins, ve["energy_quantization"]), requires_grad=False)
        d = model_config["transformer"]["encoder_hidden"]
        self.pitch_embedding = nn.Embedding(n_bins, d)
        self.energy_embedding = nn.Embedding(n_bins, d)

    def arena_groups(self):
        """Duration + pitch first convs adjacent in the flat arena (both read the encoder output x when
        pitch is phoneme-level): the fused [512, 256, k] weight of ONE GEMM is a view."""
        if self.pitch_feature_level != "phoneme_level":
            return []
        d = self.duration_predictor.conv_layer.conv1d_1.conv
        p = self.pitch_predictor.conv_layer.conv1d_1.conv
        return [[d.weight, p.weight], [d.bias, p.bias]]

    def _variance(self, predictor, bins, table, x, target, lengths, control, h1=None):
        pred = predictor(x, lengths) if h1 is None else predictor.rest(h1, lengths)
        if target is not None:
            values = target
        else:
            pred = _apply_control(pred, control)
            values = pred
        x = ops.bucketize_embed_add(x, values, bins, table.weight if ops.use_hip(x) else table.weight.to(x.dtype))
        return pred, x

    def packable(self):
        """Frame-level variance features act on the padded frame domain: no packed decoder then."""
        return self.pitch_feature_level == "phoneme_level" and self.energy_feature_level == "phoneme_level"

    def forward(self, x, src_lens, mel_lens=None, max_len=None, pitch_target=None, energy_target=None,
                duration_target=None, p_control=1.0, e_control=1.0, d_control=1.0, style=None, regulate=True,
                exact_pad=False):
        """``exact_pad`` (inference on the unregulated path): every tensor a k = 3 predictor conv reads has its rows
        past ``src_lens`` zeroed first, so a text padded inside a longer bucket gets the predictions of the unpadded
        text (the reference lets the speaker / pitch embeddings and the LayerNorm output of the pad rows leak into
        the last phonemes of the shorter texts of a batch, and so does every other path here)."""
        p_pred = e_pred = None
        assert not exact_pad or (not regulate and not self.training), "exact_pad: the packed inference path only"

        def mp(t):
            return ops.mask_pad_rows_(t, src_lens) if exact_pad else t

        x = mp(x)
        if self.pitch_feature_level == "phoneme_level":
            # duration and pitch predictors read the same x: their first conv blocks run as one GEMM
            dp, pp_ = self.duration_predictor, self.pitch_predictor
            wd, bd, lnd = dp.first_block()
            wp, bp, lnp = pp_.first_block()
            c1 = dp.conv_layer.conv1d_1
            h_d, h_p = ops.dual_conv_relu_layernorm(x, (wd, wp), (bd, bp), c1.pad, c1.dil, (lnd, lnp),
                                                    post_drop=dp.dropout, training=self.training)
            log_d = dp.rest(mp(h_d), src_lens, style)
            p_pred, x = self._variance(pp_, self.pitch_bins, self.pitch_embedding, x, pitch_target, src_lens, p_control,
                                       h1=mp(h_p))
            x = mp(x)
        else:
            log_d = self.duration_predictor.rest(mp(self.duration_predictor.first(x)), src_lens, style)
        if self.energy_feature_level == "phoneme_level":
            e_pred, x = self._variance(self.energy_predictor, self.energy_bins, self.energy_embedding, x, energy_target,
                                       src_lens, e_control, h1=mp(self.energy_predictor.first(x)))

        if not regulate:  # the packed decoder regulates itself (Decoder.forward_packed)
            return x, p_pred, e_pred, log_d, duration_target, mel_lens
        if duration_target is not None:
            d_rounded = duration_target
            x, mel_len = ops.length_regulate(x, duration_target, max_len)
            if mel_lens is not None:
                mel_len = mel_lens
        else:
            d_rounded, mel_len = ops.duration_round(log_d, src_lens, d_control)  # one kernel on the GPU
            x, mel_len = ops.length_regulate(x, d_rounded, None, mel_len=mel_len)

        if self.pitch_feature_level == "frame_level":
            p_pred, x = self._variance(self.pitch_predictor, self.pitch_bins, self.pitch_embedding, x, pitch_target, mel_len, p_control)
        if self.energy_feature_level == "frame_level":
            e_pred, x = self._variance(self.energy_predictor, self.energy_bins, self.energy_embedding, x, energy_target, mel_len, e_control)
        return x, p_pred, e_pred, log_d, d_rounded, mel_len


def _bins(lo, hi, n_bins, quant):
    if quant == "log":
        if not lo > 0:
            raise ValueError(
                f"log pitch/energy quantization needs positive feature stats (min={lo}); z-score normalised "
                "features (preprocessing.*.normalization: True) only work with linear quantization")
        return torch.exp(torch.linspace(math.log(lo), math.log(hi), n_bins - 1))
    return torch.linspace(lo, hi, n_bins - 1)


def _load_stats(preprocess_config):
    path = os.path.join(preprocess_config["path"]["preprocessed_path"], "stats.json")
    if os.path.exists(path):
        with open(path) as f:
            return json.load(f)
    # no stats.json (synthetic runs / fresh configs): a generous range in the features' own units --
    # z-scores when normalised, Hz and STFT-magnitude energy otherwise (positive: log bins work)
    pp = preprocess_config["preprocessing"]
    norm_p = pp["pitch"].get("normalization", True)
    norm_e = pp["energy"].get("normalization", True)
    return {"pitch": [-4.0, 12.0, 0.0, 1.0] if norm_p else [40.0, 900.0, 0.0, 1.0],
            "energy": [-2.0, 10.0, 0.0, 1.0] if norm_e else [0.01, 400.0, 0.0, 1.0]}


def _spker_table(preprocess_config):
    """[n_speakers, dim] fp32 table of ``spker_embed/{speaker}-spker_embed.npy`` (ordered by the
    speakers.json ids), or None when no speaker embedder is configured.  Missing files are an error."""
    emb = preprocess_config["preprocessing"].get("speaker_embedder", "none")
    if emb in (None, "none"):
        return None
    root = preprocess_config["path"]["preprocessed_path"]
    with open(os.path.join(root, "speakers.json")) as f:
        smap = json.load(f)
    import numpy as np

    rows = [None] * len(smap)
    for name, i in smap.items():
        v = np.load(os.path.join(root, "spker_embed", f"{name}-spker_embed.npy"), allow_pickle=False)
        rows[int(i)] = np.asarray(v, dtype=np.float32).reshape(-1)
    return torch.from_numpy(np.stack(rows))


def _n_speakers(preprocess_config):
    path = os.path.join(preprocess_config["path"]["preprocessed_path"], "speakers.json")
    if os.path.exists(path):
        with open(path) as f:
            return len(json.load(f))
    return int(preprocess_config.get("n_speakers", 1))


class FastSpeech2(nn.Module):
    def __init__(self, preprocess_config, model_config):
        super().__init__()
        self.model_config = model_config
        self.style = style_mode(model_config)
        film = self.style != "none"
        self.encoder = Encoder(model_config, film=film)
        if self.style == "film":
            self.reference_encoder = ReferenceEncoder(preprocess_config, model_config)
        elif self.style == "gst":
            self.gst = GlobalStyleTokens(preprocess_config, model_config)
        self.variance_adaptor = VarianceAdaptor(preprocess_config, model_config, film=film)
        self.decoder = Decoder(model_config, film=film)
        n_mel = preprocess_config["preprocessing"]["mel"]["n_mel_channels"]
        self.mel_linear = nn.Linear(model_config["transformer"]["decoder_hidden"], n_mel)
        self.postnet = PostNet(n_mel)
        self.speaker_emb = None
        d = model_config["transformer"]["encoder_hidden"]
        if model_config["multi_speaker"]:
            self.speaker_emb = nn.Embedding(_n_speakers(preprocess_config), d)
        # external speaker embeddings (reference ``synthesize.py:268-277``: ``{spk}-spker_embed.npy`` under
        # ``preprocessed_path/spker_embed`` when ``preprocessing.speaker_embedder != 'none'``).  The
        # reference loads them and drops them, and so does this model unless ``speaker_embed_proj: true``
        # is set in model.yaml (opt-in: it adds a trainable projection the reference checkpoints lack).
        # With it, a per-speaker table (non-persistent buffer, looked up by speaker id in training and
        # synthesis alike) is projected to the encoder width and added next to the speaker-id embedding.
        use_table = model_config["multi_speaker"] and bool(model_config.get("speaker_embed_proj", False))
        table = _spker_table(preprocess_config) if use_table else None
        self.spker_embed_proj = None
        if table is not None:
            self.register_buffer("spker_table", table, persistent=False)
            self.spker_embed_proj = nn.Linear(table.shape[1], d)
        # alignment learner (model.yaml ``aligner:`` block; absent by default): durations for teacher forcing come
        # from its Viterbi path when the batch carries none (preprocessing.duration.source: learned)
        self.aligner = None
        if model_config.get("aligner"):
            from .aligner import AlignmentEncoder

            self.aligner = AlignmentEncoder(n_mel, d, model_config["aligner"])
        self.compute_dtype = torch.float32

    # ------------------------------------------------------------------ helpers
    def set_compute_dtype(self, dtype):
        self.compute_dtype = dtype
        return self

    def fused_param_groups(self):
        return fused_param_groups(self)

    def style_encoder(self):
        return getattr(self, "reference_encoder", None) or getattr(self, "gst", None)

    def film_scalars(self):
        """Stacked s_gamma/s_beta parameters (reference ``utils/model.py:53-59``).  The parameter
        list is collected once (named_parameters() walks the whole module tree every call)."""
        ps = self._film_param_list()
        if not ps:
            return None
        if ops.use_hip(ps[0]):
            from ..ops import hip

            return hip.film_scalars_cat(ps)  # L2 gradient folded into the sites' FiLM kernels
        return torch.cat(ps)

    def _film_param_list(self):
        ps = self.__dict__.get("_film_ps")
        if ps is None:
            ps = [p for n, p in self.named_parameters() if ("s_gamma" in n or "s_beta" in n)]
            self.__dict__["_film_ps"] = ps
        return ps

    def compute_style(self, mels, mel_lens, max_mel_len, batch, device, style_weights=None):
        enc = self.style_encoder()
        if enc is None:
            return None
        if style_weights is not None and self.style == "gst":
            g, b = self.gst.from_token_weights(style_weights.to(device))
        elif mels is None:
            d = self.model_config["transformer"]["encoder_hidden"]
            z = torch.zeros(batch, d, device=device, dtype=self.compute_dtype)
            return (z, z)
        else:
            g, b = enc(mels.to(self.compute_dtype), mel_lens, max_mel_len)
        g, b = g.to(self.compute_dtype), b.to(self.compute_dtype)
        if ops.use_hip(g):  # fresh per forward, read only by FiLM LayerNorm sites: one shared gradient buffer (_FilmAcc)
            g._ssamd_film_acc = b._ssamd_film_acc = True
        return (g, b)

    # ------------------------------------------------------------------ forward
    def forward(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None,
                p_targets=None, e_targets=None, d_targets=None, p_control=1.0, e_control=1.0, d_control=1.0,
                style_weights=None, mel_lens_host=None, mels_style_only=False):
        """Reference ``model/fastspeech2.py:45-113``.  ``mel_lens_host`` (host int array of the
        batch's mel lengths, provided by the data pipeline) enables the packed decoder in training.

        ``mels_style_only`` (synthesis with ``d_targets``, ``infer/transfer.py``): ``mels`` / ``mel_lens`` /
        ``max_mel_len`` describe the style reference alone.  Without it they are also the teacher-forcing target:
        the length regulator pads or cuts to ``max_mel_len`` and the decoder runs at ``mel_lens``.  With it the
        result has ``sum(d_targets)`` frames whatever the reference's length."""
        dev = texts.device
        cd = self.compute_dtype
        if torch.is_grad_enabled() and ops.use_hip(texts):
            ps = self._film_param_list()
            if ps:  # the FiLM-L2 holder exists before the sites' forward (same hook pattern every step)
                from ..ops import gradslots

                gradslots.film_holder_for(ps)
        if mel_lens_host is None and mel_lens is not None:
            mel_lens_host = getattr(mel_lens, "host_lengths", None)
        if mels is not None and max_mel_len is None:
            max_mel_len = mels.shape[1]
        align = None
        if d_targets is None and (p_targets is not None or e_targets is not None):
            # teacher forcing without durations: they are learned (MAS over the aligner's lattice)
            align = self.learn_alignment(texts, src_lens, mels, mel_lens, mel_lens_host, p_targets, e_targets)
            d_targets, p_targets, e_targets = align["durations"], align["p_targets"], align["e_targets"]
        style = self.compute_style(mels, mel_lens, max_mel_len, texts.shape[0], dev, style_weights)
        x = self.encoder(texts, src_lens, style, cd)
        if self.speaker_emb is not None:
            if self.spker_embed_proj is None:  # table lookup fused into the add (one HIP kernel each way)
                x = ops.add_table_rows(x, self.speaker_emb.weight, speakers)
            else:
                spk = self.speaker_emb(speakers) + self.spker_embed_proj(self.spker_table[speakers])
                x = ops.add_rowvec(x, spk)
        training_lr = d_targets is not None and not mels_style_only
        packed = (self.training and training_lr and mel_lens is not None and mel_lens_host is not None
                  and max_mel_len is not None and self.variance_adaptor.packable())
        x, p_pred, e_pred, log_d, d_rounded, mel_lens_out = self.variance_adaptor(
            x, src_lens, None if mels_style_only else mel_lens, max_mel_len if training_lr else None, p_targets,
            e_targets, d_targets,
            p_control, e_control, d_control, style, regulate=not packed,
        )
        if packed:
            M = min(int(max_mel_len), self.decoder.max_seq_len)
            R = int(sum(min(int(v), M) for v in mel_lens_host))
            x, dec_lens, pk = self.decoder.forward_packed(x, d_targets, mel_lens, int(max_mel_len), R, style)
            mel = ops.linear(x, self.mel_linear.weight, self.mel_linear.bias).float()
            # padded frames: decoder output 0 -> mel_linear gives the bias there (reference semantics)
            mel = ops.unpack_rows(mel, pk, fill=self.mel_linear.bias)
        else:
            x, dec_lens = self.decoder(x, mel_lens_out, style)
            mel = ops.linear(x, self.mel_linear.weight, self.mel_linear.bias).float()
        post = self.postnet(mel.to(cd)).float() + mel
        src_masks = ops.lengths_to_mask(src_lens, texts.shape[1])
        mel_masks = ops.lengths_to_mask(dec_lens, mel.shape[1])
        out = (mel, post, p_pred, e_pred, log_d, d_rounded, src_masks, mel_masks, src_lens, mel_lens_out)
        # learned-duration mode only: the alignment terms travel as one extra element (FastSpeech2Loss reads it)
        return out if align is None else out + (align,)

    def learn_alignment(self, texts, src_lens, mels, mel_lens, mel_lens_host, p_targets, e_targets):
        """Teacher forcing from a batch without durations: the aligner's lattice lp [B, T, N] (differentiable: the
        forward-sum loss trains it), its MAS durations (no gradient; they sum to ``mel_lens``) and the frame-level
        pitch / energy contours averaged over each token's frames where the feature is phoneme-level.
        The keys read the phoneme embedding table without sending a gradient into it: the table is trained by the
        synthesis losses alone.
        -> {"lp", "t_lens", "n_lens", "durations", "p_targets", "e_targets"}"""
        if self.aligner is None:
            raise ValueError("the batch has mel / pitch / energy targets but no durations, and the model has no "
                             "aligner: add an `aligner:` block to model.yaml (config/LJSpeech_unaligned) or provide "
                             "durations")
        if mels is None or mel_lens is None:
            raise ValueError("learned durations need the target mel and its lengths")
        cd = self.compute_dtype
        emb = F.embedding(texts, self.encoder.src_word_emb.weight.detach()).to(cd)
        lp = self.aligner(mels.to(cd), mel_lens, emb, src_lens)
        t_lens = mel_lens
        if getattr(mel_lens, "host_lengths", None) is None and mel_lens_host is not None:
            t_lens = [int(v) for v in mel_lens_host]  # host lengths: the ops' checks need no device sync
        with torch.no_grad():
            dur = ops.align_mas(lp.detach(), t_lens, src_lens)
            va = self.variance_adaptor
            if p_targets is not None and va.pitch_feature_level == "phoneme_level":
                p_targets = ops.segment_mean(p_targets, dur)
            if e_targets is not None and va.energy_feature_level == "phoneme_level":
                e_targets = ops.segment_mean(e_targets, dur)
        return {"lp": lp, "t_lens": t_lens, "n_lens": src_lens, "durations": dur, "p_targets": p_targets,
                "e_targets": e_targets}

    def packed_inference_ok(self, texts) -> bool:
        return (not self.training and ops.use_hip(texts) and self.variance_adaptor.packable()
                and self.compute_dtype == torch.bfloat16)

    @torch.no_grad()
    def infer_packed(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None,
                     p_control=1.0, e_control=1.0, d_control=1.0, style_weights=None):
        """Synthesis with predicted durations, the length-regulated half on PACKED rows: the decoder, mel_linear
        and the PostNet run on the R = sum(mel lengths) valid frames only (``Decoder.forward_packed``,
        ``PostNet.forward_packed``) instead of B x max(mel length) padded rows -- at batch 256 of LJSpeech-like
        lengths ~45 % of the padded rows.  Each utterance's frames are exactly its batch-1 synthesis (every conv
        zero-pads at its own ends; the padded reference path lets the padded frames' mel_linear bias leak into the
        last PostNet frames of shorter utterances).  The one host sync is the same as the padded path's (the mel
        lengths, which size the length regulator): here all B lengths come back at once.
        Returns (post-net mel [R, n_mel] fp32 rows of utterance b at cu[b].., host lengths (list), device mel_len)."""
        front = self.infer_front(speakers, texts, src_lens, max_src_len, mels, mel_lens, max_mel_len, p_control,
                                 e_control, d_control, style_weights)
        lens = [int(v) for v in front[2].cpu().tolist()]  # the one D2H: sizes the packed decoder
        return self.infer_back(front, lens), lens, front[2]

    @torch.no_grad()
    def infer_front(self, speakers, texts, src_lens, max_src_len, mels=None, mel_lens=None, max_mel_len=None,
                    p_control=1.0, e_control=1.0, d_control=1.0, style_weights=None, exact_pad=False, *,
                    p_targets=None, e_targets=None, d_targets=None, return_preds=False):
        """``infer_packed`` up to the durations (no host sync, fixed shapes: HIP-graph capturable,
        ``infer/graphs.py``) -> (x [B, T, d], rounded durations [B, T], mel_len [B], style).

        ``p_targets`` / ``e_targets`` [B, T] (normalised, phoneme-level): embedded in place of the predictions;
        ``d_targets`` [B, T] integers: the durations and mel lengths are theirs (0 past ``src_lens``), the duration
        predictor's output is not used (the second pass of ``infer/transfer.py``).  ``return_preds``: also the
        pitch / energy predictions [B, T] (controls applied), as a fifth element (p_pred, e_pred).

        ``exact_pad``: for the ``pad_for_bucket`` inputs of a capacity run -- each row comes out as its unpadded
        text would (``VarianceAdaptor.forward``); the encoder already masks its pad rows."""
        cd = self.compute_dtype
        dev = texts.device
        if mels is not None and max_mel_len is None:
            max_mel_len = mels.shape[1]
        style = self.compute_style(mels, mel_lens, max_mel_len, texts.shape[0], dev, style_weights)
        x = self.encoder(texts, src_lens, style, cd)
        if self.speaker_emb is not None:
            if self.spker_embed_proj is None:
                x = ops.add_table_rows(x, self.speaker_emb.weight, speakers)
            else:
                spk = self.speaker_emb(speakers) + self.spker_embed_proj(self.spker_table[speakers])
                x = ops.add_rowvec(x, spk)
        x, p_pred, e_pred, log_d, _, _ = self.variance_adaptor(x, src_lens, None, None, p_targets, e_targets, None,
                                                               p_control, e_control, d_control, style, regulate=False,
                                                               exact_pad=exact_pad)
        if d_targets is not None:
            d_rounded = d_targets.long().clamp(min=0).masked_fill(ops.lengths_to_mask(src_lens, texts.shape[1]), 0)
            mel_len = d_rounded.sum(1)
        else:
            d_rounded, mel_len = ops.duration_round(log_d, src_lens, d_control)
        front = (x, d_rounded, mel_len, style)
        return front + ((p_pred, e_pred),) if return_preds else front

    @staticmethod
    def pad_text_bucket(T: int) -> int:
        """Text capacity of the bucketed synthesis graphs: T rounded up to a multiple of 16, at least 16."""
        return max(16, -(-int(T) // 16) * 16)

    @staticmethod
    @torch.no_grad()
    def pad_for_bucket(speakers, texts, src_lens, Tb, mels=None, mel_lens=None, style_weights=None, controls=()):
        """The B + 1-row inputs of a capacity run (``infer_front`` then ``infer_back(..., cap=)``): the B real rows
        padded to ``Tb`` phonemes with the pad id (``src_lens`` masks them as in any batch), plus the filler row --
        ONE phoneme (utterance 0's first), ``src_len`` 1, utterance 0's speaker, reference mel and style weights.  It
        becomes the sequence that takes up the capacity's unused frames.  Per-phoneme ``controls`` ([B, T] tensors)
        are padded with 1.0; scalars pass through.
        -> (speakers, texts, src_lens, mels, mel_lens, style_weights, controls)"""
        B, T = texts.shape
        assert T <= Tb, "pad_for_bucket: text longer than the bucket"
        tp = texts.new_zeros(B + 1, Tb)
        tp[:B, :T] = texts
        tp[B, 0] = texts[0, 0]
        sl = torch.cat([src_lens, src_lens.new_ones(1)])

        def first_again(t):
            return None if t is None else torch.cat([t, t[:1]])

        cs = []
        for c in controls:
            if isinstance(c, torch.Tensor) and c.dim() == 2:
                cp = c.new_ones(B + 1, Tb)
                cp[:B, : c.shape[1]] = c[:, :Tb]
                c = cp
            cs.append(c)
        return (first_again(speakers), tp, sl, first_again(mels), first_again(mel_lens),
                first_again(style_weights), tuple(cs))

    @torch.no_grad()
    def infer_back(self, front, lens, cap=None):
        """``infer_packed`` after the durations, for host mel lengths ``lens`` (fixed shapes given lens:
        capturable) -> post-net mel rows [R, n_mel] fp32.

        ``cap = (Rcap, Mcap)``: ``front`` is a ``pad_for_bucket`` front whose filler row has been sized on the device
        (``hip.VocPackCap.update``: the device mel lengths then sum to Rcap, none above Mcap); ``lens`` is ignored
        and the B + 1 sequences run at R = Rcap rows, M = Mcap frames -> [Rcap, n_mel]."""
        x, d_rounded, mel_len, style = front
        if cap is not None:
            R, M = int(cap[0]), int(cap[1])
        else:
            M, R = max(lens) if lens else 0, sum(lens)
        x, dec_lens, pk = self.decoder.forward_packed(x, d_rounded, mel_len, M, R, style)
        mel = ops.linear(x, self.mel_linear.weight, self.mel_linear.bias).float()
        post = self.postnet.forward_packed(mel.to(self.compute_dtype), pk).float() + mel
        return post.reshape(R, -1)
