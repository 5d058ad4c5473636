"""Bucketed synthesis graphs, host side: the capacity ladder and the numpy reference of the device table kernel
(``hip.cap_tables_host``) against the exact-length ``hip.VocPack`` tables of the same sequences + the filler."""
import os

import numpy as np
import pytest
import torch

from speakingstyle_amd.ops import hip

CASES = [[37], [64], [1], [5, 9, 1], [63], [200, 311]]  # [63]: F = 1; [64]: a whole number of 64-row tiles
RATE_TILES = [(rate, bm) for rate in (1, 8, 256) for bm in (64, 128, 256)]


def test_ladder_is_monotone_and_covers():
    prev = 0
    for n in range(1, 3000):
        c = hip.cap_ceil(n)
        assert c >= n and c >= prev
        step = 64 if c <= 1024 else 128
        assert c - n < step and c % step == 0, (n, c)
        prev = c
    assert [hip.cap_ceil(v) for v in (1, 64, 65, 512, 513, 1024, 1025)] == [64, 64, 128, 512, 576, 1024, 1152]


@pytest.mark.parametrize("lens", CASES + [[511], [512], [1023, 1], [8] * 8])
def test_bucket_holds_the_utterances_and_the_filler(lens):
    rcap, mcap = hip.cap_bucket(lens)
    F = rcap - sum(lens)
    assert rcap >= sum(lens) + 1 and F >= 1
    assert mcap >= F and mcap >= max(lens)
    assert rcap == hip.cap_ceil(sum(lens) + 1) and mcap == hip.cap_ceil(max(max(lens), F))
    canon = hip.cap_lens(len(lens), rcap)
    assert len(canon) == len(lens) + 1 and sum(canon) == rcap and min(canon) >= 1


@pytest.mark.parametrize("lens", CASES)
def test_cap_tables_host_equals_vocpack_plus_null_tiles(lens):
    rcap, mcap = hip.cap_bucket(lens)
    F = rcap - sum(lens)
    geoms, words = hip.cap_geoms(len(lens), rcap, RATE_TILES)
    assert len(geoms) == len(RATE_TILES)
    got_lens, cu, tabs = hip.cap_tables_host(lens, rcap, geoms, mcap)
    assert got_lens.tolist() == lens + [F]
    vp = hip.VocPack(lens + [F], torch.device("cpu"), RATE_TILES)
    assert cu.tolist() == vp.cu.tolist() and cu[-1] == rcap
    end = len(lens) + 2
    for rate, bm, n_cap, off in geoms:
        assert off >= end and off % 4 == 0  # tables behind cu, 16-byte aligned, back to back
        end = off + 4 * n_cap
        tt, n = vp.tiles(rate, bm)
        assert n <= n_cap == -(-rcap * rate // bm) + len(lens)  # the bound: never exceeded
        tab = tabs[(rate, bm)]
        assert tab.shape == (n_cap, 4) and tab.dtype == np.int32
        assert np.array_equal(tab[:n], tt.numpy().reshape(n, 4))  # real tiles first, in VocPack order
        assert not tab[n:].any()  # the rest: null tiles
    assert end == words


def test_cap_tables_host_clamps_a_wrong_bucket():
    """Lengths that do not fit the capacity the host chose: nothing may point past Rcap rows or Mcap frames."""
    geoms, _ = hip.cap_geoms(3, 64, [(1, 64), (256, 128)])
    for lens in ([100, 50, 7], [40, 40, 40], [-5, 70, 0], [63, 63, 63]):
        got, cu, tabs = hip.cap_tables_host(lens, 64, geoms, 32)
        assert (got >= 0).all() and (got <= 32).all() and got[-1] >= 1 and cu[-1] <= 64
        for (rate, bm), tab in tabs.items():
            assert ((tab[:, 0] + tab[:, 1]) <= 64 * rate).all() and (tab[:, 2] < np.maximum(tab[:, 1], 1)).all()
            assert (tab[:, 1] <= 32 * rate).all() and (tab[:, 3] <= 3).all()


def _small_model():
    import math

    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2

    pp, mc, tc = load_named("BC2013_GST")
    mc["transformer"]["encoder_layer"] = 2
    mc["transformer"]["decoder_layer"] = 2
    torch.manual_seed(0)
    model = FastSpeech2(pp, mc)
    with torch.no_grad():
        lin = model.variance_adaptor.duration_predictor.linear_layer
        lin.weight.normal_(0.0, 0.005)
        lin.bias.fill_(math.log(4.0))
    model.eval().requires_grad_(False)
    return (pp, mc, tc), model


def test_padded_front_equals_unpadded_text():
    """``pad_for_bucket`` + ``infer_front(exact_pad=True)`` (reference ops, fp32): every real row gets the durations
    and the encoder rows of its unpadded text; without ``exact_pad`` the pad rows reach the last phonemes."""
    _, model = _small_model()
    rng = np.random.default_rng(0)
    Ts = [5, 11, 8]
    texts = torch.zeros(3, 11, dtype=torch.int64)
    for i, n in enumerate(Ts):
        texts[i, :n] = torch.from_numpy(rng.integers(1, 300, size=n))
    speakers, src_lens = torch.zeros(3, dtype=torch.int64), torch.tensor(Ts)
    sw = torch.softmax(torch.randn(3, model.gst.embed.shape[0]), -1)  # one weight per style token
    Tb = model.pad_text_bucket(11)
    assert Tb == 16 and model.pad_text_bucket(16) == 16 and model.pad_text_bucket(17) == 32
    sp, tp, sl, _, _, swp, _ = model.pad_for_bucket(speakers, texts, src_lens, Tb, style_weights=sw)
    assert tp.shape == (4, 16) and sl.tolist() == Ts + [1] and tp[3].tolist() == [int(texts[0, 0])] + [0] * 15
    x, d, ml, _ = model.infer_front(sp, tp, sl, Tb, style_weights=swp, exact_pad=True)
    for i, n in enumerate(Ts):
        x1, d1, ml1, _ = model.infer_front(speakers[i:i + 1], texts[i:i + 1, :n], src_lens[i:i + 1], n,
                                           style_weights=sw[i:i + 1])
        assert d[i, :n].tolist() == d1[0].tolist() and not d[i, n:].any() and int(ml[i]) == int(ml1[0])
        assert torch.allclose(x[i, :n], x1[0], atol=1e-4, rtol=1e-4)
    # the reference semantics of a padded batch (no exact_pad): the speaker / pitch embedding of the pad rows reaches
    # the last phonemes through the k = 3 predictor convs
    x_leak = model.infer_front(sp, tp, sl, Tb, style_weights=swp)[0]
    assert not torch.allclose(x_leak[0, :5], x[0, :5], atol=1e-4, rtol=1e-4)


def test_synthesizer_on_cpu(tmp_path):
    """``Synthesizer.tts`` on the CPU: the single-mode ``synthesize`` path, int16 samples of mel length * hop."""
    from speakingstyle_amd.infer.serve import Synthesizer
    from speakingstyle_amd.models.hifigan import Generator, default_config
    from speakingstyle_amd.utils.model import ROOT

    configs, model = _small_model()
    for k, v in configs[0]["path"].items():
        if isinstance(v, str) and not os.path.isabs(v):
            configs[0]["path"][k] = os.path.join(ROOT, v)
    torch.manual_seed(1)
    h = default_config()
    h["upsample_initial_channel"] = 64  # a narrow HiFi-GAN (same hop): the CPU generator is slow at full width
    g = Generator(h).eval().fold_weight_norm()
    s = Synthesizer(configs, device="cpu", model=model, vocoder=g)
    assert s.graphs is None and s.stats is None
    wav = s.tts("Hi.")
    assert wav.dtype == np.int16 and wav.ndim == 1 and wav.size > 0 and wav.size % s.hop == 0
    slow = s.tts("Hi.", duration_control=2.0)
    assert slow.size > wav.size
