"""``ops.weights``: the weight generation and ``DerivedCache``, and the caches built on it -- a value derived from
weights is rebuilt after a raw write (one that torch's version counters do not see) once the generation is bumped."""
import gc

import torch

from speakingstyle_amd.ops import weights


def test_derived_cache_rebuilds_when_it_should():
    cache = weights.DerivedCache()
    a, b = torch.nn.Parameter(torch.randn(4, 3)), torch.randn(3)
    built = []

    def get(sources, extra=()):
        def build():
            assert not torch.is_grad_enabled()
            built.append(1)
            return len(built)

        return cache.get(a, sources, build, extra)

    assert cache.peek(a) is None
    assert [get((a, None)) for _ in range(3)] == [1, 1, 1] and cache.peek(a) == 1
    with torch.no_grad():
        a.add_(1.0)  # in place: _version moves
    assert get((a, None)) == 2 and get((a, None)) == 2
    weights.bump_generation()
    assert get((a, None)) == 3 and get((a, None)) == 3
    assert get((a, None), extra=torch.bfloat16) == 4 and get((a, None), extra=torch.bfloat16) == 4
    assert get((a, b), extra=torch.bfloat16) == 5 and get((a, b), extra=torch.bfloat16) == 5
    assert cache.peek(a) == 5 and len(built) == 5


def test_bump_generation_moves_the_generation():
    g = weights.generation()
    weights.bump_generation()
    assert weights.generation() == g + 1


def test_peek_is_none_once_the_anchor_is_gone():
    cache = weights.DerivedCache()
    a = torch.zeros(3)
    assert cache.peek(a) is None
    assert cache.get(a, (a,), lambda: "v") == "v" and cache.peek(a) == "v"
    del a
    gc.collect()
    # whatever tensor comes next (at the same address or not) is not the anchor the value was stored under
    assert all(cache.peek(t) is None for t in [torch.zeros(3) for _ in range(8)])


def _gst():
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.models.style import GlobalStyleTokens

    pp, mc, _ = load_named("BC2013_GST")
    torch.manual_seed(1)
    m = GlobalStyleTokens(pp, mc)
    for bn in m.bns:
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.data.uniform_(0.5, 1.5)
    return m.eval()


def test_gst_refolds_after_a_raw_write_and_a_bump():
    m = _gst()
    mel, lens = torch.randn(2, 32, 80), torch.tensor([32, 19])
    with torch.no_grad():
        first = m.reference_embedding(mel, lens)
        v = m.convs[1].weight._version
        m.convs[1].weight.data.mul_(0.5)  # as the optimizer writes: no version counter moves
        assert m.convs[1].weight._version == v
        weights.bump_generation()
        got = m.reference_embedding(mel, lens)
    ref = m.reference_embedding(mel, lens).detach()  # grad enabled: the conv + BatchNorm path, never cached
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
    assert not torch.allclose(got, first, rtol=1e-4, atol=1e-5)


def test_postnet_refolds_after_a_raw_write_and_a_bump():
    from speakingstyle_amd.models.layers import PostNet
    from speakingstyle_amd.ops.packing import PackInfo, pack, unpack

    torch.manual_seed(0)
    pn = PostNet(n_mel_channels=16, emb=32, k=5, n=5)
    for _, bn in pn.convolutions:
        bn.running_mean.uniform_(-0.5, 0.5)
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.data.uniform_(0.5, 1.5)
    pn.eval()
    lens, L = torch.tensor([11, 5]), 11
    x = torch.randn(2, L, 16)
    pk = PackInfo.build(lens, L, int(lens.sum()))

    def unfolded():  # each utterance alone through conv + eval BatchNorm
        return [pn(x[b:b + 1, : int(lens[b])]).squeeze(0) for b in range(2)]

    with torch.no_grad():
        first = unpack(pn.forward_packed(pack(x, pk), pk), pk)
        w = pn.convolutions[2][0].conv.weight
        v = w._version
        w.data.mul_(0.5)
        assert w._version == v
        weights.bump_generation()
        got = unpack(pn.forward_packed(pack(x, pk), pk), pk)
        ref = unfolded()
    for b in range(2):
        n = int(lens[b])
        torch.testing.assert_close(got[b, :n], ref[b], rtol=1e-5, atol=1e-5)
    assert not torch.allclose(got, first, rtol=1e-4, atol=1e-5)
    assert "_fold" not in pn.state_dict() and "_fold" not in pn.__dict__


def test_positional_rows_two_dtypes_from_one_table():
    from speakingstyle_amd.models.fastspeech2 import positional_rows

    pe = torch.nn.Parameter(torch.randn(1, 10, 4), requires_grad=False)
    for dtype, L in ((torch.bfloat16, 5), (torch.float16, 7), (torch.bfloat16, 3), (torch.float64, 10)):
        rows = positional_rows(pe, L, 4, "cpu", dtype)
        assert rows.dtype == dtype and torch.equal(rows, pe[0, :L].to(dtype))
