"""D=128 attention with sequence-to-XCD block placement (``attn_xcd``).

H=2, D=128, padded layout and packed rows, lengths that cross the 64-row tile and 128-row block
boundaries and leave whole blocks empty.  The default path and both values of ``attn_xcd`` (the
split dK / dV passes measured slower and were not kept, so there is no ``attn_kv_split`` arm) are
checked against ``ops.reference.attention`` in fp32 with the tolerances of
``test_attention_fwd_variants`` / ``test_attention_bwd_variants``; padded rows of the gradient are
exactly zero, the backward is bitwise reproducible, and placement changes no bit.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from speakingstyle_amd import experimental  # noqa: E402
from speakingstyle_amd.ops import hip, reference as ref  # noqa: E402
from speakingstyle_amd.ops.packing import PackInfo, pack, unpack  # noqa: E402

DEV = "cuda"
H, D = 2, 128
CASES = {"bh10": ([1, 63, 64, 65, 127], 127),  # B*H = 10: not a multiple of the 8 XCDs
         "bh8": ([128, 129, 150, 257], 257)}
ARMS = [None, 0, 1]  # None: the default path; else the value of attn_xcd


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@pytest.fixture(autouse=True, scope="module")
def _lib_loaded():
    assert hip.available(), "kernel library must be built and loadable on the GPU box"


@functools.lru_cache(maxsize=None)
def _inputs(case):
    lens_l, M = CASES[case]
    torch.manual_seed(31)
    lens = torch.tensor(lens_l, device=DEV)
    pk = PackInfo.build(lens, M, int(lens.sum()))
    qkv = torch.randn(len(lens_l), M, 3 * H * D, device=DEV).to(torch.bfloat16)
    g = torch.randn(len(lens_l), M, H * D, device=DEV).to(torch.bfloat16)
    qr = qkv.float().requires_grad_(True)
    orr = ref.attention(qr, lens, H)
    orr.backward(g.float())
    return lens, M, pk, qkv, g, orr.detach(), qr.grad


@functools.lru_cache(maxsize=None)
def _run(case, arm):
    """(o, grad, grad again) of the padded layout and of packed rows under one switch setting."""
    lens, M, pk, qkv, g, _, _ = _inputs(case)
    kw = {} if arm is None else {"attn_xcd": arm}
    out = {}
    with experimental.overrides(**kw):
        for name, x, gi, lens_arg, pki in (("padded", qkv, g, lens, None),
                                           ("packed", pack(qkv, pk).contiguous(), pack(g, pk).contiguous(), None, pk)):
            qh = x.clone().requires_grad_(True)
            o = hip.attention(qh, lens_arg, H, pki)
            g1, = torch.autograd.grad(o, qh, gi, retain_graph=True)
            g2, = torch.autograd.grad(o, qh, gi)
            out[name] = (o.detach(), g1, g2)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("arm", ARMS, ids=lambda a: "default" if a is None else f"xcd{a}")
@pytest.mark.parametrize("case", list(CASES))
def test_attention_xcd_vs_reference(case, arm):
    lens, M, pk, qkv, g, orr, gr = _inputs(case)
    res = _run(case, arm)
    pad_rows = torch.arange(M, device=DEV)[None, :] >= lens[:, None]  # [B, M]
    for layout in ("padded", "packed"):
        o, g1, g2 = res[layout]
        if layout == "packed":
            o, g1u = unpack(o, pk), unpack(g1, pk)
        else:
            g1u = g1
        fwd = _rel(o, orr)
        print(case, arm, layout, "fwd", fwd)
        assert fwd < 1e-2, (layout, fwd)
        for part in range(3):  # dQ, dK, dV
            sl = slice(part * H * D, (part + 1) * H * D)
            e = _rel(g1u[..., sl], gr[..., sl])
            print(case, arm, layout, "dQ dK dV".split()[part], e)
            assert e < 2e-2, (layout, part, e)
            if layout == "padded":  # rows >= len of every gradient slice are written as zeros
                assert (g1[..., sl][pad_rows] == 0).all(), (layout, part)
        assert torch.equal(g1, g2), layout  # fixed accumulation order: run-to-run bitwise stable


@pytest.mark.parametrize("case", list(CASES))
def test_attention_placement_changes_no_bit(case):
    off, on, dflt = _run(case, 0), _run(case, 1), _run(case, None)
    for layout in ("padded", "packed"):
        for other in (on, dflt):
            assert torch.equal(off[layout][0], other[layout][0]), layout
            assert torch.equal(off[layout][1], other[layout][1]), layout
