"""The weight-stationary K = 256 GEMM (csrc/k_gemm.hip conv_gemm_k256_kernel) against the tile kernels it
replaces: every comparison is bitwise (``torch.equal``) between ``ssamd_gemm_set_k256(1)`` and ``(0)``, with the
skinny and split-K kernels off in both arms."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from speakingstyle_amd import experimental  # noqa: E402
from speakingstyle_amd.ops import hip  # noqa: E402
from speakingstyle_amd.ops import reference as ref  # noqa: E402

DEV = "cuda"
K = 256


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


@contextlib.contextmanager
def _tile_kernels_only():
    lib = hip.lib()
    lib.ssamd_gemm_set_splitk(0)
    lib.ssamd_gemm_set_skinny(0)
    try:
        yield lib
    finally:
        lib.ssamd_gemm_set_splitk(-1)
        lib.ssamd_gemm_set_skinny(1)
        lib.ssamd_gemm_set_k256(-1)
        lib.ssamd_gemm_set_k256_blocks(0)


def _both(lib, fn, blocks=0):
    """fn() with the streaming kernel off, then on (optionally with a grid cap)."""
    lib.ssamd_gemm_set_k256(0)
    lib.ssamd_gemm_set_k256_blocks(0)
    y0 = fn()
    lib.ssamd_gemm_set_k256(1)
    lib.ssamd_gemm_set_k256_blocks(blocks)
    y1 = fn()
    lib.ssamd_gemm_set_k256_blocks(0)
    return y0, y1


def _operands(M, N, Cin=K, ks=1, seed=0):
    g = torch.Generator(DEV).manual_seed(1000 * N + M + seed)
    x = (torch.randn(1, M, Cin, device=DEV, generator=g) / 16).to(torch.bfloat16)
    w = (torch.randn(N, ks, Cin, device=DEV, generator=g) / 16).to(torch.bfloat16)
    b = torch.randn(N, device=DEV, generator=g)
    return x, w, b


@pytest.mark.parametrize("N", [256, 768, 1024])
def test_k256_rows_and_widths(N):
    """Chunk edges, a ragged last chunk, fewer chunks than blocks; with and without bias; one fp32 anchor."""
    with _tile_kernels_only() as lib:
        for M in (1, 63, 64, 65, 255, 257, 1001, 4097):
            x, w, b = _operands(M, N)
            for bias in (None, b):
                y0, y1 = _both(lib, lambda: hip.conv_gemm_raw(x, w, bias, 1, M, K, 1, 1, 0, N, 0))
                assert torch.equal(y0, y1), (M, N, bias is not None)
            if N == 768 and M == 1001:
                yr = ref.conv1d(x.float(), w.float().permute(0, 2, 1), b, 0, 1, None)
                assert _rel(y1, yr) < 1e-2


@pytest.mark.parametrize("blocks", [2, 3])
def test_k256_many_chunks_per_block(blocks):
    """A capped grid: ring wrap-around, the steady state, unequal ranges, a block count the column groups
    do not divide."""
    with _tile_kernels_only() as lib:
        for M in (1001, 4097):
            for N in (256, 1024):
                x, w, b = _operands(M, N, seed=7)
                for bias in (None, b):
                    y0, y1 = _both(lib, lambda: hip.conv_gemm_raw(x, w, bias, 1, M, K, 1, 1, 0, N, 0), blocks)
                    assert torch.equal(y0, y1), (M, N, blocks, bias is not None)


def test_k256_bitmask_epilogue():
    """The ReLU-bitmask data gradient: equal to the tile kernel with mask_in and to the bf16-aux form."""
    M, N = 1001, 1024
    with _tile_kernels_only() as lib:
        x, w, _ = _operands(M, N, seed=3)
        g = torch.Generator(DEV).manual_seed(5)
        mask = torch.randint(0, 256, (M, N // 8), device=DEV, dtype=torch.uint8, generator=g)
        bits = ((mask.view(M, N // 8, 1).int() >> torch.arange(8, device=DEV)) & 1).view(1, M, N)
        h = bits.to(torch.bfloat16)  # a ReLU output that is positive exactly where the bit is set
        for blocks in (0, 2):
            y0, y1 = _both(lib, lambda: hip.conv_gemm_mask_raw(x, w, None, 1, M, K, 1, 0, N, 0, mask_in=mask), blocks)
            assert torch.equal(y0, y1), blocks
            assert torch.equal(y1, hip.conv_gemm_raw(x, w, None, 1, M, K, 1, 1, 0, N, 0, aux=h)), blocks


def test_k256_routing():
    """Shapes and epilogues the streaming kernel does not take run on the tile kernels, unchanged."""
    M = 1001
    with _tile_kernels_only() as lib:
        x5, w5, b5 = _operands(M, 256, Cin=512)
        x, w3, b = _operands(M, 256, ks=3)
        _, w320, b320 = _operands(M, 320)
        _, w, _ = _operands(M, 256)
        res = (torch.randn(1, M, 256, device=DEV) / 4).to(torch.bfloat16)
        B, L = 7, 143
        lens = torch.tensor([143, 100, 1, 77, 143, 50, 9], device=DEV, dtype=torch.int64)
        cases = {
            "K = 512": lambda: hip.conv_gemm_raw(x5, w5, b5, 1, M, 512, 1, 1, 0, 256, 0),
            "ks = 3": lambda: hip.conv_gemm_raw(x, w3, b, 1, M, K, 3, 1, 1, 256, 0),
            "N = 320": lambda: hip.conv_gemm_raw(x, w320, b320, 1, M, K, 1, 1, 0, 320, 0),
            "out_f32": lambda: hip.conv_gemm_raw(x, w, b, 1, M, K, 1, 1, 0, 256, 0, out_f32=True),
            "resid": lambda: hip.conv_gemm_raw(x, w, b, 1, M, K, 1, 1, 0, 256, 0, resid=res),
            "lens": lambda: hip.conv_gemm_raw(x, w, b, B, L, K, 1, 1, 0, 256, 0, lens=lens),
        }
        for name, fn in cases.items():
            y0, y1 = _both(lib, fn)
            assert torch.equal(y0, y1), name


def test_k256_fft_block_autograd():
    """One FFT block, forward and backward on packed rows: output, input gradient and every parameter
    gradient are bitwise the same with the streaming kernel on and off."""
    from speakingstyle_amd.models.layers import FFTBlock
    from speakingstyle_amd.ops.packing import PackInfo

    torch.manual_seed(11)
    blk = FFTBlock(256, 2, 128, 128, 1024, (9, 1), dropout=0.2, film=False).to(DEV).train()
    lens = torch.tensor([700, 512, 633, 580, 575], device=DEV)
    pk = PackInfo.build(lens, int(lens.max()), int(lens.sum()))
    x = torch.randn(1, pk.R, 256, device=DEV).to(torch.bfloat16)
    gout = torch.randn(1, pk.R, 256, device=DEV).to(torch.bfloat16)
    runs = []
    for mode in (0, 1):
        with experimental.overrides(gemm_k256=mode):
            hip.set_seed(1234)
            for p in blk.parameters():
                p.grad = None
            xi = x.clone().requires_grad_(True)
            y = blk(xi, lens, None, pk)
            y.backward(gout)
            torch.cuda.synchronize()
            runs.append([y.detach().clone(), xi.grad.clone()] + [p.grad.clone() for p in blk.parameters()])
    assert all(p.grad is not None for p in blk.parameters())
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_k256_non_default_stream():
    M, N = 4097, 768
    with _tile_kernels_only() as lib:
        x, w, b = _operands(M, N, seed=9)
        lib.ssamd_gemm_set_k256(1)
        y = hip.conv_gemm_raw(x, w, b, 1, M, K, 1, 1, 0, N, 0)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            ys = hip.conv_gemm_raw(x, w, b, 1, M, K, 1, 1, 0, N, 0)
        st.synchronize()
        assert torch.equal(y, ys)
