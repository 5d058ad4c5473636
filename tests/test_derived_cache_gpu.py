"""Values derived from weights follow a raw write (one torch's version counters do not see, as the fused Adam step
makes) once the weight generation is bumped; the tile heights follow the ResBlock tile mode."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from speakingstyle_amd.ops import hip  # noqa: E402

DEV = "cuda"


def _rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).norm() / (b.float().cpu().norm() + 1e-12)).item()


def test_gst_refolds_on_device_after_a_raw_write_and_a_bump():
    """In-training validation: eval + no_grad takes the folded convs; after the optimizer has written the weights
    the embedding is that of the new weights (against the fp32 CPU module carrying the same weights)."""
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.models.style import GlobalStyleTokens

    pp, mc, _ = load_named("BC2013_GST")
    torch.manual_seed(5)
    cpu = GlobalStyleTokens(pp, mc)
    for bn in cpu.bns:
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 2.0)
    cpu.eval()
    gpu = copy.deepcopy(cpu).to(DEV)
    mel = torch.randn(2, 32, 80).to(torch.bfloat16)
    lens = torch.tensor([32, 19])
    with torch.no_grad():
        first = gpu.reference_embedding(mel.to(DEV), lens.to(DEV))
        for m in (cpu, gpu):
            v = m.convs[1].weight._version
            m.convs[1].weight.data.mul_(0.5)
            assert m.convs[1].weight._version == v
        hip.bump_weight_generation()
        got = gpu.reference_embedding(mel.to(DEV), lens.to(DEV))
        ref = cpu.reference_embedding(mel.float(), lens)
    print("rel to the CPU module:", _rel(got, ref), "rel of the stale embedding:", _rel(first, ref))
    assert _rel(got, ref) < 3e-2
    assert not torch.equal(got, first)


def test_projection_group_outside_an_arena_follows_a_raw_write_and_a_bump():
    """The cached concatenation of a Q/K/V group is rebuilt: bitwise the GEMM on a fresh concatenation (same kernel,
    same operands)."""
    torch.manual_seed(6)
    ws = [torch.nn.Parameter(torch.randn(64, 64, device=DEV) / 8) for _ in range(3)]
    bs = [torch.nn.Parameter(torch.randn(64, device=DEV)) for _ in range(3)]
    x = torch.randn(1, 8, 64, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        first = hip.linear_group(x, ws, bs)
        assert torch.equal(first, hip.linear(x, torch.cat(ws, 0), torch.cat(bs, 0)))
        v = ws[1]._version
        ws[1].data.mul_(-0.5)
        assert ws[1]._version == v
        hip.bump_weight_generation()
        got = hip.linear_group(x, ws, bs)
        ref = hip.linear(x, torch.cat(ws, 0), torch.cat(bs, 0))
    assert got.shape == (1, 8, 192) and torch.equal(got, ref)
    assert torch.equal(got[..., :64], first[..., :64]) and not torch.equal(got[..., 64:128], first[..., 64:128])


def test_tile_heights_follow_the_resblock_tile_mode():
    """C = 256 has no half-tall instance (one height in every mode); C = 128, K = 7 has: 4 waves' 128 staged rows
    against 8 waves' 256, so its kind-3 height must change with the mode."""
    seen = {}
    try:
        for mode in (2, 0):
            hip.set_resblock_tall(mode)
            for C, K in ((256, 3), (128, 7)):
                seen[mode, C] = hip.voc_tile_rows(3, C, K)
                assert seen[mode, C] == hip.lib().ssamd_voc_tile_rows(3, C, K, 0, 0, 0) > 0
    finally:
        hip.set_resblock_tall(1)  # the production tile
    assert seen[2, 128] != seen[0, 128]
    assert hip.voc_tile_rows(3, 256, 3) == hip.lib().ssamd_voc_tile_rows(3, 256, 3, 0, 0, 0)
