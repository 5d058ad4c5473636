"""csrc/k_align.hip against ``ops.reference`` in float64, at the lane, wave and block edges of the kernels.

Numerics convention (as for Griffin-Lim): the yardstick of a case is the float32 torch reference's own deviation from
the float64 reference on the same inputs, the maximum over 8 seeds with lp = log_softmax(3 randn); the kernels may
deviate from float64 by up to 8 times that (hardware exp / log are about 1 ulp against libm's 0.5, and the chain is
T deep).  Every comparison prints its figures (``ALIGNNUM`` lines) before it asserts.  The references of a case are
computed once and shared."""
import functools

import pytest
import torch

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

SEEDS = 8
MARGIN = 8.0
# (T, N): N in {1, 2, 63, 64, 65, 128, 129, 200} x T in {N, N + 1, 64, 65, 129, 300}
CASES = [(1, 1), (64, 1), (2, 2), (3, 2), (63, 63), (64, 63), (129, 63), (64, 64), (65, 64), (300, 64), (65, 65),
         (66, 65), (129, 65), (128, 128), (300, 128), (129, 129), (130, 129), (300, 129), (200, 200), (201, 200),
         (300, 200)]


def rand_lp(T, N, seeds=SEEDS):
    g = torch.Generator().manual_seed(1000 * T + N)
    return torch.log_softmax(3.0 * torch.randn(seeds, T, N, generator=g, dtype=torch.float64), -1).float()


def int_lp(T, N, seeds=2):
    g = torch.Generator().manual_seed(77 * T + N)
    return -torch.randint(0, 4, (seeds, T, N), generator=g).float()


def fsum(fn, lp, T, N):
    lp = lp.clone().requires_grad_(True)
    nll = fn(lp, [T] * lp.shape[0], [N] * lp.shape[0])
    (g,) = torch.autograd.grad(nll.sum(), lp)
    return nll.detach(), g


def path_score(lp64, dur):
    """float64 total of the path with durations ``dur`` [N] over lp64 [T, N]."""
    tok = torch.repeat_interleave(torch.arange(dur.shape[0]), dur.long())
    return float(lp64[torch.arange(tok.shape[0]), tok].sum())


@functools.lru_cache(maxsize=None)
def references(T, N):
    """float64 and float32 torch references of a case (8 seeds as one batch), and the MAS optimum."""
    lp = rand_lp(T, N)
    n64, g64 = fsum(ref.align_forward_sum, lp.double(), T, N)
    n32, g32 = fsum(ref.align_forward_sum, lp, T, N)
    tl, nl = [T] * SEEDS, [N] * SEEDS
    d64 = ref.align_mas(lp.double(), tl, nl)
    d32 = ref.align_mas(lp, tl, nl)
    best = [path_score(lp[s].double(), d64[s]) for s in range(SEEDS)]
    mas_dev = max(abs(path_score(lp[s].double(), d32[s]) - best[s]) for s in range(SEEDS))
    return {"lp": lp, "nll64": n64, "g64": g64, "nll_dev": float((n32.double() - n64).abs().max()),
            "post_dev": float((g32.double() - g64).abs().max()), "best": best, "mas_dev": mas_dev}


@pytest.mark.parametrize("T,N", CASES)
def test_forward_sum_against_float64(T, N):
    r = references(T, N)
    nll, g = fsum(ops.align_forward_sum, r["lp"].cuda(), T, N)
    nll_err = float((nll.cpu().double() - r["nll64"]).abs().max())
    post_err = float((g.cpu().double() - r["g64"]).abs().max())
    print(f"ALIGNNUM fsum T={T} N={N} |alpha|={float(r['nll64'].abs().max()):.1f} nll: ref32 {r['nll_dev']:.3e} "
          f"hip {nll_err:.3e}  posterior: ref32 {r['post_dev']:.3e} hip {post_err:.3e}")
    assert torch.isfinite(g).all()
    assert nll_err <= MARGIN * r["nll_dev"]
    assert post_err <= MARGIN * r["post_dev"]
    # every frame is on exactly one token, up to the posterior's own error
    assert float((-g.cpu().double().sum(2) - 1.0).abs().max()) <= max(N * MARGIN * r["post_dev"], 1e-6)


@pytest.mark.parametrize("T,N", CASES)
def test_mas_against_reference(T, N):
    r = references(T, N)
    tl, nl = [T] * SEEDS, [N] * SEEDS
    d = ops.align_mas(r["lp"].cuda(), tl, nl).cpu()
    assert d.dtype == torch.int32 and d.shape == (SEEDS, N)
    assert int(d.min()) >= 1 and (d.sum(1) == T).all()
    err = max(abs(path_score(r["lp"][s].double(), d[s]) - r["best"][s]) for s in range(SEEDS))
    print(f"ALIGNNUM mas T={T} N={N} float64 optimum - path score: ref32 {r['mas_dev']:.3e} hip {err:.3e}")
    assert err <= MARGIN * r["mas_dev"]
    # integer-valued scores are exact in fp32: the durations are the reference's, ties included
    ilp = int_lp(T, N)
    want = ref.align_mas(ilp.double(), [T, T], [N, N])
    assert torch.equal(ops.align_mas(ilp.cuda(), [T, T], [N, N]).cpu(), want)


BATCH = [(300, 200), (64, 63), (1, 1), (129, 65), (65, 64), (300, 129), (3, 2), (128, 128), (64, 1), (130, 129)]
TMAX, NMAX = 320, 208  # larger than every utterance of the batch


def mixed_batch(integer=False):
    g = torch.Generator().manual_seed(5)
    lp = 100.0 * torch.randn(len(BATCH), TMAX, NMAX, generator=g)  # padding holds anything
    for b, (T, N) in enumerate(BATCH):
        lp[b, :T, :N] = (int_lp(T, N) if integer else rand_lp(T, N))[0]
    return lp, [c[0] for c in BATCH], [c[1] for c in BATCH]


def test_mixed_batch_is_each_utterance_alone_and_repeatable():
    lp, tl, nl = mixed_batch()
    lpd = lp.cuda().requires_grad_(True)
    w = torch.linspace(-2.0, 3.0, len(BATCH)).cuda()
    nll = ops.align_forward_sum(lpd, tl, nl)
    (g,) = torch.autograd.grad((nll * w).sum(), lpd)
    nll2 = ops.align_forward_sum(lpd, torch.tensor(tl).cuda(), torch.tensor(nl).cuda())  # device lengths
    (g1,) = torch.autograd.grad(nll2.sum(), lpd)
    dur = ops.align_mas(lpd, tl, nl)
    assert torch.equal(nll, nll2) and torch.equal(dur, ops.align_mas(lpd.detach(), tl, nl))
    assert torch.equal(g, w.view(-1, 1, 1) * g1)  # the gradient scales with grad_nll
    for b, (T, N) in enumerate(BATCH):
        r = references(T, N)
        one = r["lp"][:1].cuda()
        n1, ga = fsum(ops.align_forward_sum, one, T, N)
        assert torch.equal(nll[b].detach(), n1[0])
        assert torch.equal(g1[b, :T, :N], ga[0])
        outside = g[b].clone()
        outside[:T, :N] = 0
        assert (outside == 0).all()  # exactly 0 outside the lattice
        d1 = ops.align_mas(one, [T], [N])
        assert torch.equal(dur[b, :N], d1[0]) and (dur[b, N:] == 0).all()
        assert abs(float(n1[0]) - float(r["nll64"][0])) <= MARGIN * r["nll_dev"]


def test_mixed_batch_integer_scores_match_reference():
    lp, tl, nl = mixed_batch(integer=True)
    assert torch.equal(ops.align_mas(lp.cuda(), tl, nl).cpu(), ref.align_mas(lp.double(), tl, nl))


def test_segment_mean_against_reference():
    g = torch.Generator().manual_seed(9)
    B, Tmax, Nmax = 5, 333, 130
    d = torch.zeros(B, Nmax, dtype=torch.int32)
    d[0, :129] = torch.randint(0, 5, (129,), generator=g, dtype=torch.int32)
    d[1, :64] = torch.randint(1, 6, (64,), generator=g, dtype=torch.int32)
    d[2, 0] = Tmax
    d[3, :65] = 1
    values = torch.randn(B, Tmax, generator=g)
    want = ref.segment_mean(values, d)
    got = ops.segment_mean(values.cuda(), d.cuda()).cpu()
    err = float((got - want).abs().max())
    print(f"ALIGNNUM segment_mean max |hip - reference| = {err:.3e}")
    # frames are added in order on both sides; the bound is the rounding of a run's sequential sum
    bound = (d.max(1).values.float() * 2.0 ** -24 * values.abs().max(1).values).unsqueeze(1)
    assert ((got - want).abs() <= bound).all()
    assert (got[4] == 0).all() and float(got[2, 0]) == pytest.approx(float(values[2].double().mean()), abs=1e-5)


def test_invalid_input_raises_on_the_host(monkeypatch):
    from speakingstyle_amd.ops import hip

    launched = []
    real = hip.lib()

    class Spy:
        def __getattr__(self, name):
            launched.append(name)
            return getattr(real, name)

    monkeypatch.setattr(hip, "lib", lambda: Spy())
    lp = torch.zeros(2, 4, 5, device="cuda")
    for fn in (ops.align_forward_sum, ops.align_mas):
        with pytest.raises(ValueError):
            fn(lp, [4, 3], [3, 4])  # T < N
        with pytest.raises(ValueError):
            fn(lp, [4, 3], [3, 0])  # N = 0
        with pytest.raises(ValueError):
            fn(torch.zeros(1, 1030, 1025, device="cuda"), [1030], [1025])  # Nmax > 1024
    assert not launched


def _rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm().clamp(min=1e-12))


def test_unaligned_training_step_hip_vs_reference():
    """One training step of ``LJSpeech_unaligned`` from a batch without durations: HIP bf16 (aligner convs, MAS,
    segment means, forward-sum loss and its backward through the kernels) against the torch fp32 reference backend
    on the same device.  Tolerances and the reference-sensitivity rule are those of
    ``test_kernels_gpu.py::test_model_step_hip_vs_reference``."""
    import copy

    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.models.loss import FastSpeech2Loss
    from speakingstyle_amd.train.optim import FlatArena

    dev = torch.device("cuda", 0)
    pp, mc, tc = load_named("LJSpeech_unaligned")
    mc["transformer"]["encoder_dropout"] = mc["transformer"]["decoder_dropout"] = 0.0
    mc["variance_predictor"]["dropout"] = 0.0
    torch.manual_seed(9)
    m = FastSpeech2(pp, mc).to(dev).train()
    m.postnet.dropout = 0.0
    mr = copy.deepcopy(m)
    m.set_compute_dtype(torch.bfloat16)
    arena = FlatArena(list(reversed(list(m.parameters()))), groups=m.fused_param_groups())
    b = SyntheticBatches(4, device=dev, seed=11, phone_counts=[40, 55, 61, 20], learned_durations=True).make_batch()
    assert b[11] is None
    lossf = FastSpeech2Loss(pp, tc)
    out = m(*b[2:])
    lo = lossf(b, out, m.film_scalars())
    lo[0].backward()
    arena.finalize_grads()
    assert len(out) == 11 and len(lo) == 8
    dur = out[5]
    assert torch.equal(dur.sum(1).long(), b[7]) and int(dur.min()) >= 0
    assert all(int(dur[i, :int(n)].min()) >= 1 for i, n in enumerate(b[4].tolist()))
    # integer-valued scores: the step's MAS durations are the same on both backends
    g = torch.Generator().manual_seed(3)
    ilp = -torch.randint(0, 4, tuple(out[10]["lp"].shape), generator=g).float().to(dev)
    d_hip = ops.align_mas(ilp, b[7], b[4])
    sens = {}
    mp = copy.deepcopy(mr)
    ops.set_backend("reference")
    try:
        assert torch.equal(ops.align_mas(ilp, b[7], b[4]), d_hip)
        outr = mr(*b[2:])
        lr_ = lossf(b, outr, mr.film_scalars())
        lr_[0].backward()
        # conditioning of the fp32 reference itself: the same step with every weight and the reference mel
        # perturbed by a relative 2^-9 (half a bf16 ulp)
        gp = torch.Generator(dev).manual_seed(5)
        with torch.no_grad():
            for q in mp.parameters():
                q.mul_(1 + 2 ** -9 * torch.randn(q.shape, device=dev, generator=gp).sign())
        bp = list(b)
        bp[6] = b[6] * (1 + 2 ** -9 * torch.randn(b[6].shape, device=dev, generator=gp).sign())
        lp_ = lossf(bp, mp(*bp[2:]), mp.film_scalars())
        lp_[0].backward()
        gpd = dict(mp.named_parameters())
        for n, q in mr.named_parameters():
            if q.grad is not None and q.grad.norm() > 1e-6 and gpd[n].grad is not None:
                sens[n] = _rel(gpd[n].grad, q.grad)
    finally:
        ops.set_backend(None)
    moved = int((dur != outr[5]).sum())
    print(f"ALIGNNUM step: MAS durations that differ between bf16 HIP and fp32 reference: {moved} of {dur.numel()}; "
          f"align loss hip {float(lo[7]):.6f} reference {float(lr_[7]):.6f}")
    assert _rel(out[1], outr[1]) < 3e-2
    for a, c in zip(lo[:6] + lo[7:], lr_[:6] + lr_[7:]):
        assert abs(a.item() - c.item()) <= 3e-2 * abs(c.item()) + 1e-3
    gr = dict(mr.named_parameters())
    bad, errs = [], []
    for n, p in m.named_parameters():
        if p.grad is None or gr[n].grad is None or p.numel() == 1:
            continue
        if gr[n].grad.norm() > 1e-6:
            e = _rel(p.grad, gr[n].grad)
            errs.append(min(e, 0.15) if sens.get(n, 0.0) > 0.075 else e)
            if e > max(0.15, 2.0 * sens.get(n, 0.0)):
                bad.append((n, e, sens.get(n)))
    assert any(n.startswith("aligner.") for n, p in m.named_parameters() if p.grad is not None)
    assert not bad, bad[:40]
    errs.sort()
    assert errs[len(errs) // 2] <= 0.03 and errs[int(0.9 * len(errs))] <= 0.08, (errs[len(errs) // 2],
                                                                                errs[int(0.9 * len(errs))])
