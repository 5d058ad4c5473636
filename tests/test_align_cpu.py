"""``ops.reference.align_forward_sum`` / ``align_mas`` / ``segment_mean`` (the CPU path and the oracle of
csrc/k_align.hip): brute force over every monotone alignment, the closed-form gradient against autograd through that
enumeration, the stay-wins tie rule, batching; and the aligner inside the model on the reference backend."""
import itertools

import numpy as np
import pytest
import torch

from speakingstyle_amd import ops
from speakingstyle_amd.ops import reference as ref


def all_paths(T, N):
    """Every monotone alignment of T frames to N tokens as a token index per frame: starts at 0, ends at N - 1,
    stays or advances by one."""
    out = []
    for cuts in itertools.combinations(range(1, T), N - 1):  # the frames at which the path advances
        tok, n = [], 0
        for t in range(T):
            if t in cuts:
                n += 1
            tok.append(n)
        out.append(tok)
    return out


def brute_nll(lp):
    T, N = lp.shape
    scores = torch.stack([lp[torch.arange(T), torch.tensor(p)].sum() for p in all_paths(T, N)])
    return -torch.logsumexp(scores, 0)


def rand_lp(T, N, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.log_softmax(3.0 * torch.randn(T, N, generator=g, dtype=torch.float64), -1).to(dtype)


def int_lp(T, N, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return -torch.randint(0, 4, (T, N), generator=g).to(dtype)


SHAPES = [(1, 1), (2, 1), (2, 2), (5, 5), (9, 1), (9, 2), (9, 4), (8, 7), (7, 3), (6, 5)]


@pytest.mark.parametrize("T,N", SHAPES)
def test_forward_sum_against_brute_force(T, N):
    lp = rand_lp(T, N, 100 * T + N).requires_grad_(True)
    nll = ref.align_forward_sum(lp.unsqueeze(0), [T], [N])
    want = brute_nll(lp)
    assert nll.shape == (1,) and nll.dtype == torch.float64
    assert abs(nll[0].item() - want.item()) <= 1e-12 * max(1.0, abs(want.item()))
    (g,) = torch.autograd.grad(nll.sum(), lp)
    (gw,) = torch.autograd.grad(want, lp)
    assert torch.isfinite(g).all()
    assert float((g - gw).abs().max()) <= 1e-12
    # minus the path posterior: every frame is on exactly one token
    assert float((-g.sum(1) - 1.0).abs().max()) <= 1e-12
    # unreachable cells are exactly 0
    t, n = torch.arange(T).unsqueeze(1), torch.arange(N).unsqueeze(0)
    unreachable = (n > t) | ((N - 1 - n) > (T - 1 - t))
    assert (g[unreachable] == 0).all()


def test_forward_sum_single_path_and_single_token():
    lp = rand_lp(5, 5, 1)
    assert float(ref.align_forward_sum(lp.unsqueeze(0), [5], [5])[0]) == pytest.approx(-float(lp.diagonal().sum()), abs=1e-12)
    lp = rand_lp(9, 1, 2) - 0.3
    assert float(ref.align_forward_sum(lp.unsqueeze(0), [9], [1])[0]) == pytest.approx(-float(lp.sum()), abs=1e-12)
    lp = rand_lp(1, 1, 3) - 0.7
    assert float(ref.align_forward_sum(lp.unsqueeze(0), [1], [1])[0]) == -float(lp[0, 0])


def test_forward_sum_gradient_scales_with_grad_nll():
    lp = rand_lp(7, 3, 5).unsqueeze(0).repeat(2, 1, 1).requires_grad_(True)
    nll = ref.align_forward_sum(lp, [7, 7], [3, 3])
    (g,) = torch.autograd.grad((nll * torch.tensor([1.0, -2.5], dtype=torch.float64)).sum(), lp)
    assert torch.equal(g[1], -2.5 * g[0])


def test_invalid_lengths_raise():
    lp = torch.zeros(2, 4, 5)
    for fn in (ref.align_forward_sum, ref.align_mas, ops.align_forward_sum, ops.align_mas):
        with pytest.raises(ValueError):
            fn(lp, [4, 3], [3, 4])  # T < N
        with pytest.raises(ValueError):
            fn(lp, [4, 3], [3, 0])  # no tokens
        with pytest.raises(ValueError):
            fn(lp, [4, 5], [3, 3])  # longer than the lattice
        with pytest.raises(ValueError):
            fn(lp, [4], [3])
        with pytest.raises(ValueError):
            fn(torch.zeros(1, 1100, 1025), [1100], [1025])


def brute_mas(lp):
    """Durations of the best path in float64; among equal scores the path that stays longest at the latest frames'
    decisions -- the stay-wins rule applied from the end backwards."""
    T, N = lp.shape
    best, best_s = None, None
    for p in all_paths(T, N):
        s = float(lp[torch.arange(T), torch.tensor(p)].double().sum())
        if best is None or s > best_s:
            best, best_s = [p], s
        elif s == best_s:
            best.append(p)
    return best, best_s


def durations_of(path, N):
    return np.bincount(np.asarray(path), minlength=N)


@pytest.mark.parametrize("T,N", SHAPES)
def test_mas_against_brute_force(T, N):
    lp = rand_lp(T, N, 7 * T + N)
    d = ref.align_mas(lp.unsqueeze(0), [T], [N])
    assert d.dtype == torch.int32 and d.shape == (1, N)
    best, _ = brute_mas(lp)
    assert len(best) == 1
    assert d[0].tolist() == durations_of(best[0], N).tolist()


@pytest.mark.parametrize("T,N", [(6, 3), (9, 4), (8, 7), (9, 2)])
def test_mas_integer_scores_tie_rule(T, N):
    for seed in range(6):
        lp = int_lp(T, N, seed)
        d32 = ref.align_mas(lp.unsqueeze(0), [T], [N])
        d64 = ref.align_mas(lp.double().unsqueeze(0), [T], [N])
        assert torch.equal(d32, d64)
        assert int(d32.min()) >= 1 and int(d32.sum()) == T
        best, _ = brute_mas(lp)
        # stay wins: walking back from the end, the chosen path stays on its token wherever an equally good path
        # does, i.e. it is the tied path whose token index is largest at the latest frame where the tied paths differ
        want = max(best, key=lambda p: p[::-1])
        assert d32[0].tolist() == durations_of(want, N).tolist()


def test_mas_all_equal_scores():
    # every path ties: stay wins everywhere, so the path advances as early as it can only where it must
    d = ref.align_mas(torch.zeros(1, 7, 3), [7], [3])
    assert d[0].tolist() == [1, 1, 5]


def mixed_batch(dtype=torch.float32, integer=False):
    shapes = [(9, 4), (5, 5), (12, 1), (7, 6), (3, 2)]
    Tmax, Nmax = 14, 8  # larger than every utterance
    g = torch.Generator().manual_seed(11)
    lp = torch.randn(len(shapes), Tmax, Nmax, generator=g).to(dtype)  # padding holds anything
    singles = []
    for b, (T, N) in enumerate(shapes):
        one = int_lp(T, N, b, dtype) if integer else rand_lp(T, N, b, dtype)
        lp[b, :T, :N] = one
        singles.append(one)
    return shapes, lp, singles


def test_mixed_batch_equals_each_alone():
    shapes, lp, singles = mixed_batch()
    tl, nl = [s[0] for s in shapes], [s[1] for s in shapes]
    lpg = lp.clone().requires_grad_(True)
    nll = ops.align_forward_sum(lpg, tl, nl)
    w = torch.arange(1, len(shapes) + 1, dtype=torch.float32)
    (g,) = torch.autograd.grad((nll * w).sum(), lpg)
    dur = ops.align_mas(lp, torch.tensor(tl), torch.tensor(nl))
    for b, ((T, N), one) in enumerate(zip(shapes, singles)):
        o = one.clone().unsqueeze(0).requires_grad_(True)
        n1 = ref.align_forward_sum(o, [T], [N])
        (g1,) = torch.autograd.grad(n1.sum() * w[b], o)
        assert torch.equal(nll[b], n1[0])
        assert torch.equal(g[b, :T, :N], g1[0])
        outside = g[b].clone()
        outside[:T, :N] = 0
        assert (outside == 0).all()
        d1 = ref.align_mas(one.unsqueeze(0), [T], [N])
        assert torch.equal(dur[b, :N], d1[0]) and (dur[b, N:] == 0).all()
        assert int(dur[b].sum()) == T and int(dur[b, :N].min()) >= 1


def test_segment_mean_against_phoneme_average():
    from speakingstyle_amd.data.preprocess import phoneme_average

    g = torch.Generator().manual_seed(3)
    durs = [[3, 1, 0, 4, 2], [1, 1, 1, 1, 1, 1, 1], [10], [0, 0, 5]]
    Tmax, Nmax = 13, 8
    values = torch.randn(len(durs), Tmax, generator=g)
    d = torch.zeros(len(durs), Nmax, dtype=torch.int32)
    for b, row in enumerate(durs):
        d[b, :len(row)] = torch.tensor(row, dtype=torch.int32)
    out = ops.segment_mean(values, d)
    assert out.shape == (len(durs), Nmax) and out.dtype == torch.float32
    for b, row in enumerate(durs):
        want = phoneme_average(values[b].double().numpy(), row)
        assert np.abs(out[b, :len(row)].numpy() - want).max() <= 4 * 2.0 ** -24 * max(1.0, np.abs(want).max()) * max(row)
        assert (out[b, len(row):] == 0).all()


# ------------------------------------------------------------------ the aligner inside the model
def unaligned_setup(seed=0):
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.data.synthetic import SyntheticBatches
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2
    from speakingstyle_amd.models.loss import FastSpeech2Loss

    pre, mc, tr = load_named("LJSpeech_unaligned")
    assert pre["preprocessing"]["duration"]["source"] == "learned" and tr["loss"]["lambda_align"] == 1.0
    mc["transformer"].update(encoder_layer=1, decoder_layer=1, encoder_hidden=32, decoder_hidden=32, encoder_head=2,
                             decoder_head=2, conv_filter_size=64)
    mc["variance_predictor"]["filter_size"] = 32
    mc["aligner"]["hidden"] = 32
    torch.manual_seed(seed)
    model = FastSpeech2(pre, mc)
    loss = FastSpeech2Loss(pre, tr)
    batch = SyntheticBatches(3, seed=seed, phone_counts=[12, 9, 5], frames_per_phone=4.0,
                             learned_durations=True).make_batch()
    return model, loss, batch


def test_unaligned_config_forward_backward():
    model, loss, batch = unaligned_setup()
    assert batch[11] is None  # no durations in this mode
    model.train()
    out = model(*batch[2:])
    assert len(out) == 11
    dur = out[5]
    assert dur.dtype == torch.int32
    assert torch.equal(dur.sum(1).long(), batch[7].long())  # the durations sum to the mel lengths
    assert batch[9].shape == batch[6].shape[:2]  # frame-level contours in the batch ...
    assert out[10]["p_targets"].shape == dur.shape  # ... phoneme-level targets from the MAS durations
    src_lens = batch[4]
    for b in range(dur.shape[0]):
        assert int(dur[b, :int(src_lens[b])].min()) >= 1 and int(dur[b, int(src_lens[b]):].sum()) == 0
    losses = loss(batch, out)
    assert len(losses) == 8
    assert all(torch.isfinite(torch.as_tensor(v)).all() for v in losses)
    losses[0].backward()
    grads = {n: p.grad for n, p in model.named_parameters() if n.startswith("aligner.")}
    assert grads and all(g is not None and torch.isfinite(g).all() for g in grads.values())
    assert any(float(g.abs().max()) > 0 for g in grads.values())


def test_model_without_aligner_keeps_its_keys_and_needs_durations():
    from speakingstyle_amd.config import load_named
    from speakingstyle_amd.models.fastspeech2 import FastSpeech2

    pre, mc, _ = load_named("LJSpeech")
    pre_u, mc_u, _ = load_named("LJSpeech_unaligned")
    for c in (mc, mc_u):
        c["transformer"].update(encoder_layer=1, decoder_layer=1)
    plain = FastSpeech2(pre, mc)
    with_al = FastSpeech2(pre_u, mc_u)
    keys = set(plain.state_dict())
    assert not any(k.startswith("aligner.") for k in keys)
    extra = set(with_al.state_dict()) - keys
    assert extra and all(k.startswith("aligner.") for k in extra)
    assert keys <= set(with_al.state_dict())
    _, _, batch = unaligned_setup()
    pre, mc, _ = load_named("LJSpeech")
    mc["transformer"].update(encoder_layer=1, decoder_layer=1)
    with pytest.raises(ValueError):
        FastSpeech2(pre, mc).train()(*batch[2:])  # mel targets but no durations and no aligner


def test_alignment_loss_falls():
    model, loss, batch = unaligned_setup(seed=1)
    model.train()
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    history = []
    for _ in range(20):
        opt.zero_grad()
        losses = loss(batch, model(*batch[2:]))
        history.append(losses[7].item())
        losses[0].backward()
        opt.step()
    assert history[-1] < history[0]
