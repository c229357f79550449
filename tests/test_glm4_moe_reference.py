"""The definitions behind GLM-4.5 checkpoints (dmcp/ops/reference.py), in fp64
on the CPU: the sigmoid router against a literal transcription of the
checkpoint's own router with one expert group, the identity that lets a shared
MLP of width S * I ride as S always-chosen experts of width I, and the head
permutation that turns a partial rotary embedding into a whole-head one."""
import pytest
import torch

from dmcp.ops import reference as R


def _hf_router(h, weight, bias, top_k, norm_topk, scale, n_group=1, topk_group=1):
    """``Glm4MoeTopkRouter.forward``, statement for statement (fp64 in place of fp32)."""
    E = weight.shape[0]
    router_logits = torch.nn.functional.linear(h, weight)
    scores = router_logits.sigmoid()
    scores_for_choice = scores + bias
    group_scores = scores_for_choice.view(-1, n_group, E // n_group).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(-1, n_group, E // n_group).reshape(-1, E)
    scores_for_choice = scores_for_choice.masked_fill(~score_mask.bool(), float("-inf"))
    topk_indices = torch.topk(scores_for_choice, k=top_k, dim=-1, sorted=False)[1]
    topk_weights = scores.gather(1, topk_indices)
    if norm_topk:
        topk_weights = topk_weights / (topk_weights.sum(dim=-1, keepdim=True) + 1e-20)
    return topk_weights * scale, topk_indices


@pytest.mark.parametrize("E,k,norm,scale,seed", [(8, 2, True, 1.0, 1), (16, 4, False, 2.5, 2), (160, 8, True, 2.5, 3),
                                                 (8, 8, True, 1.0, 4), (8, 1, False, 0.5, 5)])
def test_router_is_the_checkpoints_own(E, k, norm, scale, seed):
    g = torch.Generator().manual_seed(seed)
    T, H = 200, 64
    h = torch.randn(T, H, generator=g, dtype=torch.float64)
    w = torch.randn(E, H, generator=g, dtype=torch.float64) / H ** 0.5
    bias = 0.5 * torch.randn(E, generator=g, dtype=torch.float64)
    ids, p = R.moe_route_sig_math(h, w, bias, k, norm, scale)
    hw, hi = _hf_router(h, w, bias, k, norm, scale)
    # the same (expert, weight) pairs; the checkpoint's code leaves the order open (sorted=False)
    dense = torch.zeros(T, E, dtype=torch.float64).scatter_(1, ids, p)
    dense_hf = torch.zeros(T, E, dtype=torch.float64).scatter_(1, hi, hw)
    assert torch.equal(ids.sort(1).values, hi.sort(1).values)
    assert torch.allclose(dense, dense_hf, rtol=1e-13, atol=0)
    # rank order: descending selection score
    sel = (torch.sigmoid(h @ w.t()) + bias).gather(1, ids)
    assert bool((sel[:, :-1] >= sel[:, 1:]).all())
    if k < E:
        # the bias decides: without it another set is chosen on at least a quarter of the rows
        plain = R.moe_route_sig_math(h, w, torch.zeros(E, dtype=torch.float64), k, norm, scale)[0]
        changed = (plain.sort(1).values != ids.sort(1).values).any(1).float().mean().item()
        assert changed >= 0.25, changed
    if norm:
        assert torch.allclose(p.sum(1), torch.full((T,), scale, dtype=torch.float64), rtol=1e-12)
    # the shared pseudo-experts: (E + s, 1.0) behind the routed pairs, which do not change
    ids2, p2 = R.moe_route_sig_math(h, w, bias, k, norm, scale, n_shared=2)
    assert torch.equal(ids2[:, :k], ids) and torch.equal(p2[:, :k], p)
    assert ids2[:, k:].tolist() == [[E, E + 1]] * T and bool((p2[:, k:] == 1.0).all())


def test_ties_go_to_the_lower_id_and_nan_never_wins():
    h = torch.zeros(3, 4, dtype=torch.float64)
    h[1, 0] = float("nan")
    h[2, 1] = 1.0
    w = torch.zeros(6, 4, dtype=torch.float64)
    w[2, 0] = 1.0  # expert 2 reads the NaN of row 1
    w[4, 1] = 3.0
    bias = torch.zeros(6, dtype=torch.float64)
    ids, p = R.moe_route_sig_math(h, w, bias, 2, False)
    assert ids[0].tolist() == [0, 1] and p[0].tolist() == [0.5, 0.5]
    # row 1: every logit is NaN (0 * NaN): nothing wins on merit, the selection still completes
    assert ids[1].tolist() == [0, 1] and p[1].tolist() == [0.0, 0.0]
    assert ids[2].tolist() == [4, 0]
    h2 = torch.zeros(1, 4, dtype=torch.float64)
    w2 = w.clone()
    w2[2, 0] = float("nan")
    h2[0, 0] = 1.0  # only expert 2's logit is NaN
    ids, p = R.moe_route_sig_math(h2, w2, bias + torch.tensor([0, 0, 9, 0, 0, 0.0]), 5, True)
    assert 2 not in ids[0].tolist() and bool(p.isfinite().all())


@pytest.mark.parametrize("S", [1, 2, 3])
def test_a_shared_mlp_is_s_always_chosen_experts(S):
    """down(silu(gate h) * up h) over width S * I == the sum over S slices of
    width I, so stacking the slices behind the routed experts with weight 1
    computes routed(h) + shared(h)."""
    g = torch.Generator().manual_seed(10 + S)
    T, H, I, E, k = 33, 64, 48, 8, 2
    d = dict(generator=g, dtype=torch.float64)
    h = torch.randn(T, H, **d)
    wr, bias = torch.randn(E, H, **d) / 8, 0.3 * torch.randn(E, **d)
    wgu, wd = torch.randn(E, 2 * I, H, **d) / 8, torch.randn(E, H, I, **d) / 7
    sg, su, sd = torch.randn(S * I, H, **d) / 8, torch.randn(S * I, H, **d) / 8, torch.randn(H, S * I, **d) / 7
    routed = R.moe_mlp_sh_math(h, wr, bias, wgu, wd, k, True, 2.5, 0)
    gate = h @ sg.t()
    shared = (gate / (1.0 + torch.exp(-gate)) * (h @ su.t())) @ sd.t()
    G, D = R.moe_stack_shared(wgu, wd, sg, su, sd, S)
    assert G.shape == (E + S, 2 * I, H) and D.shape == (E + S, H, I)
    for s in range(S):
        assert torch.equal(G[E + s, :I], sg[s * I:(s + 1) * I]) and torch.equal(G[E + s, I:], su[s * I:(s + 1) * I])
        assert torch.equal(D[E + s], sd[:, s * I:(s + 1) * I])
    got = R.moe_mlp_sh_math(h, wr, bias, G, D, k, True, 2.5, S)
    exp = routed + shared
    assert ((got - exp).abs().max() / exp.abs().max()).item() < 1e-12
    # the wrong slice order is a different function
    if S > 1:
        Dw = torch.cat([D[:E], D[E:].flip(0)], 0)
        bad = R.moe_mlp_sh_math(h, wr, bias, G, Dw, k, True, 2.5, S)
        assert ((bad - exp).abs().max() / exp.abs().max()).item() > 1e-2
    with pytest.raises(ValueError, match="moe_stack_shared"):
        R.moe_stack_shared(wgu, wd, sg[:-1], su, sd, S)


def _hf_partial_rope(x, pos, R_, theta):
    """The checkpoint's partial rotation of x [D] at position ``pos``:
    the first R dims in half-split pairs (i, i + R/2), the rest passed through."""
    inv = 1.0 / (theta ** (torch.arange(0, R_, 2, dtype=torch.float64) / R_))
    emb = torch.cat([pos * inv, pos * inv])
    rot, rest = x[:R_], x[R_:]
    half = torch.cat([-rot[R_ // 2:], rot[:R_ // 2]])
    return torch.cat([rot * emb.cos() + half * emb.sin(), rest])


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("frac", [0.5, 1.0, 0.25])
def test_partial_rotary_is_a_head_permutation_and_a_zero_frequency_table(D, frac):
    R_ = int(D * frac)
    theta = 1e6
    perm = R.partial_rotary_perm(D, 0 if R_ == D else R_)
    assert sorted(perm.tolist()) == list(range(D))
    if R_ == D:
        assert perm.tolist() == list(range(D))
    inv = R.rope_inv_freq(D, theta, None, 0 if R_ == D else R_)
    assert inv.shape == (D // 2,) and bool((inv[R_ // 2:] == 0).all())
    assert torch.equal(inv[:R_ // 2], 1.0 / (theta ** (torch.arange(0, R_, 2, dtype=torch.float64) / R_)))
    tab = R.rope_tables(1000, D, theta, rotary_dim=0 if R_ == D else R_)
    assert bool((tab[:, R_ // 2:, 0] == 1).all()) and bool((tab[:, R_ // 2:, 1] == 0).all())
    g = torch.Generator().manual_seed(D + R_)
    for _ in range(20):
        q, k = torch.randn(D, generator=g, dtype=torch.float64), torch.randn(D, generator=g, dtype=torch.float64)
        pq, pk = (int(v) for v in torch.randint(0, 1000, (2,), generator=g))
        exp = _hf_partial_rope(q, pq, R_, theta) @ _hf_partial_rope(k, pk, R_, theta)
        ang_q, ang_k = pq * inv, pk * inv
        cs = lambda a: torch.stack([a.cos(), a.sin()], -1)[None]  # noqa: E731 -- a one-row table
        rq = R.apply_rope(q[perm][None, None].double(), torch.zeros(1), cs(ang_q).double())
        rk = R.apply_rope(k[perm][None, None].double(), torch.zeros(1), cs(ang_k).double())
        # apply_rope works in fp32; redo its arithmetic in fp64
        def rot(x, a):
            x1, x2 = x[:D // 2], x[D // 2:]
            return torch.cat([x1 * a.cos() - x2 * a.sin(), x2 * a.cos() + x1 * a.sin()])
        got = rot(q[perm], ang_q) @ rot(k[perm], ang_k)
        assert abs(got - exp) <= 1e-12 * max(1.0, abs(exp)), (got, exp)
        assert abs((rq[0, 0].double() @ rk[0, 0].double()) - exp) <= 1e-4 * max(1.0, abs(exp))
    for bad in (3, D + 2, -2):
        with pytest.raises(ValueError, match="rotary_dim"):
            R.rope_inv_freq(D, theta, None, bad)
