"""``reference.moe_route`` / ``reference.moe_mlp`` (the CPU path of the routed
expert MLP and the definition the gfx950 kernels are tested against) against a
per-token fp64 loop written from the Qwen3-MoE block's definition."""
import math

import pytest
import torch

from dmcp import ops
from dmcp.ops import reference


def _case(T, H, I, E, seed, router_scale=2.0):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(T, H, generator=g).to(torch.bfloat16)
    wr = (torch.randn(E, H, generator=g) * (router_scale / H ** 0.5)).to(torch.bfloat16)
    wgu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)
    return h, wr, wgu, wd


def _loop(h, wr, wgu, wd, k, norm):
    """Per token, in Python floats / fp64 tensors: ids, p, y."""
    T, H = h.shape
    E, I = wr.shape[0], wd.shape[2]
    hd, wrd, wgud, wdd = h.double(), wr.double(), wgu.double(), wd.double()
    ids, ps, ys = [], [], []
    for t in range(T):
        logits = [float(hd[t] @ wrd[e]) for e in range(E)]
        mx = max(logits)
        ex = [math.exp(v - mx) for v in logits]
        prob = [v / sum(ex) for v in ex]
        order = sorted(range(E), key=lambda e: (-prob[e], e))[:k]  # a tie goes to the lower id
        p = [prob[e] for e in order]
        if norm:
            p = [v / sum(p) for v in p]
        y = torch.zeros(H, dtype=torch.float64)
        for e, pe in zip(order, p):
            gu = wgud[e] @ hd[t]
            gate, up = gu[:I], gu[I:]
            y += pe * (wdd[e] @ (gate / (1 + torch.exp(-gate)) * up))
        ids.append(order)
        ps.append(p)
        ys.append(y)
    return torch.tensor(ids), torch.tensor(ps, dtype=torch.float64), torch.stack(ys)


@pytest.mark.parametrize("k,norm", [(1, True), (1, False), (2, True), (2, False), (8, True), (8, False)])
def test_route_and_mlp_match_the_per_token_loop(k, norm):
    T, H, I, E = 24, 64, 64, 8
    h, wr, wgu, wd = _case(T, H, I, E, seed=3 + k)
    ids, p, y = _loop(h, wr, wgu, wd, k, norm)
    rid, rp = reference.moe_route(h, wr, k, norm)
    assert rid.dtype == torch.int32 and rp.dtype == torch.float32 and tuple(rid.shape) == (T, k)
    assert torch.equal(rid.long(), ids)
    torch.testing.assert_close(rp.double(), p, rtol=1e-5, atol=1e-7)
    if norm:
        torch.testing.assert_close(rp.sum(-1), torch.ones(T), rtol=1e-6, atol=1e-6)
    # fp64 definition: exact up to summation order
    yd = reference.moe_mlp_math(h.double(), wr.double(), wgu.double(), wd.double(), k, norm)
    torch.testing.assert_close(yd, y, rtol=1e-12, atol=1e-12)
    # the op: bf16 in, act and the result rounded to bf16 (2^-9 each, relative to sum |terms|)
    m = reference.moe_mlp(h, wr, wgu, wd, k, norm)
    assert m.dtype == torch.bfloat16
    assert ((m.double() - y).abs().max() / y.abs().max()).item() < 2 ** -6
    assert ops.moe_mlp(h, wr, wgu, wd, k, norm).equal(m)  # CPU tensors dispatch to the reference


def test_an_expert_without_rows_and_one_expert_with_every_row():
    T, H, I, E, k = 12, 64, 64, 8, 2
    h, wr, wgu, wd = _case(T, H, I, E, seed=9)
    # every row onto experts 5 then 1: their router rows point along every h
    unit = wr.float() / wr.float().pow(2).sum(-1, keepdim=True)
    h = (0.05 * h.float() + 9.0 * unit[5] + 7.0 * unit[1]).to(torch.bfloat16)
    ids, p, y = _loop(h, wr, wgu, wd, k, True)
    assert ids.tolist() == [[5, 1]] * T  # rank order, not id order; six experts have no row
    rid, _ = reference.moe_route(h, wr, k, True)
    assert torch.equal(rid.long(), ids)
    yd = reference.moe_mlp_math(h.double(), wr.double(), wgu.double(), wd.double(), k, True)
    torch.testing.assert_close(yd, y, rtol=1e-12, atol=1e-12)
    # k = 1: one expert owns every row
    ids1, _, y1 = _loop(h, wr, wgu, wd, 1, False)
    assert ids1.unique().tolist() == [5]
    torch.testing.assert_close(reference.moe_mlp_math(h.double(), wr.double(), wgu.double(), wd.double(), 1, False),
                               y1, rtol=1e-12, atol=1e-12)


def test_a_tie_goes_to_the_lower_expert_id():
    H, I, E = 64, 64, 8
    h, wr, wgu, wd = _case(5, H, I, E, seed=4)
    wr[6] = wr[2]  # experts 2 and 6 always tie
    wr[3] = wr[2]
    for k in (1, 2, 3, 4):
        ids, _ = reference.moe_route(h, wr, k, True)
        lid, _, _ = _loop(h, wr, wgu, wd, k, True)
        assert torch.equal(ids.long(), lid)
        for row in ids.tolist():
            tied = [e for e in row if e in (2, 3, 6)]
            assert tied == sorted(tied) and tied == [2, 3, 6][:len(tied)]
    # an all-equal router: the k lowest ids, equal probabilities
    flat = torch.zeros_like(wr)
    ids, p = reference.moe_route(h, flat, 3, True)
    assert ids.tolist() == [[0, 1, 2]] * 5 and bool((p == p[0, 0]).all())
    ids, p = reference.moe_route(h, flat, 3, False)
    torch.testing.assert_close(p, torch.full((5, 3), 1 / 8))


def test_fused_residual_and_norm_is_add_rmsnorm():
    T, H, I, E, k = 7, 64, 128, 4, 2
    h, wr, wgu, wd = _case(T, H, I, E, seed=6)
    g = torch.Generator().manual_seed(7)
    resid = torch.randn(T, H, generator=g).to(torch.bfloat16)
    nw = (1 + 0.25 * torch.randn(H, generator=g)).to(torch.bfloat16)
    m = reference.moe_mlp(h, wr, wgu, wd, k, True)
    r1, r2, r3 = resid.clone(), resid.clone(), resid.clone()
    out = reference.moe_mlp(h, wr, wgu, wd, k, True, residual=r1, norm_w=nw, eps=1e-6)
    assert torch.equal(out, reference.add_rmsnorm(m, nw, 1e-6, residual=r2)) and torch.equal(r1, r2)
    assert reference.moe_mlp(h, wr, wgu, wd, k, True, residual=r3) is r3 and torch.equal(r3, r2)


def test_bad_arguments():
    h, wr, wgu, wd = _case(3, 64, 64, 4, seed=1)
    for k in (0, 5):
        with pytest.raises(ValueError, match="top_k"):
            reference.moe_route(h, wr, k, True)
    with pytest.raises(ValueError):
        reference.moe_mlp(h, wr, wgu[:, :-1], wd, 2, True)
    assert "moe_route" in ops.DEVICE_OPS and "moe_mlp" in ops.DEVICE_OPS
