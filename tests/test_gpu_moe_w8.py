"""The routed expert MLP over block-scaled FP8 expert weights (csrc/moe.hip,
ops.moe_mlp_w8) on the GPU, with the helpers of tests/test_gpu_moe.py.

Exact structure.  The integer construction of tests/test_gpu_moe.py, with
each 128 x 128 weight block stored as W / s for a power-of-two scale s in
{0.5, 1, 2, 4} chosen by (e + 3 nb + 5 kb + offset) % 4 (offset 0 for the gate,
1 for the up, 2 for the down projection).  Every stored value (64 ... 0.25) is
an e4m3 value, every partial sum a multiple of 1/4 below 2^13 and every
expected output still an exact integer; a scale taken from the wrong block,
projection or expert changes it.  (320, 192, 8, 2) has a 64-deep last K block
in gate/up and down, a 64-wide last N block in both, and no fragment 1 in
down's last column block.

Numerics.  The cases of tests/test_block_fp8_reference.py (which shows on the
CPU that five wrong scale readers miss this bound on them): the oracle is
fp64 over the exactly dequantised weights, B the same pass with absolute
values, the baseline the bf16 torch loop over the weights dequantised and
rounded to bf16 -- what load-time dequantisation would give -- and the kernel
may reach 2x the loop's max |err| / B.  Routing is untouched by the weight
format; the 2 % exclusion cap is asserted on the reference before a kernel runs.
"""
import pytest
import torch

from tests.test_block_fp8_reference import W8_NUM_CASES, w8_case
from tests.test_gpu_moe import (ROWS, _chosen, _fp64_oracle, _structured_case, _structured_weights,  # noqa: F401
                                _torch_loop, hip)

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SHAPES = [(256, 128, 8, 2), (512, 192, 128, 8), (320, 192, 8, 2)]
B = 128


# ------------------------------------------------------------ exact structure
def _pow2_scales(E, N, K, offset):
    e = torch.arange(E)[:, None, None]
    nb = torch.arange(-(-N // B))[None, :, None]
    kb = torch.arange(-(-K // B))[None, None, :]
    return 2.0 ** (((e + 3 * nb + 5 * kb + offset) % 4).float() - 1.0)   # 0.5, 1, 2, 4


def _expand(s, rows, cols):
    return s.repeat_interleave(B, dim=-2)[..., :rows, :].repeat_interleave(B, dim=-1)[..., :cols]


_STRUCT8 = {}


def _structured_w8(H, I, E):
    if (H, I, E) not in _STRUCT8:
        from dmcp.ops import reference
        wr, wgu, wd = _structured_weights(H, I, E)
        wgu, wd = wgu.float().cpu(), wd.float().cpu()
        sg, su, sd = _pow2_scales(E, I, H, 0), _pow2_scales(E, I, H, 1), _pow2_scales(E, H, I, 2)
        assert not torch.equal(sg, su)
        g8 = (wgu[:, :I] / _expand(sg, I, H)).to(torch.float8_e4m3fn)
        u8 = (wgu[:, I:] / _expand(su, I, H)).to(torch.float8_e4m3fn)
        d8 = (wd / _expand(sd, H, I)).to(torch.float8_e4m3fn)
        gu8, gs = torch.cat([g8, u8], 1).contiguous(), torch.cat([sg, su], 1).contiguous()
        # the stored values are e4m3 values: the real weights come back exactly
        back_gu, back_d = reference.moe_w8_dequant(gu8, gs, d8, sd)
        assert torch.equal(back_gu, wgu) and torch.equal(back_d, wd)
        assert float(gu8.float().abs().max()) == 64.0 and float(d8.float()[d8.float() > 0].min()) == 0.25
        _STRUCT8[H, I, E] = (wr, gu8.cuda(), gs.cuda(), d8.cuda(), sd.contiguous().cuda())
    return _STRUCT8[H, I, E]


def _exact_cases():
    cases = []
    for shape in SHAPES:
        for T in ROWS:
            cases += [(shape, T, "uniform", 0), (shape, T, "same", 0)]
        for T in (130, 300):
            cases += [(shape, T, "tile", d) for d in (-1, 0, 1)]
    return cases


@pytest.mark.parametrize("shape,T,routing,delta", _exact_cases())
def test_exact_structure(hip, shape, T, routing, delta):
    H, I, E, k = shape
    MT = hip.moe_row_tile(T, E, k)
    assert MT in hip.MOE_ROW_TILES
    chosen = _chosen(routing, T, E, k, n_special=MT + delta)
    wr, gu8, gs, d8, ds = _structured_w8(H, I, E)
    h, exp, ch = _structured_case(H, I, E, k, T, chosen)
    ids, p = hip.moe_route(h, wr, k, True)
    assert torch.equal(ids.cpu().long(), ch.sort(1).values)
    assert bool((p == 1.0 / k).all())
    if routing == "tile":
        assert int((ids == 2).sum()) == MT + delta
    got = hip.moe_mlp_w8(h, wr, gu8, gs, d8, ds, k, True)
    bad = (got.float() != exp).nonzero()
    assert bad.numel() == 0, (bad[:5].tolist(), got.float()[tuple(bad[0])].item(), exp[tuple(bad[0])].item())


def test_row_tiles_and_block_edges_are_covered():
    """Both row tiles are exercised by the shapes above, each with a row
    count just below and just above it; so are a half K block and a half N
    block in both GEMMs, and a last down block without its second fragment."""
    from dmcp.ops import hip as h
    for shape in SHAPES[:2]:
        assert {h.moe_row_tile(T, shape[2], shape[3]) for T in ROWS} <= set(h.MOE_ROW_TILES)
    tiles = {h.moe_row_tile(T, E, k) for (_, _, E, k) in SHAPES for T in ROWS}
    assert tiles == set(h.MOE_ROW_TILES) == {32, 128}
    assert {h.moe_row_tile(T, 8, 2) for T in ROWS} == {32, 128}   # the half-block shape sees both, too
    H, I, _, _ = SHAPES[2]
    assert H % 128 == 64 and I % 128 == 64 and (H // 64) % 2 == 1


# ------------------------------------------------------------------- numerics
@pytest.mark.parametrize("shape,T,norm,seed", W8_NUM_CASES)
def test_numerics_against_fp64_relative_to_the_bf16_loop(hip, shape, T, norm, seed):
    from dmcp.ops import reference
    H, I, E, k = shape
    h, wr, (gu8, gs, d8, ds) = w8_case(shape, T, seed)
    wgu, wd = reference.moe_w8_dequant(gu8, gs, d8, ds)          # exact, fp32
    ids, p, y, Bd, keep, _ = _fp64_oracle(h, wr, wgu, wd, k, norm)
    assert int((~keep).sum()) <= 0.02 * T, "the reference alone must meet the exclusion cap"
    hc, wrc = h.cuda(), wr.cuda()
    loop = _torch_loop(hc, wgu.to(torch.bfloat16).cuda(), wd.to(torch.bfloat16).cuda(), ids.cuda(),
                       p.float().cuda()).double().cpu()
    got = hip.moe_mlp_w8(hc, wrc, gu8.cuda(), gs.cuda(), d8.cuda(), ds.cuda(), k, norm).double().cpu()
    kids = hip.moe_route(hc, wrc, k, norm)[0].long().cpu()
    assert torch.equal(kids[keep], ids[keep])
    Bk = Bd[keep] + 1e-30
    r_loop = ((loop[keep] - y[keep]).abs() / Bk).max().item()
    r_kern = ((got[keep] - y[keep]).abs() / Bk).max().item()
    print(f"moe w8 numerics {shape} T={T} norm={norm}: max |err| / B  torch bf16 loop on dequantised weights "
          f"{r_loop:.3e}  kernel {r_kern:.3e} ({r_kern / r_loop:.2f}x), rows excluded {int((~keep).sum())}")
    assert r_kern <= 2 * r_loop, (r_kern, r_loop)


# ----------------------------------------------------- fused residual + norm
@pytest.mark.parametrize("shape,T", [((256, 128, 8, 2), 17), ((320, 192, 8, 2), 130)])
def test_fused_residual_norm_is_add_rmsnorm(hip, shape, T):
    H, I, E, k = shape
    h, wr, w8 = w8_case(shape, T, 31)
    h, wr, w8 = h.cuda(), wr.cuda(), tuple(t.cuda() for t in w8)
    g = torch.Generator(device="cuda").manual_seed(32)
    resid = torch.randn(T, H, generator=g, device="cuda").to(torch.bfloat16)
    nw = (1.0 + 0.25 * torch.randn(H, generator=g, device="cuda")).to(torch.bfloat16)
    ws = hip.moe_workspace(T + 3, H, I, E, k, "cuda")
    m = hip.moe_mlp_w8(h, wr, *w8, k, True, workspace=ws)
    r1, r2, r3 = resid.clone(), resid.clone(), resid.clone()
    out = hip.moe_mlp_w8(h, wr, *w8, k, True, residual=r1, norm_w=nw, eps=1e-6, workspace=ws)
    exp = hip.add_rmsnorm(m, nw, 1e-6, residual=r2)
    assert torch.equal(out, exp) and torch.equal(r1, r2) and not torch.equal(r1, resid)
    back = hip.moe_mlp_w8(h, wr, *w8, k, True, residual=r3, workspace=ws)
    assert back is r3 and torch.equal(r3, r2)
    assert torch.equal(hip.moe_mlp_w8(h, wr, *w8, k, True, norm_w=nw, eps=1e-6), hip.add_rmsnorm(m, nw, 1e-6))


# --------------------------------------------------------------- graph replay
def test_graph_replay_follows_the_routing_bit_for_bit(hip):
    H, I, E, k = SHAPES[0]
    T = 40
    h0, wr, w8 = w8_case(SHAPES[0], T, 41)
    h0, wr, w8 = h0.cuda(), wr.cuda(), tuple(t.cuda() for t in w8)
    g = torch.Generator(device="cuda").manual_seed(42)
    h1 = torch.randn(T, H, generator=g, device="cuda").to(torch.bfloat16)
    unit = wr.float() / wr.float().pow(2).sum(-1, keepdim=True)
    h2 = (0.1 * torch.randn(T, H, generator=g, device="cuda") + 8.0 * (unit[3] + unit[5])).to(torch.bfloat16)
    assert hip.moe_route(h2, wr, k, True)[0].unique().tolist() == [3, 5]
    assert hip.moe_route(h0, wr, k, True)[0].unique().numel() == E
    inputs = [h0, h1, h2]
    eager = [hip.moe_mlp_w8(x, wr, *w8, k, True) for x in inputs]
    assert not torch.equal(eager[0], eager[1])
    ws = hip.moe_workspace(T, H, I, E, k, "cuda")
    static_h = h0.clone()
    static_out = torch.empty_like(static_h)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.moe_mlp_w8(static_h, wr, *w8, k, True, workspace=ws, out=static_out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.moe_mlp_w8(static_h, wr, *w8, k, True, workspace=ws, out=static_out)
    for x, exp in list(zip(inputs, eager)) + [(inputs[2], eager[2]), (inputs[0], eager[0])]:
        static_h.copy_(x)
        graph.replay()
        first = static_out.clone()
        graph.replay()
        assert torch.equal(first, exp) and torch.equal(static_out, first)


def test_bad_arguments_are_refused(hip):
    H, I, E, k = SHAPES[0]
    h, wr, (gu8, gs, d8, ds) = w8_case(SHAPES[0], 4, 51)
    h, wr, gu8, gs, d8, ds = (t.cuda() for t in (h, wr, gu8, gs, d8, ds))
    assert hip.moe_mlp_w8(h, wr, gu8, gs, d8, ds, k, True).shape == h.shape
    bad = [dict(k=E + 1), dict(kw=dict(workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))),
           dict(h=h.float()), dict(gu8=gu8.view(torch.uint8)), dict(d8=d8.view(torch.uint8)),
           dict(gu8=gu8.to(torch.bfloat16)), dict(gs=gs[:, :1].contiguous()), dict(gs=gs.to(torch.bfloat16)),
           dict(ds=ds.transpose(1, 2)), dict(ds=ds.cpu()), dict(gs=None)]
    for b in bad:
        with pytest.raises(hip.HipOpsError):
            hip.moe_mlp_w8(b.get("h", h), wr, b.get("gu8", gu8), b.get("gs", gs), b.get("d8", d8), b.get("ds", ds),
                           b.get("k", k), True, **b.get("kw", {}))
