"""The sigmoid-routed expert MLP with shared pseudo-experts (csrc/moe.hip,
``ops.moe_route_sig`` / ``ops.moe_mlp_sh``) on the GPU, by the methods of
tests/test_gpu_moe.py: the exact-integer structure test, the routing against
fp64 under that file's near-tie exclusion, numerics against fp64 measured
relative to the bf16 torch per-expert loop, the fused residual + RMSNorm
against add_rmsnorm, determinism and bit-exact hipGraph replays.

Exact structure.  That file's construction (see its docstring) under the
sigmoid router: a chosen expert's logit is 8, any other's 0, the bias 0, so the
chosen set has the k largest scores; equal chosen scores renormalise to exactly
1 / k (a butterfly sum of k equal values, k a power of two) and the scale c is a
power of two, so p = c / k exactly.  The S shared pseudo-experts E .. E + S - 1
carry the same integer weights as a routed expert of that id, so

    y[t, c] = 32 (c / k sum_{e chosen} u(t, c, e) + sum_{s < S} u(t, c, E + s)),
    u(t, c, e) = a_t (e % 3 + 1) + b_t (((c + e) % I) % 4)

with the bracket a multiple of c / k below 256 c / k steps: exact in bf16.
"""
import pytest
import torch

from tests.test_gpu_moe import _chosen, _torch_loop

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SHAPES = [(256, 128, 8, 2), (512, 192, 160, 8)]  # 160 experts: a partly filled third slot per routing lane
SHARED = [0, 1, 2]
ROWS = [1, 16, 17, 33, 130, 300]
SCALE = {2: 4.0, 8: 8.0}  # per top_k, a power of two: p = 2 and p = 1


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


# ------------------------------------------------------------ exact structure
_STRUCT = {}


def _structured_weights(H, I, E, S):
    """tests/test_gpu_moe.py's integer weights over E + S stacked experts; the router has the E routed rows."""
    if (H, I, E, S) not in _STRUCT:
        G = E + S
        wr = torch.zeros(E, H)
        wr[torch.arange(E), 8 + torch.arange(E)] = 8.0
        wgu = torch.zeros(G, 2 * I, H)
        wgu[:, :I, 0] = 32.0
        wgu[:, I:, 1] = (torch.arange(G) % 3 + 1).float()[:, None]
        wgu[:, I:, 2] = (torch.arange(I) % 4).float()[None, :]
        wd = torch.zeros(G, H, I)
        c = torch.arange(H)
        for e in range(G):
            wd[e, c, (c + e) % I] = 1.0
        _STRUCT[H, I, E, S] = tuple(t.to(torch.bfloat16).cuda() for t in (wr, wgu, wd))
    return _STRUCT[H, I, E, S]


def _structured_case(H, I, E, k, S, T, chosen, scale):
    h = torch.zeros(T, H)
    t = torch.arange(T)
    a, b = (t % 5 + 1).float(), ((t // 5) % 4).float()
    h[:, 0], h[:, 1], h[:, 2] = 1.0, a, b
    ch = torch.tensor(chosen)  # [T, k]
    h[t[:, None], 8 + ch] = 1.0
    c = torch.arange(H)

    def u(ids):  # [T, n] expert ids -> [T, n, H]
        col = ((c[None, None, :] + ids[:, :, None]) % I) % 4
        return a[:, None, None] * (ids % 3 + 1)[:, :, None].float() + b[:, None, None] * col.float()
    routed = u(ch).sum(1)
    shared = u((E + torch.arange(S))[None, :].expand(T, S)).sum(1) if S else torch.zeros(T, H)
    w = scale / k
    # every partial sum is a multiple of w with fewer than 256 steps: exact in bf16 and fp32
    assert float((routed + shared / w).max()) < 256 and (w >= 1 or float(1 / w).is_integer())
    exp = 32.0 * (w * routed + shared)
    return h.to(torch.bfloat16).cuda(), exp.cuda(), ch


def _exact_cases():
    cases = []
    for shape in SHAPES:
        for S in SHARED:
            for T in ROWS:
                cases += [(shape, S, T, "uniform", 0), (shape, S, T, "same", 0)]
            for T in (130, 300):
                cases += [(shape, S, T, "tile", d) for d in (-1, 0, 1)]
    return cases


@pytest.mark.parametrize("shape,S,T,routing,delta", _exact_cases())
def test_exact_structure(hip, shape, S, T, routing, delta):
    H, I, E, k = shape
    scale = SCALE[k]
    MT = hip.moe_row_tile(T, E + S, k + S)
    assert MT in hip.MOE_ROW_TILES
    chosen = _chosen(routing, T, E, k, n_special=MT + delta)
    wr, wgu, wd = _structured_weights(H, I, E, S)
    bias = torch.zeros(E, device="cuda")
    h, exp, ch = _structured_case(H, I, E, k, S, T, chosen, scale)
    ids, p = hip.moe_route_sig(h, wr, bias, k, True, scale, S)
    assert tuple(ids.shape) == tuple(p.shape) == (T, k + S)
    assert torch.equal(ids[:, :k].cpu().long(), ch.sort(1).values), "ties go to the lower id: the chosen set, ascending"
    assert bool((p[:, :k] == scale / k).all())
    assert ids[:, k:].cpu().tolist() == [[E + s for s in range(S)]] * T and bool((p[:, k:] == 1.0).all())
    if routing == "tile":
        assert int((ids == 2).sum()) == MT + delta
    got = hip.moe_mlp_sh(h, wr, bias, wgu, wd, k, True, scale, S)
    bad = (got.float() != exp).nonzero()
    assert bad.numel() == 0, (bad[:5].tolist(), got.float()[tuple(bad[0])].item(), exp[tuple(bad[0])].item())


def test_row_tile_threshold_is_covered(hip):
    """Both row tiles are exercised by the cases above for every S, each with
    a row count below and above the switch."""
    for S in SHARED:
        tiles = {hip.moe_row_tile(T, E + S, k + S) for (_, _, E, k) in SHAPES for T in ROWS}
        assert tiles == set(hip.MOE_ROW_TILES) == {32, 128}, S


def test_the_bias_decides_the_selection_and_stays_out_of_the_weight(hip):
    """Without renormalisation: expert 1 (logit 0, bias 1: 0.5 + 1) is chosen
    over experts 4 and 6 (logit 8, bias 0: 0.9997), its weight is exactly
    sigmoid(0) = 0.5, and the second rank goes to the lower of the two."""
    H, I, E, k = SHAPES[0]
    wr, _, _ = _structured_weights(H, I, E, 0)
    T = 70
    h = torch.zeros(T, H)
    h[:, 0] = 1.0
    h[:, 8 + 4] = 1.0
    h[:, 8 + 6] = 1.0
    h = h.to(torch.bfloat16).cuda()
    bias = torch.zeros(E)
    bias[1] = 1.0
    ids, p = hip.moe_route_sig(h, wr, bias.cuda(), k, False, 1.0, 1)
    assert ids.cpu().tolist() == [[1, 4, E]] * T
    assert bool((p[:, 0] == 0.5).all()) and bool((p[:, 2] == 1.0).all())
    s8 = 1.0 / (1.0 + torch.exp(torch.tensor(-8.0, dtype=torch.float64))).item()
    assert float((p[:, 1].double().cpu() - s8).abs().max()) < 1e-6
    # the same rows without the bias choose 4 and 6
    ids0, _ = hip.moe_route_sig(h, wr, torch.zeros(E, device="cuda"), k, False, 1.0, 0)
    assert ids0.cpu().tolist() == [[4, 6]] * T


# ---------------------------------------------------------- random cases, fp64
def _random_sh_case(shape, S, T, seed):
    """tests/test_gpu_moe.py's random case -- randn rows, router and experts,
    each row with a planted preference for k random experts -- at logits the
    sigmoid does not saturate: noise of std 0.15, planted logits near 2, 2.25,
    ... (that file's 4, 4.5, ... put the planted scores within 0.02 of 1 and the
    k-th within the 2^-7 margin of the (k+1)-th on a tenth of the rows at E =
    160; no seed meets the 2 % cap there).  A selection bias of std 0.02, the
    size of the planted scores' spacing, reorders ranks and changes choices.
    S shared slices are drawn like the experts."""
    H, I, E, k = shape
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(T, H, generator=g)
    wr = (torch.randn(E, H, generator=g) * (0.15 / H ** 0.5)).to(torch.bfloat16)
    pick = torch.rand(T, E, generator=g).argsort(-1)[:, :k]
    unit = wr.float() / wr.float().pow(2).sum(-1, keepdim=True)
    for j in range(k):
        h += (2.0 + 0.25 * j) * unit[pick[:, j]]
    h = h.to(torch.bfloat16)
    wgu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)
    g = torch.Generator().manual_seed(seed + 5000)
    bias = 0.02 * torch.randn(E, generator=g)
    if S:
        wgu = torch.cat([wgu, (torch.randn(S, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)], 0)
        wd = torch.cat([wd, (torch.randn(S, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)], 0)
    return h, wr, bias, wgu, wd


def _fp64_oracle(h, wr, bias, wgu, wd, k, norm, scale, S):
    """ids, p, y, bound B, the rows kept by the margin rule -- all fp64, CPU.
    The margin is tests/test_gpu_moe.py's, on the selection score s + bias: rows
    whose k-th and (k+1)-th scores lie within 2^-7 of the row's largest |score|
    are excluded."""
    from dmcp.ops import reference
    hd, wrd, bd, wgud, wdd = (t.double() for t in (h, wr, bias, wgu, wd))
    ids, p = reference.moe_route_sig_math(hd, wrd, bd, k, norm, scale, S)
    y = reference.moe_mlp_sh_math(hd, wrd, bd, wgud, wdd, k, norm, scale, S)
    I = wd.shape[2]
    B = torch.zeros_like(y)
    for j in range(k + S):
        for e in ids[:, j].unique().tolist():
            rows = (ids[:, j] == e).nonzero()[:, 0]
            gu = hd[rows].abs() @ wgud[e].abs().t()
            B[rows] += p[rows, j:j + 1] * ((gu[:, :I] * gu[:, I:]) @ wdd[e].abs().t())
    score = torch.sigmoid(hd @ wrd.t()) + bd
    srt = score.sort(-1, descending=True).values
    E = wr.shape[0]
    gap = srt[:, k - 1] - srt[:, k] if k < E else torch.full((h.shape[0],), float("inf"), dtype=torch.float64)
    keep = gap > score.abs().max(-1).values * 2.0 ** -7
    return ids, p, y, B, keep


ROUTE_CASES = [((256, 128, 8, 2), 300, True, 1.0, 21), ((512, 192, 160, 8), 300, False, 2.5, 22),
               ((512, 192, 160, 8), 130, True, 2.5, 23), ((256, 128, 8, 8), 40, True, 1.0, 24),
               ((256, 128, 8, 1), 40, False, 0.5, 25)]


@pytest.mark.parametrize("shape,T,norm,scale,seed", ROUTE_CASES)
def test_routing_matches_fp64(hip, shape, T, norm, scale, seed):
    """ids on every row outside the margin rule; the weights on those rows
    within tests/test_gpu_moe.py's bound, derived the same way: |d logit| <= H
    2^-24 sum |h w|; d s / s = (1 - s) d logit <= |d logit|, so a weight's
    relative error is at most twice the largest logit error (numerator and
    denominator), plus 1e-5 for expf and the divisions."""
    H, I, E, k = shape
    S = 1
    h, wr, bias, _, _ = _random_sh_case(shape, 0, T, seed)
    from dmcp.ops import reference
    hd, wrd, bd = h.double(), wr.double(), bias.double()
    ids, p = reference.moe_route_sig_math(hd, wrd, bd, k, norm, scale, S)
    score = torch.sigmoid(hd @ wrd.t()) + bd
    srt = score.sort(-1, descending=True).values
    gap = srt[:, k - 1] - srt[:, k] if k < E else torch.full((T,), float("inf"), dtype=torch.float64)
    keep = gap > score.abs().max(-1).values * 2.0 ** -7
    assert int((~keep).sum()) <= 0.02 * T, "the reference alone must meet the exclusion cap"
    if 1 < k < E:  # the bias matters on these inputs: it reorders the ranks
        plain = reference.moe_route_sig_math(hd, wrd, torch.zeros_like(bd), k, norm, scale, S)[0]
        assert int((plain != ids).any(1).sum()) >= T // 10
    kids, kp = hip.moe_route_sig(h.cuda(), wr.cuda(), bias.cuda(), k, norm, scale, S)
    kids, kp = kids.long().cpu(), kp.double().cpu()
    assert torch.equal(kids[keep], ids[keep])
    dense = torch.zeros(T, E + S, dtype=torch.float64).scatter_(1, ids, p)
    kdense = torch.zeros(T, E + S, dtype=torch.float64).scatter_(1, kids, kp)
    rtol = 2 * H * 2.0 ** -24 * (hd.abs() @ wrd.abs().t()).max().item() + 1e-5
    on = dense[keep] > 0
    worst = ((kdense[keep] - dense[keep]).abs()[on] / dense[keep][on]).max().item()
    print(f"glm routing {shape} T={T}: rows excluded {int((~keep).sum())}, worst rel weight error {worst:.3e} "
          f"(bound {rtol:.3e})")
    assert worst <= rtol
    # every row, excluded or not: k distinct routed ids inside [0, E), then the shared pair
    assert int(kids[:, :k].min()) >= 0 and int(kids[:, :k].max()) < E
    assert all(len(set(r)) == k for r in kids[:, :k].tolist())
    assert bool((kids[:, k:] == E).all()) and bool((kp[:, k:] == 1.0).all())
    # rank order: the kernel's own selection scores descend
    ks = score.gather(1, kids[:, :k])
    assert bool((ks[:, :-1] >= ks[:, 1:] - 1e-6).all())


NUM_CASES = [((256, 128, 8, 2), 1, 130, True, 1.0, 11), ((256, 128, 8, 2), 2, 300, False, 2.5, 12),
             ((512, 192, 160, 8), 1, 33, True, 2.5, 113), ((512, 192, 160, 8), 2, 300, True, 1.0, 14),
             ((256, 128, 8, 2), 0, 130, True, 2.5, 15)]


@pytest.mark.parametrize("shape,S,T,norm,scale,seed", NUM_CASES)
def test_numerics_against_fp64_relative_to_the_bf16_loop(hip, shape, S, T, norm, scale, seed):
    """max |err| / B against the fp64 definition on the bf16-rounded inputs; the
    kernel may reach 2x the figure of the bf16 torch loop (shared slices
    included, as experts E + s with weight 1) on the same inputs and routing."""
    H, I, E, k = shape
    h, wr, bias, wgu, wd = _random_sh_case(shape, S, T, seed)
    ids, p, y, B, keep = _fp64_oracle(h, wr, bias, wgu, wd, k, norm, scale, S)
    assert int((~keep).sum()) <= 0.02 * T, "the reference alone must meet the exclusion cap"
    hc, wrc, bc, wguc, wdc = (t.cuda() for t in (h, wr, bias, wgu, wd))
    loop = _torch_loop(hc, wguc, wdc, ids.cuda(), p.float().cuda()).double().cpu()
    got = hip.moe_mlp_sh(hc, wrc, bc, wguc, wdc, k, norm, scale, S).double().cpu()
    kids = hip.moe_route_sig(hc, wrc, bc, k, norm, scale, S)[0].long().cpu()
    assert torch.equal(kids[keep], ids[keep])
    Bk = B[keep] + 1e-30
    r_loop = ((loop[keep] - y[keep]).abs() / Bk).max().item()
    r_kern = ((got[keep] - y[keep]).abs() / Bk).max().item()
    print(f"glm moe numerics {shape} S={S} T={T} norm={norm} scale={scale}: max |err| / B  torch bf16 loop "
          f"{r_loop:.3e}  kernel {r_kern:.3e} ({r_kern / r_loop:.2f}x), rows excluded {int((~keep).sum())}")
    assert r_kern <= 2 * r_loop, (r_kern, r_loop)


# ----------------------------------------------------- fused residual + norm
@pytest.mark.parametrize("shape,S,T", [((256, 128, 8, 2), 1, 17), ((512, 192, 160, 8), 2, 130)])
def test_fused_residual_norm_is_add_rmsnorm(hip, shape, S, T):
    H, I, E, k = shape
    h, wr, bias, wgu, wd = (t.cuda() for t in _random_sh_case(shape, S, T, 31))
    g = torch.Generator(device="cuda").manual_seed(32)
    resid = torch.randn(T, H, generator=g, device="cuda").to(torch.bfloat16)
    nw = (1.0 + 0.25 * torch.randn(H, generator=g, device="cuda")).to(torch.bfloat16)
    ws = hip.moe_sh_workspace(T + 3, H, I, E, k, S, "cuda")
    args = (wr, bias, wgu, wd, k, True, 2.5, S)
    m = hip.moe_mlp_sh(h, *args, workspace=ws)
    assert torch.equal(hip.moe_mlp_sh(h, *args), m), "two eager runs are bit-identical"
    r1, r2, r3 = resid.clone(), resid.clone(), resid.clone()
    out = hip.moe_mlp_sh(h, *args, residual=r1, norm_w=nw, eps=1e-6, workspace=ws)
    exp = hip.add_rmsnorm(m, nw, 1e-6, residual=r2)
    assert torch.equal(out, exp) and torch.equal(r1, r2) and not torch.equal(r1, resid)
    back = hip.moe_mlp_sh(h, *args, residual=r3, workspace=ws)
    assert back is r3 and torch.equal(r3, r2)
    assert torch.equal(hip.moe_mlp_sh(h, *args, norm_w=nw, eps=1e-6), hip.add_rmsnorm(m, nw, 1e-6))


# --------------------------------------------------------------- graph replay
def test_graph_replay_follows_the_routing_bit_for_bit(hip):
    shape = SHAPES[0]
    H, I, E, k = shape
    S, T = 1, 40
    h0, wr, bias, wgu, wd = (t.cuda() for t in _random_sh_case(shape, S, T, 41))
    g = torch.Generator(device="cuda").manual_seed(42)
    h1 = torch.randn(T, H, generator=g, device="cuda").to(torch.bfloat16)
    # every row onto experts 3 and 5: their router rows dominate the input
    unit = wr.float() / wr.float().pow(2).sum(-1, keepdim=True)
    h2 = (0.1 * torch.randn(T, H, generator=g, device="cuda") + 8.0 * (unit[3] + unit[5])).to(torch.bfloat16)
    args = (wr, bias, wgu, wd, k, True, 2.5, S)
    ids2 = hip.moe_route_sig(h2, wr, bias, k, True, 2.5, S)[0]
    assert ids2.unique().tolist() == [3, 5, E]
    assert hip.moe_route_sig(h0, wr, bias, k, True, 2.5, S)[0].unique().numel() == E + S
    inputs = [h0, h1, h2]
    eager = [hip.moe_mlp_sh(x, *args) for x in inputs]
    assert all(torch.equal(hip.moe_mlp_sh(x, *args), e) for x, e in zip(inputs, eager))
    assert not torch.equal(eager[0], eager[1])
    ws = hip.moe_sh_workspace(T, H, I, E, k, S, "cuda")
    static_h = h0.clone()
    static_out = torch.empty_like(static_h)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.moe_mlp_sh(static_h, *args, workspace=ws, out=static_out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # one stream: the op is six launches in a line
        hip.moe_mlp_sh(static_h, *args, workspace=ws, out=static_out)
    for x, exp in list(zip(inputs, eager)) + [(inputs[2], eager[2]), (inputs[0], eager[0])]:
        static_h.copy_(x)
        graph.replay()
        assert torch.equal(static_out, exp)


def test_bad_arguments_are_refused(hip):
    shape = SHAPES[0]
    H, I, E, k = shape
    h, wr, bias, wgu, wd = (t.cuda() for t in _random_sh_case(shape, 1, 4, 51))
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp_sh(h, wr, bias, wgu, wd, E + 1, True, 1.0, 1)
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp_sh(h, wr, bias, wgu, wd, k, True, 1.0, 2)  # the stack holds one shared slice
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp_sh(h, wr, bias.cpu(), wgu, wd, k, True, 1.0, 1)
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp_sh(h, wr, bias, wgu, wd, k, True, 1.0, 1,
                       workspace=hip.moe_workspace(4, H, I, E, k, "cuda"))  # sized without the shared pair
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp_sh(h, wr, bias, wgu, wd, k, True, float("inf"), 1)
