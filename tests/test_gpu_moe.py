"""The routed expert MLP (csrc/moe.hip) on the GPU: an exact-integer structure
test, numerics against fp64 measured relative to a bf16 torch per-expert loop,
the routing against fp64, the fused residual + RMSNorm against add_rmsnorm, and
bit-exact hipGraph replays under changing routing.

Exact structure.  Inputs are built so every intermediate is an exactly
representable integer (or integer / k):

    h[t, 0] = 1, h[t, 1] = a_t = t % 5 + 1, h[t, 2] = b_t = (t // 5) % 4,
    h[t, 8 + e] = 1 for the experts e the row is meant to choose
    router[e]   = 8 at column 8 + e             -> logit 8 (chosen) or 0
    gate_e[i]   = 32 at column 0                -> silu(32) = 32 in fp32
                  (1 + exp(-32) rounds to 1)
    up_e[i]     = (e % 3 + 1) at column 1, (i % 4) at column 2
    down_e[c]   = 1 at column (c + e) % I       -> picks act[(c + e) % I]

so with k a power of two p = 1 / k exactly (k equal probabilities, a
butterfly sum) and

    y[t, c] = 32 / k * sum_{e chosen} (a_t (e % 3 + 1) + b_t (((c + e) % I) % 4))

with every partial sum an integer below 256 * 32 / k: exact in bf16 and fp32.
A row gathered from the wrong place, a pair added twice or dropped, a wrong
expert's weights or a shifted column changes the integer.

Numerics.  randn inputs rounded to bf16, expected = the fp64 definition on
them, per-element bound B = sum_j p_j (|wd| . (Gabs * Uabs)) with Gabs = |h| .
|wg|, Uabs = |h| . |wu| (the second pass with absolute values; |silu(g)| <=
|g|).  The figure is max |err| / B; the kernel may reach 2x the figure of the
bf16 torch loop (index_select + F.linear + weighted index_add_) on the same
inputs and routing.  Rows whose k-th and (k+1)-th router logits lie within
2^-7 of the row's largest |logit| are excluded (their routing may
legitimately differ from fp64); at most 2 % of the rows, asserted on the
reference before a kernel runs.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(300)]

SHAPES = [(256, 128, 8, 2), (512, 192, 128, 8)]
ROWS = [1, 15, 16, 17, 33, 130, 300]


@pytest.fixture(scope="module")
def hip():
    from dmcp.ops import hip as h
    h.lib()
    return h


# ------------------------------------------------------------ exact structure
def _uniform(t, E, k):
    return [(t + j * (E // k)) % E for j in range(k)]


def _chosen(routing, T, E, k, n_special=0, e0=2):
    if routing == "uniform":
        return [_uniform(t, E, k) for t in range(T)]
    if routing == "same":
        return [[(3 + 2 * j) % E for j in range(k)] for _ in range(T)]
    # "tile": expert e0 gets exactly n_special rows (the first ones); nobody else chooses it
    out = []
    for t in range(T):
        others = [i if i < e0 else i + 1 for i in _uniform(t, E - 1, k)]
        out.append(([e0] + others[:k - 1]) if t < n_special else others)
    return out


_STRUCT = {}


def _structured_weights(H, I, E):
    if (H, I, E) not in _STRUCT:
        wr = torch.zeros(E, H)
        wr[torch.arange(E), 8 + torch.arange(E)] = 8.0
        wgu = torch.zeros(E, 2 * I, H)
        wgu[:, :I, 0] = 32.0
        wgu[:, I:, 1] = (torch.arange(E) % 3 + 1).float()[:, None]
        wgu[:, I:, 2] = (torch.arange(I) % 4).float()[None, :]
        wd = torch.zeros(E, H, I)
        c = torch.arange(H)
        for e in range(E):
            wd[e, c, (c + e) % I] = 1.0
        _STRUCT[H, I, E] = tuple(t.to(torch.bfloat16).cuda() for t in (wr, wgu, wd))
    return _STRUCT[H, I, E]


def _structured_case(H, I, E, k, T, chosen):
    h = torch.zeros(T, H)
    t = torch.arange(T)
    a, b = (t % 5 + 1).float(), ((t // 5) % 4).float()
    h[:, 0], h[:, 1], h[:, 2] = 1.0, a, b
    ch = torch.tensor(chosen)  # [T, k]
    h[t[:, None], 8 + ch] = 1.0
    c = torch.arange(H)
    col = ((c[None, None, :] + ch[:, :, None]) % I) % 4                     # [T, k, H]
    u = a[:, None, None] * (ch % 3 + 1)[:, :, None].float() + b[:, None, None] * col.float()
    exp = u.sum(1) * (32.0 / k)
    assert float(u.sum(1).max()) < 256
    return h.to(torch.bfloat16).cuda(), exp.cuda(), ch


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
    wr, wgu, wd = _structured_weights(H, I, E)
    h, exp, ch = _structured_case(H, I, E, k, T, chosen)
    ids, p = hip.moe_route(h, wr, k, True)
    assert torch.equal(ids.cpu().long(), ch.sort(1).values), "ties go to the lower id: the chosen set, ascending"
    assert bool((p == 1.0 / k).all())
    if routing == "tile":
        assert int((ids == 2).sum()) == MT + delta
    got = hip.moe_mlp(h, wr, wgu, wd, k, True)
    bad = (got.float() != exp).nonzero()
    assert bad.numel() == 0, (bad[:5].tolist(), got.float()[tuple(bad[0])].item(), exp[tuple(bad[0])].item())


def test_row_tile_threshold_is_covered():
    """Both row tiles are exercised by the shapes above, each with a row
    count just below and just above it."""
    from dmcp.ops import hip as h
    tiles = {h.moe_row_tile(T, E, k) for (_, _, E, k) in SHAPES for T in ROWS}
    assert tiles == set(h.MOE_ROW_TILES) == {32, 128}
    assert h.moe_row_tile(255, 8, 2) == 32 and h.moe_row_tile(256, 8, 2) == 128


# ------------------------------------------------------------------- numerics
NUM_CASES = [((256, 128, 8, 2), 130, True, 11), ((256, 128, 8, 2), 300, False, 12),
             ((512, 192, 128, 8), 33, True, 113), ((512, 192, 128, 8), 300, True, 14)]


def _random_case(shape, T, seed):
    """randn rows, router, experts.  Among E random logits the k-th and
    (k+1)-th are closer than the margin rule's 2^-7 max |logit| on a third of
    the rows at E = 128 (dense order statistics), so no seed meets the 2 % cap
    on noise alone: each row also carries a planted preference for k random
    experts (logits near 4, 4.5, ...: above the noise of std 0.5), as a
    trained router's rows do."""
    H, I, E, k = shape
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(T, H, generator=g)
    wr = (torch.randn(E, H, generator=g) * (0.5 / H ** 0.5)).to(torch.bfloat16)
    pick = torch.rand(T, E, generator=g).argsort(-1)[:, :k]
    unit = wr.float() / wr.float().pow(2).sum(-1, keepdim=True)
    for j in range(k):
        h += (4.0 + 0.5 * j) * unit[pick[:, j]]
    h = h.to(torch.bfloat16)
    wgu = (torch.randn(E, 2 * I, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    wd = (torch.randn(E, H, I, generator=g) / I ** 0.5).to(torch.bfloat16)
    return h, wr, wgu, wd


def _fp64_oracle(h, wr, wgu, wd, k, norm):
    """ids, p, y, bound B, the rows kept by the margin rule -- all fp64, CPU."""
    from dmcp.ops import reference
    hd, wrd, wgud, wdd = (t.double() for t in (h, wr, wgu, wd))
    ids, p = reference.moe_route_math(hd, wrd, k, norm)
    y = reference.moe_mlp_math(hd, wrd, wgud, wdd, k, norm)
    I = wd.shape[2]
    B = torch.zeros_like(y)
    for j in range(k):
        for e in ids[:, j].unique().tolist():
            rows = (ids[:, j] == e).nonzero()[:, 0]
            gu = hd[rows].abs() @ wgud[e].abs().t()
            B[rows] += p[rows, j:j + 1] * ((gu[:, :I] * gu[:, I:]) @ wdd[e].abs().t())
    logits = hd @ wrd.t()
    srt = logits.sort(-1, descending=True).values
    E = wr.shape[0]
    gap = srt[:, k - 1] - srt[:, k] if k < E else torch.full((h.shape[0],), float("inf"), dtype=torch.float64)
    keep = gap > logits.abs().max(-1).values * 2.0 ** -7
    return ids, p, y, B, keep, logits


def _torch_loop(h, wgu, wd, ids, p):
    """The bf16 per-expert loop: index_select + F.linear + weighted index_add_."""
    I = wd.shape[2]
    out = torch.zeros_like(h)
    pb = p.to(torch.bfloat16)
    for e in ids.unique().tolist():
        rows, rank = (ids == e).nonzero(as_tuple=True)
        x = h.index_select(0, rows)
        gu = F.linear(x, wgu[e])
        y = F.linear(F.silu(gu[:, :I]) * gu[:, I:], wd[e])
        out.index_add_(0, rows, y * pb[rows, rank][:, None])
    return out


@pytest.mark.parametrize("shape,T,norm,seed", NUM_CASES)
def test_numerics_against_fp64_relative_to_the_bf16_loop(hip, shape, T, norm, seed):
    H, I, E, k = shape
    h, wr, wgu, wd = _random_case(shape, T, seed)
    ids, p, y, B, keep, _ = _fp64_oracle(h, wr, wgu, wd, k, norm)
    assert int((~keep).sum()) <= 0.02 * T, "the reference alone must meet the exclusion cap"
    hc, wrc, wguc, wdc = (t.cuda() for t in (h, wr, wgu, wd))
    loop = _torch_loop(hc, wguc, wdc, ids.cuda(), p.float().cuda()).double().cpu()
    got = hip.moe_mlp(hc, wrc, wguc, wdc, k, norm).double().cpu()
    kids = hip.moe_route(hc, wrc, k, norm)[0].long().cpu()
    assert torch.equal(kids[keep], ids[keep])
    Bk = B[keep] + 1e-30
    r_loop = ((loop[keep] - y[keep]).abs() / Bk).max().item()
    r_kern = ((got[keep] - y[keep]).abs() / Bk).max().item()
    print(f"moe numerics {shape} T={T} norm={norm}: max |err| / B  torch bf16 loop {r_loop:.3e}  kernel {r_kern:.3e} "
          f"({r_kern / r_loop:.2f}x), rows excluded {int((~keep).sum())}")
    assert r_kern <= 2 * r_loop, (r_kern, r_loop)


# -------------------------------------------------------------------- routing
@pytest.mark.parametrize("shape,T,norm,seed", [((256, 128, 8, 2), 300, True, 21), ((512, 192, 128, 8), 300, False, 22),
                                               ((512, 192, 128, 8), 130, True, 23), ((256, 128, 8, 8), 40, True, 24),
                                               ((256, 128, 8, 1), 40, False, 25)])
def test_routing_matches_fp64(hip, shape, T, norm, seed):
    """ids on every row outside the margin rule; p on those rows within the
    fp32 dot product's worst case: |d logit| <= H 2^-24 sum |h w| (products of
    bf16 values are exact in fp32, H - 1 additions and the wave reduction round),
    p's relative error is at most twice the largest logit error (numerator and
    denominator), plus 1e-5 for expf and the divisions."""
    H, I, E, k = shape
    h, wr, _, _ = _random_case((H, I, E, k), T, seed)
    ids, p, keep, logits = None, None, None, None
    from dmcp.ops import reference
    hd, wrd = h.double(), wr.double()
    ids, p = reference.moe_route_math(hd, wrd, k, norm)
    logits = hd @ wrd.t()
    srt = logits.sort(-1, descending=True).values
    gap = srt[:, k - 1] - srt[:, k] if k < E else torch.full((T,), float("inf"), dtype=torch.float64)
    keep = gap > logits.abs().max(-1).values * 2.0 ** -7
    assert int((~keep).sum()) <= 0.02 * T, "the reference alone must meet the exclusion cap"
    kids, kp = hip.moe_route(h.cuda(), wr.cuda(), k, norm)
    kids, kp = kids.long().cpu(), kp.double().cpu()
    assert torch.equal(kids[keep], ids[keep])
    rtol = 2 * H * 2.0 ** -24 * (hd.abs() @ wrd.abs().t()).max().item() + 1e-5
    worst = ((kp[keep] - p[keep]).abs() / p[keep]).max().item()
    print(f"moe routing {shape} T={T}: rows excluded {int((~keep).sum())}, worst rel p error {worst:.3e} (bound {rtol:.3e})")
    assert worst <= rtol
    # every row, excluded or not: k distinct ids inside [0, E)
    assert int(kids.min()) >= 0 and int(kids.max()) < E
    assert all(len(set(r)) == k for r in kids.tolist())


def test_routing_of_unplanted_rows_with_dense_near_ties(hip):
    """Plain randn rows and router at E = 128, k = 8, nothing planted: about a
    third of the rows have their 8th and 9th logits inside the margin (which
    is why the cases above plant preferences: the 2 % cap is out of reach
    here and is not asserted).  The rows outside the margin must match fp64
    id for id, as above; on the others every chosen expert must still be a
    defensible one -- its fp64 logit within the margin of the row's k-th
    largest -- and the k ids distinct and in rank order of the kernel's own
    probabilities."""
    H, I, E, k = 512, 192, 128, 8
    T = 300
    g = torch.Generator().manual_seed(61)
    h = torch.randn(T, H, generator=g).to(torch.bfloat16)
    wr = (torch.randn(E, H, generator=g) / H ** 0.5).to(torch.bfloat16)
    from dmcp.ops import reference
    hd, wrd = h.double(), wr.double()
    ids, p = reference.moe_route_math(hd, wrd, k, True)
    logits = hd @ wrd.t()
    srt = logits.sort(-1, descending=True).values
    margin = logits.abs().max(-1).values * 2.0 ** -7
    keep = srt[:, k - 1] - srt[:, k] > margin
    n_tied = int((~keep).sum())
    # order statistics of 128 normal logits: the test is about near ties, so
    # it needs both kinds of row in numbers
    assert n_tied >= T // 10 and int(keep.sum()) >= T // 3, n_tied
    kids, kp = hip.moe_route(h.cuda(), wr.cuda(), k, True)
    kids, kp = kids.long().cpu(), kp.double().cpu()
    assert torch.equal(kids[keep], ids[keep])
    rtol = 2 * H * 2.0 ** -24 * (hd.abs() @ wrd.abs().t()).max().item() + 1e-5
    worst = ((kp[keep] - p[keep]).abs() / p[keep]).max().item()
    chosen = logits.gather(1, kids)
    slack = (srt[:, k - 1:k] - margin[:, None] - chosen).max().item()
    print(f"moe routing unplanted T={T}: rows inside the margin {n_tied}, worst rel p error on the others "
          f"{worst:.3e} (bound {rtol:.3e}), chosen logit below the k-th by at most {max(slack, 0.0):.3e} + margin")
    assert worst <= rtol
    assert slack <= 0, "a chosen expert's logit is more than the margin below the row's k-th largest"
    assert all(len(set(r)) == k for r in kids.tolist())
    assert bool((kp[:, :-1] >= kp[:, 1:]).all()) and bool(((kp.sum(-1) - 1).abs() < 1e-5).all())


# ----------------------------------------------------- fused residual + norm
@pytest.mark.parametrize("shape,T", [((256, 128, 8, 2), 17), ((512, 192, 128, 8), 130)])
def test_fused_residual_norm_is_add_rmsnorm(hip, shape, T):
    H, I, E, k = shape
    h, wr, wgu, wd = (t.cuda() for t in _random_case(shape, T, 31))
    g = torch.Generator(device="cuda").manual_seed(32)
    resid = torch.randn(T, H, generator=g, device="cuda").to(torch.bfloat16)
    nw = (1.0 + 0.25 * torch.randn(H, generator=g, device="cuda")).to(torch.bfloat16)
    ws = hip.moe_workspace(T + 3, H, I, E, k, "cuda")
    m = hip.moe_mlp(h, wr, wgu, wd, k, True, workspace=ws)
    r1, r2, r3 = resid.clone(), resid.clone(), resid.clone()
    out = hip.moe_mlp(h, wr, wgu, wd, k, True, residual=r1, norm_w=nw, eps=1e-6, workspace=ws)
    exp = hip.add_rmsnorm(m, nw, 1e-6, residual=r2)
    assert torch.equal(out, exp) and torch.equal(r1, r2) and not torch.equal(r1, resid)
    back = hip.moe_mlp(h, wr, wgu, wd, k, True, residual=r3, workspace=ws)
    assert back is r3 and torch.equal(r3, r2)
    # no residual: the norm of m alone
    assert torch.equal(hip.moe_mlp(h, wr, wgu, wd, k, True, norm_w=nw, eps=1e-6), hip.add_rmsnorm(m, nw, 1e-6))


# --------------------------------------------------------------- graph replay
def test_graph_replay_follows_the_routing_bit_for_bit(hip):
    H, I, E, k = SHAPES[0]
    T = 40
    h0, wr, wgu, wd = (t.cuda() for t in _random_case(SHAPES[0], T, 41))
    g = torch.Generator(device="cuda").manual_seed(42)
    h1 = torch.randn(T, H, generator=g, device="cuda").to(torch.bfloat16)
    # every row onto experts 3 and 5: their router rows dominate the input
    unit = wr.float() / wr.float().pow(2).sum(-1, keepdim=True)
    h2 = (0.1 * torch.randn(T, H, generator=g, device="cuda") + 8.0 * (unit[3] + unit[5])).to(torch.bfloat16)
    ids2 = hip.moe_route(h2, wr, k, True)[0]
    assert ids2.unique().tolist() == [3, 5]
    assert hip.moe_route(h0, wr, k, True)[0].unique().numel() == E
    inputs = [h0, h1, h2]
    eager = [hip.moe_mlp(x, wr, wgu, wd, k, True) for x in inputs]
    assert not torch.equal(eager[0], eager[1])
    ws = hip.moe_workspace(T, H, I, E, k, "cuda")
    static_h = h0.clone()
    static_out = torch.empty_like(static_h)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        hip.moe_mlp(static_h, wr, wgu, wd, k, True, workspace=ws, out=static_out)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.moe_mlp(static_h, wr, wgu, wd, k, True, workspace=ws, out=static_out)
    for x, exp in list(zip(inputs, eager)) + [(inputs[2], eager[2]), (inputs[0], eager[0])]:
        static_h.copy_(x)
        graph.replay()
        first = static_out.clone()
        graph.replay()
        assert torch.equal(first, exp) and torch.equal(static_out, first)


def test_bad_arguments_are_refused(hip):
    H, I, E, k = SHAPES[0]
    h, wr, wgu, wd = (t.cuda() for t in _random_case(SHAPES[0], 4, 51))
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp(h, wr, wgu, wd, E + 1, True)
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp(h, wr, wgu, wd, k, True, workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(hip.HipOpsError):
        hip.moe_mlp(h.float(), wr, wgu, wd, k, True)
    assert not hip.moe_supported(2048, 800, 128, 8) and hip.moe_supported(2048, 768, 128, 8)
