"""The block-scaled FP8 weight format (dmcp/ops/reference.py: block_fp8_quant,
block_fp8_dequant, moe_mlp_w8) on the CPU, and the evidence that the GPU
numerics bound of tests/test_gpu_moe_w8.py means something: five readers that
take a scale from the wrong place each miss that bound -- r <= 2 r_loop, r the
largest |err| / B against the fp64 oracle over the exactly dequantised weights,
r_loop the figure of the bf16 torch loop over the weights dequantised and
rounded to bf16 -- on every numerics case (the bf16 loop runs on the CPU here).

The inputs (shared with the GPU test, which imports them from here): the
shapes and seeds of tests/test_gpu_moe.py's numerics cases plus one with a
half K block and a half N block ((320, 192, 8, 2)); each 128 x 128 block of the
expert weights is multiplied by 2^u, u in -3..3 drawn from the seed, before
quantising, so neighbouring blocks' scales differ by factors, not per cents.

The wrong readers, as a kernel would commit them (a flat index into the
expert's scale table, per weight row n and 64-deep chunk c of the K loop):

    ignored      every scale 1
    transposed   s[k // 128, n // 128] of the projection's table
    gate_for_up  the gate's block row for the up rows
    late_block   the K block of the previous chunk, (c - 1) // 2, at a block edge
    one_matrix   s_gu's block rows counted through gate and up as one 2I-row
                 matrix, (I + n) // 128 for an up row

At I a multiple of 128 ``one_matrix`` is the definition itself (asserted);
it can only be wrong, and is shown to miss the bound, at I = 192.
"""
import pytest
import torch

from tests.test_gpu_moe import NUM_CASES, _fp64_oracle, _random_case, _torch_loop

W8_NUM_CASES = list(NUM_CASES) + [((320, 192, 8, 2), 130, True, 15)]
READERS = ("ignored", "transposed", "gate_for_up", "late_block", "one_matrix")
B = 128


def _blocks(n):
    return -(-n // B)


def _expand(s, rows, cols):
    return s.repeat_interleave(B, dim=-2)[..., :rows, :].repeat_interleave(B, dim=-1)[..., :cols]


_CASES = {}


def w8_case(shape, T, seed):
    """h, router (bf16) and the quantised experts (w_gu8, s_gu, w_down8, s_down)
    of one numerics case; computed once and left unchanged."""
    key = (shape, T, seed)
    if key not in _CASES:
        from dmcp.ops import reference
        H, I, E, k = shape
        h, wr, wgu, wd = _random_case(shape, T, seed)
        g = torch.Generator().manual_seed(seed + 7000)

        def quant(w):  # [E, N, K] bf16 -> each block times 2^u, then e4m3 + scales
            u = torch.randint(-3, 4, (w.shape[0], _blocks(w.shape[1]), _blocks(w.shape[2])), generator=g)
            return reference.block_fp8_quant(w.float() * _expand(2.0 ** u.float(), w.shape[1], w.shape[2]))
        g8, gs = quant(wgu[:, :I])
        u8, us = quant(wgu[:, I:])
        d8, ds = quant(wd)
        _CASES[key] = (h, wr, (torch.cat([g8, u8], 1).contiguous(), torch.cat([gs, us], 1).contiguous(), d8, ds))
    return _CASES[key]


def _read(reader, w8, s, gate_up):
    """fp32 weights [E, N, K] as ``reader`` dequantises them; ``gate_up``: the
    stacked [E, 2I, K] tensor with s [E, 2 nbI, nbK]."""
    E, rows, K = w8.shape
    N = rows // 2 if gate_up else rows
    nbn, nbk = _blocks(N), _blocks(K)
    per_expert = s.shape[1] * s.shape[2]
    n = torch.arange(rows)
    f, nloc = (n // N, n % N) if gate_up else (torch.zeros_like(n), n)
    c = torch.arange(K // 64)
    kb = (c // 2)[None, :]
    base = (f * nbn)[:, None]          # the projection's first block row
    nb = (nloc // B)[:, None]
    if reader == "ignored":
        return w8.float()
    if reader == "right":
        idx = (base + nb) * nbk + kb
    elif reader == "transposed":
        idx = base * nbk + (kb * nbk + nb) % (nbn * nbk)
    elif reader == "gate_for_up":
        idx = nb * nbk + kb
    elif reader == "late_block":
        idx = (base + nb) * nbk + ((c - 1).clamp(min=0) // 2)[None, :]
    elif reader == "one_matrix":
        idx = (n // B)[:, None] * nbk + kb
    else:
        raise AssertionError(reader)
    idx = idx.expand(rows, K // 64)
    flat = s.reshape(E, per_expert)
    sc = flat[:, idx.reshape(-1)].reshape(E, rows, K // 64).repeat_interleave(64, dim=-1)
    return w8.float() * sc


# ---------------------------------------------------------------- the format
def test_round_trip_error_is_within_an_e4m3_step_of_the_block_amax():
    from dmcp.ops import reference
    g = torch.Generator().manual_seed(3)
    for shape in ((256, 384), (192, 320), (3, 192, 320)):
        w = torch.randn(shape, generator=g) * torch.exp(2.0 * torch.randn(shape, generator=g))
        w8, s = reference.block_fp8_quant(w)
        assert w8.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and w8.shape == w.shape
        assert tuple(s.shape) == tuple(shape[:-2]) + (_blocks(shape[-2]), _blocks(shape[-1]))
        back = reference.block_fp8_dequant(w8, s)
        assert back.dtype == torch.float32
        amax = _expand(s * 448.0, shape[-2], shape[-1])
        assert bool(((back - w).abs() <= amax * 2.0 ** -4).all())
        assert float(w8.float().abs().max()) <= 448.0
        assert reference.block_fp8_dequant(w8, s, torch.bfloat16).dtype == torch.bfloat16


def test_partial_blocks_take_their_own_scales():
    from dmcp.ops import reference
    w = torch.ones(192, 320)
    w[128:, :] = 7.0       # the 64-row edge blocks
    w[:, 256:] *= 0.5      # the 64-column edge blocks
    w8, s = reference.block_fp8_quant(w)
    assert tuple(s.shape) == (2, 3)
    assert torch.equal(s * 448.0, torch.tensor([[1.0, 1.0, 0.5], [7.0, 7.0, 3.5]]))
    assert bool((w8.float() == 448.0).all())
    assert torch.equal(reference.block_fp8_dequant(w8, s), w)


def test_an_all_zero_block_has_scale_one():
    from dmcp.ops import reference
    w = torch.randn(256, 256, generator=torch.Generator().manual_seed(4))
    w[128:, :128] = 0.0
    w8, s = reference.block_fp8_quant(w)
    assert float(s[1, 0]) == 1.0 and bool(torch.isfinite(s).all())
    back = reference.block_fp8_dequant(w8, s)
    assert bool((back[128:, :128] == 0).all()) and bool(torch.isfinite(back).all())


def test_values_are_clamped_not_nan():
    """amax / 448 * 448 may round above 448: the clamp keeps e4m3fn (no inf) off its NaN."""
    from dmcp.ops import reference
    w = torch.full((128, 128), 1e-3)
    w[0, 0] = 3.3333
    w8, s = reference.block_fp8_quant(w)
    assert bool(torch.isfinite(w8.float()).all()) and float(w8.float().abs().max()) == 448.0


def test_dequant_refuses_wrong_shapes_and_dtypes():
    from dmcp.ops import reference
    w8, s = reference.block_fp8_quant(torch.ones(192, 320))
    with pytest.raises(ValueError, match="scale_inv"):
        reference.block_fp8_dequant(w8, s[:, :2])
    with pytest.raises(ValueError, match="float8_e4m3fn"):
        reference.block_fp8_dequant(w8.view(torch.uint8), s)


# ------------------------------------------------------------------- the op
@pytest.mark.parametrize("shape,T,seed", [((256, 128, 8, 2), 33, 5), ((320, 192, 8, 2), 17, 6)])
def test_moe_mlp_w8_is_moe_mlp_on_the_dequantised_fp32_weights(shape, T, seed):
    from dmcp.ops import reference
    H, I, E, k = shape
    h, wr, (g8, gs, d8, ds) = w8_case(shape, T, seed)
    nbi = _blocks(I)
    wgu = torch.cat([reference.block_fp8_dequant(g8[:, :I], gs[:, :nbi]),
                     reference.block_fp8_dequant(g8[:, I:], gs[:, nbi:])], 1)
    wd = reference.block_fp8_dequant(d8, ds)
    assert wgu.dtype == torch.float32 and not torch.equal(wgu, wgu.to(torch.bfloat16).float())
    assert torch.equal(_read("right", g8, gs, True), wgu) and torch.equal(_read("right", d8, ds, False), wd)
    got = reference.moe_mlp_w8(h, wr, g8, gs, d8, ds, k, True)
    exp = reference.moe_mlp(h, wr, wgu, wd, k, True)   # moe_mlp's own .float() leaves fp32 weights as they are
    assert got.dtype == torch.bfloat16 and torch.equal(got, exp)
    # the add_rmsnorm contract, as moe_mlp's
    g = torch.Generator().manual_seed(seed)
    resid = torch.randn(T, H, generator=g).to(torch.bfloat16)
    nw = (1.0 + 0.25 * torch.randn(H, generator=g)).to(torch.bfloat16)
    r1, r2 = resid.clone(), resid.clone()
    out = reference.moe_mlp_w8(h, wr, g8, gs, d8, ds, k, True, residual=r1, norm_w=nw, eps=1e-6)
    assert torch.equal(out, reference.add_rmsnorm(got, nw, 1e-6, residual=r2)) and torch.equal(r1, r2)
    r3 = resid.clone()
    assert reference.moe_mlp_w8(h, wr, g8, gs, d8, ds, k, True, residual=r3) is r3 and torch.equal(r3, r2)
    with pytest.raises(ValueError):
        reference.moe_mlp_w8(h, wr, g8, gs[:, :1], d8, ds, k, True)
    with pytest.raises(ValueError):
        reference.moe_mlp_w8(h, wr, g8.view(torch.uint8), gs, d8, ds, k, True)


def test_device_ops_dispatch():
    from dmcp import ops
    assert "moe_mlp_w8" in ops.DEVICE_OPS
    h, wr, w8 = w8_case((256, 128, 8, 2), 33, 5)
    assert torch.equal(ops.moe_mlp_w8(h, wr, *w8, 2, True), ops.reference.moe_mlp_w8(h, wr, *w8, 2, True))


# -------------------------------------------------- what the GPU bound catches
@pytest.mark.parametrize("shape,T,norm,seed", W8_NUM_CASES)
def test_wrong_scale_readers_miss_the_gpu_bound(shape, T, norm, seed):
    from dmcp.ops import reference
    H, I, E, k = shape
    h, wr, (g8, gs, d8, ds) = w8_case(shape, T, seed)
    wgu, wd = reference.moe_w8_dequant(g8, gs, d8, ds)
    ids, p, y, Bd, keep, _ = _fp64_oracle(h, wr, wgu, wd, k, norm)
    assert int((~keep).sum()) <= 0.02 * T, "the reference alone must meet the exclusion cap"
    Bk = Bd[keep] + 1e-30

    def figure(out):
        return ((out.double()[keep] - y[keep]).abs() / Bk).max().item()
    r_loop = figure(_torch_loop(h, wgu.to(torch.bfloat16), wd.to(torch.bfloat16), ids, p.float()))
    r_right = figure(reference.moe_mlp_w8(h, wr, g8, gs, d8, ds, k, norm))
    print(f"moe w8 readers {shape} T={T}: bf16 loop {r_loop:.3e}, definition (fp32, bf16 act and m) {r_right:.3e}")
    assert r_right <= 2 * r_loop  # the definition itself meets the bound the kernel is held to
    for reader in READERS:
        bad_gu, bad_d = _read(reader, g8, gs, True), _read(reader, d8, ds, False)
        if reader == "one_matrix" and I % B == 0:
            assert torch.equal(bad_gu, wgu)  # not a wrong reader at this width: the definition
            continue
        assert not torch.equal(bad_gu, wgu) or not torch.equal(bad_d, wd)
        r = figure(reference.moe_mlp(h, wr, bad_gu, bad_d, k, norm))
        print(f"    reader {reader}: {r:.3e} ({r / r_loop:.0f}x the loop)")
        assert r > 2 * r_loop, (reader, r, r_loop)
