"""The per-row scaled fp8 KV-cache format (kv_dtype fp8s) on the CPU: the
encoder / decoder of dmcp.ops.reference, the scaled needle harness (every
wrong-exponent mutant must fail the needles' bound before the GPU is asked),
and the CPU LocalLM on a K-biased Qwen2-layout checkpoint."""
import pytest
import torch

from dmcp.models.llm import LocalLM, preset
from dmcp.ops import reference
from tests import needles, needles_scaled


def _e4m3_values(n, seed):
    g = torch.Generator().manual_seed(seed)
    # magnitudes up to 0x7d = 416: the row maximum is the one the test sets
    return torch.randint(0, 126, (n, 64), generator=g, dtype=torch.uint8).view(torch.float8_e4m3fn).float()


def test_round_trip_is_exact_and_the_exponent_minimal():
    for e in (-20, -3, 0, 2, 9):
        x = _e4m3_values(32, e + 50) * 2.0 ** e
        # the row's largest value is e4m3's second largest at this scale: e is the minimal exponent
        # (at exactly 448 * 2^e the MX rule's frexp returns e + 1, in mx_quant and the kernels alike)
        x[:, 0] = 416.0 * 2.0 ** e
        q, s = reference.kv_encode_scaled(x)
        assert torch.equal(reference.kv_decode_scaled(q, s), x)
        assert bool((s.int() - 127 == e).all())
        # one exponent lower would not hold the row
        assert bool((x.abs().amax(-1) / 2.0 ** (e - 1) > reference.FP8_MAX).all())


def test_zero_row_and_large_rows():
    q, s = reference.kv_encode_scaled(torch.zeros(3, 64))
    assert bool((s == 127).all()) and not bool(reference.kv_decode_scaled(q, s).any())
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(16, 64, generator=g) * 2 - 1) * 3000.0
    x[:, 0] = 3000.0
    q, s = reference.kv_encode_scaled(x)
    d = reference.kv_decode_scaled(q, s)
    # e4m3's half step: 2^-4 of the element's binade, at least half the subnormal step of the row's scale
    sc = reference._pow2(s.int() - 127).float()[:, None]
    half = torch.maximum(2.0 ** torch.floor(torch.log2(x.abs().clamp_min(1e-30))) / 16, sc * 2.0 ** -10)
    assert bool(((d - x).abs() <= half).all())
    unit = reference.kv_float(reference.kv_encode(x, torch.uint8))
    assert float(unit.abs().max()) == 448.0 and float(d.abs().max()) >= 2816.0


def test_cpu_model_runs_with_fp8s_and_counts_the_tables():
    cfg = preset("tiny", max_batch=2, max_seq=64, kv_dtype="fp8s")
    m = LocalLM(cfg, device="cpu")
    assert m.k_scale.shape == m.k_cache.shape[:-1] and m.k_scale.dtype == torch.uint8
    out = m.forward_tokens(torch.tensor([256, 65, 66, 67], dtype=torch.int32), 0, 0)
    assert bool(torch.isfinite(out.float()).all())
    rows = 2 * cfg.layers * cfg.max_batch * cfg.n_kv_heads * cfg.max_seq
    assert cfg.kv_bytes() == rows * cfg.head_dim + rows
    fp8 = preset("tiny", max_batch=2, max_seq=64, kv_dtype="fp8")
    assert fp8.kv_bytes() == rows * cfg.head_dim
    for kv in ("fp8", "bf16"):
        assert LocalLM(preset("tiny", max_batch=2, max_seq=64, kv_dtype=kv), device="cpu").k_scale is None
    with pytest.raises(ValueError, match="kv_dtype"):
        LocalLM(preset("tiny", max_batch=2, max_seq=64, kv_dtype="fp4"), device="cpu")
    for knob in ("prefill_dtype", "decode_dtype"):
        with pytest.raises(ValueError, match="LOCAL_LLM_" + knob.upper()):
            LocalLM(preset("tiny", max_batch=2, max_seq=64, kv_dtype="fp8s", **{knob: "fp8"}), device="cpu")
    assert not LocalLM(preset("tiny", max_batch=2, max_seq=64, kv_dtype="fp8s", prefill_dtype="auto"),
                       device="cpu").prefill_fp8


def test_biased_checkpoint_fp8s_beats_fp8(tmp_path):
    """K rows pass 448.  Against the fp32 reference model AND against the
    bf16-cache model's logits, the fp8s logits are closer than fp8's, and within
    twice the fp8 error of the same checkpoint with the bias scaled down until
    nothing saturates (e4m3's relative step does not depend on the scale; 2 is
    the margin for a different rounding pattern)."""
    from tests.kv_scaled_model import biased_checkpoint, max_k, step_errors
    big = biased_checkpoint(str(tmp_path / "big"))
    small = biased_checkpoint(str(tmp_path / "small"), k_bias_scale=10.0)
    assert max_k(big) > 448.0 > max_k(small)
    for against in ("fp32", "bf16"):
        eb = {kv: step_errors(big, kv, "cpu", against=against) for kv in ("fp8", "fp8s")}
        es = step_errors(small, "fp8", "cpu", against=against)
        for step in es:
            print(f"vs {against} {step}: fp8 {eb['fp8'][step]:.4f} fp8s {eb['fp8s'][step]:.4f} "
                  f"fp8 unsaturated {es[step]:.4f}")
            assert eb["fp8s"][step] < eb["fp8"][step]
            assert eb["fp8s"][step] <= 2 * es[step]


def _case_ids():
    ns = needles_scaled
    out = []
    for g in ns.RGEOMS:
        out += [("decode", g, (si, pairs)) for si in range(len(ns.DECODE_SEQS)) for pairs in (False, True)]
        out += [("prefill", g, pc) for pc in ns.PREFILL_CASES]
        out.append(("varlen", g, ()))
    return out


@pytest.mark.parametrize("kind,geom,args", _case_ids(), ids=lambda v: str(v).replace(" ", ""))
def test_scaled_needles_reject_every_wrong_exponent(kind, geom, args):
    """Every case the GPU readers run (tests/needles_scaled.py), through the
    CPU reference: a reader that takes the wrong exponent byte -- each of
    MUTANTS -- misses the needles' bound on at least one head."""
    ns = needles_scaled
    c, kc, vc, ks, vs = getattr(ns, kind + "_case")(*geom, *args)
    expected = (lambda cc: cc.decode_expected()) if kind == "decode" else (lambda cc: cc.prefill_expected())
    exp, bound = expected(c)
    c.check_single_needles(exp)
    assert needles.error_ratio(exp, exp, bound).max() == 0
    for what, mutate in ns.MUTANTS.items():
        if "parent" in what and not ns.shares_keys(c):
            continue  # no key of this case is read from another slot
        mk, mv = mutate(ks, vs, c)
        got, _ = expected(ns.with_decoded(c, kc, vc, mk, mv))
        ratio = float(needles.error_ratio(got, exp, bound).max())
        assert ratio > 1.0, f"{kind} {geom} {args}: mutant '{what}' passes the bound (ratio {ratio:.3f})"
