"""Needle cases (tests/needles.py) re-encoded in the per-row scaled fp8 cache
format (kv_dtype fp8s, dmcp.ops.reference.kv_encode_scaled).

Every cached row gets a deliberately NON-minimal exponent e_min + delta, delta
in {0..3} drawn per (slot, head, position, K or V) and lowered only where the
row would lose a bit (its smallest elements falling under e4m3's subnormal
step), so the decoded values are exactly the fp8 case's: the needle weights
``needles.build`` asserted hold unchanged, and the expected values are the
fp64 reference on the decoded caches with the bound REL, ABS.

``MUTANTS`` are the ways a reader can take the wrong exponent byte; each
returns scale tables that a correct reader of the SAME bytes would have to
see to reproduce the mutant's output.
"""
import torch

from dmcp.ops import reference
from tests import needles
from tests.needles import Seq

# ---- the cases the GPU readers run (tests/test_gpu_kv_scaled.py) and the CPU
# mutant test checks first (tests/test_kv_scaled_reference.py): one list, so
# the harness is shown to discriminate on exactly what the GPU is asked
NMAXS = 512
OWN, PARENT, PREFIX = 0, 1, 2
RGEOMS = [(64, 32, 8), (128, 12, 2)]  # (D, Hq, Hkv)
# own keys with a partial last tile; a shared prefix; the fork point inside a tile, with and without a prefix
DECODE_SEQS = [Seq(257, OWN), Seq(300, OWN, 45, PREFIX), Seq(257, OWN, 0, None, 77, PARENT),
               Seq(300, OWN, 45, PREFIX, 45 + 96, PARENT)]
PREFILL_CASES = [(37, 0, 0), (129, 45, 45), (5, 256, 256)]  # (T, start, P)
VARLEN_P, VARLEN_PSLOT = 100, 5
VARLEN_MIX = [(1, VARLEN_P, VARLEN_P), (157, VARLEN_P, VARLEN_P), (33, 0, 0), (5, 0, 0), (96, 300, 0)]


def decode_case(D, Hq, Hkv, si, pairs):
    """(scaled case, kc, vc, ks, vs) of DECODE_SEQS[si] on the CPU."""
    seq = DECODE_SEQS[si]
    ta, tb = needles.sweep_targets(seq.L, Hq, pairs)
    B = ta.shape[0]
    c = needles.build(D, Hq, Hkv, "fp8", [seq], [0] * B, [seq.L] * B, ta, tb, n_slots=3, maxs=NMAXS,
                      seed=si + pairs)
    return scaled(c, seed=si)


def prefill_case(D, Hq, Hkv, T, start, P):
    ta = needles.prefill_targets(T, start, P, Hq, seed=T + start)
    vis = torch.arange(start + 1, start + T + 1)
    seq = Seq(start + T, OWN, P, PREFIX if P else None)
    c = needles.build(D, Hq, Hkv, "fp8", [seq], [0] * T, vis, ta, n_slots=3, maxs=NMAXS, seed=T + start + D)
    return scaled(c, seed=T)


def varlen_case(D, Hq, Hkv):
    mix = VARLEN_MIX
    seqs = [Seq(st + T, i, pl, VARLEN_PSLOT if pl else None) for i, (T, st, pl) in enumerate(mix)]
    row_seq = torch.cat([torch.full((T,), i) for i, (T, _, _) in enumerate(mix)])
    vis = torch.cat([torch.arange(st + 1, st + T + 1) for T, st, _ in mix])
    ta = torch.cat([needles.prefill_targets(T, st, pl, Hq, seed=i) for i, (T, st, pl) in enumerate(mix)])
    c = needles.build(D, Hq, Hkv, "fp8", seqs, row_seq, vis, ta, n_slots=6, maxs=NMAXS, seed=D + Hq)
    return scaled(c, seed=D)


def scaled(c, seed):
    kc, vc, ks, vs = rescale(c, seed)
    return with_decoded(c, kc, vc, ks, vs), kc, vc, ks, vs


def to(dev, c, kc, vc, ks, vs):
    """A scaled case and its tables on ``dev`` (the fp64 views decoded there)."""
    cd = c.to(dev)
    kc, vc, ks, vs = (t.to(dev) for t in (kc, vc, ks, vs))
    return with_decoded(cd, kc, vc, ks, vs), kc, vc, ks, vs


def shares_keys(c) -> bool:
    return any(s.parent is not None or s.P for s in c.seqs)


def rescale(case: needles.Case, seed: int = 0):
    """(kc, vc, k_scale, v_scale) of ``case`` (built with kv="fp8"): e4m3 bytes
    and exponent bytes whose decoded values equal the case's, on its device."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for cache in (case.kc, case.vc):
        x = reference.kv_float(cache.cpu())
        emin = reference.kv_row_exp(x.abs().amax(-1))
        delta = torch.randint(0, 4, emin.shape, generator=g, dtype=torch.int32)
        q = torch.zeros_like(cache.cpu())
        e = torch.zeros_like(emin)
        done = torch.zeros(emin.shape, dtype=torch.bool)
        for d in (3, 2, 1, 0):
            ed = emin + delta.clamp(max=d)
            qd = (x.double() * reference._pow2(-ed)[..., None]).float().to(torch.float8_e4m3fn)
            ok = ((qd.double() * reference._pow2(ed)[..., None]).float() == x).all(-1) & ~done
            q[ok] = qd.view(torch.uint8)[ok]
            e[ok] = ed[ok]
            done |= ok
        assert bool(done.all())
        s = (e + 127).to(torch.uint8)
        assert torch.equal(reference.kv_decode_scaled(q, s), x)
        out += [q.to(cache.device), s.to(cache.device)]
    return out[0], out[2], out[1], out[3]


def with_decoded(case: needles.Case, kc, vc, ks, vs) -> needles.Case:
    """``case`` whose fp64 views are the caches ``kc`` / ``vc`` decoded with
    the tables ``ks`` / ``vs`` (its *_expected() then use them)."""
    c = needles.Case(**{k: v for k, v in case.__dict__.items() if k != "_f64"})
    c._f64 = (case.q.double(), reference.kv_decode_scaled(kc, ks, torch.float64),
              reference.kv_decode_scaled(vc, vs, torch.float64))
    return c


def _shift(ks, vs, case):
    return torch.roll(ks, 1, -1), torch.roll(vs, 1, -1)


def _swap(ks, vs, case):
    return vs, ks


def _own_for_shared(ks, vs, case):
    ks, vs = ks.clone(), vs.clone()
    for s in case.seqs:
        for other in (s.parent, s.prefix if s.P else None):
            if other is not None:
                ks[other], vs[other] = ks[s.own], vs[s.own]
    return ks, vs


def _next_head(ks, vs, case):
    return torch.roll(ks, -1, 1), torch.roll(vs, -1, 1)


def _ignored(ks, vs, case):
    return torch.full_like(ks, 127), torch.full_like(vs, 127)


MUTANTS = {"shifted by one key": _shift, "K and V tables swapped": _swap,
           "own slot's scales for parent / prefix keys": _own_for_shared, "head h + 1's scales": _next_head,
           "scales ignored": _ignored}
