"""Needle-key inputs for the attention kernels, shared by
tests/test_attention_needles.py (CPU: does the harness discriminate?) and
tests/test_gpu_attention_needles.py (GPU: do the kernels read every key once,
from the right slot?).

With ``randn`` q / K / V the softmax over a few hundred keys is nearly uniform
and one key carries ~1/L of the output: a kernel that drops, repeats or
misplaces a single key passes a 2e-2 comparison.  Here every query head is
aimed at one key (or two), so that the head's output IS that key's V row:

* K rows are ``randn`` normalised to norm sqrt(D), rounded to the cache format;
  V rows are ``randn``.
* a single-needle head targets key n: q = C1 * K[n] (decoded, rounded to
  bf16).  With scale = 1/sqrt(D) the needle scores C1 * sqrt(D) (48 at D = 64),
  every other key ~N(0, C1^2): the needle holds all the weight.
* a two-needle head targets keys a, b: q = (C2 / 2) * (K[a] + K[b]); both keep
  a real share, so split merges, the prefix merge and the online rescale run
  with weight on both sides, and a key counted twice moves the output.
* both weight conditions are asserted on the fp64 softmax of the inputs before
  any kernel runs (:func:`build`); they are conditions on the inputs.
* every cache position a query must not read holds a decoy: K = 1.5 x the
  effective key (j mod L) of the sequence, V = the constant MARKER.  A kernel
  that counts such a position hands the marker to the head aimed at the key it
  shadows.  Decoys are finite: they model a reused slot's stale keys.

One logical sequence of L keys (:class:`Seq`): keys [0, P) live in the
``prefix`` slot, [P, min(fend, L)) in the ``parent`` slot when a fork is
given, the rest in the ``own`` slot.

The expected value is ``dmcp.ops.reference`` evaluated in fp64 on the decoded
caches; the per-element bound is REL * sum_k p_k |V_k[d]| + ABS from a second
fp64 pass with |V|.  The kernels round P to bf16 and the output to bf16 and sum
l unrounded in fp32.  A round-to-nearest bf16 is within 2^-9 of the value's
binade, at most 2^-8 of the value itself, so the two roundings stay within
REL = 2^-7 of sum p |V| in the worst case and within half of it typically.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from dmcp.ops import reference
from dmcp.ops.reference import SharedPrefix

C1, C2 = 6.0, 12.0
DECOY_GAIN, MARKER = 1.5, 7.0
SINGLE_MIN = 1.0 - 2.0 ** -12
PAIR_EACH_MIN, PAIR_SUM_MIN = 0.2, 0.999
REL, ABS = 2.0 ** -7, 1e-3


class Seq(NamedTuple):
    """One logical sequence of ``L`` keys and the slots that hold them."""
    L: int
    own: int
    P: int = 0
    prefix: Optional[int] = None
    fend: int = 0                  # as written to the fork table (may lie past L)
    parent: Optional[int] = None

    @property
    def fork_end(self) -> int:
        """End of the keys actually read from the parent slot."""
        return max(self.P, min(self.fend, self.L)) if self.parent is not None else self.P

    def source(self, j: int) -> int:
        if j < self.P:
            return self.prefix
        return self.parent if j < self.fork_end else self.own


def cache_dtype(kv: str) -> torch.dtype:
    return torch.uint8 if kv == "fp8" else torch.bfloat16


def decode(t: torch.Tensor) -> torch.Tensor:
    """Stored cache values (bf16 or e4m3 bytes) as fp64."""
    return reference.kv_float(t).double()


class Case:
    """Caches, queries and the bookkeeping of one needle input (see :func:`build`).

    ``q`` bf16 [R, Hq, D]; ``kc`` / ``vc`` [S, Hkv, MAXS, D] in the cache
    format; ``row_seq`` / ``row_vis`` int64 [R]: the sequence of each query row
    and how many of its keys the row sees; ``ta`` / ``tb`` int64 [R, Hq]: the
    head's target key(s) (``tb`` -1 = single needle; ``ta`` >= the row's
    ``row_vis`` = a future key the row must NOT see); ``wa`` / ``wb``: the fp64
    softmax weight of each target; ``khat`` / ``vhat``: per sequence, the
    effective keys as stored, decoded to fp64 [Hkv, L, D]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self._f64 = None  # the fp64 views, decoded once

    @property
    def scale(self) -> float:
        return 1.0 / math.sqrt(self.D)

    def to(self, device) -> "Case":
        d = dict(self.__dict__)
        for name in ("q", "kc", "vc", "row_seq", "row_vis", "ta", "tb", "wa", "wb"):
            d[name] = d[name].to(device)
        d["khat"] = [x.to(device) for x in self.khat]
        d["vhat"] = [x.to(device) for x in self.vhat]
        return Case(**d)

    # -- what the heads should return ------------------------------------
    @property
    def single(self) -> torch.Tensor:
        """[R, Hq] bool: single-needle heads whose target the row sees."""
        return (self.tb < 0) & (self.ta < self.row_vis[:, None])

    @property
    def future(self) -> torch.Tensor:
        return self.ta >= self.row_vis[:, None]

    def needle_v(self) -> torch.Tensor:
        """fp64 [R, Hq, D]: the stored V row of each head's first target."""
        out = torch.zeros(self.q.shape, dtype=torch.float64, device=self.q.device)
        kvh = torch.arange(self.Hq, device=self.q.device) // (self.Hq // self.Hkv)
        for si in range(len(self.seqs)):
            rows = (self.row_seq == si).nonzero().flatten()
            if rows.numel():
                out[rows] = self.vhat[si][kvh[None, :], self.ta[rows]]
        return out

    def check_single_needles(self, exp: torch.Tensor) -> None:
        """A check on the test itself: where one key holds weight w, the fp64
        reference differs from that key's V row by sum_{k != n} p_k (V_k - V_n),
        at most 2 (1 - w) max|V|."""
        vmax = max(float(v.abs().max()) for v in self.vhat)
        tol = (2.0 * (1.0 - self.wa).clamp_min(0.0) * vmax + 1e-12)[..., None]
        err = (exp.double() - self.needle_v()).abs()
        sel = self.single
        assert bool((err <= tol)[sel].all()), \
            f"reference is not the needle's V row: max excess {float((err - tol)[sel].max()):.3e}"

    # -- decode launch arguments -----------------------------------------
    def decode_inputs(self):
        """(slot int32 [R], seq_len int32 [R], prefix SharedPrefix or None,
        fork int32 [S, 2] or None) of a decode launch over all rows."""
        dev = self.q.device
        own = torch.tensor([s.own for s in self.seqs], device=dev)
        slot = own[self.row_seq].to(torch.int32)
        lens = self.row_vis.to(torch.int32)
        pre = None
        on = [s for s in self.seqs if s.P]
        if on:
            P, ps = on[0].P, on[0].prefix
            assert all(s.P == P and s.prefix == ps for s in on), "one shared prefix per launch"
            rows = None
            if len(on) < len(self.seqs):
                flag = torch.tensor([1 if s.P else 0 for s in self.seqs], device=dev)
                rows = flag[self.row_seq].to(torch.int32)
            pre = SharedPrefix(self.kc[ps], self.vc[ps], torch.tensor([P], dtype=torch.int32, device=dev), rows)
        fork = None
        if any(s.parent is not None for s in self.seqs):
            S = self.kc.shape[0]
            fork = torch.stack([torch.arange(S), torch.zeros(S, dtype=torch.long)], 1).to(torch.int32)
            for s in self.seqs:
                if s.parent is not None:
                    fork[s.own] = torch.tensor([s.parent, s.fend], dtype=torch.int32)
            fork = fork.to(dev).contiguous()
        return slot, lens, pre, fork

    def _fp64(self):
        if self._f64 is None or self._f64[0].device != self.q.device:
            self._f64 = (self.q.double(), decode(self.kc), decode(self.vc))
        return self._f64

    def decode_expected(self):
        """(expected fp64 [R, Hq, D], bound fp64 [R, Hq, D]) of the decode launch."""
        slot, lens, pre, fork = self.decode_inputs()
        q, k, v = self._fp64()

        def run(vv):
            p = None if pre is None else SharedPrefix(k[self.seqs_prefix_slot()], vv[self.seqs_prefix_slot()],
                                                      pre.length, pre.rows)
            return reference.decode_attention(q, k, vv, slot, lens, self.scale, prefix=p, fork=fork)
        return run(v), REL * run(v.abs()) + ABS

    def seqs_prefix_slot(self) -> int:
        return next(s.prefix for s in self.seqs if s.P)

    # -- prefill launch arguments ----------------------------------------
    def prefill_tables(self):
        """(offsets, slots, starts, prefix slot, prefix lens) of the packed
        prefill over all rows (rows of a sequence are consecutive positions)."""
        offsets, slots, starts, plens = [0], [], [], []
        pslot = None
        for si, s in enumerate(self.seqs):
            rows = (self.row_seq == si).nonzero().flatten()
            vis = self.row_vis[rows]
            assert rows.numel() and int(rows[0]) == offsets[-1] and bool((vis[1:] - vis[:-1] == 1).all())
            assert int(vis[-1]) == s.L and s.parent is None
            offsets.append(offsets[-1] + rows.numel())
            slots.append(s.own)
            starts.append(int(vis[0]) - 1)
            plens.append(s.P)
            if s.P:
                pslot = s.prefix
        return offsets, slots, starts, pslot, plens

    def prefill_expected(self):
        offsets, slots, starts, pslot, plens = self.prefill_tables()
        q, k, v = self._fp64()
        exp = reference.prefill_attention_varlen(q, k, v, offsets, slots, starts, pslot, plens, self.scale)
        mag = reference.prefill_attention_varlen(q, k, v.abs(), offsets, slots, starts, pslot, plens, self.scale)
        return exp, REL * mag + ABS

    # -- an explicit read list, for mutants ------------------------------
    def reads(self, r: int) -> list:
        """[(slot, position)] of the keys row ``r`` reads, in key order."""
        s = self.seqs[int(self.row_seq[r])]
        return [(s.source(j), j) for j in range(int(self.row_vis[r]))]

    def attend(self, r: int, kreads: list, vreads: Optional[list] = None) -> torch.Tensor:
        """fp64 attention [Hq, D] of row ``r`` over an explicit list of cache
        positions (a key listed twice counts twice); ``vreads``: where each
        key's V row is taken from (default: the same positions)."""
        q, k, v = self._fp64()
        G = self.Hq // self.Hkv

        def gather(c, reads):
            sl = torch.tensor([a for a, _ in reads], device=c.device)
            ps = torch.tensor([b for _, b in reads], device=c.device)
            return c[sl, :, ps].transpose(0, 1)  # [Hkv, n, D]
        kk, vv = gather(k, kreads), gather(v, kreads if vreads is None else vreads)
        att = torch.einsum("hgd,hld->hgl", q[r].view(self.Hkv, G, self.D), kk) * self.scale
        return torch.einsum("hgl,hld->hgd", torch.softmax(att, -1), vv).reshape(self.Hq, self.D)


def build(D: int, Hq: int, Hkv: int, kv: str, seqs: list, row_seq, row_vis, ta, tb=None, n_slots: Optional[int] = None,
          maxs: int = 1024, seed: int = 0, c1: float = C1, c2: float = C2) -> Case:
    """Caches and queries (on the CPU) for ``seqs`` and R query rows: row r
    belongs to sequence ``row_seq[r]``, sees its first ``row_vis[r]`` keys and
    its head h targets key ``ta[r][h]`` (and ``tb[r][h]`` where >= 0).

    Sequences that name the same ``prefix`` slot share their first P keys.
    Asserts the weight preconditions on the fp64 softmax of the inputs."""
    cdt = cache_dtype(kv)
    g = torch.Generator().manual_seed(seed)
    G = Hq // Hkv
    assert Hq == G * Hkv
    n_slots = n_slots or 1 + max(x for s in seqs for x in (s.own, s.parent, s.prefix) if x is not None)
    row_seq = torch.as_tensor(row_seq, dtype=torch.int64)
    row_vis = torch.as_tensor(row_vis, dtype=torch.int64)
    ta = torch.as_tensor(ta, dtype=torch.int64)
    tb = torch.full_like(ta, -1) if tb is None else torch.as_tensor(tb, dtype=torch.int64)
    R = row_seq.numel()
    assert ta.shape == (R, Hq) and tb.shape == (R, Hq) and row_vis.shape == (R,)

    q = torch.zeros(R, Hq, D, dtype=torch.bfloat16)
    wa = torch.zeros(R, Hq, dtype=torch.float64)
    wb = torch.zeros(R, Hq, dtype=torch.float64)
    kvh = (torch.arange(Hq) // G)[None, :]

    def draw_keys(*shape):
        k = torch.randn(*shape, D, generator=g, dtype=torch.float64)
        return decode(reference.kv_encode(k * (math.sqrt(D) / k.norm(dim=-1, keepdim=True)), cdt))

    def aim(k, a, b, vis):
        """(q bf16, weight of a, weight of b) of heads aimed at keys a (and b) of k."""
        ka, kb = k[kvh, a], k[kvh, b.clamp_min(0)]
        qs = torch.where((b >= 0)[..., None], (c2 / 2) * (ka + kb), c1 * ka).to(torch.bfloat16)
        att = torch.einsum("rhgd,hld->rhgl", qs.double().view(-1, Hkv, G, D), k) / math.sqrt(D)
        att = att.reshape(a.shape[0], Hq, k.shape[1])
        hidden = torch.arange(k.shape[1])[None, None, :] >= vis[:, None, None]
        lse = torch.logsumexp(att.masked_fill(hidden, float("-inf")), -1)
        sa = att.gather(-1, a[..., None])[..., 0]
        sb = att.gather(-1, b.clamp_min(0)[..., None])[..., 0]
        # a future key: the weight it WOULD take if the row saw it too (a leak is visible)
        w_a = torch.where(a >= vis[:, None], torch.sigmoid(sa - lse), torch.exp(sa - lse))
        return qs, w_a, torch.where(b >= 0, torch.exp(sb - lse), torch.zeros_like(sb))

    # effective keys as stored, the queries aimed at them, and their fp64 softmax weights
    khat, vhat, prefix_owner = [], [], {}
    shared = {s.prefix for s in seqs if s.P and sum(1 for o in seqs if o.P and o.prefix == s.prefix) > 1}
    for si, s in enumerate(seqs):
        assert 0 < s.L <= maxs and 0 <= s.P <= s.L and (s.P == 0 or s.prefix is not None)
        k = draw_keys(Hkv, s.L)
        v = decode(reference.kv_encode(torch.randn(Hkv, s.L, D, generator=g, dtype=torch.float64), cdt))
        if s.P:
            first = prefix_owner.setdefault(s.prefix, si)
            if first != si:
                assert seqs[first].P == s.P, "sequences on one prefix slot share one prefix"
                k[:, :s.P], v[:, :s.P] = khat[first][:, :s.P], vhat[first][:, :s.P]
        khat.append(k)
        vhat.append(v)
        rows = (row_seq == si).nonzero().flatten()
        if not rows.numel():
            continue
        a, b, vis = ta[rows], tb[rows], row_vis[rows]
        assert bool((vis >= 1).all()) and bool((vis <= s.L).all())
        assert bool((a >= 0).all()) and bool((a < s.L).all()) and bool((b < vis[:, None]).all())
        assert bool(((b < 0) | (a < vis[:, None])).all()), "a two-needle head targets visible keys"
        for _ in range(64):
            q[rows], wa[rows], wb[rows] = aim(k, a, b, vis)
            # Among the thousands of pairs of an exhaustive sweep a few keys
            # point nearly away from each other (K[a] + K[b] is short) and a
            # third key outscores them.  Such a key is drawn again -- still a
            # random direction of norm sqrt(D) -- until the pair conditions
            # hold; what is asserted below is unchanged.
            weak = (b >= 0) & ((wa[rows] < PAIR_EACH_MIN) | (wb[rows] < PAIR_EACH_MIN) |
                               (wa[rows] + wb[rows] < PAIR_SUM_MIN))
            if not bool(weak.any()) or s.prefix in shared:
                break
            hh, kk = kvh.expand_as(a)[weak], a[weak]
            k[hh, kk] = draw_keys(hh.numel())

    # decoys everywhere, then the real keys over them
    kc = torch.zeros(n_slots, Hkv, maxs, D, dtype=cdt)
    vc = reference.kv_encode(torch.full((n_slots, Hkv, maxs, D), MARKER, dtype=torch.float64), cdt)
    users: dict = {}
    for si, s in enumerate(seqs):
        for slot in (s.own, s.parent if s.fork_end > s.P else None, s.prefix if s.P else None):
            if slot is not None and si not in users.setdefault(slot, []):
                users[slot].append(si)
    pos = torch.arange(maxs)
    for slot, us in users.items():
        for i, si in enumerate(us):  # several users (a shared prefix slot): positions dealt round-robin
            sel = pos[pos % len(us) == i]
            kc[slot][:, sel] = reference.kv_encode(DECOY_GAIN * khat[si][:, sel % seqs[si].L], cdt)
    for si, s in enumerate(seqs):
        fe = s.fork_end
        for slot, a, b in ((s.prefix, 0, s.P), (s.parent, s.P, fe), (s.own, fe, s.L)):
            if b > a:
                kc[slot][:, a:b] = reference.kv_encode(khat[si][:, a:b], cdt)
                vc[slot][:, a:b] = reference.kv_encode(vhat[si][:, a:b], cdt)

    # the weight preconditions: conditions on the inputs, before any kernel runs
    pair = tb >= 0
    assert bool((wa[~pair] >= SINGLE_MIN).all()), f"single needle holds only {float(wa[~pair].min()):.6f}"
    if bool(pair.any()):
        assert bool((wa[pair] >= PAIR_EACH_MIN).all()) and bool((wb[pair] >= PAIR_EACH_MIN).all()), \
            f"a needle of a pair holds only {float(torch.minimum(wa[pair], wb[pair]).min()):.4f}"
        assert bool(((wa + wb)[pair] >= PAIR_SUM_MIN).all()), \
            f"a needle pair holds only {float((wa + wb)[pair].min()):.6f}"
    return Case(D=D, Hq=Hq, Hkv=Hkv, kv=kv, maxs=maxs, seqs=list(seqs), q=q, kc=kc, vc=vc, row_seq=row_seq,
                row_vis=row_vis, ta=ta, tb=tb, wa=wa, wb=wb, khat=khat, vhat=vhat)


# ---- target plans ---------------------------------------------------------
def sweep_targets(L: int, Hq: int, pairs: bool = False):
    """The exhaustive decode sweep: B = ceil(L / Hq) rows of one sequence,
    head h of row b targets key (b Hq + h) mod L -- every key position is some
    head's needle.  ``pairs``: key j paired with key (j + L // 2) mod L."""
    B = -(-L // Hq)
    ta = (torch.arange(B * Hq) % L).view(B, Hq)
    if not pairs or L < 2:
        return ta, None
    return ta, (ta + L // 2) % L


PREFILL_KINDS = ("diag", "diag-1", "zero", "P-1", "P", "start-1", "start", "tile", "tile-1", "random", "future")


def prefill_targets(T: int, start: int, P: int, Hq: int, seed: int = 0) -> torch.Tensor:
    """ta [T, Hq] for one prefill of T tokens at positions [start, start + T):
    token t / head h takes kind (t Hq + h) mod 11 of PREFILL_KINDS, or the next
    kind that exists for it.  "future" (the key after the query's own) is
    returned as a target past the row's visible keys."""
    g = torch.Generator().manual_seed(seed)
    ta = torch.zeros(T, Hq, dtype=torch.int64)
    for t in range(T):
        pos = start + t
        tile = pos // 32 * 32
        rnd = torch.randint(0, pos + 1, (Hq,), generator=g).tolist()
        for h in range(Hq):
            cand = (pos, pos - 1, 0, P - 1 if P else -1, P if P else -1, start - 1, start, tile, tile - 1, rnd[h],
                    pos + 1 if t + 1 < T else -1)
            i = (t * Hq + h) % len(cand)
            while cand[i] < 0:
                i = (i + 1) % len(cand)
            ta[t, h] = cand[i]
    return ta


# ---- the comparison ---------------------------------------------------------
def error_ratio(got: torch.Tensor, exp: torch.Tensor, bound: torch.Tensor) -> torch.Tensor:
    """|got - expected| / bound per element (fp64); non-finite output counts as inf."""
    r = (got.double() - exp.double()).abs() / bound
    return torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf")))


def assert_within_bound(got: torch.Tensor, exp: torch.Tensor, bound: torch.Tensor, what: str = "") -> float:
    """Every element within its bound; returns the largest error / bound."""
    r = error_ratio(got, exp, bound)
    worst = float(r.max())
    if worst > 1.0:
        idx = tuple(int(i) for i in (r == r.max()).nonzero()[0])
        raise AssertionError(f"{what}: error / bound = {worst:.3g} at (row, head, d) = {idx}: got "
                             f"{float(got[idx]):.6g}, expected {float(exp[idx]):.6g}, bound {float(bound[idx]):.3g}; "
                             f"{int((r > 1).any(-1).sum())} heads over the bound")
    return worst
