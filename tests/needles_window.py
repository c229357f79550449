"""Needle-key inputs for sliding-window attention, shared by
tests/test_attention_needles_window.py (CPU: does the harness discriminate?)
and tests/test_gpu_attention_needles_window.py (GPU: do the kernels cut the
logical sequence at the right key?).

Built on tests/needles.py: the same constants (C1, DECOY_GAIN, MARKER,
SINGLE_MIN) and the same REL / ABS bound from a second fp64 pass with |V|.

A query row of live length L under a window W sees keys [lo, L), lo =
max(0, L - W), of its logical sequence (keys [0, P) in the prefix slot, keys up
to the fork end in the parent slot, the rest in its own slot).  Per probed row:

* head 0 of every kv head is aimed at the FIRST visible key lo (q = C1 K[lo]);
  the other heads at the row's own key L - 1, the middle of the window and key
  max(lo, L - 2) -- every head's output is its target's V row;
* logical position lo - 1 -- the last key the row must NOT see, wherever it is
  stored -- holds a decoy: K = 1.5 x K[lo], V = MARKER.  A reader whose window
  starts one key early hands the marker to head 0; one that starts a key late
  loses the needle;
* every cache position outside the logical sequence holds the decoys of
  tests/needles.py (1.5 x key j mod L, V = MARKER).

The weight condition (each target holds >= SINGLE_MIN of its head's fp64
softmax over [lo, L)) is asserted on the inputs before any kernel runs.

Decode rows each get a sequence of their own (their decoys differ); a prefill
probes every third token (the decoy of one probe is then never the first
visible key of another), the tokens between carry random queries.
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from dmcp.ops import reference
from dmcp.ops.reference import SharedPrefix
from tests.needles import ABS, C1, DECOY_GAIN, MARKER, REL, SINGLE_MIN, Seq

MAXS = 512
KVS = ("bf16", "fp8", "fp8s")
WINDOWS = (33, 64, 100)


# ---- the three cache formats ------------------------------------------------
def store(x: torch.Tensor, kv: str):
    """(stored tensor, exponent bytes or None) of fp64 rows x [..., D]."""
    if kv == "fp8s":
        return reference.kv_encode_scaled(x.float())
    return reference.kv_encode(x.float(), torch.uint8 if kv == "fp8" else torch.bfloat16), None


def stored(x: torch.Tensor, kv: str) -> torch.Tensor:
    """x as the cache holds it, decoded to fp64."""
    t, s = store(x, kv)
    return reference.kv_decode_scaled(t, s, torch.float64) if s is not None else reference.kv_float(t).double()


class WCase:
    """Caches (``kc`` / ``vc`` [S, Hkv, MAXS, D], ``ks`` / ``vs`` exponent
    tables for fp8s), queries ``q`` bf16 [R, Hq, D], the window ``W``, the
    sequences, ``row_seq`` / ``row_vis`` [R] and, per sequence, the logical keys
    as stored (``khat`` / ``vhat`` fp64 [Hkv, L, D])."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def scale(self) -> float:
        return 1.0 / math.sqrt(self.D)

    @property
    def kv_scale(self):
        return None if self.ks is None else (self.ks, self.vs)

    def to(self, device) -> "WCase":
        d = dict(self.__dict__)
        for n in ("q", "kc", "vc", "ks", "vs"):
            d[n] = None if d[n] is None else d[n].to(device)
        return WCase(**d)

    def _fp64(self):
        if self.ks is not None:
            return (self.q.double(), reference.kv_decode_scaled(self.kc, self.ks, torch.float64),
                    reference.kv_decode_scaled(self.vc, self.vs, torch.float64))
        return self.q.double(), reference.kv_float(self.kc).double(), reference.kv_float(self.vc).double()

    # -- decode ------------------------------------------------------------
    def decode_inputs(self):
        """(slot, seq_len, prefix, fork) of one decode launch over all rows."""
        dev = self.q.device
        slot = torch.tensor([self.seqs[s].own for s in self.row_seq], dtype=torch.int32, device=dev)
        lens = torch.tensor(self.row_vis, dtype=torch.int32, device=dev)
        pre = None
        on = [s for s in self.seqs if s.P]
        if on:
            P, ps = on[0].P, on[0].prefix
            assert all(s.P == P and s.prefix == ps for s in on)
            rows = torch.tensor([1 if self.seqs[s].P else 0 for s in self.row_seq], dtype=torch.int32, device=dev)
            pre = SharedPrefix(self.kc[ps], self.vc[ps], torch.tensor([P], dtype=torch.int32, device=dev), rows,
                               None if self.ks is None else self.ks[ps], None if self.vs is None else self.vs[ps])
        fork = None
        if any(s.parent is not None for s in self.seqs):
            S = self.kc.shape[0]
            fork = torch.stack([torch.arange(S), torch.zeros(S, dtype=torch.long)], 1).to(torch.int32)
            for s in self.seqs:
                if s.parent is not None:
                    fork[s.own] = torch.tensor([s.parent, s.fend], dtype=torch.int32)
            fork = fork.to(dev).contiguous()
        return slot, lens, pre, fork

    def decode_expected(self):
        """(expected, bound) fp64 [R, Hq, D]: the fp64 reference under the window."""
        slot, lens, pre, fork = self.decode_inputs()
        q, k, v = self._fp64()

        def run(vv):
            p = None if pre is None else SharedPrefix(k[pre_slot], vv[pre_slot], pre.length, pre.rows)
            return reference.decode_attention(q, k, vv, slot, lens, self.scale, prefix=p, fork=fork, window=self.W)
        pre_slot = next((s.prefix for s in self.seqs if s.P), None)
        return run(v), REL * run(v.abs()) + ABS

    # -- prefill -----------------------------------------------------------
    def prefill_tables(self):
        offsets, slots, starts, plens, pslot = [0], [], [], [], None
        for si, s in enumerate(self.seqs):
            rows = [r for r, x in enumerate(self.row_seq) if x == si]
            assert rows and rows[0] == offsets[-1] and self.row_vis[rows[-1]] == s.L
            offsets.append(offsets[-1] + len(rows))
            slots.append(s.own)
            starts.append(self.row_vis[rows[0]] - 1)
            plens.append(s.P)
            pslot = s.prefix if s.P else pslot
        return offsets, slots, starts, pslot, plens

    def prefill_expected(self):
        offsets, slots, starts, pslot, plens = self.prefill_tables()
        q, k, v = self._fp64()

        def run(vv):
            return reference.prefill_attention_varlen(q, k, vv, offsets, slots, starts, pslot, plens, self.scale,
                                                      window=self.W)
        return run(v), REL * run(v.abs()) + ABS

    # -- explicit readers, for mutants ---------------------------------------
    def lo(self, r: int) -> int:
        return max(0, self.row_vis[r] - self.W)

    def attend(self, r: int, keys) -> torch.Tensor:
        """fp64 attention [Hq, D] of row ``r`` over the logical positions ``keys``."""
        si = self.row_seq[r]
        idx = torch.tensor(sorted(set(keys)), dtype=torch.long)
        k, v = self.khat[si][:, idx], self.vhat[si][:, idx]
        G = self.Hq // self.Hkv
        att = torch.einsum("hgd,hld->hgl", self.q[r].double().view(self.Hkv, G, self.D), k) * self.scale
        return torch.einsum("hgl,hld->hgd", torch.softmax(att, -1), v).reshape(self.Hq, self.D)


def targets(lo: int, L: int, Hq: int, G: int) -> list:
    """Head h's target key: the kv head's first query head takes ``lo``."""
    kinds = (lo, L - 1, lo + (L - lo) // 2, max(lo, L - 2))
    return [kinds[(h % G) % 4] if G > 1 else kinds[h % 2] for h in range(Hq)]


def build(D: int, G: int, kv: str, W: int, seqs: list, row_seq: list, row_vis: list, probe: Optional[list] = None,
          seed: int = 0, Hkv: int = 2) -> WCase:
    """The caches and queries of ``seqs`` and R rows: row r is a query of
    sequence ``row_seq[r]`` that sees its first ``row_vis[r]`` keys; probed rows
    (all by default) carry needle heads and put their decoy at lo - 1."""
    g = torch.Generator().manual_seed(seed)
    Hq = Hkv * G
    R = len(row_seq)
    probe = [True] * R if probe is None else probe
    n_slots = 1 + max(x for s in seqs for x in (s.own, s.parent, s.prefix) if x is not None)

    def draw_keys(n):
        k = torch.randn(Hkv, n, D, generator=g, dtype=torch.float64)
        return stored(k * (math.sqrt(D) / k.norm(dim=-1, keepdim=True)), kv)

    khat = [draw_keys(s.L) for s in seqs]
    vhat = [stored(torch.randn(Hkv, s.L, D, generator=g, dtype=torch.float64), kv) for s in seqs]
    # sequences on one prefix slot share their first P keys
    first = {}
    for si, s in enumerate(seqs):
        if s.P:
            o = first.setdefault(s.prefix, si)
            assert seqs[o].P == s.P
            khat[si][:, :s.P], vhat[si][:, :s.P] = khat[o][:, :s.P], vhat[o][:, :s.P]
    # the window decoys, at the logical position below each probed row's window
    shadow = [dict() for _ in seqs]  # per sequence: decoy position -> the key it shadows
    for r in range(R):
        si, L = row_seq[r], row_vis[r]
        lo = max(0, L - W)
        if probe[r] and lo >= 1:
            s = seqs[si]
            shadow[si][lo - 1] = lo
            group = [x for x, o in enumerate(seqs) if lo - 1 < s.P and o.P and o.prefix == s.prefix] or [si]
            for x in group:  # a decoy inside the shared prefix is every sharer's key
                khat[x][:, lo - 1] = stored(DECOY_GAIN * khat[si][:, lo], kv)
                vhat[x][:, lo - 1] = stored(torch.full((Hkv, D), MARKER, dtype=torch.float64), kv)
    # queries, aimed at the keys as they are now stored
    q = torch.randn(R, Hq, D, generator=g).to(torch.bfloat16)
    kvh = torch.arange(Hq) // G
    for r in range(R):
        if not probe[r]:
            continue
        si, L = row_seq[r], row_vis[r]
        lo = max(0, L - W)
        t = targets(lo, L, Hq, G)
        for h in range(Hq):  # a target whose decoy (another probe's) the row sees: the key below it instead
            while t[h] > lo and shadow[si].get(t[h] - 1) == t[h]:
                t[h] -= 1
        t = torch.tensor(t)
        q[r] = (C1 * khat[si][kvh, t]).to(torch.bfloat16)
        att = torch.einsum("hd,hld->hl", q[r].double(), khat[si][kvh][:, lo:L]) / math.sqrt(D)
        w = torch.softmax(att, -1).gather(-1, (t - lo)[:, None])[:, 0]
        assert bool((w >= SINGLE_MIN).all()), f"row {r}: a needle holds only {float(w.min()):.6f} of its window"

    # decoys everywhere (tests/needles.py), then the logical keys over them
    kc = torch.zeros(n_slots, Hkv, MAXS, D, dtype=torch.float64)
    vc = torch.full((n_slots, Hkv, MAXS, D), MARKER, dtype=torch.float64)
    pos = torch.arange(MAXS)
    for si, s in enumerate(seqs):
        for slot in {s.own, s.parent if s.fork_end > s.P else None, s.prefix if s.P else None} - {None}:
            kc[slot] = DECOY_GAIN * khat[si][:, pos % s.L]
    for si, s in enumerate(seqs):
        fe = s.fork_end
        for slot, a, b in ((s.prefix, 0, s.P), (s.parent, s.P, fe), (s.own, fe, s.L)):
            if b > a:
                kc[slot][:, a:b], vc[slot][:, a:b] = khat[si][:, a:b], vhat[si][:, a:b]
    kc, ks = store(kc, kv)
    vc, vs = store(vc, kv)
    # the logical keys exactly as the caches hold them (what every reader is compared on)
    dk = reference.kv_decode_scaled(kc, ks, torch.float64) if ks is not None else reference.kv_float(kc).double()
    dv = reference.kv_decode_scaled(vc, vs, torch.float64) if vs is not None else reference.kv_float(vc).double()
    for si, s in enumerate(seqs):
        for slot, a, b in ((s.prefix, 0, s.P), (s.parent, s.P, s.fork_end), (s.own, s.fork_end, s.L)):
            if b > a:
                khat[si][:, a:b], vhat[si][:, a:b] = dk[slot][:, a:b], dv[slot][:, a:b]
    return WCase(D=D, Hq=Hq, Hkv=Hkv, G=G, kv=kv, W=W, seqs=list(seqs), q=q, kc=kc, vc=vc, ks=ks, vs=vs,
                 row_seq=list(row_seq), row_vis=list(row_vis), probe=probe, khat=khat, vhat=vhat)


# ---- the listed cases -------------------------------------------------------
P_DEC, FEND = 70, 40  # the decode cases' shared prefix (off a 32-key tile edge) and fork end
DECODE_ROWS = ("W-1", "W", "W+1", "W+31", "2W+5", "lo<P", "lo==P", "lo>P", "lo<fork", "lo==fork", "lo>fork")


def decode_case(D: int, G: int, kv: str, W: int, seed: int = 0) -> WCase:
    """One batch of eleven rows, one sequence each: lengths W - 1, W, W + 1,
    W + 31 and 2 W + 5 in their own slots (``prefix.rows`` 0: not on the shared
    prefix), three rows behind the shared prefix of P_DEC keys with lo below P
    (off a tile edge), at P and above P, and three fork branches (parent keys
    below FEND) with lo below, at and above the fork end."""
    seqs, slot = [], 1
    for L in (W - 1, W, W + 1, W + 31, 2 * W + 5):
        seqs.append(Seq(L, slot))
        slot += 1
    for L in (P_DEC + W - 13, P_DEC + W, P_DEC + W + 9):
        seqs.append(Seq(L, slot, P_DEC, 0))
        slot += 1
    for L in (W + 20, W + FEND, W + 55):
        seqs.append(Seq(L, slot, fend=FEND, parent=slot + 1))
        slot += 2
    return build(D, G, kv, W, seqs, list(range(len(seqs))), [s.L for s in seqs], seed=seed)


P_PF = 40
PREFILL_SEQS = ((70, 0, 0), (70, 90, P_PF), (150, 0, 0))  # (T, start, P): two prefills and an extend behind a prefix


def prefill_case(D: int, G: int, kv: str, W: int, seed: int = 0) -> WCase:
    """A pack of three sequences of different lengths: T = 70 and T = 150 from
    start 0 and an extend of 70 tokens at start 90 behind a prefix of P_PF keys
    (the windows of its queries cross P for W = 64 and 100).  Every third token
    is probed."""
    seqs, row_seq, row_vis, probe = [], [], [], []
    for i, (T, start, P) in enumerate(PREFILL_SEQS):
        seqs.append(Seq(start + T, i + 1, P, 0 if P else None))
        for t in range(T):
            row_seq.append(i)
            row_vis.append(start + t + 1)
            probe.append(t % 3 == 0)
    return build(D, G, kv, W, seqs, row_seq, row_vis, probe, seed=seed)


# ---- wrong readers ------------------------------------------------------------
def reader_keys(case: WCase, r: int, kind: str):
    """The logical positions row ``r`` reads under reader ``kind``."""
    s = case.seqs[case.row_seq[r]]
    L, W, lo = case.row_vis[r], case.W, case.lo(r)
    if kind == "true":
        return range(lo, L)
    if kind == "W+1":
        return range(max(0, L - W - 1), L)
    if kind == "W-1":
        return range(max(0, L - W + 1), L)
    if kind == "tile":  # the lower bound rounded down to a 32-key tile
        return range(lo // 32 * 32, L)
    if kind == "own-only":  # W keys counted from the own-slot keys [P, L), the prefix ignored
        return range(s.P + max(0, (L - s.P) - W), L)
    if kind == "prefix":  # the whole prefix left visible
        return list(range(0, min(s.P, L))) + list(range(lo, L))
    if kind == "parent":  # the fork parent's keys left visible
        return list(range(s.P, min(s.fork_end, L))) + list(range(lo, L))
    raise ValueError(kind)


WRONG_READERS = ("W+1", "W-1", "tile", "own-only", "prefix", "parent")
