// Large-tile decode GEMM for steps of 257-1024 rows (gfx950 / MI355X, CDNA4):
//
//   Y[M, N] = X[M, K] . W[N, K]^T      bf16 in, fp32 accumulate
//
// The decode step's row count passes 512 whenever the engine's jump-forward
// rows fill its spare capacity (max_rows = 768 at 512 KV slots).  There the
// projections are compute-bound (a 640-row step is ~1.2 TFLOP over ~2 GB of
// weights) and wgemm.hip's 64-128-row weight tiles re-stage the activation
// rows once per tile: its staged bytes grow with M x N / NB.  This kernel
// keeps wgemm's building blocks (LDS-DMA ring with a counted vmcnt + raw
// barrier per stage, C^T = W . X^T tiles on v_mfma_f32_16x16x32_bf16, the M
// parts of one weight tile on one XCD, fused epilogues) with a 4x larger
// weight tile:
//
//   * a block owns 256 weight rows (SwiGLU: 128 gate + the 128 up rows of the
//     same intermediate columns) x 32 XT activation rows (XT = 2..8), i.e. up
//     to 256 x 256 outputs, over 8 waves (two per SIMD): 4 weight quarters x
//     2 M halves, each 64 weight rows x 16 XT rows (4 A x XT B fragments,
//     16 XT accumulators) -- near-square wave tiles keep the LDS fragment
//     reads (the CU's LDS array served ~90 % of its bandwidth to 128 x 32
//     wave tiles' redundant reads) at (64 + 16 XT) rows per wave and k step.
//     The X rows go in 32-row steps (round 6; 64 before): a 153-row M part
//     stages 160 rows, and (256 + 160) x 128 B stages fit THREE in the LDS
//     where 192 rows fit two -- one stage more in flight;
//   * waves 4-7 (one per SIMD) also issue the block's LDS-DMA: an LDS-DMA
//     instruction holds its wave's issue for ~60-185 cycles
//     (MI355X_MICROARCH.md, cycle constants), and with one wave per SIMD doing
//     both, the 8 pieces per stage ran in series with its MFMAs (v1 of this
//     kernel: 45 % of MFMA time at 1,024 rows); now the SIMD partner keeps
//     issuing MFMAs meanwhile;
//   * 64-deep K stages ([rows][8 x 16 B] images, 8-row 1-KiB LDS-DMA
//     pieces) in a 2-4-stage ring filling the CU's LDS (tstages);
//   * chunk j of row r sits in slot j ^ (r & 7): the 16 lanes of each
//     ds_read_b128 group of the 16x16x32 operand layout (lane (l16, g):
//     row l16, chunk g) cover all 64 banks;
//   * split-K slices of whole stages (any count: the last slice may be
//     shorter) for the narrow projections; the fp32 partials are reduced by
//     splitk_reduce.hip (RoPE + KV append, residual + RMSNorm);
//   * MODE_ARGMAX: the LM head + grammar-masked greedy selection (per block
//     and row one (max, id) pair per 64 vocabulary ids, a per-row
//     reduction kernel selects), no [M, V] logits;
//   * TM_SAMPLE: TM_ARGMAX at a temperature -- each allowed id's value
//     perturbed in the epilogue with Gumbel noise (dmcp_common.hpp
//     gumbel_score) keyed by the row's slot and position.
#include "dmcp_common.hpp"

namespace {

constexpr int TKC = 64;  // K per LDS stage: 128-B image rows, full cache lines per DMA lane group
// ring stages: as many stages as fit the CU's 160 KiB of LDS, at most 6
template <int XT>
constexpr int tstages() {
    return 160 * 1024 / ((256 + 32 * XT) * TKC * 2) < 6 ? 160 * 1024 / ((256 + 32 * XT) * TKC * 2) : 6;
}

// s_waitcnt vmcnt(n * GL) for a runtime n in [0, 5] (the count is an immediate)
// (counts past the 6-bit field are never reached: n <= stages - 2, and a
// ring of that many stages of GL pieces fits the counter; they compile to
// the full wait)
template <int K>
__device__ __forceinline__ void wait_vm_k() {
    if constexpr (K <= 63) asm volatile("s_waitcnt vmcnt(%0)" ::"i"(K) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
template <int GL>
__device__ __forceinline__ void wait_vm(int n) {
    switch (n) {
        case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        case 1: wait_vm_k<GL>(); break;
        case 2: wait_vm_k<2 * GL>(); break;
        case 3: wait_vm_k<3 * GL>(); break;
        case 4: wait_vm_k<4 * GL>(); break;
        default: wait_vm_k<5 * GL>(); break;
    }
}
constexpr int TNB = 256;  // weight rows per block
constexpr int TTH = 512;  // threads per block: 8 waves, two per SIMD
constexpr int TM_BF16 = 0, TM_PART = 1, TM_SWIGLU = 2, TM_ARGMAX = 3, TM_SAMPLE = 4;

// slot of logical 16-B chunk j of image row r (128-B rows, 8 chunks): the
// 16 lanes of each ds_read_b128 group of the 16x16x32 operand layout (lane
// (l16, g): row l16, chunk g of the k step) cover all 64 banks
__device__ __forceinline__ int tslot(int j, int r) { return j ^ (r & 7); }

// PROBE (dmcp_tgemm_probe only; diagnostics of scripts/bench_tgemm.py --probe):
// 1 = the K loop issues no refill DMAs (MFMA + LDS reads + barriers on stale
// stages), 2 = no fragment reads / MFMAs (the DMA ring alone)
//
// Measured slower and removed (git history has the code): an L2 prefetch of
// the weight stream, 32-deep stages, a 2-stage ring cap and a register-weight
// kernel (profiles/tgemm_l2_prefetch_ab_r5.jsonl, profiles/tgemm_regweights_ab_r5.jsonl).
template <int XT, int MODE, int PROBE = 0, bool PENAL = false>
__global__ __launch_bounds__(TTH) __attribute__((amdgpu_waves_per_eu(2, 2))) void tgemm_kernel(
    const uint16_t* __restrict__ x, const uint16_t* __restrict__ w, uint16_t* __restrict__ y, float* __restrict__ part,
    int M, int N, int K, int cps, int S, int ntiles, int mparts, int mrows, int I, const uint32_t* __restrict__ masks,
    const int32_t* __restrict__ midx, int n_masks, int wwords, sample_keys_t<MODE == TM_SAMPLE> sk,
    penalty_keys_t<PENAL> pk) {
    constexpr int NF = TNB / 64;       // A fragments per wave (16 weight rows each): a quarter of the tile's rows
    constexpr int RCH = TKC / 8;       // 16-B chunks per image row
    constexpr int PR = 64 / RCH;       // image rows per 1-KiB LDS-DMA piece
    constexpr int MR = 32 * XT;        // staged X rows (XT B fragments of 16 rows per wave, 2 M halves)
    constexpr int WI = TNB / PR / 4;   // pieces per loader wave per stage: weights
    constexpr int XI = MR / PR / 4;    //                                   X rows
    constexpr int GL = WI + XI;        // LDS-DMA instructions per loader wave per stage
    constexpr int WCH = TNB * RCH;     // 16-B chunks of a stage's weight image
    constexpr int SCH = WCH + MR * RCH;  // ... plus the X image
    constexpr int TST = tstages<XT>();
    static_assert(MR % (PR * 4) == 0, "X pieces per loader wave");
    static_assert(TST >= 2 && TST * SCH * 16 <= 160 * 1024, "LDS ring");
    __shared__ uint4 lds[TST * SCH];   // ONE shared array (cdna_hip_programming.md §5 item 4a)

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    // waves 0-3 and 4-7 each cover the 4 SIMDs once: waves 4-7 also issue the
    // block's LDS-DMA (one loader per SIMD), so while a loader waits on its
    // DMA issue its SIMD partner keeps the matrix core busy
    const bool loader = wv >= 4;
    const int lw = wv & 3;                 // loader index
    const int wn = wv & 3, wm = wv >> 2;   // weight quarter (64 rows) x M half (16 XT rows)
    const int l16 = lane & 15, g = lane >> 4;
    // block -> (weight tile nt, K slice s, M part mp): the M parts of one
    // (nt, s) unit share blockIdx % 8 (one XCD) and consecutive dispatch slots
    const int units = ntiles * S;
    int u, mp;
    if ((units & 7) == 0) {
        const int j = blockIdx.x >> 3;
        u = (j / mparts) * 8 + (blockIdx.x & 7);
        mp = j % mparts;
    } else {
        // XCD-contiguous ranges (bijective for any grid; blocks are dealt
        // round-robin over the 8 XCDs): a unit's M parts are consecutive in
        // one XCD's range, so its weight tile is read once from HBM / MALL
        // and hit in that XCD's L2 by the other parts (the LM head: 501
        // units, whose parts had landed on three different XCDs)
        const int nblk = units * mparts, b = blockIdx.x;
        const int xcd = b & 7, q8 = nblk >> 3, r8 = nblk & 7;
        const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
        u = L / mparts;
        mp = L % mparts;
    }
    const int nt = u % ntiles, s = u / ntiles;
    const int chunks_all = K / TKC;
    const int cbeg = s * cps;
    const int chunks = min(chunks_all, cbeg + cps) - cbeg;  // > 0 (host contract)
    const int m_lo = mp * mrows;
    const int m_hi = min(M, m_lo + mrows);
    const int mw = wm * (XT * 16);
    int mtv = (m_hi - m_lo - mw + 15) / 16;  // valid 16-row tiles of this wave (wave-uniform)
    mtv = max(0, min(XT, mtv));

    const int n0 = nt * TNB;
    const int n0h = nt * (TNB / 2);
    // weight row of image row r.  SwiGLU: each 64-row quarter holds 32 gate
    // rows then the 32 up rows of the same intermediate columns, so a wave's
    // gate fragment f and up fragment f + NF / 2 meet in one lane
    auto wrow = [&](int r) -> int {
        if constexpr (MODE == TM_SWIGLU) {
            const int h = r >> 6, i = r & 63;
            return (i < 32 ? 0 : I) + n0h + 32 * h + (i & 31);
        } else {
            return n0 + r;
        }
    };
    // LDS-DMA sources: lane L of a piece fills image row base + L / RCH, slot
    // L % RCH with logical chunk tslot(L % RCH, row) (an involution)
    const uint16_t* wsrc[WI];
    const uint16_t* xsrc[XI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int r = (lw * WI + i) * PR + lane / RCH;
        wsrc[i] = w + (size_t)wrow(r) * K + (size_t)cbeg * TKC + tslot(lane % RCH, r) * 8;
    }
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int r = (lw * XI + i) * PR + lane / RCH;
        xsrc[i] = x + (size_t)min(m_lo + r, M - 1) * K + (size_t)cbeg * TKC + tslot(lane % RCH, r) * 8;
    }
    auto issue = [&](int c, int slot) {
        uint4* base = lds + slot * SCH;
#pragma unroll
        for (int i = 0; i < WI; ++i) glds16(wsrc[i] + c * TKC, base + (lw * WI + i) * 64);
#pragma unroll
        for (int i = 0; i < XI; ++i) glds16(xsrc[i] + c * TKC, base + WCH + (lw * XI + i) * 64);
    };

    f32x4_t acc[NF][XT];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int t = 0; t < XT; ++t) acc[f][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // Per stage TKC / 32 k steps of XT X fragments and NF weight fragments
    // (this wave's 64 weight rows) and NF x XT MFMAs; the next k step's
    // reads are threaded between the current one's MFMAs (pinned: the
    // scheduler would sink each read to its use).
    constexpr int KS = TKC / 32;
    auto compute = [&](const uint4* st) {
        const uint4* wl = st;
        const uint4* xl = st + WCH;
        bf16x8_t a[KS][NF], b[KS][XT];
        auto load = [&](int kk) {
#pragma unroll
            for (int t = 0; t < XT; ++t) {
                const int r = mw + 16 * t + l16;
                b[kk][t] = as_bf16x8(xl[r * RCH + tslot(4 * kk + g, r)]);
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int r = 64 * wn + 16 * f + l16;
                a[kk][f] = as_bf16x8(wl[r * RCH + tslot(4 * kk + g, r)]);
            }
        };
        auto mma = [&](int kk) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
#pragma unroll
                for (int t = 0; t < XT; ++t)
                    acc[f][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk][f], b[kk][t], acc[f][t], 0, 0, 0);
        };
        load(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            if (kk + 1 < KS) load(kk + 1);
            mma(kk);
            if (kk + 1 < KS) {
                constexpr int NR = NF + XT, NM = NF * XT, RM = NM / NR > 0 ? NM / NR : 1;
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one DS read
                    __builtin_amdgcn_sched_group_barrier(0x008, RM, 0);  // RM MFMAs
                }
                __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);      // the rest
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    };

    // TST-stage ring, TST - 1 stages in flight: a loader waits for its pieces
    // of stage c (counted vmcnt: the newer stages stay in flight), one raw
    // barrier (stage c landed for every wave; every wave done with stage
    // c - 1, the slot about to be refilled), the loaders refill it with stage
    // c + TST - 1, everyone computes stage c.  No __syncthreads() in the loop.
    if (loader) {
#pragma unroll
        for (int j = 0; j < TST - 1; ++j)
            if (j < chunks) issue(j, j);
    }
    for (int c = 0; c < chunks; ++c) {
        if (loader) {
            if constexpr ((PROBE & 1) != 0) wait_vm<GL>(0);
            else wait_vm<GL>(min(TST - 2, chunks - 1 - c));
        }
        asm volatile("s_barrier" ::: "memory");
        if ((PROBE & 1) == 0 && loader && c + TST - 1 < chunks) issue(c + TST - 1, (c + TST - 1) % TST);
        if constexpr ((PROBE & 2) == 0) compute(lds + (c % TST) * SCH);
    }

    // epilogue: lane (l16, g) holds Y[row m_lo + mw + 16t + l16][col c0 + 16f + 4g + i]
    // with c0 = n0 + 64 wn (SwiGLU: intermediate column n0h + 32 wn + 16f + 4g + i of f < NF / 2)
    const int c0 = n0 + 64 * wn;
#pragma unroll
    for (int t = 0; t < XT; ++t) {
        if (t >= mtv) continue;
        const int m = m_lo + mw + 16 * t + l16;
        if constexpr (MODE == TM_ARGMAX || MODE == TM_SAMPLE) {
            // TM_SAMPLE perturbs each allowed value (row key once per row, no
            // hash or log for masked ids); a padding row (slot < 0) keeps
            // the empty pair
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            bool live = m < m_hi;
            uint32_t key = 0;
            if constexpr (MODE == TM_SAMPLE) {
                if (live) {
                    const int slot = sk.slots[m];
                    live = slot >= 0;
                    key = gumbel_key(sk.seed, slot, sk.positions[m]);
                }
            }
            if (live) {
                int mr = midx ? midx[m] : 0;
                mr = mr < 0 ? 0 : (mr >= n_masks ? n_masks - 1 : mr);
                const uint32_t* mrow = masks + (size_t)mr * wwords + (c0 >> 5);
                // PENAL: the row's history word beside its mask word (wgemm.hip)
                [[maybe_unused]] const uint32_t* hrow = nullptr;
                if constexpr (PENAL) {
                    hrow = penalty_row(pk, m, mr);
                    if (hrow) hrow += c0 >> 5;
                }
#pragma unroll
                for (int f = 0; f < NF; ++f) {
                    const uint32_t word = mrow[(16 * f + 4 * g) >> 5];
                    [[maybe_unused]] uint32_t hword = 0u;
                    if constexpr (PENAL) hword = hrow ? hrow[(16 * f + 4 * g) >> 5] : 0u;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int c = 16 * f + 4 * g + i;
                        if ((word >> (c & 31)) & 1u) {
                            float v = bf2f(f2bf(acc[f][t][i]));
                            if constexpr (PENAL) {
                                if ((hword >> (c & 31)) & 1u) v = penalize(v, pk.theta, pk.inv_theta, pk.alpha);
                            }
                            if constexpr (MODE == TM_SAMPLE) v = gumbel_score(v, sk.inv_t, key, c0 + c);
                            if (v > bv) { bv = v; bi = c0 + c; }  // columns ascend: strict > keeps the lowest
                        }
                    }
                }
            }
#pragma unroll
            for (int msk = 16; msk < kWave; msk <<= 1) {
                const float ob = __shfl_xor(bv, msk, kWave);
                const int oi = __shfl_xor(bi, msk, kWave);
                if (ob > bv || (ob == bv && oi < bi)) { bv = ob; bi = oi; }
            }
            // one (max, id) pair per 64-id quarter tile and row
            if (m < m_hi && g == 0)
                reinterpret_cast<float2*>(part)[(size_t)(4 * nt + wn) * M + m] = make_float2(bv, __int_as_float(bi));
            continue;
        }
        if (m >= m_hi) continue;
        if constexpr (MODE == TM_SWIGLU) {
#pragma unroll
            for (int f = 0; f < NF / 2; ++f) {
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // gate / up rounded to bf16 as the unfused GEMM output is
                    const float gg = bf2f(f2bf(acc[f][t][i])), uu = bf2f(f2bf(acc[f + NF / 2][t][i]));
                    o[i] = silu(gg) * uu;
                }
                *reinterpret_cast<uint2*>(y + (size_t)m * I + n0h + 32 * wn + 16 * f + 4 * g) = pack4(o);
            }
        } else if constexpr (MODE == TM_PART) {
            float* dst = part + ((size_t)s * M + m) * N + c0 + 4 * g;
#pragma unroll
            for (int f = 0; f < NF; ++f)
                *reinterpret_cast<float4*>(dst + 16 * f) =
                    make_float4(acc[f][t][0], acc[f][t][1], acc[f][t][2], acc[f][t][3]);
        } else {
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float o[4] = {acc[f][t][0], acc[f][t][1], acc[f][t][2], acc[f][t][3]};
                *reinterpret_cast<uint2*>(y + (size_t)m * N + c0 + 16 * f + 4 * g) = pack4(o);
            }
        }
    }
}

template <int MODE, int PROBE = 0, bool PENAL = false>
hipError_t launch_tgemm(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, int M, int N, int K, int S,
                        int mparts, int I, hipStream_t st, const uint32_t* masks, const int32_t* midx, int n_masks,
                        int wwords, const SampleKeys& sk = SampleKeys{}, const PenaltyKeys& pk = PenaltyKeys{}) {
    const auto keys = pick_keys<MODE == TM_SAMPLE>(sk);
    const auto pen = pick_penalty<PENAL>(pk);
    const int ntiles = (MODE == TM_SWIGLU ? 2 * I : N) / TNB;
    const int mrows = (((M + mparts - 1) / mparts) + 15) & ~15;
    // staged X rows in 32-row steps (>= 64)
    int xt = (mrows + 31) / 32;
    xt = xt < 2 ? 2 : xt;
    const int chunks = K / TKC;
    const int cps = (chunks + S - 1) / S;
    const dim3 grid((unsigned)(ntiles * S * mparts));
#define DMCP_TG(XT)                                                                                          \
    tgemm_kernel<XT, MODE, PROBE, PENAL><<<grid, TTH, 0, st>>>(x, w, y, part, M, N, K, cps, S, ntiles, mparts,   \
                                                               mrows, I, masks, midx, n_masks, wwords, keys, pen)
    switch (xt) {
        case 2: DMCP_TG(2); break;
        case 3: DMCP_TG(3); break;
        case 4: DMCP_TG(4); break;
        case 5: DMCP_TG(5); break;
        case 6: DMCP_TG(6); break;
        case 7: DMCP_TG(7); break;
        case 8: DMCP_TG(8); break;
        default: return hipErrorInvalidValue;
    }
#undef DMCP_TG
    return hipGetLastError();
}

}  // namespace

extern "C" {

// Large-tile GEMM.
//   mode 0: y[M, N] bf16 = x . w^T                              (S == 1)
//   mode 1: part[S, M, N] fp32 partials over S K slices of ceil(K / 64 / S) stages
//   mode 2: y[M, I] bf16 = silu(x . w[:I]^T) * (x . w[I:]^T)     (w = [gate; up] [2I, K], S == 1)
//   mode 3: ids[M] = masked argmax of bf16(x . w^T) (w [V = N, K]; part: float2 workspace of N / 64 * M pairs;
//           masks [n_masks, wwords], midx [M]; S == 1)
// Contract (checked by dmcp/ops/hip.py, guarded here): K % 64 == 0, N % 256 == 0 (mode 2: I % 128 == 0),
// rows per M part <= 256, every K slice non-empty.
int dmcp_tgemm(const void* x, const void* w, void* y, void* part, int M, int N, int K, int S, int mparts, int mode,
               int I, const void* masks, const void* midx, int n_masks, int wwords, void* ids, void* stream) {
    if (M <= 0) return 0;
    const int chunks = K / TKC;
    if (!x || !w || S < 1 || mparts < 1 || K <= 0 || K % TKC != 0 || S > chunks ||
        (S - 1) * ((chunks + S - 1) / S) >= chunks || (((M + mparts - 1) / mparts + 15) & ~15) > 256 ||
        (mode == 1 && !part) || (mode != 1 && S != 1) || ((mode == 0 || mode == 2) && !y) ||
        (mode == 2 ? (I <= 0 || I % (TNB / 2) != 0) : (N <= 0 || N % TNB != 0)) ||
        (mode == 3 && (!part || !masks || !ids || n_masks < 1 || wwords < (N + 31) / 32)))
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    auto yy = (uint16_t*)y;
    auto pp = (float*)part;
    auto mk = (const uint32_t*)masks;
    auto mi = (const int32_t*)midx;
    switch (mode) {
        case 0: return launch_tgemm<TM_BF16>(xx, ww, yy, pp, M, N, K, S, mparts, 0, st, nullptr, nullptr, 0, 0);
        case 1: return launch_tgemm<TM_PART>(xx, ww, yy, pp, M, N, K, S, mparts, 0, st, nullptr, nullptr, 0, 0);
        case 2: return launch_tgemm<TM_SWIGLU>(xx, ww, yy, pp, M, 2 * I, K, S, mparts, I, st, nullptr, nullptr, 0, 0);
        case 3: {
            hipError_t e = launch_tgemm<TM_ARGMAX>(xx, ww, nullptr, pp, M, N, K, 1, mparts, 0, st, mk, mi, n_masks,
                                                   wwords);
            if (e != hipSuccess) return e;
            argmax_pairs_kernel<<<(M + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, st>>>(
                (const float2*)part, 4 * (N / TNB), M, (int32_t*)ids);
            return hipGetLastError();
        }
        default: return hipErrorInvalidValue;
    }
}

// mode 3 at a temperature: ids[M] = argmax over the allowed v of
// bf16(x . w^T) * inv_temperature + Gumbel noise keyed by (seed, slots[m],
// positions[m], v) (dmcp_common.hpp); rows with slots[m] < 0 select 0.  Same
// contract, workspace and pair reduction as mode 3.
int dmcp_tgemm_sample(const void* x, const void* w, void* part, int M, int N, int K, int mparts, const void* masks,
                      const void* midx, int n_masks, int wwords, void* ids, const void* slots, const void* positions,
                      unsigned seed, float inv_temperature, void* stream) {
    if (M <= 0) return 0;
    if (!x || !w || mparts < 1 || K <= 0 || K % TKC != 0 || (((M + mparts - 1) / mparts + 15) & ~15) > 256 ||
        N <= 0 || N % TNB != 0 || !part || !masks || !ids || n_masks < 1 || wwords < (N + 31) / 32 || !slots ||
        !positions || !(inv_temperature > 0.f))
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    const SampleKeys sk{(const int32_t*)slots, (const int32_t*)positions, seed, inv_temperature};
    hipError_t e = launch_tgemm<TM_SAMPLE>((const uint16_t*)x, (const uint16_t*)w, nullptr, (float*)part, M, N, K, 1,
                                           mparts, 0, st, (const uint32_t*)masks, (const int32_t*)midx, n_masks,
                                           wwords, sk);
    if (e != hipSuccess) return e;
    argmax_pairs_kernel<<<(M + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, st>>>(
        (const float2*)part, 4 * (N / TNB), M, (int32_t*)ids);
    return hipGetLastError();
}

// mode 3 (inv_temperature == 0; slots / positions / seed unused) or
// dmcp_tgemm_sample (inv_temperature > 0) under a repetition / presence
// penalty: the penalty arguments of dmcp_masked_penal (dmcp_kernels.hip), the
// flags indexed by the mask row.  Same contract, workspace and pair reduction.
int dmcp_tgemm_penal(const void* x, const void* w, void* part, int M, int N, int K, int mparts, const void* masks,
                     const void* midx, int n_masks, int wwords, void* ids, const void* slots, const void* positions,
                     unsigned seed, float inv_temperature, const void* history, int hwords, int n_slots,
                     const void* pslots, const void* prows, int n_rows, float theta, float inv_theta, float alpha,
                     void* stream) {
    if (M <= 0) return 0;
    const bool sample = inv_temperature != 0.f;
    if (!x || !w || mparts < 1 || K <= 0 || K % TKC != 0 || (((M + mparts - 1) / mparts + 15) & ~15) > 256 ||
        N <= 0 || N % TNB != 0 || !part || !masks || !ids || n_masks < 1 || wwords < (N + 31) / 32 ||
        (sample && (!slots || !positions || !(inv_temperature > 0.f))) || !history || !pslots ||
        hwords < (N + 31) / 32 || n_slots <= 0 || (prows && n_rows < n_masks) || !(theta > 0.f) ||
        !(inv_theta > 0.f) || !(alpha == alpha))
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    const SampleKeys sk{(const int32_t*)slots, (const int32_t*)positions, seed, inv_temperature};
    const PenaltyKeys pk{(const uint32_t*)history, (const int32_t*)pslots, (const int32_t*)prows, hwords, n_slots,
                         n_rows, theta, inv_theta, alpha};
    hipError_t e;
    if (sample)
        e = launch_tgemm<TM_SAMPLE, 0, true>((const uint16_t*)x, (const uint16_t*)w, nullptr, (float*)part, M, N, K, 1,
                                             mparts, 0, st, (const uint32_t*)masks, (const int32_t*)midx, n_masks,
                                             wwords, sk, pk);
    else
        e = launch_tgemm<TM_ARGMAX, 0, true>((const uint16_t*)x, (const uint16_t*)w, nullptr, (float*)part, M, N, K, 1,
                                             mparts, 0, st, (const uint32_t*)masks, (const int32_t*)midx, n_masks,
                                             wwords, sk, pk);
    if (e != hipSuccess) return e;
    argmax_pairs_kernel<<<(M + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, st>>>(
        (const float2*)part, 4 * (N / TNB), M, (int32_t*)ids);
    return hipGetLastError();
}

// diagnostics (scripts/bench_tgemm.py --probe): mode-1 partials with a part
// of the kernel switched off -- probe 1: no refill DMAs, 2: no MFMAs (PROBE above)
int dmcp_tgemm_probe(int probe, const void* x, const void* w, void* part, int M, int N, int K, int S, int mparts,
                     void* stream) {
    const int chunks = K / TKC;
    if (M <= 0 || !x || !w || !part || S < 1 || mparts < 1 || K % TKC != 0 || S > chunks ||
        (S - 1) * ((chunks + S - 1) / S) >= chunks || N % TNB != 0 || (((M + mparts - 1) / mparts + 15) & ~15) > 256)
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    auto pp = (float*)part;
    switch (probe) {
        case 1: return launch_tgemm<TM_PART, 1>(xx, ww, nullptr, pp, M, N, K, S, mparts, 0, st, nullptr, nullptr, 0, 0);
        case 2: return launch_tgemm<TM_PART, 2>(xx, ww, nullptr, pp, M, N, K, S, mparts, 0, st, nullptr, nullptr, 0, 0);
        default: return hipErrorInvalidValue;
    }
}

}  // extern "C"
