// Weight-streaming GEMM for the decode step (gfx950 / MI355X, CDNA4):
//
//   Y[M, N] = X[M, K] . W[N, K]^T      bf16 in, fp32 accumulate,  M <= 512
//
// At the enrichment operating point (256 sequences + jump-forward rows, ~300
// rows per step) every projection streams its whole weight matrix from HBM
// once per step while the activations are a few MB (L2-resident).
// hipBLASLt tiles M in 64-row blocks spread over all 8 XCDs, so each weight
// tile leaves HBM once per M tile: 0.6-2 TB/s of weight traffic at 320 rows
// (profiles/decode_step_320rows_fp8_r3_kernel_stats.csv: 91 us of GEMMs per
// layer against ~20 us at the HBM roofline).  Here:
//
//   * a block owns NB weight rows (64, or 128 = 64 gate + 64 up rows of the
//     same intermediate columns) and ALL rows of its M part: the weight tile
//     is read once and the M parts of one tile run on the SAME XCD (block
//     ids congruent mod 8, dispatched back to back), so the second part's
//     read is an L2 hit;
//   * both operands reach LDS by LDS-DMA (global_load_lds_dwordx4: full
//     128-B lines, no VGPR round trip) into a 3-stage ring of 64-deep K
//     chunks, two stages in flight while one is computed, one counted
//     vmcnt + raw barrier per chunk -- HBM latency needs ~60 KB in flight
//     per CU and a block's compute per chunk is a fraction of one latency;
//     with register-direct X loads every X wait also waited for the weight
//     loads issued before it (vmcnt retires in order): 2x slower than
//     hipBLASLt;
//   * LDS images are [rows][8 x 16 B] with chunk j of row r in slot
//     j ^ (r & 7) (the swizzle applied on the DMA's source address):
//     conflict-free ds_read_b128 of both MFMA operands;
//   * v_mfma_f32_16x16x32_bf16: A = 16 weight rows x 32 k, B = 32 k x 16 X
//     rows, C = Y^T tile (lane: 4 consecutive output columns of one row);
//   * the bound (profiles/wgemm_parts_r3.txt): each CU ingests its weight
//     tile at ~23 KB/us and its activation rows at ~42 KB/us through the
//     same load path, t ~= W_block / 23 + X_block / 42 (KB, us); 64 / 128
//     weight rows x the M part already minimise that for ~256 blocks;
//   * split-K (S > 1) writes fp32 partials, reduced by splitk_reduce.hip's
//     fused consumers (residual + RMSNorm of the next op; RoPE + KV append);
//     MODE_SWIGLU writes silu(gate) * up directly (no gate/up activation in
//     HBM, no SwiGLU launch);
//   * MODE_ARGMAX is the LM head + the grammar-masked greedy selection: each
//     block reduces its tile's vocabulary columns of every row to one
//     (max, id) pair under the row's mask bitset (the grammar state's mask
//     row), a tiny kernel reduces the pairs per row -- the [rows, vocab]
//     logits never exist (at 128,256 ids and 512 rows: 131 MB written and
//     read back per step by F.linear + masked_argmax);
//   * MODE_SAMPLE is MODE_ARGMAX at a temperature: the same tiles and pairs,
//     each allowed id's value perturbed in the epilogue with Gumbel noise
//     (dmcp_common.hpp gumbel_score) keyed by the row's slot and position;
//   * PENAL (either selection mode): the repetition / presence penalty
//     (dmcp_common.hpp penalize).  The row's history word is read where its
//     mask word is -- history + slot * hwords + (n0 >> 5), once per row and
//     32 ids -- and an allowed id whose bit is set competes with its
//     penalised value (before the noise); ids the grammar excludes cost
//     nothing more.
#include "dmcp_common.hpp"

namespace {

constexpr int kKC = 64;  // K per LDS stage
constexpr int MODE_BF16 = 0, MODE_PART = 1, MODE_SWIGLU = 2, MODE_ARGMAX = 3, MODE_SAMPLE = 4;

template <int NB, int MT, int MR, int MODE, int ST, int AUXW = 0, bool PENAL = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(1, 1))) void wgemm_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ w,
                                                       uint16_t* __restrict__ y, float* __restrict__ part, int M, int N,
                                                       int K, int ks, int S, int ntiles, int mparts, int mrows,
                                                       int I, const uint32_t* __restrict__ masks,
                                                       const int32_t* __restrict__ midx, int n_masks, int wwords,
                                                       sample_keys_t<MODE == MODE_SAMPLE> sk,
                                                       penalty_keys_t<PENAL> pk) {
    constexpr int NF = NB / 16;         // A fragments (16 weight rows each)
    // X rows staged per block (a multiple of 32, <= 4 waves x MT 16-row
    // tiles): the M part rounded up to 32 rows, not to 64 -- at 320 rows
    // (two parts of 160) the X image is 160 rows instead of 192, and X is
    // most of the bytes each CU stages (profiles/decode_late_ab_r3.txt)
    static_assert(MR % 32 == 0 && MR <= MT * 64 && MR > (MT - 1) * 64, "MR: staged X rows");
    constexpr int WCH = NB * 8;         // 16-B chunks of a stage's weight image [NB][64 k]
    constexpr int SCH = WCH + MR * 8;   // ... plus the X image [MR][64 k]
    constexpr int WI = NB / 32;         // 1-KiB LDS-DMA pieces (8 rows x 128 B) per wave per stage: weights
    constexpr int XI = MR / 32;         //                                                          X rows
    constexpr int GL = WI + XI;         // LDS-DMA instructions per wave per stage
    // ONE shared array (a second __shared__ object can make hipcc wait vmcnt(0)
    // before every LDS read, draining the DMA ring: cdna_hip_programming.md §5)
    __shared__ uint4 lds[ST * SCH];

    const int tid = threadIdx.x;
    const int lane = tid & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int l16 = lane & 15, g = lane >> 4;
    // block -> (weight tile nt, K slice s, M part mp); the M parts of one
    // (nt, s) unit share blockIdx % 8 (one XCD) and consecutive dispatch slots
    const int units = ntiles * S;
    int u, mp;
    if ((units & 7) == 0) {
        const int j = blockIdx.x >> 3;
        u = (j / mparts) * 8 + (blockIdx.x & 7);
        mp = j % mparts;
    } else {  // XCD-contiguous ranges (bijective for any grid): a unit's M parts on one XCD
        const int nblk = units * mparts, b = blockIdx.x;
        const int xcd = b & 7, q8 = nblk >> 3, r8 = nblk & 7;
        const int L = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (b >> 3);
        u = L / mparts;
        mp = L % mparts;
    }
    const int nt = u % ntiles, s = u / ntiles;
    const int k0 = s * ks;
    const int chunks = ks / kKC;
    const int m_lo = mp * mrows;
    const int m_hi = min(M, m_lo + mrows);
    const int mw = wv * (MT * 16);                 // this wave's first row inside the part
    int mtv = (m_hi - m_lo - mw + 15) / 16;        // valid 16-row tiles of this wave (wave-uniform)
    mtv = max(0, min(MT, mtv));

    // weight rows of this block: NB contiguous rows, or (SwiGLU) 64 gate rows
    // n0h.. and the 64 up rows I + n0h..
    const int n0 = nt * NB;
    const int n0h = nt * (NB / 2);
    auto wrow = [&](int r) -> int {
        if constexpr (MODE == MODE_SWIGLU) return r < NB / 2 ? n0h + r : I + n0h + (r - NB / 2);
        else return n0 + r;
    };
    // LDS images [rows][8 x 16 B], chunk j of row r stored at slot j ^ (r & 7)
    // (conflict-free ds_read_b128 of the fragments); LDS-DMA writes lane-linear,
    // so the swizzle goes on each lane's SOURCE address: lane L of a piece
    // fills row base + L / 8, slot L % 8 with logical chunk (L % 8) ^ (row & 7)
    const uint16_t* wsrc[WI];
    const uint16_t* xsrc[XI];
#pragma unroll
    for (int i = 0; i < WI; ++i) {
        const int r = (wv * WI + i) * 8 + (lane >> 3);
        wsrc[i] = w + (size_t)wrow(r) * K + k0 + (((lane & 7) ^ (r & 7)) * 8);
    }
#pragma unroll
    for (int i = 0; i < XI; ++i) {
        const int r = (wv * XI + i) * 8 + (lane >> 3);
        xsrc[i] = x + (size_t)min(m_lo + r, M - 1) * K + k0 + (((lane & 7) ^ (r & 7)) * 8);
    }
    auto issue = [&](int c, int slot) {
        uint4* base = lds + slot * SCH;
#pragma unroll
        for (int i = 0; i < WI; ++i) glds16<AUXW>(wsrc[i] + c * kKC, base + (wv * WI + i) * 64);
#pragma unroll
        for (int i = 0; i < XI; ++i) glds16(xsrc[i] + c * kKC, base + WCH + (wv * XI + i) * 64);
    };

    f32x4_t acc[NF][MT];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[f][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    // Both 32-deep k steps' operand fragments are read from LDS before the
    // first MFMA of the chunk, the second step's reads overlapping the first
    // step's MFMAs: one exposed LDS latency per chunk instead of one per
    // fragment group.  At one wave per SIMD (the LDS ring holds one block per
    // CU) nothing else hides those latencies: the compiler's register-lean
    // schedule (2 A fragments live, lgkmcnt(0) before every 3-6 MFMAs) left
    // the matrix cores idle ~2/3 of the time (the 320-row gate/up GEMM with its
    // loads switched off: 32 -> 29 us, whole kernel 40 -> 38 us against
    // ~10 us of MFMA; the rest is the CU's load path: profiles/wgemm_parts_r3.txt).
    auto compute = [&](const uint4* st) {
        const uint4* wl = st;
        const uint4* xl = st + WCH;
        bf16x8_t b[2][MT], a[2][NF];
        auto load = [&](int kk) {
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                // rows past the staged image (the last wave's spare tile
                // when MR < MT * 64) read the image's last row; their
                // results are never stored (mtv / m_hi)
                const int r = min(mw + 16 * t + l16, MR - 1);
                b[kk][t] = as_bf16x8(xl[r * 8 + ((4 * kk + g) ^ (r & 7))]);
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int r = 16 * f + l16;
                a[kk][f] = as_bf16x8(wl[r * 8 + ((4 * kk + g) ^ (r & 7))]);
            }
        };
        auto mma = [&](int kk) {
#pragma unroll
            for (int f = 0; f < NF; ++f)
                // every tile, valid or not: the waves meet at a barrier per
                // chunk, so a wave's idle tiles cost no wall time, and a
                // per-tile branch breaks back-to-back MFMA issue
#pragma unroll
                for (int t = 0; t < MT; ++t)
                    acc[f][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[kk][f], b[kk][t], acc[f][t], 0, 0, 0);
        };
        // k step 0's reads, then its MFMAs with k step 1's reads threaded
        // between them (one read per RM MFMAs, pinned: the scheduler would
        // sink each read to its use), then k step 1's MFMAs.  At most
        // NF + MT <= 12 reads are in flight, within lgkmcnt's range, so the
        // waits stay counted (22 queued reads made the compiler wait for 0).
        constexpr int NR = NF + MT;            // fragment reads per k step
        constexpr int NM = NF * MT;            // MFMAs per k step
        constexpr int RM = NM / NR > 0 ? NM / NR : 1;
        load(0);
        __builtin_amdgcn_sched_barrier(0);
        load(1);
        mma(0);
#pragma unroll
        for (int i = 0; i < NR; ++i) {
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // one DS read
            __builtin_amdgcn_sched_group_barrier(0x008, RM, 0);  // RM MFMAs
        }
        __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);      // the rest
        __builtin_amdgcn_sched_barrier(0);
        mma(1);
    };

    // ST-stage ring, ST - 1 stages in flight: wait for this wave's pieces of
    // stage c (counted vmcnt, the next stage may stay in flight), one raw
    // barrier (every wave's pieces landed; every wave done reading the slot
    // about to be refilled), refill, compute.  No __syncthreads() in the loop:
    // its fence would drain the DMA ring (vmcnt(0)).
#pragma unroll
    for (int j = 0; j < ST - 1; ++j)
        if (j < chunks) issue(j, j);
    for (int c = 0; c < chunks; ++c) {
        if (c + ST - 2 < chunks) {
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"i"(GL * (ST - 2)) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
        }
        if (c + ST - 1 < chunks) issue(c + ST - 1, (c + ST - 1) % ST);
        compute(lds + (c % ST) * SCH);
    }

    // epilogue: lane (l16, g) holds Y[row m_lo + mw + 16t + l16][col 16f + 4g + i]
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        if (t >= mtv) continue;
        const int m = m_lo + mw + 16 * t + l16;
        if constexpr (MODE == MODE_ARGMAX || MODE == MODE_SAMPLE) {
            // masked max of this row over the tile's NB columns: each lane its
            // 4 NF columns, then across the 4 lane groups g (every lane takes
            // part in the shuffles; rows past the part only skip the store).
            // Values are bf16-rounded (what F.linear + masked_argmax compare),
            // ties go to the lowest id.  MODE_SAMPLE perturbs each allowed
            // value (row key once per row, no hash or log for masked ids);
            // a padding row (slot < 0) keeps the empty pair.
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            bool live = m < m_hi;
            uint32_t key = 0;
            if constexpr (MODE == MODE_SAMPLE) {
                if (live) {
                    const int slot = sk.slots[m];
                    live = slot >= 0;
                    key = gumbel_key(sk.seed, slot, sk.positions[m]);
                }
            }
            if (live) {
                int mr = midx ? midx[m] : 0;
                mr = mr < 0 ? 0 : (mr >= n_masks ? n_masks - 1 : mr);
                const uint32_t* mrow = masks + (size_t)mr * wwords + (n0 >> 5);
                [[maybe_unused]] const uint32_t* hrow = nullptr;
                if constexpr (PENAL) {
                    hrow = penalty_row(pk, m, mr);
                    if (hrow) hrow += n0 >> 5;
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
                            float x = bf2f(f2bf(acc[f][t][i]));
                            if constexpr (PENAL) {
                                if ((hword >> (c & 31)) & 1u) x = penalize(x, pk.theta, pk.inv_theta, pk.alpha);
                            }
                            if constexpr (MODE == MODE_SAMPLE) x = gumbel_score(x, sk.inv_t, key, n0 + c);
                            if (x > bv) { bv = x; bi = n0 + c; }  // columns ascend: strict > keeps the lowest
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
            if (m < m_hi && g == 0)
                reinterpret_cast<float2*>(part)[(size_t)nt * M + m] = make_float2(bv, __int_as_float(bi));
            continue;
        }
        if (m >= m_hi) continue;
        if constexpr (MODE == MODE_SWIGLU) {
#pragma unroll
            for (int f = 0; f < NF / 2; ++f) {
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {  // gate / up rounded to bf16 as the unfused GEMM output is
                    const float gg = bf2f(f2bf(acc[f][t][i])), uu = bf2f(f2bf(acc[f + NF / 2][t][i]));
                    o[i] = silu(gg) * uu;
                }
                *reinterpret_cast<uint2*>(y + (size_t)m * I + n0h + 16 * f + 4 * g) = pack4(o);
            }
        } else if constexpr (MODE == MODE_PART) {
            float* dst = part + ((size_t)s * M + m) * N + n0 + 4 * g;
#pragma unroll
            for (int f = 0; f < NF; ++f)
                *reinterpret_cast<float4*>(dst + 16 * f) =
                    make_float4(acc[f][t][0], acc[f][t][1], acc[f][t][2], acc[f][t][3]);
        } else {
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const float o[4] = {acc[f][t][0], acc[f][t][1], acc[f][t][2], acc[f][t][3]};
                *reinterpret_cast<uint2*>(y + (size_t)m * N + n0 + 16 * f + 4 * g) = pack4(o);
            }
        }
    }
}

constexpr int kStages = 3;  // LDS ring stages (2 in flight while one is computed)
// dmcp_wgemm_set_aux: the weight stream's cache policy (0 default, 2 nt)
int g_wgemm_auxw = 0;

template <int NB, int MODE, bool PENAL = false>
hipError_t launch_wgemm(const uint16_t* x, const uint16_t* w, uint16_t* y, float* part, int M, int N, int K, int S,
                        int mparts, int I, hipStream_t st, const uint32_t* masks = nullptr,
                        const int32_t* midx = nullptr, int n_masks = 0, int wwords = 0,
                        const SampleKeys& sk = SampleKeys{}, const PenaltyKeys& pk = PenaltyKeys{}) {
    const auto keys = pick_keys<MODE == MODE_SAMPLE>(sk);
    const auto pen = pick_penalty<PENAL>(pk);
    const int ntiles = (MODE == MODE_SWIGLU ? 2 * I : N) / NB;
    const int mrows = (((M + mparts - 1) / mparts) + 15) & ~15;
    const int mt = (mrows + 4 * 16 - 1) / (4 * 16);  // 16-row tiles per wave
    const bool full = ((mrows + 31) & ~31) > (mt - 1) * 64 + 32;  // staged rows: mt * 64, else mt * 64 - 32
    const dim3 grid((unsigned)(ntiles * S * mparts));
    const int ks = K / S;
#define DMCP_WG1(MT, MR)                                                                                        \
    do {                                                                                                        \
        if (g_wgemm_auxw == 2)                                                                                  \
            wgemm_kernel<NB, MT, MR, MODE, kStages, 2, PENAL><<<grid, kBlock, 0, st>>>(                         \
                x, w, y, part, M, N, K, ks, S, ntiles, mparts, mrows, I, masks, midx, n_masks, wwords, keys,    \
                pen);                                                                                           \
        else                                                                                                    \
            wgemm_kernel<NB, MT, MR, MODE, kStages, 0, PENAL><<<grid, kBlock, 0, st>>>(                         \
                x, w, y, part, M, N, K, ks, S, ntiles, mparts, mrows, I, masks, midx, n_masks, wwords, keys,    \
                pen);                                                                                           \
    } while (0)
#define DMCP_WG(MT)                  \
    do {                             \
        if (full)                    \
            DMCP_WG1(MT, MT * 64);   \
        else                         \
            DMCP_WG1(MT, MT * 64 - 32); \
    } while (0)
    switch (mt) {
        case 1: DMCP_WG(1); break;
        case 2: DMCP_WG(2); break;
        case 3: DMCP_WG(3); break;
        case 4: DMCP_WG(4); break;
        default: return hipErrorInvalidValue;
    }
#undef DMCP_WG
#undef DMCP_WG1
    return hipGetLastError();
}

}  // namespace

extern "C" {

// cache policy of the weight stream's LDS-DMA (0 or 2 = nt); returns the previous value
int dmcp_wgemm_set_aux(int aux) {
    const int old = g_wgemm_auxw;
    if (aux == 0 || aux == 2) g_wgemm_auxw = aux;
    return old;
}

// Plain / partial / SwiGLU weight-streaming GEMM.
//   mode 0: y[M, N] bf16 = x . w^T                        (S == 1)
//   mode 1: part[S, M, N] fp32 partials over K / S slices
//   mode 2: y[M, I] bf16 = silu(x . w[:I]^T) * (x . w[I:]^T)  (w = [gate; up] [2I, K], S == 1)
// Contract (checked by dmcp/ops/hip.py, guarded here): M in [1, 512],
// K % (64 S) == 0, N % 64 == 0 (mode 2: I % 64 == 0), rows / parts <= 256.
int dmcp_wgemm(const void* x, const void* w, void* y, void* part, int M, int N, int K, int S, int mparts, int mode,
               int I, void* stream) {
    if (M <= 0) return 0;
    if (!x || !w || M > 512 || S < 1 || mparts < 1 || K % (kKC * S) != 0 || (mode == 1 && !part) ||
        (mode != 1 && (!y || S != 1)) || (mode == 2 ? (I <= 0 || I % 64 != 0) : (N <= 0 || N % 64 != 0)) ||
        (((M + mparts - 1) / mparts + 15) & ~15) > 256)
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    auto yy = (uint16_t*)y;
    auto pp = (float*)part;
    // 64 weight rows per block (128 = 64 gate + 64 up for SwiGLU): 128-row
    // tiles for the plain / split-K forms measured slower at 78 and 320 rows
    // (4.80 vs 4.68 ms per fp8 step at 320, profiles/wgemm_r3.txt) -- the
    // halved X traffic does not pay for the doubled accumulators
    switch (mode) {
        case 0: return launch_wgemm<64, MODE_BF16>(xx, ww, yy, pp, M, N, K, S, mparts, 0, st);
        case 1: return launch_wgemm<64, MODE_PART>(xx, ww, yy, pp, M, N, K, S, mparts, 0, st);
        case 2: return launch_wgemm<128, MODE_SWIGLU>(xx, ww, yy, pp, M, 2 * I, K, S, mparts, I, st);
        default: return hipErrorInvalidValue;
    }
}

// LM head + grammar-masked greedy selection: ids[m] = argmax over the ids v
// allowed by mask row midx[m] (masks [n_masks, wwords] bitsets) of
// bf16(x[m] . w[v]); best: float2 workspace of (V / NB) * M pairs.  NB = 128
// vocabulary rows per block when V % 128 == 0 (fewer re-reads of x), else
// 64.  Contract: M in [1, 512], K % 64 == 0, V % 64 == 0, rows / part <= 256.
int dmcp_lm_head_argmax(const void* x, const void* w, const void* masks, const void* midx, int n_masks, int wwords,
                        void* best, void* ids, int M, int V, int K, int mparts, void* stream) {
    if (M <= 0) return 0;
    if (!x || !w || !masks || !best || !ids || M > 512 || n_masks < 1 || wwords < (V + 31) / 32 || mparts < 1 ||
        K % kKC != 0 || V <= 0 || V % 64 != 0 || (((M + mparts - 1) / mparts + 15) & ~15) > 256)
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    auto bb = (float*)best;
    auto mk = (const uint32_t*)masks;
    auto mi = (const int32_t*)midx;
    hipError_t e;
    int ntiles;
    if (V % 128 == 0) {
        ntiles = V / 128;
        e = launch_wgemm<128, MODE_ARGMAX>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks, wwords);
    } else {
        ntiles = V / 64;
        e = launch_wgemm<64, MODE_ARGMAX>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks, wwords);
    }
    if (e != hipSuccess) return e;
    argmax_pairs_kernel<<<(M + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, st>>>(
        (const float2*)best, ntiles, M, (int32_t*)ids);
    return hipGetLastError();
}

// dmcp_lm_head_argmax at a temperature: ids[m] = argmax over the allowed v of
// bf16(x[m] . w[v]) * inv_temperature + Gumbel noise keyed by (seed, slots[m],
// positions[m], v) (dmcp_common.hpp) -- an exact sample of softmax(logits / T)
// over the allowed ids; rows with slots[m] < 0 select 0.  Same contract,
// tiles, workspace and pair reduction as the greedy entry point.
int dmcp_lm_head_sample(const void* x, const void* w, const void* masks, const void* midx, int n_masks, int wwords,
                        void* best, void* ids, int M, int V, int K, int mparts, const void* slots,
                        const void* positions, unsigned seed, float inv_temperature, void* stream) {
    if (M <= 0) return 0;
    if (!x || !w || !masks || !best || !ids || M > 512 || n_masks < 1 || wwords < (V + 31) / 32 || mparts < 1 ||
        K % kKC != 0 || V <= 0 || V % 64 != 0 || (((M + mparts - 1) / mparts + 15) & ~15) > 256 || !slots ||
        !positions || !(inv_temperature > 0.f))
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    auto bb = (float*)best;
    auto mk = (const uint32_t*)masks;
    auto mi = (const int32_t*)midx;
    const SampleKeys sk{(const int32_t*)slots, (const int32_t*)positions, seed, inv_temperature};
    hipError_t e;
    int ntiles;
    if (V % 128 == 0) {
        ntiles = V / 128;
        e = launch_wgemm<128, MODE_SAMPLE>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks, wwords, sk);
    } else {
        ntiles = V / 64;
        e = launch_wgemm<64, MODE_SAMPLE>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks, wwords, sk);
    }
    if (e != hipSuccess) return e;
    argmax_pairs_kernel<<<(M + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, st>>>(
        (const float2*)best, ntiles, M, (int32_t*)ids);
    return hipGetLastError();
}

// dmcp_lm_head_argmax (inv_temperature == 0; slots / positions / seed unused)
// or dmcp_lm_head_sample (inv_temperature > 0) under a repetition / presence
// penalty: the penalty arguments of dmcp_masked_penal (dmcp_kernels.hip), the
// flags indexed by the mask row.  Same contract, tiles, workspace and pair
// reduction as the unpenalised entry points.
int dmcp_lm_head_penal(const void* x, const void* w, const void* masks, const void* midx, int n_masks, int wwords,
                       void* best, void* ids, int M, int V, int K, int mparts, const void* slots,
                       const void* positions, unsigned seed, float inv_temperature, const void* history, int hwords,
                       int n_slots, const void* pslots, const void* prows, int n_rows, float theta, float inv_theta,
                       float alpha, void* stream) {
    if (M <= 0) return 0;
    const bool sample = inv_temperature != 0.f;
    if (!x || !w || !masks || !best || !ids || M > 512 || n_masks < 1 || wwords < (V + 31) / 32 || mparts < 1 ||
        K % kKC != 0 || V <= 0 || V % 64 != 0 || (((M + mparts - 1) / mparts + 15) & ~15) > 256 ||
        (sample && (!slots || !positions || !(inv_temperature > 0.f))) || !history || !pslots ||
        hwords < (V + 31) / 32 || n_slots <= 0 || (prows && n_rows < n_masks) || !(theta > 0.f) ||
        !(inv_theta > 0.f) || !(alpha == alpha))
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto xx = (const uint16_t*)x;
    auto ww = (const uint16_t*)w;
    auto bb = (float*)best;
    auto mk = (const uint32_t*)masks;
    auto mi = (const int32_t*)midx;
    const SampleKeys sk{(const int32_t*)slots, (const int32_t*)positions, seed, inv_temperature};
    const PenaltyKeys pk{(const uint32_t*)history, (const int32_t*)pslots, (const int32_t*)prows, hwords, n_slots,
                         n_rows, theta, inv_theta, alpha};
    hipError_t e;
    const int nb = V % 128 == 0 ? 128 : 64;
    if (nb == 128 && sample)
        e = launch_wgemm<128, MODE_SAMPLE, true>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks,
                                                 wwords, sk, pk);
    else if (nb == 128)
        e = launch_wgemm<128, MODE_ARGMAX, true>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks,
                                                 wwords, sk, pk);
    else if (sample)
        e = launch_wgemm<64, MODE_SAMPLE, true>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks,
                                                wwords, sk, pk);
    else
        e = launch_wgemm<64, MODE_ARGMAX, true>(xx, ww, nullptr, bb, M, V, K, 1, mparts, 0, st, mk, mi, n_masks,
                                                wwords, sk, pk);
    if (e != hipSuccess) return e;
    argmax_pairs_kernel<<<(M + kBlock / kWave - 1) / (kBlock / kWave), kBlock, 0, st>>>(
        (const float2*)best, V / nb, M, (int32_t*)ids);
    return hipGetLastError();
}

}  // extern "C"
