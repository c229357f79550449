// Sampled selection with top-k / top-p / min-p truncation over materialised
// bf16 logits: ids[b] = argmax over the KEPT ids of bf16 logit / T + Gumbel
// noise (dmcp_common.hpp gumbel_score -- the hash, key and tie rule of
// masked_sample), the kept set defined once in dmcp/ops/reference.py
// truncation_threshold:
//
//   A     = the ids the row's mask allows, below V;   x_v = the bf16 logit;
//   x_max = max over A;    kept = {v in A : x_v >= tau},  tau = max of
//   tau_k = the k-th largest x over A counting multiplicity (k = 0 or
//           k >= |A|: -inf);
//   tau_p = over the top-k survivors, walking the distinct values downwards
//           and accumulating count(value) * exp((value - x_max) / T), the
//           first value at which the running sum reaches p * Z (Z the
//           survivors' total; p = 1: -inf);
//   tau_m = v is kept iff (x_v - x_max) * inv_t >= ln_min_p in fp32 (a
//           subtract, then a multiply; min_p = 0: -inf).
//
// Every filter is a threshold on the VALUE, so the search runs on the
// order-preserving 16-bit key of the bf16 (sign folded; -0 keyed as +0): a
// radix search, four bits per pass from the top.  A pass reads the row once;
// each thread keeps the 16 candidate digits' integer counts (and, for top-p,
// their fp32 weight sums) of the ids that match the prefix found so far in
// registers -- compare/select chains, no indexed array, no atomics -- and the
// block adds them in a fixed order: xor butterflies inside a wave, the 16
// waves in index order.  Every thread then walks the 16 totals downwards and
// takes the same digit.  The same inputs therefore give the same tau and the
// same id on every run (nothing here uses a floating-point atomic; the
// library is built with -munsafe-fp-atomics).
//
//   pass 0      x_max and |A|                                   1 row read
//   top-k       4 count passes (skipped when k = 0 or k >= |A|) 4 row reads
//   top-p       4 count + weight passes over the ids >= tau_k   4 row reads
//               (skipped when p = 1); the first one's total is Z
//   selection   the perturbed argmax over x >= tau under the    1 row read
//               min-p predicate, the kept count and the lowest
//               kept value (tau as reported in stats)
//
// A row of 128,256 bf16 (250 KB) does not fit LDS: the passes re-read it from
// L2.  One 1,024-thread block per row as masked_argmax_kernel; whole 8-id
// chunks as one 16-B load with their 8 mask bits when every row start is
// 16-B aligned, the ids past the last whole chunk (and unaligned rows)
// element-wise.
#include "dmcp_common.hpp"

namespace {

constexpr int TS_T = 1024;          // threads per block (one block per row)
constexpr int TS_W = TS_T / kWave;  // waves per block
constexpr uint32_t TS_NEG_INF = 0xFF80u;  // bf16 -inf: the reported tau when nothing is cut

// order-preserving key of a bf16: a < b as values <=> key(a) < key(b); -0 -> key(+0)
__device__ __forceinline__ uint32_t bf_key(uint32_t bits) {
    bits = bits == 0x8000u ? 0u : bits;
    return bits ^ ((bits & 0x8000u) ? 0xFFFFu : 0x8000u);
}
__device__ __forceinline__ uint32_t key_bits(uint32_t key) {
    return key ^ ((key & 0x8000u) ? 0x8000u : 0xFFFFu);
}
__device__ __forceinline__ float key_value(uint32_t key) { return __uint_as_float(key_bits(key) << 16); }

// The PENAL variant's view of a row (repetition / presence penalty,
// dmcp_common.hpp penalize): every pass maps a loaded value whose history
// bit is set through the penalty BEFORE keying it, so the radix passes, the
// thresholds and the reported tau are those of the penalised values.  The
// history byte of an 8-id chunk travels with its mask byte.  hrow is null for
// a row that is not penalised; the plain variant carries nothing.
struct RowPenalty {
    const uint32_t* hrow;
    float theta, inv_theta, alpha;
};
struct NoRowPenalty {};
template <bool PENAL>
using row_penalty_t = std::conditional_t<PENAL, RowPenalty, NoRowPenalty>;

// f(key, id) for every id of the row that the mask allows
template <bool PENAL, class F>
__device__ __forceinline__ void for_allowed(const uint16_t* __restrict__ row, const uint32_t* __restrict__ mrow,
                                            int V, int nch, const row_penalty_t<PENAL>& rp, F&& f) {
    for (int c = threadIdx.x; c < nch; c += TS_T) {
        const uint4 q = *reinterpret_cast<const uint4*>(row + (size_t)c * 8);
        const uint32_t m = mrow ? (mrow[c >> 2] >> ((c & 3) * 8)) & 0xFFu : 0xFFu;
        [[maybe_unused]] uint32_t h = 0u;
        if constexpr (PENAL) h = rp.hrow ? (rp.hrow[c >> 2] >> ((c & 3) * 8)) & 0xFFu : 0u;
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if ((m >> j) & 1u) {
                uint32_t bits = (j & 1) ? (w[j >> 1] >> 16) : (w[j >> 1] & 0xFFFFu);
                if constexpr (PENAL) {
                    if ((h >> j) & 1u) bits = f2bf(penalize(bf2f((uint16_t)bits), rp.theta, rp.inv_theta, rp.alpha));
                }
                f(bf_key(bits), c * 8 + j);
            }
    }
    for (int v = nch * 8 + threadIdx.x; v < V; v += TS_T) {
        if (mrow && !((mrow[v >> 5] >> (v & 31)) & 1u)) continue;
        uint32_t bits = row[v];
        if constexpr (PENAL) {
            if (rp.hrow && ((rp.hrow[v >> 5] >> (v & 31)) & 1u))
                bits = f2bf(penalize(bf2f((uint16_t)bits), rp.theta, rp.inv_theta, rp.alpha));
        }
        f(bf_key(bits), v);
    }
}

// Block totals of 16 counts (and 16 weight sums), the same in every thread:
// xor butterflies inside a wave, then the waves in index order.
template <bool WEIGHTS>
__device__ __forceinline__ void block_totals(int (&cnt)[16], float (&wsum)[16], int (*red_c)[16], float (*red_w)[16],
                                             int* tot_c, float* tot_w) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            cnt[j] += __shfl_xor(cnt[j], m, kWave);
            if constexpr (WEIGHTS) wsum[j] += __shfl_xor(wsum[j], m, kWave);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            red_c[wave][j] = cnt[j];
            if constexpr (WEIGHTS) red_w[wave][j] = wsum[j];
        }
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        int c = 0;
        float w = 0.f;
        for (int k = 0; k < TS_W; ++k) {
            c += red_c[k][threadIdx.x];
            if constexpr (WEIGHTS) w += red_w[k][threadIdx.x];
        }
        tot_c[threadIdx.x] = c;
        if constexpr (WEIGHTS) tot_w[threadIdx.x] = w;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        cnt[j] = tot_c[j];
        if constexpr (WEIGHTS) wsum[j] = tot_w[j];
    }
}

// One radix pass: the counts (and weights) per 4-bit digit at `shift` of the
// allowed ids whose key is >= floor_key and whose bits above the digit equal
// `prefix`.
template <bool WEIGHTS, bool PENAL>
__device__ __forceinline__ void digit_pass(const uint16_t* __restrict__ row, const uint32_t* __restrict__ mrow, int V,
                                           int nch, const row_penalty_t<PENAL>& rp, int shift, uint32_t prefix,
                                           uint32_t floor_key, float x_max,
                                           float inv_t, int (&cnt)[16], float (&wsum)[16], int (*red_c)[16],
                                           float (*red_w)[16], int* tot_c, float* tot_w) {
#pragma unroll
    for (int j = 0; j < 16; ++j) { cnt[j] = 0; wsum[j] = 0.f; }
    for_allowed<PENAL>(row, mrow, V, nch, rp, [&](uint32_t key, int) {
        if ((key >> (shift + 4)) != prefix || key < floor_key) return;
        const uint32_t d = (key >> shift) & 15u;
        float w = 0.f;
        if constexpr (WEIGHTS) w = expf((key_value(key) - x_max) * inv_t);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool hit = d == (uint32_t)j;
            cnt[j] += hit ? 1 : 0;
            if constexpr (WEIGHTS) wsum[j] += hit ? w : 0.f;
        }
    });
    block_totals<WEIGHTS>(cnt, wsum, red_c, red_w, tot_c, tot_w);
}

template <bool PENAL>
__global__ __launch_bounds__(TS_T) void truncated_sample_kernel(
    const uint16_t* __restrict__ logits, const uint32_t* __restrict__ mask, const int32_t* __restrict__ mask_idx,
    int n_masks, int32_t* __restrict__ ids, int V, int ld, int nch, SampleKeys sk, int top_k, float top_p,
    float ln_min_p, int32_t* __restrict__ stats, penalty_keys_t<PENAL> pk) {
    __shared__ int red_c[TS_W][16];
    __shared__ float red_w[TS_W][16];
    __shared__ int tot_c[16];
    __shared__ float tot_w[16];
    __shared__ float fin_s[TS_W];
    __shared__ int fin_i[TS_W], fin_n[TS_W];
    __shared__ uint32_t fin_k[TS_W];
    const int b = blockIdx.x;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int slot = sk.slots[b];
    if (slot < 0) {  // block-uniform: a padding row
        if (threadIdx.x == 0) {
            ids[b] = 0;
            if (stats) { stats[2 * b] = (int32_t)TS_NEG_INF; stats[2 * b + 1] = 0; }
        }
        return;
    }
    const uint32_t gkey = gumbel_key(sk.seed, slot, sk.positions[b]);
    const float inv_t = sk.inv_t;
    const uint16_t* row = logits + (size_t)b * ld;
    int mr = b;
    if (mask_idx) {
        mr = mask_idx[b];
        mr = mr < 0 ? 0 : (mr >= n_masks ? n_masks - 1 : mr);
    }
    const uint32_t* mrow = mask ? mask + (size_t)mr * ((V + 31) >> 5) : nullptr;
    row_penalty_t<PENAL> rp;
    if constexpr (PENAL) rp = RowPenalty{penalty_row(pk, b, mr), pk.theta, pk.inv_theta, pk.alpha};

    // pass 0: x_max (as a key) and |A|
    uint32_t kmax = 0;
    int n_allowed = 0;
    for_allowed<PENAL>(row, mrow, V, nch, rp, [&](uint32_t key, int) {
        kmax = key > kmax ? key : kmax;
        ++n_allowed;
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t ok = __shfl_xor(kmax, m, kWave);
        kmax = ok > kmax ? ok : kmax;
        n_allowed += __shfl_xor(n_allowed, m, kWave);
    }
    if (lane == 0) { fin_k[wave] = kmax; fin_n[wave] = n_allowed; }
    __syncthreads();
    kmax = 0;
    n_allowed = 0;
    for (int k = 0; k < TS_W; ++k) {
        kmax = fin_k[k] > kmax ? fin_k[k] : kmax;
        n_allowed += fin_n[k];
    }
    __syncthreads();  // fin_k / fin_n are reused by the selection pass
    if (n_allowed == 0) {  // block-uniform: the mask allows nothing
        if (threadIdx.x == 0) {
            ids[b] = 0;
            if (stats) { stats[2 * b] = (int32_t)TS_NEG_INF; stats[2 * b + 1] = 0; }
        }
        return;
    }
    const float x_max = key_value(kmax);
    const bool cut_k = top_k > 0 && top_k < n_allowed;
    const bool cut_p = top_p < 1.f;
    const bool cut_m = ln_min_p > -INFINITY;

    int cnt[16];
    float wsum[16];
    uint32_t tkey = 0;  // the threshold as a key: 0 keeps every value
    if (cut_k) {
        uint32_t prefix = 0;
        int need = top_k;  // the need-th largest among the ids under the prefix
        for (int shift = 12; shift >= 0; shift -= 4) {
            digit_pass<false, PENAL>(row, mrow, V, nch, rp, shift, prefix, 0u, x_max, inv_t, cnt, wsum, red_c, red_w,
                                     tot_c, tot_w);
            int pick = 0;
            bool found = false;
#pragma unroll
            for (int j = 15; j >= 0; --j) {
                if (!found) {
                    if (cnt[j] >= need) { pick = j; found = true; }
                    else need -= cnt[j];
                }
            }
            prefix = (prefix << 4) | (uint32_t)pick;
        }
        tkey = prefix;
    }
    if (cut_p) {
        uint32_t prefix = 0;
        float above = 0.f, target = 0.f;  // the weight above the prefix's range; p * Z
        for (int shift = 12; shift >= 0; shift -= 4) {
            digit_pass<true, PENAL>(row, mrow, V, nch, rp, shift, prefix, tkey, x_max, inv_t, cnt, wsum, red_c, red_w,
                                    tot_c, tot_w);
            if (shift == 12) {  // every survivor is in one of the 16 ranges: their total is Z
                float z = 0.f;
#pragma unroll
                for (int j = 15; j >= 0; --j) z += wsum[j];
                target = top_p * z;
            }
            // downwards: the first non-empty range at which the running sum
            // reaches p * Z; if fp32 rounding leaves the sum short of it at
            // the end, the lowest non-empty range
            int pick = 0, lowest = 0;
            bool found = false;
            float run = above;
#pragma unroll
            for (int j = 15; j >= 0; --j) {
                if (cnt[j] > 0) {
                    lowest = j;
                    if (!found) {
                        if (run + wsum[j] >= target) { pick = j; found = true; above = run; }
                        else run += wsum[j];
                    }
                }
            }
            if (!found) {
                pick = lowest;
                above = run - wsum[lowest];
            }
            prefix = (prefix << 4) | (uint32_t)pick;
        }
        tkey = prefix > tkey ? prefix : tkey;
    }

    // selection: the perturbed argmax over the kept ids
    float best = -INFINITY;
    int bi = 0x7fffffff, kept = 0;
    uint32_t kmin = 0xFFFFu;
    for_allowed<PENAL>(row, mrow, V, nch, rp, [&](uint32_t key, int v) {
        if (key < tkey) return;
        const float x = key_value(key);
        if (cut_m && !((x - x_max) * inv_t >= ln_min_p)) return;
        ++kept;
        kmin = key < kmin ? key : kmin;
        argmax_take(gumbel_score(x, inv_t, gkey, v), v, best, bi);
    });
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, kWave);
        const int oi = __shfl_xor(bi, m, kWave);
        argmax_take(ob, oi, best, bi);
        kept += __shfl_xor(kept, m, kWave);
        const uint32_t ok = __shfl_xor(kmin, m, kWave);
        kmin = ok < kmin ? ok : kmin;
    }
    if (lane == 0) { fin_s[wave] = best; fin_i[wave] = bi; fin_n[wave] = kept; fin_k[wave] = kmin; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float B = fin_s[0];
        int I = fin_i[0], N = fin_n[0];
        uint32_t K = fin_k[0];
        for (int k = 1; k < TS_W; ++k) {
            argmax_take(fin_s[k], fin_i[k], B, I);
            N += fin_n[k];
            K = fin_k[k] < K ? fin_k[k] : K;
        }
        ids[b] = (I == 0x7fffffff) ? 0 : I;
        if (stats) {
            // tau: the lowest kept value when a filter is on (each of tau_k,
            // tau_p, tau_m is a value of A, so the largest of them is the
            // lowest kept value), -inf when none is
            stats[2 * b] = (int32_t)((cut_k || cut_p || cut_m) ? key_bits(K) : TS_NEG_INF);
            stats[2 * b + 1] = N;
        }
    }
}

}  // namespace

extern "C" {

// ids[b] = the sampled id of row b under top-k / top-p / min-p truncation
// (top_k 0, top_p 1, ln_min_p -inf: off -- then dmcp_masked_sample's id).
// logits bf16 [B, ld], V <= ld ids per row; mask / mask_idx / n_masks, slots,
// positions, seed, inv_temperature as dmcp_masked_sample.  stats (optional)
// int32 [B, 2]: the bf16 bits of tau (0xFF80 = -inf when no filter is on) and
// the kept count.  No allocation, no synchronisation: capturable.
int dmcp_truncated_sample(const void* logits, const void* mask, const void* mask_idx, int n_masks, void* ids, int B,
                          int V, int ld, const void* slots, const void* positions, unsigned seed,
                          float inv_temperature, int top_k, float top_p, float ln_min_p, void* stats, void* stream) {
    if (B <= 0) return 0;
    if (!logits || !ids || V <= 0 || V > ld || (mask_idx && (!mask || n_masks <= 0)) || !slots || !positions ||
        !(inv_temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f) || !(ln_min_p < 0.f))
        return hipErrorInvalidValue;
    // whole 16-B chunks only when every row start is 16-B aligned
    const bool vec = (ld % 8 == 0) && (reinterpret_cast<uintptr_t>(logits) % 16 == 0);
    const SampleKeys sk{(const int32_t*)slots, (const int32_t*)positions, seed, inv_temperature};
    truncated_sample_kernel<false><<<B, TS_T, 0, (hipStream_t)stream>>>(
        (const uint16_t*)logits, (const uint32_t*)mask, (const int32_t*)mask_idx, n_masks, (int32_t*)ids, V, ld,
        vec ? V / 8 : 0, sk, top_k, top_p, ln_min_p, (int32_t*)stats, NoPenaltyKeys{});
    return hipGetLastError();
}

// dmcp_truncated_sample under a repetition / presence penalty: the penalty
// arguments of dmcp_masked_penal (dmcp_kernels.hip); thresholds, tau and the
// kept count are those of the penalised values.
int dmcp_truncated_penal(const void* logits, const void* mask, const void* mask_idx, int n_masks, void* ids, int B,
                         int V, int ld, const void* slots, const void* positions, unsigned seed,
                         float inv_temperature, int top_k, float top_p, float ln_min_p, void* stats,
                         const void* history, int hwords, int n_slots, const void* pslots, const void* prows,
                         int n_rows, float theta, float inv_theta, float alpha, void* stream) {
    if (B <= 0) return 0;
    if (!logits || !ids || V <= 0 || V > ld || (mask_idx && (!mask || n_masks <= 0)) || !slots || !positions ||
        !(inv_temperature > 0.f) || top_k < 0 || !(top_p > 0.f && top_p <= 1.f) || !(ln_min_p < 0.f) || !history ||
        !pslots || hwords < (V + 31) / 32 || n_slots <= 0 || (prows && n_rows < (mask_idx ? n_masks : B)) ||
        !(theta > 0.f) || !(inv_theta > 0.f) || !(alpha == alpha))
        return hipErrorInvalidValue;
    const bool vec = (ld % 8 == 0) && (reinterpret_cast<uintptr_t>(logits) % 16 == 0);
    const SampleKeys sk{(const int32_t*)slots, (const int32_t*)positions, seed, inv_temperature};
    const PenaltyKeys pk{(const uint32_t*)history, (const int32_t*)pslots, (const int32_t*)prows, hwords, n_slots,
                         n_rows, theta, inv_theta, alpha};
    truncated_sample_kernel<true><<<B, TS_T, 0, (hipStream_t)stream>>>(
        (const uint16_t*)logits, (const uint32_t*)mask, (const int32_t*)mask_idx, n_masks, (int32_t*)ids, V, ld,
        vec ? V / 8 : 0, sk, top_k, top_p, ln_min_p, (int32_t*)stats, pk);
    return hipGetLastError();
}

}  // extern "C"
