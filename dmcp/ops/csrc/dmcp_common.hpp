// Shared device helpers of the dmcp gfx950 kernels (every .hip file of this
// directory): bf16 <-> fp32 packing, wave reductions, MFMA operand
// types, the LDS-DMA wrapper, fp8 KV and MXFP8 encoding, the split-K slice
// sum.  Header-only, everything in an anonymous namespace per TU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;

__device__ __forceinline__ float bf2f(uint16_t v) {
    return __uint_as_float(((uint32_t)v) << 16);
}

typedef __bf16 bf16x2v_t __attribute__((ext_vector_type(2)));
typedef float f32x2v_t __attribute__((ext_vector_type(2)));

// round-to-nearest-even fp32 -> bf16 (NaN kept quiet): one v_cvt_pk_bf16_f32
// (the bit-twiddling form compiled to a NaN branch per value -- 256 divergent
// branches in a GEMM epilogue)
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }

// two floats -> packed bf16 pair (lo = a), one instruction
__device__ __forceinline__ uint32_t f2bf2(float a, float b) {
    const f32x2v_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2v_t));
}

__device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

__device__ __forceinline__ uint4 pack8(const float* f) {
    uint4 v;
    v.x = f2bf2(f[0], f[1]);
    v.y = f2bf2(f[2], f[3]);
    v.z = f2bf2(f[4], f[5]);
    v.w = f2bf2(f[6], f[7]);
    return v;
}

__device__ __forceinline__ void unpack4(const uint2& v, float* f) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
}

__device__ __forceinline__ uint2 pack4(const float* f) {
    uint2 v;
    v.x = f2bf2(f[0], f[1]);
    v.y = f2bf2(f[2], f[3]);
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// Per-head RMSNorm of a q or k head in the RoPE thread mapping: a lane holds
// dims [d0, d0 + 4) of a head in x1 and their rotary partners (+ D/2) in x2,
// so a head is D/8 consecutive lanes (8 at D = 64, 16 at D = 128), aligned to
// their count and inside one wave.  Every lane of a head must be active.
// x <- x * rsqrt(mean_d(x^2) + eps) * w[d], all fp32; w is bf16 [D].
__device__ __forceinline__ void qk_norm_quad(float* x1, float* x2, const uint16_t* __restrict__ w, int d0, int D,
                                             float eps) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) ss += x1[j] * x1[j] + x2[j] * x2[j];
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) ss += __shfl_xor(ss, m, kWave);
    if (D == 128) ss += __shfl_xor(ss, 8, kWave);  // D is uniform: no divergence at the shuffle
    const float inv = rsqrtf(ss / (float)D + eps);
    float w1[4], w2[4];
    unpack4(*reinterpret_cast<const uint2*>(w + d0), w1);
    unpack4(*reinterpret_cast<const uint2*>(w + (D >> 1) + d0), w2);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x1[j] = x1[j] * inv * w1[j];
        x2[j] = x2[j] * inv * w2[j];
    }
}

__device__ __forceinline__ float silu(float g) { return g / (1.f + __expf(-g)); }

// LDS-DMA (global_load_lds_dwordx4): each lane's 16 source bytes land at
// the wave-uniform LDS base + 16 * lane, with no VGPR round trip; counted on
// vmcnt like any vector load.
// AUX: cache-policy bits of the load (2 = nt: streamed, evicted first from L2)
template <int AUX = 0>
__device__ __forceinline__ void glds16(const void* src, void* lds_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_base, 16, 0, AUX);
}

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef float f32x8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef short v4i16_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ bf16x8_t as_bf16x8(const uint4& v) { return __builtin_bit_cast(bf16x8_t, v); }

// x of this lane and of lane ^ 32, through v_permlane32_swap (a VALU lane
// swap; __shfl_xor(x, 32) goes through an LDS ds_bpermute round trip).
// After the swap one result holds this lane's value and the other the
// partner half's, so symmetric ops (max, +) need not know which is which.
__device__ __forceinline__ float half_swap_max(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __builtin_fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}

__device__ __forceinline__ float half_swap_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// ---- FP8 KV cache (OCP e4m3fn, gfx950's native fp8): unit scale, values
// saturated to +-448 on the way in (the hardware conversion does not clamp).
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float fp8_sat(float x) { return __builtin_fminf(__builtin_fmaxf(x, -448.f), 448.f); }

// 4 floats -> 4 e4m3 bytes (v_cvt_pk_fp8_f32 x2)
__device__ __forceinline__ uint32_t pack_fp8x4(const float* f) {
    const uint32_t lo = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_sat(f[0]), fp8_sat(f[1]), 0, false);
    return __builtin_amdgcn_cvt_pk_fp8_f32(fp8_sat(f[2]), fp8_sat(f[3]), lo, true);
}

// 4 floats rounded to bf16 first, then e4m3: the bytes of a K-cache append
// (the reference rotates the bf16 projection in fp32, rounds to bf16, then
// encodes; a direct fp32 -> e4m3 differs by one e4m3 step where the bf16
// rounding lands on an e4m3 midpoint)
__device__ __forceinline__ uint32_t pack_fp8x4_bf16r(const float* f) {
    float r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = bf2f(f2bf(f[i]));
    return pack_fp8x4(r);
}

// 8 bf16 (uint4) -> 8 e4m3 bytes (uint2)
__device__ __forceinline__ uint2 bf16x8_to_fp8x8(const uint4& v) {
    float f[8];
    unpack8(v, f);
    return make_uint2(pack_fp8x4(f), pack_fp8x4(f + 4));
}

// 4 e4m3 bytes -> 4 bf16 (uint2): v_cvt_scalef32_pk_bf16_fp8 x2 (scale 1)
__device__ __forceinline__ uint2 fp8x4_to_bf16x4(uint32_t v) {
    return make_uint2(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.f, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v, 1.f, true)));
}

// 8 e4m3 bytes -> 8 bf16 (uint4)
__device__ __forceinline__ uint4 fp8x8_to_bf16x8(const uint2& v) {
    const uint2 a = fp8x4_to_bf16x4(v.x), b = fp8x4_to_bf16x4(v.y);
    return make_uint4(a.x, a.y, b.x, b.y);
}

// ---- MXFP8 (e4m3 bytes + one E8M0 exponent per 32 elements)
// E8M0 exponent of a 32-element block of max |x| = amax: the smallest e with
// amax / 2^e <= 448 (e4m3's largest normal), clamped to the format
__device__ __forceinline__ int mx_exp(float amax) {
    if (!(amax > 0.f)) return 0;
    int e;
    frexpf(amax * (1.f / 448.f), &e);  // amax / 448 = f * 2^e, f in [0.5, 1)
    return e < -127 ? -127 : (e > 127 ? 127 : e);
}

// ---- per-row scaled FP8 KV cache (kv_dtype fp8s, dmcp/ops/reference.py
// kv_encode_scaled): beside the e4m3 bytes one exponent byte per cached row
// (layer, slot, kv head, position), e + 127 with e = mx_exp(amax of the row's D
// bf16 values); the stored element is e4m3(x * 2^-e), the decoded value
// e4m3 * 2^(byte - 127).  Readers take ANY byte, not only the minimal one.
// 2^(byte - 127) as a float (byte 0: the subnormal 2^-127).  Byte 255 is not
// a scale (E8M0's NaN; 2^128 is no fp32 value): no writer produces it (e <= 120
// for a finite amax) and a reader's result for it is undefined.
__device__ __forceinline__ float kv_scale_f(uint32_t byte) {
    return __uint_as_float(byte ? byte << 23 : 0x00400000u);
}

// 2^-e for a row exponent e of mx_exp (e in [-127, 120] for finite fp32 amax)
__device__ __forceinline__ float kv_inv_scale_f(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }

// 8 e4m3 bytes of a row with scale sc = kv_scale_f(byte) -> 8 bf16: the
// conversion instruction takes the scale as an operand, so a scaled row
// widens in as many instructions as an unscaled one, and exactly (3 mantissa
// bits times a power of two)
__device__ __forceinline__ uint4 fp8x8_to_bf16x8_s(const uint2& v, float sc) {
    return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.x, sc, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.x, sc, true)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.y, sc, false)),
                      __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(v.y, sc, true)));
}

// The exponent of a cached row from each lane's partial amax: a head is D/8
// consecutive lanes (8 at D = 64, 16 at D = 128) aligned to their count, in
// the RoPE mapping (4 + 4 values a lane) and in the V mapping (8 values a
// lane) alike -- qk_norm_quad's shuffle pattern.  Every lane of the head
// must be active; D is 64 or 128.
__device__ __forceinline__ int kv_head_exp(float amax, int D) {
#pragma unroll
    for (int m = 1; m < 8; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, kWave));
    if (D == 128) amax = fmaxf(amax, __shfl_xor(amax, 8, kWave));
    return mx_exp(amax);
}

// A K head's 4 + 4 rotated values of this lane -> bf16-rounded, scaled by the
// head's 2^-e, as two e4m3 words; returns e
__device__ __forceinline__ int kv_scaled_pack_k(const float* o1, const float* o2, int D, uint32_t& w1, uint32_t& w2) {
    float r1[4], r2[4], amax = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r1[j] = bf2f(f2bf(o1[j]));
        r2[j] = bf2f(f2bf(o2[j]));
        amax = fmaxf(amax, fmaxf(fabsf(r1[j]), fabsf(r2[j])));
    }
    const int e = kv_head_exp(amax, D);
    const float inv = kv_inv_scale_f(e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        r1[j] *= inv;
        r2[j] *= inv;
    }
    w1 = pack_fp8x4(r1);
    w2 = pack_fp8x4(r2);
    return e;
}

// A V head's 8 bf16 values of this lane -> scaled e4m3 bytes; returns e
__device__ __forceinline__ int kv_scaled_pack_v(const uint4& v, int D, uint2& w) {
    float f[8], amax = 0.f;
    unpack8(v, f);
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf(f[j]));
    const int e = kv_head_exp(amax, D);
    const float inv = kv_inv_scale_f(e);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] *= inv;
    w = make_uint2(pack_fp8x4(f), pack_fp8x4(f + 4));
    return e;
}

// byte address of element `off` of a bf16 or fp8 (KV8) cache
template <bool KV8>
__device__ __forceinline__ const void* kv_ptr(const void* base, size_t off) {
    return static_cast<const uint8_t*>(base) + off * (KV8 ? 1 : 2);
}

// h[0..7] += sum over split-K slices s < S of part[(s * M + m) * N + 8 idx ..
// + 7] (fp32 partials), RSU slices' loads in flight at once: a plain loop
// over s waited for each slice before issuing the next (S serial round trips
// per reduction).  Branch-free (a guarded add let the loads sink to their
// uses); the clamped surplus loads repeat the last slice with weight 0.
template <int RSU = 4>
__device__ __forceinline__ void sum_slices8(const float* __restrict__ part, int S, int M, int m, int N, int idx,
                                            float (&h)[8]) {
    for (int s0 = 0; s0 < S; s0 += RSU) {
        float4 a[RSU], b[RSU];
#pragma unroll
        for (int j = 0; j < RSU; ++j) {
            const float4* pp = reinterpret_cast<const float4*>(part + ((size_t)min(s0 + j, S - 1) * M + m) * N);
            a[j] = pp[2 * idx];
            b[j] = pp[2 * idx + 1];
        }
#pragma unroll
        for (int j = 0; j < RSU; ++j) {
            const float u = s0 + j < S ? 1.f : 0.f;
            h[0] = fmaf(u, a[j].x, h[0]); h[1] = fmaf(u, a[j].y, h[1]);
            h[2] = fmaf(u, a[j].z, h[2]); h[3] = fmaf(u, a[j].w, h[3]);
            h[4] = fmaf(u, b[j].x, h[4]); h[5] = fmaf(u, b[j].y, h[5]);
            h[6] = fmaf(u, b[j].z, h[6]); h[7] = fmaf(u, b[j].w, h[7]);
        }
    }
}

// ---- temperature sampling as a perturbed argmax (Gumbel-max): the id with
// the highest bf16(logit) / T + g_v, g_v independent standard Gumbel noise, is
// an exact sample of softmax(logits / T) over the allowed ids, so the
// selection kernels keep their tiles, pair reduction and launch count.  The
// noise is a counter-based hash of (seed, slot, position, id) in uint32
// arithmetic -- the same bits here and in dmcp/ops/reference.py gumbel_bits:
//   key(row)     = fmix32(seed ^ fmix32(slot * 0x9E3779B1 + position))
//   bits(row, v) = fmix32(key(row) + v * 0x9E3779B1)
//   u = ((bits >> 9) + 0.5) * 2^-23   (exact in fp32, inside (0, 1))
//   g = -log(-log(u))                 (logf, not the fast intrinsic)
__device__ __forceinline__ uint32_t fmix32(uint32_t h) {  // MurmurHash3's finaliser
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t gumbel_key(uint32_t seed, int slot, int position) {
    return fmix32(seed ^ fmix32((uint32_t)slot * 0x9E3779B1u + (uint32_t)position));
}

// score of id v: x (a bf16-rounded logit) / T + g_v; one call per ALLOWED id
// (two logs: callers skip the ids their mask excludes)
__device__ __forceinline__ float gumbel_score(float x, float inv_t, uint32_t key, int v) {
    const uint32_t bits = fmix32(key + (uint32_t)v * 0x9E3779B1u);
    const float u = (float)((bits >> 9) * 2u + 1u) * 0x1p-24f;  // (2 k + 1) / 2^24, k < 2^23: exact
    return fmaf(x, inv_t, -logf(-logf(u)));
}

// The sampling variants' extra kernel argument (per-row keys: the step's
// slots and positions); the greedy instantiations take an empty struct, so
// their code does not change.  Rows with slot < 0 (padding) draw nothing.
struct SampleKeys {
    const int32_t* slots;
    const int32_t* positions;
    uint32_t seed;
    float inv_t;
};
struct NoSampleKeys {};
template <bool SAMPLE>
using sample_keys_t = std::conditional_t<SAMPLE, SampleKeys, NoSampleKeys>;
template <bool SAMPLE>
inline sample_keys_t<SAMPLE> pick_keys(const SampleKeys& sk) {
    if constexpr (SAMPLE) return sk;
    else return {};
}

// ---- repetition / presence penalty (dmcp/ops/reference.py penalize): an
// allowed id whose bit is set in the row's history (a bitset row per KV slot,
// hwords words each) competes with
//   x' = bf16_rne((x > 0 ? x * inv_theta : x * theta) - alpha)
// instead of its bf16 logit x; everything downstream (argmax, Gumbel score,
// truncation keys) works on x' unchanged.  The multiply and the subtract are
// rounded separately (no fma contraction), as the reference's two fp32 ops.
__device__ __forceinline__ float penalize(float x, float theta, float inv_theta, float alpha) {
    const float y = __fsub_rn(x > 0.f ? __fmul_rn(x, inv_theta) : __fmul_rn(x, theta), alpha);
    return bf2f(f2bf(y));
}

// The PENAL variants' extra kernel argument; the other instantiations take an
// empty struct, so their code does not change.  A row is penalised when its
// slot is in [0, n_slots) and its mask row's flag (rows, optional) is set.
struct PenaltyKeys {
    const uint32_t* history;  // [n_slots, hwords]
    const int32_t* slots;     // [rows of the launch]
    const int32_t* rows;      // per mask row flags, nullptr = every row
    int hwords, n_slots, n_rows;
    float theta, inv_theta, alpha;
};
struct NoPenaltyKeys {};
template <bool PENAL>
using penalty_keys_t = std::conditional_t<PENAL, PenaltyKeys, NoPenaltyKeys>;
template <bool PENAL>
inline penalty_keys_t<PENAL> pick_penalty(const PenaltyKeys& pk) {
    if constexpr (PENAL) return pk;
    else return {};
}

// the history row of launch row m under mask row mr, nullptr when the row is
// not penalised (padding, a slot outside the table, a choice mask)
__device__ __forceinline__ const uint32_t* penalty_row(const PenaltyKeys& pk, int m, int mr) {
    const int slot = pk.slots[m];
    if (slot < 0 || slot >= pk.n_slots) return nullptr;
    if (pk.rows && (mr < 0 || mr >= pk.n_rows || pk.rows[mr] == 0)) return nullptr;
    return pk.history + (size_t)slot * pk.hwords;
}

// the selection kernels' merge rule: the highest value, the lowest id among ties
__device__ __forceinline__ void argmax_take(float x, int v, float& best, int& bi) {
    if (x > best || (x == best && v < bi)) { best = x; bi = v; }
}

// The LM head's per-row selection from per-tile (max, id) pairs (wgemm.hip /
// tgemm.hip MODE_ARGMAX write best[tile * M + row]): the highest value, the
// lowest id among ties; 0 when the mask allowed nothing (as masked_argmax).
// One wave per row; each lane keeps 8 pairs' loads in flight (a plain
// strided loop waited for every load: ~30 serial round trips per row at
// 128,256 ids).  A clamped duplicate of the last pair never changes the result.
__global__ __launch_bounds__(kBlock) void argmax_pairs_kernel(const float2* __restrict__ best, int ntiles, int M,
                                                              int32_t* __restrict__ ids) {
    constexpr int U = 8;
    const int lane = threadIdx.x & (kWave - 1);
    const int m = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (m >= M) return;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int t0 = lane; t0 < ntiles; t0 += U * kWave) {
        float2 p[U];
#pragma unroll
        for (int j = 0; j < U; ++j) p[j] = best[(size_t)min(t0 + j * kWave, ntiles - 1) * M + m];
#pragma unroll
        for (int j = 0; j < U; ++j) {
            const int pi = __float_as_int(p[j].y);
            if (p[j].x > bv || (p[j].x == bv && pi < bi)) { bv = p[j].x; bi = pi; }
        }
    }
#pragma unroll
    for (int msk = 32; msk >= 1; msk >>= 1) {
        const float ob = __shfl_xor(bv, msk, kWave);
        const int oi = __shfl_xor(bi, msk, kWave);
        if (ob > bv || (ob == bv && oi < bi)) { bv = ob; bi = oi; }
    }
    if (lane == 0) ids[m] = bi == 0x7fffffff ? 0 : bi;
}

}  // namespace
