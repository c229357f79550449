// The split-K reductions of the decode GEMM families (wgemm.hip, tgemm.hip,
// pgemm.hip's wmx_kernel).  All three write fp32 partials part[S, M, N]; one
// block per row sums the S slices and applies the consumer:
//
//   * residual add + RMSNorm of the next op, output bf16 or MXFP8;
//   * QKV bias + RoPE + q write + KV-cache append (bf16 or fp8 KV).
//
// These entry points are the only launch sites of the kernels below.
#include "dmcp_common.hpp"

namespace {

// split-K slices whose partials the reductions below load at once
constexpr int RSU = 4;

// split-K reduction + residual add + RMSNorm of the next op (one block per
// row): resid += bf16(sum_s part[s]); out = RMSNorm(resid) * gw.  The GEMM
// output is rounded to bf16 before the add and the stream after it (what
// F.linear + add_rmsnorm compute).
template <int VPT>
__global__ __launch_bounds__(kBlock) void reduce_resid_norm_kernel(const float* __restrict__ part, int S,
                                                                   uint16_t* __restrict__ resid,
                                                                   const uint16_t* __restrict__ gw,
                                                                   uint16_t* __restrict__ out, int M, int N,
                                                                   float eps) {
    const int m = blockIdx.x;
    const int nvec = N >> 3;
    float h[VPT][8];
    uint4 rv[VPT], wv[VPT];
    uint4* rr = reinterpret_cast<uint4*>(resid + (size_t)m * N);
    const uint4* wr = reinterpret_cast<const uint4*>(gw);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        if (idx < nvec) {
            rv[i] = rr[idx];
            wv[i] = wr[idx];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) h[i][j] = 0.f;
    }
    // the partials of RSU slices in flight at once (a plain loop over s waited
    // for each slice's loads before issuing the next: S serial round trips)
    for (int s0 = 0; s0 < S; s0 += RSU) {
        float4 a[RSU][VPT], b[RSU][VPT];
#pragma unroll
        for (int j = 0; j < RSU; ++j) {
            const float4* pp = reinterpret_cast<const float4*>(part + ((size_t)min(s0 + j, S - 1) * M + m) * N);
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                const int idx = min(threadIdx.x + i * kBlock, nvec - 1);
                a[j][i] = pp[2 * idx];
                b[j][i] = pp[2 * idx + 1];
            }
        }
#pragma unroll
        for (int j = 0; j < RSU; ++j) {
            const float u = s0 + j < S ? 1.f : 0.f;  // branch-free: a branch let the loads sink to their uses
#pragma unroll
            for (int i = 0; i < VPT; ++i) {
                h[i][0] = fmaf(u, a[j][i].x, h[i][0]); h[i][1] = fmaf(u, a[j][i].y, h[i][1]);
                h[i][2] = fmaf(u, a[j][i].z, h[i][2]); h[i][3] = fmaf(u, a[j][i].w, h[i][3]);
                h[i][4] = fmaf(u, b[j][i].x, h[i][4]); h[i][5] = fmaf(u, b[j][i].y, h[i][5]);
                h[i][6] = fmaf(u, b[j][i].z, h[i][6]); h[i][7] = fmaf(u, b[j][i].w, h[i][7]);
            }
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        if (idx < nvec) {
            float yv[8], r[8];
            unpack8(pack8(h[i]), yv);
            unpack8(rv[i], r);
#pragma unroll
            for (int j = 0; j < 8; ++j) yv[j] += r[j];
            const uint4 packed = pack8(yv);
            rr[idx] = packed;
            unpack8(packed, h[i]);
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += h[i][j] * h[i][j];
        }
    }
    __shared__ float red[kBlock / kWave];
    ss = wave_sum(ss);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kBlock / kWave; ++i) tot += red[i];
    const float inv = rsqrtf(tot / (float)N + eps);
    uint4* orow = reinterpret_cast<uint4*>(out + (size_t)m * N);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        if (idx < nvec) {
            float gv[8], o[8];
            unpack8(wv[i], gv);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = h[i][j] * inv * gv[j];
            orow[idx] = pack8(o);
        }
    }
}

// split-K reduction of the QKV projection + rotate-half RoPE on q and k, q
// written out, k / v appended to the KV cache (bf16, or KV8 fp8 e4m3) at
// (slot[t], :, pos[t], :) -- dmcp_kernels.hip::rope_kv_kernel over an LDS row
// of the bf16-rounded sum (what F.linear + rope_kv compute).  QKN: the
// per-head q / k RMSNorm (qk_norm_quad) on the bf16 row ahead of the rotation.
// SC: the per-row scaled fp8 cache (KV8 only; D 64 or 128), as rope_kv_kernel's.
template <bool KV8, bool QKN = false, bool SC = false>
__global__ __launch_bounds__(kBlock) void reduce_rope_kv_kernel(
    const float* __restrict__ part, int S, int M, const int32_t* __restrict__ pos, const int32_t* __restrict__ slot,
    const float2* __restrict__ cos_sin, uint16_t* __restrict__ q_out, void* __restrict__ k_cache,
    void* __restrict__ v_cache, int Hq, int Hkv, int D, int max_seq, int max_pos, int num_slots,
    const uint16_t* __restrict__ bias, const uint16_t* __restrict__ qn = nullptr,
    const uint16_t* __restrict__ kn = nullptr, float eps = 0.f, uint8_t* __restrict__ k_scale = nullptr,
    uint8_t* __restrict__ v_scale = nullptr) {
    static_assert(KV8 || !SC, "scaled caches are fp8");
    __shared__ uint4 rowbuf[8192 / 8];
    const int t = blockIdx.x;
    const int N = (Hq + 2 * Hkv) * D;
    const int nvec = N >> 3;
    for (int idx = threadIdx.x; idx < nvec; idx += kBlock) {
        float h[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        sum_slices8(part, S, M, t, N, idx, h);
        if (bias) {  // projection bias [N] bf16, on the fp32 sum
            float b[8];
            unpack8(reinterpret_cast<const uint4*>(bias)[idx], b);
#pragma unroll
            for (int j = 0; j < 8; ++j) h[j] += b[j];
        }
        rowbuf[idx] = pack8(h);
    }
    __syncthreads();
    const uint16_t* row = reinterpret_cast<const uint16_t*>(rowbuf);
    const int p = pos[t];
    const int sl = slot[t];
    const bool write_cache = (p >= 0 && p < max_seq && sl >= 0 && sl < num_slots);
    const int half = D >> 1;
    const int quads = half >> 2;
    const float2* cs = cos_sin + (size_t)min(max(p, 0), max_pos - 1) * half;
    const int nunits = (Hq + Hkv) * quads;
    for (int uu = threadIdx.x; uu < nunits; uu += kBlock) {
        const int hh = uu / quads;
        const int d0 = (uu - hh * quads) * 4;
        const uint16_t* src = row + (size_t)hh * D;
        float x1[4], x2[4], o1[4], o2[4];
        unpack4(*reinterpret_cast<const uint2*>(src + d0), x1);
        unpack4(*reinterpret_cast<const uint2*>(src + half + d0), x2);
        if constexpr (QKN) qk_norm_quad(x1, x2, hh < Hq ? qn : kn, d0, D, eps);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float2 c = cs[d0 + j];
            o1[j] = x1[j] * c.x - x2[j] * c.y;
            o2[j] = x2[j] * c.x + x1[j] * c.y;
        }
        if (hh < Hq) {
            uint16_t* dst = q_out + ((size_t)t * Hq + hh) * D;
            *reinterpret_cast<uint2*>(dst + d0) = pack4(o1);
            *reinterpret_cast<uint2*>(dst + half + d0) = pack4(o2);
            continue;
        }
        if (!write_cache) continue;
        const size_t kofs = (((size_t)sl * Hkv + (hh - Hq)) * max_seq + p) * D;
        if constexpr (SC) {
            uint8_t* dst = static_cast<uint8_t*>(k_cache) + kofs;
            uint32_t w1, w2;
            const int e = kv_scaled_pack_k(o1, o2, D, w1, w2);
            *reinterpret_cast<uint32_t*>(dst + d0) = w1;
            *reinterpret_cast<uint32_t*>(dst + half + d0) = w2;
            if (d0 == 0) k_scale[((size_t)sl * Hkv + (hh - Hq)) * max_seq + p] = (uint8_t)(e + 127);
        } else if constexpr (KV8) {
            uint8_t* dst = static_cast<uint8_t*>(k_cache) + kofs;
            *reinterpret_cast<uint32_t*>(dst + d0) = pack_fp8x4_bf16r(o1);
            *reinterpret_cast<uint32_t*>(dst + half + d0) = pack_fp8x4_bf16r(o2);
        } else {
            uint16_t* dst = static_cast<uint16_t*>(k_cache) + kofs;
            *reinterpret_cast<uint2*>(dst + d0) = pack4(o1);
            *reinterpret_cast<uint2*>(dst + half + d0) = pack4(o2);
        }
    }
    if (!write_cache) return;
    const int vvec = (Hkv * D) >> 3;
    const uint4* vsrc = rowbuf + (((Hq + Hkv) * D) >> 3);
    for (int uu = threadIdx.x; uu < vvec; uu += kBlock) {
        const int e = uu << 3;
        const int kh = e / D;
        const int d = e - kh * D;
        const size_t vofs = (((size_t)sl * Hkv + kh) * max_seq + p) * D + d;
        if constexpr (SC) {
            uint2 w;
            const int ve = kv_scaled_pack_v(vsrc[uu], D, w);
            *reinterpret_cast<uint2*>(static_cast<uint8_t*>(v_cache) + vofs) = w;
            if (d == 0) v_scale[((size_t)sl * Hkv + kh) * max_seq + p] = (uint8_t)(ve + 127);
        } else if constexpr (KV8)
            *reinterpret_cast<uint2*>(static_cast<uint8_t*>(v_cache) + vofs) = bf16x8_to_fp8x8(vsrc[uu]);
        else
            *reinterpret_cast<uint4*>(static_cast<uint16_t*>(v_cache) + vofs) = vsrc[uu];
    }
}

// split-K reduction + residual add + RMSNorm, output MXFP8 (the next MX
// GEMM's activation): resid += bf16(sum_s part[s]); h = RMSNorm(resid) * w.
// One block per row, N % 2048 == 0, N <= 8192.
template <int VPT>
__global__ __launch_bounds__(kBlock) void reduce_resid_norm_mx_kernel(const float* __restrict__ part, int S,
                                                                      uint16_t* __restrict__ resid,
                                                                      const uint16_t* __restrict__ w,
                                                                      uint8_t* __restrict__ q, uint8_t* __restrict__ s,
                                                                      int M, int N, float eps) {
    const int m = blockIdx.x;
    uint4* rr = reinterpret_cast<uint4*>(resid + (size_t)m * N);
    const uint4* wr = reinterpret_cast<const uint4*>(w);
    float h[VPT][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        sum_slices8(part, S, M, m, N, idx, acc);
        float y[8], r[8];
        unpack8(pack8(acc), y);  // the GEMM output rounded to bf16, as F.linear's
        unpack8(rr[idx], r);
#pragma unroll
        for (int j = 0; j < 8; ++j) y[j] += r[j];
        const uint4 packed = pack8(y);
        rr[idx] = packed;
        unpack8(packed, h[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += h[i][j] * h[i][j];
    }
    __shared__ float red[kBlock / kWave];
    ss = wave_sum(ss);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int i = 0; i < kBlock / kWave; ++i) tot += red[i];
    const float inv = rsqrtf(tot / (float)N + eps);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        float g[8], o[8];
        unpack8(wr[idx], g);
        float amax = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = h[i][j] * inv * g[j];
            amax = __builtin_fmaxf(amax, __builtin_fabsf(o[j]));
        }
        amax = __builtin_fmaxf(amax, __shfl_xor(amax, 1, kWave));
        amax = __builtin_fmaxf(amax, __shfl_xor(amax, 2, kWave));
        const int ex = mx_exp(amax);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = ldexpf(o[j], -ex);
        reinterpret_cast<uint2*>(q + (size_t)m * N)[idx] = make_uint2(pack_fp8x4(o), pack_fp8x4(o + 4));
        if ((idx & 3) == 0) s[(size_t)m * (N >> 5) + (idx >> 2)] = (uint8_t)(ex + 127);
    }
}

}  // namespace

extern "C" {

// resid += bf16(sum of the S partials); out = RMSNorm(resid) * g
int dmcp_reduce_resid_norm(const void* part, int S, void* resid, const void* g, void* out, int M, int N, float eps,
                           void* stream) {
    if (M <= 0) return 0;
    if (!part || S < 1 || !resid || !g || !out || N % 8 != 0 || N > 8 * 4 * kBlock) return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    const int vpt = (N / 8 + kBlock - 1) / kBlock;
    auto pp = (const float*)part;
    auto rr = (uint16_t*)resid;
    auto gg = (const uint16_t*)g;
    auto oo = (uint16_t*)out;
    if (vpt == 1) reduce_resid_norm_kernel<1><<<M, kBlock, 0, st>>>(pp, S, rr, gg, oo, M, N, eps);
    else if (vpt == 2) reduce_resid_norm_kernel<2><<<M, kBlock, 0, st>>>(pp, S, rr, gg, oo, M, N, eps);
    else reduce_resid_norm_kernel<4><<<M, kBlock, 0, st>>>(pp, S, rr, gg, oo, M, N, eps);
    return hipGetLastError();
}

// RoPE + q write + KV append of QKV partials [S, M, (Hq + 2 Hkv) D]
// (+ bias [N] bf16, nullptr = none)
int dmcp_reduce_rope_kv(const void* part, int S, const void* pos, const void* slot, const void* cos_sin, void* q_out,
                        void* k_cache, void* v_cache, int M, int Hq, int Hkv, int D, int max_seq, int max_pos,
                        int num_slots, int kv8, void* stream, const void* bias) {
    if (M <= 0) return 0;
    if (!part || S < 1 || D % 16 != 0 || (Hq + 2 * Hkv) * D > 8192 || !pos || !slot || !cos_sin || !q_out ||
        !k_cache || !v_cache || max_pos <= 0)
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto pp = (const float*)part;
    auto bb = (const uint16_t*)bias;  // [N] bf16 or nullptr
    if (kv8)
        reduce_rope_kv_kernel<true><<<M, kBlock, 0, st>>>(pp, S, M, (const int32_t*)pos, (const int32_t*)slot,
                                                          (const float2*)cos_sin, (uint16_t*)q_out, k_cache, v_cache,
                                                          Hq, Hkv, D, max_seq, max_pos, num_slots, bb);
    else
        reduce_rope_kv_kernel<false><<<M, kBlock, 0, st>>>(pp, S, M, (const int32_t*)pos, (const int32_t*)slot,
                                                           (const float2*)cos_sin, (uint16_t*)q_out, k_cache,
                                                           v_cache, Hq, Hkv, D, max_seq, max_pos, num_slots, bb);
    return hipGetLastError();
}

// dmcp_reduce_rope_kv with the per-head q / k RMSNorm (weights qn / kn [D]
// bf16) between the bias and the rotation; D is 64 or 128
int dmcp_reduce_rope_kv_norm(const void* part, int S, const void* pos, const void* slot, const void* cos_sin,
                             void* q_out, void* k_cache, void* v_cache, int M, int Hq, int Hkv, int D, int max_seq,
                             int max_pos, int num_slots, int kv8, void* stream, const void* bias, const void* qn,
                             const void* kn, float eps) {
    if (M <= 0) return 0;
    if (!part || S < 1 || (D != 64 && D != 128) || (Hq + 2 * Hkv) * D > 8192 || !pos || !slot || !cos_sin ||
        !q_out || !k_cache || !v_cache || max_pos <= 0 || !qn || !kn)
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto pp = (const float*)part;
    auto bb = (const uint16_t*)bias;  // [N] bf16 or nullptr
    if (kv8)
        reduce_rope_kv_kernel<true, true><<<M, kBlock, 0, st>>>(
            pp, S, M, (const int32_t*)pos, (const int32_t*)slot, (const float2*)cos_sin, (uint16_t*)q_out, k_cache,
            v_cache, Hq, Hkv, D, max_seq, max_pos, num_slots, bb, (const uint16_t*)qn, (const uint16_t*)kn, eps);
    else
        reduce_rope_kv_kernel<false, true><<<M, kBlock, 0, st>>>(
            pp, S, M, (const int32_t*)pos, (const int32_t*)slot, (const float2*)cos_sin, (uint16_t*)q_out, k_cache,
            v_cache, Hq, Hkv, D, max_seq, max_pos, num_slots, bb, (const uint16_t*)qn, (const uint16_t*)kn, eps);
    return hipGetLastError();
}

// dmcp_reduce_rope_kv / _norm (qn / kn nullptr = no QK-norm) appending to a
// per-row scaled fp8 cache: k_scale / v_scale uint8 [S, Hkv, max_seq]; D is 64
// or 128
int dmcp_reduce_rope_kv_scaled(const void* part, int S, const void* pos, const void* slot, const void* cos_sin,
                               void* q_out, void* k_cache, void* v_cache, int M, int Hq, int Hkv, int D, int max_seq,
                               int max_pos, int num_slots, void* stream, const void* bias, const void* qn,
                               const void* kn, float eps, void* k_scale, void* v_scale) {
    if (M <= 0) return 0;
    if (!part || S < 1 || (D != 64 && D != 128) || (Hq + 2 * Hkv) * D > 8192 || !pos || !slot || !cos_sin ||
        !q_out || !k_cache || !v_cache || max_pos <= 0 || (!qn != !kn) || !k_scale || !v_scale)
        return hipErrorInvalidValue;
    auto st = (hipStream_t)stream;
    auto pp = (const float*)part;
    auto bb = (const uint16_t*)bias;  // [N] bf16 or nullptr
    if (qn)
        reduce_rope_kv_kernel<true, true, true><<<M, kBlock, 0, st>>>(
            pp, S, M, (const int32_t*)pos, (const int32_t*)slot, (const float2*)cos_sin, (uint16_t*)q_out, k_cache,
            v_cache, Hq, Hkv, D, max_seq, max_pos, num_slots, bb, (const uint16_t*)qn, (const uint16_t*)kn, eps,
            (uint8_t*)k_scale, (uint8_t*)v_scale);
    else
        reduce_rope_kv_kernel<true, false, true><<<M, kBlock, 0, st>>>(
            pp, S, M, (const int32_t*)pos, (const int32_t*)slot, (const float2*)cos_sin, (uint16_t*)q_out, k_cache,
            v_cache, Hq, Hkv, D, max_seq, max_pos, num_slots, bb, nullptr, nullptr, 0.f, (uint8_t*)k_scale,
            (uint8_t*)v_scale);
    return hipGetLastError();
}

// resid += bf16(sum of the S partials); RMSNorm(resid) * w -> MXFP8 q / s
int dmcp_reduce_resid_norm_mx(const void* part, int S, void* resid, const void* w, void* q, void* s, int M, int N,
                              float eps, void* stream) {
    if (M <= 0) return 0;
    if (!part || S < 1 || !resid || !w || !q || !s || N % (8 * kBlock) != 0 || N > 4 * 8 * kBlock)
        return hipErrorInvalidValue;
    const int vpt = N / (8 * kBlock);
    auto st = (hipStream_t)stream;
    auto pp = (const float*)part;
    auto rr = (uint16_t*)resid;
    auto ww = (const uint16_t*)w;
    auto qq = (uint8_t*)q;
    auto ss = (uint8_t*)s;
    if (vpt == 1) reduce_resid_norm_mx_kernel<1><<<M, kBlock, 0, st>>>(pp, S, rr, ww, qq, ss, M, N, eps);
    else if (vpt == 2) reduce_resid_norm_mx_kernel<2><<<M, kBlock, 0, st>>>(pp, S, rr, ww, qq, ss, M, N, eps);
    else if (vpt == 3) reduce_resid_norm_mx_kernel<3><<<M, kBlock, 0, st>>>(pp, S, rr, ww, qq, ss, M, N, eps);
    else reduce_resid_norm_mx_kernel<4><<<M, kBlock, 0, st>>>(pp, S, rr, ww, qq, ss, M, N, eps);
    return hipGetLastError();
}

}  // extern "C"
