// Routed expert MLP (Qwen3-MoE sparse block) for gfx950 / MI355X:
//
//   ids, p = top-k of softmax(h . Wr^T)            (fp32, ties to the lower id)
//   y[t]   = sum_j p[t, j] * down_e(silu(gate_e(h[t])) * up_e(h[t])),  e = ids[t, j]
//
// bf16 operands, fp32 accumulation on v_mfma_f32_16x16x32_bf16.  Six launches,
// every grid sized by host-known upper bounds, so the whole op is capturable
// in a hipGraph although the routing is data dependent:
//
//   1. route    one wave per row: E router dot products (fp32), softmax, k
//               rounds of a wave arg-max (value, then lower id), optional
//               renormalisation -> ids / p [T * k]
//   2. count    one wave per expert scans ids -> cnt [E]
//   3. scatter  one wave per expert: its offset (sum of the counts before
//               it), its pairs in ascending pair order (ballot + popcount: a
//               stable counting sort without atomics) -> perm, and its rows
//               of the tile table (expert, first pair, rows); the last wave
//               writes the tile count
//   4. gate/up  grid (I / 64, ceil(T k / MT) + E): a block owns one row tile
//               and 64 gate + 64 up columns; X rows are gathered through perm
//               into a double-buffered LDS image, weight fragments go from
//               global memory straight to the MFMA A operand (each weight
//               element is used once per block); SwiGLU in the epilogue,
//               act [T k, I] bf16 in grouped order
//   5. down     the same kernel body over act and w_down (128 columns per
//               block), y [T k, H] fp32, one row per pair at the PAIR's index
//               t * k + j, so the combine reads k consecutive rows
//   6. combine  one block per row: m = bf16(sum_j p_j * y_j) in rank order,
//               then exactly add_rmsnorm_kernel's arithmetic (residual add,
//               bf16 residual stream, RMSNorm)
//
// Blocks past the live tile count (a device value) exit at once.  No atomics
// of any kind: every output element has one writer and a fixed summation
// order, so equal inputs give equal bits.
//
// Block-scaled FP8 expert weights (dmcp_moe_mlp_w8; the format is defined in
// dmcp/ops/reference.py, block_fp8_dequant): e4m3 bytes with one fp32
// multiplier per 128 x 128 block.  Steps 4 and 5 then run the same kernel body
// with WT = uint8_t: a lane takes 16 weight bytes per 64-deep chunk, widens
// them exactly to bf16 in registers (fp8x8_to_bf16x8) and feeds the same MFMA;
// the products of a 128-deep K block go to a partial accumulator and the
// block's scale is applied to that fp32 partial sum (acc += s * part), never
// to a weight.  Everything else -- activations, routing, grouping, combine --
// is bf16 / fp32 as above.
//
// Sigmoid routing with shared experts (dmcp_moe_route_sig / dmcp_moe_mlp_sh;
// GLM-4.5, defined in dmcp/ops/reference.py, moe_route_sig_math): step 1 is
// moe_route_sig_kernel -- sigmoid scores, an fp32 bias added for the selection
// only, the unbiased scores renormalised over the k routed ranks and scaled --
// and a shared MLP of width S I rides along as S pseudo-experts E .. E + S - 1
// that every row chooses with weight 1 (a SwiGLU MLP is a sum over slices of
// its intermediate dimension).  Steps 2-6 are the same kernels over E + S
// groups and k + S pairs per row: a shared slice is one group holding all T
// rows, a dense GEMM on the same kernel body.
#include "dmcp_common.hpp"

namespace {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

constexpr int kMaxExperts = 256;
constexpr int kEPL = kMaxExperts / kWave;  // expert slots per lane of the routing wave

// ---------------------------------------------------------------- 1. route
__global__ __launch_bounds__(kBlock) void moe_route_kernel(const uint16_t* __restrict__ h,
                                                           const uint16_t* __restrict__ wr,
                                                           int32_t* __restrict__ ids, float* __restrict__ p, int T,
                                                           int H, int E, int k, int norm) {
    const int lane = threadIdx.x & (kWave - 1);
    const int t = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (t >= T) return;  // whole waves leave; no block-level barrier below
    const uint4* hr = reinterpret_cast<const uint4*>(h + (size_t)t * H);
    const int nvec = H >> 3;
    // logit of expert e lands in lane e % 64, slot e / 64
    float lg[kEPL];
#pragma unroll
    for (int s = 0; s < kEPL; ++s) lg[s] = -INFINITY;
    for (int e = 0; e < E; ++e) {
        const uint4* we = reinterpret_cast<const uint4*>(wr + (size_t)e * H);
        float acc = 0.f;
        for (int v = lane; v < nvec; v += kWave) {
            float a[8], b[8];
            unpack8(hr[v], a);
            unpack8(we[v], b);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(a[j], b[j], acc);
        }
        acc = wave_sum(acc);
        if (!(acc == acc)) acc = -INFINITY;  // a NaN logit never wins, and never blocks the selection
#pragma unroll
        for (int s = 0; s < kEPL; ++s)
            if ((e >> 6) == s && (e & 63) == lane) lg[s] = acc;
    }
    float mx = -INFINITY;
#pragma unroll
    for (int s = 0; s < kEPL; ++s) mx = fmaxf(mx, lg[s]);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m, kWave));
    if (mx == -INFINITY) mx = 0.f;
    float pr[kEPL], sum = 0.f;
#pragma unroll
    for (int s = 0; s < kEPL; ++s) {
        pr[s] = (s * kWave + lane < E) ? expf(lg[s] - mx) : 0.f;
        sum += pr[s];
    }
    sum = wave_sum(sum);
#pragma unroll
    for (int s = 0; s < kEPL; ++s) pr[s] = pr[s] / sum;
    // k rounds of arg-max over the experts not taken yet: the largest
    // probability, the lowest id among equals.  Every round finds one (k <= E
    // and -inf == -inf compares equal), so ids are distinct and in [0, E).
    uint32_t taken = 0u;
    float sel[kEPL];  // rank j's probability in lane j % 64, slot j / 64
#pragma unroll
    for (int s = 0; s < kEPL; ++s) sel[s] = 0.f;
    for (int j = 0; j < k; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int s = 0; s < kEPL; ++s) {
            const int e = s * kWave + lane;
            if (e < E && !((taken >> s) & 1u)) {
                const float v = pr[s] == pr[s] ? pr[s] : -INFINITY;
                if (v > bv || (v == bv && e < bi)) { bv = v; bi = e; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, kWave);
            const int oi = __shfl_xor(bi, m, kWave);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        bi = min(max(bi, 0), E - 1);
        if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
        if (lane == 0) ids[(size_t)t * k + j] = bi;
#pragma unroll
        for (int s = 0; s < kEPL; ++s)
            if ((j >> 6) == s && (j & 63) == lane) sel[s] = bv > 0.f ? bv : 0.f;
    }
    float den = 1.f;
    if (norm) {
        // a butterfly sum: equal probabilities (k a power of two) add up
        // exactly, so p comes out as exactly 1 / k
        float sacc = 0.f;
#pragma unroll
        for (int s = 0; s < kEPL; ++s) sacc += sel[s];
        den = wave_sum(sacc);
        if (!(den > 0.f)) den = 1.f;
    }
#pragma unroll
    for (int s = 0; s < kEPL; ++s) {
        const int j = s * kWave + lane;
        if (j < k) p[(size_t)t * k + j] = sel[s] / den;
    }
}

// ------------------------------------------- 1b. route, sigmoid scores (GLM-4.5)
// The router of GLM-4.5 / DeepSeek-V3-style blocks with one expert group
// (dmcp/ops/reference.py, moe_route_sig_math): s = sigmoid(h . Wr^T); the k
// largest of s + bias (bias fp32 [E], for the selection only; ties to the
// lower id) are chosen; their weights are the unbiased s, divided by
// (sum + 1e-20) when `norm`, then multiplied by `scale`.  A row has k + S
// pairs: after the k routed ones come the S shared pseudo-experts
// (E + s, 1.0), which the grouping and the GEMMs treat as experts E .. E + S - 1
// that every row chooses.
__global__ __launch_bounds__(kBlock) void moe_route_sig_kernel(const uint16_t* __restrict__ h,
                                                               const uint16_t* __restrict__ wr,
                                                               const float* __restrict__ bias,
                                                               int32_t* __restrict__ ids, float* __restrict__ p, int T,
                                                               int H, int E, int k, int S, int norm, float scale) {
    const int lane = threadIdx.x & (kWave - 1);
    const int t = blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
    if (t >= T) return;  // whole waves leave; no block-level barrier below
    const uint4* hr = reinterpret_cast<const uint4*>(h + (size_t)t * H);
    const int nvec = H >> 3;
    const int kk = k + S;
    // expert e lives in lane e % 64, slot e / 64: its score sg and its
    // selection score sc = sg + bias (-inf: no such expert, or a NaN logit)
    float sg[kEPL], sc[kEPL];
#pragma unroll
    for (int s = 0; s < kEPL; ++s) {
        sg[s] = 0.f;
        sc[s] = -INFINITY;
    }
    for (int e = 0; e < E; ++e) {
        const uint4* we = reinterpret_cast<const uint4*>(wr + (size_t)e * H);
        float acc = 0.f;
        for (int v = lane; v < nvec; v += kWave) {
            float a[8], b[8];
            unpack8(hr[v], a);
            unpack8(we[v], b);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(a[j], b[j], acc);
        }
        acc = wave_sum(acc);
        const bool ok = acc == acc;  // a NaN logit never wins, and never blocks the selection
        const float sig = ok ? 1.f / (1.f + expf(-acc)) : 0.f;
        float sel = ok ? sig + bias[e] : -INFINITY;
        if (!(sel == sel)) sel = -INFINITY;
#pragma unroll
        for (int s = 0; s < kEPL; ++s)
            if ((e >> 6) == s && (e & 63) == lane) {
                sg[s] = sig;
                sc[s] = sel;
            }
    }
    // k rounds of arg-max over the experts not taken yet, as in
    // moe_route_kernel: the largest selection score, the lowest id among equals
    uint32_t taken = 0u;
    float sel[kEPL];  // rank j's weight in lane j % 64, slot j / 64
#pragma unroll
    for (int s = 0; s < kEPL; ++s) sel[s] = 0.f;
    for (int j = 0; j < k; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int s = 0; s < kEPL; ++s) {
            const int e = s * kWave + lane;
            if (e < E && !((taken >> s) & 1u)) {
                const float v = sc[s];
                if (v > bv || (v == bv && e < bi)) { bv = v; bi = e; }
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float ov = __shfl_xor(bv, m, kWave);
            const int oi = __shfl_xor(bi, m, kWave);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        bi = min(max(bi, 0), E - 1);
        if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
        if (lane == 0) ids[(size_t)t * kk + j] = bi;
        // the chosen expert's unbiased score, from the lane that holds it
        float mine = 0.f;
#pragma unroll
        for (int s = 0; s < kEPL; ++s)
            if ((bi >> 6) == s) mine = sg[s];
        const float wj = __shfl(mine, bi & 63, kWave);
#pragma unroll
        for (int s = 0; s < kEPL; ++s)
            if ((j >> 6) == s && (j & 63) == lane) sel[s] = wj;
    }
    float den = 1.f;
    if (norm) {
        // a butterfly sum: equal scores (k a power of two) add up exactly,
        // so the weights come out as exactly scale / k
        float sacc = 0.f;
#pragma unroll
        for (int s = 0; s < kEPL; ++s) sacc += sel[s];
        den = wave_sum(sacc) + 1e-20f;
    }
#pragma unroll
    for (int s = 0; s < kEPL; ++s) {
        const int j = s * kWave + lane;
        if (j < k) p[(size_t)t * kk + j] = sel[s] / den * scale;
    }
    if (lane < S) {  // S <= 64 (moe_sh_shape_ok)
        ids[(size_t)t * kk + k + lane] = E + lane;
        p[(size_t)t * kk + k + lane] = 1.f;
    }
}

// ------------------------------------------------------- 2. count, 3. scatter
__global__ __launch_bounds__(kWave) void moe_count_kernel(const int32_t* __restrict__ ids, int32_t* __restrict__ cnt,
                                                          int P) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int c = 0;
    for (int i = lane; i < P; i += kWave) c += ids[i] == e;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, kWave);
    if (lane == 0) cnt[e] = c;
}

// tiles: int32 [max_tiles][3] = (expert, first grouped row, rows)
__global__ __launch_bounds__(kWave) void moe_scatter_kernel(const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ cnt,
                                                            int32_t* __restrict__ offs, int32_t* __restrict__ perm,
                                                            int32_t* __restrict__ tiles, int32_t* __restrict__ ntiles,
                                                            int P, int E, int MT, int max_tiles) {
    const int e = blockIdx.x, lane = threadIdx.x;
    int before = 0, tbefore = 0;
    for (int i = lane; i < e; i += kWave) {
        const int c = cnt[i];
        before += c;
        tbefore += (c + MT - 1) / MT;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        before += __shfl_xor(before, m, kWave);
        tbefore += __shfl_xor(tbefore, m, kWave);
    }
    const int mine = cnt[e];
    const int nt = (mine + MT - 1) / MT;
    if (lane == 0) {
        offs[e] = before;
        if (e == E - 1) {
            offs[E] = before + mine;
            *ntiles = min(tbefore + nt, max_tiles);
        }
    }
    for (int i = lane; i < nt; i += kWave) {
        if (tbefore + i < max_tiles) {
            int32_t* te = tiles + 3 * (size_t)(tbefore + i);
            te[0] = e;
            te[1] = before + i * MT;
            te[2] = min(MT, mine - i * MT);
        }
    }
    // stable placement: pairs of this expert in ascending pair index
    int placed = 0;
    for (int i0 = 0; i0 < P; i0 += kWave) {
        const int i = i0 + lane;
        const bool hit = i < P && ids[i] == e;
        const unsigned long long bal = __ballot(hit);
        if (hit) {
            const int dst = before + placed + __popcll(bal & ((1ull << lane) - 1ull));
            if (dst < P) perm[dst] = i;
        }
        placed += __popcll(bal);
    }
}

// --------------------------------------------------- 4. gate/up, 5. down GEMM
// Y[rows of a tile][columns of the block] = X[rows][K] . W[e][columns][K]^T.
// A wave owns two 16-column weight fragments: columns c0 + 16 wv and the same
// + `second` (gate/up: the up rows, I further down; down: 64 columns on).
// RT 16-row subtiles per tile (MT = 16 RT).  X rows reach LDS in 64-deep K
// chunks, [row][8 x 16 B] with chunk j of row r in slot j ^ (r & 7)
// (conflict-free ds_read_b128 of the B operand), double buffered: chunk c + 1
// is loaded to registers before chunk c's MFMAs and stored after them.
//
// WT = uint16_t: bf16 weights, ws unused.  WT = uint8_t: e4m3 weights with the
// block scales ws (gate/up: [E][2 ceil(N / 128)][ceil(K / 128)], the gate's
// block rows, then the up's; down: [E][ceil(N / 128)][ceil(K / 128)]).  A
// block's 64 gate + 64 up columns, or its 128 down columns, lie inside one
// 128-row scale block, so per 128-deep K block the wave needs one scalar per
// fragment (gate and up differ; down's two fragments share one).  A lane
// takes the 16 bytes k = 16 g .. 16 g + 15 of each 64-deep chunk in one load
// (two chunks per K block; one when K % 128 == 64 ends on a half block) and
// uses 8 of them per MFMA: even g the low half first, odd g the high half
// first, i.e. sub-step kk pairs with the X piece 2 g + (kk ^ (g & 1)).  K is
// permuted inside the chunk, for A and B alike.  The parity flip keeps the
// ds_read_b128 of X conflict-free: in each of the instruction's 16-lane groups
// (eight rows of one g, eight of the next) the two g read pieces of opposite
// parity, which the slot swizzle j ^ (r & 7) sends to disjoint slots of the
// 256-byte bank row, as the bf16 mapping's pieces 4 kk + g and 4 kk + g + 1 are.
template <int RT, bool SWIGLU, typename WT>
__global__ __launch_bounds__(kBlock) void moe_gemm_kernel(const uint16_t* __restrict__ x,
                                                          const WT* __restrict__ w,
                                                          const float* __restrict__ ws,
                                                          const int32_t* __restrict__ perm,
                                                          const int32_t* __restrict__ tiles,
                                                          const int32_t* __restrict__ ntiles, uint16_t* __restrict__ act,
                                                          float* __restrict__ y, int P, int K, int N, int topk) {
    constexpr bool W8 = sizeof(WT) == 1;
    constexpr int LK = W8 ? 16 : 8;  // weight elements of a lane's 16-byte load
    constexpr int MT = RT * 16;
    constexpr int XP = MT * 8 / kBlock > 0 ? MT * 8 / kBlock : 1;  // 16-B pieces per thread per chunk
    static_assert(MT * 8 % kBlock == 0 || MT * 8 < kBlock, "row tile");
    __shared__ uint4 lds[2 * MT * 8];
    __shared__ int32_t srow[MT];

    const int tile = blockIdx.y;
    if (tile >= *ntiles) return;
    const int e = tiles[3 * (size_t)tile], first = tiles[3 * (size_t)tile + 1], rows = tiles[3 * (size_t)tile + 2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int l16 = lane & 15, g = lane >> 4;
    // source row of X per tile row (rows past the tile repeat its first row;
    // their results are never stored): gate/up gathers token perm / k, down
    // reads act in grouped order
    if (tid < MT) {
        const int gr = first + (tid < rows ? tid : 0);
        const int pair = min(max(perm[min(gr, P - 1)], 0), P - 1);
        srow[tid] = SWIGLU ? pair / topk : min(gr, P - 1);
    }
    __syncthreads();

    // weight rows of this wave's two fragments.  SWIGLU: N = I, w [E][2 I][K];
    // else N = H, w [E][H][K]
    const int cblk = SWIGLU ? 64 : 128;
    const int c0 = blockIdx.x * cblk + wv * 16;
    const int c1 = SWIGLU ? c0 : c0 + 64;          // output column of fragment 1
    const bool f1 = SWIGLU || c1 < N;              // fragment 1 exists (H % 128 == 64: the last block's does not)
    const size_t wrows = SWIGLU ? 2 * (size_t)N : (size_t)N;
    const WT* wbase = w + (size_t)e * wrows * K;
    const WT* wa0 = wbase + (size_t)(c0 + l16) * K + g * LK;
    const WT* wa1 = wbase + (size_t)(SWIGLU ? N + c0 + l16 : (f1 ? c1 + l16 : c0 + l16)) * K + g * LK;

    const uint16_t* xsrc[XP];
    int xdst[XP];
    bool xon[XP];
#pragma unroll
    for (int i = 0; i < XP; ++i) {
        const int piece = tid + i * kBlock;        // row = piece / 8, logical 16-B chunk = piece % 8
        xon[i] = piece < MT * 8;
        const int r = xon[i] ? piece >> 3 : 0, j = piece & 7;
        xsrc[i] = x + (size_t)srow[r] * K + j * 8;
        xdst[i] = r * 8 + (j ^ (r & 7));
    }

    f32x4_t acc[2][RT];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
        for (int t = 0; t < RT; ++t) acc[f][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

    const int chunks = K / 64;
    uint4 xr[XP], a[2][2], an[2][2];
#pragma unroll
    for (int i = 0; i < XP; ++i)
        if (xon[i]) lds[xdst[i]] = *reinterpret_cast<const uint4*>(xsrc[i]);
    if constexpr (!W8) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            a[0][kk] = *reinterpret_cast<const uint4*>(wa0 + kk * 32);
            a[1][kk] = *reinterpret_cast<const uint4*>(wa1 + kk * 32);
        }
        __syncthreads();
        for (int c = 0; c < chunks; ++c) {
            const bool more = c + 1 < chunks;
            if (more) {
#pragma unroll
                for (int i = 0; i < XP; ++i)
                    if (xon[i]) xr[i] = *reinterpret_cast<const uint4*>(xsrc[i] + (c + 1) * 64);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    an[0][kk] = *reinterpret_cast<const uint4*>(wa0 + (c + 1) * 64 + kk * 32);
                    an[1][kk] = *reinterpret_cast<const uint4*>(wa1 + (c + 1) * 64 + kk * 32);
                }
            }
            const uint4* xl = lds + (c & 1) * (MT * 8);
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const int r = 16 * t + l16;
                    const bf16x8_t b = as_bf16x8(xl[r * 8 + ((4 * kk + g) ^ (r & 7))]);
                    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a[0][kk]), b, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(a[1][kk]), b, acc[1][t], 0, 0, 0);
                }
            }
            if (more) {
                uint4* xs = lds + ((c + 1) & 1) * (MT * 8);
#pragma unroll
                for (int i = 0; i < XP; ++i)
                    if (xon[i]) xs[xdst[i]] = xr[i];
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    a[0][kk] = an[0][kk];
                    a[1][kk] = an[1][kk];
                }
            }
            // one barrier per chunk: chunk c + 1 is complete, and nobody still
            // reads the buffer that chunk c + 2 will overwrite after the next one
            __syncthreads();
        }
    } else {
        // a[f][hh]: fragment f's 16 bytes of chunk 2 kb + hh.  The K block after
        // this one is in flight while this one multiplies: as many bytes per
        // wave as the bf16 form keeps in flight, over twice the depth.
        const int nkb = (chunks + 1) >> 1;
        const int nbn = (N + 127) >> 7;
        const float* sc0 = ws + ((size_t)e * (SWIGLU ? 2 * nbn : nbn) + (SWIGLU ? blockIdx.x >> 1 : blockIdx.x)) * nkb;
        const float* sc1 = SWIGLU ? sc0 + (size_t)nbn * nkb : sc0;
        const bool odd = g & 1;
        u32x4_t xq[XP];  // chunk c + 1 of X on its way to LDS (a native vector: the array stays in registers)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const int cc = min(hh, chunks - 1);  // half a block: its second slot repeats the first, unused
            a[0][hh] = *reinterpret_cast<const uint4*>(wa0 + cc * 64);
            a[1][hh] = *reinterpret_cast<const uint4*>(wa1 + cc * 64);
        }
        __syncthreads();
        for (int kb = 0; kb < nkb; ++kb) {
            const bool next = kb + 1 < nkb;
            if (next) {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const int cc = min(2 * kb + 2 + hh, chunks - 1);
                    an[0][hh] = *reinterpret_cast<const uint4*>(wa0 + cc * 64);
                    an[1][hh] = *reinterpret_cast<const uint4*>(wa1 + cc * 64);
                }
            }
            const float s0 = sc0[kb], s1 = sc1[kb];
            f32x4_t part[2][RT];
#pragma unroll
            for (int f = 0; f < 2; ++f)
#pragma unroll
                for (int t = 0; t < RT; ++t) part[f][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const int c = 2 * kb + hh;
                if (c >= chunks) break;  // uniform: K % 128 == 64, the last block is one chunk
                const bool more = c + 1 < chunks;
                if (more) {
#pragma unroll
                    for (int i = 0; i < XP; ++i)
                        if (xon[i]) xq[i] = *reinterpret_cast<const u32x4_t*>(xsrc[i] + (c + 1) * 64);
                }
                const uint4* xl = lds + (c & 1) * (MT * 8);
#pragma unroll
                for (int kk = 0; kk < 2; ++kk) {
                    const bool hi = (kk == 1) != odd;
                    const uint4 w0 = fp8x8_to_bf16x8(hi ? make_uint2(a[0][hh].z, a[0][hh].w)
                                                        : make_uint2(a[0][hh].x, a[0][hh].y));
                    const uint4 w1 = fp8x8_to_bf16x8(hi ? make_uint2(a[1][hh].z, a[1][hh].w)
                                                        : make_uint2(a[1][hh].x, a[1][hh].y));
                    const int j = 2 * g + (kk ^ (g & 1));
#pragma unroll
                    for (int t = 0; t < RT; ++t) {
                        const int r = 16 * t + l16;
                        const bf16x8_t b = as_bf16x8(xl[r * 8 + (j ^ (r & 7))]);
                        part[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w0), b, part[0][t], 0, 0, 0);
                        part[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_bf16x8(w1), b, part[1][t], 0, 0, 0);
                    }
                }
                if (more) {
                    u32x4_t* xs = reinterpret_cast<u32x4_t*>(lds + ((c + 1) & 1) * (MT * 8));
#pragma unroll
                    for (int i = 0; i < XP; ++i)
                        if (xon[i]) xs[xdst[i]] = xq[i];
                }
                __syncthreads();  // as in the bf16 loop: one barrier per chunk
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    acc[0][t][i] = fmaf(s0, part[0][t][i], acc[0][t][i]);
                    acc[1][t][i] = fmaf(s1, part[1][t][i], acc[1][t][i]);
                }
            }
            if (next) {
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    a[0][hh] = an[0][hh];
                    a[1][hh] = an[1][hh];
                }
            }
        }
    }

    // lane (l16, g) holds Y[tile row 16 t + l16][fragment column 4 g + i]
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int r = 16 * t + l16;
        if (r >= rows) continue;
        const int gr = first + r;
        if (gr >= P) continue;
        if constexpr (SWIGLU) {
            float o[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) o[i] = silu(acc[0][t][i]) * acc[1][t][i];
            *reinterpret_cast<uint2*>(act + (size_t)gr * N + c0 + 4 * g) = pack4(o);
        } else {
            const int pair = min(max(perm[gr], 0), P - 1);
            float* dst = y + (size_t)pair * N;
            *reinterpret_cast<float4*>(dst + c0 + 4 * g) =
                make_float4(acc[0][t][0], acc[0][t][1], acc[0][t][2], acc[0][t][3]);
            if (f1)
                *reinterpret_cast<float4*>(dst + c1 + 4 * g) =
                    make_float4(acc[1][t][0], acc[1][t][1], acc[1][t][2], acc[1][t][3]);
        }
    }
}

// ------------------------------------------------------------- 6. combine
// m = bf16(sum_j p[t, j] * y[t k + j]) in rank order, then add_rmsnorm_kernel
// (dmcp_kernels.hip) on m, operation for operation: h = m (+ residual),
// residual <- bf16(h), out = h * rsqrt(mean(h^2) + eps) * w.  w == nullptr:
// no norm (out <- m when there is no residual either).
template <int VPT>
__global__ __launch_bounds__(kBlock) void moe_combine_kernel(const float* __restrict__ y, const float* __restrict__ p,
                                                             uint16_t* __restrict__ residual,
                                                             const uint16_t* __restrict__ w,
                                                             uint16_t* __restrict__ out, int H, int topk, float eps) {
    const int row = blockIdx.x;
    const int nvec = H >> 3;
    uint4* rr = residual ? reinterpret_cast<uint4*>(residual + (size_t)row * H) : nullptr;
    const uint4* wr = reinterpret_cast<const uint4*>(w);
    const float* pr = p + (size_t)row * topk;
    const float* yr = y + (size_t)row * topk * H;
    float h[VPT][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        if (idx < nvec) {
            float m[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            for (int j = 0; j < topk; ++j) {
                const float pj = pr[j];
                const float4 lo = *reinterpret_cast<const float4*>(yr + (size_t)j * H + idx * 8);
                const float4 hi = *reinterpret_cast<const float4*>(yr + (size_t)j * H + idx * 8 + 4);
                m[0] = fmaf(pj, lo.x, m[0]); m[1] = fmaf(pj, lo.y, m[1]);
                m[2] = fmaf(pj, lo.z, m[2]); m[3] = fmaf(pj, lo.w, m[3]);
                m[4] = fmaf(pj, hi.x, m[4]); m[5] = fmaf(pj, hi.y, m[5]);
                m[6] = fmaf(pj, hi.z, m[6]); m[7] = fmaf(pj, hi.w, m[7]);
            }
            uint4 packed = pack8(m);
            unpack8(packed, h[i]);  // the MLP output as the bf16 row add_rmsnorm would be given
            if (rr) {
                float r[8];
                unpack8(rr[idx], r);
#pragma unroll
                for (int j = 0; j < 8; ++j) h[i][j] += r[j];
                packed = pack8(h[i]);
                rr[idx] = packed;
                unpack8(packed, h[i]);
            }
            if (!w && out) reinterpret_cast<uint4*>(out + (size_t)row * H)[idx] = packed;
#pragma unroll
            for (int j = 0; j < 8; ++j) ss += h[i][j] * h[i][j];
        }
    }
    if (!w) return;  // uniform: a kernel argument
    __shared__ float red[kBlock / kWave];
    ss = wave_sum(ss);
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = ss;
    __syncthreads();
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < kBlock / kWave; ++k) tot += red[k];
    const float inv = rsqrtf(tot / (float)H + eps);
    uint4* orow = reinterpret_cast<uint4*>(out + (size_t)row * H);
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
        const int idx = threadIdx.x + i * kBlock;
        if (idx < nvec) {
            float wf[8], o[8];
            unpack8(wr[idx], wf);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = h[i][j] * inv * wf[j];
            orow[idx] = pack8(o);
        }
    }
}

bool moe_shape_ok(int T, int H, int I, int E, int k, int MT) {
    return T > 0 && H > 0 && I > 0 && H % 64 == 0 && I % 64 == 0 && H <= 8192 && E >= 1 && E <= kMaxExperts &&
           k >= 1 && k <= E && (MT == 32 || MT == 128) && (long long)T * k < (1ll << 30);
}

// The sigmoid-routed block with S shared pseudo-experts: the same contract
// over E + S groups and k + S pairs per row; scale finite is the caller's.
bool moe_sh_shape_ok(int T, int H, int I, int E, int k, int S, int MT) {
    return E >= 1 && k >= 1 && k <= E && S >= 0 && S <= 64 && moe_shape_ok(T, H, I, E + S, k + S, MT);
}

template <int RT, typename WT>
void launch_gemms(const uint16_t* h, const WT* wgu, const float* sgu, const WT* wdown, const float* sdown,
                  const int32_t* perm, const int32_t* tiles, const int32_t* ntiles, uint16_t* act, float* y, int P,
                  int H, int I, int k, int max_tiles, hipStream_t st) {
    moe_gemm_kernel<RT, true, WT><<<dim3(I / 64, max_tiles), kBlock, 0, st>>>(h, wgu, sgu, perm, tiles, ntiles, act,
                                                                               nullptr, P, H, I, k);
    moe_gemm_kernel<RT, false, WT><<<dim3((H + 127) / 128, max_tiles), kBlock, 0, st>>>(
        act, wdown, sdown, perm, tiles, ntiles, nullptr, y, P, I, H, k);
}

// The six launches of dmcp_moe_mlp / dmcp_moe_mlp_w8 (WT: the expert weights'
// element; sgu / sdown: the e4m3 form's block scales, null for bf16).
//
// sig: the sigmoid router (moe_route_sig_kernel) with its selection bias,
// weight scale and S shared pseudo-experts; wgu / wdown then stack E + S
// experts, a row has k + S pairs, and every later stage runs over E + S groups
// and k + S pairs per row exactly as it does over E and k.
template <typename WT>
int moe_mlp_launch(const void* h, const void* wr, const void* wgu, const void* sgu, const void* wdown,
                   const void* sdown, void* ids, void* p, void* cnt, void* offs, void* perm, void* tiles, void* ntiles,
                   void* act, void* y, void* residual, const void* norm_w, void* out, int T, int H, int I, int E_r,
                   int k_r, int norm, int MT, float eps, void* stream, bool sig = false, const void* bias = nullptr,
                   float scale = 1.f, int S = 0) {
    if (sig ? !moe_sh_shape_ok(T, H, I, E_r, k_r, S, MT) || !bias : !moe_shape_ok(T, H, I, E_r, k_r, MT))
        return (int)hipErrorInvalidValue;
    if (!norm_w && !residual && !out) return (int)hipErrorInvalidValue;
    if (norm_w && !out) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int E = E_r + S, k = k_r + S;  // groups, pairs per row
    const int P = T * k;
    const int max_tiles = (P + MT - 1) / MT + E;
    if (max_tiles > 65535) return (int)hipErrorInvalidValue;  // grid.y
    const int wpb = kBlock / kWave;
    if (sig)
        moe_route_sig_kernel<<<(T + wpb - 1) / wpb, kBlock, 0, st>>>((const uint16_t*)h, (const uint16_t*)wr,
                                                                     (const float*)bias, (int32_t*)ids, (float*)p, T,
                                                                     H, E_r, k_r, S, norm, scale);
    else
        moe_route_kernel<<<(T + wpb - 1) / wpb, kBlock, 0, st>>>((const uint16_t*)h, (const uint16_t*)wr,
                                                                 (int32_t*)ids, (float*)p, T, H, E, k, norm);
    moe_count_kernel<<<E, kWave, 0, st>>>((const int32_t*)ids, (int32_t*)cnt, P);
    moe_scatter_kernel<<<E, kWave, 0, st>>>((const int32_t*)ids, (const int32_t*)cnt, (int32_t*)offs, (int32_t*)perm,
                                            (int32_t*)tiles, (int32_t*)ntiles, P, E, MT, max_tiles);
    if (MT == 32)
        launch_gemms<2, WT>((const uint16_t*)h, (const WT*)wgu, (const float*)sgu, (const WT*)wdown,
                            (const float*)sdown, (const int32_t*)perm, (const int32_t*)tiles, (const int32_t*)ntiles,
                            (uint16_t*)act, (float*)y, P, H, I, k, max_tiles, st);
    else
        launch_gemms<8, WT>((const uint16_t*)h, (const WT*)wgu, (const float*)sgu, (const WT*)wdown,
                            (const float*)sdown, (const int32_t*)perm, (const int32_t*)tiles, (const int32_t*)ntiles,
                            (uint16_t*)act, (float*)y, P, H, I, k, max_tiles, st);
    const int vpt = (H / 8 + kBlock - 1) / kBlock;
    const float* yy = (const float*)y;
    const float* pp = (const float*)p;
    uint16_t* rr = (uint16_t*)residual;
    const uint16_t* ww = (const uint16_t*)norm_w;
    uint16_t* oo = (uint16_t*)out;
    if (vpt == 1) moe_combine_kernel<1><<<T, kBlock, 0, st>>>(yy, pp, rr, ww, oo, H, k, eps);
    else if (vpt == 2) moe_combine_kernel<2><<<T, kBlock, 0, st>>>(yy, pp, rr, ww, oo, H, k, eps);
    else moe_combine_kernel<4><<<T, kBlock, 0, st>>>(yy, pp, rr, ww, oo, H, k, eps);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

// h [T, H] bf16, wr [E, H] bf16 -> ids int32 [T, k], p fp32 [T, k]
int dmcp_moe_route(const void* h, const void* wr, void* ids, void* p, int T, int H, int E, int k, int norm,
                   void* stream) {
    if (!moe_shape_ok(T, H, 64, E, k, 32)) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int wpb = kBlock / kWave;
    moe_route_kernel<<<(T + wpb - 1) / wpb, kBlock, 0, st>>>((const uint16_t*)h, (const uint16_t*)wr, (int32_t*)ids,
                                                             (float*)p, T, H, E, k, norm);
    return (int)hipGetLastError();
}

// The whole block.  Scratch (the caller's workspace): ids / p [T k], cnt [E],
// offs [E + 1], perm [T k], tiles [3 (ceil(T k / MT) + E)], ntiles [1],
// act bf16 [T k, I], y fp32 [T k, H].  residual / norm_w / out: the combine's
// add_rmsnorm contract (norm_w null: out <- m, or residual += m).
int dmcp_moe_mlp(const void* h, const void* wr, const void* wgu, const void* wdown, void* ids, void* p, void* cnt,
                 void* offs, void* perm, void* tiles, void* ntiles, void* act, void* y, void* residual,
                 const void* norm_w, void* out, int T, int H, int I, int E, int k, int norm, int MT, float eps,
                 void* stream) {
    return moe_mlp_launch<uint16_t>(h, wr, wgu, nullptr, wdown, nullptr, ids, p, cnt, offs, perm, tiles, ntiles, act,
                                    y, residual, norm_w, out, T, H, I, E, k, norm, MT, eps, stream);
}

// The same block over block-scaled FP8 expert weights: wgu8 [E, 2 I, H] and
// wdown8 [E, H, I] e4m3 bytes, sgu fp32 [E, 2 ceil(I / 128), ceil(H / 128)]
// (gate block rows, then up block rows) and sdown fp32 [E, ceil(H / 128),
// ceil(I / 128)]: W[n, k] = e4m3[n, k] * s[n / 128, k / 128].  The other
// arguments, the workspace parts and the refusals are dmcp_moe_mlp's.
int dmcp_moe_mlp_w8(const void* h, const void* wr, const void* wgu8, const void* sgu, const void* wdown8,
                    const void* sdown, void* ids, void* p, void* cnt, void* offs, void* perm, void* tiles,
                    void* ntiles, void* act, void* y, void* residual, const void* norm_w, void* out, int T, int H,
                    int I, int E, int k, int norm, int MT, float eps, void* stream) {
    if (!wgu8 || !sgu || !wdown8 || !sdown) return (int)hipErrorInvalidValue;
    return moe_mlp_launch<uint8_t>(h, wr, wgu8, sgu, wdown8, sdown, ids, p, cnt, offs, perm, tiles, ntiles, act, y,
                                   residual, norm_w, out, T, H, I, E, k, norm, MT, eps, stream);
}

// The sigmoid router alone (GLM-4.5; one expert group): bias fp32 [E] enters
// the selection only, the weights are the unbiased scores, renormalised over
// the k routed ones when norm, then times scale.  ids int32 / p fp32
// [T, k + S]: the last S pairs of a row are the shared pseudo-experts
// (E + s, 1.0).
int dmcp_moe_route_sig(const void* h, const void* wr, const void* bias, void* ids, void* p, int T, int H, int E, int k,
                       int S, int norm, float scale, void* stream) {
    if (!bias || !moe_sh_shape_ok(T, H, 64, E, k, S, 32) || !(scale > 0.f) || scale > 3.0e38f)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const int wpb = kBlock / kWave;
    moe_route_sig_kernel<<<(T + wpb - 1) / wpb, kBlock, 0, st>>>((const uint16_t*)h, (const uint16_t*)wr,
                                                                 (const float*)bias, (int32_t*)ids, (float*)p, T, H, E,
                                                                 k, S, norm, scale);
    return (int)hipGetLastError();
}

// dmcp_moe_mlp under the sigmoid router with S shared experts as
// pseudo-experts E .. E + S - 1: wgu [E + S, 2 I, H], wdown [E + S, H, I] (the
// shared MLP of width S I cut into S slices of width I), and every workspace
// part sized with k + S for k and E + S for E.  The combine adds the k routed
// ranks in rank order, then the S shared slices in order (weight 1).
int dmcp_moe_mlp_sh(const void* h, const void* wr, const void* bias, const void* wgu, const void* wdown, void* ids,
                    void* p, void* cnt, void* offs, void* perm, void* tiles, void* ntiles, void* act, void* y,
                    void* residual, const void* norm_w, void* out, int T, int H, int I, int E, int k, int S, int norm,
                    float scale, int MT, float eps, void* stream) {
    if (!(scale > 0.f) || scale > 3.0e38f) return (int)hipErrorInvalidValue;
    return moe_mlp_launch<uint16_t>(h, wr, wgu, nullptr, wdown, nullptr, ids, p, cnt, offs, perm, tiles, ntiles, act,
                                    y, residual, norm_w, out, T, H, I, E, k, norm, MT, eps, stream, true, bias, scale,
                                    S);
}

}  // extern "C"
