// Implicit-GEMM convolution on the fp32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32).
//
// Replaces nn.ReflectionPad2d + nn.Conv2d (+bias, +activation) and their autograd
// (reference networks.py:579-585) — the padded copy is never materialised: the reflect
// (or, for the data gradient, zero) boundary rule is applied to the gather index while the
// input tile is staged into LDS.
//
// GEMM view (forward):  Y[m][n] = sum_k A[m][k] * Wt[k][n]
//     m = (image, oh, ow) output pixel          M = B*Ho*Wo
//     n = output channel                        N = Cout
//     k = (kh, kw, ci), ci fastest              K = KH*KW*Cin     (NHWC makes ci contiguous)
// The data gradient is the same kernel with another index rule (see dwc_conv2d_bwd_data);
// the weight gradient contracts over m instead (conv_wgrad_kernel).
//
// Tiling: 256 threads = 4 waves, block tile BM x BN x 32(K); each wave owns TMxTN 32x32
// accumulator tiles (16 VGPRs each).  Operands are staged global -> LDS directly (16-byte
// vectors along the channel axis) into a double-buffered LDS tile: the next K-slab's loads are
// issued before the MFMAs of the current one and there is ONE barrier per slab.
// Tile shape is picked per problem so that every CU holds >= 2 workgroups whenever the grid
// allows it (one wave per SIMD cannot hide its own LDS/barrier latency), and products with few
// output tiles but a long K (the discriminator tails, M = B*16 rows) are split along K into
// partial images that a small epilogue kernel sums (+bias, +activation) in a fixed order.
#include <type_traits>

#include <atomic>

#include "conv_im2col_entry.h"

namespace {

constexpr int BK = 32;


// ------------------------------------------------------------------------------------------
// Forward / data-gradient GEMM.  Staging is DIRECT global->LDS (global_load_lds_dwordx4): no
// staging registers, no ds_write pass.  A wave instruction deposits 64 x 16 B contiguously, i.e.
// 8 rows x 128 B of an UNPADDED [row][32] tile; bank conflicts of the ds_read_b128 fragment reads
// are avoided by an XOR swizzle of the 16-byte chunk index with ((row >> 1) & 7), applied on the
// SOURCE address (which K-chunk a lane fetches) and again on the read.  Out-of-bounds taps of the
// zero-padded data gradient fetch from a zero page.  (Measured against the register-staged
// variant this replaced, r01: 5x5 256->128 @64^2 113 -> 130 TFLOP/s, 3x3 256->256 @32^2 94 -> 98.)
// ------------------------------------------------------------------------------------------
__device__ __attribute__((aligned(16))) float g_zero_page[64];

#ifdef DWC_CLOCK_PROBE   // development builds only (make PROBE=1): average shader clock seen by the GEMM kernels
__device__ unsigned long long g_clock_probe[2];
struct ClockProbe {
    long long c0, r0;
    __device__ ClockProbe() : c0(clock64()), r0(wall_clock64()) {}
    __device__ ~ClockProbe() {
        if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
            atomicAdd(&g_clock_probe[0], (unsigned long long)(clock64() - c0));
            atomicAdd(&g_clock_probe[1], (unsigned long long)(wall_clock64() - r0));
        }
    }
};
#define DWC_PROBE() ClockProbe clock_probe_
#else
#define DWC_PROBE()
#endif

// Workgroup barrier that also retires this wave's outstanding direct-to-LDS loads.  hipcc's
// __syncthreads() already drains vmcnt when an LDS-DMA is in flight (checked in the ISA: every
// s_barrier is preceded by s_waitcnt vmcnt(0) lgkmcnt(0)); the explicit wait makes the kernels
// independent of that compiler behaviour.
__device__ __forceinline__ void lds_dma_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// One output tile (or, when part_stride != 0, its contribution from K-slabs [kt0, kt1_in)).  `bid`/`nb`: this
// workgroup's linear tile index and the number of tiles of the launch; (oph, opw): parity class of a stride-2 gradient.
// X3 (r04): the SAME kernel -- staging, geometry, prepared fp32 weights, epilogue -- with the inner product taken as exact
// three-way bf16 split products on the bf16 matrix cores (conv_halo_x3.hip explains the arithmetic: a = a0 + a1 + a2 with 8
// significand bits each, six of the nine partial products, the rest below one fp32 rounding; leading product and corrections
// in separate accumulators).  The fp32 fragments are read from the unchanged LDS image and split in registers in front of the
// MFMAs: ~44 vector-ALU instructions per 32x16 fragment, which two workgroups per CU hide behind each other's 48 bf16 MFMAs
// per slab.  For the layers the halo form cannot take (small discriminator layers, 7x7 image layers, ring strips, 1x1).
typedef __bf16 gx3_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned gx3_u32x4 __attribute__((ext_vector_type(4)));

// 8 fp32 (two 16-byte chunks of a row) -> three bf16x8 planes, exact: v = p0 + p1 + p2 (truncate, subtract, truncate, subtract)
__device__ __forceinline__ void gx3_split8(const f32x4& a, const f32x4& b, gx3_bf16x8& p0, gx3_bf16x8& p1, gx3_bf16x8& p2) {
    unsigned h[8], m[8], l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float v = k < 4 ? a[k] : b[k - 4];
        const unsigned hb = __float_as_uint(v) & 0xffff0000u;
        const float r = v - __uint_as_float(hb);
        const unsigned mb = __float_as_uint(r) & 0xffff0000u;
        const float q = r - __uint_as_float(mb);
        h[k] = hb; m[k] = mb; l[k] = __float_as_uint(q);
    }
    gx3_u32x4 u0, u1, u2;
#pragma unroll
    for (int k = 0; k < 4; ++k) {                      // bytes 2,3 of the even element below bytes 2,3 of the odd one
        u0[k] = __builtin_amdgcn_perm(h[2 * k + 1], h[2 * k], 0x07060302u);
        u1[k] = __builtin_amdgcn_perm(m[2 * k + 1], m[2 * k], 0x07060302u);
        u2[k] = __builtin_amdgcn_perm(l[2 * k + 1], l[2 * k], 0x07060302u);
    }
    p0 = __builtin_bit_cast(gx3_bf16x8, u0);
    p1 = __builtin_bit_cast(gx3_bf16x8, u1);
    p2 = __builtin_bit_cast(gx3_bf16x8, u2);
}

template <int BM, int BN, int WM, int WN, int TM, int TN, bool X3 = false>
__device__ __forceinline__ void conv_gemm_body(const Gather& g, const float* __restrict__ wmat, const Scatter& o,
                                               const float* __restrict__ bias, int act, int tiles_n, int kt0, int kt1_in,
                                               size_t part_offset, bool partial, int oph, int opw, int bid, int nb) {
    static_assert(WM * WN == 4 && WM * TM * 32 == BM && WN * TN * 32 == BN, "tile shape");
    constexpr int A_PASSES = BM / 32, B_PASSES = BN / 32;
    constexpr int A_TILE = BM * BK, B_TILE = BN * BK;
    __shared__ __attribute__((aligned(16))) float smem[2 * (A_TILE + B_TILE)];
    float* sA = smem;
    float* sB = smem + 2 * A_TILE;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, hi = lane >> 5;

    if (nb >= 16) {     // XCD-aware remap: the 32 CUs of one XCD walk neighbouring tiles
        const int q = nb >> 3, r = nb & 7, x = bid & 7, y = bid >> 3;
        bid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + y;
    }
    const int tile_m = bid / tiles_n, tile_n = bid % tiles_n;
    const int m0 = tile_m * BM, n0 = tile_n * BN;

    const int arow = t >> 3;                              // tile row this lane stages (+32 per pass)
    const int acol = (((t & 7) ^ ((arow >> 1) & 7))) * 4;  // LOGICAL k offset fetched into physical chunk t&7
    int a_bh[A_PASSES], a_bw[A_PASSES], a_img[A_PASSES];
    const int ohw = g.OH * g.OW;
#pragma unroll
    for (int i = 0; i < A_PASSES; ++i) {
        const int mm = min(m0 + arow + 32 * i, g.M - 1);
        const int n = mm / ohw;
        const int rem = mm - n * ohw;
        const int oh = rem / g.OW, ow = rem - oh * g.OW;
        a_bh[i] = oh * g.mul_h + g.off_h;
        a_bw[i] = ow * g.mul_w + g.off_w;
        a_img[i] = n * g.SH * g.SW;
    }
    const int Kp = (g.K + BK - 1) / BK * BK;
    const float* b_ptr[B_PASSES];
#pragma unroll
    for (int p = 0; p < B_PASSES; ++p) b_ptr[p] = wmat + (size_t)min(n0 + arow + 32 * p, o.N - 1) * Kp + acol;

    const int nk_all = Kp / BK;
    const int kt1 = min(nk_all, kt1_in);
    const int n_taps = g.KH * g.KW;

    int cur_tap = -1;
    const float* a_src[A_PASSES];     // per-row source of the current tap (zero page when out of bounds)
    const bool tap_uniform = g.SC >= BK;
    auto row_sources = [&](int tap, int ci) {
        int kh = (tap * g.kw_magic) >> 16;
        int kw = tap - kh * g.KW;
        if (g.tap_t) {          // square filters only: the same decode gives (kw, kh)
            const int x = kh;
            kh = kw;
            kw = x;
        }
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            int h = a_bh[i] + kh * g.kstep;
            int w = a_bw[i] + kw * g.kstep;
            bool inb = true;
            if (g.reflect) {
                h = reflect_idx(h, g.SH);
                w = reflect_idx(w, g.SW);
            } else {
                inb = h >= 0 && h < g.SH && w >= 0 && w < g.SW;
                h = min(max(h, 0), g.SH - 1);
                w = min(max(w, 0), g.SW - 1);
            }
            const float* p = (const float*)g.src + ((a_img[i] + h * g.SW + w) << g.logSC) + ci;
            a_src[i] = inb ? p : g_zero_page;   // (no channel offset is ever added to the zero page, see stage_slab)
        }
    };
    // issue the direct loads of slab kt into LDS buffer `buf`
    auto stage_slab = [&](int kt, int buf) {
        int coff;   // channel offset added to a_src (0 when the source is the zero page)
        if (tap_uniform) {
            const int kg0 = kt * BK;
            const int tap = min(kg0 >> g.logSC, n_taps - 1);
            if (tap != cur_tap) {
                row_sources(tap, acol);
                cur_tap = tap;
            }
            coff = kg0 & (g.SC - 1);
        } else {
            const int kg = kt * BK + acol;
            row_sources(min(kg >> g.logSC, n_taps - 1), kg & (g.SC - 1));
            coff = 0;
        }
        float* la = sA + buf * A_TILE + wave * (8 * BK);
        float* lb = sB + buf * B_TILE + wave * (8 * BK);
#pragma unroll
        for (int i = 0; i < A_PASSES; ++i) {
            const float* s = a_src[i];
            if (s != g_zero_page) s += coff;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)s,
                                             (__attribute__((address_space(3))) void*)(la + i * 32 * BK), 16, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < B_PASSES; ++p)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(b_ptr[p] + kt * BK),
                                             (__attribute__((address_space(3))) void*)(lb + p * 32 * BK), 16, 0, 0);
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // fragment reads: logical chunk 2q+hi of row r sits in physical chunk (2q+hi) ^ ((r>>1)&7)
    const int fsw = (l31 >> 1) & 7;
    int frag_off[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) frag_off[q] = ((2 * q + hi) ^ fsw) * 4;
    const int a_row = (wm * TM * 32 + l31) * BK;
    const int b_row = (wn * TN * 32 + l31) * BK;
    f32x4 fa[2][TM], fb[2][TN];
    auto load_frags = [&](int set, int buf, int q) {
        const float* a = sA + buf * A_TILE + a_row + frag_off[q];
        const float* b = sB + buf * B_TILE + b_row + frag_off[q];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[set][i] = *reinterpret_cast<const f32x4*>(a + i * 32 * BK);
#pragma unroll
        for (int n = 0; n < TN; ++n) fb[set][n] = *reinterpret_cast<const f32x4*>(b + n * 32 * BK);
    };
    auto mfma_group = [&](int set) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int n = 0; n < TN; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][i][j], fb[set][n][j], acc[i][n], 0, 0, 0);
    };

    if constexpr (X3) {
        static_assert(TM * TN <= 2, "split accumulators: at most two 32x32 tiles per wave");
        f32x16 lo[TM][TN];                               // the five correction products, merged once at the end
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) lo[i][j][r] = 0.f;
        // k-step s (16 deep) of a slab: lane half hi takes k = 16 s + 8 hi .. + 7 = logical chunks 4 s + 2 hi, + 1 of its row
        int xoff[2][2];
#pragma unroll
        for (int ss = 0; ss < 2; ++ss)
#pragma unroll
            for (int e = 0; e < 2; ++e) xoff[ss][e] = ((4 * ss + 2 * hi + e) ^ fsw) * 4;
        gx3_bf16x8 pa[3][TM], pb[3][TN];
        auto frags_x3 = [&](int buf, int ss) {
            const float* a = sA + buf * A_TILE + a_row;
            const float* b = sB + buf * B_TILE + b_row;
#pragma unroll
            for (int i = 0; i < TM; ++i)
                gx3_split8(*reinterpret_cast<const f32x4*>(a + i * 32 * BK + xoff[ss][0]),
                           *reinterpret_cast<const f32x4*>(a + i * 32 * BK + xoff[ss][1]), pa[0][i], pa[1][i], pa[2][i]);
#pragma unroll
            for (int n = 0; n < TN; ++n)
                gx3_split8(*reinterpret_cast<const f32x4*>(b + n * 32 * BK + xoff[ss][0]),
                           *reinterpret_cast<const f32x4*>(b + n * 32 * BK + xoff[ss][1]), pb[0][n], pb[1][n], pb[2][n]);
        };
        auto mfma_x3 = [&]() {
            constexpr int TA[6] = {0, 1, 0, 2, 1, 0}, TB[6] = {0, 0, 1, 0, 1, 2};
#pragma unroll
            for (int term = 0; term < 6; ++term)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int n = 0; n < TN; ++n) {
                        if (term == 0) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[TA[term]][i], pb[TB[term]][n], acc[i][n], 0, 0, 0);
                        else lo[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[TA[term]][i], pb[TB[term]][n], lo[i][n], 0, 0, 0);
                    }
        };
        if (kt0 < kt1) {
            stage_slab(kt0, 0);
            lds_dma_barrier();
            int buf = 0;
            for (int kt = kt0; kt < kt1; ++kt) {
                if (kt + 1 < kt1) stage_slab(kt + 1, buf ^ 1);   // other buffer: fully read before the last barrier
                frags_x3(buf, 0);
                mfma_x3();
                frags_x3(buf, 1);
                lds_dma_barrier();                            // direct loads landed (vmcnt), this buffer fully read
                mfma_x3();
                buf ^= 1;
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += lo[i][j][r];
    } else if (kt0 < kt1) {
        stage_slab(kt0, 0);
        lds_dma_barrier();
        int buf = 0;
        load_frags(0, 0, 0);
        for (int kt = kt0; kt < kt1; ++kt) {
            const bool more = kt + 1 < kt1;
            if (more) stage_slab(kt + 1, buf ^ 1);       // other buffer: fully read before the last barrier
            load_frags(1, buf, 1);
            mfma_group(0);
            load_frags(0, buf, 2);
            mfma_group(1);
            load_frags(1, buf, 3);
            mfma_group(0);
            lds_dma_barrier();                            // direct loads landed (vmcnt), this buffer fully read
            if (more) load_frags(0, buf ^ 1, 0);
            mfma_group(1);
            buf ^= 1;
        }
    }

    float* dst = (float*)o.dst + part_offset;
    const float slope = dwc_act_slope(act);
    // bias of this lane's TN columns, loaded ONCE in one batch (r04: inside the per-element conditionals of the store loop the
    // compiler can neither hoist nor batch the load -- TM*16*TN dependent round trips per lane)
    float bcol[TN];
#pragma unroll
    for (int n = 0; n < TN; ++n) bcol[n] = 0.f;
    if (bias && !partial) {
#pragma unroll
        for (int n = 0; n < TN; ++n) bcol[n] = bias[min(n0 + (wn * TN + n) * 32 + l31, o.N - 1)];
    }
    // two loop nests (dwc_common.h, dwc_act_simple): the transcendental activations stay out of the common path's code
    auto store = [&](auto general) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                const int m = m0 + row;
                if (m >= g.M) continue;
                const int n_img = m / ohw;
                const int rem = m - n_img * ohw;
                const int oh = rem / g.OW, ow = rem - oh * g.OW;
                const int py = oh * o.os + oph, px = ow * o.os + opw;
                float* drow = dst + (((size_t)n_img * o.OHf + py) * o.OWf + px) * o.N;
                if (o.crop && !partial) {                 // Scatter::crop: interior pixels of a padded gradient image go straight to dx
                    const int yy = py - o.crop, xx = px - o.crop;
                    if ((unsigned)yy < (unsigned)o.IH && (unsigned)xx < (unsigned)o.IW)
                        drow = (float*)o.inner + (((size_t)n_img * o.IH + yy) * o.IW + xx) * o.N;
                }
#pragma unroll
                for (int n = 0; n < TN; ++n) {
                    const int col = n0 + (wn * TN + n) * 32 + l31;
                    if (col < o.N) {
                        float v = acc[i][n][r];
                        if (!partial) {
                            v += bcol[n];
                            if constexpr (decltype(general)::value) v = dwc_act_apply(v, act, col);
                            else v = dwc_act_simple(v, slope);
                        }
                        drow[col] = v;
                    }
                }
            }
        }
    };
    if (dwc_act_is_simple(act)) store(std::false_type{});
    else store(std::true_type{});
}

template <int BM, int BN, int WM, int WN, int TM, int TN, bool X3 = false>
__global__ __launch_bounds__(256) void conv_gemm_kernel(Gather g, const float* __restrict__ wmat, size_t w_class_stride,
                                                             Scatter o, const float* __restrict__ bias, int act, int tiles_n,
                                                             int kt_per_split, size_t part_stride) {
    DWC_PROBE();
    const int cls = blockIdx.z, split = blockIdx.y;
    conv_gemm_body<BM, BN, WM, WN, TM, TN, X3>(g, wmat + (size_t)cls * w_class_stride, o, bias, act, tiles_n, split * kt_per_split,
                                           (split + 1) * kt_per_split, (size_t)split * part_stride, part_stride != 0, cls >> 1,
                                           cls & 1, blockIdx.x, gridDim.x);
}

template <int BM, int BN, int WM, int WN, int TM, int TN, bool X3 = false>
__global__ __launch_bounds__(256) void conv_gemm_strips_kernel(StripSet ss) {
    const Strip& s = ss.s[blockIdx.z];
    if ((int)blockIdx.x >= s.tiles) return;
    const int kt0 = s.kt0 + blockIdx.y * ss.kt_per_part;
    conv_gemm_body<BM, BN, WM, WN, TM, TN, X3>(s.g, (const float*)s.w, s.o, nullptr, DWC_ACT_NONE, s.tiles_n, kt0, min(s.kt1, kt0 + ss.kt_per_part),
                                           blockIdx.y * ss.part_stride, false, s.oph, s.opw, blockIdx.x, s.tiles);
}

// ------------------------------------------------------------------------------------------
// weight gradient: dW[k][n] = sum_m A[m][k] * dY[m][n], split over m ("split-K") into slabs
// ------------------------------------------------------------------------------------------
// X3: the contraction over pixels as exact bf16 split products (see conv_gemm_body): both operands are read from the unchanged
// fp32 LDS tiles -- eight pixels of one k / n column per lane and 16-deep step, the same ds_read_b32 count as the fp32 MFMA path --
// and split in registers.
// ZP: the zero rule (weight gradient of a zero-padded convolution): an A^T row whose gathered pixel lies outside the image comes
// from the zero page, as in conv_gemm_body.  A compile-time rule: the reflect instantiations are the instructions they were.
template <int BN, int WM, int WN, int TM, int TN, bool X3 = false, bool ZP = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(Gather g, const float* __restrict__ dy, int N, float* __restrict__ slab,
                                                         int m_chunk, int splits_per_class = 0, size_t src_class_stride = 0,
                                                         size_t dy_class_stride = 0) {
    static_assert(WM * WN == 4 && WM * TM * 32 == 128 && WN * TN * 32 == BN, "tile shape");
    DWC_PROBE();
    constexpr int A_TILE = 32 * 128, B_TILE = 32 * BN;
    __shared__ __attribute__((aligned(16))) float smem[2 * (A_TILE + B_TILE)];
    float* sA = smem;               // [buf][m][k]
    float* sB = smem + 2 * A_TILE;  // [buf][m][n]
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, hi = lane >> 5;
    const int k0 = blockIdx.x * 128, n0 = blockIdx.y * BN;
    int split = blockIdx.z;
    if (splits_per_class > 0) {       // batched form (Winograd): blockIdx.z = class * splits_per_class + split
        const int cls = blockIdx.z / splits_per_class;
        split = blockIdx.z - cls * splits_per_class;
        g.src = (const float*)g.src + (size_t)cls * src_class_stride;
        dy += (size_t)cls * dy_class_stride;
    }
    const int m_begin = split * m_chunk;
    const int m_end = min(g.M, m_begin + m_chunk);

    // A^T tile: thread owns one 4-wide k group (fixed tap / channel) and rows (t>>5)+8i.
    // k >= K (tile tail) is clamped to a valid tap: those output rows are never stored.
    const int kg = k0 + (t & 31) * 4;
    const int tap = min(kg >> g.logSC, g.KH * g.KW - 1);
    const int ci = kg & (g.SC - 1);
    const int kh = (tap * g.kw_magic) >> 16;
    const int kw = tap - kh * g.KW;
    const int dh = kh * g.kstep + g.off_h, dw = kw * g.kstep + g.off_w;
    const int arow = t >> 5;
    constexpr int B_F4 = BN / 4;
    constexpr int B_ROWS_PER_PASS = 256 / B_F4;
    constexpr int B_PASSES = 32 / B_ROWS_PER_PASS;
    const int brow = t / B_F4, bcol = (t % B_F4) * 4;
    const int ohw = g.OH * g.OW;

    const int bcol_c = min(n0 + bcol, N - 4);    // columns past N are never stored: clamp instead of masking
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    // Direct global->LDS staging (global_load_lds_dwordx4): lane t deposits its 16 bytes at float
    // offset 4*t of the pass, which IS [row][k] / [row][n] order for these unpadded tiles (the MFMA
    // operands are read along the lanes, so no swizzle is needed).  Rows past the end of this
    // m-chunk must contribute nothing: their dY operand comes from the zero page, the gathered x
    // operand may then be anything finite (row index clamped).
    auto stage_slab = [&](int mb, int buf) {
        float* la = sA + buf * A_TILE + wave_u * 256;
        float* lb = sB + buf * B_TILE + wave_u * 256;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int m = min(mb + arow + 8 * i, g.M - 1);
            int n, oh, ow;
            if (g.logOW >= 0) {                   // power-of-two pixel grid: shifts instead of divisions
                n = m >> g.logOHW;
                const int rem = m & (ohw - 1);
                oh = rem >> g.logOW;
                ow = rem & (g.OW - 1);
            } else {
                n = m / ohw;
                const int rem = m - n * ohw;
                oh = rem / g.OW;
                ow = rem - oh * g.OW;
            }
            const float* s;
            if constexpr (ZP) {
                const int h = oh * g.mul_h + dh, w = ow * g.mul_w + dw;
                const bool inb = (unsigned)h < (unsigned)g.SH && (unsigned)w < (unsigned)g.SW;
                const int hc = min(max(h, 0), g.SH - 1), wc = min(max(w, 0), g.SW - 1);
                s = inb ? (const float*)g.src + (((n * g.SH + hc) * g.SW + wc) << g.logSC) + ci : g_zero_page;
            } else {
                const int h = reflect_idx(oh * g.mul_h + dh, g.SH);
                const int w = reflect_idx(ow * g.mul_w + dw, g.SW);
                s = (const float*)g.src + (((n * g.SH + h) * g.SW + w) << g.logSC) + ci;
            }
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)s,
                                             (__attribute__((address_space(3))) void*)(la + i * 8 * 128), 16, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < B_PASSES; ++p) {
            const int m = mb + brow + p * B_ROWS_PER_PASS;
            const float* s = m < m_end ? dy + (size_t)m * N + bcol_c : g_zero_page;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)s,
                                             (__attribute__((address_space(3))) void*)(lb + p * B_ROWS_PER_PASS * BN), 16, 0, 0);
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // Same skewed pipeline as conv_gemm_kernel: a slab is four groups of four MFMA steps; the
    // operands of group g+1 are fetched from LDS while group g is multiplied, the registers->LDS
    // store of the next slab sits between groups 1 and 2, and group 3 (fetched before the barrier)
    // is multiplied after it while the next slab's group 0 is being fetched.
    float av[2][4][TM], bv[2][4][TN];
    auto load_ops = [&](int set, int buf, int grp) {
        const float* a = sA + buf * A_TILE + (wm * TM) * 32 + l31;
        const float* b = sB + buf * B_TILE + (wn * TN) * 32 + l31;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int ml = 2 * (4 * grp + s) + hi;
#pragma unroll
            for (int i = 0; i < TM; ++i) av[set][s][i] = a[ml * 128 + i * 32];
#pragma unroll
            for (int n = 0; n < TN; ++n) bv[set][s][n] = b[ml * BN + n * 32];
        }
    };
    auto mfma_ops = [&](int set) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int n = 0; n < TN; ++n)
                    acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[set][s][i], bv[set][s][n], acc[i][n], 0, 0, 0);
    };
    if constexpr (X3) {
        f32x16 lo[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) lo[i][j][r] = 0.f;
        gx3_bf16x8 pa[3][TM], pb[3][TN];
        auto ops_x3 = [&](int buf, int ss) {              // 16-pixel step ss of the slab: lane half hi takes pixels 16 ss + 8 hi .. + 7
            const float* a = sA + buf * A_TILE + (wm * TM) * 32 + l31 + (16 * ss + 8 * hi) * 128;
            const float* b = sB + buf * B_TILE + (wn * TN) * 32 + l31 + (16 * ss + 8 * hi) * BN;
#pragma unroll
            for (int i = 0; i < TM; ++i)
                gx3_split8(f32x4{a[i * 32], a[128 + i * 32], a[2 * 128 + i * 32], a[3 * 128 + i * 32]},
                           f32x4{a[4 * 128 + i * 32], a[5 * 128 + i * 32], a[6 * 128 + i * 32], a[7 * 128 + i * 32]}, pa[0][i], pa[1][i],
                           pa[2][i]);
#pragma unroll
            for (int n = 0; n < TN; ++n)
                gx3_split8(f32x4{b[n * 32], b[BN + n * 32], b[2 * BN + n * 32], b[3 * BN + n * 32]},
                           f32x4{b[4 * BN + n * 32], b[5 * BN + n * 32], b[6 * BN + n * 32], b[7 * BN + n * 32]}, pb[0][n], pb[1][n],
                           pb[2][n]);
        };
        auto mfma_x3 = [&]() {
            constexpr int TA[6] = {0, 1, 0, 2, 1, 0}, TB[6] = {0, 0, 1, 0, 1, 2};
#pragma unroll
            for (int term = 0; term < 6; ++term)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int n = 0; n < TN; ++n) {
                        if (term == 0) acc[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[TA[term]][i], pb[TB[term]][n], acc[i][n], 0, 0, 0);
                        else lo[i][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa[TA[term]][i], pb[TB[term]][n], lo[i][n], 0, 0, 0);
                    }
        };
        if (m_begin < m_end) {
            stage_slab(m_begin, 0);
            lds_dma_barrier();
            int buf = 0;
            for (int mb = m_begin; mb < m_end; mb += 32) {
                if (mb + 32 < m_end) stage_slab(mb + 32, buf ^ 1);
                ops_x3(buf, 0);
                mfma_x3();
                ops_x3(buf, 1);
                lds_dma_barrier();
                mfma_x3();
                buf ^= 1;
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += lo[i][j][r];
    } else if (m_begin < m_end) {
        stage_slab(m_begin, 0);
        lds_dma_barrier();
        int buf = 0;
        load_ops(0, 0, 0);
        for (int mb = m_begin; mb < m_end; mb += 32) {
            const bool more = mb + 32 < m_end;
            if (more) stage_slab(mb + 32, buf ^ 1);      // other buffer: fully read before the last barrier
            load_ops(1, buf, 1);
            mfma_ops(0);
            load_ops(0, buf, 2);
            mfma_ops(1);
            load_ops(1, buf, 3);
            mfma_ops(0);
            lds_dma_barrier();
            if (more) load_ops(0, buf ^ 1, 0);
            mfma_ops(1);
            buf ^= 1;
        }
    }
    float* out = slab + (size_t)blockIdx.z * g.K * N;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            if (k >= g.K) continue;
#pragma unroll
            for (int n = 0; n < TN; ++n) {
                const int col = n0 + (wn * TN + n) * 32 + l31;
                if (col < N) out[(size_t)k * N + col] = acc[i][n][r];
            }
        }
}


template <int BM, int BN, int WM, int WN, int TM, int TN, bool X3 = false>
void launch_variant(const Gather& g, const float* w, size_t wcs, int classes, const Scatter& o, const float* bias, int act,
                    const Plan& p, size_t part_stride, hipStream_t st) {
    const int tiles_m = (g.M + BM - 1) / BM, tiles_n = (o.N + BN - 1) / BN;
    hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, WM, WN, TM, TN, X3>), dim3(tiles_m * tiles_n, p.splits, classes), dim3(256), 0, st,
                       g, w, wcs, o, bias, act, tiles_n, p.kt_per_split, part_stride);
}

// 1: the im2col GEMM takes its inner product as split products on the bf16 matrix cores (conv_gemm_body<..., X3>): default for every
// product with K >= 128 (below that the launch is latency, not arithmetic).  DWC_X3_GEMM=0: the native fp32 MFMA everywhere.
// Process-wide switch of the split-product inner products: bit 0 the forward / data-gradient GEMM, bit 1 the weight-gradient
// kernel.  Initialised from DWC_X3_GEMM / DWC_X3_WGRAD (default on); dwc_x3_gemm_mode() reads / sets it at run time (tests use it
// to obtain the native fp32 MFMA result as a yardstick).
static std::atomic<int> g_x3_mode{-1};
static int x3_mode() {
    int m = g_x3_mode.load(std::memory_order_relaxed);
    if (m < 0) {
        const int a = getenv("DWC_X3_GEMM") ? atoi(getenv("DWC_X3_GEMM")) : 1;
        const int b = getenv("DWC_X3_WGRAD") ? atoi(getenv("DWC_X3_WGRAD")) : 1;
        m = (a ? 1 : 0) | (b ? 2 : 0);
        g_x3_mode.store(m, std::memory_order_relaxed);
    }
    return m;
}
static bool wgrad_x3_on() { return (x3_mode() & 2) != 0; }
static bool gemm_x3_on(int K) { return (x3_mode() & 1) != 0 && K >= 128; }

// What the shared entry layer (conv_im2col_entry.h) needs to know about the fp32 kernels.
struct Im2colF32 {
    typedef float T;
    static constexpr int BK = ::BK;
    static constexpr int MIN_LOG_C = 2;             // a 16-byte staging chunk is 4 channels
    static constexpr int CH_MASK = 3;
    static constexpr bool ZERO_BY_OFFSET = false;   // out-of-image rows come from g_zero_page
    static constexpr bool HALF_STRIPS = false;      // only the 64-row strip tile exists (strip_bm)
    static constexpr int WGRAD_SLAB_ROWS = 32;
    static constexpr int IMAGE_PX = 8;              // NHWC4 images: 8 pixels x 4 planes per GEMM row
    static constexpr int IMAGE_GROUPS = 1;          // groups of 4 planes the fold behind it handles: 32 / (4 * IMAGE_PX)
    // (f relative to 128x128 at 2 WG/CU: r01 kernel_bench, 130 / 108 / ~95 TFLOP/s)
    static constexpr TileCand TILES[] = {{128, 128, 2, 1.0f}, {128, 64, 3, 0.85f}, {64, 64, 5, 0.72f}, {128, 32, 4, 0.5f}};
    // (r05: the threshold was NUM_CU / 2 -- 128 tiles of a 4096-deep contraction ran 128 slabs each, one barrier per slab: c1's
    // discriminator tail launches 32.9 -> 28.5 us with up to 2 * NUM_CU tiles split, +28 reduce launches; net -0.2 ms per step)
    static constexpr int SPLIT_BELOW = 2 * NUM_CU;

    static int launch_gemm(const Gather& g, const float* w, size_t w_class_stride, int classes, Scatter o, const float* bias, int act,
                           size_t dst_elems, void* ws, size_t ws_bytes, hipStream_t st) {
        Plan p = im2col_plan<Im2colF32>(g.M, o.N, g.K, classes);
        float* final_dst = (float*)o.dst;
        size_t part_stride = 0;
        if (p.splits > 1) {
            if (!ws || ws_bytes < gemm_ws_bytes(p, dst_elems)) {
                p.splits = 1;   // not enough scratch: run un-split (slower, same result up to summation order)
                p.kt_per_split = (g.K + BK - 1) / BK;
            } else {
                o.dst = (float*)ws;
                part_stride = dst_elems;
            }
        }
        if (gemm_x3_on(g.K)) {
            // (split accumulators need the registers of two tiles: the 128x128 plan runs as 128x64 with twice the column tiles)
            if (p.bm == 128 && p.bn >= 64) launch_variant<128, 64, 2, 2, 2, 1, true>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
            else if (p.bm == 64 && p.bn == 64) launch_variant<64, 64, 2, 2, 1, 1, true>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
            else launch_variant<128, 32, 4, 1, 1, 1, true>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
        } else if (p.bm == 128 && p.bn == 128) launch_variant<128, 128, 2, 2, 2, 2>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
        else if (p.bm == 128 && p.bn == 64) launch_variant<128, 64, 2, 2, 2, 1>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
        else if (p.bm == 64 && p.bn == 64) launch_variant<64, 64, 2, 2, 1, 1>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
        else launch_variant<128, 32, 4, 1, 1, 1>(g, w, w_class_stride, classes, o, bias, act, p, part_stride, st);
        DWC_LAUNCH_CHECK();
        if (p.splits > 1) return splitk_reduce((const float*)ws, final_dst, bias, dst_elems, p.splits, o.N, act, st);
        return DWC_OK;
    }

    // The ring strips of a data gradient (same_dgrad_geom / s2_ring_geom).  Only the 64-row tile exists here, and every
    // destination is fp32: `f32out` makes no difference.
    static int launch_strips(const StripSet& ss, int bm, dim3 grid, hipStream_t st, bool /*f32out*/) {
        if (bm != 64) return DWC_EINVAL;
        if (gemm_x3_on(ss.s[0].g.K)) hipLaunchKernelGGL((conv_gemm_strips_kernel<64, 64, 2, 2, 1, 1, true>), grid, dim3(256), 0, st, ss);
        else hipLaunchKernelGGL((conv_gemm_strips_kernel<64, 64, 2, 2, 1, 1>), grid, dim3(256), 0, st, ss);
        DWC_LAUNCH_CHECK();
        return DWC_OK;
    }

    template <bool X3, bool ZP>
    static void wgrad_kernels(const Gather& g, const float* dy, int Cout, float* slab, int splits, int chunk, hipStream_t st) {
        const int tk = (g.K + 127) / 128, bn = wgrad_bn(Cout);
        if (bn == 128)
            hipLaunchKernelGGL((conv_wgrad_kernel<128, 2, 2, 2, 2, X3, ZP>), dim3(tk, (Cout + 127) / 128, splits), dim3(256), 0, st, g, dy,
                               Cout, slab, chunk);
        else if (bn == 64)
            hipLaunchKernelGGL((conv_wgrad_kernel<64, 2, 2, 2, 1, X3, ZP>), dim3(tk, 1, splits), dim3(256), 0, st, g, dy, Cout, slab, chunk);
        else
            hipLaunchKernelGGL((conv_wgrad_kernel<32, 4, 1, 1, 1, X3, ZP>), dim3(tk, 1, splits), dim3(256), 0, st, g, dy, Cout, slab, chunk);
    }

    static int wgrad_launch(const FwdGeom& f, const float* dy, float* dw_oihw, int Cin, int Cout, int KHW, int cin_real, int cout_real,
                            void* ws, size_t ws_bytes, hipStream_t st) {
        const Gather& g = f.g;
        int splits, chunk;
        if (!ws || ws_bytes < wgrad_ws_bytes(g.M, g.K, Cout, WGRAD_SLAB_ROWS, &splits, &chunk)) return DWC_EWORKSPACE;
        float* slab = (float*)ws;
        // (Gather::reflect == 0: the zero-rule instantiations, conv2d_bwd_weight_zeropad)
        if (wgrad_x3_on()) g.reflect ? wgrad_kernels<true, false>(g, dy, Cout, slab, splits, chunk, st) : wgrad_kernels<true, true>(g, dy, Cout, slab, splits, chunk, st);
        else g.reflect ? wgrad_kernels<false, false>(g, dy, Cout, slab, splits, chunk, st) : wgrad_kernels<false, true>(g, dy, Cout, slab, splits, chunk, st);
        DWC_LAUNCH_CHECK();
        wgrad_reduce(slab, dw_oihw, splits, g.K, Cout, Cin, KHW, cin_real, cout_real, st);
        DWC_LAUNCH_CHECK();
        return DWC_OK;
    }

    static int fold_image(const float* dxp, float* dx, int B, int H, int W, int C, int pad, hipStream_t st) {
        return fold_reflect(dxp, dx, B, H, W, C / 4, pad, W + 2 * pad, st);
    }

    // dwc_reflect_pad_adjoint_band: NULL tensors and C <= 0 are rejected here and not by the bf16 twin; the bf16 twin's limits
    // H, B <= 65535 are not applied here.
    static bool band_args_bad(const void* dxp, const void* dx, int /*B*/, int /*H*/, int C) { return !dxp || !dx || C <= 0; }
};

}  // namespace

#define DWC_F32_NAME(x) dwc_##x
DWC_IM2COL_EXPORTS(DWC_F32_NAME, Im2colF32, float)
#undef DWC_F32_NAME

extern "C" {

int dwc_version(void) { return DWC_ABI_VERSION; }

/* mode >= 0: set the split-product switch of the im2col kernels (bit 0: forward / data-gradient GEMM, bit 1: weight gradient;
 * 0 = native fp32 MFMA everywhere); returns the previous value.  mode < 0: query only. */
int dwc_x3_gemm_mode(int mode) {
    const int prev = x3_mode();
    if (mode >= 0) g_x3_mode.store(mode & 3, std::memory_order_relaxed);
    return prev;
}

/* dwc_reflect_pad_adjoint for a padded gradient image whose rows are `pitch` >= W + 2*pad pixels apart (the 8-pixel-group grid of
 * dwc_x3_conv2d_narrow's image gradient). */
int dwc_reflect_pad_adjoint_pitch(const float* dxp, float* dx, int B, int H, int W, int C, int pad, int pitch, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || pad < 0 || pad >= H || pad >= W || pitch < W + 2 * pad) return DWC_EINVAL;
    return fold_reflect(dxp, dx, B, H, W, C / 4, pad, pitch, (hipStream_t)stream);
}

}  // extern "C"

#ifdef DWC_CLOCK_PROBE
extern "C" int dwc_debug_clock_probe(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_clock_probe), 16) != hipSuccess) return DWC_ELAUNCH;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_clock_probe), z, 16) != hipSuccess) return DWC_ELAUNCH;
    }
    return 0;
}
#endif
