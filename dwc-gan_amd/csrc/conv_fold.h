// What surrounds the GEMM bodies of the im2col convolutions, written once for fp32 (conv_igemm.hip) and bf16 (conv_bf16.hip) tensors:
// the reflect-pad adjoint of a data gradient ("fold": whole image, band, ring strips), the split-K reduce and the weight re-layout.
// Templates only -- a translation unit compiles what it instantiates.  Elements are reached through ld4 / st4 (groups of 4) and
// ldv / stv (16 bytes: 4 fp32 / 8 bf16) of dwc_common.h: sums are fp32, a bf16 value is rounded once, at its store.
#pragma once
#include "conv_geom.h"

namespace {

// ---- reflect-pad adjoint ---------------------------------------------------------------------
// The coordinates of the padded axis (length n + 2*pad) that reflect padding copies from coordinate p of the un-padded axis: its own
// position first (callers whose destination already holds the interior skip index 0), then the mirror images about the first and the
// last element.  Returns how many (1..3).
__device__ __forceinline__ int reflect_src(int p, int n, int pad, int (&out)[3]) {
    int c = 0;
    out[c++] = p + pad;
    if (p >= 1 && p <= pad) out[c++] = pad - p;
    if (p >= n - 1 - pad && p <= n - 2) out[c++] = pad + 2 * (n - 1) - p;
    return c;
}

// reflect-pad adjoint: fold the padded gradient image back onto the un-padded one (groups of 4 channels)
template <typename T>
__global__ void fold_reflect_kernel(const T* __restrict__ gp, T* __restrict__ dx, int B, int H, int W, int C4, int pad,
                                    int Wp) {   // Wp: row pitch of gp in pixels (>= W + 2*pad)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * H * W * C4;
    if (idx >= total) return;
    const int c = idx % C4;
    size_t r = idx / C4;
    const int w = r % W;
    r /= W;
    const int h = r % H;
    const int n = r / H;
    const int Hp = H + 2 * pad;
    int hs[3], ws[3];
    const int nh = reflect_src(h, H, pad, hs), nw = reflect_src(w, W, pad, ws);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int a = 0; a < nh; ++a)
        for (int b = 0; b < nw; ++b) s += ld4(gp, ((size_t)(n * Hp + hs[a]) * Wp + ws[b]) * C4 + c);
    st4(dx, idx, s);
}

template <typename T>
int fold_reflect(const T* gp, T* dx, int B, int H, int W, int C4, int pad, int Wp, hipStream_t st) {
    const size_t total = (size_t)B * H * W * C4;
    hipLaunchKernelGGL(fold_reflect_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gp, dx, B, H, W, C4, pad, Wp);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

// zero-pad adjoint: the interior of the padded gradient image gp ([B][H+2pad][W+2pad][C]) copied to dx ([B][H][W][C]), groups of 4
// channels.  For the data gradients of zero-padded convolutions whose GEMM could not write the interior itself (split-K).
template <typename T>
__global__ void crop_image_kernel(const T* __restrict__ gp, T* __restrict__ dx, int B, int H, int W, int C4, int pad) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)B * H * W * C4;
    if (idx >= total) return;
    const int c = idx % C4;
    size_t r = idx / C4;
    const int w = r % W;
    r /= W;
    const int h = r % H;
    const size_t n = r / H;
    st4(dx, idx, ld4(gp, ((n * (H + 2 * pad) + h + pad) * (size_t)(W + 2 * pad) + w + pad) * C4 + c));
}

template <typename T>
int crop_image(const T* gp, T* dx, int B, int H, int W, int C4, int pad, hipStream_t st) {
    const size_t total = (size_t)B * H * W * C4;
    hipLaunchKernelGGL(crop_image_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, gp, dx, B, H, W, C4, pad);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

// dx (holds the interior of the padded gradient image already: Scatter::crop) += the border ring of gp folded back by the reflect
// rule; only the pixels a ring pixel folds onto are visited (rows 1..pad and H-1-pad..H-2 whole, columns 1..pad and W-1-pad..W-2
// of the other rows).  CV = C / VecOf<T>::V channel groups of 16 bytes.
template <typename T>
__global__ __launch_bounds__(256) void fold_band_kernel(const T* __restrict__ gp, T* __restrict__ dx, int B, int H, int W, int CV,
                                                        int pad, int Wp) {
    constexpr int V = VecOf<T>::V;
    // one thread per (image, band pixel, channel chunk): per image the 2*pad band rows whole (W pixels each), then the 2*pad band
    // columns of the H - 2*pad other rows
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int rows_done = 2 * pad, rest = H - 2 * pad;          // band rows, other rows
    const int band = rows_done * W + rest * 2 * pad;            // band pixels per image
    const size_t total = (size_t)B * band * CV;
    if (idx >= total) return;
    const int c = idx % CV;
    size_t r = idx / CV;
    const int q = r % band;
    const size_t n = r / band;
    const int Hp = H + 2 * pad;
    int h, w;
    if (q < rows_done * W) {
        const int br = q / W;
        w = q - br * W;
        h = br < pad ? 1 + br : H - 1 - pad + (br - pad);
    } else {
        const int q2 = q - rows_done * W;
        const int hr = q2 / (2 * pad), k = q2 - hr * 2 * pad;
        // the hr-th row that is NOT a band row: rows 0, pad+1 .. H-2-pad, H-1
        h = hr == 0 ? 0 : (hr == rest - 1 ? H - 1 : pad + hr);
        w = k < pad ? 1 + k : W - 1 - pad + (k - pad);
    }
    int hs[3], ws[3];
    const int nh = reflect_src(h, H, pad, hs), nw = reflect_src(w, W, pad, ws);
    if (nh * nw == 1) return;
    const size_t o = ((n * H + h) * (size_t)W + w) * CV + c;
    float s[V], v[V];
    ldv(dx, o, s);
    for (int a = 0; a < nh; ++a)
        for (int b = 0; b < nw; ++b) {
            if (a == 0 && b == 0) continue;               // the pixel's own (interior) value is in dx already
            ldv(gp, ((n * Hp + hs[a]) * (size_t)Wp + ws[b]) * CV + c, v);
#pragma unroll
            for (int k = 0; k < V; ++k) s[k] += v[k];
        }
    stv(dx, o, s);
}

// gp: [B][H+2pad][W+2pad][C], C a multiple of VecOf<T>::V, H and W >= 2*pad + 2 (the two bands of an axis must not overlap)
template <typename T>
int fold_band(const T* gp, T* dx, int B, int H, int W, int C, int pad, hipStream_t st) {
    const int CV = C / VecOf<T>::V;
    const size_t band_items = (size_t)B * (2 * pad * W + (H - 2 * pad) * 2 * pad) * CV;
    hipLaunchKernelGGL(fold_band_kernel<T>, dim3((unsigned)((band_items + 255) / 256)), dim3(256), 0, st, gp, dx, B, H, W, CV, pad,
                       W + 2 * pad);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

// dx += the border ring of the padded gradient image, folded back by the reflect rule.  dx already holds the interior;
// the ring (fp32 whatever T) lives in four strips: top/bottom [B][pad][Wp][C], left/right [B][H][pad][C], `parts` copies
// `part_stride` apart (partial sums over K, added in order).  Only the bands of dx that receive something are visited: per image
// 2*pad rows x W pixels (rows 1..pad, H-1-pad..H-2) then 2*pad columns x H pixels (skipping the rows already done).
template <typename T>
__global__ void fold_ring_kernel(T* __restrict__ dx, const float* __restrict__ ring, size_t off_bottom, size_t off_left,
                                 size_t off_right, int parts, size_t part_stride, int B, int H, int W, int C4, int pad) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int band = 2 * pad * (W + H);
    const size_t total = (size_t)B * band * C4;
    if (idx >= total) return;
    const int c = idx % C4;
    size_t r = idx / C4;
    const int q = r % band;
    const int n = r / band;
    int h, w;
    if (q < 2 * pad * W) {
        const int br = q / W;
        w = q - br * W;
        h = br < pad ? 1 + br : H - 1 - pad + (br - pad);
    } else {
        const int q2 = q - 2 * pad * W, bc = q2 / H;
        h = q2 - bc * H;
        w = bc < pad ? 1 + bc : W - 1 - pad + (bc - pad);
        if ((h >= 1 && h <= pad) || (h >= H - 1 - pad && h <= H - 2)) return;   // covered by the row bands
    }
    if (h < 0 || h >= H || w < 0 || w >= W) return;
    const int Wp = W + 2 * pad;
    int hs[3], ws[3];
    const int nh = reflect_src(h, H, pad, hs), nw = reflect_src(w, W, pad, ws);
    const size_t o = ((size_t)(n * H + h) * W + w) * C4 + c;
    f32x4 s = ld4(dx, o);
    for (int a = 0; a < nh; ++a)
        for (int b = 0; b < nw; ++b) {
            if (a == 0 && b == 0) continue;
            const int rh = hs[a], rw = ws[b];
            size_t e;   // element offset inside one part's ring
            if (rh < pad) e = ((size_t)(n * pad + rh) * Wp + rw) * C4;
            else if (rh >= pad + H) e = off_bottom / 4 + ((size_t)(n * pad + rh - pad - H) * Wp + rw) * C4;
            else if (rw < pad) e = off_left / 4 + ((size_t)(n * H + rh - pad) * pad + rw) * C4;
            else e = off_right / 4 + ((size_t)(n * H + rh - pad) * pad + rw - pad - W) * C4;
            for (int p = 0; p < parts; ++p) s += ld4(ring + p * part_stride, e + c);
        }
    st4(dx, o, s);
}

// the ring as same_dgrad_geom laid it out (strips in the order top, bottom, left, right)
template <typename T>
int fold_ring(T* dx, const float* ring, const SameDgrad& f, int B, int H, int W, int C, int pad, hipStream_t st) {
    const size_t total = (size_t)B * 2 * pad * (W + H) * (C / 4);
    hipLaunchKernelGGL(fold_ring_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, dx, ring, f.ring_elems[0],
                       f.ring_elems[0] + f.ring_elems[1], f.ring_elems[0] + f.ring_elems[1] + f.ring_elems[2], f.parts, f.ring_total,
                       B, H, W, C / 4, pad);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

// ---- split-K reduce --------------------------------------------------------------------------
// dst[i] = act(sum_s part[s][i] + bias[i % N]), fixed summation order
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ part, T* __restrict__ dst,
                                                            const float* __restrict__ bias, size_t total4, size_t stride4, int splits,
                                                            int N, int act) {
    const int nq = N >> 2;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total4; i += (size_t)gridDim.x * blockDim.x) {
        f32x4 s = ld4(part, i);
        for (int z = 1; z < splits; ++z) s += ld4(part, (size_t)z * stride4 + i);
        const int c4 = i % nq;
        if (bias) s += ld4(bias, c4);
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = dwc_act_apply(s[k], act, c4 * 4 + k);
        st4(dst, i, s);
    }
}

// part: `splits` images of dst_elems fp32 values, one after the other
template <typename T>
int splitk_reduce(const float* part, T* dst, const float* bias, size_t dst_elems, int splits, int N, int act, hipStream_t st) {
    const size_t total4 = dst_elems / 4;
    size_t blocks = (total4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, st, part, dst, bias, total4, total4, splits, N, act);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

// ---- weight re-layout ------------------------------------------------------------------------
// Weight layouts streamed by the im2col GEMM kernels: one row per GEMM column n, K contiguous and zero-padded to a multiple of
// the K-slab depth `bk` (32 fp32 / 64 bf16 elements) ("[N][Kp]"), so the B tile is staged exactly like the A tile.  Source: the
// fp32 OIHW master weights; T: the element type of the prepared matrix.
//   forward : row = co, k = (kh*KW + kw)*cin_pad + ci                      value W[co][ci][kh][kw]
//   dgrad s1: row = ci, k = (kh'*KW + kw')*cout_pad + co                   value W[co][ci][KH-1-kh'][KW-1-kw']
//   dgrad s2: [class ph*2+pw] row = ci, k = (th*2 + tw)*cout_pad + co      value W[co][ci][ph+2th][pw+2tw]  (4x4 kernel)
template <typename T>
__global__ void weight_prepare_fwd_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin, int KHW,
                                          int cout_pad, int cin_pad, int Kp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)cout_pad * Kp) return;
    const int k = idx % Kp, co = idx / Kp;
    const int ci = k % cin_pad, tap = k / cin_pad;
    float v = 0.f;
    if (co < Cout && ci < Cin && tap < KHW) v = w[((size_t)co * Cin + ci) * KHW + tap];
    out[idx] = (T)v;
}

template <typename T>
__global__ void weight_prepare_dgrad_kernel(const float* __restrict__ w, T* __restrict__ out, int Cout, int Cin, int KH, int KW,
                                            int stride, int cout_pad, int cin_pad, int Kp) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per_class = (size_t)cin_pad * Kp;
    const int classes = stride == 1 ? 1 : 4;
    if (idx >= per_class * classes) return;
    const int cls = idx / per_class;
    const size_t r = idx % per_class;
    const int k = r % Kp, ci = r / Kp;
    const int co = k % cout_pad, tapo = k / cout_pad;
    int kh, kw;
    bool ok = co < Cout && ci < Cin;
    if (stride == 1) {
        ok = ok && tapo < KH * KW;
        kh = KH - 1 - tapo / KW;
        kw = KW - 1 - tapo % KW;
    } else {
        ok = ok && tapo < 4;
        kh = (cls >> 1) + 2 * (tapo >> 1);
        kw = (cls & 1) + 2 * (tapo & 1);
    }
    out[idx] = (T)(ok ? w[((size_t)co * Cin + ci) * KH * KW + kh * KW + kw] : 0.f);
}

// row length of a prepared matrix: `taps` filter taps of c_pad channels, rounded up to whole K-slabs
inline int weight_prepared_kp(int taps, int c_pad, int bk) { return (taps * c_pad + bk - 1) / bk * bk; }

inline size_t weight_prepared_elems(int KH, int KW, int stride, int cout_pad, int cin_pad, int for_dgrad, int bk) {
    if (!for_dgrad) return (size_t)cout_pad * weight_prepared_kp(KH * KW, cin_pad, bk);
    if (stride == 1) return (size_t)cin_pad * weight_prepared_kp(KH * KW, cout_pad, bk);
    return (size_t)4 * cin_pad * weight_prepared_kp(4, cout_pad, bk);
}

template <typename T>
int weight_prepare_fwd(const float* w, T* out, int Cout, int Cin, int KH, int KW, int cout_pad, int cin_pad, int bk, hipStream_t st) {
    const int Kp = weight_prepared_kp(KH * KW, cin_pad, bk);
    const size_t total = (size_t)cout_pad * Kp;
    hipLaunchKernelGGL(weight_prepare_fwd_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, out, Cout, Cin, KH * KW,
                       cout_pad, cin_pad, Kp);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

// stride 1, or stride 2 with a 4x4 filter (four parity classes)
template <typename T>
int weight_prepare_dgrad(const float* w, T* out, int Cout, int Cin, int KH, int KW, int stride, int cout_pad, int cin_pad, int bk,
                         hipStream_t st) {
    const int Kp = weight_prepared_kp(stride == 1 ? KH * KW : 4, cout_pad, bk);
    const size_t total = (size_t)(stride == 1 ? 1 : 4) * cin_pad * Kp;
    hipLaunchKernelGGL(weight_prepare_dgrad_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, w, out, Cout, Cin, KH, KW,
                       stride, cout_pad, cin_pad, Kp);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

}  // namespace
