// The entry layer of the im2col convolutions, written once for fp32 (conv_igemm.hip, policy Im2colF32) and bf16 (conv_bf16.hip,
// policy Im2colBF16): argument checks, geometry, scratch sizes and the order of launches of every exported function the two files
// share.  Templates only, resolved statically; a translation unit defines its policy P and stamps its exports with
// DWC_IM2COL_EXPORTS.  Activations, prepared weights and their gradients are P::T tensors and cross this layer as void pointers,
// as the geometry builders of conv_geom.h take them.  A policy names what differs between the precisions:
//   T                  element type (float / bf16)
//   BK                 K-slab depth in elements (32 / 64: 128 bytes)
//   MIN_LOG_C          log2 of the channels a 16-byte staging chunk covers (2 / 3), for the geometry builders
//   CH_MASK            produced channel counts are multiples of CH_MASK + 1 (3 / 7)
//                      (in fp32 this is no restriction of its own: every `& CH_MASK` check below repeats what conv_args_ok, bwd_geom,
//                      zeropad_dgrad_geom and fwd_geom_ex already reject with `& 3`, so the fp32 return codes are those of the geometry
//                      builders alone; only bf16's 7 rejects anything they accept)
//   ZERO_BY_OFFSET     the zero rule of the weight-gradient / crop entries is an offset past a 2 GiB buffer descriptor (false / true):
//                      those entries then refuse larger gathered tensors
//   HALF_STRIPS        the `half` flag of strip_bm: the 128-row strip tile exists (false / true)
//   WGRAD_SLAB_ROWS    pixels per slab of the weight-gradient kernel (32 / 64)
//   IMAGE_PX           pixels per GEMM row of image_dgrad_geom (8 x 4 planes / 4 x 8 planes)
//   IMAGE_GROUPS       groups of 4 planes of the fold behind it (1 / 2)
//   TILES, SPLIT_BELOW candidate table and split-K threshold of plan_gemm
//   launch_gemm, launch_strips(ss, bm, grid, st, f32out), wgrad_launch      the launchers of the precision's kernels
//   fold_image         the whole-image reflect-pad adjoint
//   band_args_bad      the argument checks of reflect_pad_adjoint_band in which the precisions differ
// Return codes are the same for both precisions unless a policy member says otherwise.  Three checks do NOT follow CH_MASK, in either
// precision: reflect_pad_adjoint accepts any multiple of 4 channels; of the *_ws_bytes functions only bwd_data_zeropad_ws_bytes and
// bwd_data_crop_ws_bytes apply CH_MASK (the others answer for every count their geometry builder takes, multiples of 4); and zeropad_dgrad_geom /
// same_dgrad_geom take no min_log_c (the bf16 entry points rely on CH_MASK there).
#pragma once
#include "conv_fold.h"

namespace {

template <class P>
Plan im2col_plan(int M, int N, int K, int classes) {
    return plan_gemm(M, N, K, classes, P::BK, P::TILES, P::SPLIT_BELOW);
}

// ---- prepared weights ------------------------------------------------------------------------
template <class P>
size_t im2col_weight_prepared_elems(int Cout, int Cin, int KH, int KW, int stride, int cout_pad, int cin_pad, int for_dgrad) {
    return weight_prepared_elems(KH, KW, stride, cout_pad, cin_pad, for_dgrad, P::BK);
}

template <class P>
int im2col_weight_prepare_fwd(const float* w, void* out, int Cout, int Cin, int KH, int KW, int cout_pad, int cin_pad, void* stream) {
    if (cout_pad < Cout || cin_pad < Cin) return DWC_EINVAL;
    return weight_prepare_fwd(w, (typename P::T*)out, Cout, Cin, KH, KW, cout_pad, cin_pad, P::BK, (hipStream_t)stream);
}

template <class P>
int im2col_weight_prepare_dgrad(const float* w, void* out, int Cout, int Cin, int KH, int KW, int stride, int cout_pad, int cin_pad,
                                void* stream) {
    if (cout_pad < Cout || cin_pad < Cin) return DWC_EINVAL;
    if (stride == 2 && !(KH == 4 && KW == 4)) return DWC_EINVAL;
    if (stride != 1 && stride != 2) return DWC_EINVAL;
    return weight_prepare_dgrad(w, (typename P::T*)out, Cout, Cin, KH, KW, stride, cout_pad, cin_pad, P::BK, (hipStream_t)stream);
}

// ---- forward ---------------------------------------------------------------------------------
template <class P>
size_t im2col_fwd_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    FwdGeom f;
    if (!fwd_geom(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::MIN_LOG_C)) return 0;
    return gemm_ws_bytes(im2col_plan<P>(f.g.M, Cout, f.g.K, 1), f.dst_elems);
}

// The Plan im2col_fwd hands to launch_gemm for this shape, out = {bm, bn, splits, kt_per_split}: the same checks, the same fwd_geom and
// the same im2col_plan call, nothing launched.  (launch_gemm runs that plan as it stands, except that a split plan without its scratch
// runs unsplit and that the fp32 split-product form runs a 128x128 plan on the 128x64 kernel.)  For tests: they assert the branch they
// claim to cover instead of carrying a copy of the planner.
template <class P>
int im2col_fwd_plan(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* out) {
    FwdGeom f;
    if (!out || (Cout & P::CH_MASK) || !fwd_geom(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::MIN_LOG_C))
        return DWC_EINVAL;
    const Plan p = im2col_plan<P>(f.g.M, f.o.N, f.g.K, 1);
    out[0] = p.bm; out[1] = p.bn; out[2] = p.splits; out[3] = p.kt_per_split;
    return DWC_OK;
}

// reflect != 0: reflect pad + convolution (+ bias, + activation).  reflect == 0, the zero-padded convolutions (the frozen VGG16 of
// the perceptual loss, reference networks.py:639-688: nn.Conv2d(padding=1)): the same kernel with the zero rule.
template <class P>
int im2col_fwd(const void* x, const void* w_prepared, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int KH,
               int KW, int stride, int pad, int act, void* ws, size_t ws_bytes, void* stream, int reflect) {
    FwdGeom f;
    if ((Cout & P::CH_MASK) || !fwd_geom(x, y, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::MIN_LOG_C)) return DWC_EINVAL;
    f.g.reflect = reflect;
    return P::launch_gemm(f.g, (const typename P::T*)w_prepared, 0, 1, f.o, bias, act, f.dst_elems, ws, ws_bytes, (hipStream_t)stream);
}

// forward with per-axis stride and reflect pad (no scratch: never split)
template <class P>
int im2col_fwd_ex(const void* x, const void* w_prepared, const float* bias, void* y, int B, int H, int W, int Cin, int Cout, int KH,
                  int KW, int stride_h, int stride_w, int pad_h, int pad_w, int act, void* stream) {
    FwdGeom f;
    if ((Cout & P::CH_MASK) || !fwd_geom_ex(x, y, B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w, &f, P::MIN_LOG_C))
        return DWC_EINVAL;
    return P::launch_gemm(f.g, (const typename P::T*)w_prepared, 0, 1, f.o, bias, act, f.dst_elems, nullptr, 0, (hipStream_t)stream);
}

// ---- data gradient ---------------------------------------------------------------------------
// of a zero-padded stride-1 convolution: the zero-padded correlation with the flipped filter on the H x W grid (the adjoint of zero
// padding is a crop: nothing to fold)
template <class P>
size_t im2col_bwd_data_zeropad_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int pad) {
    FwdGeom f;
    if ((Cin & P::CH_MASK) || (Cout & P::CH_MASK) || !zeropad_dgrad_geom(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, pad, &f)) return 0;
    return gemm_ws_bytes(im2col_plan<P>(f.g.M, Cin, f.g.K, 1), f.dst_elems);
}

template <class P>
int im2col_bwd_data_zeropad(const void* dy, const void* w_dgrad, void* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                            int pad, void* ws, size_t ws_bytes, void* stream) {
    FwdGeom f;
    if ((Cin & P::CH_MASK) || (Cout & P::CH_MASK) || !zeropad_dgrad_geom(dy, dx, B, H, W, Cin, Cout, KH, KW, pad, &f)) return DWC_EINVAL;
    return P::launch_gemm(f.g, (const typename P::T*)w_dgrad, 0, 1, f.o, nullptr, DWC_ACT_NONE, f.dst_elems, ws, ws_bytes,
                          (hipStream_t)stream);
}

// step 1 of the two-step form: the gradient of the reflect-PADDED image
template <class P>
size_t im2col_bwd_data_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    BwdGeom f;
    if (!bwd_geom(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::BK, P::MIN_LOG_C)) return 0;
    return gemm_ws_bytes(im2col_plan<P>(f.g.M, Cin, f.g.K, f.classes), f.dst_elems);
}

template <class P>
int im2col_bwd_data(const void* dy, const void* w_dgrad, void* dxp, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                    int pad, void* ws, size_t ws_bytes, void* stream) {
    BwdGeom f;
    if ((Cin & P::CH_MASK) || !bwd_geom(dy, dxp, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::BK, P::MIN_LOG_C)) return DWC_EINVAL;
    return P::launch_gemm(f.g, (const typename P::T*)w_dgrad, f.wcs, f.classes, f.o, nullptr, DWC_ACT_NONE, f.dst_elems, ws, ws_bytes,
                          (hipStream_t)stream);
}

// step 2: the reflect-pad adjoint, dxp [B][H+2pad][W+2pad][C] folded onto dx [B][H][W][C]
template <class P>
int im2col_reflect_pad_adjoint(const void* dxp, void* dx, int B, int H, int W, int C, int pad, void* stream) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || pad < 0 || pad >= H || pad >= W) return DWC_EINVAL;
    return P::fold_image((const typename P::T*)dxp, (typename P::T*)dx, B, H, W, C, pad, (hipStream_t)stream);
}

// dx (already holding the interior of the padded gradient image dxp) += the border ring of dxp folded back by the reflect rule; only
// the band of dx a ring pixel folds onto is visited.  The second half of bwd_data_fold, for producers with their own epilogue.
template <class P>
int im2col_reflect_pad_adjoint_band(const void* dxp, void* dx, int B, int H, int W, int C, int pad, void* stream) {
    if (P::band_args_bad(dxp, dx, B, H, C) || B <= 0 || (C & P::CH_MASK) || pad <= 0 || H < 2 * pad + 2 || W < 2 * pad + 2)
        return DWC_EINVAL;
    return fold_band((const typename P::T*)dxp, (typename P::T*)dx, B, H, W, C, pad, (hipStream_t)stream);
}

// bwd_data + reflect_pad_adjoint as one call: dx ([B,H,W,Cin]) = reflect-pad adjoint of the gradient of the padded image.  Where the
// GEMM runs unsplit the interior of that image is written straight into dx (Scatter::crop) and only its border ring into dxp (scratch
// for [B,H+2pad,W+2pad,Cin]), a band kernel then folds the ring onto dx: one pass over the tensor instead of three.  Otherwise
// (split-K) the two-step form runs.
template <class P>
int im2col_bwd_data_fold(const void* dy, const void* w_dgrad, void* dxp, void* dx, int B, int H, int W, int Cin, int Cout, int KH,
                         int KW, int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
    BwdGeom f;
    if ((Cin & P::CH_MASK) || pad <= 0 || !bwd_geom(dy, dxp, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::BK, P::MIN_LOG_C))
        return DWC_EINVAL;
    if (H < 2 * pad + 2 || W < 2 * pad + 2 || H > 65535 - 2 * pad || B > 65535) return DWC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool direct = im2col_plan<P>(f.g.M, f.o.N, f.g.K, f.classes).splits == 1;
    if (direct) {
        f.o.crop = pad; f.o.IH = H; f.o.IW = W; f.o.inner = dx;
    }
    const int rc = P::launch_gemm(f.g, (const typename P::T*)w_dgrad, f.wcs, f.classes, f.o, nullptr, DWC_ACT_NONE, f.dst_elems, ws,
                                  ws_bytes, st);
    if (rc != DWC_OK) return rc;
    if (!direct) return im2col_reflect_pad_adjoint<P>(dxp, dx, B, H, W, Cin, pad, stream);
    return fold_band((const typename P::T*)dxp, (typename P::T*)dx, B, H, W, Cin, pad, st);
}

// Data gradient of a ZERO-padded convolution at any stride and pad bwd_geom takes: the adjoint of zero padding is a crop, so the
// interior of the gradient of the padded image IS dx.  One scratch arena, ws = [padded gradient image, rounded up to 256 bytes]
// [split-K partials].  Where the GEMM runs unsplit Scatter::crop writes the interior straight into dx (the border ring lands in the
// scratch image and is dropped: the `direct` branch of bwd_data_fold without the band fold); a split plan reduces into the scratch
// image and a copy crops it.  pad == 0: no scratch image, the GEMM writes dx.
template <class P>
size_t im2col_bwd_data_crop_image_bytes(int B, int H, int W, int Cin, int pad) {
    if (pad == 0) return 0;
    return ((size_t)B * (H + 2 * pad) * (W + 2 * pad) * Cin * sizeof(typename P::T) + 255) / 256 * 256;
}

template <class P>
size_t im2col_bwd_data_crop_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    BwdGeom f;
    if ((Cin & P::CH_MASK) || !bwd_geom(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::BK, P::MIN_LOG_C)) return 0;
    return im2col_bwd_data_crop_image_bytes<P>(B, H, W, Cin, pad) +
           gemm_ws_bytes(im2col_plan<P>(f.g.M, Cin, f.g.K, f.classes), f.dst_elems);
}

template <class P>
int im2col_bwd_data_crop(const void* dy, const void* w_dgrad, void* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                         int stride, int pad, void* ws, size_t ws_bytes, void* stream) {
    BwdGeom f;
    if (!dy || !w_dgrad || !dx || (Cin & P::CH_MASK) ||
        !bwd_geom(dy, dx, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::BK, P::MIN_LOG_C))
        return DWC_EINVAL;
    // (the zero rule of the bf16 gather is an offset past the descriptor, conv_bf16.hip OOB; the fp32 gather reads the zero page)
    if (P::ZERO_BY_OFFSET && (size_t)B * f.g.SH * f.g.SW * Cout * sizeof(typename P::T) >= 0x80000000ull) return DWC_EINVAL;
    const size_t image_bytes = im2col_bwd_data_crop_image_bytes<P>(B, H, W, Cin, pad);
    const Plan plan = im2col_plan<P>(f.g.M, f.o.N, f.g.K, f.classes);
    const size_t part_bytes = gemm_ws_bytes(plan, f.dst_elems);
    if (image_bytes + part_bytes && (!ws || ws_bytes < image_bytes + part_bytes)) return DWC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const bool direct = plan.splits == 1;
    if (pad > 0) {
        f.o.dst = ws;
        if (direct) {
            f.o.crop = pad; f.o.IH = H; f.o.IW = W; f.o.inner = dx;
        }
    }
    const int rc = P::launch_gemm(f.g, (const typename P::T*)w_dgrad, f.wcs, f.classes, f.o, nullptr, DWC_ACT_NONE, f.dst_elems,
                                  part_bytes ? (char*)ws + image_bytes : nullptr, part_bytes, st);
    if (rc != DWC_OK || pad == 0 || direct) return rc;
    return crop_image((const typename P::T*)ws, (typename P::T*)dx, B, H, W, Cin / 4, pad, st);
}

// Data gradient of a stride-1 "same" convolution in one call (same_dgrad_geom): the interior on the H x W grid straight into dx, the
// border ring as four strips of fp32 partials at the head of ws, folded onto dx.
template <class P>
size_t im2col_bwd_data_same_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int pad) {
    SameDgrad f;
    if (!same_dgrad_geom(nullptr, nullptr, nullptr, nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, pad, &f, P::BK, P::HALF_STRIPS)) return 0;
    const size_t ring = (f.ring_total * f.parts * sizeof(float) + 255) / 256 * 256;
    return ring + gemm_ws_bytes(im2col_plan<P>(f.g.M, Cin, f.g.K, 1), f.dst_elems);
}

// ring_only: dx must already hold the interior (a halo-tiled kernel with the zero rule and the dgrad weights wrote it)
template <class P>
int im2col_bwd_data_same(const void* dy, const void* w_dgrad, const void* w_dgrad_t, void* dx, int B, int H, int W, int Cin, int Cout,
                         int KH, int KW, int pad, void* ws, size_t ws_bytes, void* stream, bool ring_only) {
    SameDgrad f;
    if ((Cin & P::CH_MASK) ||
        !same_dgrad_geom(dy, w_dgrad, w_dgrad_t, dx, (float*)ws, B, H, W, Cin, Cout, KH, KW, pad, &f, P::BK, P::HALF_STRIPS))
        return DWC_EINVAL;
    const size_t ring_bytes = (f.ring_total * f.parts * sizeof(float) + 255) / 256 * 256;
    if (!ws || ws_bytes < ring_bytes) return DWC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (!ring_only) {
        const int rc = P::launch_gemm(f.g, (const typename P::T*)w_dgrad, 0, 1, f.o, nullptr, DWC_ACT_NONE, f.dst_elems,
                                      (char*)ws + ring_bytes, ws_bytes - ring_bytes, st);
        if (rc != DWC_OK) return rc;
    }
    const int rc = P::launch_strips(f.ss, f.bm, dim3(f.max_tiles, f.parts, 4), st, true);
    if (rc != DWC_OK) return rc;
    return fold_ring((typename P::T*)dx, (const float*)ws, f, B, H, W, Cin, pad, st);
}

// Border ring + fold of the data gradient of a 4x4 stride-2 reflect-pad-1 convolution whose INTERIOR (the H x W pixels of dx) has
// been written by a halo-tiled kernel: the ring of the padded gradient image is computed as eight thin whole-K strips into the scratch
// image dxp ([B][H+2][W+2][Cin], only its ring is touched) and folded onto dx by the band kernel.  w_dgrad: the stride-2
// data-gradient layout of weight_prepare_dgrad.
template <class P>
int im2col_bwd_data_s2_ring(const void* dy, const void* w_dgrad, void* dxp, void* dx, int B, int H, int W, int Cin, int Cout,
                            void* stream) {
    S2Ring f;
    if (!dy || !w_dgrad || !dxp || !dx || (Cin & P::CH_MASK) || H > 65535 - 2 || B > 65535 ||
        !s2_ring_geom(dy, w_dgrad, dxp, sizeof(typename P::T), B, H, W, Cin, Cout, &f, P::BK, P::MIN_LOG_C, P::HALF_STRIPS))
        return DWC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int rc = P::launch_strips(f.ss, f.bm, dim3(f.max_tiles, 1, 8), st, false);
    if (rc != DWC_OK) return rc;
    return fold_band((const typename P::T*)dxp, (typename P::T*)dx, B, H, W, Cin, 1, st);
}

// Gradient w.r.t. an IMAGE of 32 / IMAGE_PX planes through a stem convolution (image_dgrad_geom): the padded gradient image is built
// in ws and folded onto dx.
template <class P>
size_t im2col_bwd_data_image_ws_bytes(int B, int H, int W, int Cout, int KH, int KW, int pad) {
    FwdGeom f;
    if (!image_dgrad_geom(nullptr, nullptr, B, H, W, Cout, KH, KW, pad, &f, P::IMAGE_PX)) return 0;
    return f.dst_elems * sizeof(typename P::T);
}

template <class P>
int im2col_bwd_data_image(const void* dy, const void* w_wide, void* dx, int B, int H, int W, int Cout, int KH, int KW, int pad, void* ws,
                          size_t ws_bytes, void* stream) {
    FwdGeom f;
    if (!image_dgrad_geom(dy, ws, B, H, W, Cout, KH, KW, pad, &f, P::IMAGE_PX)) return DWC_EINVAL;
    if (!ws || ws_bytes < f.dst_elems * sizeof(typename P::T)) return DWC_EWORKSPACE;
    const int rc = P::launch_gemm(f.g, (const typename P::T*)w_wide, 0, 1, f.o, nullptr, DWC_ACT_NONE, f.dst_elems, nullptr, 0,
                                  (hipStream_t)stream);
    if (rc != DWC_OK) return rc;
    return fold_reflect((const typename P::T*)ws, (typename P::T*)dx, B, H, W, P::IMAGE_GROUPS, pad, f.g.OW * P::IMAGE_PX,
                        (hipStream_t)stream);
}

// ---- weight gradient -------------------------------------------------------------------------
template <class P>
size_t im2col_bwd_weight_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {
    const int Ho = (H + 2 * pad - KH) / stride + 1, Wo = (W + 2 * pad - KW) / stride + 1;
    int splits, chunk;
    return wgrad_ws_bytes(B * Ho * Wo, KH * KW * Cin, Cout, P::WGRAD_SLAB_ROWS, &splits, &chunk);
}

// reflect == 0: the weight gradient of a zero-padded convolution -- the same kernel, A^T rows outside the image read as zeros
// (wgrad_launch picks the zero-rule instantiation by Gather::reflect).  Same plan, same scratch.
template <class P>
int im2col_bwd_weight(const void* x, const void* dy, float* dw_oihw, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,
                      int pad, int cin_real, int cout_real, void* ws, size_t ws_bytes, void* stream, int reflect = 1) {
    FwdGeom f;
    if (!fwd_geom(x, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::MIN_LOG_C)) return DWC_EINVAL;
    if (cin_real > Cin || cout_real > Cout || (Cout & P::CH_MASK)) return DWC_EINVAL;
    if (!reflect) {
        // (the zero rule of the bf16 gather is an offset past the descriptor, conv_bf16.hip OOB; the fp32 gather reads the zero page)
        if (!x || !dy || !dw_oihw) return DWC_EINVAL;
        if (P::ZERO_BY_OFFSET && (size_t)B * H * W * Cin * sizeof(typename P::T) >= 0x80000000ull) return DWC_EINVAL;
        f.g.reflect = 0;
    }
    return P::wgrad_launch(f, (const typename P::T*)dy, dw_oihw, Cin, Cout, KH * KW, cin_real, cout_real, ws, ws_bytes,
                           (hipStream_t)stream);
}

// What im2col_bwd_weight launches for this shape, out = {bn, splits, chunk, wide_reduce}: the column tile of the kernel wgrad_launch
// picks (wgrad_bn: 128 / 64 / 32), the pixel split of wgrad_ws_bytes and whether wgrad_reduce takes the wide form
// (wgrad_reduce_takes_wide).  Nothing launched; DWC_EINVAL where im2col_bwd_weight returns it for the shape alone.
template <class P>
int im2col_bwd_weight_plan(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* out) {
    FwdGeom f;
    if (!out || (Cout & P::CH_MASK) || !fwd_geom(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, stride, pad, &f, P::MIN_LOG_C))
        return DWC_EINVAL;
    int splits, chunk;
    wgrad_ws_bytes(f.g.M, f.g.K, Cout, P::WGRAD_SLAB_ROWS, &splits, &chunk);
    out[0] = wgrad_bn(Cout); out[1] = splits; out[2] = chunk; out[3] = wgrad_reduce_takes_wide(splits, f.g.K, Cout) ? 1 : 0;
    return DWC_OK;
}

// with per-axis stride and reflect pad
template <class P>
size_t im2col_bwd_weight_ex_ws_bytes(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride_h, int stride_w, int pad_h,
                                     int pad_w) {
    FwdGeom f;
    if (!fwd_geom_ex(nullptr, nullptr, B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w, &f, P::MIN_LOG_C)) return 0;
    int splits, chunk;
    return wgrad_ws_bytes(f.g.M, f.g.K, Cout, P::WGRAD_SLAB_ROWS, &splits, &chunk);
}

template <class P>
int im2col_bwd_weight_ex(const void* x, const void* dy, float* dw_oihw, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                         int stride_h, int stride_w, int pad_h, int pad_w, int cin_real, int cout_real, void* ws, size_t ws_bytes,
                         void* stream) {
    FwdGeom f;
    if (!fwd_geom_ex(x, nullptr, B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w, &f, P::MIN_LOG_C)) return DWC_EINVAL;
    if (cin_real > Cin || cout_real > Cout || (Cout & P::CH_MASK)) return DWC_EINVAL;
    return P::wgrad_launch(f, (const typename P::T*)dy, dw_oihw, Cin, Cout, KH * KW, cin_real, cout_real, ws, ws_bytes,
                           (hipStream_t)stream);
}

}  // namespace

// The exported functions of one precision, as include/dwcgan_hip.h declares them: NAME(x) pastes the family's prefix (dwc_ /
// dwc_bf16_) in front of x, X is the element type in the signatures (float / void).  Each forwards to its template above.
#define DWC_IM2COL_EXPORTS(NAME, P, X)                                                                                                   \
    extern "C" {                                                                                                                         \
    size_t NAME(weight_prepared_elems)(int Cout, int Cin, int KH, int KW, int stride, int cout_pad, int cin_pad, int for_dgrad) {        \
        return im2col_weight_prepared_elems<P>(Cout, Cin, KH, KW, stride, cout_pad, cin_pad, for_dgrad);                                 \
    }                                                                                                                                    \
    int NAME(weight_prepare_fwd)(const float* w, X* out, int Cout, int Cin, int KH, int KW, int cout_pad, int cin_pad, void* stream) {   \
        return im2col_weight_prepare_fwd<P>(w, out, Cout, Cin, KH, KW, cout_pad, cin_pad, stream);                                       \
    }                                                                                                                                    \
    int NAME(weight_prepare_dgrad)(const float* w, X* out, int Cout, int Cin, int KH, int KW, int stride, int cout_pad, int cin_pad,     \
                                   void* stream) {                                                                                       \
        return im2col_weight_prepare_dgrad<P>(w, out, Cout, Cin, KH, KW, stride, cout_pad, cin_pad, stream);                             \
    }                                                                                                                                    \
    size_t NAME(conv2d_fwd_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {                      \
        return im2col_fwd_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, stride, pad);                                                          \
    }                                                                                                                                    \
    int NAME(conv2d_fwd_plan)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* out) {                   \
        return im2col_fwd_plan<P>(B, H, W, Cin, Cout, KH, KW, stride, pad, out);                                                         \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_weight_plan)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int* out) {            \
        return im2col_bwd_weight_plan<P>(B, H, W, Cin, Cout, KH, KW, stride, pad, out);                                                  \
    }                                                                                                                                    \
    int NAME(conv2d_fwd)(const X* x, const X* w, const float* bias, X* y, int B, int H, int W, int Cin, int Cout, int KH, int KW,        \
                         int stride, int pad, int act, void* ws, size_t ws_bytes, void* stream) {                                        \
        return im2col_fwd<P>(x, w, bias, y, B, H, W, Cin, Cout, KH, KW, stride, pad, act, ws, ws_bytes, stream, 1);                      \
    }                                                                                                                                    \
    int NAME(conv2d_fwd_zeropad)(const X* x, const X* w, const float* bias, X* y, int B, int H, int W, int Cin, int Cout, int KH,        \
                                 int KW, int stride, int pad, int act, void* ws, size_t ws_bytes, void* stream) {                        \
        return im2col_fwd<P>(x, w, bias, y, B, H, W, Cin, Cout, KH, KW, stride, pad, act, ws, ws_bytes, stream, 0);                      \
    }                                                                                                                                    \
    int NAME(conv2d_fwd_ex)(const X* x, const X* w, const float* bias, X* y, int B, int H, int W, int Cin, int Cout, int KH, int KW,     \
                            int stride_h, int stride_w, int pad_h, int pad_w, int act, void* stream) {                                   \
        return im2col_fwd_ex<P>(x, w, bias, y, B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w, act, stream);               \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_data_zeropad_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int pad) {                     \
        return im2col_bwd_data_zeropad_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, pad);                                                     \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_zeropad)(const X* dy, const X* w, X* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW, int pad,   \
                                      void* ws, size_t ws_bytes, void* stream) {                                                         \
        return im2col_bwd_data_zeropad<P>(dy, w, dx, B, H, W, Cin, Cout, KH, KW, pad, ws, ws_bytes, stream);                             \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_data_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {                 \
        return im2col_bwd_data_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, stride, pad);                                                     \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data)(const X* dy, const X* w, X* dxp, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,       \
                              int pad, void* ws, size_t ws_bytes, void* stream) {                                                        \
        return im2col_bwd_data<P>(dy, w, dxp, B, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes, stream);                            \
    }                                                                                                                                    \
    int NAME(reflect_pad_adjoint)(const X* dxp, X* dx, int B, int H, int W, int C, int pad, void* stream) {                              \
        return im2col_reflect_pad_adjoint<P>(dxp, dx, B, H, W, C, pad, stream);                                                          \
    }                                                                                                                                    \
    int NAME(reflect_pad_adjoint_band)(const X* dxp, X* dx, int B, int H, int W, int C, int pad, void* stream) {                         \
        return im2col_reflect_pad_adjoint_band<P>(dxp, dx, B, H, W, C, pad, stream);                                                     \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_fold)(const X* dy, const X* w, X* dxp, X* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW,       \
                                   int stride, int pad, void* ws, size_t ws_bytes, void* stream) {                                       \
        return im2col_bwd_data_fold<P>(dy, w, dxp, dx, B, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes, stream);                   \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_data_same_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int pad) {                        \
        return im2col_bwd_data_same_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, pad);                                                        \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_same)(const X* dy, const X* w, const X* w_t, X* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW, \
                                   int pad, void* ws, size_t ws_bytes, void* stream) {                                                   \
        return im2col_bwd_data_same<P>(dy, w, w_t, dx, B, H, W, Cin, Cout, KH, KW, pad, ws, ws_bytes, stream, false);                    \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_ring)(const X* dy, const X* w, const X* w_t, X* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW, \
                                   int pad, void* ws, size_t ws_bytes, void* stream) {                                                   \
        return im2col_bwd_data_same<P>(dy, w, w_t, dx, B, H, W, Cin, Cout, KH, KW, pad, ws, ws_bytes, stream, true);                     \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_s2_ring)(const X* dy, const X* w, X* dxp, X* dx, int B, int H, int W, int Cin, int Cout, void* stream) {    \
        return im2col_bwd_data_s2_ring<P>(dy, w, dxp, dx, B, H, W, Cin, Cout, stream);                                                   \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_data_image_ws_bytes)(int B, int H, int W, int Cout, int KH, int KW, int pad) {                                \
        return im2col_bwd_data_image_ws_bytes<P>(B, H, W, Cout, KH, KW, pad);                                                            \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_image)(const X* dy, const X* w, X* dx, int B, int H, int W, int Cout, int KH, int KW, int pad, void* ws,    \
                                    size_t ws_bytes, void* stream) {                                                                     \
        return im2col_bwd_data_image<P>(dy, w, dx, B, H, W, Cout, KH, KW, pad, ws, ws_bytes, stream);                                    \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_weight_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {               \
        return im2col_bwd_weight_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, stride, pad);                                                   \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_weight)(const X* x, const X* dy, float* dw, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,  \
                                int pad, int cin_real, int cout_real, void* ws, size_t ws_bytes, void* stream) {                         \
        return im2col_bwd_weight<P>(x, dy, dw, B, H, W, Cin, Cout, KH, KW, stride, pad, cin_real, cout_real, ws, ws_bytes, stream);      \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_weight_zeropad_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {       \
        return im2col_bwd_weight_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, stride, pad);                                                   \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_weight_zeropad)(const X* x, const X* dy, float* dw, int B, int H, int W, int Cin, int Cout, int KH, int KW,      \
                                        int stride, int pad, int cin_real, int cout_real, void* ws, size_t ws_bytes, void* stream) {     \
        return im2col_bwd_weight<P>(x, dy, dw, B, H, W, Cin, Cout, KH, KW, stride, pad, cin_real, cout_real, ws, ws_bytes, stream, 0);   \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_data_crop_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad) {            \
        return im2col_bwd_data_crop_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, stride, pad);                                                \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_data_crop)(const X* dy, const X* w, X* dx, int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride,   \
                                   int pad, void* ws, size_t ws_bytes, void* stream) {                                                   \
        return im2col_bwd_data_crop<P>(dy, w, dx, B, H, W, Cin, Cout, KH, KW, stride, pad, ws, ws_bytes, stream);                        \
    }                                                                                                                                    \
    size_t NAME(conv2d_bwd_weight_ex_ws_bytes)(int B, int H, int W, int Cin, int Cout, int KH, int KW, int stride_h, int stride_w,       \
                                               int pad_h, int pad_w) {                                                                   \
        return im2col_bwd_weight_ex_ws_bytes<P>(B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w);                           \
    }                                                                                                                                    \
    int NAME(conv2d_bwd_weight_ex)(const X* x, const X* dy, float* dw, int B, int H, int W, int Cin, int Cout, int KH, int KW,           \
                                   int stride_h, int stride_w, int pad_h, int pad_w, int cin_real, int cout_real, void* ws,              \
                                   size_t ws_bytes, void* stream) {                                                                      \
        return im2col_bwd_weight_ex<P>(x, dy, dw, B, H, W, Cin, Cout, KH, KW, stride_h, stride_w, pad_h, pad_w, cin_real, cout_real, ws, \
                                       ws_bytes, stream);                                                                                \
    }                                                                                                                                    \
    }
