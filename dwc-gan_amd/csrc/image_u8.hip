// uint8 HWC crops -> the trainer's internal image buffer (NHWC4 fp32 / NHWC8 bf16) in one launch: PIL's antialiased BILINEAR
// resize of an 8-bit image followed by the loader's normalisation, bit for bit (gfx950).
//
// PIL resizes an 8-bit image with integer arithmetic only: a horizontal pass into an 8-bit intermediate, then a vertical pass,
// each pixel = clip(((1 << 21) + sum_k v[start + k] * coef[k]) >> 22, 0, 255) with per-output-index windows (start, coef[ksize])
// that hipdwc/u8image.py builds on the host in float64 by PIL's rule.  The kernel repeats exactly that in 32-bit integers (the
// coefficients of a window sum to 2^22 give or take ksize roundings, so 255 * sum + 2^21 < 2^31) and then looks the byte up in a
// 256-entry fp32 table holding ((b / 255) - 0.5) / 0.5 as the loader computes it: no division and no float arithmetic on the device.
//
// One workgroup takes one image and one band of output rows.  The horizontal pass writes the source rows the band needs, at the
// output width, as bytes: into LDS where rows x Wout x 3 fits (the band shrinks from 16 rows until it does), else into the
// workgroup's own slice of caller scratch.  After a barrier the vertical pass reads them back, looks up and stores one 16-byte pixel.
// HBM-trivial (12 MB in, 34 MB out at B = 128, 178 -> 128), so it is written plainly: byte loads (a source row is 534 bytes, not
// 4-byte aligned), plain C++ stores.  Windows come from caller memory, so every index taken from them is clamped before use.
#include "dwc_common.h"

namespace {

constexpr int IU8_MAX_DIM = 16384;       // largest accepted extent of either image, per axis
constexpr int IU8_BAND = 16;             // output rows per workgroup (fewer where the LDS would not hold their source rows)
constexpr size_t IU8_LDS_BYTES = 65536;  // dynamic LDS a launch may ask for without opting in to more

int iu8_ksize(int n_in, int n_out) {     // 2 * ceil(max(n_in / n_out, 1)) + 1
    return 2 * (n_in <= n_out ? 1 : (n_in + n_out - 1) / n_out) + 1;
}

// Source rows a band of `band` output rows can need: the windows of its first and last row lie at most (band - 1) * scale apart and
// each reaches `support` to either side of its centre (+ 2: the two roundings to whole rows).
int iu8_rows_cap(int Hin, int Hout, int band) {
    const double scale = (double)Hin / Hout, support = scale < 1.0 ? 1.0 : scale;
    const double rows = (band - 1) * scale + 2.0 * support + 2.0;
    return rows < (double)Hin ? (int)rows : Hin;
}

struct Iu8Plan {
    bool ok, lds;
    int band, nbands, rows_cap;
    size_t tile_bytes, ws_bytes;
};

Iu8Plan iu8_plan(int B, int Hin, int Win, int C, int Hout, int Wout) {
    Iu8Plan p = {};
    if (C != 3 || B <= 0 || B > 65535 || Hin <= 0 || Win <= 0 || Hout <= 0 || Wout <= 0 || Hin > IU8_MAX_DIM || Win > IU8_MAX_DIM ||
        Hout > IU8_MAX_DIM || Wout > IU8_MAX_DIM)
        return p;
    // Image.resize shrinks an image more than 100 times as tall as wide vertically FIRST: another 8-bit intermediate, other bytes
    if ((long)Hin > 100L * Win && Hout < Hin) return p;
    p.ok = true;
    p.band = IU8_BAND < Hout ? IU8_BAND : Hout;
    while (p.band > 1 && (size_t)iu8_rows_cap(Hin, Hout, p.band) * Wout * 3 > IU8_LDS_BYTES) p.band /= 2;
    p.lds = (size_t)iu8_rows_cap(Hin, Hout, p.band) * Wout * 3 <= IU8_LDS_BYTES;
    if (!p.lds) p.band = IU8_BAND < Hout ? IU8_BAND : Hout;     // scratch holds any band: back to the full one
    p.nbands = (Hout + p.band - 1) / p.band;
    p.rows_cap = iu8_rows_cap(Hin, Hout, p.band);
    p.tile_bytes = ((size_t)p.rows_cap * Wout * 3 + 15) & ~(size_t)15;
    p.ws_bytes = p.lds ? 0 : p.tile_bytes * p.nbands * B;
    return p;
}

__device__ __forceinline__ int iu8_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ __forceinline__ void iu8_store(float* y, size_t pix, float a, float b, float c) {
    reinterpret_cast<f32x4*>(y)[pix] = f32x4{a, b, c, 0.f};
}
__device__ __forceinline__ void iu8_store(dwc_bf16* y, size_t pix, float a, float b, float c) {
    dwc_bf16x8 v;
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (dwc_bf16)0.f;
    v[0] = (dwc_bf16)a; v[1] = (dwc_bf16)b; v[2] = (dwc_bf16)c;      // the conversion of pack_nhwc8_kernel (csrc/pointwise.hip)
    reinterpret_cast<dwc_bf16x8*>(y)[pix] = v;
}

// grid (bands, B), 256 threads.  `tile`: this workgroup's rows_cap x Wout x 3 bytes (LDS or its slice of scratch).
template <typename T>
__device__ __forceinline__ void iu8_band(const uint8_t* __restrict__ u8, const int* __restrict__ xstart, const int* __restrict__ xcoef,
                                         const int* __restrict__ ystart, const int* __restrict__ ycoef, const float* __restrict__ lut,
                                         T* __restrict__ y, uint8_t* tile, int Hin, int Win, int Hout, int Wout, int kx, int ky, int band,
                                         int rows_cap) {
    const int n = blockIdx.y;
    const int r0 = blockIdx.x * band;
    const int r1 = min(r0 + band, Hout);                             // output rows [r0, r1)
    // windows start in non-decreasing order: the band reads source rows [y0, y0 + rows)
    const int y0 = min(max(ystart[r0], 0), Hin - 1);
    const int yend = min(max(ystart[r1 - 1], y0) + ky, Hin);
    const int rows = min(yend - y0, rows_cap);
    const uint8_t* src = u8 + ((size_t)n * Hin + y0) * Win * 3;

    for (int i = threadIdx.x; i < rows * Wout; i += blockDim.x) {    // horizontal pass
        const int r = i / Wout, x = i - r * Wout;
        const int xs = min(max(xstart[x], 0), Win - 1);
        const int taps = min(kx, Win - xs);
        const uint8_t* p = src + ((size_t)r * Win + xs) * 3;
        const int* k = xcoef + (size_t)x * kx;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < taps; ++t) {
            const int c = k[t];
            a0 += p[3 * t] * c; a1 += p[3 * t + 1] * c; a2 += p[3 * t + 2] * c;
        }
        uint8_t* q = tile + (size_t)i * 3;
        q[0] = (uint8_t)iu8_clip8(a0); q[1] = (uint8_t)iu8_clip8(a1); q[2] = (uint8_t)iu8_clip8(a2);
    }
    __syncthreads();                                                 // (orders the workgroup's own scratch writes too)

    for (int i = threadIdx.x; i < (r1 - r0) * Wout; i += blockDim.x) {   // vertical pass, lookup, store
        const int r = i / Wout, x = i - r * Wout, oy = r0 + r;
        const int ys = min(max(ystart[oy], y0), y0 + rows - 1);
        const int taps = min(ky, y0 + rows - ys);
        const uint8_t* p = tile + ((size_t)(ys - y0) * Wout + x) * 3;
        const int* k = ycoef + (size_t)oy * ky;
        int a0 = 1 << 21, a1 = 1 << 21, a2 = 1 << 21;
        for (int t = 0; t < taps; ++t) {
            const int c = k[t];
            const uint8_t* v = p + (size_t)t * Wout * 3;
            a0 += v[0] * c; a1 += v[1] * c; a2 += v[2] * c;
        }
        iu8_store(y, ((size_t)n * Hout + oy) * Wout + x, lut[iu8_clip8(a0)], lut[iu8_clip8(a1)], lut[iu8_clip8(a2)]);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void image_u8_lds_kernel(const uint8_t* u8, const int* xstart, const int* xcoef, const int* ystart,
                                                           const int* ycoef, const float* lut, T* y, int Hin, int Win, int Hout, int Wout,
                                                           int kx, int ky, int band, int rows_cap) {
    extern __shared__ uint8_t iu8_tile[];
    iu8_band<T>(u8, xstart, xcoef, ystart, ycoef, lut, y, iu8_tile, Hin, Win, Hout, Wout, kx, ky, band, rows_cap);
}

template <typename T>
__global__ __launch_bounds__(256) void image_u8_ws_kernel(const uint8_t* u8, const int* xstart, const int* xcoef, const int* ystart,
                                                          const int* ycoef, const float* lut, T* y, uint8_t* ws, size_t tile_bytes, int Hin,
                                                          int Win, int Hout, int Wout, int kx, int ky, int band, int rows_cap) {
    uint8_t* tile = ws + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * tile_bytes;
    iu8_band<T>(u8, xstart, xcoef, ystart, ycoef, lut, y, tile, Hin, Win, Hout, Wout, kx, ky, band, rows_cap);
}

template <typename T>
int image_u8_launch(const uint8_t* u8, const int* xstart, const int* xcoef, const int* ystart, const int* ycoef, const float* lut, T* y,
                    int B, int Hin, int Win, int C, int Hout, int Wout, void* ws, size_t ws_bytes, void* stream) {
    const Iu8Plan p = iu8_plan(B, Hin, Win, C, Hout, Wout);
    if (!p.ok || !u8 || !xstart || !xcoef || !ystart || !ycoef || !lut || !y) return DWC_EINVAL;
    if (p.ws_bytes && (!ws || ws_bytes < p.ws_bytes)) return DWC_EWORKSPACE;
    const int kx = iu8_ksize(Win, Wout), ky = iu8_ksize(Hin, Hout);
    const dim3 grid(p.nbands, B);
    if (p.lds)
        hipLaunchKernelGGL(image_u8_lds_kernel<T>, grid, dim3(256), (size_t)p.rows_cap * Wout * 3, (hipStream_t)stream, u8, xstart, xcoef,
                           ystart, ycoef, lut, y, Hin, Win, Hout, Wout, kx, ky, p.band, p.rows_cap);
    else
        hipLaunchKernelGGL(image_u8_ws_kernel<T>, grid, dim3(256), 0, (hipStream_t)stream, u8, xstart, xcoef, ystart, ycoef, lut, y,
                           (uint8_t*)ws, p.tile_bytes, Hin, Win, Hout, Wout, kx, ky, p.band, p.rows_cap);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

}  // namespace

int dwc_image_u8_ksize(int n_in, int n_out) {
    return (n_in <= 0 || n_out <= 0 || n_in > IU8_MAX_DIM || n_out > IU8_MAX_DIM) ? 0 : iu8_ksize(n_in, n_out);
}

size_t dwc_image_u8_ws_bytes(int B, int Hin, int Win, int C, int Hout, int Wout) {
    return iu8_plan(B, Hin, Win, C, Hout, Wout).ws_bytes;
}

int dwc_image_u8_to_nhwc4(const uint8_t* u8, const int* xstart, const int* xcoef, const int* ystart, const int* ycoef, const float* lut,
                          float* y, int B, int Hin, int Win, int C, int Hout, int Wout, void* ws, size_t ws_bytes, void* stream) {
    return image_u8_launch<float>(u8, xstart, xcoef, ystart, ycoef, lut, y, B, Hin, Win, C, Hout, Wout, ws, ws_bytes, stream);
}

int dwc_bf16_image_u8_to_nhwc8(const uint8_t* u8, const int* xstart, const int* xcoef, const int* ystart, const int* ycoef,
                               const float* lut, void* y, int B, int Hin, int Win, int C, int Hout, int Wout, void* ws, size_t ws_bytes,
                               void* stream) {
    return image_u8_launch<dwc_bf16>(u8, xstart, xcoef, ystart, ycoef, lut, (dwc_bf16*)y, B, Hin, Win, C, Hout, Wout, ws, ws_bytes, stream);
}
