// Image batches -> one uint8 HWC grid: make_grid(nrow, padding 0, normalize) and save_image's byte conversion of the reference's
// image writers (reference utils.py:69-73), byte for byte what the chain of CPU tensor ops gives (gfx950).
//
// The chain is, per value and with every operation rounded to fp32 on its own:
//     v = min(max(x, lo), hi);  v = v - lo;  v = v / d;  v = v * 255;  v = v + 0.5;  byte = (uint8) min(max(v, 0), 255)
// with d = (float) max((double) hi - (double) lo, 1e-5).  A multiplication by 1 / d or a fused v * 255 + 0.5 gives other bytes at
// the rounding boundaries, so this file is compiled with contraction off (pragma below and -ffp-contract=off in the Makefile) and
// divides with `/`, which hipcc rounds correctly for fp32.
//
// Up to DWC_IMAGE_OUT_MAX_SOURCES sources in four layouts enter through one by-value table.  Without a value_range a first launch
// leaves one (min, max) pair per workgroup in caller scratch, over exactly the values that enter: the used images, planes 0..2.
// Every workgroup of the second launch reduces those pairs again (min and max are exact, so neither order nor repetition matters),
// then converts: four neighbouring pixels per thread as three 32-bit stores where W % 4 == 0, one pixel per thread as three bytes
// otherwise.  Memory-bound and tiny (at most 16 bytes in and 3 out per pixel), so it is written plainly.
#include "dwc_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int IO_MAX_DIM = 16384;        // largest accepted H or W, as on the input side (csrc/image_u8.hip)
constexpr int IO_MAX_BATCH = 65535;
constexpr int IO_THREADS = 256;
constexpr int IO_MAX_BLOCKS = 2048;      // map launch: grid-stride beyond this
constexpr long IO_ITEMS_PER_BLOCK = 4L * IO_THREADS;     // range launch: 16-byte loads per workgroup before another one is added

struct IoSource {
    const void* p;
    int layout;
    int used;        // images of this source that enter
    int first;       // grid index of its first image
    int vec;         // dense layouts: the pointer is 16-byte aligned (rows of 4 floats may be loaded whole where W % 4 == 0)
};

struct IoTable {
    int K, N;        // sources; images in the grid
    IoSource s[DWC_IMAGE_OUT_MAX_SOURCES];
};

struct IoPlan {
    bool ok;
    int N, cols, rows, nparts;
    long range_items;                    // 16-byte (or tail) loads of the range launch, all sources
    size_t ws_bytes;
};

__host__ __device__ inline long io_range_items(int layout, int used, int H, int W) {
    const long px = (long)used * H * W;
    if (layout == DWC_IMAGE_OUT_NHWC4 || layout == DWC_IMAGE_OUT_NHWC8_BF16) return px;      // one pixel per load
    const long n = layout == DWC_IMAGE_OUT_NCHW3 ? 3 * px : px;                             // a dense prefix of the buffer
    return n / 4 + n % 4;                                                                    // whole quads, then single floats
}

IoPlan io_plan(const int* layout, const int* batch, const int* used, int K, int H, int W, int nrow, bool from_data) {
    IoPlan p = {};
    if (!layout || !batch || !used || K < 1 || K > DWC_IMAGE_OUT_MAX_SOURCES || H < 1 || W < 1 || nrow < 1 || H > IO_MAX_DIM ||
        W > IO_MAX_DIM)
        return p;
    long n = 0;
    for (int k = 0; k < K; ++k) {
        if (layout[k] < DWC_IMAGE_OUT_NCHW1 || layout[k] > DWC_IMAGE_OUT_NHWC8_BF16) return p;
        if (batch[k] < 1 || batch[k] > IO_MAX_BATCH || used[k] < 1 || used[k] > batch[k]) return p;
        n += used[k];
        p.range_items += io_range_items(layout[k], used[k], H, W);
    }
    p.ok = true;
    p.N = (int)n;                                                   // <= 8 * 65535
    p.cols = nrow < p.N ? nrow : p.N;
    p.rows = (p.N + p.cols - 1) / p.cols;
    if (from_data) {
        const long want = (p.range_items + IO_ITEMS_PER_BLOCK - 1) / IO_ITEMS_PER_BLOCK;
        p.nparts = (int)(want < DWC_IMAGE_OUT_MAX_PARTIALS ? want : DWC_IMAGE_OUT_MAX_PARTIALS);
        p.ws_bytes = (size_t)p.nparts * 2 * sizeof(float);
    }
    return p;
}

// ---- reductions -------------------------------------------------------------------------------------------------------------------
// fminf / fmaxf drop a NaN operand: a NaN never becomes the range (its bytes are unspecified anyway).
__device__ __forceinline__ void io_wave_minmax(float& lo, float& hi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
}

// over the 256 threads of a workgroup; the result is valid in every thread.  `sm`: 8 floats.
__device__ __forceinline__ void io_block_minmax(float& lo, float& hi, float* sm) {
    io_wave_minmax(lo, hi);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wave] = lo; sm[4 + wave] = hi; }
    __syncthreads();
    lo = fminf(fminf(sm[0], sm[1]), fminf(sm[2], sm[3]));
    hi = fmaxf(fmaxf(sm[4], sm[5]), fmaxf(sm[6], sm[7]));
}

__device__ __forceinline__ void io_fold(float& lo, float& hi, float v) { lo = fminf(lo, v); hi = fmaxf(hi, v); }

// grid nparts, 256 threads: parts[2 * block] = min, parts[2 * block + 1] = max of this workgroup's share (+inf / -inf for an empty one)
__global__ __launch_bounds__(IO_THREADS) void image_out_range_kernel(IoTable t, int H, int W, float* __restrict__ parts) {
    __shared__ float sm[8];
    float lo = __builtin_inff(), hi = -__builtin_inff();
    const long stride = (long)gridDim.x * IO_THREADS;
    for (int k = 0; k < t.K; ++k) {
        const IoSource s = t.s[k];
        const long items = io_range_items(s.layout, s.used, H, W);
        if (s.layout == DWC_IMAGE_OUT_NHWC4) {
            const f32x4* p = reinterpret_cast<const f32x4*>(s.p);
            for (long i = (long)blockIdx.x * IO_THREADS + threadIdx.x; i < items; i += stride) {
                const f32x4 v = p[i];
                io_fold(lo, hi, v[0]); io_fold(lo, hi, v[1]); io_fold(lo, hi, v[2]);      // plane 3: attention map or padding
            }
        } else if (s.layout == DWC_IMAGE_OUT_NHWC8_BF16) {
            const dwc_bf16x8* p = reinterpret_cast<const dwc_bf16x8*>(s.p);
            for (long i = (long)blockIdx.x * IO_THREADS + threadIdx.x; i < items; i += stride) {
                const dwc_bf16x8 v = p[i];
                io_fold(lo, hi, (float)v[0]); io_fold(lo, hi, (float)v[1]); io_fold(lo, hi, (float)v[2]);
            }
        } else {
            const float* p = reinterpret_cast<const float*>(s.p);
            const long n = (long)s.used * H * W * (s.layout == DWC_IMAGE_OUT_NCHW3 ? 3 : 1);
            const long quads = n / 4;
            for (long i = (long)blockIdx.x * IO_THREADS + threadIdx.x; i < items; i += stride) {
                if (i < quads) {
                    if (s.vec) {
                        const f32x4 v = reinterpret_cast<const f32x4*>(p)[i];
                        io_fold(lo, hi, v[0]); io_fold(lo, hi, v[1]); io_fold(lo, hi, v[2]); io_fold(lo, hi, v[3]);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e) io_fold(lo, hi, p[4 * i + e]);
                    }
                } else {
                    io_fold(lo, hi, p[4 * quads + (i - quads)]);
                }
            }
        }
    }
    io_block_minmax(lo, hi, sm);
    if (threadIdx.x == 0) { parts[2 * blockIdx.x] = lo; parts[2 * blockIdx.x + 1] = hi; }
}

// ---- conversion -------------------------------------------------------------------------------------------------------------------
struct IoRange { float lo, hi, d; };

__device__ __forceinline__ IoRange io_range(double lo, double hi) {
    const double span = hi - lo;
    IoRange r;
    r.lo = (float)lo; r.hi = (float)hi;
    r.d = (float)(span > 1e-5 ? span : 1e-5);
    return r;
}

__device__ __forceinline__ unsigned io_byte(float x, IoRange r) {
    float v = fminf(fmaxf(x, r.lo), r.hi);
    v = v - r.lo;
    v = v / r.d;
    v = v * 255.f;
    v = v + 0.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);           // (a NaN leaves here as 0: the conversion below is always defined)
    return (unsigned)(int)v;
}

// the source of grid image j (j < t.N), and j's index inside it
__device__ __forceinline__ IoSource io_find(const IoTable& t, int j, int& b) {
    IoSource s = t.s[0];                       // (selects over the by-value table: no per-lane index into it)
#pragma unroll
    for (int q = 1; q < DWC_IMAGE_OUT_MAX_SOURCES; ++q)
        if (q < t.K && j >= t.s[q].first) s = t.s[q];
    b = j - s.first;
    return s;
}

// channels of pixel (y, x) of image b
__device__ __forceinline__ void io_load1(const IoSource& s, int b, int y, int x, int H, int W, float (&c)[3]) {
    const size_t px = ((size_t)b * H + y) * W + x;
    if (s.layout == DWC_IMAGE_OUT_NHWC4) {
        const f32x4 v = reinterpret_cast<const f32x4*>(s.p)[px];
        c[0] = v[0]; c[1] = v[1]; c[2] = v[2];
    } else if (s.layout == DWC_IMAGE_OUT_NHWC8_BF16) {
        const dwc_bf16x8 v = reinterpret_cast<const dwc_bf16x8*>(s.p)[px];
        c[0] = (float)v[0]; c[1] = (float)v[1]; c[2] = (float)v[2];
    } else if (s.layout == DWC_IMAGE_OUT_NCHW3) {
        const float* p = reinterpret_cast<const float*>(s.p) + ((size_t)b * 3 * H + y) * W + x;
        c[0] = p[0]; c[1] = p[(size_t)H * W]; c[2] = p[2 * (size_t)H * W];
    } else {
        c[0] = c[1] = c[2] = reinterpret_cast<const float*>(s.p)[px];
    }
}

__device__ __forceinline__ f32x4 io_row4(const float* p, int vec) {
    if (vec) return *reinterpret_cast<const f32x4*>(p);
    return f32x4{p[0], p[1], p[2], p[3]};
}

// channels of pixels (y, x .. x + 3) of image b; x % 4 == 0 and W % 4 == 0
__device__ __forceinline__ void io_load4(const IoSource& s, int b, int y, int x, int H, int W, float (&c)[4][3]) {
    const size_t px = ((size_t)b * H + y) * W + x;
    if (s.layout == DWC_IMAGE_OUT_NHWC4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 v = reinterpret_cast<const f32x4*>(s.p)[px + i];
            c[i][0] = v[0]; c[i][1] = v[1]; c[i][2] = v[2];
        }
    } else if (s.layout == DWC_IMAGE_OUT_NHWC8_BF16) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const dwc_bf16x8 v = reinterpret_cast<const dwc_bf16x8*>(s.p)[px + i];
            c[i][0] = (float)v[0]; c[i][1] = (float)v[1]; c[i][2] = (float)v[2];
        }
    } else if (s.layout == DWC_IMAGE_OUT_NCHW3) {
        const float* p = reinterpret_cast<const float*>(s.p) + ((size_t)b * 3 * H + y) * W + x;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const f32x4 v = io_row4(p + ch * (size_t)H * W, s.vec);
            c[0][ch] = v[0]; c[1][ch] = v[1]; c[2][ch] = v[2]; c[3][ch] = v[3];
        }
    } else {
        const f32x4 v = io_row4(reinterpret_cast<const float*>(s.p) + px, s.vec);
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i][0] = c[i][1] = c[i][2] = v[i];
    }
}

// QUAD: a thread converts 4 neighbouring pixels of one image row (W % 4 == 0, out 4-byte aligned); else one pixel.
// nparts > 0: the range is the reduction of parts[0 .. 2 * nparts); else it is (lo, hi).
template <bool QUAD>
__global__ __launch_bounds__(IO_THREADS) void image_out_map_kernel(IoTable t, int H, int W, int cols, int rows, const float* __restrict__ parts,
                                                                   int nparts, double lo, double hi, uint8_t* __restrict__ out) {
    __shared__ float sm[8];
    if (nparts > 0) {                                               // (workgroup-uniform)
        float a = __builtin_inff(), b = -__builtin_inff();
        if ((int)threadIdx.x < nparts) { a = parts[2 * threadIdx.x]; b = parts[2 * threadIdx.x + 1]; }     // nparts <= 256 threads
        io_block_minmax(a, b, sm);
        lo = (double)a; hi = (double)b;
    }
    const IoRange r = io_range(lo, hi);
    const long gw = (long)cols * W;                                 // pixels per grid row
    const long per_row = QUAD ? gw / 4 : gw;
    const long items = (long)rows * H * per_row;
    for (long i = (long)blockIdx.x * IO_THREADS + threadIdx.x; i < items; i += (long)gridDim.x * IO_THREADS) {
        const long gy = i / per_row;
        const long gx = (i - gy * per_row) * (QUAD ? 4 : 1);
        const int ry = (int)(gy / H), y = (int)(gy - (long)ry * H);
        const int cx = (int)(gx / W), x = (int)(gx - (long)cx * W);
        const long j = (long)ry * cols + cx;
        uint8_t* o = out + (gy * gw + gx) * 3;
        if (QUAD) {
            unsigned w0 = 0, w1 = 0, w2 = 0;
            if (j < t.N) {
                int b;
                const IoSource s = io_find(t, (int)j, b);
                float c[4][3];
                io_load4(s, b, y, x, H, W, c);
                unsigned q[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) q[e] = io_byte(c[e / 3][e % 3], r);
                w0 = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
                w1 = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
                w2 = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
            }
            unsigned* o4 = reinterpret_cast<unsigned*>(o);          // (gy * gw + gx) * 3 is a multiple of 12
            o4[0] = w0; o4[1] = w1; o4[2] = w2;
        } else {
            unsigned q0 = 0, q1 = 0, q2 = 0;
            if (j < t.N) {
                int b;
                const IoSource s = io_find(t, (int)j, b);
                float c[3];
                io_load1(s, b, y, x, H, W, c);
                q0 = io_byte(c[0], r); q1 = io_byte(c[1], r); q2 = io_byte(c[2], r);
            }
            o[0] = (uint8_t)q0; o[1] = (uint8_t)q1; o[2] = (uint8_t)q2;
        }
    }
}

}  // namespace

size_t dwc_image_out_ws_bytes(const int* layout, const int* batch, const int* used, int K, int H, int W, int nrow, int from_data) {
    return io_plan(layout, batch, used, K, H, W, nrow, from_data != 0).ws_bytes;
}

int dwc_image_out_grid_u8(const void* const* src, const int* layout, const int* batch, const int* used, int K, int H, int W, int nrow,
                          const double* value_range, uint8_t* out, void* ws, size_t ws_bytes, void* stream) {
    const IoPlan p = io_plan(layout, batch, used, K, H, W, nrow, value_range == nullptr);
    if (!p.ok || !src || !out) return DWC_EINVAL;
    IoTable t = {};
    t.K = K; t.N = p.N;
    int first = 0;
    for (int k = 0; k < K; ++k) {
        const bool internal = layout[k] == DWC_IMAGE_OUT_NHWC4 || layout[k] == DWC_IMAGE_OUT_NHWC8_BF16;
        const uintptr_t a = (uintptr_t)src[k];
        if (!src[k] || (a & (internal ? 15 : 3))) return DWC_EINVAL;
        t.s[k].p = src[k]; t.s[k].layout = layout[k]; t.s[k].used = used[k]; t.s[k].first = first;
        t.s[k].vec = (a & 15) == 0;
        first += used[k];
    }
    if (p.ws_bytes && (!ws || ws_bytes < p.ws_bytes || ((uintptr_t)ws & 3))) return DWC_EWORKSPACE;
    if (p.nparts) {
        hipLaunchKernelGGL(image_out_range_kernel, dim3(p.nparts), dim3(IO_THREADS), 0, (hipStream_t)stream, t, H, W, (float*)ws);
        DWC_LAUNCH_CHECK();
    }
    const double lo = value_range ? value_range[0] : 0.0, hi = value_range ? value_range[1] : 0.0;
    const bool quad = W % 4 == 0 && ((uintptr_t)out & 3) == 0;
    const long items = (long)p.rows * H * ((long)p.cols * W / (quad ? 4 : 1));
    const long want = (items + IO_THREADS - 1) / IO_THREADS;
    const dim3 grid((unsigned)(want < IO_MAX_BLOCKS ? want : IO_MAX_BLOCKS));
    if (quad)
        hipLaunchKernelGGL(image_out_map_kernel<true>, grid, dim3(IO_THREADS), 0, (hipStream_t)stream, t, H, W, p.cols, p.rows,
                           (const float*)ws, p.nparts, lo, hi, out);
    else
        hipLaunchKernelGGL(image_out_map_kernel<false>, grid, dim3(IO_THREADS), 0, (hipStream_t)stream, t, H, W, p.cols, p.rows,
                           (const float*)ws, p.nparts, lo, hi, out);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}
