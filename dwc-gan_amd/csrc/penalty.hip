// Gradient / R1 penalty of the discriminator (reference solver.py:291-315), the passes that are not convolutions (gfx950, fp32):
//   * q_n = |g_n|^2 over the real planes of an NHWC image gradient, the penalty P and dP/dg's per-sample coefficient k_n
//   * ghat = dout * k_n * g, the seed of the second-order chain
//   * d_L = w_s * act'(a_L), the seed of the first-order chain under the 1x1 'src' head
// HBM-bound, 16-byte accesses where the pitch allows (planes == 4 / C % 4 == 0 and aligned pointers), wave shuffles then LDS.
// Every sum is taken in a fixed order: strided per thread, xor butterfly per wave, the waves of the workgroup in index order by
// one thread -- no floating-point atomics, bit-identical run to run.
#include "dwc_common.h"

namespace {

constexpr int PEN_THREADS = 1024;      // one workgroup per sample: 16 waves cover a 128 x 128 image in 16 loads per thread
constexpr int PEN_MAX_GRID = 2048;     // grid cap of the elementwise passes (grid-stride beyond it), as the norm kernels' plans

// sum over the workgroup (blockDim.x a multiple of 64, <= 1024); valid in thread 0 only.  `sm` >= 16 floats.
__device__ __forceinline__ float pen_block_sum(float v, float* sm) {
    v = dwc_wave_sum(v);
    const int wave = threadIdx.x >> 6, waves = (blockDim.x + 63) >> 6;
    __syncthreads();                                     // (sm may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) sm[wave] = v;
    __syncthreads();
    float s = 0.f;
    if (threadIdx.x == 0)
        for (int w = 0; w < waves; ++w) s += sm[w];
    return s;
}

// q[n] = sum over pixels and the first `real` planes of g^2; grid = B.  VEC: planes == 4 and g 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(PEN_THREADS) void penalty_q_kernel(const float* __restrict__ g, float* __restrict__ q, int pixels, int planes,
                                                                int real) {
    __shared__ float sm[16];
    const float* gn = g + (size_t)blockIdx.x * pixels * planes;
    float s = 0.f;
    if (VEC) {
        for (int p = threadIdx.x; p < pixels; p += PEN_THREADS) {
            const f32x4 v = reinterpret_cast<const f32x4*>(gn)[p];
            float t = v[0] * v[0];
            if (real > 1) t += v[1] * v[1];
            if (real > 2) t += v[2] * v[2];
            if (real > 3) t += v[3] * v[3];
            s += t;
        }
    } else {
        for (int p = threadIdx.x; p < pixels; p += PEN_THREADS) {
            float t = 0.f;
            for (int c = 0; c < real; ++c) {
                const float v = gn[(size_t)p * planes + c];
                t += v * v;
            }
            s += t;
        }
    }
    s = pen_block_sum(s, sm);
    if (threadIdx.x == 0) q[blockIdx.x] = s;
}

// k[n] and P from q[0..B): one workgroup of 256 threads
__global__ __launch_bounds__(256) void penalty_final_kernel(const float* __restrict__ q, float* __restrict__ k, float* __restrict__ out,
                                                            int B, int mode) {
    __shared__ float sm[16];
    const float inv_b = 1.f / (float)B;
    float s = 0.f;
    for (int n = threadIdx.x; n < B; n += 256) {
        const float qn = q[n];
        if (mode == DWC_PENALTY_GP) {
            const float r = sqrtf(qn);
            s += (r - 1.f) * (r - 1.f);
            k[n] = qn > 0.f ? 2.f * (r - 1.f) / ((float)B * r) : 0.f;      // (d sqrt at 0: the sample contributes no gradient)
        } else {
            s += qn * qn;
            k[n] = 4.f * qn * inv_b;
        }
    }
    s = pen_block_sum(s, sm);
    if (threadIdx.x == 0) out[0] = s * inv_b;
}

// ghat = dout[0] * k[n] * g on the real planes, 0 elsewhere; grid (pixel chunks, B)
template <bool VEC>
__global__ __launch_bounds__(256) void penalty_scale_kernel(const float* __restrict__ g, const float* __restrict__ k,
                                                            const float* __restrict__ dout, float* __restrict__ ghat, int pixels,
                                                            int planes, int real) {
    const float sc = dout[0] * k[blockIdx.y];
    const size_t base = (size_t)blockIdx.y * pixels * planes;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < pixels; p += gridDim.x * 256) {
        if (VEC) {
            const f32x4 v = reinterpret_cast<const f32x4*>(g + base)[p];
            f32x4 o;
            o[0] = sc * v[0];
            o[1] = real > 1 ? sc * v[1] : 0.f;
            o[2] = real > 2 ? sc * v[2] : 0.f;
            o[3] = real > 3 ? sc * v[3] : 0.f;
            reinterpret_cast<f32x4*>(ghat + base)[p] = o;
        } else {
            for (int c = 0; c < planes; ++c) {
                const size_t i = base + (size_t)p * planes + c;
                ghat[i] = c < real ? sc * g[i] : 0.f;
            }
        }
    }
}

// d[r][c] = w[c] * act'(a[r][c]); n4 = rows * C / 4 groups of 4 channels, cq = C / 4
__global__ __launch_bounds__(256) void src_head_seed_kernel(const float* __restrict__ a, const float* __restrict__ w, float* __restrict__ d,
                                                            size_t n4, int cq, int act) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
        const int col = (int)(i % (size_t)cq);
        const f32x4 y = reinterpret_cast<const f32x4*>(a)[i];
        const f32x4 ww = reinterpret_cast<const f32x4*>(w)[col];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ww[j] * dwc_act_grad(y[j], act, 0);
        reinterpret_cast<f32x4*>(d)[i] = o;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool penalty_args_ok(int B, int pixels, int planes, int real_planes) {
    return B > 0 && B <= 65535 && pixels > 0 && planes > 0 && real_planes > 0 && real_planes <= planes &&
           (size_t)pixels * planes < ((size_t)1 << 31);
}

}  // namespace

extern "C" {

int dwc_grad_penalty_fwd(const float* g, float* q, float* k, float* out, int B, int pixels, int planes, int real_planes, int mode,
                         void* stream) {
    if (!g || !q || !k || !out || !penalty_args_ok(B, pixels, planes, real_planes)) return DWC_EINVAL;
    if (mode != DWC_PENALTY_GP && mode != DWC_PENALTY_R1) return DWC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (planes == 4 && aligned16(g))
        hipLaunchKernelGGL(penalty_q_kernel<true>, dim3(B), dim3(PEN_THREADS), 0, st, g, q, pixels, planes, real_planes);
    else
        hipLaunchKernelGGL(penalty_q_kernel<false>, dim3(B), dim3(PEN_THREADS), 0, st, g, q, pixels, planes, real_planes);
    DWC_LAUNCH_CHECK();
    hipLaunchKernelGGL(penalty_final_kernel, dim3(1), dim3(256), 0, st, (const float*)q, k, out, B, mode);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_grad_penalty_scale(const float* g, const float* k, const float* dout, float* ghat, int B, int pixels, int planes,
                           int real_planes, void* stream) {
    if (!g || !k || !dout || !ghat || !penalty_args_ok(B, pixels, planes, real_planes)) return DWC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int chunks = (pixels + 255) / 256;
    const int cap = PEN_MAX_GRID / B > 0 ? PEN_MAX_GRID / B : 1;
    if (chunks > cap) chunks = cap;
    if (planes == 4 && aligned16(g) && aligned16(ghat))
        hipLaunchKernelGGL(penalty_scale_kernel<true>, dim3(chunks, B), dim3(256), 0, st, g, k, dout, ghat, pixels, planes, real_planes);
    else
        hipLaunchKernelGGL(penalty_scale_kernel<false>, dim3(chunks, B), dim3(256), 0, st, g, k, dout, ghat, pixels, planes, real_planes);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_src_head_seed(const float* a, const float* w_s, float* d, int rows, int C, int act, void* stream) {
    if (!a || !w_s || !d || rows <= 0 || C <= 0 || (C & 3)) return DWC_EINVAL;
    if (act != DWC_ACT_NONE && act != DWC_ACT_RELU && act != DWC_ACT_LRELU) return DWC_EINVAL;
    if (!aligned16(a) || !aligned16(w_s) || !aligned16(d)) return DWC_EINVAL;
    const size_t n4 = (size_t)rows * (C / 4);
    size_t blocks = (n4 + 255) / 256;
    if (blocks > (size_t)PEN_MAX_GRID) blocks = PEN_MAX_GRID;
    hipLaunchKernelGGL(src_head_seed_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, w_s, d, n4, C / 4, act);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

}  // extern "C"
