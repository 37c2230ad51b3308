// Spectral normalisation of convolution weights (reference networks.py:754-816, norm='sn'): the power iteration for every SN layer
// of a network in a few plain launches, and the segmented epilogues that apply 1/sigma_s to a convolution run on W_bar itself.
//
// Per layer, W_bar is viewed as [Cout, K] (K = Cin*kh*kw, torch's [Cout, Cin, kh, kw] order).  Iteration s (eps = 1e-12):
//     t = W_bar^T u_{s-1};  v_s = t / (|t| + eps);  w = W_bar v_s;  u_s = w / (|w| + eps);  sigma_s = u_s . w;  r_s = 1 / sigma_s
// with u_{-1} the layer's weight_u parameter as stored.  The raw t_s and w_s go to the caller's saved buffer (V_s / U_s rows); a
// launch that needs the normalised vector recomputes the norm from the short raw vector itself (fixed order, so every workgroup
// gets the same value), and the finalize launch normalises the rows in place, writes r_s and the last u / v into the parameters.
// No float atomics and no cross-workgroup hand-off: every reduction has one fixed order, results are bit-identical run to run.
#include <algorithm>

#include "dwc_common.h"

namespace {

constexpr float SN_EPS = 1e-12f;
constexpr int SN_COLS = 64;        // columns of W_bar per workgroup of the t = W_bar^T u launch
constexpr int SN_ROWS = 8;         // rows of W_bar per workgroup of the w = W_bar v launch (two per wave)
constexpr int SN_MAX_K = 8192;     // v is staged in LDS by the row launch
constexpr int SN_MAX_COUT = 1024;  // u is staged in LDS by the column launch

// sum of squares of p[0..n) over the 256 threads of a block, fixed order; valid in every thread
__device__ float sn_sumsq(const float* p, int n, float* sm) {
    float a = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) a += p[i] * p[i];
    return dwc_block_sum_256(a, sm);
}

__device__ __forceinline__ int sn_find(const dwc_sn_desc* d, int L, int blk, bool rows) {
    int l = 0;
    for (int j = 1; j < L; ++j)
        if ((rows ? d[j].row_blk0 : d[j].col_blk0) <= blk) l = j;
    return l;
}

// t_s = W_bar^T u_{s-1} over blocks of SN_COLS columns.  256 threads = column lanes x row groups; a lane owns 4 consecutive
// columns (16-byte loads) or 1, row groups take rows rg, rg + RG, ...; the partials meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void sn_col_kernel(const dwc_sn_desc* __restrict__ desc, int L, float* __restrict__ base, int s) {
    __shared__ float u_sm[SN_MAX_COUT];
    __shared__ float part[16 * SN_COLS];
    __shared__ float red[4];
    const dwc_sn_desc d = desc[sn_find(desc, L, blockIdx.x, false)];
    const int col0 = (blockIdx.x - d.col_blk0) * SN_COLS;
    const int cout = d.cout, K = d.k;
    const float* U = base + d.off_u;
    float* V = base + d.off_v;
    if (s == 0) {
        for (int i = threadIdx.x; i < cout; i += 256) u_sm[i] = d.u[i];
    } else {
        const float* w = U + (size_t)(s - 1) * cout;
        const float nrm = sqrtf(sn_sumsq(w, cout, red)) + SN_EPS;
        for (int i = threadIdx.x; i < cout; i += 256) u_sm[i] = w[i] / nrm;
    }
    __syncthreads();
    const float* W = d.w;
    if (d.vec) {                                  // K % 4 == 0 and W_bar 16-byte aligned
        const int cl = threadIdx.x & 15, rg = threadIdx.x >> 4;
        const int c = col0 + 4 * cl;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (c < K) {
            for (int i = rg; i < cout; i += 16) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(W + (size_t)i * K + c);
                const float ui = u_sm[i];
                acc[0] += x[0] * ui; acc[1] += x[1] * ui; acc[2] += x[2] * ui; acc[3] += x[3] * ui;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) part[rg * SN_COLS + 4 * cl + q] = acc[q];
        __syncthreads();
        if (threadIdx.x < SN_COLS && col0 + (int)threadIdx.x < K) {
            float t = 0.f;
            for (int g = 0; g < 16; ++g) t += part[g * SN_COLS + threadIdx.x];
            V[(size_t)s * K + col0 + threadIdx.x] = t;
        }
    } else {
        const int cl = threadIdx.x & 63, rg = threadIdx.x >> 6;
        const int c = col0 + cl;
        float acc = 0.f;
        if (c < K)
            for (int i = rg; i < cout; i += 4) acc += W[(size_t)i * K + c] * u_sm[i];
        part[rg * SN_COLS + cl] = acc;
        __syncthreads();
        if (threadIdx.x < SN_COLS && col0 + (int)threadIdx.x < K) {
            float t = 0.f;
            for (int g = 0; g < 4; ++g) t += part[g * SN_COLS + threadIdx.x];
            V[(size_t)s * K + col0 + threadIdx.x] = t;
        }
    }
}

// w_s = W_bar v_s over blocks of SN_ROWS rows, v_s = t_s / (|t_s| + eps) staged in LDS; one wave per row, lanes stride the row.
__global__ __launch_bounds__(256) void sn_row_kernel(const dwc_sn_desc* __restrict__ desc, int L, float* __restrict__ base, int s) {
    __shared__ float v_sm[SN_MAX_K];
    __shared__ float red[4];
    const dwc_sn_desc d = desc[sn_find(desc, L, blockIdx.x, true)];
    const int cout = d.cout, K = d.k;
    float* U = base + d.off_u;
    const float* t = base + d.off_v + (size_t)s * K;
    const float nrm = sqrtf(sn_sumsq(t, K, red)) + SN_EPS;
    for (int k = threadIdx.x; k < K; k += 256) v_sm[k] = t[k] / nrm;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row0 = (blockIdx.x - d.row_blk0) * SN_ROWS;
    for (int rr = wave; rr < SN_ROWS; rr += 4) {
        const int i = row0 + rr;
        if (i >= cout) break;                                    // (wave-uniform)
        const float* Wr = d.w + (size_t)i * K;
        float a = 0.f;
        if (d.vec) {
            for (int k = 4 * lane; k < K; k += 256) {
                const f32x4 x = *reinterpret_cast<const f32x4*>(Wr + k);
                a += x[0] * v_sm[k] + x[1] * v_sm[k + 1] + x[2] * v_sm[k + 2] + x[3] * v_sm[k + 3];
            }
        } else {
            for (int k = lane; k < K; k += 64) a += Wr[k] * v_sm[k];
        }
        a = dwc_wave_sum(a);
        if (lane == 0) U[(size_t)s * cout + i] = a;
    }
}

// One workgroup per layer: normalise the raw rows in place (u_s, v_s), r_s = 1 / (u_s . w_s), the last pair into the parameters.
// Every thread reads and writes the same elements (index tid + 256 j) throughout, so the in-place rewrite needs no extra barrier.
__global__ __launch_bounds__(256) void sn_finalize_kernel(const dwc_sn_desc* __restrict__ desc, float* __restrict__ base, int S) {
    __shared__ float red[4];
    const dwc_sn_desc d = desc[blockIdx.x];
    const int cout = d.cout, K = d.k;
    float* U = base + d.off_u;
    float* V = base + d.off_v;
    float* R = base + d.off_r;
    for (int s = 0; s < S; ++s) {
        float* w = U + (size_t)s * cout;
        float* t = V + (size_t)s * K;
        const float nw = sqrtf(sn_sumsq(w, cout, red)) + SN_EPS;
        const float nt = sqrtf(sn_sumsq(t, K, red)) + SN_EPS;
        float a = 0.f;
        for (int i = threadIdx.x; i < cout; i += 256) a += (w[i] / nw) * w[i];
        const float sigma = dwc_block_sum_256(a, red);
        for (int i = threadIdx.x; i < cout; i += 256) w[i] = w[i] / nw;
        for (int k = threadIdx.x; k < K; k += 256) t[k] = t[k] / nt;
        if (threadIdx.x == 0) R[s] = 1.f / sigma;
    }
    const float* ul = U + (size_t)(S - 1) * cout;
    const float* vl = V + (size_t)(S - 1) * K;
    for (int i = threadIdx.x; i < cout; i += 256) d.u[i] = ul[i];
    for (int k = threadIdx.x; k < K; k += 256) d.v[k] = vl[k];
}

// ---- segmented epilogues --------------------------------------------------------------------------------------------------------
// Z: [rows, C] (NHWC, C padded to whole vectors), rows = S segments of rows / S; p = Z * r_s + b; y = act(p).
template <typename T>
__global__ __launch_bounds__(256) void sn_epi_fwd_kernel(const T* __restrict__ Z, const float* __restrict__ r, const float* __restrict__ b,
                                                         T* __restrict__ y, size_t nvec, int cq, size_t rows_per_seg, int act,
                                                         unsigned long long* amax, unsigned amax_ep) {
    constexpr int V = VecOf<T>::V;
    unsigned am = 0;
    for (size_t iv = (size_t)blockIdx.x * 256 + threadIdx.x; iv < nvec; iv += (size_t)gridDim.x * 256) {
        const size_t row = iv / cq;
        const int c0 = (int)(iv - row * cq) * V;
        const float rs = r[row / rows_per_seg];
        float o[V], bb[V];
        ldv(Z, iv, o);
        ldf<V>(b, c0, bb);
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = dwc_act_apply(o[k] * rs + bb[k], act, c0 + k);
        stv(y, iv, o);
        am = dwc_amax_fold<V>(am, o);
    }
    dwc_amax_wave_publish(amax, amax_ep, am);
}

// Backward, one pass: g = dy * act'(p), dZ = g * r_s, and per workgroup the partials of db (per channel) and c_s = <g_s, Z_s>.
// Grid (chunks, S): workgroup (chunk, s) takes rows [chunk * rpc, ...) of segment s.  256 threads = cq column lanes x RL = 256 / cq
// row lanes (threads beyond RL * cq idle); the partials meet in LDS in a fixed order.
template <typename T>
__global__ __launch_bounds__(256) void sn_epi_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ Z, const float* __restrict__ r,
                                                         const float* __restrict__ b, T* __restrict__ dZ, float* __restrict__ ws_db,
                                                         float* __restrict__ ws_c, int cq, int rows_per_seg, int rpc, int act,
                                                         unsigned long long* amax, unsigned amax_ep) {
    constexpr int V = VecOf<T>::V;
    __shared__ float sm_db[256 * V];
    __shared__ float sm_c[256];
    const int s = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
    const int RL = 256 / cq;
    const int q = threadIdx.x % cq, rl = threadIdx.x / cq;
    const float rs = r[s];
    float db[V], cacc = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k) db[k] = 0.f;
    unsigned am = 0;
    if (rl < RL) {
        float bb[V];
        ldf<V>(b, (size_t)q * V, bb);
        const int r0 = chunk * rpc, r1 = min(rows_per_seg, r0 + rpc);
        for (int rr = r0 + rl; rr < r1; rr += RL) {
            const size_t iv = ((size_t)s * rows_per_seg + rr) * cq + q;
            float g[V], z[V];
            ldv(dy, iv, g);
            ldv(Z, iv, z);
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const float yv = dwc_act_apply(z[k] * rs + bb[k], act, q * V + k);
                g[k] *= dwc_act_grad(yv, act, q * V + k);
                db[k] += g[k];
                cacc += g[k] * z[k];
                g[k] *= rs;
            }
            stv(dZ, iv, g);
            am = dwc_amax_fold<V>(am, g);
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k) sm_db[threadIdx.x * V + k] = db[k];
    sm_c[threadIdx.x] = cacc;
    __syncthreads();
    const size_t part = (size_t)s * chunks + chunk;
    for (int e = threadIdx.x; e < cq * V; e += 256) {            // channel e = qq * V + k
        const int qq = e / V, k = e - qq * V;
        float a = 0.f;
        for (int l = 0; l < RL; ++l) a += sm_db[(l * cq + qq) * V + k];
        ws_db[part * cq * V + e] = a;
    }
    if (threadIdx.x == 0) {
        float a = 0.f;
        for (int l = 0; l < RL * cq; ++l) a += sm_c[l];
        ws_c[part] = a;
    }
    dwc_amax_wave_publish(amax, amax_ep, am);
}

// db[c] = sum of the S * chunks partial rows (fixed order); c[s] = sum of segment s's chunk partials.  One workgroup.
__global__ __launch_bounds__(256) void sn_epi_bwd_final(const float* __restrict__ ws_db, const float* __restrict__ ws_c, float* __restrict__ db,
                                                        float* __restrict__ c, int C, int S, int chunks) {
    if (db) {
        for (int e = threadIdx.x; e < C; e += 256) {
            float a = 0.f;
            for (int p = 0; p < S * chunks; ++p) a += ws_db[(size_t)p * C + e];
            db[e] = a;
        }
    }
    for (int s = threadIdx.x; s < S; s += 256) {
        float a = 0.f;
        for (int p = 0; p < chunks; ++p) a += ws_c[(size_t)s * chunks + p];
        c[s] = a;
    }
}

// dW[i, k] (+)= -sum_s c_s r_s^2 u_s[i] v_s[k], u_s = U + s * u_stride, v_s = Vv + s * v_stride (stride 0: one pair for every s)
__global__ __launch_bounds__(256) void sn_rank_kernel(const float* __restrict__ U, int u_stride, const float* __restrict__ Vv, int v_stride,
                                                      const float* __restrict__ r, const float* __restrict__ c, float* __restrict__ dw,
                                                      int S, int cout, int K, int accumulate) {
    const size_t n = (size_t)cout * K;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
        const int i = (int)(e / K), k = (int)(e - (size_t)i * K);
        float a = 0.f;
        for (int s = 0; s < S; ++s) a += (c[s] * r[s] * r[s]) * U[(size_t)s * u_stride + i] * Vv[(size_t)s * v_stride + k];
        dw[e] = accumulate ? dw[e] - a : -a;
    }
}

void sn_bwd_plan(int rows_per_seg, int S, int cq, int* chunks, int* rpc) {
    const int RL = 256 / cq;
    int ch = (1024 + S - 1) / S;                                // ~1024 workgroups in all
    const int max_ch = (rows_per_seg + RL - 1) / RL;            // at least one row per row lane
    if (ch > max_ch) ch = max_ch;
    if (ch < 1) ch = 1;
    *rpc = (rows_per_seg + ch - 1) / ch;
    *chunks = (rows_per_seg + *rpc - 1) / *rpc;
}

template <typename T>
int sn_fwd_t(const T* Z, const float* r, const float* b, T* y, int rows, int C, int S, int act, unsigned long long* amax, unsigned ep,
             void* stream) {
    constexpr int V = VecOf<T>::V;
    if (rows <= 0 || C <= 0 || (C % V) || S <= 0 || (rows % S) || !Z || !r || !b || !y) return DWC_EINVAL;
    if (act < DWC_ACT_NONE || act > DWC_ACT_SIGMOID) return DWC_EINVAL;
    const size_t nvec = (size_t)rows * (C / V);
    const size_t grid = std::min<size_t>((nvec + 255) / 256, 4096);
    hipLaunchKernelGGL(sn_epi_fwd_kernel<T>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, Z, r, b, y, nvec, C / V,
                       (size_t)(rows / S), act, amax, ep);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

template <typename T>
int sn_bwd_t(const T* dy, const T* Z, const float* r, const float* b, T* dZ, float* db, float* c, int rows, int C, int S, int act,
             void* ws, size_t ws_bytes, unsigned long long* amax, unsigned ep, void* stream) {
    constexpr int V = VecOf<T>::V;
    if (rows <= 0 || C <= 0 || (C % V) || S <= 0 || (rows % S) || C / V > 256 || !dy || !Z || !r || !b || !dZ || !c) return DWC_EINVAL;
    if (act < DWC_ACT_NONE || act > DWC_ACT_SIGMOID) return DWC_EINVAL;
    if (!ws || ws_bytes < dwc_sn_epilogue_bwd_ws_bytes(rows, C, S, V)) return DWC_EWORKSPACE;
    const int cq = C / V, rps = rows / S;
    int chunks, rpc;
    sn_bwd_plan(rps, S, cq, &chunks, &rpc);
    float* ws_db = (float*)ws;
    float* ws_c = ws_db + (size_t)S * chunks * C;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(sn_epi_bwd_kernel<T>, dim3(chunks, S), dim3(256), 0, st, dy, Z, r, b, dZ, ws_db, ws_c, cq, rps, rpc, act, amax, ep);
    DWC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sn_epi_bwd_final, dim3(1), dim3(256), 0, st, (const float*)ws_db, (const float*)ws_c, db, c, C, S, chunks);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

}  // namespace

extern "C" {

size_t dwc_sn_layer_saved_floats(int S, int cout, int k) {
    if (S <= 0 || cout <= 0 || k <= 0) return 0;
    auto up4 = [](size_t n) { return (n + 3) / 4 * 4; };
    return up4((size_t)S * cout) + up4((size_t)S * k) + up4((size_t)S);
}

int dwc_sn_power_blocks(int cout, int k, int* col_blocks, int* row_blocks) {
    if (cout <= 0 || k <= 0 || cout > SN_MAX_COUT || k > SN_MAX_K || !col_blocks || !row_blocks) return DWC_EINVAL;
    *col_blocks = (k + SN_COLS - 1) / SN_COLS;
    *row_blocks = (cout + SN_ROWS - 1) / SN_ROWS;
    return DWC_OK;
}

int dwc_sn_power_iteration(const dwc_sn_desc* desc, int L, int col_blocks, int row_blocks, float* base, int S, void* stream) {
    if (!desc || !base || L <= 0 || S <= 0 || col_blocks <= 0 || row_blocks <= 0) return DWC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    for (int s = 0; s < S; ++s) {
        hipLaunchKernelGGL(sn_col_kernel, dim3(col_blocks), dim3(256), 0, st, desc, L, base, s);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(sn_row_kernel, dim3(row_blocks), dim3(256), 0, st, desc, L, base, s);
        DWC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sn_finalize_kernel, dim3(L), dim3(256), 0, st, desc, base, S);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

size_t dwc_sn_epilogue_bwd_ws_bytes(int rows, int C, int S, int vec) {
    if (rows <= 0 || C <= 0 || S <= 0 || vec <= 0 || (C % vec) || C / vec > 256 || (rows % S)) return 0;
    int chunks, rpc;
    sn_bwd_plan(rows / S, S, C / vec, &chunks, &rpc);
    return ((size_t)S * chunks * C + (size_t)S * chunks) * sizeof(float);
}

int dwc_sn_epilogue_fwd(const float* Z, const float* r, const float* b, float* y, int rows, int C, int S, int act, void* y_amax,
                        unsigned y_epoch, void* stream) {
    return sn_fwd_t<float>(Z, r, b, y, rows, C, S, act, (unsigned long long*)y_amax, y_epoch, stream);
}
int dwc_bf16_sn_epilogue_fwd(const void* Z, const float* r, const float* b, void* y, int rows, int C, int S, int act, void* stream) {
    return sn_fwd_t<dwc_bf16>((const dwc_bf16*)Z, r, b, (dwc_bf16*)y, rows, C, S, act, nullptr, 0, stream);
}
int dwc_sn_epilogue_bwd(const float* dy, const float* Z, const float* r, const float* b, float* dZ, float* db, float* c, int rows, int C,
                        int S, int act, void* ws, size_t ws_bytes, void* dz_amax, unsigned dz_epoch, void* stream) {
    return sn_bwd_t<float>(dy, Z, r, b, dZ, db, c, rows, C, S, act, ws, ws_bytes, (unsigned long long*)dz_amax, dz_epoch, stream);
}
int dwc_bf16_sn_epilogue_bwd(const void* dy, const void* Z, const float* r, const float* b, void* dZ, float* db, float* c, int rows,
                             int C, int S, int act, void* ws, size_t ws_bytes, void* stream) {
    return sn_bwd_t<dwc_bf16>((const dwc_bf16*)dy, (const dwc_bf16*)Z, r, b, (dwc_bf16*)dZ, db, c, rows, C, S, act, ws, ws_bytes,
                              nullptr, 0, stream);
}

int dwc_sn_weight_grad(const float* U, int u_stride, const float* V, int v_stride, const float* r, const float* c, float* dw, int S,
                       int cout, int k, int accumulate, void* stream) {
    if (!U || !V || !r || !c || !dw || S <= 0 || cout <= 0 || k <= 0 || u_stride < 0 || v_stride < 0) return DWC_EINVAL;
    const size_t n = (size_t)cout * k;
    const size_t grid = std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(sn_rank_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, U, u_stride, V, v_stride, r, c, dw, S,
                       cout, k, accumulate);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

}  // extern "C"
