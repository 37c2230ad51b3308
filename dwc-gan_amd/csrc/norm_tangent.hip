// Forward-mode derivative ("tangent") of instance norm and MUNIT LayerNorm, and its backward, NHWC fp32 (gfx950).
//
// The gradient / R1 penalties differentiate D twice.  With ghat = dP/dg held constant, dP/dtheta is the gradient of the directional
// derivative of y along ghat, so a normalisation needs one new once-differentiable op: the tangent of its output
// for a tangent zd of its input z.  Per normalisation group (IN: one (n, c), M = HW; LN: one sample, M = C * HW):
//
//     c = z - mean z,  xh = r c,  cd = zd - mean zd,  A = <xh, cd>
//     IN: r = (var_biased + eps)^-1/2,  lam = r / M,  rho = 1
//     LN: s = unbiased std,  r = 1 / (s + eps),  lam = 1 / ((M - 1) s),  rho = (s + eps) / s     (s = 0: lam = rho = 0)
//     forward    out = gamma_c (r cd - lam A xh)                                       (IN: no gamma)
//     backward   u = gamma_c dout,  ub = mean u,  U = <u, xh>,  Cu = <u, cd>
//                dzd = r (u - ub) - lam U xh                                           (the ordinary norm backward)
//                dz  = -lam r [Cu xh + U cd + A (u - ub)] + (2 + rho) lam^2 A U xh
//                dgamma_c = sum over samples and pixels of dout (r cd - lam A xh)      (LN only)
//
// Pass structure, as csrc/norm.hip: HBM-bound, 16-byte accesses, channels on the lanes, a 256-thread block = row groups x column
// groups of 4 channels.  Each direction is a statistics pass (per-chunk, per-channel partial sums to caller scratch), a small
// closing launch that combines the partials in a fixed order (no atomics: bitwise reproducible) and an apply pass.  The sums are
// taken about a pivot (the group's first element of z and of zd), so that sum z zd - M mean z mean zd does not cancel; the closing
// launches combine in double.  Both group kinds share the row-walking kernels: layer norm only takes ONE pivot per sample, and its
// closing launch adds the channels up as well.  (The row geometry repeats plan_rows / plan_apply / RowGeom of csrc/norm.hip, which
// keeps them in its own anonymous namespace: that file's code generation is pinned by its register report and stays untouched.)
#include "dwc_common.h"

namespace {

constexpr int V = 4;                 // fp32 channels per 16-byte access
constexpr int NT_STATS = 6;          // planes of `stats`: mean z, r, mean zd, A, lam, rho
constexpr int NT_COEF = 5;           // planes of the backward's per-group coefficients: ub, lam U, and the factors of xh, cd, u - ub in dz

struct RowSplit {
    int chunks, rows_per_chunk;
};

// statistics passes: one partial per (sample, chunk, channel)
RowSplit nt_plan_rows(int B, int HW) {
    int chunks = HW / 64;
    int cap = 2048 / (B > 0 ? B : 1);
    if (cap < 1) cap = 1;
    if (chunks > cap) chunks = cap;
    if (chunks < 1) chunks = 1;
    RowSplit r;
    r.rows_per_chunk = (HW + chunks - 1) / chunks;
    r.chunks = (HW + r.rows_per_chunk - 1) / r.rows_per_chunk;
    return r;
}

// apply passes: no partials, so they split finer (up to 32 rows per thread, at least ~4 blocks per CU)
RowSplit nt_plan_apply(int B, int HW, int C) {
    const int cq = C / V > 0 ? C / V : 1;
    const int groups = 256 / cq > 0 ? 256 / cq : 1;
    int rpc = groups * 32;
    while (rpc > groups * 4 && (long)B * ((HW + rpc - 1) / rpc) < 1024) rpc /= 2;
    while ((long)B * ((HW + rpc - 1) / rpc) > 16384 && rpc < HW) rpc *= 2;
    RowSplit r;
    r.rows_per_chunk = rpc < HW ? rpc : HW;
    r.chunks = (HW + r.rows_per_chunk - 1) / r.rows_per_chunk;
    return r;
}

// thread (rg, col) takes rows r0 + rg, r0 + rg + groups, ... of its column group; groups * cq == 256 (C a power of two, 4 .. 1024)
struct RowGeom {
    int cq, groups, col, rg;
    __device__ __forceinline__ explicit RowGeom(int C) : cq(C / V), groups(256 / cq), col(threadIdx.x % cq), rg(threadIdx.x / cq) {}
};

// Caller scratch in floats: [4 planes of per-(sample, chunk, channel) partials][NT_COEF planes of per-group coefficients][16 spare]
struct TangentScratch {
    RowSplit rs;
    size_t plane, coef, bytes;
    TangentScratch(int B, int HW, int C)
        : rs(nt_plan_rows(B, HW)), plane((size_t)B * rs.chunks * C), coef(4 * plane),
          bytes((coef + (size_t)NT_COEF * B * C + 16) * sizeof(float)) {}
};

bool nt_shape_ok(int kind, int B, int HW, int C) {
    if (kind != DWC_NORM_TANGENT_IN && kind != DWC_NORM_TANGENT_LN) return false;
    if (B <= 0 || B > 65535 || HW <= 0) return false;
    if (dwc_ilog2_exact(C) < 2 || C > 1024) return false;                       // C / 4 column groups must divide the 256 threads
    if ((size_t)B * HW * C >= ((size_t)1 << 31) * V) return false;              // row indices stay inside 32 bits of 16-byte units
    return kind == DWC_NORM_TANGENT_IN || (size_t)HW * C >= 2;                  // the unbiased std needs two values
}

// s[j][k] of the thread with rg == 0 += those of the other row groups of its column, in group order (fixed order)
template <int N>
__device__ __forceinline__ void nt_colsum(float (&s)[N][V], float* sm, const RowGeom& geo) {
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) sm[(j * 256 + threadIdx.x) * V + k] = s[j][k];
    __syncthreads();
    if (geo.rg == 0) {
        for (int g = 1; g < geo.groups; ++g) {
#pragma unroll
            for (int j = 0; j < N; ++j)
#pragma unroll
                for (int k = 0; k < V; ++k) s[j][k] += sm[(j * 256 + g * geo.cq + geo.col) * V + k];
        }
    }
}

// The front of the instance-norm closing kernels (grid (ceil(C / 64), B), 256 threads = 64 channels x 4 chunk lanes): the sums over
// the chunks of the N partial planes of (sample blockIdx.y, channel c); lane q takes chunks q, q + 4, ..., the four lane sums are
// added in lane order.  True for the one thread of the channel that holds them.
template <int N>
__device__ __forceinline__ bool nt_chunk_sums(const float* __restrict__ part, size_t plane, int C, int chunks, int& c, float (&s)[N]) {
    __shared__ float sm[N][4][64];
    const int n = blockIdx.y, cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    c = blockIdx.x * 64 + cl;
    float a[N];
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = 0.f;
    if (c < C) {
        for (int k = q; k < chunks; k += 4) {
            const size_t i = ((size_t)n * chunks + k) * C + c;
#pragma unroll
            for (int j = 0; j < N; ++j) a[j] += part[j * plane + i];
        }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) sm[j][q][cl] = a[j];
    __syncthreads();
    if (q != 0 || c >= C) return false;
#pragma unroll
    for (int j = 0; j < N; ++j) s[j] = ((sm[j][0][cl] + sm[j][1][cl]) + sm[j][2][cl]) + sm[j][3][cl];
    return true;
}

// sum of a[j] over the 256 threads of the block in a fixed tree; valid in thread 0
template <int N>
__device__ __forceinline__ void nt_block_sum_double(double (&a)[N], double (*sm)[256]) {
#pragma unroll
    for (int j = 0; j < N; ++j) sm[j][threadIdx.x] = a[j];
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
#pragma unroll
            for (int j = 0; j < N; ++j) sm[j][threadIdx.x] += sm[j][threadIdx.x + off];
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < N; ++j) a[j] = sm[j][0];
}

// the V per-channel values of plane j of a per-group table (IN: [B * C], LN: [B], broadcast)
template <bool LN>
__device__ __forceinline__ void nt_group_vals(const float* __restrict__ tab, size_t G, int j, int n, int C, int col, float (&o)[V]) {
    if constexpr (LN) {
        const float v = tab[(size_t)j * G + n];
#pragma unroll
        for (int k = 0; k < V; ++k) o[k] = v;
    } else {
        ldf<V>(tab + (size_t)j * G, (size_t)n * C + col * V, o);
    }
}

// ---------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------
// partial planes: sum a, sum a^2, sum b, sum a b with a = z - pivot_z, b = zd - pivot_zd
template <bool LN>
__global__ __launch_bounds__(256) void nt_fwd_partial(const float* __restrict__ z, const float* __restrict__ zd, float* __restrict__ part,
                                                      int HW, int C, int rows_per_chunk, size_t plane) {
    __shared__ float sm[4 * 256 * V];
    const RowGeom geo(C);
    const int cq = geo.cq, groups = geo.groups, col = geo.col, rg = geo.rg;
    const int n = blockIdx.y, chunk = blockIdx.x;
    const float* zs = z + (size_t)n * HW * C;
    const float* ds = zd + (size_t)n * HW * C;
    float pz[V], pd[V];
    if constexpr (LN) {
#pragma unroll
        for (int k = 0; k < V; ++k) pz[k] = zs[0], pd[k] = ds[0];
    } else {
        ldv(zs, col, pz);
        ldv(ds, col, pd);
    }
    const int r0 = chunk * rows_per_chunk;
    const int r1 = min(HW, r0 + rows_per_chunk);
    float s[4][V];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) s[j][k] = 0.f;
    auto acc = [&](const float (&zv)[V], const float (&dv)[V]) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float a = zv[k] - pz[k], b = dv[k] - pd[k];
            s[0][k] += a;
            s[1][k] += a * a;
            s[2][k] += b;
            s[3][k] += a * b;
        }
    };
    if (rg < groups) {
        int r = r0 + rg;
        for (; r + groups < r1; r += 2 * groups) {               // two rows of both tensors in flight per thread
            const size_t i0 = (size_t)r * cq + col, i1 = i0 + (size_t)groups * cq;
            float z0[V], z1[V], d0[V], d1[V];
            ldv(zs, i0, z0);
            ldv(zs, i1, z1);
            ldv(ds, i0, d0);
            ldv(ds, i1, d1);
            acc(z0, d0);
            acc(z1, d1);
        }
        for (; r < r1; r += groups) {
            float z0[V], d0[V];
            ldv(zs, (size_t)r * cq + col, z0);
            ldv(ds, (size_t)r * cq + col, d0);
            acc(z0, d0);
        }
    }
    nt_colsum<4>(s, sm, geo);
    if (rg == 0) {
        const size_t o = ((size_t)n * gridDim.x + chunk) * C + col * V;
#pragma unroll
        for (int j = 0; j < 4; ++j) stf<V>(part + j * plane, o, s[j]);
    }
}

// the six statistics of one group from its four sums about the pivots (pz, pd), M values
__device__ __forceinline__ void nt_write_stats(float* __restrict__ stats, size_t G, size_t g, bool ln, double M, double pz, double pd, double s0,
                                               double s1, double s2, double s3, double eps) {
    const double d = s0 / M, dd = s2 / M;
    const double cc = s3 - s0 * dd;                          // sum c cd
    double r, lam, rho;
    if (ln) {
        double var = (s1 - s0 * d) / (M - 1.0);              // unbiased, as torch.std
        if (var < 0) var = 0;
        const double sd = sqrt(var);
        r = 1.0 / (sd + eps);
        lam = sd > 0 ? 1.0 / ((M - 1.0) * sd) : 0.0;
        rho = sd > 0 ? (sd + eps) / sd : 0.0;
    } else {
        double var = s1 / M - d * d;
        if (var < 0) var = 0;
        r = 1.0 / sqrt(var + eps);
        lam = r / M;
        rho = 1.0;
    }
    stats[g] = (float)(pz + d);
    stats[G + g] = (float)r;
    stats[2 * G + g] = (float)(pd + dd);
    stats[3 * G + g] = (float)(r * cc);
    stats[4 * G + g] = (float)lam;
    stats[5 * G + g] = (float)rho;
}

__global__ __launch_bounds__(256) void nt_fwd_final_in(const float* __restrict__ z, const float* __restrict__ zd, const float* __restrict__ part,
                                                       float* __restrict__ stats, int B, int HW, int C, int chunks, size_t plane, float eps) {
    int c;
    float s[4];
    if (!nt_chunk_sums<4>(part, plane, C, chunks, c, s)) return;
    const int n = blockIdx.y;
    const size_t first = (size_t)n * HW * C + c;
    nt_write_stats(stats, (size_t)B * C, (size_t)n * C + c, false, (double)HW, z[first], zd[first], s[0], s[1], s[2], s[3], eps);
}

// grid B: thread t adds entries t, t + 256, ... of the sample's chunks x C partials, then the block tree
__global__ __launch_bounds__(256) void nt_fwd_final_ln(const float* __restrict__ z, const float* __restrict__ zd, const float* __restrict__ part,
                                                       float* __restrict__ stats, int B, int HW, int C, int chunks, size_t plane, float eps) {
    __shared__ double sm[4][256];
    const int n = blockIdx.x;
    const size_t count = (size_t)chunks * C, base = (size_t)n * count;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t i = threadIdx.x; i < count; i += 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] += (double)part[j * plane + base + i];
    }
    nt_block_sum_double<4>(a, sm);
    if (threadIdx.x == 0) {
        const size_t first = (size_t)n * HW * C;
        nt_write_stats(stats, (size_t)B, (size_t)n, true, (double)HW * C, z[first], zd[first], a[0], a[1], a[2], a[3], eps);
    }
}

template <bool LN>
__global__ __launch_bounds__(256) void nt_fwd_apply(const float* __restrict__ z, const float* __restrict__ zd, const float* __restrict__ gamma,
                                                    const float* __restrict__ stats, float* __restrict__ out, int HW, int C, size_t G,
                                                    int rows_per_chunk) {
    const RowGeom geo(C);
    const int cq = geo.cq, groups = geo.groups, col = geo.col, rg = geo.rg;
    const int n = blockIdx.y;
    float mu[V], rs[V], md[V], kx[V], lam[V], ga[V];
    nt_group_vals<LN>(stats, G, 0, n, C, col, mu);
    nt_group_vals<LN>(stats, G, 1, n, C, col, rs);
    nt_group_vals<LN>(stats, G, 2, n, C, col, md);
    nt_group_vals<LN>(stats, G, 3, n, C, col, kx);
    nt_group_vals<LN>(stats, G, 4, n, C, col, lam);
#pragma unroll
    for (int k = 0; k < V; ++k) kx[k] *= lam[k], ga[k] = 1.f;
    if (gamma) ldf<V>(gamma, (size_t)col * V, ga);
    const size_t base = (size_t)n * HW * cq + col;
    const int r0 = blockIdx.x * rows_per_chunk;
    const int r1 = rg < groups ? min(HW, r0 + rows_per_chunk) : r0;
    auto one = [&](const float (&zv)[V], const float (&dv)[V], float (&o)[V]) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float xh = (zv[k] - mu[k]) * rs[k];
            o[k] = ga[k] * (rs[k] * (dv[k] - md[k]) - kx[k] * xh);
        }
    };
    int r = r0 + rg;
    for (; r + groups < r1; r += 2 * groups) {
        const size_t i0 = base + (size_t)r * cq, i1 = i0 + (size_t)groups * cq;
        float z0[V], z1[V], d0[V], d1[V], o0[V], o1[V];
        ldv(z, i0, z0);
        ldv(z, i1, z1);
        ldv(zd, i0, d0);
        ldv(zd, i1, d1);
        one(z0, d0, o0);
        one(z1, d1, o1);
        stv(out, i0, o0);
        stv(out, i1, o1);
    }
    for (; r < r1; r += groups) {
        const size_t i0 = base + (size_t)r * cq;
        float z0[V], d0[V], o0[V];
        ldv(z, i0, z0);
        ldv(zd, i0, d0);
        one(z0, d0, o0);
        stv(out, i0, o0);
    }
}

// ---------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------
// partial planes (of the upstream gradient WITHOUT gamma: dgamma needs them per channel): sum dout, sum dout xh, sum dout cd
template <bool LN>
__global__ __launch_bounds__(256) void nt_bwd_partial(const float* __restrict__ dout, const float* __restrict__ z, const float* __restrict__ zd,
                                                      const float* __restrict__ stats, float* __restrict__ part, int HW, int C, size_t G,
                                                      int rows_per_chunk, size_t plane) {
    __shared__ float sm[3 * 256 * V];
    const RowGeom geo(C);
    const int cq = geo.cq, groups = geo.groups, col = geo.col, rg = geo.rg;
    const int n = blockIdx.y, chunk = blockIdx.x;
    float mu[V], rs[V], md[V];
    nt_group_vals<LN>(stats, G, 0, n, C, col, mu);
    nt_group_vals<LN>(stats, G, 1, n, C, col, rs);
    nt_group_vals<LN>(stats, G, 2, n, C, col, md);
    const size_t base = (size_t)n * HW * cq + col;
    const int r0 = chunk * rows_per_chunk;
    const int r1 = min(HW, r0 + rows_per_chunk);
    float s[3][V];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < V; ++k) s[j][k] = 0.f;
    auto acc = [&](const float (&gv)[V], const float (&zv)[V], const float (&dv)[V]) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            s[0][k] += gv[k];
            s[1][k] += gv[k] * ((zv[k] - mu[k]) * rs[k]);
            s[2][k] += gv[k] * (dv[k] - md[k]);
        }
    };
    if (rg < groups) {
        int r = r0 + rg;
        for (; r + groups < r1; r += 2 * groups) {               // two rows of the three tensors in flight per thread
            const size_t i0 = base + (size_t)r * cq, i1 = i0 + (size_t)groups * cq;
            float g0[V], g1[V], z0[V], z1[V], d0[V], d1[V];
            ldv(dout, i0, g0);
            ldv(dout, i1, g1);
            ldv(z, i0, z0);
            ldv(z, i1, z1);
            ldv(zd, i0, d0);
            ldv(zd, i1, d1);
            acc(g0, z0, d0);
            acc(g1, z1, d1);
        }
        for (; r < r1; r += groups) {
            const size_t i0 = base + (size_t)r * cq;
            float g0[V], z0[V], d0[V];
            ldv(dout, i0, g0);
            ldv(z, i0, z0);
            ldv(zd, i0, d0);
            acc(g0, z0, d0);
        }
    }
    nt_colsum<3>(s, sm, geo);
    if (rg == 0) {
        const size_t o = ((size_t)n * gridDim.x + chunk) * C + col * V;
#pragma unroll
        for (int j = 0; j < 3; ++j) stf<V>(part + j * plane, o, s[j]);
    }
}

// the five coefficients of one group from su = sum u, U = <u, xh>, Cu = <u, cd>
__device__ __forceinline__ void nt_write_coef(float* __restrict__ coef, const float* __restrict__ stats, size_t G, size_t g, double M, double su,
                                              double U, double Cu) {
    const double r = stats[G + g], A = stats[3 * G + g], lam = stats[4 * G + g], rho = stats[5 * G + g];
    coef[g] = (float)(su / M);
    coef[G + g] = (float)(lam * U);
    coef[2 * G + g] = (float)(-lam * r * Cu + (2.0 + rho) * lam * lam * A * U);
    coef[3 * G + g] = (float)(-lam * r * U);
    coef[4 * G + g] = (float)(-lam * r * A);
}

__global__ __launch_bounds__(256) void nt_bwd_final_in(const float* __restrict__ part, const float* __restrict__ stats, float* __restrict__ coef,
                                                       int B, int HW, int C, int chunks, size_t plane) {
    int c;
    float s[3];
    if (!nt_chunk_sums<3>(part, plane, C, chunks, c, s)) return;
    nt_write_coef(coef, stats, (size_t)B * C, (size_t)blockIdx.y * C + c, (double)HW, s[0], s[1], s[2]);
}

// blocks [0, B): the sample's sums with gamma, over chunks and channels -> coefficients;
// blocks [B, B + ceil(C / 64)) (only with dgamma): dgamma[c] = sum over (sample, chunk) of r_n <dout, cd> - lam_n A_n <dout, xh>,
// 64 channels x 4 lanes, lane q takes the (sample, chunk) pairs q, q + 4, ..., lane sums added in lane order
__global__ __launch_bounds__(256) void nt_bwd_final_ln(const float* __restrict__ part, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, float* __restrict__ coef, float* __restrict__ dgamma,
                                                       int B, int HW, int C, int chunks, size_t plane) {
    __shared__ double sm[3][256];
    if ((int)blockIdx.x < B) {
        const int n = blockIdx.x;
        const size_t count = (size_t)chunks * C, base = (size_t)n * count;
        double a[3] = {0.0, 0.0, 0.0};
        for (size_t i = threadIdx.x; i < count; i += 256) {
            const double ga = gamma ? (double)gamma[i % C] : 1.0;
#pragma unroll
            for (int j = 0; j < 3; ++j) a[j] += ga * (double)part[j * plane + base + i];
        }
        nt_block_sum_double<3>(a, sm);
        if (threadIdx.x == 0) nt_write_coef(coef, stats, (size_t)B, (size_t)n, (double)HW * C, a[0], a[1], a[2]);
        return;
    }
    const int cl = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int c = ((int)blockIdx.x - B) * 64 + cl;
    double a = 0.0;
    if (c < C) {
        for (int m = q; m < B * chunks; m += 4) {
            const int n = m / chunks;
            const double r = stats[(size_t)B + n], kx = (double)stats[(size_t)4 * B + n] * (double)stats[(size_t)3 * B + n];
            a += r * (double)part[2 * plane + (size_t)m * C + c] - kx * (double)part[plane + (size_t)m * C + c];
        }
    }
    sm[0][threadIdx.x] = a;
    __syncthreads();
    if (q == 0 && c < C) dgamma[c] = (float)(((sm[0][cl] + sm[0][64 + cl]) + sm[0][128 + cl]) + sm[0][192 + cl]);
}

template <bool LN>
__global__ __launch_bounds__(256) void nt_bwd_apply(const float* __restrict__ dout, const float* __restrict__ z, const float* __restrict__ zd,
                                                    const float* __restrict__ gamma, const float* __restrict__ stats,
                                                    const float* __restrict__ coef, float* __restrict__ dz, float* __restrict__ dzd, int HW, int C,
                                                    size_t G, int rows_per_chunk) {
    const RowGeom geo(C);
    const int cq = geo.cq, groups = geo.groups, col = geo.col, rg = geo.rg;
    const int n = blockIdx.y;
    float mu[V], rs[V], md[V], ub[V], k1[V], k2[V], k3[V], k4[V], ga[V];
    nt_group_vals<LN>(stats, G, 0, n, C, col, mu);
    nt_group_vals<LN>(stats, G, 1, n, C, col, rs);
    nt_group_vals<LN>(stats, G, 2, n, C, col, md);
    nt_group_vals<LN>(coef, G, 0, n, C, col, ub);
    nt_group_vals<LN>(coef, G, 1, n, C, col, k1);
    nt_group_vals<LN>(coef, G, 2, n, C, col, k2);
    nt_group_vals<LN>(coef, G, 3, n, C, col, k3);
    nt_group_vals<LN>(coef, G, 4, n, C, col, k4);
#pragma unroll
    for (int k = 0; k < V; ++k) ga[k] = 1.f;
    if (gamma) ldf<V>(gamma, (size_t)col * V, ga);
    const size_t base = (size_t)n * HW * cq + col;
    const int r0 = blockIdx.x * rows_per_chunk;
    const int r1 = rg < groups ? min(HW, r0 + rows_per_chunk) : r0;
    auto one = [&](const float (&gv)[V], const float (&zv)[V], const float (&dv)[V], float (&oz)[V], float (&od)[V]) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const float xh = (zv[k] - mu[k]) * rs[k];
            const float cd = dv[k] - md[k];
            const float uc = ga[k] * gv[k] - ub[k];
            od[k] = rs[k] * uc - k1[k] * xh;
            oz[k] = k2[k] * xh + k3[k] * cd + k4[k] * uc;
        }
    };
    int r = r0 + rg;
    for (; r + groups < r1; r += 2 * groups) {                   // two rows of the three tensors in flight per thread
        const size_t i0 = base + (size_t)r * cq, i1 = i0 + (size_t)groups * cq;
        float g0[V], g1[V], z0[V], z1[V], d0[V], d1[V], oz0[V], oz1[V], od0[V], od1[V];
        ldv(dout, i0, g0);
        ldv(dout, i1, g1);
        ldv(z, i0, z0);
        ldv(z, i1, z1);
        ldv(zd, i0, d0);
        ldv(zd, i1, d1);
        one(g0, z0, d0, oz0, od0);
        one(g1, z1, d1, oz1, od1);
        stv(dz, i0, oz0);
        stv(dz, i1, oz1);
        stv(dzd, i0, od0);
        stv(dzd, i1, od1);
    }
    for (; r < r1; r += groups) {
        const size_t i0 = base + (size_t)r * cq;
        float g0[V], z0[V], d0[V], oz0[V], od0[V];
        ldv(dout, i0, g0);
        ldv(z, i0, z0);
        ldv(zd, i0, d0);
        one(g0, z0, d0, oz0, od0);
        stv(dz, i0, oz0);
        stv(dzd, i0, od0);
    }
}

}  // namespace

extern "C" {

size_t dwc_norm_tangent_ws_bytes(int kind, int B, int HW, int C) {
    return nt_shape_ok(kind, B, HW, C) ? TangentScratch(B, HW, C).bytes : 0;
}

size_t dwc_norm_tangent_stats_elems(int kind, int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    return (size_t)NT_STATS * (kind == DWC_NORM_TANGENT_LN ? (size_t)B : (size_t)B * C);
}

int dwc_norm_tangent_fwd(const float* z, const float* zdot, const float* gamma, float* out, float* stats, int kind, int B, int HW, int C,
                         float eps, void* ws, size_t ws_bytes, void* stream) {
    if (!nt_shape_ok(kind, B, HW, C) || !z || !zdot || !out || !stats) return DWC_EINVAL;
    const bool ln = kind == DWC_NORM_TANGENT_LN;
    if (!ln && gamma) return DWC_EINVAL;                      // plain instance norm: no affine parameters
    const TangentScratch sc(B, HW, C);
    if (!ws || ws_bytes < sc.bytes) return DWC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    const dim3 gp(sc.rs.chunks, B);
    const RowSplit ra = nt_plan_apply(B, HW, C);
    const dim3 ga(ra.chunks, B);
    const size_t G = ln ? (size_t)B : (size_t)B * C;
    if (ln) {
        hipLaunchKernelGGL(nt_fwd_partial<true>, gp, dim3(256), 0, st, z, zdot, part, HW, C, sc.rs.rows_per_chunk, sc.plane);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_fwd_final_ln, dim3(B), dim3(256), 0, st, z, zdot, part, stats, B, HW, C, sc.rs.chunks, sc.plane, eps);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_fwd_apply<true>, ga, dim3(256), 0, st, z, zdot, gamma, stats, out, HW, C, G, ra.rows_per_chunk);
    } else {
        hipLaunchKernelGGL(nt_fwd_partial<false>, gp, dim3(256), 0, st, z, zdot, part, HW, C, sc.rs.rows_per_chunk, sc.plane);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_fwd_final_in, dim3((C + 63) / 64, B), dim3(256), 0, st, z, zdot, part, stats, B, HW, C, sc.rs.chunks, sc.plane,
                           eps);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_fwd_apply<false>, ga, dim3(256), 0, st, z, zdot, gamma, stats, out, HW, C, G, ra.rows_per_chunk);
    }
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_norm_tangent_bwd(const float* dout, const float* z, const float* zdot, const float* gamma, const float* stats, float* dz,
                         float* dzdot, float* dgamma, int kind, int B, int HW, int C, void* ws, size_t ws_bytes, void* stream) {
    if (!nt_shape_ok(kind, B, HW, C) || !dout || !z || !zdot || !stats || !dz || !dzdot) return DWC_EINVAL;
    const bool ln = kind == DWC_NORM_TANGENT_LN;
    if (!ln && (gamma || dgamma)) return DWC_EINVAL;
    const TangentScratch sc(B, HW, C);
    if (!ws || ws_bytes < sc.bytes) return DWC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    float* coef = part + sc.coef;
    const dim3 gp(sc.rs.chunks, B);
    const RowSplit ra = nt_plan_apply(B, HW, C);
    const dim3 ga(ra.chunks, B);
    const size_t G = ln ? (size_t)B : (size_t)B * C;
    if (ln) {
        hipLaunchKernelGGL(nt_bwd_partial<true>, gp, dim3(256), 0, st, dout, z, zdot, stats, part, HW, C, G, sc.rs.rows_per_chunk, sc.plane);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_bwd_final_ln, dim3(B + (dgamma ? (C + 63) / 64 : 0)), dim3(256), 0, st, part, stats, gamma, coef, dgamma, B, HW,
                           C, sc.rs.chunks, sc.plane);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_bwd_apply<true>, ga, dim3(256), 0, st, dout, z, zdot, gamma, stats, coef, dz, dzdot, HW, C, G,
                           ra.rows_per_chunk);
    } else {
        hipLaunchKernelGGL(nt_bwd_partial<false>, gp, dim3(256), 0, st, dout, z, zdot, stats, part, HW, C, G, sc.rs.rows_per_chunk, sc.plane);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_bwd_final_in, dim3((C + 63) / 64, B), dim3(256), 0, st, part, stats, coef, B, HW, C, sc.rs.chunks, sc.plane);
        DWC_LAUNCH_CHECK();
        hipLaunchKernelGGL(nt_bwd_apply<false>, ga, dim3(256), 0, st, dout, z, zdot, gamma, stats, coef, dz, dzdot, HW, C, G,
                           ra.rows_per_chunk);
    }
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

}  // extern "C"
