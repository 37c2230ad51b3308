// Data movement of the text encoder around its bi-LSTM layers (networks/networks_v2.py TxtEncoder; reference networks_v2.py:171-254).
//
// What the recurrent kernels (lstm.hip) and the dense products leave over is movement on a few hundred kilobytes: the embedding
// lookup in length-sorted order with its dropout mask and the style columns, the [2,T,B,H] -> [T,B,2H] re-layout between two layers,
// the gather of the final states into the heads' feature row, and the adjoints of all three.  As stock tensor ops that is ~260
// launches of 2-5 us per training iteration; here each is ONE launch, and every output element is written exactly once (the
// gradient tensors included: no zero fill followed by a scatter, no partial gradients added up afterwards).  Nothing here
// re-associates a floating-point sum: the two reductions of the backward (style rows, table rows) stay with the caller.
//
// Index conventions shared by all kernels: j is a sample's position in the length-sorted batch, order[j] its position in the
// caller's batch, unsort the inverse permutation, last[j] = len[j] - 1.
#include "dwc_common.h"

namespace {

// An entry of order / unsort, held inside the batch whatever the caller staged (a bad permutation gives wrong rows, not a stray access).
__device__ __forceinline__ int txt_perm(const int* __restrict__ perm, int k, int B) { return min(max(perm[k], 0), B - 1); }

// (t, j) row of the layer-1 operand: X[t][j] = [ table[token] * mask[t][j] | style[order[j]] ].
// grid t_max * B, 256 threads.  A token outside the table yields a NaN row (torch raises there; nothing is read out of bounds).
__global__ __launch_bounds__(256) void txt_operand_fwd_kernel(const float* __restrict__ table, const long long* __restrict__ tokens,
                                                              const int* __restrict__ order, const float* __restrict__ mask,
                                                              const float* __restrict__ style, float* __restrict__ X, int B,
                                                              int seq_len, int E, int S, int vocab) {
    const int row = blockIdx.x, t = row / B, j = row - t * B;
    const int src = txt_perm(order, j, B);
    const long long tok = tokens[(size_t)src * seq_len + t];
    const bool ok = tok >= 0 && tok < vocab;
    const float* e = table + (size_t)(ok ? tok : 0) * E;
    const float* m = mask ? mask + (size_t)row * E : nullptr;
    float* x = X + (size_t)row * (E + S);
    for (int k = threadIdx.x; k < E; k += 256) {
        const float v = m ? e[k] * m[k] : e[k];
        x[k] = ok ? v : __builtin_nanf("");
    }
    const float* s = style + (size_t)src * S;
    for (int k = threadIdx.x; k < S; k += 256) x[E + k] = s[k];
}

// Adjoint of the operand, as data movement: dX = dxa (+ dxb: the two directions' input gradients, summed on the fly),
// [t_max][B][E+S], is laid out as the stock expression's own intermediate gradients, so that the two SUMS behind them (the style
// rows over t, the table rows per token id) can be taken by the same reductions on the same values, shapes and strides as without
// these kernels -- a training run keeps its bits.  One block per slot (t, j) of the FULL [seq_len][B] grid; slots with
// t >= t_max (cut off before the first layer) get zeros.
//   d_emb [seq_len][B][E]    dX[t][j][:E] * mask[t][j]: the gradient of the embedded tokens, sorted order
//   idx   [seq_len][B]       the token id of each slot (the index tensor of the lookup), sorted order
//   d_cat [seq_len][B][E+S]  only columns E.. are written: dX[t][j][E:] at row order[j], i.e. the gradient of the expanded style rows
//                            with the pitch of the concatenated operand, already in CALLER order
__global__ __launch_bounds__(256) void txt_operand_bwd_kernel(const float* __restrict__ dxa, const float* __restrict__ dxb,
                                                              const long long* __restrict__ tokens, const int* __restrict__ order,
                                                              const float* __restrict__ mask, float* __restrict__ d_cat,
                                                              float* __restrict__ d_emb, long long* __restrict__ idx, int t_max, int B,
                                                              int seq_len, int E, int S) {
    const int row = blockIdx.x, t = row / B, j = row - t * B, I = E + S;
    const int src = txt_perm(order, j, B);
    const bool live = t < t_max;
    const size_t in = (size_t)row * I;                          // (read only where live: dxa / dxb end at t_max)
    if (d_emb) {
        const float* m = mask ? mask + (size_t)row * E : nullptr;
        for (int k = threadIdx.x; k < E; k += 256) {
            float g = 0.f;
            if (live) {
                g = dxb ? dxa[in + k] + dxb[in + k] : dxa[in + k];
                if (m) g = __fmul_rn(g, m[k]);
            }
            d_emb[(size_t)row * E + k] = g;
        }
    }
    if (d_cat) {
        float* o = d_cat + ((size_t)t * B + src) * I + E;
        for (int k = threadIdx.x; k < S; k += 256) o[k] = live ? (dxb ? dxa[in + E + k] + dxb[in + E + k] : dxa[in + E + k]) : 0.f;
    }
    if (idx && threadIdx.x == 0) idx[row] = tokens[(size_t)src * seq_len + t];
}

// The same operand from the CALLER'S embedded words instead of a table lookup (TxtEncoder.forward_embed): emb is [B][seq_len][E] in
// caller order, lens the sorted lengths.  A slot with t >= lens[j] is a SELECT of 0: what the caller left there is never loaded,
// so neither a NaN nor an Inf behind a sample's length reaches X (and through dw_ih = dG^T X a gradient).  On a table whose padding
// row is zero this is txt_operand_fwd_kernel's output bit for bit.  grid t_max * B, 256 threads.
__global__ __launch_bounds__(256) void txt_operand_embed_fwd_kernel(const float* __restrict__ emb, const int* __restrict__ order,
                                                                    const int* __restrict__ lens, const float* __restrict__ mask,
                                                                    const float* __restrict__ style, float* __restrict__ X, int B,
                                                                    int seq_len, int E, int S) {
    const int row = blockIdx.x, t = row / B, j = row - t * B;
    const int src = txt_perm(order, j, B);
    const bool live = t < lens[j];
    const float* e = emb + ((size_t)src * seq_len + t) * E;
    const float* m = mask ? mask + (size_t)row * E : nullptr;
    float* x = X + (size_t)row * (E + S);
    for (int k = threadIdx.x; k < E; k += 256) {
        float v = 0.f;
        if (live) v = m ? e[k] * m[k] : e[k];
        x[k] = v;
    }
    const float* s = style + (size_t)src * S;
    for (int k = threadIdx.x; k < S; k += 256) x[E + k] = s[k];
}

// Its adjoint.  d_emb is the gradient of the caller's tensor itself, [B][seq_len][E] in CALLER order: block (t, j) owns row
// (order[j], t), so every element is written once -- dX[t][j][:E] * mask where t < min(t_max, lens[j]), +0.0 elsewhere.  d_cat is
// what txt_operand_bwd_kernel writes (the style-row sum stays the caller's reduction).  One block per slot of the FULL
// [seq_len][B] grid, 256 threads.
__global__ __launch_bounds__(256) void txt_operand_embed_bwd_kernel(const float* __restrict__ dxa, const float* __restrict__ dxb,
                                                                    const int* __restrict__ order, const int* __restrict__ lens,
                                                                    const float* __restrict__ mask, float* __restrict__ d_cat,
                                                                    float* __restrict__ d_emb, int t_max, int B, int seq_len, int E,
                                                                    int S) {
    const int row = blockIdx.x, t = row / B, j = row - t * B, I = E + S;
    const int src = txt_perm(order, j, B);
    const bool live = t < t_max;
    const size_t in = (size_t)row * I;                          // (read only where live: dxa / dxb end at t_max)
    if (d_emb) {
        const bool own = live && t < lens[j];
        const float* m = mask ? mask + (size_t)row * E : nullptr;
        float* o = d_emb + ((size_t)src * seq_len + t) * E;
        for (int k = threadIdx.x; k < E; k += 256) {
            float g = 0.f;
            if (own) {
                g = dxb ? dxa[in + k] + dxb[in + k] : dxa[in + k];
                if (m) g = __fmul_rn(g, m[k]);
            }
            o[k] = g;
        }
    }
    if (d_cat) {
        float* o = d_cat + ((size_t)t * B + src) * I + E;
        for (int k = threadIdx.x; k < S; k += 256) o[k] = live ? (dxb ? dxa[in + E + k] + dxb[in + E + k] : dxa[in + E + k]) : 0.f;
    }
}

// The state entering each step of a layer, for its recurrent weight gradient: hprev[0][t] = out[0][t-1], hprev[1][t] = out[1][t+1],
// zeros at the two ends (out is zero past each sample's length, so the reverse direction starts from zeros at its own last token).
// grid (T * B, 2), 256 threads.
__global__ __launch_bounds__(256) void txt_prev_state_kernel(const float* __restrict__ out, float* __restrict__ hprev, int T, int B, int H) {
    const int row = blockIdx.x, d = blockIdx.y, t = row / B;
    const int tp = d == 0 ? t - 1 : t + 1;
    const bool has = tp >= 0 && tp < T;
    const float* src = out + ((size_t)d * T * B + (size_t)(has ? tp : t) * B + (row - t * B)) * H;
    float* dst = hprev + ((size_t)d * T * B + row) * H;
    for (int u = threadIdx.x; u < H; u += 256) dst[u] = has ? src[u] : 0.f;
}

// Between two layers: data[t][j][d*H + u] = out[d][t][j][u] * mask.  mask_row NULL: mask is [T][B][2H]; else the mask row of
// slot (t, j) is mask_row[t*B + j] (the packed-order draw of parity mode).  grid T * B, 256 threads.
__global__ __launch_bounds__(256) void txt_inter_fwd_kernel(const float* __restrict__ out, const float* __restrict__ mask,
                                                            const long long* __restrict__ mask_row, float* __restrict__ data, int T,
                                                            int B, int H) {
    const size_t row = blockIdx.x, TB = (size_t)T * B;
    const float* m = mask ? mask + (size_t)(mask_row ? mask_row[row] : (long long)row) * 2 * H : nullptr;
    for (int k = threadIdx.x; k < 2 * H; k += 256) {
        const int d = k >= H, u = k - d * H;
        const float v = out[(d * TB + row) * H + u];
        data[row * 2 * H + k] = m ? v * m[k] : v;
    }
}

// Where the final state of direction d of sorted sample j is taken from: its last token (forward) or t = 0 (reverse).
__device__ __forceinline__ bool txt_is_final(int d, int t, int last_j) { return t == (d == 0 ? last_j : 0); }
// Its place in feat, read as [L][2B][2][H]: rows [0, B) of a layer are h of the caller's samples, rows [B, 2B) their c (the
// reference concatenates h_n and c_n along the BATCH axis before its view(bsz, -1); reproduced).
__device__ __forceinline__ size_t txt_feat_at(int l, int is_c, int caller_row, int d, int u, int B, int H) {
    return ((((size_t)l * 2 + is_c) * B + caller_row) * 2 + d) * H + u;
}

// feat from out / c of every layer.  grid (B, 2 * layers), 256 threads: block (i, 2l + is_c) writes the [2][H] row of caller sample i.
__global__ __launch_bounds__(256) void txt_states_fwd_kernel(dwc_txt_layers ly, const int* __restrict__ last,
                                                             const int* __restrict__ unsort, float* __restrict__ feat, int T, int B,
                                                             int H) {
    const int i = blockIdx.x, l = blockIdx.y >> 1, is_c = blockIdx.y & 1;
    const int j = txt_perm(unsort, i, B);
    const float* src = is_c ? ly.c[l] : ly.out[l];
    const int t_fwd = min(max(last[j], 0), T - 1);
    for (int k = threadIdx.x; k < 2 * H; k += 256) {
        const int d = k >= H, u = k - d * H;
        const int t = d == 0 ? t_fwd : 0;
        feat[txt_feat_at(l, is_c, i, d, u, B, H)] = src[(((size_t)d * T + t) * B + j) * H + u];
    }
}

// Adjoint: d_feat scattered into d_out / d_c of the layers, zeros everywhere else.  grid (T * B, 2, 2 * layers): block
// (t*B + j, d, 2l + is_c) writes H values; a NULL tensor is skipped (d_out of a lower layer comes from txt_inter_bwd_kernel).
__global__ __launch_bounds__(256) void txt_states_bwd_kernel(const float* __restrict__ d_feat, const int* __restrict__ order,
                                                             const int* __restrict__ last, dwc_txt_layers ly, int T, int B, int H) {
    const int l = blockIdx.z >> 1, is_c = blockIdx.z & 1, d = blockIdx.y;
    float* dst = is_c ? ly.c[l] : ly.out[l];
    if (!dst) return;
    const int row = blockIdx.x, t = row / B, j = row - t * B;
    const bool fin = txt_is_final(d, t, last[j]);
    const int i = txt_perm(order, j, B);
    float* o = dst + ((size_t)d * T * B + row) * H;
    for (int u = threadIdx.x; u < H; u += 256) o[u] = fin ? d_feat[txt_feat_at(l, is_c, i, d, u, B, H)] : 0.f;
}

// d_out of layer l below the top one, written once: the gradient coming down from the next layer's operand (dxa + dxb,
// [T][B][2H], times the inter-layer mask) plus layer l's own final-state rows of d_feat.  grid (T * B, 2), 256 threads.
__global__ __launch_bounds__(256) void txt_inter_bwd_kernel(const float* __restrict__ dxa, const float* __restrict__ dxb,
                                                            const float* __restrict__ mask, const long long* __restrict__ mask_row,
                                                            const float* __restrict__ d_feat, const int* __restrict__ order,
                                                            const int* __restrict__ last, int l, float* __restrict__ d_out, int T,
                                                            int B, int H) {
    const int row = blockIdx.x, d = blockIdx.y, t = row / B, j = row - t * B;
    const float* m = mask ? mask + (size_t)(mask_row ? mask_row[row] : (long long)row) * 2 * H + d * H : nullptr;
    const bool fin = txt_is_final(d, t, last[j]);
    const int i = txt_perm(order, j, B);
    const size_t in = (size_t)row * 2 * H + d * H;
    float* o = d_out + ((size_t)d * T * B + row) * H;
    for (int u = threadIdx.x; u < H; u += 256) {
        float g = dxb ? dxa[in + u] + dxb[in + u] : dxa[in + u];
        if (m) g = __fmul_rn(g, m[u]);                        // (rounded product: not to be contracted with the add below)
        o[u] = fin ? g + d_feat[txt_feat_at(l, 0, i, d, u, B, H)] : g;
    }
}

// Regrouping feat (TxtEncoder's `group` / `sync`).  feat:[B][4LH] read flat is [2L planes][B] rows of 2H floats -- plane 2l + is_c,
// caller sample b (txt_feat_at) --, and the feature row of a sample is 2L CONSECUTIVE flat rows: the reference's view(B, -1) over
// the whole call.  Taking that view over another set of samples is a permutation of the rows.  The four forms give the source row
// of destination row `o`; n counts rows inside the set the view is taken over:
//   group fwd  (a = B,  b = G)  out row o = i*2L + k of sample i, group g = i / G:   n = o - g*G*2L  <- feat row (n/G)*B + g*G + n%G
//   group bwd  (a = B,  b = G)  d_feat row o = p*B + g*G + rr:                       <- d_out row g*G*2L + p*G + rr
//   rank fwd   (a = Bl, b = W)  out row o of rank r, n = r*Bl*2L + o, Bg = W*Bl:     <- rank (n%Bg)/Bl's feat row (n/Bg)*Bl + n%Bg%Bl
//   rank bwd   (a = Bl, b = W)  d_feat row o = p*Bl + i2 of rank r:                  <- row p*Bg + r*Bl + i2 of the gathered d_out
// Every source row lies inside its buffer for a, b >= 1 and b | a (group) or 0 <= r < b (rank): the host checks exactly that.
enum { TXT_GROUP_FWD = 0, TXT_GROUP_BWD = 1, TXT_RANK_FWD = 2, TXT_RANK_BWD = 3 };

__device__ __forceinline__ int txt_regroup_src(int form, int o, int L2, int a, int b, int r) {
    if (form == TXT_GROUP_FWD) {
        const int g = o / L2 / b, n = o - g * b * L2;
        return (n / b) * a + g * b + n % b;
    }
    if (form == TXT_GROUP_BWD) {
        const int p = o / a, s = o - p * a, g = s / b;
        return g * b * L2 + p * b + (s - g * b);
    }
    if (form == TXT_RANK_FWD) {
        const int Bg = a * b, n = r * a * L2 + o, p = n / Bg, row = n - p * Bg, s = row / a;
        return s * a * L2 + p * a + (row - s * a);
    }
    const int p = o / a;
    return p * a * b + r * a + (o - p * a);
}

// One block per destination row, 256 threads; VEC: 2H % 4 == 0 and both bases 16-byte aligned, the row moves as 16-byte words.
template <bool VEC>
__global__ __launch_bounds__(256) void txt_regroup_kernel(const float* __restrict__ src, float* __restrict__ dst, int form, int L2,
                                                          int a, int b, int r, int width) {
    const int o = blockIdx.x;
    const size_t from = (size_t)txt_regroup_src(form, o, L2, a, b, r) * width, to = (size_t)o * width;
    if (VEC) {
        typedef float v4f __attribute__((ext_vector_type(4)));
        const v4f* s = reinterpret_cast<const v4f*>(src + from);
        v4f* d = reinterpret_cast<v4f*>(dst + to);
        for (int k = threadIdx.x; k < width / 4; k += 256) d[k] = s[k];
    } else {
        for (int k = threadIdx.x; k < width; k += 256) dst[to + k] = src[from + k];
    }
}

// rows: destination rows (one block each); rows_src: rows of the source buffer.  Both must fit a grid, and the larger buffer's last
// 16-byte word an unsigned 32-bit index.
int txt_regroup_launch(const float* src, float* dst, int form, int L, int a, int b, int r, int H, long long rows, long long rows_src,
                       void* stream) {
    if (rows < 1 || rows > 0x7fffffffLL || rows_src > 0x7fffffffLL) return DWC_EINVAL;
    const unsigned long long width = 2ull * (unsigned)H;
    if ((unsigned long long)(rows_src > rows ? rows_src : rows) * width > 4ull * 0xffffffffull) return DWC_EINVAL;
    const bool vec = width % 4 == 0 && ((uintptr_t)src | (uintptr_t)dst) % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(txt_regroup_kernel<true>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, src, dst, form, 2 * L, a, b,
                           r, (int)width);
    else
        hipLaunchKernelGGL(txt_regroup_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, src, dst, form, 2 * L, a,
                           b, r, (int)width);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

bool txt_group_ok(const float* src, const float* dst, int L, int B, int H, int G) {
    return src && dst && L >= 1 && L <= DWC_TXT_MAX_LAYERS && B >= 1 && H >= 1 && H <= 0x3fffffff && G >= 1 && B % G == 0;
}

bool txt_rank_ok(const float* src, const float* dst, int L, int W, int Bl, int H, int rank) {
    return src && dst && L >= 1 && L <= DWC_TXT_MAX_LAYERS && W >= 1 && Bl >= 1 && H >= 1 && H <= 0x3fffffff && rank >= 0 && rank < W &&
           (long long)W * Bl <= 0x7fffffffLL;
}

bool txt_layers_ok(const dwc_txt_layers& ly) { return ly.n >= 1 && ly.n <= DWC_TXT_MAX_LAYERS; }

}  // namespace

extern "C" {

int dwc_txt_operand_fwd(const float* table, const long long* tokens, const int* order, const float* mask, const float* style,
                        float* x, int t_max, int B, int seq_len, int E, int S, int vocab, void* stream) {
    if (!table || !tokens || !order || !x || (S > 0 && !style) || t_max < 1 || t_max > seq_len || B < 1 || E < 1 || S < 0 || vocab < 1)
        return DWC_EINVAL;
    hipLaunchKernelGGL(txt_operand_fwd_kernel, dim3(t_max * B), dim3(256), 0, (hipStream_t)stream, table, tokens, order, mask, style, x,
                       B, seq_len, E, S, vocab);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_operand_bwd(const float* dxa, const float* dxb, const long long* tokens, const int* order, const float* mask,
                        float* d_cat, float* d_emb, long long* idx, int t_max, int B, int seq_len, int E, int S, void* stream) {
    if (!dxa || !tokens || !order || (!d_cat && !d_emb && !idx) || t_max < 1 || t_max > seq_len || B < 1 || E < 1 || S < 0 ||
        (d_cat && S < 1) || (long long)seq_len * B > 0x7fffffffLL)
        return DWC_EINVAL;
    hipLaunchKernelGGL(txt_operand_bwd_kernel, dim3(seq_len * B), dim3(256), 0, (hipStream_t)stream, dxa, dxb, tokens, order, mask,
                       d_cat, d_emb, idx, t_max, B, seq_len, E, S);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_operand_embed_fwd(const float* emb, const int* order, const int* lens, const float* mask, const float* style, float* x,
                              int t_max, int B, int seq_len, int E, int S, void* stream) {
    if (!emb || !order || !lens || !x || (S > 0 && !style) || seq_len < 1 || t_max < 1 || t_max > seq_len || B < 1 || E < 1 || S < 0 ||
        (long long)seq_len * B > 0x7fffffffLL)
        return DWC_EINVAL;
    hipLaunchKernelGGL(txt_operand_embed_fwd_kernel, dim3(t_max * B), dim3(256), 0, (hipStream_t)stream, emb, order, lens, mask, style,
                       x, B, seq_len, E, S);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_operand_embed_bwd(const float* dxa, const float* dxb, const int* order, const int* lens, const float* mask, float* d_cat,
                              float* d_emb, int t_max, int B, int seq_len, int E, int S, void* stream) {
    if (!dxa || !order || !lens || (!d_cat && !d_emb) || seq_len < 1 || t_max < 1 || t_max > seq_len || B < 1 || E < 1 || S < 0 ||
        (d_cat && S < 1) || (long long)seq_len * B > 0x7fffffffLL)
        return DWC_EINVAL;
    hipLaunchKernelGGL(txt_operand_embed_bwd_kernel, dim3(seq_len * B), dim3(256), 0, (hipStream_t)stream, dxa, dxb, order, lens, mask,
                       d_cat, d_emb, t_max, B, seq_len, E, S);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_prev_state(const float* out, float* hprev, int T, int B, int H, void* stream) {
    if (!out || !hprev || T < 1 || B < 1 || H < 1 || (long long)T * B > 0x7fffffffLL) return DWC_EINVAL;
    hipLaunchKernelGGL(txt_prev_state_kernel, dim3(T * B, 2), dim3(256), 0, (hipStream_t)stream, out, hprev, T, B, H);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_inter_fwd(const float* out, const float* mask, const long long* mask_row, float* data, int T, int B, int H, void* stream) {
    if (!out || !data || (mask_row && !mask) || T < 1 || B < 1 || H < 1) return DWC_EINVAL;
    hipLaunchKernelGGL(txt_inter_fwd_kernel, dim3(T * B), dim3(256), 0, (hipStream_t)stream, out, mask, mask_row, data, T, B, H);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_inter_bwd(const float* dxa, const float* dxb, const float* mask, const long long* mask_row, const float* d_feat,
                      const int* order, const int* last, int layer, float* d_out, int T, int B, int H, void* stream) {
    if (!dxa || !d_feat || !order || !last || !d_out || (mask_row && !mask) || layer < 0 || layer >= DWC_TXT_MAX_LAYERS || T < 1 ||
        B < 1 || H < 1)
        return DWC_EINVAL;
    hipLaunchKernelGGL(txt_inter_bwd_kernel, dim3(T * B, 2), dim3(256), 0, (hipStream_t)stream, dxa, dxb, mask, mask_row, d_feat, order,
                       last, layer, d_out, T, B, H);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_states_fwd(dwc_txt_layers layers, const int* last, const int* unsort, float* feat, int T, int B, int H, void* stream) {
    if (!txt_layers_ok(layers) || !last || !unsort || !feat || T < 1 || B < 1 || H < 1) return DWC_EINVAL;
    for (int l = 0; l < layers.n; ++l)
        if (!layers.out[l] || !layers.c[l]) return DWC_EINVAL;
    hipLaunchKernelGGL(txt_states_fwd_kernel, dim3(B, 2 * layers.n), dim3(256), 0, (hipStream_t)stream, layers, last, unsort, feat, T, B,
                       H);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_states_bwd(const float* d_feat, const int* order, const int* last, dwc_txt_layers grads, int T, int B, int H,
                       void* stream) {
    if (!txt_layers_ok(grads) || !d_feat || !order || !last || T < 1 || B < 1 || H < 1 || (long long)T * B > 0x7fffffffLL)
        return DWC_EINVAL;
    hipLaunchKernelGGL(txt_states_bwd_kernel, dim3(T * B, 2, 2 * grads.n), dim3(256), 0, (hipStream_t)stream, d_feat, order, last, grads,
                       T, B, H);
    DWC_LAUNCH_CHECK();
    return DWC_OK;
}

int dwc_txt_regroup_fwd(const float* feat, float* out, int L, int B, int H, int G, void* stream) {
    if (!txt_group_ok(feat, out, L, B, H, G)) return DWC_EINVAL;
    return txt_regroup_launch(feat, out, TXT_GROUP_FWD, L, B, G, 0, H, 2LL * L * B, 2LL * L * B, stream);
}

int dwc_txt_regroup_bwd(const float* d_out, float* d_feat, int L, int B, int H, int G, void* stream) {
    if (!txt_group_ok(d_out, d_feat, L, B, H, G)) return DWC_EINVAL;
    return txt_regroup_launch(d_out, d_feat, TXT_GROUP_BWD, L, B, G, 0, H, 2LL * L * B, 2LL * L * B, stream);
}

int dwc_txt_regroup_rank_fwd(const float* feat_all, float* out, int L, int W, int Bl, int H, int rank, void* stream) {
    if (!txt_rank_ok(feat_all, out, L, W, Bl, H, rank)) return DWC_EINVAL;
    return txt_regroup_launch(feat_all, out, TXT_RANK_FWD, L, Bl, W, rank, H, 2LL * L * Bl, 2LL * L * Bl * W, stream);
}

int dwc_txt_regroup_rank_bwd(const float* d_out_all, float* d_feat, int L, int W, int Bl, int H, int rank, void* stream) {
    if (!txt_rank_ok(d_out_all, d_feat, L, W, Bl, H, rank)) return DWC_EINVAL;
    return txt_regroup_launch(d_out_all, d_feat, TXT_RANK_BWD, L, Bl, W, rank, H, 2LL * L * Bl, 2LL * L * Bl * W, stream);
}

}  // extern "C"
