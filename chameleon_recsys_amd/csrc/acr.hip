// ACR module (Article Content Representation): the CNN article encoder's hot path.
//
// Replaces (acr_module/acr/acr_model.py):
//   * :83-87    tf.nn.embedding_lookup of the CONSTANT word-embedding matrix
//   * :272-289  cnn_feature_extractor: per filter size k a "valid" conv1d + bias + ReLU, reduce_max over time, concat
//   * :196-198  tf.losses.sparse_softmax_cross_entropy with per-class weights (SUM_BY_NONZERO_WEIGHTS), :171 argmax predictions
//   * the gradients of both (autodiff under :232)
//
// Forward: x[b,t,:] = table[text[b,t],:] is never materialised.  One workgroup stages rows t0 .. t0+TM+kmax-2 of ONE article straight
// from the table into LDS; the A operand of output position t and tap j is then LDS row t+j (the overlapping window IS the im2col
// matrix).  W_k [k, E, F] streams from L2, one dword per lane per MFMA.  Accumulation on v_mfma_f32_32x32x2_f32 (exact fp32, a fixed
// K order per output row: bit-equal windows give bit-equal values, which the first-index tie rule below relies on).  Epilogue: + bias,
// ReLU, rows t > L-k dropped, max over the tile's positions with the FIRST index on ties -> one (max, argmax) partial per
// (article, position tile, column); a second kernel reduces the tiles in ascending order.  No float atomics: bit-reproducible.
#include "common.h"

#define ACR_TM 32           /* output positions per workgroup (one 32-row MFMA tile) */
#define ACR_FN 128          /* filters per workgroup: 4 waves x 32 */
#define ACR_MAX_SIZES 8
#define ACR_MAX_K 16
#define ACR_EC 320          /* embedding columns staged per pass (% 8 == 0); E = 300 fits in one pass */

struct AcrConvArgs {
    const float* W[ACR_MAX_SIZES];      // [k, E, F] as tf.layers.conv1d stores it
    const float* bias[ACR_MAX_SIZES];   // [F]
    float* dW[ACR_MAX_SIZES];           // backward only
    float* dbias[ACR_MAX_SIZES];
    int k[ACR_MAX_SIZES];
    int n_sizes, kmax;
};

__device__ __forceinline__ long long acr_token(const int32_t* __restrict__ tok, int t, long long V) {
    long long id = tok[t];                                   // the host validates ids; a bad one must still never leave the table
    return id < 0 ? 0 : (id >= V ? V - 1 : id);
}

__global__ __launch_bounds__(256) void k_acr_conv_pool(const int32_t* __restrict__ tokens, int L, const float* __restrict__ table,
                                                       long long V, int E, long long ldE, AcrConvArgs a, int F, int S, int n_chunks,
                                                       int n_tiles, float* __restrict__ pmax, int32_t* __restrict__ parg) {
    extern __shared__ float xs[];                            // [ACR_TM + kmax - 1][S]
    const int b = blockIdx.z, tile = blockIdx.x, t0 = tile * ACR_TM;
    const int rows = ACR_TM + a.kmax - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, kl = lane >> 5, fl = lane & 31;
    const int f = blockIdx.y * ACR_FN + wave * 32 + fl;
    const int fc = f < F ? f : F - 1;                        // columns beyond F compute on a clamped address and are dropped
    const int32_t* tok = tokens + (size_t)b * L;
    const int PW = a.n_sizes * F;

    for (int s = 0; s < a.n_sizes; ++s) {
        const int k = a.k[s];
        const float* __restrict__ W = a.W[s];
        floatx16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
        for (int c = 0; c < n_chunks; ++c) {
            const int e0 = c * ACR_EC, ec = min(ACR_EC, E - e0), ec8 = (ec + 7) & ~7, q4 = ec8 >> 2;
            if (n_chunks > 1 || s == 0) {                    // one staged tile serves every filter size when E fits in one pass
                __syncthreads();
                for (int idx = threadIdx.x; idx < rows * q4; idx += 256) {
                    const int r = idx / q4, q = idx - r * q4, t = t0 + r, e = e0 + 4 * q;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (t < L && e < E) {                    // (ldE % 4 == 0 and ldE >= E: the 16 bytes lie inside the row)
                        v = ld4(table + (size_t)acr_token(tok, t, V) * (size_t)ldE + e);
                        if (e + 1 >= E) v.y = 0.f;           // the tail of E is zero-filled: pad columns of the table never enter
                        if (e + 2 >= E) v.z = 0.f;
                        if (e + 3 >= E) v.w = 0.f;
                    }
                    st4(xs + r * S + 4 * q, v);
                }
                __syncthreads();
            }
            // K order of one pass: taps ascending, within a tap 8 columns per step (lanes 0-31 take e..e+3, lanes 32-63 e+4..e+7)
            for (int j = 0; j < k; ++j) {
                const float* arow = xs + (fl + j) * S + 4 * kl;
                const float* wrow = W + ((size_t)j * E + e0) * F + fc;
#pragma unroll 2
                for (int e = 0; e < ec8; e += 8) {
                    const float4 av = *reinterpret_cast<const float4*>(arow + e);
                    const int ee = e + 4 * kl;
                    float w[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int er = ee + u < ec ? ee + u : ec - 1;
                        const float x = wrow[(size_t)er * F];
                        w[u] = ee + u < ec ? x : 0.f;
                    }
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, w[0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, w[1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, w[2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, w[3], acc, 0, 0, 0);
                }
            }
        }
        // epilogue: bias, ReLU, valid rows only, first index of the maximum (a lane's rows ascend with e).  ReLU output is >= 0, so -1
        // marks "no valid position in this tile".
        const float bv = a.bias[s][fc];
        const int npos = L - k + 1;
        float best = -1.f;
        int bi = 0;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int t = t0 + (e & 3) + 8 * (e >> 2) + 4 * kl;
            const float v = fmaxf(acc[e] + bv, 0.f);
            if (t < npos && v > best) { best = v; bi = t; }
        }
        const float ob = __shfl_xor(best, 32, 64);
        const int oi = __shfl_xor(bi, 32, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        if (kl == 0 && f < F) {
            const size_t o = ((size_t)b * n_tiles + tile) * PW + (size_t)s * F + f;
            pmax[o] = best; parg[o] = bi;
        }
    }
}

// pool[b, col] / argmax[b, col] = the tiles' partials reduced in ascending tile order (strict >: the first index wins a tie)
__global__ __launch_bounds__(256) void k_acr_pool_reduce(const float* __restrict__ pmax, const int32_t* __restrict__ parg, int B, int PW,
                                                         int n_tiles, float* __restrict__ pool, int ldP, int32_t* __restrict__ argmax) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)B * PW) return;
    const int b = (int)(i / PW), col = (int)(i - (size_t)b * PW);
    float best = -1.f;
    int bi = 0;
    for (int t = 0; t < n_tiles; ++t) {
        const size_t o = ((size_t)b * n_tiles + t) * PW + col;
        const float v = pmax[o];
        if (v > best) { best = v; bi = parg[o]; }
    }
    pool[(size_t)b * ldP + col] = best;
    argmax[i] = bi;
}

static int acr_check_sizes(const int* sizes, int n_sizes, int* kmin, int* kmax) {
    if (!sizes || n_sizes < 1 || n_sizes > ACR_MAX_SIZES) return -CHAM_ERR_ARG;
    *kmin = ACR_MAX_K; *kmax = 1;
    for (int s = 0; s < n_sizes; ++s) {
        if (sizes[s] < 1 || sizes[s] > ACR_MAX_K) return -CHAM_ERR_ARG;
        if (sizes[s] < *kmin) *kmin = sizes[s];
        if (sizes[s] > *kmax) *kmax = sizes[s];
    }
    return CHAM_OK;
}

extern "C" size_t cham_acr_conv_pool_workspace_bytes(int B, int L, const int* sizes, int n_sizes, int F) {
    int kmin, kmax;
    if (acr_check_sizes(sizes, n_sizes, &kmin, &kmax) != CHAM_OK || B <= 0 || F <= 0 || L < kmax) return 0;
    const size_t n_tiles = (size_t)(L - kmin + 1 + ACR_TM - 1) / ACR_TM;
    return (size_t)B * n_tiles * n_sizes * F * (sizeof(float) + sizeof(int32_t));
}

extern "C" int cham_acr_conv_pool_fwd(const int32_t* tokens, int B, int L, const float* table, long long V, int E, long long ldE,
                                      const int* sizes, int n_sizes, int F, const float* const* W, const float* const* bias, float* pool,
                                      int ldP, int32_t* argmax, void* workspace, size_t workspace_bytes, void* stream) {
    int kmin, kmax;
    if (acr_check_sizes(sizes, n_sizes, &kmin, &kmax) != CHAM_OK) return -CHAM_ERR_ARG;
    if (!tokens || !table || !W || !bias || !pool || !argmax || !workspace) return -CHAM_ERR_ARG;
    if (B <= 0 || B > 65535 || L < kmax || V < 1 || E < 1 || F < 1 || ldE < E || (ldE & 3) || ((uintptr_t)table & 15)) return -CHAM_ERR_ARG;
    if ((long long)n_sizes * F > 0x7fffffffLL || ldP < n_sizes * F) return -CHAM_ERR_ARG;
    if (workspace_bytes < cham_acr_conv_pool_workspace_bytes(B, L, sizes, n_sizes, F) || ((uintptr_t)workspace & 3)) return -CHAM_ERR_ARG;
    AcrConvArgs a = {};
    a.n_sizes = n_sizes; a.kmax = kmax;
    for (int s = 0; s < n_sizes; ++s) {
        if (!W[s] || !bias[s]) return -CHAM_ERR_ARG;
        a.W[s] = W[s]; a.bias[s] = bias[s]; a.k[s] = sizes[s];
    }
    const int n_tiles = (L - kmin + 1 + ACR_TM - 1) / ACR_TM, PW = n_sizes * F;
    const int n_chunks = (E + ACR_EC - 1) / ACR_EC;
    const int s0 = ((E < ACR_EC ? E : ACR_EC) + 7) & ~7, S = s0 + 4;      // S / 4 odd: the 32 rows of a 16-byte column read spread over the banks
    const int lds = (ACR_TM + kmax - 1) * S * (int)sizeof(float);        // <= 47 x 324 x 4 = 60 912 bytes
    float* pmax = reinterpret_cast<float*>(workspace);
    int32_t* parg = reinterpret_cast<int32_t*>(pmax + (size_t)B * n_tiles * PW);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_acr_conv_pool, dim3(n_tiles, (F + ACR_FN - 1) / ACR_FN, B), dim3(256), lds, st, tokens, L, table, V, E, ldE, a, F, S,
                       n_chunks, n_tiles, pmax, parg);
    CHAM_CHECK_LAUNCH();
    const size_t n = (size_t)B * PW;
    hipLaunchKernelGGL(k_acr_pool_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pmax, parg, B, PW, n_tiles, pool, ldP, argmax);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// ---- backward of conv + ReLU + max (the table is a constant: no dx).  g[b,f] = dpool[b,f] (pool[b,f] > 0);
//   dW_k[(j,e), f] = sum_b g[b,f] table[text[b, argmax_k[b,f] + j], e],   dbias_k[f] = sum_b g[b,f]
// One workgroup per (size, tap j, filter f); lanes over e (coalesced table rows); b ascending with one fma each: a fixed order, no atomics.
__global__ __launch_bounds__(256) void k_acr_conv_pool_bwd(const int32_t* __restrict__ tokens, int B, int L, const float* __restrict__ table,
                                                           long long V, int E, long long ldE, const float* __restrict__ dpool,
                                                           const float* __restrict__ pool, int ldP, const int32_t* __restrict__ argmax,
                                                           int F, AcrConvArgs a) {
    int s = 0, r = blockIdx.x;
    while (s < a.n_sizes - 1 && r >= a.k[s] * F) { r -= a.k[s] * F; ++s; }
    const int j = r / F, f = r - j * F, col = s * F + f, PW = a.n_sizes * F;
    float* __restrict__ dW = a.dW[s];
    for (int e = threadIdx.x; e < E; e += 256) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) {
            const float g = pool[(size_t)b * ldP + col] > 0.f ? dpool[(size_t)b * ldP + col] : 0.f;
            if (g != 0.f) {
                int t = argmax[(size_t)b * PW + col] + j;
                t = t < 0 ? 0 : (t >= L ? L - 1 : t);
                acc = fmaf(g, table[(size_t)acr_token(tokens + (size_t)b * L, t, V) * (size_t)ldE + e], acc);
            }
        }
        dW[((size_t)j * E + e) * F + f] = acc;
    }
    if (j == 0 && threadIdx.x == 0) {
        float acc = 0.f;
        for (int b = 0; b < B; ++b) acc += pool[(size_t)b * ldP + col] > 0.f ? dpool[(size_t)b * ldP + col] : 0.f;
        a.dbias[s][f] = acc;
    }
}

extern "C" int cham_acr_conv_pool_bwd(const int32_t* tokens, int B, int L, const float* table, long long V, int E, long long ldE,
                                      const int* sizes, int n_sizes, int F, const float* dpool, const float* pool, int ldP,
                                      const int32_t* argmax, float* const* dW, float* const* dbias, void* stream) {
    int kmin, kmax;
    if (acr_check_sizes(sizes, n_sizes, &kmin, &kmax) != CHAM_OK) return -CHAM_ERR_ARG;
    if (!tokens || !table || !dpool || !pool || !argmax || !dW || !dbias) return -CHAM_ERR_ARG;
    if (B <= 0 || L < kmax || V < 1 || E < 1 || F < 1 || ldE < E || ldP < n_sizes * F) return -CHAM_ERR_ARG;
    AcrConvArgs a = {};
    a.n_sizes = n_sizes; a.kmax = kmax;
    long long blocks = 0;
    for (int s = 0; s < n_sizes; ++s) {
        if (!dW[s] || !dbias[s]) return -CHAM_ERR_ARG;
        a.dW[s] = dW[s]; a.dbias[s] = dbias[s]; a.k[s] = sizes[s];
        blocks += (long long)sizes[s] * F;
    }
    if (blocks > 0x7fffffffLL) return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_acr_conv_pool_bwd, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tokens, B, L, table, V, E, ldE, dpool, pool,
                       ldP, argmax, F, a);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// ---- sparse softmax cross-entropy of one label head, tf.losses reduction SUM_BY_NONZERO_WEIGHTS:
//   loss = sum_b w_b ce_b / #{b : w_b != 0} (0 when no weight is non-zero), w_b = class_weights[label_b] or 1;
//   dlogits[b,c] = w_b / # (softmax[b,c] - [c == label_b]) for c < C and 0 for the padded columns c in [C, ld);  pred[b] = first argmax.
// One wave per row; the padded columns of `logits` are never read.
__device__ __forceinline__ int acr_label(const int32_t* __restrict__ labels, int b, int C) {
    const int y = labels[b];
    return y < 0 ? 0 : (y >= C ? C - 1 : y);                 // validated on the host; clamped so that no id can leave the row
}
__device__ __forceinline__ float acr_nonzero_weights(const int32_t* __restrict__ labels, const float* __restrict__ cw, int B, int C, float* red) {
    float cnt = 0.f;                                          // (a count below 2^24: exact in fp32)
    for (int i = threadIdx.x; i < B; i += 256) cnt += (cw ? cw[acr_label(labels, i, C)] : 1.f) != 0.f ? 1.f : 0.f;
    return block_sum(cnt, red);
}
__global__ __launch_bounds__(256) void k_acr_xent(const float* __restrict__ logits, int ld, int B, int C, const int32_t* __restrict__ labels,
                                                  const float* __restrict__ cw, float* __restrict__ dlogits, int32_t* __restrict__ pred,
                                                  float* __restrict__ row_ce) {
    __shared__ float red[4];
    const float cnt = acr_nonzero_weights(labels, cw, B, C, red);
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= B) return;
    const float* x = logits + (size_t)row * ld;
    float m = -INFINITY;
    int mi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) {
        const float v = x[c];
        if (v > m) { m = v; mi = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float om = __shfl_xor(m, o, 64);
        const int oi = __shfl_xor(mi, o, 64);
        if (om > m || (om == m && oi < mi)) { m = om; mi = oi; }
    }
    if (mi == 0x7fffffff) mi = 0;
    float s = 0.f;
    for (int c = lane; c < C; c += 64) s += expf(x[c] - m);
    s = wave_sum(s);
    const int y = acr_label(labels, row, C);
    const float w = cw ? cw[y] : 1.f;
    if (lane == 0) {
        row_ce[row] = w * ((m + logf(s)) - x[y]);
        pred[row] = mi;
    }
    if (dlogits) {
        const float scale = cnt > 0.f ? w / cnt : 0.f, inv = 1.f / s;
        float* d = dlogits + (size_t)row * ld;
        for (int c = lane; c < ld; c += 64) d[c] = c < C ? scale * (expf(x[c] - m) * inv - (c == y ? 1.f : 0.f)) : 0.f;
    }
}
__global__ __launch_bounds__(256) void k_acr_xent_loss(const float* __restrict__ row_ce, int B, int C, const int32_t* __restrict__ labels,
                                                       const float* __restrict__ cw, float* __restrict__ loss) {
    __shared__ float red[4];
    const float cnt = acr_nonzero_weights(labels, cw, B, C, red);
    float s = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) s += row_ce[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) loss[0] = cnt > 0.f ? s / cnt : 0.f;
}

extern "C" int cham_acr_softmax_xent(const float* logits, int ld, int B, int C, const int32_t* labels, const float* class_weights,
                                     float* loss, float* dlogits, int32_t* pred, float* row_workspace, void* stream) {
    if (!logits || !labels || !loss || !pred || !row_workspace || B <= 0 || C <= 0 || ld < C) return -CHAM_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_acr_xent, dim3((B + 3) / 4), dim3(256), 0, st, logits, ld, B, C, labels, class_weights, dlogits, pred, row_workspace);
    CHAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_acr_xent_loss, dim3(1), dim3(256), 0, st, row_workspace, B, C, labels, class_weights, loss);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// ---- sigmoid cross-entropy of one MULTILABEL head (acr_model.py:202-215; predictions :6-8; precision / recall :254-268) against the
// multi-hot target built from a ragged, zero-padded id list, which never reaches memory:
//   z[b,c] = #{k < K : ids[b,k] == c} for c >= 1 (reduce_sum(one_hot): a duplicated id counts twice), z[b,0] = 0 (the padding id);
//   term = max(x,0) - x z + log1p(exp(-|x|));  loss = sum term / (B C);  dlogits = (sigmoid(x) - z) / (B C), 0 in the padded columns;
//   pred = x > 0;  counts = (tp, fp, fn) over c < C.
// Grid (column chunks of ACR_ML_CHUNK, rows).  A workgroup counts the row's ids that fall into its chunk into LDS (integer adds; an id
// outside [1, C) is ignored, one_hot's rule, so no id can index outside the chunk), then each lane takes 4 consecutive columns.  Float
// sums: the lane's 4 terms ascending, the butterfly wave sum, the 4 waves ascending -> one partial per (row, chunk); a single final
// workgroup adds the partials in a fixed order.  Counts are integers.  No float atomics: two runs are bit-identical.
#define ACR_ML_CHUNK 1024    /* columns per workgroup = 256 lanes x 4; one int of LDS per column */

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// the three per-workgroup counts: wave sums, then integer LDS adds; valid in cred[] after the trailing barrier
__device__ __forceinline__ void acr_block_counts(int tp, int fp, int fn, int* cred) {
    tp = wave_sum_int(tp); fp = wave_sum_int(fp); fn = wave_sum_int(fn);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&cred[0], tp); atomicAdd(&cred[1], fp); atomicAdd(&cred[2], fn); }
    __syncthreads();
}
__global__ __launch_bounds__(256) void k_acr_sigmoid_xent(const float* __restrict__ logits, int ld, int C, const int32_t* __restrict__ ids,
                                                          int K, int ldK, float inv_n, float* __restrict__ dlogits,
                                                          uint8_t* __restrict__ pred, int ldp, float* __restrict__ part,
                                                          int32_t* __restrict__ cpart, int vec) {
    __shared__ __attribute__((aligned(16))) int zc[ACR_ML_CHUNK];
    __shared__ float red[4];
    __shared__ int cred[3];
    const int b = blockIdx.y, c0 = blockIdx.x * ACR_ML_CHUNK, cl = 4 * threadIdx.x, c = c0 + cl;
    const int hi = min(C, c0 + ACR_ML_CHUNK), lo = max(c0, 1);
    *reinterpret_cast<int4*>(zc + cl) = make_int4(0, 0, 0, 0);
    if (threadIdx.x < 3) cred[threadIdx.x] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < K; k += 256) {
        const int id = ids[(size_t)b * ldK + k];
        if (id >= lo && id < hi) atomicAdd(&zc[id - c0], 1);
    }
    __syncthreads();
    const float* xr = logits + (size_t)b * ld;
    const int n = min(4, C - c);                             // this lane's columns inside [0, C); <= 0 for the lanes beyond
    float x[4] = {0.f, 0.f, 0.f, 0.f}, d[4];
    if (n == 4 && vec) {
        const float4 v = ld4(xr + c);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        for (int u = 0; u < n; ++u) x[u] = xr[c + u];        // (the padded columns [C, ld) are never read)
    }
    const int4 z4 = *reinterpret_cast<const int4*>(zc + cl);
    const int z[4] = {z4.x, z4.y, z4.z, z4.w};
    float s = 0.f;
    int tp = 0, fp = 0, fn = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const float zf = (float)z[u], e = expf(-fabsf(x[u]));
        const float term = (fmaxf(x[u], 0.f) - x[u] * zf) + log1pf(e);
        const float sig = (x[u] >= 0.f ? 1.f : e) / (1.f + e);
        const bool p = x[u] > 0.f, in = u < n;
        d[u] = in ? (sig - zf) * inv_n : 0.f;
        if (in) {
            s += term;
            tp += p && z[u] > 0; fp += p && z[u] == 0; fn += !p && z[u] > 0;
            pred[(size_t)b * ldp + c + u] = p ? 1 : 0;
        }
    }
    if (dlogits) {
        float* dr = dlogits + (size_t)b * ld;
        if (vec && c + 3 < min(ld, c0 + ACR_ML_CHUNK)) {
            if (n > 0) st4(dr + c, make_float4(d[0], d[1], d[2], d[3]));     // (a group that straddles C writes the zeros of [C, c + 4) too)
        } else {
            for (int u = 0; u < n; ++u) dr[c + u] = d[u];
        }
        if (blockIdx.x == gridDim.x - 1)                     // the last chunk zero-fills [C, ld) (what a straddling float4 wrote is 0 already)
            for (int cc = C + threadIdx.x; cc < ld; cc += 256) dr[cc] = 0.f;
    }
    s = block_sum(s, red);
    acr_block_counts(tp, fp, fn, cred);
    const size_t o = (size_t)b * gridDim.x + blockIdx.x;
    if (threadIdx.x == 0) part[o] = s;
    if (threadIdx.x < 3) cpart[3 * o + threadIdx.x] = cred[threadIdx.x];
}
__global__ __launch_bounds__(256) void k_acr_sigmoid_xent_loss(const float* __restrict__ part, const int32_t* __restrict__ cpart, int n_part,
                                                               float inv_n, float* __restrict__ loss, int32_t* __restrict__ counts) {
    __shared__ float red[4];
    __shared__ int cred[3];
    if (threadIdx.x < 3) cred[threadIdx.x] = 0;
    float s = 0.f;
    int tp = 0, fp = 0, fn = 0;
    for (int i = threadIdx.x; i < n_part; i += 256) {
        s += part[i];
        tp += cpart[3 * i]; fp += cpart[3 * i + 1]; fn += cpart[3 * i + 2];
    }
    s = block_sum(s, red);                                   // (its barriers also order the zeroing of cred before the adds below)
    acr_block_counts(tp, fp, fn, cred);
    if (threadIdx.x == 0) loss[0] = s * inv_n;
    if (threadIdx.x < 3) counts[threadIdx.x] = cred[threadIdx.x];
}

static long long acr_ml_chunks(int C) { return ((long long)C + ACR_ML_CHUNK - 1) / ACR_ML_CHUNK; }

extern "C" size_t cham_acr_sigmoid_xent_workspace_bytes(int B, int C) {
    if (B <= 0 || C <= 0) return 0;
    return (size_t)B * (size_t)acr_ml_chunks(C) * (sizeof(float) + 3 * sizeof(int32_t));
}

extern "C" int cham_acr_sigmoid_xent(const float* logits, int ld, int B, int C, const int32_t* label_ids, int K, int ldK, float* loss,
                                     float* dlogits, uint8_t* pred, int ldp, int32_t* counts, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (!logits || !loss || !pred || !counts || !workspace || B <= 0 || B > 65535 || C <= 0 || ld < C || ldp < C) return -CHAM_ERR_ARG;
    if (K < 0 || ldK < K || (K > 0 && !label_ids)) return -CHAM_ERR_ARG;
    const long long n_part = (long long)B * acr_ml_chunks(C);
    if ((long long)B * C > 0x7fffffffLL || n_part > 0x7fffffffLL) return -CHAM_ERR_ARG;                // (the counts are int32)
    if (workspace_bytes < cham_acr_sigmoid_xent_workspace_bytes(B, C) || ((uintptr_t)workspace & 3)) return -CHAM_ERR_ARG;
    const int vec = !(ld & 3) && !((uintptr_t)logits & 15) && !((uintptr_t)dlogits & 15);
    const float inv_n = (float)(1.0 / ((double)B * (double)C));
    float* part = reinterpret_cast<float*>(workspace);
    int32_t* cpart = reinterpret_cast<int32_t*>(part + n_part);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_acr_sigmoid_xent, dim3((unsigned)acr_ml_chunks(C), B), dim3(256), 0, st, logits, ld, C, label_ids, K, ldK, inv_n, dlogits,
                       pred, ldp, part, cpart, vec);
    CHAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_acr_sigmoid_xent_loss, dim3(1), dim3(256), 0, st, part, cpart, (int)n_part, inv_n, loss, counts);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// ---- the dense layers' small elementwise pieces (cham_gemm_f32 has no ReLU epilogue).  act: 0 = ReLU, 1 = tanh; y = the saved
// POST-activation value.  In place; n % 4 == 0 (padded widths).
__global__ __launch_bounds__(256) void k_acr_relu(float* __restrict__ x, size_t n4) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 v = reinterpret_cast<float4*>(x)[i];
        v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
        reinterpret_cast<float4*>(x)[i] = v;
    }
}
__global__ __launch_bounds__(256) void k_acr_act_bwd(float* __restrict__ dy, const float* __restrict__ y, size_t n4, int act) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        float4 d = reinterpret_cast<float4*>(dy)[i];
        const float4 v = reinterpret_cast<const float4*>(y)[i];
        if (act == 0) {
            d.x = v.x > 0.f ? d.x : 0.f; d.y = v.y > 0.f ? d.y : 0.f; d.z = v.z > 0.f ? d.z : 0.f; d.w = v.w > 0.f ? d.w : 0.f;
        } else {
            d.x *= 1.f - v.x * v.x; d.y *= 1.f - v.y * v.y; d.z *= 1.f - v.z * v.z; d.w *= 1.f - v.w * v.w;
        }
        reinterpret_cast<float4*>(dy)[i] = d;
    }
}
static unsigned acr_blocks(size_t n4) {
    size_t blocks = (n4 + 255) / 256;
    return (unsigned)(blocks > 8192 ? 8192 : blocks);
}
extern "C" int cham_acr_relu(float* x, size_t n, void* stream) {
    if (!x || (n & 3) || ((uintptr_t)x & 15)) return -CHAM_ERR_ARG;
    if (n == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_acr_relu, dim3(acr_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, x, n / 4);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
extern "C" int cham_acr_act_bwd(float* dy, const float* y, size_t n, int act, void* stream) {
    if (!dy || !y || (n & 3) || ((uintptr_t)dy & 15) || ((uintptr_t)y & 15) || (act != 0 && act != 1)) return -CHAM_ERR_ARG;
    if (n == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_acr_act_bwd, dim3(acr_blocks(n / 4)), dim3(256), 0, (hipStream_t)stream, dy, y, n / 4, act);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
