// Top-n prediction for open sessions (NARModuleModel.predict_step): the candidate set of the recent-clicks buffer,
// the candidate chunk the forward pass scores as if it were sampled negatives, and the running top-n / log-sum-exp across chunks.
// No float atomics anywhere: every result is a function of the inputs and of the chunk order 0 .. ceil(K / Nc) - 1 alone.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "common.h"

// ---------------------------------------------------------------------------------------------------
// Candidate set: presence map over the ids, then an ordered compaction by prefix scan (ascending ids).
// A scan block covers PC_ITEMS ids: 256 threads x 16 consecutive ids each.
#define PC_PER_THREAD 16
#define PC_ITEMS (256 * PC_PER_THREAD)

__global__ __launch_bounds__(256) void k_pc_mark(const int64_t* __restrict__ buf, int n, int64_t n_items, unsigned char* __restrict__ presence) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t id = buf[i];
    if (id >= 1 && id < n_items) presence[id] = 1;          // (equal values from several threads: the byte is 1 whoever wins)
}

__device__ __forceinline__ int pc_thread_count(const unsigned char* __restrict__ presence, int64_t n_items, int64_t first) {
    int c = 0;
#pragma unroll
    for (int k = 0; k < PC_PER_THREAD; ++k) {
        const int64_t id = first + k;
        c += (id < n_items && presence[id]) ? 1 : 0;
    }
    return c;
}

// exclusive scan of one int per thread over the 256 threads of the block; returns this thread's offset, *total = the block's sum
__device__ __forceinline__ int block_scan_256(int v, int* sh /*[2][256]*/, int* total) {
    const int t = threadIdx.x;
    int cur = 0;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < 256; o <<= 1) {
        const int x = sh[cur * 256 + t] + (t >= o ? sh[cur * 256 + t - o] : 0);
        sh[(1 - cur) * 256 + t] = x;
        cur = 1 - cur;
        __syncthreads();
    }
    const int incl = sh[cur * 256 + t];
    *total = sh[cur * 256 + 255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void k_pc_count(const unsigned char* __restrict__ presence, int64_t n_items, int32_t* __restrict__ counts) {
    __shared__ int sh[512];
    const int64_t first = (int64_t)blockIdx.x * PC_ITEMS + (int64_t)threadIdx.x * PC_PER_THREAD;
    int total;
    block_scan_256(pc_thread_count(presence, n_items, first), sh, &total);
    if (threadIdx.x == 0) counts[blockIdx.x] = total;
}

// one block: exclusive scan of the nb block counts (tiles of 256 with a running carry), K = their sum
__global__ __launch_bounds__(256) void k_pc_scan(const int32_t* __restrict__ counts, int nb, int32_t* __restrict__ offs, int32_t* __restrict__ K_out) {
    __shared__ int sh[512];
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += 256) {
        const int b = b0 + threadIdx.x;
        const int v = b < nb ? counts[b] : 0;
        int total;
        const int off = block_scan_256(v, sh, &total);
        if (b < nb) offs[b] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) K_out[0] = carry;
}

__global__ __launch_bounds__(256) void k_pc_write(const unsigned char* __restrict__ presence, int64_t n_items, const int32_t* __restrict__ offs,
                                                  int64_t* __restrict__ cand, int64_t cap) {
    __shared__ int sh[512];
    const int64_t first = (int64_t)blockIdx.x * PC_ITEMS + (int64_t)threadIdx.x * PC_PER_THREAD;
    int total;
    int64_t pos = (int64_t)offs[blockIdx.x] + block_scan_256(pc_thread_count(presence, n_items, first), sh, &total);
#pragma unroll
    for (int k = 0; k < PC_PER_THREAD; ++k) {
        const int64_t id = first + k;
        if (id < n_items && presence[id]) {
            if (pos < cap) cand[pos] = id;
            ++pos;
        }
    }
}

static inline size_t pc_al256(size_t x) { return (x + 255) & ~(size_t)255; }
static inline int64_t pc_blocks(int64_t n_items) { return (n_items + PC_ITEMS - 1) / PC_ITEMS; }

extern "C" size_t cham_predict_candidates_workspace_bytes(int64_t n_items) {
    if (n_items <= 0) return 0;
    return pc_al256((size_t)n_items) + 2 * pc_al256((size_t)pc_blocks(n_items) * sizeof(int32_t));
}

extern "C" int cham_predict_candidates(const int64_t* buf_ids, int n, int64_t n_items, int64_t* cand, int64_t cap, int32_t* K_out, void* ws,
                                       size_t ws_bytes, void* stream) {
    if (!cand || !K_out || !ws || n < 0 || (n > 0 && !buf_ids) || n_items <= 0 || n_items > ((int64_t)1 << 31) - PC_ITEMS || cap < 0)
        return -CHAM_ERR_ARG;
    if (ws_bytes < cham_predict_candidates_workspace_bytes(n_items)) return -CHAM_ERR_ARG;
    const int64_t nb = pc_blocks(n_items);
    unsigned char* presence = reinterpret_cast<unsigned char*>(ws);
    int32_t* counts = reinterpret_cast<int32_t*>(presence + pc_al256((size_t)n_items));
    int32_t* offs = reinterpret_cast<int32_t*>(reinterpret_cast<unsigned char*>(counts) + pc_al256((size_t)nb * sizeof(int32_t)));
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(presence, 0, (size_t)n_items, s) != hipSuccess) return -CHAM_ERR_LAUNCH;
    if (n > 0) hipLaunchKernelGGL(k_pc_mark, dim3((n + 255) / 256), dim3(256), 0, s, buf_ids, n, n_items, presence);
    hipLaunchKernelGGL(k_pc_count, dim3((unsigned)nb), dim3(256), 0, s, presence, n_items, counts);
    hipLaunchKernelGGL(k_pc_scan, dim3(1), dim3(256), 0, s, counts, (int)nb, offs, K_out);
    hipLaunchKernelGGL(k_pc_write, dim3((unsigned)nb), dim3(256), 0, s, presence, n_items, offs, cand, cap);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// ---------------------------------------------------------------------------------------------------
// Chunk fill: candidate j Nc + i (the pad item 0 beyond K) as the "negative" i of every prediction row, pool slot i.
__global__ __launch_bounds__(256) void k_pf_fill(const int64_t* __restrict__ cand, const int32_t* __restrict__ K_dev, int j, int Nc, int P, int pmax,
                                                 int64_t* __restrict__ neg_ids, int32_t* __restrict__ neg_slot, int64_t* __restrict__ pool) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t K = K_dev[0];
    if (i < (int64_t)P * Nc) {
        const int c = (int)(i % Nc);
        const int64_t idx = (int64_t)j * Nc + c;
        neg_ids[i] = idx < K ? cand[idx] : 0;
        neg_slot[i] = c;
    }
    if (i < pmax) {
        const int64_t idx = (int64_t)j * Nc + i;
        pool[i] = (i < Nc && idx < K) ? cand[idx] : 0;
    }
}

extern "C" int cham_predict_fill_chunk(const int64_t* cand, const int32_t* K_dev, int j, int Nc, int P, int pmax, int64_t* neg_ids,
                                       int32_t* neg_slot, int64_t* pool, void* stream) {
    if (!cand || !K_dev || !neg_ids || !neg_slot || !pool || j < 0 || Nc <= 0 || P <= 0 || pmax < Nc) return -CHAM_ERR_ARG;
    const int64_t n = (int64_t)P * Nc > pmax ? (int64_t)P * Nc : pmax;
    if ((n + 255) / 256 > 0x7FFFFFFF || (int64_t)(j + 1) * Nc > 0x7FFFFFFF) return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_pf_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cand, K_dev, j, Nc, P, pmax, neg_ids,
                       neg_slot, pool);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// ---------------------------------------------------------------------------------------------------
// Top-n merge.  One wave per prediction row, four rows per workgroup; the chunk is walked in tiles of 64 columns (one per lane).
// A tile's 64 entries and the 64 running entries (rank = lane) are ranked together by counting under the strict order
// (score descending, id ascending, slot ascending): the ranks are a permutation of 0..127, the entries of rank < 64 are the new running
// list.  A masked entry (column 0, pad column, excluded id, non-finite score) is (-inf, 0).  (m, s) = running max and sum of
// exp(score / tau - m) over the non-masked entries, rescaled once per tile: the same sequence of operations whatever the scheduling.
#define PT_MAX_T 128
#define PT_MAX_N 64

__device__ __forceinline__ bool pt_beats(float sa, int64_t ia, int ka, float sb, int64_t ib, int kb) {
    return sa > sb || (sa == sb && (ia < ib || (ia == ib && ka < kb)));
}

__global__ __launch_bounds__(256) void k_pt_merge(const float* __restrict__ logits, const int64_t* __restrict__ cand, const int32_t* __restrict__ K_dev,
                                                  int j, int Nc, const int64_t* __restrict__ excl, int T, int P, int n, float inv_tau,
                                                  int64_t* __restrict__ top_id, float* __restrict__ top_score, float* __restrict__ ms) {
    __shared__ int64_t s_ex[4][PT_MAX_T];
    __shared__ int64_t s_id[4][128];
    __shared__ float s_sc[4][128];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row_raw = blockIdx.x * 4 + w;
    const bool live = row_raw < P;
    const int row = live ? row_raw : P - 1;          // (a wave beyond the last row repeats it and stores nothing: every wave reaches every barrier)
    const int64_t K = K_dev[0];
    for (int t = lane; t < T; t += 64) s_ex[w][t] = excl[(size_t)row * T + t];
    float tsc = lane < n ? top_score[(size_t)row * n + lane] : -INFINITY;
    int64_t tid = lane < n ? top_id[(size_t)row * n + lane] : 0;
    float m = ms[(size_t)row * 2], s = ms[(size_t)row * 2 + 1];
    __syncthreads();
    const float* lrow = logits + (size_t)row * (Nc + 1) + 1;
    for (int c0 = 0; c0 < Nc; c0 += 64) {
        const int c = c0 + lane;
        const int64_t idx = (int64_t)j * Nc + c;
        bool valid = c < Nc && idx < K;
        int64_t id = valid ? cand[idx] : 0;
        float x = valid ? lrow[c] : -INFINITY;
        if (!(x > -INFINITY) || !(x < INFINITY)) valid = false;
        for (int t = 0; t < T; ++t) valid = valid && s_ex[w][t] != id;
        if (!valid) { x = -INFINITY; id = 0; }
        // log-sum-exp over the non-masked entries
        const float xs = x * inv_tau;
        const float tmax = wave_max(valid ? xs : -INFINITY);
        if (tmax > -INFINITY) {                      // (wave-uniform)
            const float m_new = fmaxf(m, tmax);
            const float ts = wave_sum(valid ? expf(xs - m_new) : 0.f);
            s = (m > -INFINITY ? s * expf(m - m_new) : 0.f) + ts;
            m = m_new;
        }
        // rank the 128 entries by counting
        s_sc[w][lane] = tsc; s_id[w][lane] = tid;
        s_sc[w][64 + lane] = x; s_id[w][64 + lane] = id;
        __syncthreads();
        int ra = 0, rb = 0;
        for (int k = 0; k < 128; ++k) {
            const float sk = s_sc[w][k];
            const int64_t ik = s_id[w][k];
            ra += pt_beats(sk, ik, k, tsc, tid, lane) ? 1 : 0;
            rb += pt_beats(sk, ik, k, x, id, 64 + lane) ? 1 : 0;
        }
        __syncthreads();
        if (ra < 64) { s_sc[w][ra] = tsc; s_id[w][ra] = tid; }
        if (rb < 64) { s_sc[w][rb] = x; s_id[w][rb] = id; }
        __syncthreads();
        tsc = s_sc[w][lane]; tid = s_id[w][lane];
        __syncthreads();
    }
    if (live) {
        if (lane < n) { top_score[(size_t)row * n + lane] = tsc; top_id[(size_t)row * n + lane] = tid; }
        if (lane == 0) { ms[(size_t)row * 2] = m; ms[(size_t)row * 2 + 1] = s; }
    }
}

extern "C" int cham_predict_topn_merge(const float* logits, const int64_t* cand, const int32_t* K_dev, int j, int Nc, const int64_t* excl, int T,
                                       int P, int n, float softmax_temperature, int64_t* top_id, float* top_score, float* ms, void* stream) {
    if (!logits || !cand || !K_dev || !top_id || !top_score || !ms || j < 0 || Nc <= 0 || P <= 0 || n < 1 || n > PT_MAX_N || T < 0 ||
        T > PT_MAX_T || (T > 0 && !excl) || !(softmax_temperature > 0.f) || (int64_t)(j + 1) * Nc > 0x7FFFFFFF)
        return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_pt_merge, dim3((P + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, cand, K_dev, j, Nc, excl, T, P, n,
                       1.f / softmax_temperature, top_id, top_score, ms);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

__global__ __launch_bounds__(256) void k_pt_finish(const float* __restrict__ top_score, const float* __restrict__ ms, int P, int n, float inv_tau,
                                                   float* __restrict__ probs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P * n) return;
    const int row = i / n;
    const float x = top_score[i], m = ms[(size_t)row * 2], s = ms[(size_t)row * 2 + 1];
    probs[i] = (x > -INFINITY && s > 0.f) ? expf(x * inv_tau - m) / s : 0.f;
}

extern "C" int cham_predict_topn_finish(const float* top_score, const float* ms, int P, int n, float softmax_temperature, float* probs,
                                        void* stream) {
    if (!top_score || !ms || !probs || P <= 0 || n < 1 || n > PT_MAX_N || !(softmax_temperature > 0.f)) return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_pt_finish, dim3((P * n + 255) / 256), dim3(256), 0, (hipStream_t)stream, top_score, ms, P, n,
                       1.f / softmax_temperature, probs);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
