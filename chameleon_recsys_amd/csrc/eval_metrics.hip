// Beyond-accuracy evaluation metrics on the device (reference nar_module/nar/metrics.py: ExpectedRankSensitiveNovelty :226-266,
// ExpectedRankRelevanceSensitiveNovelty :269-314, ContentExpectedRankRelativeSensitiveIntraListDiversity :513-569,
// ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity :573-641, ItemCoverage :317-343), read straight from what the eval
// step already holds in HBM: the ranked candidate ids (cham_rank_items), the ACE matrix, articles_recent_pop_norm and the recent-clicks
// ring buffer.
//
//   k_eval_beyond_accuracy  one workgroup = one wave = one click.  Lane i < n owns ranked candidate i (n = min(topn, NC) <= 64).  The
//                           n ACE rows are staged through LDS 64 columns at a time (coalesced 256-byte row pieces, any D, 64-bit row
//                           offsets); lane i accumulates the dots <x_i, x_j> for every j in fp32, in column order, so G is exactly
//                           symmetric.  Cosine distance = clip(1 - G_ij / (|x_i| |x_j|), 0, 2) / 2 with a zero norm read as 1
//                           (sklearn's normalize: a zero row stays zero, distance 0.5 to anything; the diagonal is never used).  The
//                           per-rank terms go through LDS and lanes 0..3 sum them in rank order: fixed summation order everywhere,
//                           no atomics, bit-reproducible.  Also marks the coverage maps (top-n ids of the click as recommended, its
//                           label and clicked item as clicked): every writer stores the byte 1.
//   k_cov_seed              clicked map <- the recent-clicks buffer (a 0 included for empty slots, like set(buffer) in the reference).
//   k_cov_partial/_final    byte counts of both maps: per-block partial sums into a workspace, then one block adds them (integers).
//   k_eval_rank_hist        HitRate@n / MRR@n / NDCG@n / HitRate-by-position are functions of ONE integer histogram: how many valid clicks
//                           at session position t had their positive ranked at r (cham_rank_items' label_rank; ranks >= topn share the
//                           last bin).  One workgroup per position t; threads stride over the rows b and count into LDS integers
//                           (integer LDS atomics: order-free).  The global record ACCUMULATES over launches: element (t, r) has exactly
//                           one writer per launch (plain 64-bit read-add-write; launches are stream-ordered).  The fp64 sum of the labels'
//                           normalised popularity has a fixed order - each thread's own strided terms ascending, then a fixed LDS tree -
//                           so two runs are bit-identical.  No float atomics.
#include "common.h"

#define EVAL_MAX_TOPN 64
#define EVAL_TILE 64
#define COV_BLOCKS 256

// 1 / log2(k + 2), the reference's log_rank_discount, rounded to fp32
__constant__ float c_log_disc[EVAL_MAX_TOPN] = {
    1.0f, 0.630929768f, 0.5f, 0.43067655f, 0.386852801f, 0.356207192f, 0.333333343f, 0.315464884f,
    0.30103001f, 0.289064825f, 0.278942943f, 0.270238161f, 0.262649536f, 0.255958021f, 0.25f, 0.244650543f,
    0.239812464f, 0.235408917f, 0.231378213f, 0.227670252f, 0.22424382f, 0.221064731f, 0.218104288f, 0.215338275f,
    0.212746054f, 0.210309923f, 0.208014593f, 0.205846831f, 0.203795046f, 0.201849088f, 0.200000003f, 0.198239863f,
    0.196561635f, 0.194959015f, 0.1934264f, 0.191958725f, 0.190551415f, 0.189200357f, 0.187901825f, 0.186652407f,
    0.185449019f, 0.18428883f, 0.183169246f, 0.182087898f, 0.181042597f, 0.180031329f, 0.179052234f, 0.178103596f,
    0.177183822f, 0.176291436f, 0.175425068f, 0.174583435f, 0.173765346f, 0.172969684f, 0.172195435f, 0.1714416f,
    0.170707285f, 0.169991612f, 0.169293806f, 0.168613106f, 0.167948782f, 0.16730018f, 0.166666672f, 0.166047648f,
};

// NMAX = compile-time bound on n (16 or 64): the size of each lane's dot accumulator array (kept in VGPRs: every loop over j unrolls)
template <int NMAX>
__global__ __launch_bounds__(64) void k_eval_beyond_accuracy(const int64_t* __restrict__ pred_ids, int NC,
                                                             const int64_t* __restrict__ labels, const int64_t* __restrict__ clicked,
                                                             const float* __restrict__ ace, int D, int64_t n_items,
                                                             const float* __restrict__ pop_norm, int n, float rel_pos, float rel_neg,
                                                             float* __restrict__ per_click, uint8_t* __restrict__ rec_map,
                                                             uint8_t* __restrict__ clk_map) {
    __shared__ float tile[NMAX][EVAL_TILE + 1];      // +1: lane i reads row i of a column - no bank conflicts
    __shared__ int64_t s_id[NMAX];
    __shared__ float s_nrm[NMAX], s_rel[NMAX];
    __shared__ float s_term[4][NMAX];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x;
    const int64_t label = labels[c];
    if (clk_map != nullptr) {                        // ItemCoverage: non-zero labels and clicked items of the batch
        if (lane == 0 && label > 0 && label < n_items) clk_map[label] = 1;
        if (lane == 1 && clicked != nullptr) {
            const int64_t ci = clicked[c];
            if (ci > 0 && ci < n_items) clk_map[ci] = 1;
        }
    }
    if (label == 0) {                                // padded position (uniform over the workgroup): zeros, masked out on the host
        if (lane < 4) per_click[c * 4 + lane] = 0.f;
        return;
    }
    int64_t id = 0;
    bool ok = false;
    if (lane < n) {
        id = pred_ids[c * NC + lane];
        ok = id >= 0 && id < n_items;                // (ids outside the table read as a zero row of popularity 1: never in the product path)
        if (ok && rec_map != nullptr) rec_map[id] = 1;
        s_id[lane] = ok ? id : -1;
        s_rel[lane] = id == label ? rel_pos : rel_neg;
    }
    __syncthreads();

    float acc[NMAX];
#pragma unroll
    for (int j = 0; j < NMAX; ++j) acc[j] = 0.f;
    for (int c0 = 0; c0 < D; c0 += EVAL_TILE) {
        const int col = c0 + lane;
#pragma unroll
        for (int r = 0; r < NMAX; ++r) {
            if (r < n) {
                const int64_t rid = s_id[r];
                tile[r][lane] = (rid >= 0 && col < D) ? ace[rid * (int64_t)D + col] : 0.f;
            }
        }
        __syncthreads();
        if (lane < n) {
            const int w = min(EVAL_TILE, D - c0);
            for (int l = 0; l < w; ++l) {
                const float a = tile[lane][l];
#pragma unroll
                for (int j = 0; j < NMAX; ++j)
                    if (j < n) acc[j] = fmaf(a, tile[j][l], acc[j]);
            }
        }
        __syncthreads();
    }

    float nrm = 0.f;
#pragma unroll
    for (int j = 0; j < NMAX; ++j)
        if (j == lane) nrm = sqrtf(acc[j]);
    if (nrm == 0.f) nrm = 1.f;
    if (lane < n) s_nrm[lane] = nrm;
    __syncthreads();

    if (lane < n - 1) {
        const int i = lane;
        float num_r = 0.f, den_r = 0.f, num_rr = 0.f, den_rr = 0.f;
#pragma unroll
        for (int j = 0; j < NMAX; ++j) {
            if (j >= n || j == i) continue;
            const float sim = acc[j] / (nrm * s_nrm[j]);
            const float dist = fminf(fmaxf(1.f - sim, 0.f), 2.f) * 0.5f;
            const float w = c_log_disc[j - i - 1 > 0 ? j - i - 1 : 0];
            num_r += dist * w;                       // EILD-R: every j != i
            den_r += w;
            if (j > i) {                             // EILD-RR: j > i, relevance-weighted numerator and weights
                const float rj = s_rel[j];
                num_rr += dist * w * rj;
                den_rr += w * rj;
            }
        }
        const float wi = c_log_disc[i], ri = s_rel[i];
        const float pop = s_id[i] >= 0 ? pop_norm[s_id[i]] : 1.f;
        const float nov = -log2f(pop);
        s_term[0][i] = nov * wi;
        s_term[1][i] = nov * wi * ri;
        s_term[2][i] = num_r / den_r * wi;
        s_term[3][i] = num_rr / den_rr * wi * ri;    // 0 / 0 = NaN at relevance 0 with no positive at j > i, as in the reference
    }
    __syncthreads();
    if (lane < 4) {
        float num = 0.f, den = 0.f;
        for (int i = 0; i < n - 1; ++i) {            // rank order
            num += s_term[lane][i];
            den += c_log_disc[i];
        }
        per_click[c * 4 + lane] = num / den;
    }
}

__global__ __launch_bounds__(256) void k_cov_seed(const int64_t* __restrict__ buffer_ids, int n_buf, int64_t n_items,
                                                  uint8_t* __restrict__ clk_map) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_buf) return;
    const int64_t id = buffer_ids[k];
    if (id >= 0 && id < n_items) clk_map[id] = 1;
}

// number of non-zero bytes of a 32-bit word
__device__ __forceinline__ uint32_t nz_bytes(uint32_t w) {
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return ((w & 0x01010101u) * 0x01010101u) >> 24;
}

__global__ __launch_bounds__(256) void k_cov_partial(const uint8_t* __restrict__ rec_map, const uint8_t* __restrict__ clk_map,
                                                     int64_t n_items, int64_t* __restrict__ partial) {
    __shared__ int64_t red[2][256];
    const int64_t n16 = n_items / 16;
    int64_t cr = 0, cc = 0;
    const uint4* r4 = reinterpret_cast<const uint4*>(rec_map);
    const uint4* c4 = reinterpret_cast<const uint4*>(clk_map);
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n16; k += (int64_t)gridDim.x * blockDim.x) {
        const uint4 a = r4[k], b = c4[k];
        cr += nz_bytes(a.x) + nz_bytes(a.y) + nz_bytes(a.z) + nz_bytes(a.w);
        cc += nz_bytes(b.x) + nz_bytes(b.y) + nz_bytes(b.z) + nz_bytes(b.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < 16) {       // tail bytes
        const int64_t k = n16 * 16 + threadIdx.x;
        if (k < n_items) {
            cr += rec_map[k] != 0;
            cc += clk_map[k] != 0;
        }
    }
    red[0][threadIdx.x] = cr;
    red[1][threadIdx.x] = cc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) partial[threadIdx.x * COV_BLOCKS + blockIdx.x] = red[threadIdx.x][0];
}

__global__ __launch_bounds__(256) void k_cov_final(const int64_t* __restrict__ partial, int64_t* __restrict__ counts) {
    __shared__ int64_t red[2][COV_BLOCKS];
    red[0][threadIdx.x] = partial[threadIdx.x];
    red[1][threadIdx.x] = partial[COV_BLOCKS + threadIdx.x];
    __syncthreads();
    for (int s = COV_BLOCKS / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x < 2) counts[threadIdx.x] = red[threadIdx.x][0];
}

#define HIST_THREADS 256
#define HIST_MAX_TOPN 256

__global__ __launch_bounds__(HIST_THREADS) void k_eval_rank_hist(const int32_t* __restrict__ label_rank, const int64_t* __restrict__ labels,
                                                                 int B, int T, int topn, const float* __restrict__ pop_norm,
                                                                 int64_t n_items, int64_t* __restrict__ hist, double* __restrict__ pop_sum) {
    __shared__ int s_hist[HIST_MAX_TOPN + 1];
    __shared__ double s_sum[HIST_THREADS];
    const int t = blockIdx.x;                        // < T (the grid), T <= t_cap (checked by the host entry)
    const int tid = threadIdx.x;
    for (int k = tid; k <= topn; k += HIST_THREADS) s_hist[k] = 0;
    __syncthreads();
    double acc = 0.0;
    for (int b = tid; b < B; b += HIST_THREADS) {    // ascending b per thread
        const int64_t at = (int64_t)b * T + t;
        const int r = label_rank[at];
        if (r < 0) continue;                         // padded position
        atomicAdd(&s_hist[r < topn ? r : topn], 1);
        if (pop_norm != nullptr) {
            const int64_t id = labels[at];
            if (id >= 0 && id < n_items) acc += (double)pop_norm[id];
        }
    }
    s_sum[tid] = acc;
    __syncthreads();
    for (int s = HIST_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) s_sum[tid] += s_sum[tid + s];
        __syncthreads();
    }
    int64_t* row = hist + (int64_t)t * (topn + 1);
    for (int k = tid; k <= topn; k += HIST_THREADS) row[k] += (int64_t)s_hist[k];
    if (tid == 0 && pop_norm != nullptr) pop_sum[t] += s_sum[0];
}

extern "C" int cham_eval_rank_hist(const int32_t* label_rank, const int64_t* labels, int B, int T, int topn, const float* pop_norm,
                                   int64_t n_items, int64_t* hist, double* pop_sum, int t_cap, void* stream) {
    if (!label_rank || !labels || !hist || !pop_sum || B < 1 || T < 1 || topn < 1 || topn > HIST_MAX_TOPN || T > t_cap ||
        (pop_norm != nullptr && n_items < 1))
        return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_eval_rank_hist, dim3((unsigned)T), dim3(HIST_THREADS), 0, (hipStream_t)stream, label_rank, labels, B, T, topn,
                       pop_norm, n_items, hist, pop_sum);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_eval_beyond_accuracy(const int64_t* pred_ids, int NC, const int64_t* labels, const int64_t* clicked, int BT,
                                         const float* ace, int D, int64_t n_items, const float* pop_norm, int topn, float rel_pos,
                                         float rel_neg, float* per_click, uint8_t* rec_map, uint8_t* clk_map, void* stream) {
    const int n = topn < NC ? topn : NC;
    if (!pred_ids || !labels || !ace || !pop_norm || !per_click || BT < 0 || NC <= 0 || D <= 0 || n_items <= 0 || n < 2 ||
        n > EVAL_MAX_TOPN || (rec_map == nullptr) != (clk_map == nullptr))
        return -CHAM_ERR_ARG;
    if (BT == 0) return CHAM_OK;
    if (n <= 16)
        hipLaunchKernelGGL(k_eval_beyond_accuracy<16>, dim3((unsigned)BT), dim3(64), 0, (hipStream_t)stream, pred_ids, NC, labels, clicked,
                           ace, D, n_items, pop_norm, n, rel_pos, rel_neg, per_click, rec_map, clk_map);
    else
        hipLaunchKernelGGL(k_eval_beyond_accuracy<64>, dim3((unsigned)BT), dim3(64), 0, (hipStream_t)stream, pred_ids, NC, labels, clicked,
                           ace, D, n_items, pop_norm, n, rel_pos, rel_neg, per_click, rec_map, clk_map);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_eval_coverage_seed(const int64_t* buffer_ids, int n_buf, int64_t n_items, uint8_t* rec_map, uint8_t* clk_map,
                                       void* stream) {
    if (!rec_map || !clk_map || n_items <= 0 || n_buf < 0 || (n_buf > 0 && !buffer_ids)) return -CHAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(rec_map, 0, (size_t)n_items, s) != hipSuccess || hipMemsetAsync(clk_map, 0, (size_t)n_items, s) != hipSuccess)
        return -CHAM_ERR_LAUNCH;
    if (n_buf > 0) {
        hipLaunchKernelGGL(k_cov_seed, dim3((unsigned)((n_buf + 255) / 256)), dim3(256), 0, s, buffer_ids, n_buf, n_items, clk_map);
        CHAM_CHECK_LAUNCH();
    }
    return CHAM_OK;
}

extern "C" size_t cham_eval_coverage_workspace_bytes(int64_t n_items) {
    (void)n_items;
    return (size_t)2 * COV_BLOCKS * sizeof(int64_t);
}

extern "C" int cham_eval_coverage_count(const uint8_t* rec_map, const uint8_t* clk_map, int64_t n_items, void* workspace,
                                        size_t workspace_bytes, int64_t* counts, void* stream) {
    if (!rec_map || !clk_map || !workspace || !counts || n_items <= 0 ||
        workspace_bytes < cham_eval_coverage_workspace_bytes(n_items) || ((uintptr_t)rec_map & 15) || ((uintptr_t)clk_map & 15) ||
        ((uintptr_t)workspace & 7))
        return -CHAM_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int64_t* partial = static_cast<int64_t*>(workspace);
    hipLaunchKernelGGL(k_cov_partial, dim3(COV_BLOCKS), dim3(256), 0, s, rec_map, clk_map, n_items, partial);
    CHAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_cov_final, dim3(1), dim3(COV_BLOCKS), 0, s, partial, counts);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
