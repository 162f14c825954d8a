// Full-candidate evaluation (--eval_full_candidates; nar/full_eval.py): the rank of every valid click's label among
// ALL recent candidates, accumulated over the chunks the forward pass scores them in.  Integer bookkeeping only (ballot + popcount into
// two counters per row): no float arithmetic, no atomics - the sums do not depend on any order and two runs are bit-identical.
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>

#include "common.h"

#define EF_MAX_T1 128

// One wave per row, four rows per workgroup; the chunk is walked in tiles of 64 columns (one per lane).  Column c of chunk j is candidate
// idx = j Nc + c; columns with idx >= K are skipped.  A candidate COMPETES with the row's label l unless it is l itself or occurs in the
// session's aci row (the sampler's per-session set difference); a competitor BEATS the label unless z_c < z_l or (z_c == z_l and c > l):
// the negation puts every NaN (on either side) against the label.
__global__ __launch_bounds__(256) void k_ef_merge(const float* __restrict__ logits, const int64_t* __restrict__ cand, const int32_t* __restrict__ K_dev,
                                                  int j, int Nc, const int64_t* __restrict__ labels, const int32_t* __restrict__ row_session,
                                                  const int64_t* __restrict__ aci, int T1, int R, int32_t* __restrict__ beat,
                                                  int32_t* __restrict__ competitors) {
    __shared__ int64_t s_ex[4][EF_MAX_T1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int row_raw = blockIdx.x * 4 + w;
    const bool live = row_raw < R;
    const int row = live ? row_raw : R - 1;          // (a wave beyond the last row repeats it and stores nothing: every wave reaches the barrier)
    const int64_t K = K_dev[0];
    const int64_t sess = row_session[row];
    for (int t = lane; t < T1; t += 64) s_ex[w][t] = aci[(size_t)sess * T1 + t];
    __syncthreads();
    const int64_t l = labels[row];
    const float* lrow = logits + (size_t)row * (Nc + 1);
    const float zl = lrow[0];
    int n_beat = 0, n_comp = 0;
    for (int c0 = 0; c0 < Nc; c0 += 64) {
        const int c = c0 + lane;
        const int64_t idx = (int64_t)j * Nc + c;
        const bool valid = c < Nc && idx < K;
        const int64_t id = valid ? cand[idx] : 0;
        const float z = valid ? lrow[1 + c] : 0.f;
        bool comp = valid && id != l;
        for (int t = 0; t < T1; ++t) comp = comp && s_ex[w][t] != id;
        const bool below = z < zl || (z == zl && id > l);
        n_comp += __popcll(__ballot(comp));
        n_beat += __popcll(__ballot(comp && !below));
    }
    if (live && lane == 0) {
        beat[row] += n_beat;
        competitors[row] += n_comp;
    }
}

extern "C" int cham_eval_full_rank_merge(const float* logits, const int64_t* cand, const int32_t* K_dev, int j, int Nc, const int64_t* labels,
                                         const int32_t* row_session, const int64_t* aci, int T1, int R, int32_t* beat, int32_t* competitors,
                                         void* stream) {
    if (!logits || !cand || !K_dev || !labels || !row_session || !aci || !beat || !competitors || j < 0 || Nc <= 0 || R <= 0 || T1 < 1 ||
        T1 > EF_MAX_T1 || (int64_t)(j + 1) * Nc > 0x7FFFFFFF)
        return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_ef_merge, dim3((R + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, cand, K_dev, j, Nc, labels, row_session, aci,
                       T1, R, beat, competitors);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// The block's first R_valid rows (the rest is padding) to their (b, t): rows[i] = b T + t.
__global__ __launch_bounds__(256) void k_ef_scatter(const int32_t* __restrict__ beat, const int32_t* __restrict__ competitors,
                                                    const int32_t* __restrict__ rows, int R_valid, int32_t* __restrict__ label_rank,
                                                    int32_t* __restrict__ n_comp) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R_valid) return;
    const int at = rows[i];
    label_rank[at] = beat[i];
    n_comp[at] = competitors[i];
}

extern "C" int cham_eval_full_rank_scatter(const int32_t* beat, const int32_t* competitors, const int32_t* rows, int R_valid, int32_t* label_rank,
                                           int32_t* n_comp, void* stream) {
    if (!beat || !competitors || !rows || !label_rank || !n_comp || R_valid <= 0) return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_ef_scatter, dim3((R_valid + 255) / 256), dim3(256), 0, (hipStream_t)stream, beat, competitors, rows, R_valid,
                       label_rank, n_comp);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
