// What the baseline recommenders' translation units (baselines.hip, vsknn.hip) share: the cap on a click's candidate columns and the
// candidate row {label} + negatives.
#pragma once
#include "common.h"

#define BL_MAX_NC 1024

__device__ __forceinline__ int64_t cand_id(const int64_t* __restrict__ label_next, const int64_t* __restrict__ neg_ids, int64_t c, int col,
                                           int N) {
    return col == 0 ? label_next[c] : neg_ids[c * N + (col - 1)];
}
