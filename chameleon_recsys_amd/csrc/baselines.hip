// Baseline recommenders of the evaluation on the device (reference nar_module/nar/benchmarks: RecentlyPopularRecommender 'pop_recent',
// ContentBasedRecommender 'cb', ItemCooccurrenceRecommender 'coocurrent', SequentialRulesRecommender 'sr').  Each is a SCORE per
// (click, candidate) over state that already sits in HBM - the recent-popularity histogram, the ACE matrix - or fits a flat table of
// (item, item) -> weight pairs, followed by one ranking of the click's candidates {label} + negatives.  Gather- and latency-bound.
//
//   PAIR TABLE      open addressing in HBM: keys uint64 [cap] ((a << 32) | b, ids >= 1, so 0 = empty slot), vals int64 [cap], cap a power
//                   of two, meta int64 [2] = {dropped inserts, occupied slots}.  Insert = linear probe from mix(key) & (cap - 1); an
//                   empty slot is claimed with a 64-bit atomicCAS on the key, the weight is added with a 64-bit integer atomicAdd.  Keys
//                   never change once set and integer addition commutes: the table's CONTENTS do not depend on scheduling (slot positions
//                   may).  Every probe loop runs at most cap times; an insert that finds no slot counts into meta[0] and returns.
//   k_insert_cooc   one wave = one session row of aci [B, T1]: the ids in [1, n_items) compacted in order into LDS, then +1 for every
//                   DISTINCT ordered id pair of the session, once however often it repeats (scipy's M[rows, cols] += 1 over the
//                   permutations): (a, b), a != b, is represented by the FIRST occurrences of a and b; (a, a) by the SECOND occurrence of a.
//   k_insert_sr     one wave = one session: rules[s_j][s_i] += 2520 / (i - j) for 1 <= i - j <= max_dist (<= 10; 2520 = lcm(1..10): the
//                   reference's 1 / (i - j) 'div' decay as exact integers).
//   k_scores_*      pop_recent / pair: one thread per (click, candidate column); cb: one wave per click, the current item's row and the
//                   candidates' rows staged through LDS 64 columns at a time (coalesced row pieces, any D, 64-bit row offsets); lane i
//                   owns candidate i of a group of 64 and accumulates <x, c_i> and |c_i|^2 in fp32 in column order - the same
//                   instruction sequence for every candidate, so bit-identical rows give bit-identical scores in any column.
//   k_baseline_rank one wave per click, ranking by counting: a candidate is LIVE if it is scored and no earlier column holds the same id
//                   (the reference walks a ranking of unique items); rank = number of live candidates that beat it - larger score, or equal
//                   score and smaller id (live ids are distinct: a strict total order, no ties left).
#include "baselines.h"

#define BL_MAX_T1 1024
#define BL_TILE 64
#define BL_SR_SCALE 2520

enum { BL_POP_RECENT = 0, BL_CB = 1, BL_PAIRS = 2 };

typedef unsigned long long u64;

__device__ __forceinline__ u64 pair_mix(u64 x) {      // splitmix64 finaliser
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__device__ __forceinline__ void pair_add(u64* __restrict__ keys, u64* __restrict__ vals, u64 mask, u64* __restrict__ meta, u64 key, u64 w) {
    const u64 h = pair_mix(key);
    for (u64 i = 0; i <= mask; ++i) {
        const u64 s = (h + i) & mask;
        u64 k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            k = atomicCAS(&keys[s], 0ull, key);
            if (k == 0) {
                atomicAdd(&meta[1], 1ull);
                k = key;
            }
        }
        if (k == key) {
            atomicAdd(&vals[s], w);
            return;
        }
    }
    atomicAdd(&meta[0], 1ull);
}

__device__ __forceinline__ bool pair_find(const u64* __restrict__ keys, const u64* __restrict__ vals, u64 mask, u64 key, int64_t* out) {
    const u64 h = pair_mix(key);
    for (u64 i = 0; i <= mask; ++i) {
        const u64 s = (h + i) & mask;
        const u64 k = keys[s];
        if (k == key) {
            *out = (int64_t)vals[s];
            return true;
        }
        if (k == 0) return false;
    }
    return false;
}

// ids of row b in [1, n_items), in order -> s_id; returns their number (uniform over the wave)
__device__ __forceinline__ int compact_session(const int64_t* __restrict__ aci, int b, int T1, int64_t n_items, int64_t* s_id) {
    const int lane = threadIdx.x;
    int n = 0;
    for (int base = 0; base < T1; base += 64) {
        const int t = base + lane;
        const int64_t id = t < T1 ? aci[(int64_t)b * T1 + t] : 0;
        const bool ok = id >= 1 && id < n_items;
        const u64 m = __ballot(ok);
        if (ok) s_id[n + __popcll(m & ((1ull << lane) - 1ull))] = id;
        n += __popcll(m);
    }
    __syncthreads();
    return n;
}

__global__ __launch_bounds__(64) void k_insert_cooc(const int64_t* __restrict__ aci, int T1, int64_t n_items, u64* __restrict__ keys,
                                                    u64* __restrict__ vals, u64 mask, u64* __restrict__ meta) {
    __shared__ int64_t s_id[BL_MAX_T1];
    __shared__ int s_occ[BL_MAX_T1];                 // earlier positions holding the same id
    const int lane = threadIdx.x;
    const int n = compact_session(aci, blockIdx.x, T1, n_items, s_id);
    for (int p = lane; p < n; p += 64) {
        const int64_t id = s_id[p];
        int occ = 0;
        for (int q = 0; q < p; ++q) occ += s_id[q] == id;
        s_occ[p] = occ;
    }
    __syncthreads();
    for (int p = lane; p < n; p += 64)
        if (s_occ[p] == 1) pair_add(keys, vals, mask, meta, ((u64)s_id[p] << 32) | (u64)s_id[p], 1ull);
    for (int w = lane; w < n * n; w += 64) {
        const int p = w / n, q = w - p * n;
        if (p != q && s_occ[p] == 0 && s_occ[q] == 0) pair_add(keys, vals, mask, meta, ((u64)s_id[p] << 32) | (u64)s_id[q], 1ull);
    }
}

__global__ __launch_bounds__(64) void k_insert_sr(const int64_t* __restrict__ aci, int T1, int max_dist, int64_t n_items,
                                                  u64* __restrict__ keys, u64* __restrict__ vals, u64 mask, u64* __restrict__ meta) {
    __shared__ int64_t s_id[BL_MAX_T1];
    const int n = compact_session(aci, blockIdx.x, T1, n_items, s_id);
    for (int w = threadIdx.x; w < n * max_dist; w += 64) {
        const int i = w / max_dist, dist = w - i * max_dist + 1, j = i - dist;
        if (j >= 0) pair_add(keys, vals, mask, meta, ((u64)s_id[j] << 32) | (u64)s_id[i], (u64)(BL_SR_SCALE / dist));
    }
}

__global__ __launch_bounds__(256) void k_pairs_rehash(const u64* __restrict__ okeys, const u64* __restrict__ ovals, u64 ocap,
                                                      u64* __restrict__ keys, u64* __restrict__ vals, u64 mask, u64* __restrict__ meta) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ocap) return;
    const u64 k = okeys[s];
    if (k != 0) pair_add(keys, vals, mask, meta, k, ovals[s]);
}

__global__ __launch_bounds__(256) void k_pairs_export(const u64* __restrict__ keys, const u64* __restrict__ vals, u64 cap,
                                                      u64* __restrict__ keys_out, u64* __restrict__ vals_out, u64 max_out,
                                                      u64* __restrict__ n_out) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= cap) return;
    const u64 k = keys[s];
    if (k == 0) return;
    const u64 at = atomicAdd(n_out, 1ull);
    if (at < max_out) {
        keys_out[at] = k;
        vals_out[at] = vals[s];
    }
}

__global__ __launch_bounds__(256) void k_scores_int(int kind, const int64_t* __restrict__ item_clicked, const int64_t* __restrict__ label_next,
                                                    const int64_t* __restrict__ neg_ids, int64_t total, int N, int64_t n_items,
                                                    const int32_t* __restrict__ recent_pop, const u64* __restrict__ keys,
                                                    const u64* __restrict__ vals, u64 mask, int64_t* __restrict__ score,
                                                    uint8_t* __restrict__ scored) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const int NC = N + 1;
    const int64_t c = e / NC;
    const int col = (int)(e - c * NC);
    int64_t v = 0;
    bool ok = false;
    if (label_next[c] != 0) {
        const int64_t id = cand_id(label_next, neg_ids, c, col, N);
        if (kind == BL_POP_RECENT) {
            if (id >= 0 && id < n_items) {
                v = recent_pop[id];
                ok = v > 0;
            }
        } else {
            const int64_t item = item_clicked[c];
            if (id >= 1 && id < n_items && item >= 1 && item < n_items) ok = pair_find(keys, vals, mask, ((u64)item << 32) | (u64)id, &v);
        }
    }
    score[e] = ok ? v : 0;
    scored[e] = ok ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_scores_cb(const int64_t* __restrict__ item_clicked, const int64_t* __restrict__ label_next,
                                                  const int64_t* __restrict__ neg_ids, int N, int64_t n_items,
                                                  const float* __restrict__ ace, int D, int64_t ld, float* __restrict__ score,
                                                  uint8_t* __restrict__ scored) {
    __shared__ float tile[BL_TILE][BL_TILE + 1];     // +1: lane i reads row i of a column - no bank conflicts
    __shared__ float s_cur[BL_TILE];
    __shared__ int64_t s_cid[BL_TILE];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x, NC = N + 1;
    const int64_t item = item_clicked[c];
    const bool valid = label_next[c] != 0 && item >= 0 && item < n_items;      // uniform over the wave
    if (!valid) {
        for (int col = lane; col < NC; col += 64) {
            score[c * NC + col] = 0.f;
            scored[c * NC + col] = 0;
        }
        return;
    }
    for (int g0 = 0; g0 < NC; g0 += BL_TILE) {
        const int col = g0 + lane, ng = min(BL_TILE, NC - g0);
        int64_t id = -1;
        if (col < NC) {
            id = cand_id(label_next, neg_ids, c, col, N);
            if (id < 0 || id >= n_items) id = -1;
        }
        __syncthreads();                             // the previous group's readers of s_cid / tile are done
        s_cid[lane] = id;
        __syncthreads();
        float dot = 0.f, nc2 = 0.f, nx2 = 0.f;
        for (int c0 = 0; c0 < D; c0 += BL_TILE) {
            const int k = c0 + lane;
            s_cur[lane] = k < D ? ace[item * ld + k] : 0.f;
            for (int r = 0; r < ng; ++r) {
                const int64_t rid = s_cid[r];
                tile[r][lane] = (rid >= 0 && k < D) ? ace[rid * ld + k] : 0.f;
            }
            __syncthreads();
            if (lane < ng) {
                const int w = min(BL_TILE, D - c0);
                for (int l = 0; l < w; ++l) {        // fixed column order, the same for every candidate
                    const float x = s_cur[l], y = tile[lane][l];
                    dot = fmaf(x, y, dot);
                    nc2 = fmaf(y, y, nc2);
                    nx2 = fmaf(x, x, nx2);
                }
            }
            __syncthreads();
        }
        if (col < NC) {
            float nx = sqrtf(nx2), nc = sqrtf(nc2);  // sklearn's normalize: a zero row stays zero, its similarity is 0
            if (nx == 0.f) nx = 1.f;
            if (nc == 0.f) nc = 1.f;
            score[c * NC + col] = id >= 0 ? dot / (nx * nc) : 0.f;
            scored[c * NC + col] = id >= 0 ? 1 : 0;
        }
    }
}

template <typename S>
__global__ __launch_bounds__(64) void k_baseline_rank(const S* __restrict__ score, const uint8_t* __restrict__ scored,
                                                      const int64_t* __restrict__ label_next, const int64_t* __restrict__ neg_ids, int N,
                                                      int topn, int32_t* __restrict__ label_rank, int64_t* __restrict__ pred_ids) {
    __shared__ int64_t s_id[BL_MAX_NC];
    __shared__ S s_sc[BL_MAX_NC];
    __shared__ uint8_t s_live[BL_MAX_NC];
    const int64_t c = blockIdx.x;
    const int lane = threadIdx.x, NC = N + 1;
    for (int k = lane; k < topn; k += 64) pred_ids[c * topn + k] = 0;
    if (label_next[c] == 0) {                        // padded position (uniform over the wave)
        if (lane == 0) label_rank[c] = -1;
        return;
    }
    for (int col = lane; col < NC; col += 64) {
        s_id[col] = cand_id(label_next, neg_ids, c, col, N);
        s_sc[col] = score[c * NC + col];
        s_live[col] = scored[c * NC + col];
    }
    __syncthreads();
    bool live[BL_MAX_NC / 64];
#pragma unroll
    for (int u = 0; u < BL_MAX_NC / 64; ++u) {
        const int col = u * 64 + lane;
        live[u] = false;
        if (col < NC && s_live[col]) {
            const int64_t id = s_id[col];
            bool first = true;
            for (int q = 0; q < col; ++q) first = first && s_id[q] != id;
            live[u] = first;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < BL_MAX_NC / 64; ++u) {
        const int col = u * 64 + lane;
        if (col < NC) s_live[col] = live[u] ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0 && !s_live[0]) label_rank[c] = NC > topn ? NC : topn;      // unscored label: a miss at every topn
#pragma unroll
    for (int u = 0; u < BL_MAX_NC / 64; ++u) {
        if (!live[u]) continue;
        const int col = u * 64 + lane;
        const int64_t id = s_id[col];
        const S sc = s_sc[col];
        int rank = 0;
        for (int q = 0; q < NC; ++q) {
            if (!s_live[q]) continue;
            const S sq = s_sc[q];
            rank += (sq > sc) || (sq == sc && s_id[q] < id);
        }
        if (rank < topn) pred_ids[c * topn + rank] = id;
        if (col == 0) label_rank[c] = rank;
    }
}

static bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

extern "C" int cham_pairs_insert_cooc(const int64_t* aci, int B, int T1, int64_t n_items, uint64_t* keys, int64_t* vals, int64_t cap,
                                      int64_t* meta, void* stream) {
    if (!aci || !keys || !vals || !meta || B < 0 || T1 < 1 || T1 > BL_MAX_T1 || n_items < 1 || n_items > (1ll << 31) || !pow2(cap))
        return -CHAM_ERR_ARG;
    if (B == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_insert_cooc, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, aci, T1, n_items, (u64*)keys, (u64*)vals,
                       (u64)cap - 1, (u64*)meta);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_pairs_insert_sr(const int64_t* aci, int B, int T1, int max_dist, int64_t n_items, uint64_t* keys, int64_t* vals,
                                    int64_t cap, int64_t* meta, void* stream) {
    if (!aci || !keys || !vals || !meta || B < 0 || T1 < 1 || T1 > BL_MAX_T1 || max_dist < 1 || max_dist > 10 || n_items < 1 ||
        n_items > (1ll << 31) || !pow2(cap))
        return -CHAM_ERR_ARG;
    if (B == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_insert_sr, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, aci, T1, max_dist, n_items, (u64*)keys, (u64*)vals,
                       (u64)cap - 1, (u64*)meta);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_pairs_rehash(const uint64_t* old_keys, const int64_t* old_vals, int64_t old_cap, uint64_t* keys, int64_t* vals,
                                 int64_t cap, int64_t* meta, void* stream) {
    if (!old_keys || !old_vals || !keys || !vals || !meta || !pow2(old_cap) || !pow2(cap) || old_cap > (1ll << 38)) return -CHAM_ERR_ARG;
    hipLaunchKernelGGL(k_pairs_rehash, dim3((unsigned)((old_cap + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)old_keys,
                       (const u64*)old_vals, (u64)old_cap, (u64*)keys, (u64*)vals, (u64)cap - 1, (u64*)meta);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_pairs_export(const uint64_t* keys, const int64_t* vals, int64_t cap, uint64_t* keys_out, int64_t* vals_out,
                                 int64_t max_out, int64_t* n_out, void* stream) {
    if (!keys || !vals || !keys_out || !vals_out || !n_out || !pow2(cap) || cap > (1ll << 38) || max_out < 0) return -CHAM_ERR_ARG;
    if (hipMemsetAsync(n_out, 0, sizeof(int64_t), (hipStream_t)stream) != hipSuccess) return -CHAM_ERR_LAUNCH;
    hipLaunchKernelGGL(k_pairs_export, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const u64*)keys,
                       (const u64*)vals, (u64)cap, (u64*)keys_out, (u64*)vals_out, (u64)max_out, (u64*)n_out);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_baseline_scores(int kind, const int64_t* item_clicked, const int64_t* label_next, const int64_t* neg_ids, int BT, int N,
                                    int64_t n_items, const int32_t* recent_pop, const float* ace, int D, int64_t ace_ld,
                                    const uint64_t* keys, const int64_t* vals, int64_t cap, void* score, uint8_t* scored, void* stream) {
    if (!item_clicked || !label_next || !neg_ids || !score || !scored || BT < 0 || N < 1 || N + 1 > BL_MAX_NC || n_items < 1 ||
        n_items > (1ll << 31))
        return -CHAM_ERR_ARG;
    if (kind == BL_POP_RECENT ? !recent_pop : kind == BL_CB ? (!ace || D < 1 || ace_ld < D) : kind == BL_PAIRS ? (!keys || !vals || !pow2(cap)) : true)
        return -CHAM_ERR_ARG;
    if (BT == 0) return CHAM_OK;
    if (kind == BL_CB) {
        hipLaunchKernelGGL(k_scores_cb, dim3((unsigned)BT), dim3(64), 0, (hipStream_t)stream, item_clicked, label_next, neg_ids, N, n_items,
                           ace, D, ace_ld, (float*)score, scored);
    } else {
        const int64_t total = (int64_t)BT * (N + 1);
        hipLaunchKernelGGL(k_scores_int, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, kind, item_clicked,
                           label_next, neg_ids, total, N, n_items, recent_pop, (const u64*)keys, (const u64*)vals,
                           kind == BL_PAIRS ? (u64)cap - 1 : 0ull, (int64_t*)score, scored);
    }
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_baseline_rank(const void* score, int score_type, const uint8_t* scored, const int64_t* label_next,
                                  const int64_t* neg_ids, int BT, int N, int topn, int32_t* label_rank, int64_t* pred_ids, void* stream) {
    if (!score || !scored || !label_next || !neg_ids || !label_rank || !pred_ids || BT < 0 || N < 1 || N + 1 > BL_MAX_NC || topn < 1 ||
        score_type < 0 || score_type > 2)
        return -CHAM_ERR_ARG;
    if (BT == 0) return CHAM_OK;
    if (score_type == 2)
        hipLaunchKernelGGL(k_baseline_rank<double>, dim3((unsigned)BT), dim3(64), 0, (hipStream_t)stream, (const double*)score, scored,
                           label_next, neg_ids, N, topn, label_rank, pred_ids);
    else if (score_type == 1)
        hipLaunchKernelGGL(k_baseline_rank<float>, dim3((unsigned)BT), dim3(64), 0, (hipStream_t)stream, (const float*)score, scored,
                           label_next, neg_ids, N, topn, label_rank, pred_ids);
    else
        hipLaunchKernelGGL(k_baseline_rank<int64_t>, dim3((unsigned)BT), dim3(64), 0, (hipStream_t)stream, (const int64_t*)score, scored,
                           label_next, neg_ids, N, topn, label_rank, pred_ids);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
