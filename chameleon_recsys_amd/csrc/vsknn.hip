// V-SkNN baseline of the evaluation on the device (reference nar_module/nar/benchmarks/session_knn.py, SessionBasedKNNRecommender in the
// trainers' configuration: cosine similarity, 'div' decay of the active session's clicks, 'recent' sampling).
//
//   SESSION RING    the last S sessions in HBM: items int32 [S, L] (a session's DISTINCT ids in [1, n_items), in order of first occurrence),
//                   lens int32 [S], ids int64 [S] (session ids), order int32 [S] = the slots by session id descending (slot ascending among
//                   equal ids: a permutation).  Row r of a batch goes to slot (appended + r) mod S, `appended` counted on the host: no
//                   read-back, no atomics.  A slot never written has length 0 and matches nothing, like a session without a valid id.
//   k_vsknn_append  one wave per batch row (only the last S rows of a batch larger than the ring: one writer per slot).
//   k_vsknn_order   one thread per slot: its rank among the S session ids by counting (ids staged in LDS).
//   k_vsknn_scores  one workgroup per session row b.  Once per row: a 64-bit HIT MASK per buffered session over the row's click positions
//                   (bit p = item_clicked[b, p] is in the session), in LDS, in `order` (position j = the j-th largest session id).  Then per
//                   click t, over the masked word w = mask & bits 0..t:
//                     m = popcount(w) copies of the session in the reference's candidate list; decay = sum of 1 / (t - p + 1) over the set
//                     bits from p = t downwards; sim = decay / (sqrt(a) * sqrt(len)), a = distinct ids of item_clicked[b, 0..t]
//                     sample cut   (sum m > sample): k = clamp(sample - copies of the sessions ahead in id order, 0, m): a block prefix sum
//                     neighbours   of the sessions with k > 0 and 0 < sim < 1; if their copies exceed knn, the similarity theta of copy
//                                  number knn in (sim descending, id descending) order by bisection over the doubles' bit patterns (one
//                                  workgroup sum per step), then n = k above theta, 0 below, and at theta what is left, in id order
//                     score(c) = sum over the sessions with n > 0, in id order, of n * sim * [c in session]: a wave per candidate column,
//                                  its lanes across 64 neighbours whose ids sit in registers; a ballot yields the holders in id order
//                   float64 throughout, every operation rounded to nearest on its own (no contraction), every sum in a fixed order, no
//                   atomics: equal (decay, a, len) give equal sim bits, `sim < 1.0` decides as the reference's Python does, and the same
//                   inputs give the same bits.
#include "baselines.h"

#pragma clang fp contract(off)

#define VS_MAX_T 64
#define VS_MAX_L 65            /* ids of a ring row: T clicks + the last label */
#define VS_MAX_S 4096
#define VS_THREADS 256
#define VS_REG 32              /* ids of a neighbour session held in registers while the candidates are matched (longer ones: re-read) */

typedef unsigned long long u64;

__global__ __launch_bounds__(64) void k_vsknn_append(const int64_t* __restrict__ aci, const int64_t* __restrict__ session_ids, int first_row,
                                                     int T1, int64_t n_items, int64_t appended, int S, int L, int32_t* __restrict__ items,
                                                     int32_t* __restrict__ lens, int64_t* __restrict__ ids) {
    __shared__ int64_t s_id[2 * 64];
    __shared__ int64_t s_u[2 * 64];
    const int lane = threadIdx.x;
    const int r = first_row + blockIdx.x;
    const int slot = (int)((appended + r) % S);
    int n = 0;
    for (int base = 0; base < T1; base += 64) {      // the ids in [1, n_items), in order
        const int t = base + lane;
        const int64_t id = t < T1 ? aci[(int64_t)r * T1 + t] : 0;
        const bool ok = id >= 1 && id < n_items;
        const u64 m = __ballot(ok);
        if (ok) s_id[n + __popcll(m & ((1ull << lane) - 1ull))] = id;
        n += __popcll(m);
    }
    __syncthreads();
    int nu = 0;
    for (int base = 0; base < n; base += 64) {       // ... their first occurrences
        const int p = base + lane;
        bool first = p < n;
        if (first) {
            const int64_t id = s_id[p];
            for (int q = 0; q < p; ++q) first = first && s_id[q] != id;
        }
        const u64 m = __ballot(first);
        if (first) s_u[nu + __popcll(m & ((1ull << lane) - 1ull))] = s_id[p];
        nu += __popcll(m);
    }
    __syncthreads();
    if (nu > L) nu = L;                              // (unreachable: T1 <= L)
    for (int i = lane; i < L; i += 64) items[(int64_t)slot * L + i] = i < nu ? (int32_t)s_u[i] : 0;
    if (lane == 0) {
        lens[slot] = nu;
        ids[slot] = session_ids[r];
    }
}

__global__ __launch_bounds__(VS_THREADS) void k_vsknn_order(const int64_t* __restrict__ ids, int S, int32_t* __restrict__ order) {
    __shared__ int64_t s_ids[VS_MAX_S];
    for (int s = threadIdx.x; s < S; s += VS_THREADS) s_ids[s] = ids[s];
    __syncthreads();
    const int s = blockIdx.x * VS_THREADS + threadIdx.x;
    if (s >= S) return;
    const int64_t id = s_ids[s];
    int rank = 0;
    for (int q = 0; q < S; ++q) {
        const int64_t o = s_ids[q];
        rank += (o > id) || (o == id && q < s);
    }
    order[rank] = s;
}

// exclusive prefix sum of v over the workgroup's threads in thread order; *total = the sum (every thread).  s_w: 4 ints of LDS.
__device__ __forceinline__ int vs_block_scan(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();                                 // the previous scan's readers of s_w are done
    if (lane == 63) s_w[w] = inc;
    __syncthreads();
    int off = 0, sum = 0;
#pragma unroll
    for (int i = 0; i < VS_THREADS / 64; ++i) {
        const int x = s_w[i];
        off += i < w ? x : 0;
        sum += x;
    }
    *total = sum;
    return off + inc - v;
}

__global__ __launch_bounds__(VS_THREADS) void k_vsknn_scores(const int64_t* __restrict__ item_clicked, const int64_t* __restrict__ label_next,
                                                             const int64_t* __restrict__ neg_ids, int T, int N,
                                                             const int32_t* __restrict__ items, const int32_t* __restrict__ lens,
                                                             const int32_t* __restrict__ order, int S, int L, int sample, int knn,
                                                             double* __restrict__ score, uint8_t* __restrict__ scored,
                                                             double* __restrict__ sim_out, int32_t* __restrict__ n_out) {
    __shared__ u64 s_mask[VS_MAX_S];                 // position j of the id order: hit mask over the row's click positions
    __shared__ double s_sim[VS_MAX_S];
    __shared__ uint16_t s_slot[VS_MAX_S];
    __shared__ uint16_t s_list[VS_MAX_S];            // the neighbours' positions, compacted
    __shared__ uint8_t s_len[VS_MAX_S];
    __shared__ uint8_t s_k[VS_MAX_S];                // copies after the sample cut (m <= T <= 64 fits)
    __shared__ uint8_t s_n[VS_MAX_S];                // copies after the neighbour cut
    __shared__ double s_acc[BL_MAX_NC];              // a click's candidate columns: score, scored, id (0 = outside the item ids)
    __shared__ int32_t s_cid[BL_MAX_NC];
    __shared__ uint8_t s_hit[BL_MAX_NC];
    __shared__ int64_t s_item[VS_MAX_T];
    __shared__ int s_a[VS_MAX_T];
    __shared__ double s_inv[VS_MAX_T];               // 1 / (distance + 1): the 'div' decay
    __shared__ int s_w[VS_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, NC = N + 1;

    if (tid < T) s_item[tid] = item_clicked[(int64_t)b * T + tid];
    __syncthreads();
    if (tid < T) {                                   // a(t) = distinct values of item_clicked[b, 0..t]
        int a = 0;
        for (int p = 0; p <= tid; ++p) {
            bool first = true;
            for (int q = 0; q < p; ++q) first = first && s_item[q] != s_item[p];
            a += first;
        }
        s_a[tid] = a;
        s_inv[tid] = __ddiv_rn(1.0, (double)(tid + 1));
    }
    for (int j = tid; j < S; j += VS_THREADS) {
        int slot = order[j];
        int len = 0;
        if (slot < 0 || slot >= S) slot = 0;         // (a ring whose order was never built: nothing matches)
        else len = min(max(lens[slot], 0), L);
        u64 mask = 0;
        for (int i = 0; i < len; ++i) {
            const int64_t id = items[(int64_t)slot * L + i];
            for (int p = 0; p < T; ++p) mask |= (u64)(s_item[p] == id) << p;
        }
        s_mask[j] = mask;
        s_slot[j] = (uint16_t)slot;
        s_len[j] = (uint8_t)len;
    }
    __syncthreads();

    const int chunk = (S + VS_THREADS - 1) / VS_THREADS;     // thread tid owns positions [j0, j1) through every per-click pass
    const int j0 = min(S, tid * chunk), j1 = min(S, j0 + chunk);
    for (int t = 0; t < T; ++t) {
        const int64_t c = (int64_t)b * T + t;
        if (s_item[t] == 0) {                        // no click at this position (uniform over the workgroup): nothing scored
            for (int col = tid; col < NC; col += VS_THREADS) {
                score[c * NC + col] = 0.0;
                scored[c * NC + col] = 0;
            }
            if (sim_out)
                for (int s = tid; s < S; s += VS_THREADS) {
                    sim_out[c * S + s] = 0.0;
                    n_out[c * S + s] = 0;
                }
            continue;
        }
        const u64 low = t == 63 ? ~0ull : (1ull << (t + 1)) - 1ull;
        // copies m per session, then the sample cut in id order
        int msum = 0;
        for (int j = j0; j < j1; ++j) {
            const int m = __popcll(s_mask[j] & low);
            s_k[j] = (uint8_t)m;
            msum += m;
        }
        int M;
        const int ahead_m = vs_block_scan(msum, s_w, &M);
        if (M > sample) {
            int run = ahead_m;
            for (int j = j0; j < j1; ++j) {
                const int m = s_k[j];
                s_k[j] = (uint8_t)max(0, min(m, sample - run));
                run += m;
            }
        }
        // similarities; only 0 < sim < 1 stays a neighbour candidate
        const double sqa = __dsqrt_rn((double)s_a[t]);
        int ksum = 0;
        for (int j = j0; j < j1; ++j) {
            u64 w = s_mask[j] & low;
            double sim = 0.0;
            if (w) {
                double decay = 0.0;
                while (w) {                          // from p = t downwards
                    const int p = 63 - __clzll((long long)w);
                    decay = __dadd_rn(decay, s_inv[t - p]);
                    w &= ~(1ull << p);
                }
                sim = __ddiv_rn(decay, __dmul_rn(sqa, __dsqrt_rn((double)s_len[j])));
            }
            s_sim[j] = sim;
            const bool elig = s_k[j] > 0 && sim > 0.0 && sim < 1.0;
            if (!elig) s_k[j] = 0;
            ksum += s_k[j];
        }
        int K;
        vs_block_scan(ksum, s_w, &K);
        if (K <= knn) {
            for (int j = j0; j < j1; ++j) s_n[j] = s_k[j];
        } else {
            // The cut.  In (sim descending, id descending) order the copy number knn has the similarity theta: sessions above theta keep
            // their copies, sessions below lose them, the sessions AT theta share what is left in id order.  A positive double orders as
            // its bit pattern, so theta is the largest pattern v with copies(sim >= v) >= knn: a bisection of [0, bits(1.0)) whose every
            // step is one workgroup sum over this thread's positions, held in registers.
            u64 key[VS_MAX_S / VS_THREADS];
            int kk[VS_MAX_S / VS_THREADS];
#pragma unroll
            for (int i = 0; i < VS_MAX_S / VS_THREADS; ++i) {
                const int j = j0 + i;
                kk[i] = j < j1 ? (int)s_k[j] : 0;
                key[i] = j < j1 ? (u64)__double_as_longlong(s_sim[j]) : 0ull;
            }
            u64 lo = 0ull, hi = 0x3FF0000000000000ull;       // copies(sim >= lo) = K > knn; no neighbour candidate reaches 1.0
            while (hi - lo > 1ull) {
                const u64 mid = lo + ((hi - lo) >> 1);
                int cnt = 0, total;
#pragma unroll
                for (int i = 0; i < VS_MAX_S / VS_THREADS; ++i) cnt += key[i] >= mid ? kk[i] : 0;
                vs_block_scan(cnt, s_w, &total);
                if (total >= knn) lo = mid;
                else hi = mid;
            }
            int above = 0, at = 0, total_above;
#pragma unroll
            for (int i = 0; i < VS_MAX_S / VS_THREADS; ++i) {
                above += key[i] > lo ? kk[i] : 0;
                at += key[i] == lo ? kk[i] : 0;
            }
            vs_block_scan(above, s_w, &total_above);
            int unused;
            int run = vs_block_scan(at, s_w, &unused);        // copies at theta ahead of this thread's positions, in id order
            const int left = knn - total_above;
#pragma unroll
            for (int i = 0; i < VS_MAX_S / VS_THREADS; ++i) {
                const int j = j0 + i;
                if (j < j1) {
                    int n = key[i] > lo ? kk[i] : 0;
                    if (key[i] == lo) {
                        n = max(0, min(kk[i], left - run));
                        run += kk[i];
                    }
                    s_n[j] = (uint8_t)n;
                }
            }
        }
        __syncthreads();
        // the neighbours (n > 0) compacted in id order
        int ncnt = 0;
        for (int j = j0; j < j1; ++j) ncnt += s_n[j] > 0;
        int NN;
        int e = vs_block_scan(ncnt, s_w, &NN);
        for (int j = j0; j < j1; ++j)
            if (s_n[j]) s_list[e++] = (uint16_t)j;
        __syncthreads();
        // candidate scores: 64 neighbours at a time, a lane holding one neighbour's ids in registers; wave w owns the columns w, w + 4, ...:
        // the neighbours that hold a column's id come out of a ballot in id order and lane 0 adds their n * sim in that order
        for (int col = tid; col < NC; col += VS_THREADS) {
            const int64_t id = cand_id(label_next, neg_ids, c, col, N);
            s_cid[col] = (id >= 1 && id < (1ll << 31)) ? (int32_t)id : 0;        // 0: matches no buffered id
            s_acc[col] = 0.0;
            s_hit[col] = 0;
        }
        __syncthreads();
        {
            const int lane = tid & 63, wv = tid >> 6;
            for (int x0 = 0; x0 < NN; x0 += 64) {
                const int x = x0 + lane;
                int32_t r[VS_REG];
                const int32_t* row = items;
                int len = 0;
                if (x < NN) {
                    const int j = s_list[x];
                    row = items + (int64_t)s_slot[j] * L;
                    len = s_len[j];
                }
#pragma unroll
                for (int i = 0; i < VS_REG; ++i) r[i] = i < len ? row[i] : -1;
                for (int col = wv; col < NC; col += VS_THREADS / 64) {
                    const int32_t id = s_cid[col];
                    bool in = false;
#pragma unroll
                    for (int i = 0; i < VS_REG; ++i) in = in || r[i] == id;
                    for (int i = VS_REG; i < len; ++i) in = in || row[i] == id;
                    u64 mk = __ballot(in);
                    if (mk && lane == 0) {
                        double acc = s_acc[col];
                        while (mk) {
                            const int j = s_list[x0 + __builtin_ctzll(mk)];
                            acc = __dadd_rn(acc, __dmul_rn((double)s_n[j], s_sim[j]));
                            mk &= mk - 1;
                        }
                        s_acc[col] = acc;
                        s_hit[col] = 1;
                    }
                }
            }
        }
        __syncthreads();
        for (int col = tid; col < NC; col += VS_THREADS) {
            score[c * NC + col] = s_acc[col];
            scored[c * NC + col] = s_hit[col];
        }
        if (sim_out)
            for (int j = j0; j < j1; ++j) {
                sim_out[c * S + s_slot[j]] = s_sim[j];
                n_out[c * S + s_slot[j]] = s_n[j];
            }
        __syncthreads();                             // s_k / s_n / s_list are rewritten for the next click
    }
}

extern "C" int cham_vsknn_append(const int64_t* aci, const int64_t* session_ids, int B, int T1, int64_t n_items, int64_t appended, int S,
                                 int L, int32_t* items, int32_t* lens, int64_t* ids, int32_t* order, void* stream) {
    if (!aci || !session_ids || !items || !lens || !ids || !order || B < 0 || T1 < 1 || L < T1 || L > VS_MAX_L || S < 1 || S > VS_MAX_S ||
        n_items < 1 || n_items > (1ll << 31) || appended < 0)
        return -CHAM_ERR_ARG;
    if (B == 0) return CHAM_OK;
    const int first_row = B > S ? B - S : 0;         // of more than S rows only the last S remain
    hipLaunchKernelGGL(k_vsknn_append, dim3((unsigned)(B - first_row)), dim3(64), 0, (hipStream_t)stream, aci, session_ids, first_row, T1,
                       n_items, appended, S, L, items, lens, ids);
    CHAM_CHECK_LAUNCH();
    hipLaunchKernelGGL(k_vsknn_order, dim3((unsigned)((S + VS_THREADS - 1) / VS_THREADS)), dim3(VS_THREADS), 0, (hipStream_t)stream, ids, S,
                       order);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_vsknn_scores(const int64_t* item_clicked, const int64_t* label_next, const int64_t* neg_ids, int B, int T, int N,
                                 const int32_t* items, const int32_t* lens, const int32_t* order, int S, int L, int sample, int knn,
                                 double* score, uint8_t* scored, double* sim_out, int32_t* n_out, void* stream) {
    if (!item_clicked || !label_next || !neg_ids || !items || !lens || !order || !score || !scored || B < 0 || T < 1 || T > VS_MAX_T ||
        N < 1 || N + 1 > BL_MAX_NC || S < 1 || S > VS_MAX_S || L < 1 || L > VS_MAX_L || sample < 1 || knn < 1 || (!sim_out != !n_out))
        return -CHAM_ERR_ARG;
    if (B == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_vsknn_scores, dim3((unsigned)B), dim3(VS_THREADS), 0, (hipStream_t)stream, item_clicked, label_next, neg_ids, T, N,
                       items, lens, order, S, L, sample, knn, score, scored, sim_out, n_out);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
