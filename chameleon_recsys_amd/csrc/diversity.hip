// Content-diversity regulariser (--diversity_reg_factor): the loss the reference states in its commented-out block
// (nar_model.py:551-636, 685-702), restated per click.  For a valid click with candidates c = 0..N (0 the label, 1..N the sampled
// negatives), ids id_c and p = softmax(logits / tau):
//   e^_c  = ACE[id_c] * 1 / sqrt(max(sum_d ACE[id_c,d]^2, 1e-12))                   (tf.nn.l2_normalize, :563)
//   S_cc' = e^_c . e^_c' where id_c != id_c', 0 where the ids are equal               (:572-574: the diagonal of the UNIQUE-id matrix)
//   e     = p^T S p;   loss term = factor * sum(mask e) / sum(mask)                   (:620-630, 689, 696-698)
// S is never formed: (S p)_c = e^_c . m - |e^_c|^2 * sum_{c': id_c' = id_c} p_c' with m = sum_c' p_c' e^_c' - O(NC D) per click.
// The ACE matrix is not trainable; the only gradient is d/d logit_c = factor * mask / (tau sum(mask)) * 2 p_c ((S p)_c - e).
//
// Every sum has a fixed order (lane-private partial sums, butterfly wave sums, a fixed tree over the four waves): no atomics, two runs
// are bit-identical.
#include "common.h"

#define DIV_THREADS 256
#define DIV_WAVES (DIV_THREADS / 64)
#define DIV_MAX_LDS (160 * 1024)      /* a CU's LDS: D up to ~8 000 at NC = 101 */

// One workgroup per click; wave w owns the candidates c = w, w + 4, ... .  A row of the table is read as float4 pieces (lane k: columns
// 4k .. 4k+3 of each 256-column chunk) where the base and the row stride allow 16-byte accesses, the columns beyond the last whole piece -
// or all of them - one per lane.  Pass 1 reads a candidate's row for its norm and adds p_c r_c ACE[id_c] to the wave's partial m (lane-private
// LDS columns); pass 2 reads the row again (from L2: the workgroup has just read it) for e^_c . m.  The row offset is 64-bit: id * ld
// exceeds 2^31 elements for the 5 M-article table.  An id outside [0, n_items) gathers nothing and counts as an all-zero row.
// Dynamic LDS: ids [NC] int64 | p, r, q, t [NC] float each | m partial sums [DIV_WAVES][D] | m [D] | red [DIV_WAVES].
__global__ __launch_bounds__(DIV_THREADS) void k_diversity_fwd(const float* __restrict__ probs, const int64_t* __restrict__ label_ids,
                                                               const int64_t* __restrict__ neg_ids, const unsigned char* __restrict__ mask,
                                                               int N, const float* __restrict__ ace, int ld, int D, int64_t n_items,
                                                               int vec /* float4 pieces per row */, float factor, float* __restrict__ sp,
                                                               float* __restrict__ e_out, float* __restrict__ nll) {
    extern __shared__ __align__(16) unsigned char div_lds[];
    const int NC = N + 1, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t bt = blockIdx.x;
    if (!mask[bt]) {                                      // (uniform over the workgroup) nothing gathered, nll untouched
        for (int c = tid; c < NC; c += DIV_THREADS) sp[bt * NC + c] = 0.f;
        if (tid == 0) e_out[bt] = 0.f;
        return;
    }
    int64_t* ids = reinterpret_cast<int64_t*>(div_lds);
    float* p = reinterpret_cast<float*>(ids + NC);
    float* r = p + NC;            // 1 / sqrt(max(|row|^2, 1e-12))
    float* q = r + NC;            // |e^_c|^2 = |row|^2 r^2 (1 for every row of norm^2 >= 1e-12, up to roundoff)
    float* t = q + NC;            // e^_c . m
    float* mw = t + NC;           // [DIV_WAVES][D]
    float* m = mw + (size_t)DIV_WAVES * D;
    float* red = m + D;
    for (int c = tid; c < NC; c += DIV_THREADS) {
        ids[c] = c == 0 ? label_ids[bt] : neg_ids[bt * N + (c - 1)];
        p[c] = probs[bt * NC + c];
    }
    for (int d = tid; d < DIV_WAVES * D; d += DIV_THREADS) mw[d] = 0.f;
    __syncthreads();
    const int tail0 = 4 * vec;                            // first column of the one-per-lane part
    float* mine = mw + (size_t)w * D;
    // pass 1: norms, and m in four partial sums
    for (int c = w; c < NC; c += DIV_WAVES) {
        const int64_t id = ids[c];
        const bool in = id >= 0 && id < n_items;
        const float* row = ace + (in ? (size_t)id * (size_t)ld : (size_t)0);
        float ss = 0.f;
        float4 first = make_float4(0.f, 0.f, 0.f, 0.f);   // the row's first chunk stays in registers (D <= 256: the whole row)
        if (in) {
            for (int k = lane; k < vec; k += 64) {
                const float4 a = ld4(row + 4 * k);
                if (k == lane) first = a;
                ss += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
            }
            for (int d = tail0 + lane; d < D; d += 64) { const float a = row[d]; ss += a * a; }
        }
        ss = wave_sum(ss);                                // (butterfly: the same value in every lane)
        const float rc = 1.0f / sqrtf(fmaxf(ss, 1e-12f));
        if (lane == 0) { r[c] = rc; q[c] = ss * rc * rc; }
        if (in) {
            const float pr = p[c] * rc;
            for (int k = lane; k < vec; k += 64) {
                const float4 a = k == lane ? first : ld4(row + 4 * k);
                float* o = mine + 4 * k;
                o[0] += pr * a.x; o[1] += pr * a.y; o[2] += pr * a.z; o[3] += pr * a.w;
            }
            for (int d = tail0 + lane; d < D; d += 64) mine[d] += pr * row[d];
        }
    }
    __syncthreads();
    for (int d = tid; d < D; d += DIV_THREADS) m[d] = ((mw[d] + mw[D + d]) + mw[2 * D + d]) + mw[3 * D + d];
    __syncthreads();
    // pass 2: t_c = r_c (ACE[id_c] . m)
    for (int c = w; c < NC; c += DIV_WAVES) {
        const int64_t id = ids[c];
        float s = 0.f;
        if (id >= 0 && id < n_items) {
            const float* row = ace + (size_t)id * (size_t)ld;
            for (int k = lane; k < vec; k += 64) {
                const float4 a = ld4(row + 4 * k);
                const float* mm = m + 4 * k;
                s += a.x * mm[0] + a.y * mm[1] + a.z * mm[2] + a.w * mm[3];
            }
            for (int d = tail0 + lane; d < D; d += 64) s += row[d] * m[d];
        }
        s = wave_sum(s);
        if (lane == 0) t[c] = r[c] * s;
    }
    __syncthreads();
    // (S p)_c = t_c - |e^_c|^2 * (p summed over the candidates of c's id, c itself included), e = p . (S p)
    float part = 0.f;
    for (int c = tid; c < NC; c += DIV_THREADS) {
        const int64_t id = ids[c];
        float same = 0.f;
        for (int j = 0; j < NC; ++j) same += ids[j] == id ? p[j] : 0.f;
        const float v = t[c] - q[c] * same;
        sp[bt * NC + c] = v;
        part += p[c] * v;
    }
    const float e = block_sum(part, red);
    if (tid == 0) {
        e_out[bt] = e;
        nll[bt] += factor * e;
    }
}

// Behind the arm's softmax backward: ds[row] += gx, and dS3[row,k] = ds[row] * w4[k] * leaky'(S3[row,k]) again from the updated ds - the
// expression and operation order of k_score_softmax_bwd (csrc/scorer.hip), so a bf16 dS3 is rounded once, from the fp32 product.
template <int K3, typename T>
__global__ __launch_bounds__(256) void k_diversity_bwd(const T* __restrict__ S3, const float* __restrict__ w4, const float* __restrict__ probs,
                                                       const unsigned char* __restrict__ mask, int BT, int N, float scale /* 1/(tau*sum_mask) */,
                                                       const ChamStepScalars* __restrict__ sc, float tau, const float* __restrict__ sp,
                                                       const float* __restrict__ e, float factor, float* __restrict__ ds, T* __restrict__ dS3) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int NC = N + 1;
    if (row >= (size_t)BT * NC) return;
    if (sc) scale = 1.0f / (tau * sc->sum_mask);       // (the by-value form computes the same fp32 expression on the host)
    const size_t bt = row / NC;
    float g = ds[row];
    if (mask[bt]) g += factor * scale * 2.f * probs[row] * (sp[row] - e[bt]);
    ds[row] = g;
    const T* r = S3 + row * K3;
    T* o = dS3 + row * K3;
#pragma unroll
    for (int k = 0; k < K3 / 4; ++k) {
        const float4 x = ld4(r + 4 * k);
        float4 y;
        y.x = g * w4[4 * k] * act_bwd_from_out(x.x, ACT_LEAKY);
        y.y = g * w4[4 * k + 1] * act_bwd_from_out(x.y, ACT_LEAKY);
        y.z = g * w4[4 * k + 2] * act_bwd_from_out(x.z, ACT_LEAKY);
        y.w = g * w4[4 * k + 3] * act_bwd_from_out(x.w, ACT_LEAKY);
        st4(o + 4 * k, y);
    }
}

extern "C" int cham_diversity_fwd(const float* probs, const int64_t* label_ids, const int64_t* neg_ids, const uint8_t* mask, int BT, int N,
                                  const float* ace, int ld_ace, int D, int64_t n_items, float factor, float* sp, float* e, float* nll,
                                  void* stream) {
    if (!probs || !label_ids || !neg_ids || !mask || !ace || !sp || !e || !nll) return -CHAM_ERR_ARG;
    if (BT < 0 || N < 1 || D < 1 || ld_ace < D || n_items < 1 || !(factor >= 0.f)) return -CHAM_ERR_ARG;
    if (BT == 0) return CHAM_OK;
    const size_t NC = (size_t)N + 1;
    const size_t lds = NC * (sizeof(int64_t) + 4 * sizeof(float)) + ((size_t)(DIV_WAVES + 1) * D + DIV_WAVES) * sizeof(float);
    if (lds > DIV_MAX_LDS) return -CHAM_ERR_ARG;
    if (lds > 64 * 1024) CHAM_SET_DYNAMIC_LDS(k_diversity_fwd, DIV_MAX_LDS);      // (set once per device: the cap, not this call's size)
    // 16-byte row pieces need an aligned base and a row stride of whole pieces
    const int vec = (reinterpret_cast<uintptr_t>(ace) % 16 == 0 && ld_ace % 4 == 0) ? D / 4 : 0;
    hipLaunchKernelGGL(k_diversity_fwd, dim3((unsigned)BT), dim3(DIV_THREADS), lds, (hipStream_t)stream, probs, label_ids, neg_ids, mask, N,
                       ace, ld_ace, D, n_items, vec, factor, sp, e, nll);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

template <typename T>
static int diversity_bwd_impl(const T* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT, int N, float tau,
                              const void* scalars, float sum_mask, const float* sp, const float* e, float factor, float* ds, T* dS3,
                              void* stream) {
    if (!S3 || !w4 || !probs || !mask || !sp || !e || !ds || !dS3) return -CHAM_ERR_ARG;
    if ((K3 != 32 && K3 != 4) || BT < 0 || N < 1 || !(factor >= 0.f) || (!scalars && !(sum_mask > 0.f))) return -CHAM_ERR_ARG;
    const size_t rows = (size_t)BT * ((size_t)N + 1);
    if (rows == 0) return CHAM_OK;
    if (K3 == 4)      // the cosine head (csrc/cosine.hip): ds is what its backward reads, dS3 [rows, 4] is scratch
        hipLaunchKernelGGL((k_diversity_bwd<4, T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S3, w4, probs, mask,
                           BT, N, scalars ? 0.f : 1.0f / (tau * sum_mask), reinterpret_cast<const ChamStepScalars*>(scalars), tau, sp, e, factor,
                           ds, dS3);
    else
        hipLaunchKernelGGL((k_diversity_bwd<32, T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S3, w4, probs, mask,
                           BT, N, scalars ? 0.f : 1.0f / (tau * sum_mask), reinterpret_cast<const ChamStepScalars*>(scalars), tau, sp, e, factor,
                           ds, dS3);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

extern "C" int cham_diversity_bwd(const float* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT, int N, float tau,
                                  const void* scalars, float sum_mask, const float* sp, const float* e, float factor, float* ds, float* dS3,
                                  void* stream) {
    return diversity_bwd_impl<float>(S3, K3, w4, probs, mask, BT, N, tau, scalars, sum_mask, sp, e, factor, ds, dS3, stream);
}
extern "C" int cham_diversity_bwd_b16(const void* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT, int N,
                                      float tau, const void* scalars, float sum_mask, const float* sp, const float* e, float factor,
                                      float* ds, void* dS3, void* stream) {
    return diversity_bwd_impl<__bf16>(reinterpret_cast<const __bf16*>(S3), K3, w4, probs, mask, BT, N, tau, scalars, sum_mask, sp, e, factor,
                                      ds, reinterpret_cast<__bf16*>(dS3), stream);
}
