// Pairwise ranking losses over the sampled candidates (--loss_function bpr | top1 | bpr_max | top1_max): the last scorer layer, the
// softmax over all 1 + N candidates (evaluation and the diversity term read it under every loss) and the loss / its logit gradient.
// The default loss (softmax + masked NLL) stays with k_score_softmax_fwd / _bwd in scorer.hip; these kernels run in their place.
//
// Per valid click, r_c = logit_c / tau (c = 0 the positive, 1..N the negatives), d_n = r_0 - r_n, s(x) = 1 / (1 + exp(-x)),
// q = softmax(r_1..r_N) over the negatives alone (the weights GRU4Rec's "-max" losses use; differentiated, not a constant):
//   bpr       l = -(1/N) sum_n log s(d_n)
//   top1      l = (1/N) sum_n [s(-d_n) + s(r_n^2)]
//   bpr_max   l = -log(A + 1e-24) + lambda R,   A = sum_n q_n s(d_n),  R = sum_n q_n r_n^2
//   top1_max  l = sum_n q_n [s(-d_n) + s(r_n^2)]
// nll[bt] = mask ? l - novelty_reg_factor * (q . nov) : 0 - the novelty term exactly as k_score_softmax_fwd has it.
// DESIGN.md section 10.3 derives the gradients.
#include "common.h"

enum { RANK_BPR = 1, RANK_TOP1 = 2, RANK_BPR_MAX = 3, RANK_TOP1_MAX = 4 };
#define RANK_AUX 8      // floats per click carried from forward to backward: {max_n r_n, sum_n exp(r_n - max), P1, P2, dl/dr_0, l, 0, 0}
#define RANK_LOG_EPS 1e-24f

// s(x), s'(x) = s(x) s(-x) and log s(x) from e = exp(-|x|) in (0, 1]: no 1 - s(x) and no log of a sigmoid that may have underflowed
__device__ __forceinline__ float rl_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}
__device__ __forceinline__ float rl_dsigmoid(float x) {
    const float e = expf(-fabsf(x)), t = 1.f + e;
    return e / (t * t);
}
__device__ __forceinline__ float rl_log_sigmoid(float x) { return fminf(x, 0.f) - log1pf(expf(-fabsf(x))); }

// One wave per click (b,t); lanes strided over the 1 + N candidates; every reduction a wave butterfly over the lane partials.
template <int K3, typename T>
__global__ __launch_bounds__(256) void k_score_rankloss_fwd(const T* __restrict__ S3, const float* __restrict__ w4,
                                                            const float* __restrict__ b4, int BT, int N, float inv_tau,
                                                            const unsigned char* __restrict__ mask,
                                                            float* __restrict__ logits, float* __restrict__ probs,
                                                            float* __restrict__ nll, float nov_factor,
                                                            const int64_t* __restrict__ neg_ids, const float* __restrict__ pop_norm,
                                                            float* __restrict__ nov_aux /*[BT,3]*/, float inv_log2_base, int kind,
                                                            float lambda, float* __restrict__ aux /*[BT,RANK_AUX]*/) {
    const int lane = threadIdx.x & 63, bt = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bt >= BT) return;
    const int NC = N + 1;
    float w[K3];
#pragma unroll
    for (int k = 0; k < K3; ++k) w[k] = w4[k];
    const float bias = b4[0];
    // logits and softmax(logits / tau) over all candidates: the operation order of k_score_softmax_fwd
    float mx = -INFINITY, mxn = -INFINITY, s0 = 0.f;
    for (int c = lane; c < NC; c += 64) {
        const T* r = S3 + ((size_t)bt * NC + c) * K3;
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < K3 / 4; ++k) { const float4 x = ld4(r + 4 * k); s += x.x * w[4 * k] + x.y * w[4 * k + 1] + x.z * w[4 * k + 2] + x.w * w[4 * k + 3]; }
        s += bias;
        logits[(size_t)bt * NC + c] = s;
        mx = fmaxf(mx, s * inv_tau);
        if (c == 0) s0 = s; else mxn = fmaxf(mxn, s * inv_tau);
    }
    mx = wave_max(mx);
    mxn = wave_max(mxn);
    // r = logit * (1 / tau) and d = r_0 - r_n as separately rounded operations (no contraction into an fma): the forward and the backward
    // kernel then see the same d bit for bit, as does a plain fp32 restatement on the host
    const float r0 = __fmul_rn(__shfl(s0, 0, 64), inv_tau);      // lane 0 holds the positive
    float sum = 0.f;
    for (int c = lane; c < NC; c += 64) {
        const float e = expf(logits[(size_t)bt * NC + c] * inv_tau - mx);   // same lane wrote it
        probs[(size_t)bt * NC + c] = e;
        sum += e;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int c = lane; c < NC; c += 64) probs[(size_t)bt * NC + c] *= inv;
    // the negatives: q_n = exp(r_n - mxn) / sn; the sums below are over e_n = sn q_n and divided once
    float sn = 0.f, nov = 0.f, a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int c = lane; c < NC; c += 64) {
        if (c == 0) continue;
        const float rn = __fmul_rn(logits[(size_t)bt * NC + c], inv_tau), d = __fsub_rn(r0, rn);
        const float e = expf(rn - mxn);
        sn += e;
        if (nov_factor > 0.f) nov += e * (-log2f(pop_norm[neg_ids[(size_t)bt * N + (c - 1)]]) * inv_log2_base);
        if (kind == RANK_BPR) {
            a0 -= rl_log_sigmoid(d);
            a2 += rl_sigmoid(-d);
        } else if (kind == RANK_TOP1) {
            a0 += rl_sigmoid(-d) + rl_sigmoid(rn * rn);
            a2 += rl_dsigmoid(d);
        } else if (kind == RANK_BPR_MAX) {
            a0 += e * rl_sigmoid(d);
            a1 += e * (rn * rn);
            a2 += e * rl_dsigmoid(d);
        } else {
            a0 += e * (rl_sigmoid(-d) + rl_sigmoid(rn * rn));
            a2 += e * rl_dsigmoid(d);
        }
    }
    sn = wave_sum(sn); a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2);
    float novterm = 0.f;
    if (nov_factor > 0.f) {
        novterm = wave_sum(nov) / sn;
        if (lane == 0) { nov_aux[(size_t)bt * 3] = mxn; nov_aux[(size_t)bt * 3 + 1] = sn; nov_aux[(size_t)bt * 3 + 2] = novterm; }
    }
    if (lane == 0) {
        const float invN = 1.f / (float)N, isn = 1.f / sn;
        float p1 = 0.f, p2 = 0.f, g0, l;
        if (kind == RANK_BPR) { l = a0 * invN; g0 = -a2 * invN; }
        else if (kind == RANK_TOP1) { l = a0 * invN; g0 = -a2 * invN; }
        else if (kind == RANK_BPR_MAX) {
            p1 = a0 * isn; p2 = a1 * isn;
            l = -logf(p1 + RANK_LOG_EPS) + lambda * p2;
            g0 = -(a2 * isn) / (p1 + RANK_LOG_EPS);
        } else { l = a0 * isn; p1 = l; g0 = -a2 * isn; }
        float* a = aux + (size_t)bt * RANK_AUX;
        a[0] = mxn; a[1] = sn; a[2] = p1; a[3] = p2; a[4] = g0; a[5] = l; a[6] = 0.f; a[7] = 0.f;
        nll[bt] = mask[bt] ? l - nov_factor * novterm : 0.f;
    }
}

// ds[row] = (dl/dr_c) * mask / (tau * sum(mask)) + the novelty term's gradient;  dS3pre[row,k] = ds * w4[k] * leaky'(S3[row,k]).
// One thread per candidate row: the per-click sums come from the forward's aux record.
template <int K3, typename T>
__global__ __launch_bounds__(256) void k_score_rankloss_bwd(const T* __restrict__ S3, const float* __restrict__ w4,
                                                            const unsigned char* __restrict__ mask, int BT, int N,
                                                            float scale /* 1/(tau*sum_mask) */, float* __restrict__ ds, T* __restrict__ dS3,
                                                            float nov_factor, const int64_t* __restrict__ neg_ids,
                                                            const float* __restrict__ pop_norm, const float* __restrict__ logits,
                                                            float inv_tau, const float* __restrict__ nov_aux, float inv_log2_base,
                                                            const ChamStepScalars* __restrict__ sc, float tau, int kind, float lambda,
                                                            const float* __restrict__ aux) {
    const size_t row = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int NC = N + 1;
    if (row >= (size_t)BT * NC) return;
    if (sc) scale = 1.0f / (tau * sc->sum_mask);       // (the by-value entry points compute the same fp32 expression on the host)
    const int bt = (int)(row / NC), c = (int)(row % NC);
    float g = 0.f;
    if (mask[bt]) {
        const float* a = aux + (size_t)bt * RANK_AUX;
        if (c == 0) {
            g = a[4];
        } else {
            const float rn = __fmul_rn(logits[row], inv_tau), d = __fsub_rn(__fmul_rn(logits[(size_t)bt * NC], inv_tau), rn);
            const float q = expf(rn - a[0]) / a[1];
            const float invN = 1.f / (float)N;
            if (kind == RANK_BPR) {
                g = rl_sigmoid(-d) * invN;
            } else if (kind == RANK_TOP1) {
                g = (rl_dsigmoid(d) + 2.f * rn * rl_dsigmoid(rn * rn)) * invN;
            } else if (kind == RANK_BPR_MAX) {
                const float A = a[2], R = a[3];
                const float dA = q * (rl_sigmoid(d) - A) - q * rl_dsigmoid(d);
                const float dR = q * (rn * rn - R) + 2.f * q * rn;
                g = -dA / (A + RANK_LOG_EPS) + lambda * dR;
            } else {
                const float Tn = rl_sigmoid(-d) + rl_sigmoid(rn * rn);
                g = q * (Tn - a[2]) + q * (rl_dsigmoid(d) + 2.f * rn * rl_dsigmoid(rn * rn));
            }
        }
        g *= scale;
        if (nov_factor > 0.f && c > 0) {
            // d/ds_c of -factor * sum_n q_n nov_n: -factor/tau * q_c * (nov_c - q.nov), as k_score_softmax_bwd has it
            const float q = expf(logits[row] * inv_tau - nov_aux[(size_t)bt * 3]) / nov_aux[(size_t)bt * 3 + 1];
            const float nov_c = -log2f(pop_norm[neg_ids[(size_t)bt * N + (c - 1)]]) * inv_log2_base;
            g -= nov_factor * scale * q * (nov_c - nov_aux[(size_t)bt * 3 + 2]);
        }
    }
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

// ---------------------------------------------------------------------------------------------------
static inline bool rank_kind_ok(int kind) { return kind >= RANK_BPR && kind <= RANK_TOP1_MAX; }

template <typename T>
static int score_rankloss_fwd_impl(const T* S3, int K3, const float* w4, const float* b4, int BT, int N, float tau, const uint8_t* mask,
                                   float* logits, float* probs, float* nll, float novelty_reg_factor, const int64_t* neg_ids,
                                   const float* pop_norm, float* nov_aux, int loss_kind, float bpr_max_reg, float* aux, void* stream) {
    if (!S3 || !w4 || !b4 || !mask || !logits || !probs || !nll || !aux || (K3 != 32 && K3 != 4) || BT <= 0 || N < 1 || !(tau > 0.f) ||
        !rank_kind_ok(loss_kind))
        return -CHAM_ERR_ARG;
    if (novelty_reg_factor > 0.f && (!neg_ids || !pop_norm || !nov_aux)) return -CHAM_ERR_ARG;
    if (K3 == 4)      // the cosine head: S3 = (cos, 0, 0, 0) per row, w4 = (1, 0, 0, 0), b4 = 0
        hipLaunchKernelGGL((k_score_rankloss_fwd<4, T>), dim3((BT + 3) / 4), dim3(256), 0, (hipStream_t)stream, S3, w4, b4, BT, N, 1.0f / tau,
                           mask, logits, probs, nll, novelty_reg_factor, neg_ids, pop_norm, nov_aux, g_cham_inv_log2_pop_base, loss_kind,
                           bpr_max_reg, aux);
    else
        hipLaunchKernelGGL((k_score_rankloss_fwd<32, T>), dim3((BT + 3) / 4), dim3(256), 0, (hipStream_t)stream, S3, w4, b4, BT, N, 1.0f / tau,
                           mask, logits, probs, nll, novelty_reg_factor, neg_ids, pop_norm, nov_aux, g_cham_inv_log2_pop_base, loss_kind,
                           bpr_max_reg, aux);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
extern "C" int cham_score_rankloss_fwd(const float* S3, int K3, const float* w4, const float* b4, int BT, int N, float tau,
                                       const uint8_t* mask, float* logits, float* probs, float* nll, float novelty_reg_factor,
                                       const int64_t* neg_ids, const float* pop_norm, float* nov_aux, int loss_kind, float bpr_max_reg,
                                       float* aux, void* stream) {
    return score_rankloss_fwd_impl<float>(S3, K3, w4, b4, BT, N, tau, mask, logits, probs, nll, novelty_reg_factor, neg_ids, pop_norm,
                                          nov_aux, loss_kind, bpr_max_reg, aux, stream);
}
extern "C" int cham_score_rankloss_fwd_b16(const void* S3, int K3, const float* w4, const float* b4, int BT, int N, float tau,
                                           const uint8_t* mask, float* logits, float* probs, float* nll, float novelty_reg_factor,
                                           const int64_t* neg_ids, const float* pop_norm, float* nov_aux, int loss_kind,
                                           float bpr_max_reg, float* aux, void* stream) {
    return score_rankloss_fwd_impl<__bf16>(reinterpret_cast<const __bf16*>(S3), K3, w4, b4, BT, N, tau, mask, logits, probs, nll,
                                           novelty_reg_factor, neg_ids, pop_norm, nov_aux, loss_kind, bpr_max_reg, aux, stream);
}

template <typename T>
static int score_rankloss_bwd_impl(const T* S3, int K3, const float* w4, const uint8_t* mask, int BT, int N, float tau, float sum_mask,
                                   float* ds, T* dS3, float novelty_reg_factor, const int64_t* neg_ids, const float* pop_norm,
                                   const float* logits, const float* nov_aux, int loss_kind, float bpr_max_reg, const float* aux,
                                   void* stream, const void* scalars = nullptr) {
    if (!S3 || !w4 || !mask || !ds || !dS3 || !logits || !aux || (K3 != 32 && K3 != 4) || BT <= 0 || N < 1 || !(tau > 0.f) ||
        !rank_kind_ok(loss_kind) || (!scalars && !(sum_mask > 0.f)))
        return -CHAM_ERR_ARG;
    if (novelty_reg_factor > 0.f && (!neg_ids || !pop_norm || !nov_aux)) return -CHAM_ERR_ARG;
    const size_t rows = (size_t)BT * (N + 1);
    const float scale = scalars ? 0.f : 1.0f / (tau * sum_mask);
    if (K3 == 4)      // the cosine head: ds is what its backward reads, dS3 [rows, 4] is scratch
        hipLaunchKernelGGL((k_score_rankloss_bwd<4, T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S3, w4, mask,
                           BT, N, scale, ds, dS3, novelty_reg_factor, neg_ids, pop_norm, logits, 1.0f / tau, nov_aux, g_cham_inv_log2_pop_base,
                           reinterpret_cast<const ChamStepScalars*>(scalars), tau, loss_kind, bpr_max_reg, aux);
    else
        hipLaunchKernelGGL((k_score_rankloss_bwd<32, T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S3, w4, mask,
                           BT, N, scale, ds, dS3, novelty_reg_factor, neg_ids, pop_norm, logits, 1.0f / tau, nov_aux, g_cham_inv_log2_pop_base,
                           reinterpret_cast<const ChamStepScalars*>(scalars), tau, loss_kind, bpr_max_reg, aux);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
// (`probs` is not read: the argument lists mirror cham_score_softmax_bwd*, so that one call site serves both pairs)
extern "C" int cham_score_rankloss_bwd(const float* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT, int N,
                                       float tau, float sum_mask, float* ds, float* dS3, float novelty_reg_factor, const int64_t* neg_ids,
                                       const float* pop_norm, const float* logits, const float* nov_aux, int loss_kind, float bpr_max_reg,
                                       const float* aux, void* stream) {
    (void)probs;
    return score_rankloss_bwd_impl<float>(S3, K3, w4, mask, BT, N, tau, sum_mask, ds, dS3, novelty_reg_factor, neg_ids, pop_norm, logits,
                                          nov_aux, loss_kind, bpr_max_reg, aux, stream);
}
extern "C" int cham_score_rankloss_bwd_b16(const void* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT, int N,
                                           float tau, float sum_mask, float* ds, void* dS3, float novelty_reg_factor, const int64_t* neg_ids,
                                           const float* pop_norm, const float* logits, const float* nov_aux, int loss_kind,
                                           float bpr_max_reg, const float* aux, void* stream) {
    (void)probs;
    return score_rankloss_bwd_impl<__bf16>(reinterpret_cast<const __bf16*>(S3), K3, w4, mask, BT, N, tau, sum_mask, ds,
                                           reinterpret_cast<__bf16*>(dS3), novelty_reg_factor, neg_ids, pop_norm, logits, nov_aux, loss_kind,
                                           bpr_max_reg, aux, stream);
}
// sum(mask) from the ChamStepScalars record (device; common.h)
extern "C" int cham_score_rankloss_bwd_dev(const float* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT, int N,
                                           float tau, const void* scalars, float* ds, float* dS3, float novelty_reg_factor,
                                           const int64_t* neg_ids, const float* pop_norm, const float* logits, const float* nov_aux,
                                           int loss_kind, float bpr_max_reg, const float* aux, void* stream) {
    (void)probs;
    if (!scalars) return -CHAM_ERR_ARG;
    return score_rankloss_bwd_impl<float>(S3, K3, w4, mask, BT, N, tau, 0.f, ds, dS3, novelty_reg_factor, neg_ids, pop_norm, logits, nov_aux,
                                          loss_kind, bpr_max_reg, aux, stream, scalars);
}
extern "C" int cham_score_rankloss_bwd_b16_dev(const void* S3, int K3, const float* w4, const float* probs, const uint8_t* mask, int BT,
                                               int N, float tau, const void* scalars, float* ds, void* dS3, float novelty_reg_factor,
                                               const int64_t* neg_ids, const float* pop_norm, const float* logits, const float* nov_aux,
                                               int loss_kind, float bpr_max_reg, const float* aux, void* stream) {
    (void)probs;
    if (!scalars) return -CHAM_ERR_ARG;
    return score_rankloss_bwd_impl<__bf16>(reinterpret_cast<const __bf16*>(S3), K3, w4, mask, BT, N, tau, 0.f, ds,
                                           reinterpret_cast<__bf16*>(dS3), novelty_reg_factor, neg_ids, pop_norm, logits, nov_aux, loss_kind,
                                           bpr_max_reg, aux, stream, scalars);
}
