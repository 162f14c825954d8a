// Cosine-similarity ranking head (--recommendations_ranking cosine): the DSSM-style formulation the comments of nar_model.py:435-437 refer to
// ("l2-norm to be able to compute cosine similarity"; scopes cos_sim_positive / cos_sim_negative, tensors cos_sim_concat / cosine_sim_loss).
// For a click bt with p = pred[bt] (FC2 tanh output, width C) and candidate rows z_c = Z2c[bt (N+1) + c] (CAR tanh output; c = 0 the label):
//   inv(x) = 1 / sqrt(max(sum_k x_k^2, 1e-12))                                   (tf.nn.l2_normalize, the form csrc/diversity.hip uses)
//   rz_c = inv(z_c), rp = inv(p), z^_c = z_c rz_c, p^ = p rp,  logit_c = cos_c = sum_k z^_ck p^_k
// followed by the softmax / NLL / novelty / diversity kernels of the MLP head, which read cosq [R, 4] = (cos, 0, 0, 0) as their "S3" with
// K3 = 4, w4 = (1, 0, 0, 0), b4 = 0 (csrc/scorer.hip: the last-layer dot then returns the cosine unchanged).  The head has no weights.
// Gradients of sum_c ds_c cos_c with respect to the two tanh PRE-activations:
//   dZ2pre_ck   = ds_c rz_c (p^_k - cos_c z^_ck) (1 - z_ck^2)
//   dpred_pre_k = (sum_c ds_c rp (z^_ck - cos_c p^_k)) (1 - p_k^2)
// Where a vector's sum of squares is below 1e-12 its inverse norm is the CONSTANT 1e6 and carries no gradient: the projection term of that
// vector (- cos z^ or - cos p^) is dropped, as autograd of the clamp defines it.  The forward kernel marks exactly those vectors with
// r == 1e6 (an unclamped inverse norm that would round to 1e6 is stored one ulp lower), so the backward needs no second pass over the row.
// Every sum has a fixed order (lane-private partial sums, butterfly wave sums; per-thread loops over the candidates): no atomics.
#include "common.h"

#define COS_NORM_FLOOR 1e-12f
#define COS_RCLAMP 1.0e6f            /* 1 / sqrt(1e-12f) in fp32 */
#define COS_RCLAMP_BELOW 999999.9375f /* the fp32 number below it */
#define COS_PJ 8                      /* 16-byte pieces of pred a lane keeps in registers: C <= 2048; wider rows re-read pred (L1) */

__device__ __forceinline__ float cos_inv_norm(float ss) {
    return ss < COS_NORM_FLOOR ? COS_RCLAMP : fminf(1.0f / sqrtf(ss), COS_RCLAMP_BELOW);
}
__device__ __forceinline__ float dot4(const float4& a, const float4& b) { return a.x * b.x + a.y * b.y + a.z * b.z + a.w * b.w; }

// One workgroup per click; pred[bt] and its norm once per wave, in registers; wave w takes the candidates c = w, w + 4, ...; lanes run across
// C in 16-byte (bf16 rows: 8-byte) pieces; reads R C elements, writes 6 floats per row.  Masked clicks are computed like any other (their
// rows are finite): the softmax kernel reads their logits.
template <typename T>
__global__ __launch_bounds__(256) void k_cosine_fwd(const T* __restrict__ Z2c, long long ldz, const float* __restrict__ pred, int C, int NC,
                                                    float* __restrict__ cosq, float* __restrict__ rz, float* __restrict__ rp) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nk = C >> 2;
    const size_t bt = blockIdx.x;
    const float* pr = pred + bt * C;
    float4 p[COS_PJ];
    float pss = 0.f;
#pragma unroll
    for (int j = 0; j < COS_PJ; ++j) {
        const int k = lane + 64 * j;
        p[j] = k < nk ? ld4(pr + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
        pss += dot4(p[j], p[j]);
    }
    for (int k = lane + 64 * COS_PJ; k < nk; k += 64) { const float4 a = ld4(pr + 4 * k); pss += dot4(a, a); }
    const float rpv = cos_inv_norm(wave_sum(pss));             // (butterfly: the same value in every lane of every wave)
    if (threadIdx.x == 0) rp[bt] = rpv;
    for (int c = w; c < NC; c += 4) {
        const size_t row = bt * NC + c;
        const T* zr = Z2c + row * (size_t)ldz;
        float4 z[COS_PJ];
#pragma unroll
        for (int j = 0; j < COS_PJ; ++j) {
            const int k = lane + 64 * j;
            z[j] = k < nk ? ld4(zr + 4 * k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        float dot = 0.f, ss = 0.f;
#pragma unroll
        for (int j = 0; j < COS_PJ; ++j) { dot += dot4(z[j], p[j]); ss += dot4(z[j], z[j]); }
        for (int k = lane + 64 * COS_PJ; k < nk; k += 64) {
            const float4 a = ld4(zr + 4 * k), b = ld4(pr + 4 * k);
            dot += dot4(a, b); ss += dot4(a, a);
        }
        dot = wave_sum(dot); ss = wave_sum(ss);
        if (lane == 0) {
            const float r = cos_inv_norm(ss);
            rz[row] = r;
            // (+ 0: a cosine of -0 is stored as +0, what the softmax kernel's 0 + cos 1 + ... makes of it)
            reinterpret_cast<float4*>(cosq)[row] = make_float4(dot * r * rpv + 0.f, 0.f, 0.f, 0.f);
        }
    }
}

// t[r] = |ds_r| rz_r for r < n, 0 up to npad (a multiple of 4): cham_h2_scale_absmax(t, npad, NULL, 0, rec) then derives the scale record of
// the two-plane dZ2pre.  max_r t_r bounds every element: |p^_k - cos z^_k| <= sin angle(p^, z^) <= 1 (the component of the unit vector p^
// orthogonal to z^), |1 - z^2| <= 1; where a projection term is dropped (clamp regime) |p^_k| <= 1 still holds.
__global__ __launch_bounds__(256) void k_cosine_bound(const float* __restrict__ ds, const float* __restrict__ rz, size_t n, size_t npad,
                                                      float* __restrict__ t) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < npad) t[i] = i < n ? fabsf(ds[i]) * rz[i] : 0.f;
}

// Shaped like k_mulpred_bwd / k_mulpred_bwd_h2 (csrc/scorer.hip): one workgroup per click, a thread owns four columns and loops over the
// click's candidates (four row loads in flight), ds_c / rz_c / cos_c staged once in LDS.  Reads every Z2c row once; writes dZ2pre in the
// arm's storage - MODE 0 fp32 rows, 1 two fp16 planes x the scale of `rec` (see k_cosine_bound), 2 bf16 rows - dpred_pre [BT, C] and, where
// col_part != NULL, the column sums of the click's STORED rows (its share of the b2 gradient).  A masked click writes zeros everywhere: the
// CAR dgrad and the W2 weight gradient read its rows.
template <int MODE, typename T>
__global__ __launch_bounds__(256) void k_cosine_bwd(const T* __restrict__ Z2c, const float* __restrict__ pred, const float* __restrict__ ds,
                                                    const float* __restrict__ rz, const float* __restrict__ rp, const float* __restrict__ cosq,
                                                    const unsigned char* __restrict__ mask, int C, int NC, void* __restrict__ out, long long ps,
                                                    const H2Scale* __restrict__ rec, float* __restrict__ dpred_pre, float* __restrict__ col_part) {
    extern __shared__ float cos_lds[];                    // ds [NC] | rz [NC] | cos [NC]
    float* sd = cos_lds; float* sr = sd + NC; float* sc = sr + NC;
    const size_t bt = blockIdx.x, row0 = bt * NC;
    for (int c = threadIdx.x; c < NC; c += 256) { sd[c] = ds[row0 + c]; sr[c] = rz[row0 + c]; sc[c] = cosq[(row0 + c) * 4]; }
    __syncthreads();
    const bool live = mask[bt] != 0;
    const float rpv = rp[bt];
    const bool p_free = rpv != COS_RCLAMP;                 // pred's norm carries a gradient
    float scale = 1.f;
    if constexpr (MODE == 1) scale = rec->scale;
    for (int k = threadIdx.x; k < C / 4; k += 256) {
        const float4 p = ld4(pred + bt * C + 4 * k);
        const float4 ph = make_float4(p.x * rpv, p.y * rpv, p.z * rpv, p.w * rpv);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f), cs = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int c0 = 0; c0 < NC; c0 += 4) {
            float4 z[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) z[i] = ld4(Z2c + (row0 + min(c0 + i, NC - 1)) * C + 4 * k);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (c0 + i >= NC) break;
                const int c = c0 + i;
                const float d = sd[c], r = sr[c], cv = sc[c];
                const float a = r != COS_RCLAMP ? cv : 0.f, b = p_free ? cv : 0.f, g = d * r;
                const float4 zh = make_float4(z[i].x * r, z[i].y * r, z[i].z * r, z[i].w * r);
                acc.x += d * (zh.x - b * ph.x); acc.y += d * (zh.y - b * ph.y); acc.z += d * (zh.z - b * ph.z); acc.w += d * (zh.w - b * ph.w);
                float4 o;
                o.x = g * (ph.x - a * zh.x) * (1.f - z[i].x * z[i].x); o.y = g * (ph.y - a * zh.y) * (1.f - z[i].y * z[i].y);
                o.z = g * (ph.z - a * zh.z) * (1.f - z[i].z * z[i].z); o.w = g * (ph.w - a * zh.w) * (1.f - z[i].w * z[i].w);
                if (!live) o = make_float4(0.f, 0.f, 0.f, 0.f);
                const size_t off = (row0 + c) * C + 4 * k;
                if constexpr (MODE == 0) st4(reinterpret_cast<float*>(out) + off, o);
                if constexpr (MODE == 1) st4_planes_h2(reinterpret_cast<_Float16*>(out) + off, ps, o, scale);
                if constexpr (MODE == 2) {      // the sums are over the rows as stored: rounded first
                    o.x = (float)(__bf16)o.x; o.y = (float)(__bf16)o.y; o.z = (float)(__bf16)o.z; o.w = (float)(__bf16)o.w;
                    st4(reinterpret_cast<__bf16*>(out) + off, o);
                }
                cs.x += o.x; cs.y += o.y; cs.z += o.z; cs.w += o.w;
            }
        }
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            o.x = acc.x * rpv * (1.f - p.x * p.x); o.y = acc.y * rpv * (1.f - p.y * p.y);
            o.z = acc.z * rpv * (1.f - p.z * p.z); o.w = acc.w * rpv * (1.f - p.w * p.w);
        }
        reinterpret_cast<float4*>(dpred_pre + bt * C)[k] = o;
        if (col_part) reinterpret_cast<float4*>(col_part + bt * C)[k] = cs;
    }
}

// ---------------------------------------------------------------------------------------------------
template <typename T>
static int cosine_fwd_impl(const T* Z2c, long long ldz, const float* pred, int C, int BT, int N, float* cosq, float* rz, float* rp, void* stream) {
    if (!Z2c || !pred || !cosq || !rz || !rp || C <= 0 || (C & 3) || BT < 0 || N < 1 || ldz < C || (ldz & 3)) return -CHAM_ERR_ARG;
    if (((uintptr_t)Z2c & (4 * sizeof(T) - 1)) || (((uintptr_t)pred | (uintptr_t)cosq) & 15)) return -CHAM_ERR_ARG;
    if (BT == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_cosine_fwd<T>, dim3((unsigned)BT), dim3(256), 0, (hipStream_t)stream, Z2c, ldz, pred, C, N + 1, cosq, rz, rp);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
extern "C" int cham_cosine_fwd(const float* Z2c, long long ldz, const float* pred, int C, int BT, int N, float* cosq, float* rz, float* rp,
                               void* stream) {
    return cosine_fwd_impl<float>(Z2c, ldz, pred, C, BT, N, cosq, rz, rp, stream);
}
extern "C" int cham_cosine_fwd_b16(const void* Z2c, long long ldz, const float* pred, int C, int BT, int N, float* cosq, float* rz, float* rp,
                                   void* stream) {
    return cosine_fwd_impl<__bf16>(reinterpret_cast<const __bf16*>(Z2c), ldz, pred, C, BT, N, cosq, rz, rp, stream);
}

extern "C" int cham_cosine_bound(const float* ds, const float* rz, size_t rows, float* t, void* stream) {
    if (!ds || !rz || !t || ((uintptr_t)t & 15)) return -CHAM_ERR_ARG;
    const size_t npad = (rows + 3) & ~(size_t)3;
    if (npad == 0) return CHAM_OK;
    hipLaunchKernelGGL(k_cosine_bound, dim3((unsigned)((npad + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ds, rz, rows, npad, t);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

template <int MODE, typename T>
static int cosine_bwd_impl(const T* Z2c, const float* pred, const float* ds, const float* rz, const float* rp, const float* cosq,
                           const uint8_t* mask, int C, int BT, int N, void* out, long long ps, const void* rec, float* dpred_pre,
                           float* col_part, void* stream) {
    if (!Z2c || !pred || !ds || !rz || !rp || !cosq || !mask || !out || !dpred_pre || C <= 0 || (C & 3) || BT < 0 || N < 1) return -CHAM_ERR_ARG;
    if (MODE == 1 && (!rec || (ps & 3))) return -CHAM_ERR_ARG;
    if (((uintptr_t)Z2c & (4 * sizeof(T) - 1)) || (((uintptr_t)pred | (uintptr_t)dpred_pre | (uintptr_t)col_part) & 15) ||
        ((uintptr_t)out & (MODE == 0 ? 15 : 7)))
        return -CHAM_ERR_ARG;
    const size_t lds = (size_t)3 * (N + 1) * sizeof(float);
    if (lds > 64 * 1024) return -CHAM_ERR_ARG;            // 1 + N <= 5461 candidates per click
    if (BT == 0) return CHAM_OK;
    hipLaunchKernelGGL((k_cosine_bwd<MODE, T>), dim3((unsigned)BT), dim3(256), lds, (hipStream_t)stream, Z2c, pred, ds, rz, rp, cosq, mask, C,
                       N + 1, out, ps, reinterpret_cast<const H2Scale*>(rec), dpred_pre, col_part);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}
extern "C" int cham_cosine_bwd(const float* Z2c, const float* pred, const float* ds, const float* rz, const float* rp, const float* cosq,
                               const uint8_t* mask, int C, int BT, int N, float* dZ2pre, float* dpred_pre, float* b2part, void* stream) {
    return cosine_bwd_impl<0, float>(Z2c, pred, ds, rz, rp, cosq, mask, C, BT, N, dZ2pre, 0, nullptr, dpred_pre, b2part, stream);
}
extern "C" int cham_cosine_bwd_h2(const float* Z2c, const float* pred, const float* ds, const float* rz, const float* rp, const float* cosq,
                                  const uint8_t* mask, int C, int BT, int N, void* dZ2p, long long plane_stride, const void* scale_rec,
                                  float* dpred_pre, float* b2part, void* stream) {
    return cosine_bwd_impl<1, float>(Z2c, pred, ds, rz, rp, cosq, mask, C, BT, N, dZ2p, plane_stride, scale_rec, dpred_pre, b2part, stream);
}
extern "C" int cham_cosine_bwd_b16(const void* Z2c, const float* pred, const float* ds, const float* rz, const float* rp, const float* cosq,
                                   const uint8_t* mask, int C, int BT, int N, void* dZ2pre, float* dpred_pre, float* b2part, void* stream) {
    return cosine_bwd_impl<2, __bf16>(reinterpret_cast<const __bf16*>(Z2c), pred, ds, rz, rp, cosq, mask, C, BT, N, dZ2pre, 0, nullptr,
                                      dpred_pre, b2part, stream);
}
