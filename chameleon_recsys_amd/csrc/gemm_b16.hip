// bf16-RESIDENT MFMA GEMMs for the NAR step's bf16 configuration (BASELINE configs[2]; gfx950, wave64).
//
// Replaces the same tf.layers.Dense / matmul clusters as gemm.hip (nar_model.py:374-405 CAR, :447-500 scorer) and their
// autodiff twins, for the matrices that carry one row per CANDIDATE (B*T*(1+N) rows: 248 k at G1 shape).  In the bf16
// configuration those matrices - PreCAR / CAR activations, scorer activations, and the gradients flowing back through them - live
// in HBM as bf16, the weights have a bf16 shadow next to the fp32 master copy, accumulation / bias / activation / softmax / loss /
// Adam stay fp32.  Round 1 kept fp32 storage and rounded while staging (gemm.hip gemm_bf16_kernel): no byte was saved and the
// conversions + register transposes kept the kernels at 0.1 of either roof.
//
//   NT:  C[M,N] = epi(A[M,K] * B[N,K]^T)      A, B k-contiguous bf16 (forward with the transposed weight shadow, dgrad with the
//                                             weight as stored); C bf16 or fp32
//   TN:  C[M,N] (+)= A[K,M]^T * B[K,N]        both operands stored with the FREE index contiguous (wgrad: activations^T x
//                                             gradients, K = rows); C fp32, split-K with a deterministic fixed-order reduction
//
//   * v_mfma_f32_32x32x16_bf16 with the operands SWAPPED (B fragment first): the accumulator tile is C^T, i.e. a lane owns ONE row
//     of C and 4 x 4 CONSECUTIVE columns -> bias / saved-activation loads and the output stores are 8-byte (bf16) or 16-byte (fp32)
//     vectors per lane instead of 16 scalar accesses at a row stride.
//   * global -> register -> LDS staging in 16-byte units with NO conversion or transposition on the way: k-contiguous operands land
//     as [row][k] (row stride BK + 8 halves: conflict-free ds_read_b128 fragments); free-contiguous operands (TN) land as [k][row]
//     and the fragments - 8 consecutive k of one row per lane - are gathered by the LDS transpose read ds_read_b64_tr_b16
//     (two per fragment; layout verified on the device: tests/probe/tr_probe.hip).
//   * buffer-descriptor windows, XCD-aware tile swizzle and the one-K-split-per-XCD placement of gemm_shared.h.
#include "gemm_tile.h"
#include <stdlib.h>

struct B16Params {
    const __bf16* A; const __bf16* B; void* C;
    int M, N, K, lda, ldb, ldc;
    const float* bias;
    const __bf16* dref; int ldr;
    int accumulate;
    int kchunk, splits; float* partial;
    int nbm, nbn, xcd_split;
};

// One operand tile staged in 16-byte units.  XK: the source is k-contiguous ([row][k], 8 consecutive k per unit, LDS image
// [row][BK + 8]); !XK: the source is free-contiguous ([k][row], 8 consecutive rows per unit, LDS image [k][BF + 8]).
template <int BF, int BK, bool XK, int NTH>
struct Stage16 {
    static constexpr int LD = XK ? BK + 8 : BF + 8;
    static constexpr int NU = BF * BK / 8;
    static constexpr int NV = (NU + NTH - 1) / NTH;
    u32x4 r[NV];
    unsigned off[NV];
    int kidx[NV];
    __device__ __forceinline__ void init(int ld, int limF) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int u = threadIdx.x + i * NTH;
            unsigned o; bool ok;
            if (XK) {
                const int fr = u / (BK / 8), kc = u % (BK / 8);
                o = ((unsigned)fr * (unsigned)ld + (unsigned)kc * 8u) * 2u; kidx[i] = kc * 8; ok = fr < limF;
            } else {
                const int k = u / (BF / 8), f8 = u % (BF / 8);
                o = ((unsigned)k * (unsigned)ld + (unsigned)f8 * 8u) * 2u; kidx[i] = k; ok = f8 * 8 < limF;
            }
            if (NU % NTH != 0 && u >= NU) ok = false;
            off[i] = ok ? o : OOB_OFF;
        }
    }
    __device__ __forceinline__ void load(__amdgpu_buffer_rsrc_t win, int limK) {
        if (limK >= BK) {
#pragma unroll
            for (int i = 0; i < NV; ++i) r[i] = __builtin_amdgcn_raw_buffer_load_b128(win, off[i], 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i)
                r[i] = __builtin_amdgcn_raw_buffer_load_b128(win, kidx[i] < limK ? off[i] : OOB_OFF, 0, 0);
        }
    }
    __device__ __forceinline__ void store(__bf16* __restrict__ S) const {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int u = threadIdx.x + i * NTH;
            if (NU % NTH != 0 && u >= NU) continue;
            if (XK) {
                const int fr = u / (BK / 8), kc = u % (BK / 8);
                *reinterpret_cast<u32x4*>(S + fr * LD + kc * 8) = r[i];
            } else {
                const int k = u / (BF / 8), f8 = u % (BF / 8);
                *reinterpret_cast<u32x4*>(S + k * LD + f8 * 8) = r[i];
            }
        }
    }
};

// fragment = 8 consecutive k (kk + 8 * (lane >> 5) ...) of row f0 + (lane & 31)
template <bool XK, int LD>
__device__ __forceinline__ bf16x8 frag_read(const __bf16* __restrict__ S, int f0, int kk, int lane) {
    if (XK) {
        return *reinterpret_cast<const bf16x8*>(S + (f0 + (lane & 31)) * LD + kk + 8 * (lane >> 5));
    } else {
        // [k][row] image: each 16-lane group transposes a 4(k) x 16(row) block; lane i of the group supplies the address of
        // block[i / 4][(i % 4) * 4 ..] and receives column i = rows k .. k+3 of ONE row
        const int i = lane & 15;
        const __bf16* p = S + (kk + 8 * (lane >> 5) + (i >> 2)) * LD + f0 + 16 * ((lane >> 4) & 1) + (i & 3) * 4;
        typedef __attribute__((address_space(3))) s16x4 lds_s4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(p));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(p + 4 * LD));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        s16x8 v;
        v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
        return __builtin_bit_cast(bf16x8, v);
    }
}

// EPI: 0 plain (fp32 out: optional accumulate), 1 bias+leaky, 2 bias+tanh, 3 x leaky'(dref), 4 x tanh'(dref), 5 bias, 6 split-K partial
// MINW: __launch_bounds__ second argument = waves per SIMD the register allocation must leave room for (1 = no constraint)
template <int BM, int BN, int WM, int WN, int BK, int MINW, bool AK, bool BKC, int EPI, bool OUTF32>
__global__ __launch_bounds__(WM * WN * 64, MINW) void gemm_b16_kernel(B16Params p) {
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32, NTH = WM * WN * 64;
    using LA = Stage16<BM, BK, AK, NTH>;
    using LB = Stage16<BN, BK, BKC, NTH>;
    constexpr int ASZ = AK ? BM * LA::LD : BK * LA::LD, BSZ = BKC ? BN * LB::LD : BK * LB::LD;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    __bf16* As = reinterpret_cast<__bf16*>(smem_raw);        // [2][ASZ]
    __bf16* Bs = As + 2 * ASZ;                               // [2][BSZ]   (2 * ASZ * 2 bytes is a multiple of 16)

    int tile_m, tile_n, split;
    gemm_tile_map(p, tile_m, tile_n, split);
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int kbeg = split * p.kchunk, kend = min(p.K, kbeg + p.kchunk);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm0 = (wave / WN) * (BM / WM), wn0 = (wave % WN) * (BN / WN);

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const char* aw = reinterpret_cast<const char*>(p.A) + (AK ? ((size_t)m0 * p.lda + kbeg) : ((size_t)kbeg * p.lda + m0)) * 2;
    const char* bw = reinterpret_cast<const char*>(p.B) + (BKC ? ((size_t)n0 * p.ldb + kbeg) : ((size_t)kbeg * p.ldb + n0)) * 2;
    const size_t astep = (AK ? (size_t)BK : (size_t)BK * p.lda) * 2, bstep = (BKC ? (size_t)BK : (size_t)BK * p.ldb) * 2;
    LA la; LB lb;
    la.init(p.lda, p.M - m0);
    lb.init(p.ldb, p.N - n0);
    const int nk = (kend - kbeg + BK - 1) / BK;
    if (nk > 0) {
        la.load(make_window(aw), kend - kbeg);
        lb.load(make_window(bw), kend - kbeg);
        la.store(As); lb.store(Bs);
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        if (kt + 1 < nk) {          // tile kt+1: loads fly behind this tile's MFMAs
            aw += astep; bw += bstep;
            const int k0 = kbeg + (kt + 1) * BK;
            la.load(make_window(aw), kend - k0);
            lb.load(make_window(bw), kend - k0);
        }
        const __bf16* Ac = As + cur * ASZ;
        const __bf16* Bc = Bs + cur * BSZ;
#pragma unroll
        for (int kk = 0; kk < BK; kk += 16) {
            bf16x8 a[TM], b[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) a[i] = frag_read<AK, LA::LD>(Ac, wm0 + i * 32, kk, lane);
#pragma unroll
            for (int j = 0; j < TN; ++j) b[j] = frag_read<BKC, LB::LD>(Bc, wn0 + j * 32, kk, lane);
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)      // operands swapped: the accumulator tile is C^T (see the header)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) {
            la.store(As + (cur ^ 1) * ASZ);
            lb.store(Bs + (cur ^ 1) * BSZ);
        }
        __syncthreads();
    }

    // ---- epilogue.  acc[i][j][e]: row m = wm0 + 32 i + (lane & 31), column n = wn0 + 32 j + 8 (e >> 2) + 4 (lane >> 5) + (e & 3)
    const int limM = p.M - m0, limN = p.N - n0;
    const int fl = lane & 31, kl = lane >> 5;
    constexpr bool F32 = OUTF32 || EPI == 6;
    char* cbase = (EPI == 6) ? reinterpret_cast<char*>(p.partial + ((size_t)split * p.M + m0) * p.N + n0)
                             : reinterpret_cast<char*>(p.C) + ((size_t)m0 * p.ldc + n0) * (F32 ? 4 : 2);
    const unsigned ldc = (EPI == 6) ? (unsigned)p.N : (unsigned)p.ldc;
    const __amdgpu_buffer_rsrc_t cw = make_window(cbase);
    const __amdgpu_buffer_rsrc_t dw = make_window((EPI == 3 || EPI == 4) ? reinterpret_cast<const char*>(p.dref + (size_t)m0 * p.ldr + n0) : cbase);
    const __amdgpu_buffer_rsrc_t biasw = make_window((EPI == 1 || EPI == 2 || EPI == 5) ? reinterpret_cast<const char*>(p.bias + n0) : cbase);
    const bool accum = (EPI == 0) && F32 && p.accumulate;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = wm0 + i * 32 + fl;
        const bool mok = m < limM;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = wn0 + j * 32 + 8 * q + 4 * kl;
                const bool ok = mok && n < limN;                  // N % 4 == 0: a group of 4 columns is in or out as a whole
                float v[4] = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
                if (EPI == 1 || EPI == 2 || EPI == 5) {
                    const u32x4 bv = __builtin_amdgcn_raw_buffer_load_b128(biasw, ok ? (unsigned)n * 4u : OOB_OFF, 0, 0);
                    v[0] += __uint_as_float(bv.x); v[1] += __uint_as_float(bv.y); v[2] += __uint_as_float(bv.z); v[3] += __uint_as_float(bv.w);
                    if (EPI == 1) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] = act_fwd_c<ACT_LEAKY>(v[t]);
                    } else if (EPI == 2) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) v[t] = act_fwd_c<ACT_TANH>(v[t]);
                    }
                }
                if (EPI == 3 || EPI == 4) {
                    const u32x2 y = __builtin_amdgcn_raw_buffer_load_b64(dw, ok ? ((unsigned)m * (unsigned)p.ldr + (unsigned)n) * 2u : OOB_OFF, 0, 0);
                    const float ys[4] = {bf_lo(y.x), bf_hi(y.x), bf_lo(y.y), bf_hi(y.y)};
#pragma unroll
                    for (int t = 0; t < 4; ++t) v[t] *= (EPI == 3) ? (ys[t] > 0.f ? 1.f : 0.2f) : (1.f - ys[t] * ys[t]);
                }
                if (F32) {
                    const unsigned o = ok ? ((unsigned)m * ldc + (unsigned)n) * 4u : OOB_OFF;
                    if (accum) {
                        const u32x4 old = __builtin_amdgcn_raw_buffer_load_b128(cw, o, 0, 0);
                        v[0] += __uint_as_float(old.x); v[1] += __uint_as_float(old.y); v[2] += __uint_as_float(old.z); v[3] += __uint_as_float(old.w);
                    }
                    u32x4 w;
                    w.x = __float_as_uint(v[0]); w.y = __float_as_uint(v[1]); w.z = __float_as_uint(v[2]); w.w = __float_as_uint(v[3]);
                    __builtin_amdgcn_raw_buffer_store_b128(w, cw, o, 0, 0);
                } else {
                    u32x2 w;
                    w.x = pack_bf2(v[0], v[1]); w.y = pack_bf2(v[2], v[3]);
                    __builtin_amdgcn_raw_buffer_store_b64(w, cw, ok ? ((unsigned)m * ldc + (unsigned)n) * 2u : OOB_OFF, 0, 0);
                }
            }
    }
}

// [0] 128x128, [1] 256x128 / 8 waves, [2] 256x128 / 4 waves, [3] 256x64, [4] 256x32; of the LAST launch: [5] fp32 output, [6] epilogue
// variant, [7] K-splits (test / bench aid, not thread-safe)
static long long g_b16_launches[8];
static int g_b16_variant = -1;
extern "C" void cham_gemm_b16_set_variant(int v) { g_b16_variant = v; }
extern "C" void cham_gemm_b16_launch_counts(long long* out8, int reset) {
    for (int i = 0; i < 8; ++i) { if (out8) out8[i] = g_b16_launches[i]; if (reset && i < 5) g_b16_launches[i] = 0; }
}

// One tile instance (BK = 32): tile_plan::epilogue_b16 picks EPI and what the kernel writes, gemm_tile.h's ladder launches it and, after a
// split-K partial launch, the shared fixed-order reduction - wide up to 65536 float4 groups of output here (a [1024, 256] gradient).
template <int BM, int BN, int WM, int WN, bool AK, bool BKC>
static int b16_launch_cfg(B16Params& p, int act, int dact, int out_f32, hipStream_t st) {
    constexpr int BK = 32, NTH = WM * WN * 64;
    using LA = Stage16<BM, BK, AK, NTH>;
    using LB = Stage16<BN, BK, BKC, NTH>;
    constexpr size_t smem = (size_t)2 * ((AK ? BM * LA::LD : BK * LA::LD) + (BKC ? BN * LB::LD : BK * LB::LD)) * 2;
    bool f32;
    const int epi = tile_plan::epilogue_b16(!AK, p.bias != nullptr, act, p.dref != nullptr, dact, p.accumulate != 0, p.splits > 1, out_f32 != 0, f32);
    auto kernel = [&](auto e, auto f) -> int {
        constexpr int EPI = decltype(e)::value;
        constexpr bool OUTF32 = decltype(f)::value;
        if constexpr (tile_plan::instance_b16(EPI, OUTF32)) {
            g_b16_launches[5] = OUTF32;
            return tile_launch<gemm_b16_kernel<BM, BN, WM, WN, BK, 1, AK, BKC, EPI, OUTF32>>(p, EPI, NTH, smem, g_b16_launches + 6, st);
        } else {
            return -CHAM_ERR_ARG;
        }
    };
    return tile_ladder<BM, BN>(p, epi, 65536, st, [&](auto e) { return f32 ? kernel(e, std::true_type()) : kernel(e, std::false_type()); });
}

// tile_plan's tile index -> instance: 1 = 256x128 / 8 waves (64x64 per wave), 2 = 256x128 / 4 waves (128x64 per wave: half the LDS fragment
// bytes per MFMA; the NT epilogues push that instance past 256 VGPRs and it loses, 425 vs 653 TFLOP/s).  The tile counter moves before the
// ladder can reject the call.
template <bool AK, bool BKC>
static int b16_by_shape(B16Params& p, int act, int dact, int out_f32, hipStream_t st) {
    int counter;
    const int t = tile_plan::tile_b16(p.M, p.N, p.splits, !AK, g_b16_variant, counter);
    ++g_b16_launches[counter];
    switch (t) {
        case 1: return b16_launch_cfg<256, 128, 4, 2, AK, BKC>(p, act, dact, out_f32, st);
        case 2: return b16_launch_cfg<256, 128, 2, 2, AK, BKC>(p, act, dact, out_f32, st);
        case 3: return b16_launch_cfg<256, 64, 4, 1, AK, BKC>(p, act, dact, out_f32, st);
        case 4: return b16_launch_cfg<256, 32, 4, 1, AK, BKC>(p, act, dact, out_f32, st);
        default: return b16_launch_cfg<128, 128, 2, 2, AK, BKC>(p, act, dact, out_f32, st);
    }
}

// C[M,N] (+)= epi(op(A) op(B)) with bf16 operands resident in HBM.
//   transA = 0, transB = 1 (NT): A [M, lda] and B [N, ldb] k-contiguous; C bf16 (out_f32 = 0) or fp32; epilogues: + bias (fp32)
//     and act (CHAM_ACT_*), or x act'(dref) with dref the SAVED bf16 activation [M, ldr] (dgrad; bf16 out).
//   transA = 1, transB = 0 (TN): A stored [K, lda >= M], B stored [K, ldb >= N]; C fp32, optional accumulate; split-K through
//     `workspace` (splits_hint: 1 = none, 0 = automatic, n = at most n; deterministic fixed-order reduction).
// Extents: K % 8 == 0 (NT) / M % 8 == 0 and N % 8 == 0 (TN), N % 4 == 0, leading dimensions % 8 == 0, 16-byte aligned bases.
extern "C" int cham_gemm_b16(const void* A, int lda, int transA, const void* B, int ldb, int transB, void* C, int ldc, int out_f32,
                             int M, int N, int K, const float* bias, int act, const void* dref, int ldr, int dact, int accumulate,
                             float* workspace, size_t workspace_bytes, int splits_hint, void* stream) {
    const tile_plan::Args a = {A, lda, transA, B, ldb, transB, C, ldc, M, N, K, bias, act, dref, ldr, dact, nullptr, 0, 1,
                               accumulate, workspace, workspace_bytes, splits_hint};
    tile_plan::SplitPlan plan;
    const int rc = tile_plan::plan_b16(a, plan);
    if (rc != CHAM_OK) return rc;
    B16Params p;
    p.A = reinterpret_cast<const __bf16*>(A); p.B = reinterpret_cast<const __bf16*>(B); p.C = C;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb; p.ldc = ldc;
    p.bias = bias; p.dref = reinterpret_cast<const __bf16*>(dref); p.ldr = ldr;
    p.accumulate = accumulate; p.partial = workspace; p.xcd_split = 0;
    p.kchunk = plan.kchunk; p.splits = plan.splits;
    hipStream_t st = (hipStream_t)stream;
    if (transB) return b16_by_shape<true, true>(p, act, dact, out_f32, st);
    return b16_by_shape<false, false>(p, act, dact, out_f32, st);
}
