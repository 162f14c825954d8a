// Host side of the three register-staged GEMM families (gemm.hip, gemm_x3.hip, gemm_b16.hip): the one launch helper, the one switch from
// the epilogue number that gemm_tile_plan.h decided to the kernels' EPI template argument, and the one ladder around them (tile counts,
// the split-K partial launch followed by the fixed-order reduction).  A family supplies a generic lambda that names its kernel for an EPI.
#pragma once
#include "gemm_shared.h"
#include <type_traits>

// (gemm_x3.hip hands narrow and small-output shapes to gemm.hip through its entry point)
extern "C" int cham_gemm_f32(const float* A, int lda, int transA, const float* B, int ldb, int transB, float* C, int ldc, int M, int N, int K,
                             const float* bias, int act, const float* dref, int ldr, int dact, const float* rowscale, int ldrs, int rs_div,
                             int accumulate, float* workspace, size_t workspace_bytes, int splits_hint, void* stream);

// One launch: nbm x nbn tiles times the K-splits.  last = the family's two "last launch" counters: epilogue, K-splits.
template <auto KERNEL, class P>
static int tile_launch(const P& p, int epi, int threads, size_t smem, long long* last, hipStream_t st) {
    last[0] = epi; last[1] = p.splits;
    CHAM_SET_DYNAMIC_LDS(KERNEL, (int)smem);
    hipLaunchKernelGGL(KERNEL, dim3(p.nbm * p.nbn, p.splits, 1), dim3(threads), smem, st, p);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// runtime EPI -> f(std::integral_constant<int, EPI>).  f instantiates a kernel only where tile_plan::instance_f32 / _b16 says one exists
// (every epilogue for every layout would be a third of the library's code size more).
template <class F>
static int with_epi(int epi, F&& f) {
    switch (epi) {
        case 0: return f(std::integral_constant<int, 0>());
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 5: return f(std::integral_constant<int, 5>());
        case 6: return f(std::integral_constant<int, 6>());
    }
    return -CHAM_ERR_ARG;
}

// what the split-K reduction needs of a family's parameter block (a GemmParams goes as it is: the reduction applies its bias / act / dref)
static inline const GemmParams& reduce_params(const GemmParams& p) { return p; }
template <class P>
static GemmParams reduce_params(const P& p) {
    GemmParams g = {};
    g.C = (float*)p.C; g.M = p.M; g.N = p.N; g.K = p.K; g.ldc = p.ldc; g.act = ACT_NONE; g.dact = ACT_NONE; g.rs_div = 1;
    g.accumulate = p.accumulate; g.kchunk = p.kchunk; g.splits = p.splits; g.partial = p.partial;
    return g;
}

// The ladder of one tile instance: epi = the plan's epilogue number (or its rejection), launch = the family's EPI -> kernel lambda.
// xcd_split is set for the split-K partial launch only, for whole groups of 8 splits; its reduction follows on the same stream.
template <int BM, int BN, class P, class LAUNCH>
static int tile_ladder(P& p, int epi, size_t wide_max_n4, hipStream_t st, LAUNCH&& launch) {
    p.nbm = (p.M + BM - 1) / BM;
    p.nbn = (p.N + BN - 1) / BN;
    if (epi < 0) return epi;
    if (epi == 6) p.xcd_split = (p.splits % 8 == 0) ? 1 : 0;
    const int rc = with_epi(epi, launch);
    if (rc != CHAM_OK || epi != 6) return rc;
    launch_splitk_reduce(reduce_params(p), st, wide_max_n4);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// The fp32-storage families (GemmParams: gemm.hip, gemm_x3.hip).  kernel(EPI, RS) launches the family's instance; the row-scale instances
// exist where tile_plan::row_scale_instance says.  last[] is written before the row-scale rejection, as it always was.
template <int BM, int BN, bool AK, bool BKC, class KERNEL>
static int tile_ladder_f32(GemmParams& p, long long* last, hipStream_t st, KERNEL&& kernel) {
    const int epi = tile_plan::epilogue_f32(AK, BKC, p.bias != nullptr, p.act, p.dref != nullptr, p.dact, p.accumulate != 0, p.splits > 1);
    return tile_ladder<BM, BN>(p, epi, 32768, st, [&](auto e) -> int {
        constexpr int EPI = decltype(e)::value;
        if constexpr (tile_plan::instance_f32(EPI, AK, BKC)) {
            constexpr bool RSI = tile_plan::row_scale_instance(EPI, AK, BKC);
            if (p.rs != nullptr && !RSI) { last[0] = EPI; last[1] = p.splits; return -CHAM_ERR_ARG; }
            if constexpr (RSI) { if (p.rs != nullptr) return kernel(e, std::true_type()); }
            return kernel(e, std::false_type());
        } else {
            return -CHAM_ERR_ARG;
        }
    });
}
