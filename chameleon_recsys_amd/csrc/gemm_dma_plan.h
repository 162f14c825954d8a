// Host-side decisions of the LDS-DMA GEMM entry points (cham_gemm_p3, cham_gemm_b16_dma, cham_gemm_h2 / _h2b / _h2_dgrad_gs): which
// arguments they take, which NT epilogue a call asks for, and how a TN (weight-gradient) call is cut into K-splits.  Pure functions of plain
// C++17 - no HIP include - so that tests/test_gemm_dma_plan_cpu.py runs them in a stand-alone host program (also under ASan / UBSan).
// What only ONE family checks (tile-blocked operands, group sums, the scale records, the wide-NT switches) stays in its entry point.
#pragma once
#include <cstddef>
#include <cstdint>

namespace dma_plan {

constexpr int kOk = 0, kErrArg = 22;                         // CHAM_OK, CHAM_ERR_ARG (common.h; gemm_dma.h asserts the values)
constexpr int kActNone = 0, kActLeaky = 1, kActTanh = 2;     // ACT_* (common.h)
constexpr size_t kWindowBytes = 0x7FFFF000;                  // WINDOW_BYTES (gemm_shared.h): what a tile window addresses
constexpr int kTile = 256;                                   // every kernel of the core works on 256 x 256 output tiles

struct Args {
    const void* A; const void* B; const void* C;             // plane 0 of each operand, the output
    long long a_plane_stride, b_plane_stride;                // elements between an operand's planes (0: one plane)
    int lda, ldb, ldc;
    int tn;                                                  // 0: NT, A [M, lda] and B [N, ldb] k-contiguous; 1: TN, A [K, lda >= M], B [K, ldb >= N]
    int M, N, K;
    const void* bias; int act;
    const void* dref; int ldr; int dact;                     // saved activation of the dgrad epilogue (16-bit elements)
    int accumulate;
};

// The argument checks the three families share; -kErrArg for what none of their kernels takes.
//   kstep: the k extent of one TN stage (16, or 48 for the one-plane bf16 form) - a stage's k-rows must stay inside 32-bit offsets.
//   vector_epilogue: the bf16-out epilogues read bias 16 and dref 8 bytes at a time (gemm_b1_kernel), the fp32-out ones element by element.
inline int check_args(const Args& a, int kstep, bool vector_epilogue) {
    if (!a.A || !a.B || !a.C || a.M <= 0 || a.N <= 0 || a.K <= 0) return -kErrArg;
    // 16-byte DMA pieces and 16-byte output groups
    if ((a.lda & 7) || (a.ldb & 7) || (a.a_plane_stride & 7) || (a.b_plane_stride & 7) || (a.N & 3) || (a.ldc & 3)) return -kErrArg;
    if (((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C) & 15) return -kErrArg;
    if (vector_epilogue && ((a.dref && (a.ldr & 3)) || (((uintptr_t)a.dref | (uintptr_t)a.bias) & 15))) return -kErrArg;
    // tile windows address 2^31 bytes with 32-bit offsets: a 256-row slab of C (4-byte elements at most) and of dref must fit
    if ((size_t)a.ldc * 4 * kTile >= kWindowBytes || (size_t)a.ldr * 2 * kTile >= kWindowBytes) return -kErrArg;
    // a leading dimension is never smaller than the extent it strides over
    if (a.lda < (a.tn ? a.M : a.K) || a.ldb < (a.tn ? a.N : a.K) || a.ldc < a.N || (a.dref && a.ldr < a.N)) return -kErrArg;
    if (!a.tn) {
        if ((a.K & 15) || a.accumulate) return -kErrArg;
        if ((size_t)kTile * a.lda * 2 >= (1ull << 31) || (size_t)kTile * a.ldb * 2 >= (1ull << 31)) return -kErrArg;
        return kOk;
    }
    // TN: whole tiles (the m / n extent of a tile never leaves its k-row), no epilogue but the split-K partial
    if ((a.M & (kTile - 1)) || (a.N & (kTile - 1)) || a.bias || a.act != kActNone || a.dref) return -kErrArg;
    if ((size_t)kstep * a.lda * 2 >= (1ull << 31) || (size_t)kstep * a.ldb * 2 >= (1ull << 31)) return -kErrArg;
    return kOk;
}

// NT epilogue of a call: 0 plain, 2 bias + tanh, 3 x leaky'(dref), 5 bias only (the fp32-out families; bias_only_ok) - the EPI numbers of
// gemm_shared.h's gemm_epilogue - or -kErrArg for a combination no kernel instance computes.
inline int nt_epilogue(bool bias, int act, bool dref, int dact, bool bias_only_ok) {
    if (dref) return (bias || act != kActNone || dact != kActLeaky) ? -kErrArg : 3;
    if (bias) {
        if (act == kActTanh) return 2;
        return (act == kActNone && bias_only_ok) ? 5 : -kErrArg;
    }
    return act != kActNone ? -kErrArg : 0;
}

struct SplitPlan {
    int kchunk;          // k extent of one split: a multiple of kstep
    int splits;          // >= 1; > 1: the kernel stores partials, gemm_splitk_reduce adds them in ascending order
    int xcd_split;       // one K-split per XCD (gemm_shared.h gemm_tile_map): whole groups of 8 splits only
};

// TN split-K plan.  One workgroup per CU: below 192 tiles the automatic plan (splits_hint <= 0) asks for 256 workgroups, rounded down to whole
// groups of 8 splits (one per XCD); an explicit count (splits_hint > 1) is taken as given (e.g. 14 splits x 16 tiles = 224 workgroups: one
// round that leaves 32 CUs to the kernels of the other lane).  Either is capped by min_k_per_split reduction steps per split and by the
// workspace (M x N floats per split).  -kErrArg when a split's k-rows of the wider operand leave the 32-bit descriptor range.
inline int plan_tn_splits(int M, int N, int K, int lda, int ldb, bool have_workspace, size_t workspace_bytes, int splits_hint, int kstep,
                          int min_k_per_split, SplitPlan& out) {
    if (M <= 0 || N <= 0 || K <= 0 || kstep <= 0 || min_k_per_split <= 0) return -kErrArg;
    const long tiles = (long)((M + kTile - 1) / kTile) * ((N + kTile - 1) / kTile);
    int splits = 1;
    if (splits_hint != 1 && have_workspace) {
        long want = splits_hint > 1 ? splits_hint : (tiles >= 192 ? 1 : (256 + tiles - 1) / tiles);
        const long maxk = ((long)K + min_k_per_split - 1) / min_k_per_split;
        if (want > maxk) want = maxk;
        const long maxw = (long)(workspace_bytes / ((size_t)M * N * sizeof(float)));
        if (want > maxw) want = maxw;
        if (splits_hint <= 0 && want >= 8) want = want / 8 * 8;
        if (want > 1) splits = (int)want;
    }
    int kchunk = (K + splits - 1) / splits;
    kchunk = ((kchunk + kstep - 1) / kstep) * kstep;
    out.kchunk = kchunk;
    out.splits = (K + kchunk - 1) / kchunk;
    out.xcd_split = (out.splits > 1 && out.splits % 8 == 0) ? 1 : 0;
    if ((size_t)kchunk * (lda > ldb ? lda : ldb) * 2 >= 0xFFFFFFF0ull) return -kErrArg;
    return kOk;
}

}  // namespace dma_plan
