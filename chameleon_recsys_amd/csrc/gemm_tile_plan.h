// Host-side decisions of the register-staged GEMM families (gemm.hip: cham_gemm_f32 / _bf16; gemm_x3.hip: cham_gemm_f32x3 / _f32x2h;
// gemm_b16.hip: cham_gemm_b16): which arguments they take, how a TN (weight-gradient) call is cut into K-splits, which epilogue a call asks
// for, which kernel instances exist, and which tile a shape runs on.  Pure functions of plain C++17 - no HIP include - so that
// tests/test_gemm_tile_plan_cpu.py runs them in a stand-alone host program (also under ASan / UBSan).  gemm_tile.h turns them into launches.
// "f32" below = the families with fp32 storage (gemm.hip, gemm_x3.hip: same rules), "b16" = bf16-resident operands (gemm_b16.hip).
#pragma once
#include <cstddef>
#include <cstdint>

namespace tile_plan {

constexpr int kOk = 0, kErrArg = 22;                         // CHAM_OK, CHAM_ERR_ARG (common.h; gemm_shared.h asserts the values)
constexpr int kActNone = 0, kActLeaky = 1, kActTanh = 2;     // ACT_* (common.h)
constexpr size_t kWindowBytes = 0x7FFFF000;                  // WINDOW_BYTES (gemm_shared.h): what a tile window addresses

struct Args {          // one call; pointers are compared and tested for alignment, never dereferenced
    const void* A; int lda; int transA;
    const void* B; int ldb; int transB;
    const void* C; int ldc;
    int M, N, K;
    const void* bias; int act;
    const void* dref; int ldr; int dact;
    const void* rowscale; int ldrs; int rs_div;              // f32 only
    int accumulate;
    const void* workspace; size_t workspace_bytes; int splits_hint;
};

// ---- argument checks ------------------------------------------------------------------------------------------------------------
inline int check_f32(const Args& a) {
    if (!a.A || !a.B || !a.C || a.M <= 0 || a.N <= 0 || a.K < 0) return -kErrArg;
    if ((a.lda & 3) || (a.ldb & 3)) return -kErrArg;
    // contiguous extents must be float4 multiples (model dims are padded on the host side)
    if (!a.transA && (a.K & 3)) return -kErrArg;         // A[M,K] row-major, k contiguous
    if (a.transA && (a.M & 3)) return -kErrArg;          // A stored [K,M]
    if (!a.transB && (a.N & 3)) return -kErrArg;         // B[K,N] row-major
    if (a.transB && (a.K & 3)) return -kErrArg;          // B stored [N,K]
    if (a.rowscale && ((a.ldrs & 3) || a.rs_div <= 0)) return -kErrArg;
    // a leading dimension is never smaller than the extent it strides over (with ldc < N the rows of C would overwrite each other)
    if (a.lda < (a.transA ? a.M : a.K) || a.ldb < (a.transB ? a.K : a.N) || a.ldc < a.N || (a.dref && a.ldr < a.N) ||
        (a.rowscale && a.ldrs < (a.transA ? a.M : a.K)))
        return -kErrArg;
    // tile windows address 2^31 bytes with 32-bit offsets: a 256-row (or 32-k-row) slab of any operand must fit
    if ((size_t)a.lda * 4 * 256 >= kWindowBytes || (size_t)a.ldb * 4 * 256 >= kWindowBytes || (size_t)a.ldc * 4 * 256 >= kWindowBytes ||
        (size_t)a.ldr * 4 * 256 >= kWindowBytes)
        return -kErrArg;
    if (a.rowscale && (size_t)((a.transA ? a.K : a.M) / (a.rs_div > 0 ? a.rs_div : 1) + 1) * a.ldrs * 4 >= kWindowBytes) return -kErrArg;
    return kOk;
}

// b16: NT or TN only; 16-byte staging units (8 bf16) and output groups of four columns
inline int check_b16(const Args& a) {
    if (!a.A || !a.B || !a.C || a.M <= 0 || a.N <= 0 || a.K <= 0) return -kErrArg;
    if ((a.lda & 7) || (a.ldb & 7) || (a.N & 3) || (a.ldc & 3) || (a.dref && (a.ldr & 3))) return -kErrArg;
    if (((uintptr_t)a.A | (uintptr_t)a.B | (uintptr_t)a.C | (uintptr_t)a.dref | (uintptr_t)a.bias) & 15) return -kErrArg;
    const bool nt = !a.transA && a.transB, tn = a.transA && !a.transB;
    if (!nt && !tn) return -kErrArg;
    if (nt && (a.K & 7)) return -kErrArg;
    if (tn && ((a.M & 7) || (a.N & 7))) return -kErrArg;
    if (a.lda < (tn ? a.M : a.K) || a.ldb < (tn ? a.N : a.K) || a.ldc < a.N || (a.dref && a.ldr < a.N)) return -kErrArg;
    if ((size_t)a.lda * 2 * 256 >= kWindowBytes || (size_t)a.ldb * 2 * 256 >= kWindowBytes || (size_t)a.ldc * 4 * 256 >= kWindowBytes ||
        (size_t)a.ldr * 2 * 256 >= kWindowBytes)
        return -kErrArg;
    return kOk;
}

// ---- the split-K plan -----------------------------------------------------------------------------------------------------------
struct SplitPlan {
    int kchunk;          // k extent of one split, a multiple of the family's kchunk_multiple
    int splits;          // >= 1; > 1: the kernel stores partial slabs, gemm_splitk_reduce[_wide] adds them in a fixed order
};

// K-splits are a weight-gradient device (long reduction, small output): fill >= ~512 workgroups.  splits_hint: 1 = none, 0 = automatic,
// n = at most n.  `tiles` = the family's estimate of the output tiles; either count is capped by min_k_per_split reduction steps per split
// and by the workspace (M x N floats per split); groups_of_8: whole K-splits per XCD (b16).  K = 0 (f32 takes it) plans one empty chunk.
inline SplitPlan plan_splits(int M, int N, int K, bool may_split, size_t workspace_bytes, int splits_hint, long tiles, int min_k_per_split,
                             int kchunk_multiple, bool groups_of_8) {
    int splits = 1;
    if (may_split && splits_hint != 1) {
        long want = splits_hint > 1 ? splits_hint : (tiles >= 384 ? 1 : (512 + tiles - 1) / tiles);
        const long maxk = (K + min_k_per_split - 1) / min_k_per_split;
        if (want > maxk) want = maxk;
        const long maxw = (long)(workspace_bytes / ((size_t)M * N * sizeof(float)));
        if (want > maxw) want = maxw;
        if (groups_of_8 && want >= 8) want = want / 8 * 8;
        if (want > 1) splits = (int)want;
    }
    SplitPlan out;
    out.kchunk = (K + splits - 1) / splits;
    out.kchunk = ((out.kchunk + kchunk_multiple - 1) / kchunk_multiple) * kchunk_multiple;
    if (out.kchunk == 0) out.kchunk = kchunk_multiple;
    out.splits = (K + out.kchunk - 1) / out.kchunk;
    if (out.splits < 1) out.splits = 1;
    return out;
}

inline long ceil_tiles(int M, int N, int bm, int bn) { return (long)((M + bm - 1) / bm) * ((N + bn - 1) / bn); }

// f32: checks + plan.  >= 256 reduction steps per split, kchunk a multiple of 64 (every BK, and gemm_x3.hip's four-tile unrolled body).
// Only TN has split-K instances; the reductions walk the output in float4 groups of one row and read the bias 16 bytes at a time, so an
// output width that is not a multiple of four or a misaligned bias takes the unsplit kernel.
inline int plan_f32(const Args& a, SplitPlan& out) {
    const int rc = check_f32(a);
    if (rc != kOk) return rc;
    const bool reduce_ok = (a.N & 3) == 0 && (!a.bias || ((uintptr_t)a.bias & 15) == 0);
    const int bm = (a.N > 64) ? (((long)a.M * a.N >= (1L << 20)) ? 256 : 128) : 256, bn = (a.N > 64) ? 128 : (a.N > 32 ? 64 : 32);
    out = plan_splits(a.M, a.N, a.K, a.workspace && reduce_ok && a.transA && !a.transB, a.workspace_bytes, a.splits_hint,
                      ceil_tiles(a.M, a.N, bm, bn), 256, 64, false);
    return kOk;
}
// b16: >= 512 reduction steps per split, kchunk a multiple of 32 (BK), whole groups of 8 splits, 256-row tiles in the estimate
inline int plan_b16(const Args& a, SplitPlan& out) {
    const int rc = check_b16(a);
    if (rc != kOk) return rc;
    const int bn = (a.N > 64) ? 128 : (a.N > 32 ? 64 : 32);
    out = plan_splits(a.M, a.N, a.K, a.transA && a.workspace, a.workspace_bytes, a.splits_hint, ceil_tiles(a.M, a.N, 256, bn), 512, 32, true);
    return kOk;
}

// ---- epilogues (the EPI numbers of gemm_shared.h's gemm_epilogue): 0 plain / accumulate, 1 bias + leaky, 2 bias + tanh, 3 x leaky'(dref),
// 4 x tanh'(dref), 5 bias only, 6 split-K partial.  Layout: ak = A k-contiguous (not transposed), bkc = B k-contiguous (transposed).
// f32:  NN (forward) plain | bias | bias + leaky | bias + tanh;  NT (dgrad) plain / accumulate | x leaky'(dref) | x tanh'(dref);
//       TN (wgrad) plain / accumulate | split-K partial (bias / act / dref are then applied by the reduction).
inline int epilogue_f32(bool ak, bool bkc, bool bias, int act, bool dref, int dact, bool accumulate, bool split) {
    const bool nn = ak && !bkc, nt = ak && bkc, tn = !ak && !bkc;
    if (split) return tn ? 6 : -kErrArg;
    if (dref) {
        if (bias || act != kActNone || !nt) return -kErrArg;
        return dact == kActLeaky ? 3 : (dact == kActTanh ? 4 : -kErrArg);
    }
    if (bias || act != kActNone) {
        if (!bias || accumulate || !nn) return -kErrArg;          // every activated layer of the model has a bias
        return act == kActLeaky ? 1 : (act == kActTanh ? 2 : 5);
    }
    return 0;
}
constexpr bool instance_f32(int epi, bool ak, bool bkc) {
    return epi == 0 || ((epi == 1 || epi == 2 || epi == 5) && ak && !bkc) || ((epi == 3 || epi == 4) && ak && bkc) || (epi == 6 && !ak && !bkc);
}
// the row-broadcast scale only ever accompanies the scorer's first layer (bias + leaky, NN) and its wgrad (TN; split-K, or plain when the
// reduction is too short to split: a batch with a handful of valid positions): the instances that exist with a row scale
constexpr bool row_scale_instance(int epi, bool ak, bool bkc) { return (epi == 1 && ak && !bkc) || ((epi == 6 || epi == 0) && !ak && !bkc); }

// b16:  TN (wgrad) fp32 out, plain / accumulate | split-K partial;  NT, bf16 out: plain | bias + leaky | bias + tanh | x leaky'(dref); plain
//       also with fp32 out.  (tanh' dgrads and bias-only layers of the model run on fp32-resident operands.)  f32 = what the kernel writes.
inline int epilogue_b16(bool tn, bool bias, int act, bool dref, int dact, bool accumulate, bool split, bool out_f32, bool& f32) {
    f32 = out_f32;
    if (tn) {
        if (bias || act != kActNone || dref || !out_f32) return -kErrArg;
        return split ? 6 : 0;
    }
    if (split || accumulate) return -kErrArg;
    if (dref) return (bias || act != kActNone || out_f32 || dact != kActLeaky) ? -kErrArg : 3;
    if (bias) {
        if (out_f32) return -kErrArg;
        return act == kActLeaky ? 1 : (act == kActTanh ? 2 : -kErrArg);
    }
    return act != kActNone ? -kErrArg : 0;
}
// (EPI, what the kernel writes) with an instance; every tile has them for both layouts, as gemm_b16.hip has always been built
constexpr bool instance_b16(int epi, bool f32) { return epi == 0 || (f32 ? epi == 6 : (epi == 1 || epi == 2 || epi == 3)); }

// ---- tiles: the largest tile whose grid still gives every one of the 256 CUs a workgroup.  Results index the families' launch counters:
// 0 = 128x128, 1 = 256x128, 2 = 256x256 (f32) / 256x128 on 4 waves (b16), 3 = 256x64, 4 = 256x32.  forced >= 0: cham_gemm*_set_variant.
inline long grid_of(int M, int N, int bm, int bn, int splits) { return ceil_tiles(M, N, bm, bn) * splits; }
inline int narrow_tile(int N) { return N > 32 ? 3 : 4; }

// cham_gemm_f32: NT (dgrad) and TN (wgrad, long K) prefer the 256x256 tile; forced: 2 = 256x128, 4 = 256x256, else 128x128
inline int tile_f32(int M, int N, int K, int splits, bool ak, bool bkc, int forced) {
    if (N <= 64) return narrow_tile(N);
    int v = ((long)M * N >= (1L << 20)) ? 2 : 0;
    if (v == 2 && (!ak || bkc) && K >= 512 && M >= 1024 && N >= 512) v = 4;
    if (v == 4 && grid_of(M, N, 256, 256, splits) < 256) v = 2;       // ... demoted while the grid does not cover the chip
    if (v == 2 && grid_of(M, N, 256, 128, splits) < 256) v = 0;
    if (forced >= 0) v = forced;
    return v == 2 ? 1 : (v == 4 ? 2 : 0);
}
// cham_gemm_bf16 (forced: >= 2 = 256x128) and cham_gemm_f32x3 / _f32x2h (x3: every N; forced: 2 = 256x128, else 128x128)
inline int tile_bf16(int M, int N, int splits, int forced) {
    if (N <= 64) return narrow_tile(N);
    bool big = (long)M * N >= (1L << 20) && grid_of(M, N, 256, 128, splits) >= 256;
    if (forced >= 0) big = forced >= 2;
    return big ? 1 : 0;
}
inline int tile_x3(int M, int N, int splits, int forced) {
    int v = ((long)M * N >= (1L << 20) && grid_of(M, N, 256, 128, splits) >= 256) ? 2 : 0;
    if (forced >= 0) v = forced;
    return v == 2 ? 1 : 0;
}
// cham_gemm_b16: 256x128 / 8 waves while the grid covers the chip; TN with K-splits (the split-K partial epilogue: 208 VGPRs, two workgroups
// per CU) is faster on the 4-wave instance, 128x64 per wave.  forced: 0, 1, 2 = the instance; above: the 128x128 instance, counted at [2].
inline int tile_b16(int M, int N, int splits, bool tn, int forced, int& counter) {
    if (N <= 64) return counter = narrow_tile(N);
    int v = (grid_of(M, N, 256, 128, splits) >= 256) ? 1 : 0;
    if (v == 1 && tn && splits > 1) v = 2;
    if (forced >= 0) v = forced;
    counter = v < 3 ? v : 2;
    return (v == 1 || v == 2) ? v : 0;
}

}  // namespace tile_plan
