// The LDS-DMA GEMM core shared by the plane-resident kernel families (gemm_p3.hip: three bf16 planes, and one bf16 plane per operand;
// gemm_h2.hip: two fp16 planes): 256 x 256 output tiles, 8 waves as 2 (M) x 4 (N), 4 x 2 MFMA tiles of 32x32x16 per wave, operand slabs
// that `buffer_load_dwordx4 ... lds` writes straight from global memory into LDS - the K loop holds MFMAs, fragment reads and DMA issue
// only.  The reasons for the slab layouts, swizzles and pipelines are in the design headers of the two .hip files; here is the one copy of
// what their kernels have in common.  A family supplies its stage statement (the operand list differs), its K loop and its own epilogue if it
// has one; the host side (bottom) turns a dma_plan decision (gemm_dma_plan.h) into launches.
#pragma once
#include "gemm_shared.h"
#include "gemm_dma_plan.h"

// buffer descriptor over `bytes` bytes from `base`: a request whose offset is out of range arrives as zeros (ragged rows, K tails)
__device__ __forceinline__ u32x4 dma_rsrc(const void* base, unsigned bytes) {
    const unsigned long long a = (unsigned long long)base;
    u32x4 r;
    r.x = (unsigned)a; r.y = (unsigned)(a >> 32) & 0xFFFFu; r.z = bytes; r.w = 0x00020000u;
    return r;
}

// LDS-only barrier: builtins so that the wait-count pass sees the drain; vmcnt is handled by hand (the DMA requests are invisible to
// the compiler).
__device__ __forceinline__ void dma_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_waitcnt(0xc07f);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
    __builtin_amdgcn_sched_barrier(0);
}

// One MFMA fragment (8 consecutive k of one row; V8 = bf16x8 or half8 - 16-bit elements, the type does not matter to the read).
// NT slab: 16 bytes as stored.  TN slab ([k][free index]): two transposed reads, k-rows k .. k + 3 and k + 4 .. k + 7; hi_off = byte
// distance of k-row + 4 in the slab image (4 * 512 for a row-major operand's image, 4 * 64 for a tile-blocked one's).
template <class V8, bool TN>
__device__ __forceinline__ V8 dma_frag(const unsigned char* __restrict__ s, unsigned hi_off = 4 * 512) {
    if constexpr (!TN) {
        return *reinterpret_cast<const V8*>(s);
    } else {
        typedef __attribute__((address_space(3))) s16x4 lds_s4;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(s));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4*)(s + hi_off));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        s16x8 v;
        v[0] = lo[0]; v[1] = lo[1]; v[2] = lo[2]; v[3] = lo[3]; v[4] = hi[0]; v[5] = hi[1]; v[6] = hi[2]; v[7] = hi[3];
        return __builtin_bit_cast(V8, v);
    }
}

// ---- wide NT (64-byte source pieces: gemm_h2w_kernel, gemm_b1w_kernel; slab = [256 rows][64 bytes]).
// four requests: (r0 @ v0 -> l0), (r0 @ v1 -> l0 + 1024), (r1 @ v0 -> l1), (r1 @ v1 -> l1 + 1024): the two 16-row halves of a wave's 32 rows
// in two slabs.  16 bytes per lane, LDS destination = M0 + lane * 16 (wave-uniform); M0 is compiler-reserved: saved and restored inside the
// statement (cdna_hip_programming.md 5.7).
// (The lane -> source piece map and the fragment offsets of the two wide kernels are the same text in both and stay there: as a helper here -
// through references or as scalar-valued functions - they changed both kernels' register allocation; profiles/gemm_dma_core_notes.md.)
__device__ __forceinline__ void dma4(unsigned l0, unsigned l1, unsigned v0, unsigned v1, const u32x4& r0, const u32x4& r1) {
    unsigned keep;
    const unsigned l0b = l0 + 1024u, l1b = l1 + 1024u;
    asm volatile(
        "s_nop 4\n\t"
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %7, 0 offen lds\n\t"
        "s_mov_b32 m0, %2\n\ts_nop 0\n\tbuffer_load_dwordx4 %6, %7, 0 offen lds\n\t"
        "s_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %5, %8, 0 offen lds\n\t"
        "s_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %6, %8, 0 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(l0), "s"(l0b), "s"(l1), "s"(l1b), "v"(v0), "v"(v1), "s"(r0), "s"(r1)
        : "memory");
}
// what gemm_epilogue (plain, + bias, + bias -> tanh, split-K partial) needs of a family's parameter block
template <class P>
__device__ __forceinline__ GemmParams epilogue_params(const P& p, const float* bias) {
    GemmParams g;
    g.A = nullptr; g.B = nullptr; g.C = p.C; g.M = p.M; g.N = p.N; g.K = p.K; g.lda = 0; g.ldb = 0; g.ldc = p.ldc;
    g.bias = bias; g.act = ACT_NONE; g.dref = nullptr; g.ldr = 0; g.dact = ACT_NONE; g.rs = nullptr; g.ldrs = 0; g.rs_div = 1;
    g.accumulate = p.accumulate; g.kchunk = p.kchunk; g.splits = p.splits; g.partial = p.partial; g.nbm = p.nbm; g.nbn = p.nbn; g.xcd_split = p.xcd_split;
    g.sa = nullptr; g.sb = nullptr;
    return g;
}

// ================================================================================================================================
// Host side.
static_assert(dma_plan::kOk == CHAM_OK && dma_plan::kErrArg == CHAM_ERR_ARG && dma_plan::kWindowBytes == WINDOW_BYTES, "gemm_dma_plan.h constants");
static_assert(dma_plan::kActNone == ACT_NONE && dma_plan::kActLeaky == ACT_LEAKY && dma_plan::kActTanh == ACT_TANH, "gemm_dma_plan.h constants");

// One launch: nbm x nbn tiles times grid_y K-splits, 512 threads, SMEM bytes of dynamic LDS.  counts = the family's launch counters:
// [6] epilogue and [7] K-splits of the last launch.
template <auto KERNEL, int SMEM, int EPI, class P>
static int dma_launch(const P& p, int grid_y, long long (&counts)[8], hipStream_t st) {
    counts[6] = EPI; counts[7] = grid_y;
    CHAM_SET_DYNAMIC_LDS(KERNEL, SMEM);
    hipLaunchKernelGGL(KERNEL, dim3(p.nbm * p.nbn, grid_y, 1), dim3(512), SMEM, st, p);
    CHAM_CHECK_LAUNCH();
    return CHAM_OK;
}

// fixed-order reduction of the partials a planned TN launch left in `workspace`
static inline void launch_splitk_reduce(float* C, int ldc, int M, int N, int K, int accumulate, const dma_plan::SplitPlan& plan, float* workspace,
                                        int nbm, int nbn, hipStream_t st) {
    GemmParams g = {};
    g.C = C; g.M = M; g.N = N; g.K = K; g.ldc = ldc; g.act = ACT_NONE; g.dact = ACT_NONE; g.rs_div = 1; g.accumulate = accumulate;
    g.kchunk = plan.kchunk; g.splits = plan.splits; g.partial = workspace; g.nbm = nbm; g.nbn = nbn; g.xcd_split = plan.xcd_split;
    launch_splitk_reduce(g, st);
}

// A planned TN call: the split-K partial kernel + the reduction, or the plain (accumulating) kernel when the plan has one split.
template <auto K_PARTIAL, auto K_PLAIN, int SMEM, class P>
static int dma_launch_tn(P& p, const dma_plan::SplitPlan& plan, int accumulate, long long (&counts)[8], hipStream_t st) {
    p.kchunk = plan.kchunk; p.splits = plan.splits;
    if (plan.splits > 1) {
        p.xcd_split = plan.xcd_split;
        const int rc = dma_launch<K_PARTIAL, SMEM, 6>(p, plan.splits, counts, st);
        if (rc != CHAM_OK) return rc;
        launch_splitk_reduce(p.C, p.ldc, p.M, p.N, p.K, accumulate, plan, p.partial, p.nbm, p.nbn, st);
        CHAM_CHECK_LAUNCH();
        return CHAM_OK;
    }
    p.accumulate = accumulate;
    return dma_launch<K_PLAIN, SMEM, 0>(p, 1, counts, st);
}
