// Stand-alone driver of chameleon_recsys_amd/csrc/gemm_tile_plan.h for tests/test_gemm_tile_plan_cpu.py: one case per line of standard
// input, one result per line of standard output.  Pointers are given as integers and never dereferenced.
//   F | B  A lda transA B ldb transB C ldc M N K bias act dref ldr dact rowscale ldrs rs_div accumulate workspace workspace_bytes splits_hint
//          ->  rc [kchunk splits]                                  (F: plan_f32, B: plan_b16)
//   E ak bkc bias act dref dact accumulate split                   ->  epilogue_f32, instance_f32 of it (or 0), row_scale_instance of it (or 0)
//   G tn bias act dref dact accumulate split out_f32               ->  epilogue_b16, f32 flag, instance_b16 of it (or 0)
//   I epi ak bkc f32                                               ->  instance_f32, row_scale_instance, instance_b16(epi, f32)
//   T family M N K splits ak bkc forced                            ->  tile [counter]   (family 0 f32, 1 bf16, 2 x3, 3 b16 with tn = !ak)
#include <cstdio>
#include <cstring>

#include "../chameleon_recsys_amd/csrc/gemm_tile_plan.h"

static const void* P(unsigned long long v) { return (const void*)(uintptr_t)v; }

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == 'F' || line[0] == 'B') {
            unsigned long long A, B, C, bias, dref, rs, ws, bytes;
            int lda, tA, ldb, tB, ldc, M, N, K, act, ldr, dact, ldrs, rs_div, accumulate, hint;
            if (sscanf(line + 1, "%llu %d %d %llu %d %d %llu %d %d %d %d %llu %d %llu %d %d %llu %d %d %d %llu %llu %d", &A, &lda, &tA, &B, &ldb, &tB, &C,
                       &ldc, &M, &N, &K, &bias, &act, &dref, &ldr, &dact, &rs, &ldrs, &rs_div, &accumulate, &ws, &bytes, &hint) != 23)
                return 2;
            const tile_plan::Args a = {P(A), lda, tA, P(B), ldb, tB, P(C), ldc, M, N, K, P(bias), act, P(dref), ldr, dact, P(rs), ldrs, rs_div,
                                       accumulate, P(ws), (size_t)bytes, hint};
            tile_plan::SplitPlan plan = {0, 0};
            const int rc = line[0] == 'F' ? tile_plan::plan_f32(a, plan) : tile_plan::plan_b16(a, plan);
            if (rc == tile_plan::kOk) printf("%d %d %d\n", rc, plan.kchunk, plan.splits);
            else printf("%d\n", rc);
        } else if (line[0] == 'E') {
            int ak, bkc, bias, act, dref, dact, acc, split;
            if (sscanf(line + 1, "%d %d %d %d %d %d %d %d", &ak, &bkc, &bias, &act, &dref, &dact, &acc, &split) != 8) return 2;
            const int e = tile_plan::epilogue_f32(ak != 0, bkc != 0, bias != 0, act, dref != 0, dact, acc != 0, split != 0);
            printf("%d %d %d\n", e, e >= 0 && tile_plan::instance_f32(e, ak != 0, bkc != 0), e >= 0 && tile_plan::row_scale_instance(e, ak != 0, bkc != 0));
        } else if (line[0] == 'G') {
            int tn, bias, act, dref, dact, acc, split, out;
            if (sscanf(line + 1, "%d %d %d %d %d %d %d %d", &tn, &bias, &act, &dref, &dact, &acc, &split, &out) != 8) return 2;
            bool f32 = false;
            const int e = tile_plan::epilogue_b16(tn != 0, bias != 0, act, dref != 0, dact, acc != 0, split != 0, out != 0, f32);
            printf("%d %d %d\n", e, (int)f32, e >= 0 && tile_plan::instance_b16(e, f32));
        } else if (line[0] == 'I') {
            int epi, ak, bkc, f32;
            if (sscanf(line + 1, "%d %d %d %d", &epi, &ak, &bkc, &f32) != 4) return 2;
            printf("%d %d %d\n", (int)tile_plan::instance_f32(epi, ak != 0, bkc != 0), (int)tile_plan::row_scale_instance(epi, ak != 0, bkc != 0),
                   (int)tile_plan::instance_b16(epi, f32 != 0));
        } else if (line[0] == 'T') {
            int fam, M, N, K, splits, ak, bkc, forced;
            if (sscanf(line + 1, "%d %d %d %d %d %d %d %d", &fam, &M, &N, &K, &splits, &ak, &bkc, &forced) != 8) return 2;
            int counter = -1;
            if (fam == 0) printf("%d\n", tile_plan::tile_f32(M, N, K, splits, ak != 0, bkc != 0, forced));
            else if (fam == 1) printf("%d\n", tile_plan::tile_bf16(M, N, splits, forced));
            else if (fam == 2) printf("%d\n", tile_plan::tile_x3(M, N, splits, forced));
            else { const int t = tile_plan::tile_b16(M, N, splits, !ak, forced, counter); printf("%d %d\n", t, counter); }
        } else if (line[0] != '\n' && line[0] != '#') {
            return 2;
        }
    }
    return 0;
}
