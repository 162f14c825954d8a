// Stand-alone driver of chameleon_recsys_amd/csrc/gemm_dma_plan.h for tests/test_gemm_dma_plan_cpu.py: one case per line of standard
// input, one result per line of standard output.  Pointers are given as integers and never dereferenced.
//   P M N K lda ldb have_workspace workspace_bytes splits_hint kstep min_k_per_split     ->  rc [kchunk splits xcd_split]
//   C A B C a_ps b_ps lda ldb ldc tn M N K bias act dref ldr dact accumulate kstep vector_epilogue     ->  rc
//   E bias act dref dact bias_only_ok     ->  rc (the epilogue number, or the error)
#include <cstdio>
#include <cstring>

#include "../chameleon_recsys_amd/csrc/gemm_dma_plan.h"

int main() {
    char line[1024];
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == 'P') {
            int M, N, K, lda, ldb, have, hint, kstep, mink;
            unsigned long long bytes;
            if (sscanf(line + 1, "%d %d %d %d %d %d %llu %d %d %d", &M, &N, &K, &lda, &ldb, &have, &bytes, &hint, &kstep, &mink) != 10) return 2;
            dma_plan::SplitPlan plan = {0, 0, 0};
            const int rc = dma_plan::plan_tn_splits(M, N, K, lda, ldb, have != 0, (size_t)bytes, hint, kstep, mink, plan);
            if (rc == dma_plan::kOk) printf("%d %d %d %d\n", rc, plan.kchunk, plan.splits, plan.xcd_split);
            else printf("%d\n", rc);
        } else if (line[0] == 'C') {
            unsigned long long A, B, C, bias, dref;
            long long aps, bps;
            int lda, ldb, ldc, tn, M, N, K, act, ldr, dact, accumulate, kstep, vec;
            if (sscanf(line + 1, "%llu %llu %llu %lld %lld %d %d %d %d %d %d %d %llu %d %llu %d %d %d %d %d", &A, &B, &C, &aps, &bps, &lda, &ldb, &ldc,
                       &tn, &M, &N, &K, &bias, &act, &dref, &ldr, &dact, &accumulate, &kstep, &vec) != 20)
                return 2;
            const dma_plan::Args a = {(const void*)(uintptr_t)A, (const void*)(uintptr_t)B, (const void*)(uintptr_t)C, aps, bps, lda, ldb, ldc, tn, M, N, K,
                                      (const void*)(uintptr_t)bias, act, (const void*)(uintptr_t)dref, ldr, dact, accumulate};
            printf("%d\n", dma_plan::check_args(a, kstep, vec != 0));
        } else if (line[0] == 'E') {
            int bias, act, dref, dact, ok;
            if (sscanf(line + 1, "%d %d %d %d %d", &bias, &act, &dref, &dact, &ok) != 5) return 2;
            printf("%d\n", dma_plan::nt_epilogue(bias != 0, act, dref != 0, dact, ok != 0));
        } else if (line[0] != '\n' && line[0] != '#') {
            return 2;
        }
    }
    return 0;
}
