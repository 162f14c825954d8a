"""Host-side decisions of the LDS-DMA GEMM entry points (csrc/gemm_dma_plan.h) against a Python restatement of the rules that
cham_gemm_p3, cham_gemm_b16_dma and gemm_h2.hip's h2_run each spelled out before they shared the header.  The restatement below is the
reference - it was written from those three function bodies, not from the header.

The header is plain C++17: tests/gemm_dma_plan_main.cpp (its own main) is built with g++ twice - as is, and under AddressSanitizer +
UndefinedBehaviorSanitizer - and both programs run over the same table.  No GPU."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "gemm_dma_plan_main.cpp")
HEADER = os.path.join(ROOT, "chameleon_recsys_amd", "csrc", "gemm_dma_plan.h")
ERR = -22                      # -CHAM_ERR_ARG
ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
WINDOW_BYTES = 0x7FFFF000

CXX = os.environ.get("CXX", "g++")


# ---- the reference: the parent's rules -------------------------------------------------------------------------------------------
def ref_plan(M, N, K, lda, ldb, have_ws, ws_bytes, hint, kstep, min_k):
    """TN split-K plan: (kstep, min_k) = (16, 512) in cham_gemm_p3 and h2_run, (48, 1536) in cham_gemm_b16_dma."""
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    splits = 1
    if hint != 1 and have_ws:
        want = hint if hint > 1 else (1 if tiles >= 192 else (256 + tiles - 1) // tiles)
        want = min(want, (K + min_k - 1) // min_k)
        want = min(want, ws_bytes // (M * N * 4))
        if hint <= 0 and want >= 8:
            want = want // 8 * 8
        if want > 1:
            splits = want
    kchunk = (K + splits - 1) // splits
    kchunk = (kchunk + kstep - 1) // kstep * kstep
    nsplits = (K + kchunk - 1) // kchunk
    if kchunk * max(lda, ldb) * 2 >= 0xFFFFFFF0:
        return (ERR,)
    return (0, kchunk, nsplits, 1 if nsplits > 1 and nsplits % 8 == 0 else 0)


def ref_check(a, kstep, vec):
    """The rejections common to the three entry points; vec: cham_gemm_b16_dma's extra alignment rules for dref and bias."""
    if not a["A"] or not a["B"] or not a["C"] or a["M"] <= 0 or a["N"] <= 0 or a["K"] <= 0:
        return ERR
    if (a["lda"] & 7) or (a["ldb"] & 7) or (a["a_ps"] & 7) or (a["b_ps"] & 7) or (a["N"] & 3) or (a["ldc"] & 3):
        return ERR
    if vec and a["dref"] and (a["ldr"] & 3):
        return ERR
    ptrs = a["A"] | a["B"] | a["C"] | ((a["dref"] | a["bias"]) if vec else 0)
    if ptrs & 15:
        return ERR
    if a["ldc"] * 4 * 256 >= WINDOW_BYTES or a["ldr"] * 2 * 256 >= WINDOW_BYTES:
        return ERR
    tn = a["tn"]
    if a["lda"] < (a["M"] if tn else a["K"]) or a["ldb"] < (a["N"] if tn else a["K"]) or a["ldc"] < a["N"] or (a["dref"] and a["ldr"] < a["N"]):
        return ERR
    if not tn:
        if (a["K"] & 15) or a["accumulate"]:
            return ERR
        if 256 * a["lda"] * 2 >= 1 << 31 or 256 * a["ldb"] * 2 >= 1 << 31:
            return ERR
        return 0
    if (a["M"] & 255) or (a["N"] & 255) or a["bias"] or a["act"] != ACT_NONE or a["dref"]:
        return ERR
    if kstep * a["lda"] * 2 >= 1 << 31 or kstep * a["ldb"] * 2 >= 1 << 31:
        return ERR
    return 0


def ref_epilogue(bias, act, dref, dact, bias_only_ok):
    """NT epilogue: cham_gemm_p3 / h2_run (bias_only_ok) and cham_gemm_b16_dma."""
    if bias_only_ok:
        if dref and (bias or act != ACT_NONE or dact != ACT_LEAKY):
            return ERR
        if act != ACT_NONE and not (bias and act == ACT_TANH):
            return ERR
        if dref:
            return 3
        if bias:
            return 2 if act == ACT_TANH else 5
        return 0
    if dref:
        return ERR if (bias or act != ACT_NONE or dact != ACT_LEAKY) else 3
    if bias:
        return 2 if act == ACT_TANH else ERR
    return ERR if act != ACT_NONE else 0


# ---- the table -------------------------------------------------------------------------------------------------------------------
SHAPES = [(256, 256), (256, 512), (512, 256), (512, 512), (3584, 4096)]          # the last: 224 tiles, past the 192-tile threshold
KS = [1, 16, 70, 511, 512, 513, 1100, 1536, 1537, 248064]
HINTS = [1, 0, 3, 8, 14, 32]
CONSTANTS = [(16, 512), (48, 1536)]


def plan_cases():
    cases = []
    for (M, N), K, hint, (kstep, min_k) in itertools.product(SHAPES, KS, HINTS, CONSTANTS):
        slab = M * N * 4
        tiles = ((M + 255) // 256) * ((N + 255) // 256)
        want = hint if hint > 1 else (1 if tiles >= 192 else (256 + tiles - 1) // tiles)
        want = max(1, min(want, (K + min_k - 1) // min_k))                      # what the plan asks of the workspace
        for have_ws, ws_bytes in [(0, 0), (1, slab), (1, want * slab), (1, want * slab - 1)]:
            cases.append((M, N, K, M, N, have_ws, ws_bytes, hint, kstep, min_k))
    # the descriptor range: kchunk * max(lda, ldb) * 2 >= 0xFFFFFFF0 is rejected, one element less is taken
    for (kstep, min_k), K, hint in itertools.product(CONSTANTS, [248064, 1100], [1, 8]):
        r = ref_plan(256, 256, K, 256, 256, 1, 1 << 40, hint, kstep, min_k)
        edge = -(-0xFFFFFFF0 // (2 * r[1]))                                      # smallest leading dimension that is rejected
        for ld in (edge - 1, edge):
            cases.append((256, 256, K, ld, 256, 1, 1 << 40, hint, kstep, min_k))
            cases.append((256, 256, K, 256, ld, 1, 1 << 40, hint, kstep, min_k))
    return cases


BASE = dict(A=0x10000, B=0x20000, C=0x30000, a_ps=1 << 20, b_ps=1 << 20, lda=512, ldb=512, ldc=512, tn=0, M=512, N=256, K=512,
            bias=0, act=ACT_NONE, dref=0, ldr=0, dact=ACT_NONE, accumulate=0)
FIELDS = ["A", "B", "C", "a_ps", "b_ps", "lda", "ldb", "ldc", "tn", "M", "N", "K", "bias", "act", "dref", "ldr", "dact", "accumulate"]
NT_DREF = dict(dref=0x40000, ldr=256, dact=ACT_LEAKY)
# (name, changes to BASE, kstep, vector_epilogue, expected)
CHECK_CASES = [
    ("nt ok", {}, 16, 0, 0), ("nt ok bf16", dict(a_ps=0, b_ps=0), 48, 1, 0), ("nt dgrad ok", NT_DREF, 16, 0, 0),
    ("tn ok", dict(tn=1, M=512, N=256, K=70, lda=512, ldb=256, accumulate=1), 16, 0, 0),
    ("null A", dict(A=0), 16, 0, ERR), ("null B", dict(B=0), 16, 0, ERR), ("null C", dict(C=0), 16, 0, ERR),
    ("M 0", dict(M=0), 16, 0, ERR), ("N -4", dict(N=-4), 16, 0, ERR), ("K 0", dict(K=0), 16, 0, ERR),
    ("lda % 8", dict(lda=516), 16, 0, ERR), ("ldb % 8", dict(ldb=516), 16, 0, ERR),
    ("a plane stride % 8", dict(a_ps=(1 << 20) + 4), 16, 0, ERR), ("b plane stride % 8", dict(b_ps=(1 << 20) + 4), 16, 0, ERR),
    ("N % 4", dict(N=254), 16, 0, ERR), ("ldc % 4", dict(ldc=514), 16, 0, ERR),
    ("A alignment", dict(A=0x10008), 16, 0, ERR), ("B alignment", dict(B=0x20004), 16, 0, ERR), ("C alignment", dict(C=0x30002), 16, 0, ERR),
    ("C window", dict(ldc=WINDOW_BYTES // 1024 + 4), 16, 0, ERR), ("C window, one under", dict(ldc=WINDOW_BYTES // 1024 - 4), 16, 0, 0),
    ("dref window", dict(NT_DREF, ldr=WINDOW_BYTES // 512 + 1), 16, 0, ERR),
    ("lda < K", dict(lda=504), 16, 0, ERR), ("ldb < K", dict(ldb=504), 16, 0, ERR), ("ldc < N", dict(ldc=252), 16, 0, ERR),
    ("ldr < N", dict(NT_DREF, ldr=252), 16, 0, ERR),
    ("tn lda < M", dict(tn=1, K=70, lda=504, ldb=256), 16, 0, ERR), ("tn ldb < N", dict(tn=1, K=70, lda=512, ldb=248), 16, 0, ERR),
    ("nt K % 16", dict(K=504), 16, 0, ERR), ("nt accumulate", dict(accumulate=1), 16, 0, ERR),
    ("nt lda slab", dict(lda=1 << 22), 16, 0, ERR), ("nt ldb slab", dict(ldb=1 << 22), 16, 0, ERR),
    ("nt lda slab, one under", dict(lda=(1 << 22) - 8), 16, 0, 0),
    ("tn M % 256", dict(tn=1, M=384, K=70), 16, 0, ERR), ("tn N % 256", dict(tn=1, N=128, K=70), 16, 0, ERR),
    ("tn bias", dict(tn=1, K=70, bias=0x50000), 16, 0, ERR), ("tn act", dict(tn=1, K=70, act=ACT_TANH), 16, 0, ERR),
    ("tn dref", dict(NT_DREF, tn=1, K=70), 16, 0, ERR),
    ("tn lda stage, 48 k", dict(tn=1, K=70, lda=(1 << 31) // 96 + 8 - ((1 << 31) // 96) % 8), 48, 0, ERR),
    ("tn lda stage, 16 k takes it", dict(tn=1, K=70, lda=(1 << 31) // 96 + 8 - ((1 << 31) // 96) % 8), 16, 0, 0),
    ("tn ldb stage, 16 k", dict(tn=1, K=70, ldb=1 << 26), 16, 0, ERR),
    ("bf16: ldr % 4", dict(NT_DREF, ldr=258), 48, 1, ERR), ("fp32 out: ldr % 4 taken", dict(NT_DREF, ldr=258), 16, 0, 0),
    ("bf16: dref alignment", dict(NT_DREF, dref=0x40008), 48, 1, ERR), ("fp32 out: dref alignment taken", dict(NT_DREF, dref=0x40008), 16, 0, 0),
    ("bf16: bias alignment", dict(bias=0x50004, act=ACT_TANH), 48, 1, ERR), ("fp32 out: bias alignment taken", dict(bias=0x50004, act=ACT_TANH), 16, 0, 0),
]
EPI_CASES = list(itertools.product([0, 1], [ACT_NONE, ACT_LEAKY, ACT_TANH], [0, 1], [ACT_NONE, ACT_LEAKY, ACT_TANH], [0, 1]))


def table():
    lines = ["P " + " ".join(str(v) for v in c) for c in plan_cases()]
    for _, change, kstep, vec, _ in CHECK_CASES:
        a = dict(BASE, **change)
        lines.append("C " + " ".join(str(a[f]) for f in FIELDS) + " %d %d" % (kstep, vec))
    lines += ["E %d %d %d %d %d" % c for c in EPI_CASES]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def results(request, tmp_path_factory):
    """Output lines of the stand-alone program over the whole table."""
    exe = str(tmp_path_factory.mktemp("gemm_dma_plan") / ("plan_" + request.param))
    flags = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
    flags += ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([CXX] + flags + [MAIN, "-o", exe])
    out = subprocess.run([exe], input=table().encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert out.stderr == b"", out.stderr.decode()[-2000:]
    return [tuple(int(x) for x in ln.split()) for ln in out.stdout.decode().splitlines()]


def test_header_needs_no_hip():
    includes = [ln for ln in open(HEADER).read().splitlines() if ln.lstrip().startswith("#include")]
    assert includes and all("<c" in ln for ln in includes), includes          # standard C++ headers only


def test_split_plan(results):
    cases = plan_cases()
    got = results[:len(cases)]
    assert len(got) == len(cases)
    rejected = rounded = as_given = short = 0
    for c, g in zip(cases, got):
        M, N, K, lda, ldb, have_ws, ws_bytes, hint, kstep, min_k = c
        want = ref_plan(*c)
        assert g == want, (c, g, want)
        if g[0] != 0:
            rejected += 1
            continue
        _, kchunk, splits, xcd = g
        assert kchunk % kstep == 0 and kchunk > 0 and (splits - 1) * kchunk < K <= splits * kchunk, (c, g)
        assert xcd == (1 if splits > 1 and splits % 8 == 0 else 0), (c, g)
        assert kchunk * max(lda, ldb) * 2 < 0xFFFFFFF0, (c, g)
        if hint == 1 or not have_ws:
            assert splits == 1, (c, g)
        if splits > 1:
            assert splits * M * N * 4 <= ws_bytes and splits <= (K + min_k - 1) // min_k, (c, g)
    assert rejected == 16                                            # the descriptor-range cases: one of each pair
    # the want / 8 * 8 rounding belongs to the automatic plan alone; what it rounds is the count that kchunk is cut from
    def cut(K, want, kstep):
        kchunk = -(-(-(-K // want)) // kstep) * kstep
        n = -(-K // kchunk)
        return (0, kchunk, n, 1 if n > 1 and n % 8 == 0 else 0)
    slab = 256 * 256 * 4
    # one tile, K = 248064, 1536 k per split: at most 162 splits - 160 for the automatic plan, an explicit 14 or 32 as given
    for hint, asked, want in [(0, 162, 160), (14, 14, 14), (32, 32, 32)]:
        g = got[cases.index((256, 256, 248064, 256, 256, 1, asked * slab, hint, 48, 1536))]
        assert g == cut(248064, want, 48), (hint, g)
    assert cut(248064, 160, 48) != cut(248064, 162, 48)
    # one byte short of the 14 slabs an explicit count asks for: 13, not 8 ...
    g = got[cases.index((256, 256, 248064, 256, 256, 1, 14 * slab - 1, 14, 16, 512))]
    assert g == cut(248064, 13, 16) != cut(248064, 8, 16), g
    # ... where the automatic plan, one byte short of its 256 slabs, rounds 255 down to 248
    g = got[cases.index((256, 256, 248064, 256, 256, 1, 256 * slab - 1, 0, 16, 512))]
    assert g == cut(248064, 248, 16) != cut(248064, 255, 16), g


def test_common_rejections(results):
    n0 = len(plan_cases())
    got = results[n0:n0 + len(CHECK_CASES)]
    assert len(got) == len(CHECK_CASES)
    for (name, change, kstep, vec, expect), g in zip(CHECK_CASES, got):
        a = dict(BASE, **change)
        assert ref_check(a, kstep, vec) == expect, name              # the table states what the parent did
        assert g == (expect,), (name, g)


def test_nt_epilogue_rules(results):
    got = results[len(plan_cases()) + len(CHECK_CASES):]
    assert len(got) == len(EPI_CASES)
    for c, g in zip(EPI_CASES, got):
        assert g == (ref_epilogue(*c),), (c, g)
    assert sorted({g[0] for g in got}) == [ERR, 0, 2, 3, 5]
