"""Host-side decisions of the register-staged GEMM families (csrc/gemm_tile_plan.h) against a Python restatement of the rules that
gemm_shared.h's gemm_plan, cham_gemm_b16's prologue, the three *_launch_cfg ladders (gemm.hip, gemm_x3.hip, gemm_b16.hip) and the four
*_by_shape tile choosers each spelled out before they shared the header.  The restatement below is the reference - it was written from
those function bodies, not from the header.

The header is plain C++17: tests/gemm_tile_plan_main.cpp (its own main) is built with g++ twice - as is, and under AddressSanitizer +
UndefinedBehaviorSanitizer - and both programs run over the same table.  No GPU."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = os.path.join(ROOT, "tests", "gemm_tile_plan_main.cpp")
HEADER = os.path.join(ROOT, "chameleon_recsys_amd", "csrc", "gemm_tile_plan.h")
ERR = -22                      # -CHAM_ERR_ARG
ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
WINDOW_BYTES = 0x7FFFF000
CXX = os.environ.get("CXX", "g++")
FIELDS = ["A", "lda", "tA", "B", "ldb", "tB", "C", "ldc", "M", "N", "K", "bias", "act", "dref", "ldr", "dact", "rs", "ldrs", "rs_div",
          "accumulate", "ws", "ws_bytes", "hint"]


def sz(x):
    """(size_t)x of a C int"""
    return x % (1 << 64)


# ---- the reference: the parent's rules -------------------------------------------------------------------------------------------
def ref_gemm_plan(a):
    """gemm_shared.h gemm_plan: (rc,) or (0, kchunk, splits)."""
    A, B, C, M, N, K, lda, ldb, ldc, tA, tB = (a[k] for k in ("A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "tA", "tB"))
    bias, dref, ldr, rs, ldrs, rs_div = (a[k] for k in ("bias", "dref", "ldr", "rs", "ldrs", "rs_div"))
    if not A or not B or not C or M <= 0 or N <= 0 or K < 0:
        return (ERR,)
    if (lda & 3) or (ldb & 3):
        return (ERR,)
    if not tA and (K & 3):
        return (ERR,)
    if tA and (M & 3):
        return (ERR,)
    if not tB and (N & 3):
        return (ERR,)
    if tB and (K & 3):
        return (ERR,)
    if rs and ((ldrs & 3) or rs_div <= 0):
        return (ERR,)
    if lda < (M if tA else K) or ldb < (K if tB else N) or ldc < N or (dref and ldr < N) or (rs and ldrs < (M if tA else K)):
        return (ERR,)
    if any(sz(sz(ld) * 4 * 256) >= WINDOW_BYTES for ld in (lda, ldb, ldc, ldr)):
        return (ERR,)
    if rs and sz(((K if tA else M) // (rs_div if rs_div > 0 else 1) + 1) * ldrs * 4) >= WINDOW_BYTES:
        return (ERR,)
    splits = 1
    reduce_ok = (N & 3) == 0 and (not bias or (bias & 15) == 0)
    if a["hint"] != 1 and a["ws"] and reduce_ok and tA and not tB:
        bm = (256 if M * N >= (1 << 20) else 128) if N > 64 else 256
        bn = 128 if N > 64 else (64 if N > 32 else 32)
        tiles = ((M + bm - 1) // bm) * ((N + bn - 1) // bn)
        want = a["hint"] if a["hint"] > 1 else (1 if tiles >= 384 else (512 + tiles - 1) // tiles)
        want = min(want, (K + 255) // 256)
        want = min(want, a["ws_bytes"] // (M * N * 4))
        if want > 1:
            splits = want
    kchunk = (K + splits - 1) // splits
    kchunk = (kchunk + 63) // 64 * 64
    if kchunk == 0:
        kchunk = 64
    return (0, kchunk, max(1, (K + kchunk - 1) // kchunk))


def ref_b16_prologue(a):
    """cham_gemm_b16 up to the tile choice: (rc,) or (0, kchunk, splits)."""
    A, B, C, M, N, K, lda, ldb, ldc, tA, tB = (a[k] for k in ("A", "B", "C", "M", "N", "K", "lda", "ldb", "ldc", "tA", "tB"))
    bias, dref, ldr = a["bias"], a["dref"], a["ldr"]
    if not A or not B or not C or M <= 0 or N <= 0 or K <= 0:
        return (ERR,)
    if (lda & 7) or (ldb & 7) or (N & 3) or (ldc & 3) or (dref and (ldr & 3)):
        return (ERR,)
    if (A | B | C | dref | bias) & 15:
        return (ERR,)
    nt, tn = (not tA and tB), (tA and not tB)
    if not nt and not tn:
        return (ERR,)
    if nt and (K & 7):
        return (ERR,)
    if tn and ((M & 7) or (N & 7)):
        return (ERR,)
    if lda < (M if tn else K) or ldb < (N if tn else K) or ldc < N or (dref and ldr < N):
        return (ERR,)
    if (sz(sz(lda) * 2 * 256) >= WINDOW_BYTES or sz(sz(ldb) * 2 * 256) >= WINDOW_BYTES or sz(sz(ldc) * 4 * 256) >= WINDOW_BYTES or
            sz(sz(ldr) * 2 * 256) >= WINDOW_BYTES):
        return (ERR,)
    splits = 1
    if tn and a["hint"] != 1 and a["ws"]:
        bn = 128 if N > 64 else (64 if N > 32 else 32)
        tiles = ((M + 255) // 256) * ((N + bn - 1) // bn)
        want = a["hint"] if a["hint"] > 1 else (1 if tiles >= 384 else (512 + tiles - 1) // tiles)
        want = min(want, (K + 511) // 512)
        want = min(want, a["ws_bytes"] // (M * N * 4))
        if want >= 8:
            want = want // 8 * 8
        if want > 1:
            splits = want
    kchunk = (K + splits - 1) // splits
    kchunk = (kchunk + 31) // 32 * 32
    return (0, kchunk, (K + kchunk - 1) // kchunk)


def ref_launch_cfg(ak, bkc, bias, act, dref, dact, accumulate, split):
    """launch_cfg (gemm.hip) = x3_launch_cfg (gemm_x3.hip): the EPI it launches, or the error."""
    NN, NT, TN = ak and not bkc, ak and bkc, not ak and not bkc
    if split:
        return 6 if TN else ERR
    if dref:
        if bias or act != ACT_NONE:
            return ERR
        if NT:
            if dact == ACT_LEAKY:
                return 3
            if dact == ACT_TANH:
                return 4
        return ERR
    if bias or act != ACT_NONE:
        if not bias or accumulate:
            return ERR
        if NN:
            return 1 if act == ACT_LEAKY else (2 if act == ACT_TANH else 5)
        return ERR
    return 0


F32_INSTANCES = {(1, 0): {0, 1, 2, 5}, (1, 1): {0, 3, 4}, (0, 0): {0, 6}}          # the EPIs launch_cfg names per (AK, BKC)


def ref_rsi(epi, ak, bkc):
    return (epi == 1 and ak and not bkc) or (epi in (6, 0) and not ak and not bkc)


def ref_b16_launch_cfg(tn, bias, act, dref, dact, accumulate, split, out_f32):
    """b16_launch_cfg: (EPI, OUTF32 of the instance) or (ERR,)."""
    if tn:
        if bias or act != ACT_NONE or dref or not out_f32:
            return (ERR,)
        return (6, 1) if split else (0, 1)
    if split or accumulate:
        return (ERR,)
    if dref:
        if bias or act != ACT_NONE or out_f32 or dact != ACT_LEAKY:
            return (ERR,)
        return (3, 0)
    if bias:
        if out_f32:
            return (ERR,)
        if act == ACT_LEAKY:
            return (1, 0)
        if act == ACT_TANH:
            return (2, 0)
        return (ERR,)
    if act != ACT_NONE:
        return (ERR,)
    return (0, 1 if out_f32 else 0)


B16_REACHED = {1: {(6, 1), (0, 1)}, 0: {(3, 0), (1, 0), (2, 0), (0, 1), (0, 0)}}       # (EPI, OUTF32) b16_launch_cfg launches for TN / NT
B16_INSTANCES = B16_REACHED[0] | B16_REACHED[1]          # ... and names, for BOTH layouts: its layout test is a run-time `if`


def grid(M, N, bm, bn, splits):
    return ((M + bm - 1) // bm) * ((N + bn - 1) // bn) * splits


def ref_by_shape(fam, M, N, K, splits, ak, bkc, forced):
    """The launch counter (relative to the family's first tile counter) each *_by_shape bumps = the instance it runs:
    0 128x128, 1 256x128, 2 256x256 (f32) / 256x128 on 4 waves (b16), 3 256x64, 4 256x32.  b16: (instance, counter)."""
    if fam == 0:          # launch_by_shape
        if N > 64:
            v = 2 if M * N >= (1 << 20) else 0
            if v == 2 and (not ak or bkc) and K >= 512 and M >= 1024 and N >= 512:
                v = 4
            if v == 4 and grid(M, N, 256, 256, splits) < 256:
                v = 2
            if v == 2 and grid(M, N, 256, 128, splits) < 256:
                v = 0
            if forced >= 0:
                v = forced
            return (1,) if v == 2 else ((2,) if v == 4 else (0,))
        return (3,) if N > 32 else (4,)
    if fam == 1:          # launch_by_shape_bf16
        if N > 64:
            big = M * N >= (1 << 20) and grid(M, N, 256, 128, splits) >= 256
            if forced >= 0:
                big = forced >= 2
            return (1,) if big else (0,)
        return (3,) if N > 32 else (4,)
    if fam == 2:          # x3_by_shape
        v = 2 if (M * N >= (1 << 20) and grid(M, N, 256, 128, splits) >= 256) else 0
        if forced >= 0:
            v = forced
        return (1,) if v == 2 else (0,)
    if N > 64:            # b16_by_shape
        v = 1 if grid(M, N, 256, 128, splits) >= 256 else 0
        if v == 1 and not ak and splits > 1:
            v = 2
        if forced >= 0:
            v = forced
        return (v if v in (1, 2) else 0, v if v < 3 else 2)
    return (3, 3) if N > 32 else (4, 4)


# ---- the table -------------------------------------------------------------------------------------------------------------------
BASE = dict(A=0x10000, lda=512, tA=0, B=0x20000, ldb=256, tB=0, C=0x30000, ldc=256, M=512, N=256, K=512, bias=0, act=0, dref=0, ldr=0, dact=0,
            rs=0, ldrs=0, rs_div=1, accumulate=0, ws=0, ws_bytes=0, hint=1)
NT = dict(tB=1, ldb=512)
TN = dict(tA=1, lda=512, ldb=256)
DREF = dict(dref=0x40000, ldr=256, dact=ACT_LEAKY)
RS = dict(rs=0x60000, ldrs=512, rs_div=4)
LD_WIN4 = WINDOW_BYTES // 1024          # first leading dimension whose 256-row slab of 4-byte elements leaves the window (a multiple of 4)
LD_WIN2 = WINDOW_BYTES // 512           # ... of 2-byte elements (a multiple of 8)
RS_WIN = -(-WINDOW_BYTES // (513 * 4))  # M = 512, rs_div = 1: 513 scale rows
RS_WIN += -RS_WIN % 4
# (name, changes to BASE, expected rc): one thing wrong at a time, and its nearest accepted neighbour
F32_CHECKS = [
    ("nn ok", {}, 0), ("nt ok", NT, 0), ("tn ok", TN, 0), ("tt passes the checks (the dispatch rejects it)", dict(tA=1, tB=1, ldb=512), 0),
    ("K 0 ok", dict(K=0), 0), ("dgrad ok", dict(NT, **DREF), 0), ("row scale ok", RS, 0), ("tn row scale ok", dict(TN, **RS), 0),
    ("null A", dict(A=0), ERR), ("null B", dict(B=0), ERR), ("null C", dict(C=0), ERR), ("M 0", dict(M=0), ERR), ("N -4", dict(N=-4), ERR),
    ("K -4", dict(K=-4), ERR), ("lda % 4", dict(lda=514), ERR), ("ldb % 4", dict(ldb=258), ERR),
    ("nn K % 4", dict(K=510), ERR), ("tn M % 4", dict(TN, M=510), ERR), ("tn K % 4 taken", dict(TN, K=510), 0),
    ("nn N % 4", dict(N=254), ERR), ("nt N % 4 taken", dict(NT, N=254), 0), ("nt K % 4", dict(NT, K=510), ERR),
    ("ldrs % 4", dict(RS, ldrs=514), ERR), ("rs_div 0", dict(RS, rs_div=0), ERR), ("rs_div 0 without a row scale", dict(rs_div=0), 0),
    ("lda < K", dict(lda=508), ERR), ("tn lda < M", dict(TN, lda=508), ERR), ("ldb < N", dict(ldb=252), ERR), ("nt ldb < K", dict(NT, ldb=508), ERR),
    ("ldc < N", dict(ldc=252), ERR), ("ldr < N", dict(NT, **dict(DREF, ldr=252)), ERR), ("ldr < N without dref", dict(ldr=252), 0),
    ("ldrs < K", dict(RS, ldrs=508), ERR), ("tn ldrs < M", dict(TN, **dict(RS, ldrs=508)), ERR),
    ("lda window", dict(lda=LD_WIN4), ERR), ("lda window, one under", dict(lda=LD_WIN4 - 4), 0),
    ("ldb window", dict(ldb=LD_WIN4), ERR), ("ldb window, one under", dict(ldb=LD_WIN4 - 4), 0),
    ("ldc window", dict(ldc=LD_WIN4), ERR), ("ldc window, one under", dict(ldc=LD_WIN4 - 4), 0),
    ("ldr window", dict(NT, **dict(DREF, ldr=LD_WIN4)), ERR), ("ldr window without dref", dict(ldr=LD_WIN4), ERR),
    ("negative ldr without dref", dict(ldr=-4), ERR),
    ("row scale window", dict(RS, rs_div=1, ldrs=RS_WIN), ERR), ("row scale window, one under", dict(RS, rs_div=1, ldrs=RS_WIN - 4), 0),
]
B16_BASE = dict(BASE, **NT)
B16_TN = dict(TN, tB=0, M=512, N=256, K=500)
B16_CHECKS = [
    ("nt ok", {}, 0), ("tn ok", B16_TN, 0), ("dgrad ok", DREF, 0), ("bias ok", dict(bias=0x50000, act=ACT_TANH), 0),
    ("null A", dict(A=0), ERR), ("null B", dict(B=0), ERR), ("null C", dict(C=0), ERR), ("M 0", dict(M=0), ERR), ("N 0", dict(N=0), ERR),
    ("K 0", dict(K=0), ERR), ("lda % 8", dict(lda=516), ERR), ("ldb % 8", dict(ldb=516), ERR), ("N % 4", dict(N=254), ERR),
    ("ldc % 4", dict(ldc=258), ERR), ("ldr % 4", dict(DREF, ldr=258), ERR), ("ldr % 4 without dref", dict(ldr=258), 0),
    ("A alignment", dict(A=0x10008), ERR), ("B alignment", dict(B=0x20004), ERR), ("C alignment", dict(C=0x30002), ERR),
    ("dref alignment", dict(DREF, dref=0x40008), ERR), ("bias alignment", dict(bias=0x50004), ERR),
    ("nn", dict(tB=0, ldb=256), ERR), ("tt", dict(tA=1), ERR),
    ("nt K % 8", dict(K=508), ERR), ("tn M % 8", dict(B16_TN, M=508), ERR), ("tn N % 8", dict(B16_TN, N=252), ERR), ("nt N % 8 taken", dict(N=252), 0),
    ("lda < K", dict(lda=504), ERR), ("tn lda < M", dict(B16_TN, lda=504), ERR), ("ldb < K", dict(ldb=504), ERR), ("tn ldb < N", dict(B16_TN, ldb=248), ERR),
    ("ldc < N", dict(ldc=252), ERR), ("ldr < N", dict(DREF, ldr=252), ERR),
    ("lda window", dict(lda=LD_WIN2), ERR), ("lda window, one under", dict(lda=LD_WIN2 - 8), 0),
    ("ldb window", dict(ldb=LD_WIN2), ERR), ("ldb window, one under", dict(ldb=LD_WIN2 - 8), 0),
    ("ldc window", dict(ldc=LD_WIN4), ERR), ("ldc window, one under", dict(ldc=LD_WIN4 - 4), 0),
    ("ldr window", dict(DREF, ldr=LD_WIN2), ERR), ("ldr window without dref", dict(ldr=LD_WIN2), ERR), ("ldr window, one under", dict(DREF, ldr=LD_WIN2 - 8), 0),
]

# split plans: TN calls.  Tile estimates 1 (64 x 32, 128 x 64), 2 or 1 (256 x 128: 128- or 256-row tiles), 32 (1024^2), >= 384 (no automatic split)
SPLIT_SHAPES = [(64, 32), (128, 64), (256, 128), (1024, 128), (1024, 1024), (6144, 2048)]
SPLIT_KS = [0, 16, 31, 32, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4096, 8192, 16384, 248064]
SPLIT_HINTS = [1, 0, 5, 7, 8, 9, 32, 300]


def split_cases():
    out = []
    for (M, N), K, hint in itertools.product(SPLIT_SHAPES, SPLIT_KS, SPLIT_HINTS):
        slab = M * N * 4
        for ws, nbytes in [(0, 1 << 40), (0x70000, 0), (0x70000, slab), (0x70000, 3 * slab), (0x70000, 12 * slab - 1), (0x70000, 12 * slab), (0x70000, 1 << 40)]:
            out.append(dict(BASE, **dict(TN, M=M, N=N, K=K, lda=M, ldb=N, ldc=N, ws=ws, ws_bytes=nbytes, hint=hint)))
    # what keeps a call unsplit in the fp32 families: a misaligned bias (the reduction reads it 16 bytes at a time), any layout but TN
    for change in (dict(bias=0x50004), dict(bias=0x50010), dict(tA=0, lda=8192, M=256), dict(tA=0, tB=1, lda=8192, ldb=8192)):
        out.append(dict(BASE, **dict(dict(TN, M=256, N=128, K=8192, lda=256, ldb=128, ldc=128, ws=0x70000, ws_bytes=1 << 40, hint=0), **change)))
    return out


def line(tag, a):
    return tag + " " + " ".join(str(a[f]) for f in FIELDS)


E_CASES = [c for c in itertools.product([0, 1], [0, 1], [0, 1], [0, 1, 2, 3], [0, 1], [0, 1, 2, 3], [0, 1], [0, 1]) if (c[0], c[1]) != (0, 1)]
G_CASES = list(itertools.product([0, 1], [0, 1], [0, 1, 2, 3], [0, 1], [0, 1, 2, 3], [0, 1], [0, 1], [0, 1]))
# both sides of: M N at 2^20 (2044 | 2048 x 512, 1020 | 1024 x 1024), grid(256, 128) at 256 (7936 | 8192 x 1024, 1024^2 with 7 | 8 splits),
# grid(256, 256) at 256 (16128 | 16384 x 1024, 1024^2 with 15 | 16 splits), the 256x256 conditions K 512, M 1024, N 512, N at 32 and 64
I_CASES = list(itertools.product(range(-1, 8), [0, 1], [0, 1], [0, 1]))
T_CASES = list(itertools.product([0, 1, 2, 3], [512, 1020, 1024, 2044, 2048, 7936, 8192, 16128, 16384, 69768], [16, 32, 33, 64, 65, 128, 508, 512, 1024],
                                 [256, 508, 512], [1, 7, 8, 15, 16], [(1, 0), (1, 1), (0, 0)], [-1, 0, 1, 2, 3, 4, 5]))


def table():
    lines = [line("F", dict(BASE, **ch)) for _, ch, _ in F32_CHECKS]
    lines += [line("B", dict(B16_BASE, **ch)) for _, ch, _ in B16_CHECKS]
    for a in split_cases():
        lines += [line("F", a), line("B", a)]
    lines += ["E %d %d %d %d %d %d %d %d" % c for c in E_CASES]
    lines += ["G %d %d %d %d %d %d %d %d" % c for c in G_CASES]
    lines += ["I %d %d %d %d" % c for c in I_CASES]
    lines += ["T %d %d %d %d %d %d %d %d" % (f, M, N, K, s, ak, bkc, forced) for f, M, N, K, s, (ak, bkc), forced in T_CASES]
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def results(request, tmp_path_factory):
    """Output lines of the stand-alone program over the whole table, cut into the table's sections."""
    exe = str(tmp_path_factory.mktemp("gemm_tile_plan") / ("plan_" + request.param))
    flags = ["-std=c++17", "-Wall", "-Wextra", "-Werror"]
    flags += ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param == "sanitized" else ["-O2"]
    subprocess.check_call([CXX] + flags + [MAIN, "-o", exe])
    out = subprocess.run([exe], input=table().encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert out.stderr == b"", out.stderr.decode()[-2000:]
    rows = [tuple(int(x) for x in ln.split()) for ln in out.stdout.decode().splitlines()]
    sections, at = {}, 0
    for name, n in (("f32_checks", len(F32_CHECKS)), ("b16_checks", len(B16_CHECKS)), ("splits", 2 * len(split_cases())), ("E", len(E_CASES)),
                    ("G", len(G_CASES)), ("I", len(I_CASES)), ("T", len(T_CASES))):
        sections[name] = rows[at:at + n]
        at += n
    assert at == len(rows)
    return sections


def test_header_needs_no_hip():
    includes = [ln for ln in open(HEADER).read().splitlines() if ln.lstrip().startswith("#include")]
    assert includes and all("<c" in ln for ln in includes), includes          # standard C++ headers only


def test_f32_argument_checks(results):
    for (name, change, expect), g in zip(F32_CHECKS, results["f32_checks"]):
        want = ref_gemm_plan(dict(BASE, **change))
        assert want[0] == expect, name                                        # the table states what the parent did
        assert g == want, (name, g, want)


def test_b16_argument_checks(results):
    for (name, change, expect), g in zip(B16_CHECKS, results["b16_checks"]):
        want = ref_b16_prologue(dict(B16_BASE, **change))
        assert want[0] == expect, name
        assert g == want, (name, g, want)


def test_split_plans(results):
    cases = split_cases()
    got = results["splits"]
    seen = set()
    for a, gf, gb in zip(cases, got[0::2], got[1::2]):
        wf, wb = ref_gemm_plan(a), ref_b16_prologue(a)
        assert gf == wf and gb == wb, (a, gf, wf, gb, wb)
        M, N, K, hint = a["M"], a["N"], a["K"], a["hint"]
        for fam, g, min_k, mult in (("f32", gf, 256, 64), ("b16", gb, 512, 32)):
            if g[0] != 0:
                # only cham_gemm_b16 rejects any of these: K = 0, a misaligned bias, NN, an NT call whose ldb does not span K
                assert fam == "b16" and (K == 0 or a["bias"] & 15 or a["tA"] == a["tB"] or a["ldb"] < K), (a, g)
                continue
            _, kchunk, splits = g
            assert kchunk > 0 and kchunk % mult == 0 and splits >= 1 and (splits - 1) * kchunk < max(K, 1) <= splits * kchunk, (a, g)
            if hint == 1 or not a["ws"]:
                assert splits == 1, (a, g)
            if splits > 1:
                assert splits * M * N * 4 <= a["ws_bytes"] and splits <= (K + min_k - 1) // min_k, (a, g)
                if hint > 1:
                    assert splits <= hint
                ws_bound = a["ws_bytes"] // (M * N * 4)
                seen.add((fam, "workspace binds" if splits == ws_bound or (fam == "b16" and splits == ws_bound // 8 * 8) else
                          "k binds" if splits in ((K + min_k - 1) // min_k, (K + min_k - 1) // min_k // 8 * 8) else "as asked"))
            if K == 0:
                seen.add((fam, "K 0"))
            elif K < mult:
                seen.add((fam, "K below one chunk"))
                assert (kchunk, splits) == (mult, 1)
    assert seen >= {("f32", "workspace binds"), ("f32", "k binds"), ("f32", "as asked"), ("f32", "K 0"), ("f32", "K below one chunk"),
                    ("b16", "workspace binds"), ("b16", "k binds"), ("b16", "as asked"), ("b16", "K below one chunk")}, seen
    by = {(a["M"], a["N"], a["K"], a["hint"], a["ws_bytes"], a["bias"], a["tA"], a["tB"]): (gf, gb) for a, gf, gb in zip(cases, got[0::2], got[1::2])}
    big = 1 << 40
    assert by[(256, 128, 0, 0, big, 0, 1, 0)][0] == (0, 64, 1)                             # K = 0: one empty chunk of 64 (fp32 families only)
    assert by[(256, 128, 0, 0, big, 0, 1, 0)][1] == (ERR,)
    assert by[(256, 128, 8192, 32, big, 0, 1, 0)] == ((0, 256, 32), (0, 512, 16))          # 256 | 512 reduction steps per split
    assert by[(256, 128, 8192, 5, big, 0, 1, 0)] == ((0, 1664, 5), (0, 1664, 5))
    assert by[(1024, 128, 16384, 32, big, 0, 1, 0)] == ((0, 512, 32), (0, 512, 32))
    assert by[(1024, 128, 248064, 300, big, 0, 1, 0)] == ((0, 832, 299), (0, 864, 288))    # b16: 300 -> 296 = whole groups of 8 -> chunks of 864
    assert by[(1024, 128, 248064, 9, big, 0, 1, 0)][1][2] == 8 and by[(1024, 128, 248064, 7, big, 0, 1, 0)][1][2] == 7
    assert by[(1024, 128, 248064, 32, 12 * 1024 * 128 * 4 - 1, 0, 1, 0)] == ((0, 22592, 11), (0, 31008, 8))      # one byte short of 12 slabs
    assert by[(256, 128, 8192, 0, big, 0x50004, 1, 0)][0] == (0, 8192, 1)                  # misaligned bias: unsplit
    assert by[(256, 128, 8192, 0, big, 0x50010, 1, 0)][0][2] > 1
    assert by[(256, 128, 8192, 0, big, 0, 0, 0)][0] == (0, 8192, 1) and by[(256, 128, 8192, 0, big, 0, 0, 1)][0] == (0, 8192, 1)


def test_f32_epilogue_ladder(results):
    got = results["E"]
    assert len(got) == len(E_CASES)
    for c, g in zip(E_CASES, got):
        ak, bkc = c[0], c[1]
        e = ref_launch_cfg(*c)
        assert g[0] == e, (c, g)
        if e >= 0:
            assert e in F32_INSTANCES[(ak, bkc)] and g[1] == 1, (c, g)             # the ladder only ever names an instance that exists
            assert g[2] == int(ref_rsi(e, ak, bkc)), (c, g)
    assert {(c[0], c[1], g[0]) for c, g in zip(E_CASES, got) if g[0] >= 0} == {(ak, bkc, e) for (ak, bkc), es in F32_INSTANCES.items() for e in es}


def test_b16_epilogue_ladder(results):
    got = results["G"]
    assert len(got) == len(G_CASES)
    for c, g in zip(G_CASES, got):
        want = ref_b16_launch_cfg(*c)
        assert g[0] == want[0], (c, g)
        if want[0] >= 0:
            assert (g[0], g[1]) == want and want in B16_REACHED[c[0]] and g[2] == 1, (c, g)
    assert {(c[0], g[0], g[1]) for c, g in zip(G_CASES, got) if g[0] >= 0} == {(tn, e, f) for tn, es in B16_REACHED.items() for e, f in es}


def test_kernel_instances(results):
    """The instance predicates over every (EPI, layout, output type): exactly the kernels the three ladders named."""
    got = results["I"]
    assert len(got) == len(I_CASES)
    for (epi, ak, bkc, f32), g in zip(I_CASES, got):
        want_f32 = (ak, bkc) in F32_INSTANCES and epi in F32_INSTANCES[(ak, bkc)]
        if (ak, bkc) != (0, 1):          # (TT has no ladder)
            assert g[0] == int(want_f32), (epi, ak, bkc, g)
            assert g[1] == int(bool(ref_rsi(epi, ak, bkc))) and (not g[1] or g[0]), (epi, ak, bkc, g)
        assert g[2] == int((epi, f32) in B16_INSTANCES), (epi, f32, g)


def test_tile_choice(results):
    got = results["T"]
    assert len(got) == len(T_CASES)
    for (fam, M, N, K, splits, (ak, bkc), forced), g in zip(T_CASES, got):
        assert g == ref_by_shape(fam, M, N, K, splits, ak, bkc, forced), ((fam, M, N, K, splits, ak, bkc, forced), g)
    by = {c: g for c, g in zip(T_CASES, got)}
    # M N at 2^20
    assert by[(0, 2044, 512, 512, 16, (1, 0), -1)] == (0,) and by[(0, 2048, 512, 512, 16, (1, 0), -1)] == (1,)
    # the grid at 256 workgroups: 256x128 tiles of [7936 | 8192, 1024]; 256x256 tiles of [16128 | 16384, 1024] (NT)
    assert by[(0, 7936, 1024, 512, 1, (1, 0), -1)] == (0,) and by[(0, 8192, 1024, 512, 1, (1, 0), -1)] == (1,)
    assert by[(0, 16128, 1024, 512, 1, (1, 1), -1)] == (1,) and by[(0, 16384, 1024, 512, 1, (1, 1), -1)] == (2,)
    assert by[(0, 16384, 1024, 508, 1, (1, 1), -1)] == (1,) and by[(0, 16384, 508, 512, 1, (1, 1), -1)] == (1,) and by[(0, 16384, 1024, 512, 1, (1, 0), -1)] == (1,)
    # K-splits count towards the grid (TN)
    assert by[(0, 1024, 1024, 512, 7, (0, 0), -1)] == (0,) and by[(0, 1024, 1024, 512, 8, (0, 0), -1)] == (1,) and by[(0, 1024, 1024, 512, 16, (0, 0), -1)] == (2,)
    for fam in (0, 1, 3):
        assert [by[(fam, 1024, n, 512, 1, (1, 1), -1)][0] for n in (32, 33, 64, 65)] == [4, 3, 3, 0]
    assert by[(2, 1024, 32, 512, 1, (1, 1), -1)] == (0,)                                   # x3 has no narrow tiles (its entry point delegates N <= 64)
    # forced variants; the narrow tiles ignore them
    assert by[(0, 512, 128, 512, 1, (1, 0), 4)] == (2,) and by[(0, 512, 128, 512, 1, (1, 0), 2)] == (1,) and by[(0, 512, 128, 512, 1, (1, 0), 3)] == (0,)
    assert by[(1, 512, 128, 512, 1, (1, 0), 3)] == (1,) and by[(1, 512, 128, 512, 1, (1, 0), 1)] == (0,) and by[(2, 512, 128, 512, 1, (1, 0), 3)] == (0,)
    assert by[(0, 512, 64, 512, 1, (1, 0), 4)] == (3,)
    # b16: 256x128 while the grid covers the chip, TN with K-splits on the 4-wave instance; forced 3+ = 128x128 counted at [2]
    assert by[(3, 16128, 1024, 512, 1, (1, 1), -1)] == (1, 1) and by[(3, 7936, 1024, 512, 1, (1, 1), -1)] == (0, 0)
    assert by[(3, 1024, 1024, 512, 8, (0, 0), -1)] == (2, 2) and by[(3, 8192, 1024, 512, 1, (0, 0), -1)] == (1, 1) and by[(3, 1024, 1024, 512, 7, (0, 0), -1)] == (0, 0)
    assert by[(3, 512, 128, 512, 1, (1, 1), 5)] == (0, 2) and by[(3, 512, 128, 512, 1, (1, 1), 2)] == (2, 2)
