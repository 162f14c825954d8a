"""Where the bounds of tests/test_gemm_views_gpu.py come from, and that they can fail (no GPU here).

  * For every case of tests/gemm_reference.CASES the fp32-CPU twin (the same plane products in float32, added one k after the other, the
    entry point's K-splits added in ascending order, the epilogue in float32) is compared with the float64 reference element by element:
    e = max_ij |twin - ref| / S_ij with S the element's own sum of absolute terms.  The case's bound is 8 e (8: the rule of
    tests/test_tail_reference_cpu.py - the GPU's summation order and its tanhf differ from numpy's by a few ulp, and every slip has to stay
    10 x above the result); a bf16 output is allowed one round-to-nearest-even rounding, 2^-8 |ref|, on top.  The table is printed.
  * Each slip of gemm_reference.SLIPS, applied to the twin, moves some case's worst element past 10 x its bound or changes the guarded frame
    of its output: the case table is rich enough to see every one of them.
  * The twin itself leaves every frame intact and fills every interior.
  * Every `extern "C" int cham_gemm_*` entry point of the five GEMM files is named in tests/test_gemm_views_gpu.py; cham_split3,
    cham_split2h and the cham_h2_scale_* entry points there or in an existing tests/test_gemm_*_gpu.py.
"""
import glob
import os
import re

import numpy as np
import pytest

from tests import gemm_reference as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEMM_FILES = ("gemm.hip", "gemm_x3.hip", "gemm_b16.hip", "gemm_p3.hip", "gemm_h2.hip")


def _cost(p):
    return p.M * p.N * max(p.K, 1) * len(p.products)


def test_bound_table_and_the_twin_respects_every_guard():
    print()
    worst = {}
    for p in G.RUN_CASES:
        k = G.bound(p)
        intact, ratio = G.judge(p, G.twin(p))
        assert intact, p.name
        assert ratio <= k / G.MARGIN * 1.0000001, (p.name, ratio, k)          # (a bf16 output: the twin's own rounding stays inside 2^-8 |ref|)
        assert k < 1e-4, (p.name, k)                                        # fp32-grade everywhere: nothing hides behind a loose bound
        print("    %-44s e = %.2e   bound 8 e = %.2e   K-splits %d" % (p.name, k / G.MARGIN, k, p.plan()[0]))
        worst[p.arm] = max(worst.get(p.arm, 0.0), k)
    for arm, k in worst.items():
        print("    largest bound of %-12s %.2e" % (arm, k))


def test_the_case_table_covers_what_the_issue_lists():
    arms = {p.arm for p in G.RUN_CASES}
    assert arms == set(G.ENTRY), arms
    for arm in ('f32', 'bf16'):
        ns = {(p.form, p.N) for p in G.RUN_CASES if p.arm == arm and p.M == 300}
        assert {('NN', n) for n in (260, 72, 64, 36, 32, 12)} <= ns and {('NT', n) for n in (260, 72, 64, 36, 32, 12, 6)} <= ns, ns
    # the TN matrix of the register-staged arms: K of 70 and 1100, unsplit and splits_hint 0, 3 and 8, each with and without accumulate -
    # on the arm's own kernels (cham_gemm_f32x3 hands N <= 64 to cham_gemm_f32), and every column count the arm takes among them
    for arm, ns in (('f32', (260, 72, 64, 36, 32, 12)), ('bf16', (260, 72, 64, 36, 32, 12)), ('f32x3', (260, 72)), ('f32x2h', (260, 72)),
                    ('b16', (264, 72, 64, 40, 32, 16))):
        own = [p for p in G.RUN_CASES if p.arm == arm and p.form == 'TN' and p.M in (300, 304) and p.N in ns and not p.switch]
        assert {(K, h, a) for K in (70, 1100) for h in (1, 0, 3, 8) for a in (0, 1)} <= {(p.K, p.hint, p.accumulate) for p in own}, arm
        assert {(K, s, a) for K in (70, 1100) for s in (False, True) for a in (0, 1) if not (K == 70 and s)} <= {(p.K, p.plan()[0] > 1, p.accumulate) for p in own}, arm
        assert {(n, a) for n in ns for a in (0, 1)} <= {(p.N, p.accumulate) for p in own}, arm
        assert any(p.plan()[0] % 8 == 0 for p in own), arm          # one K-split per XCD: the other layout of the partials
    for arm in ('f32', 'bf16', 'f32x3', 'f32x2h'):      # the scalar branch of the split-K reduction: ldc % 4 != 0, split and unsplit
        odd = {p.plan()[0] > 1 for p in G.RUN_CASES if p.arm == arm and p.form == 'TN' and p.C.ld % 4}
        assert odd == {False, True}, (arm, odd)
    assert {(p.M, p.N, p.K) for p in G.RUN_CASES if p.counter and p.counter[2] == 5 and p.arm == 'f32'} == {(100, 36, 1100), (36, 12, 600), (128, 200, 777)}
    for arm in ('p3', 'h2', 'b16_dma'):
        assert {p.K for p in G.RUN_CASES if p.arm == arm and p.form == 'NT'} == {80, 96, 192}
        assert {(p.M, p.K) for p in G.RUN_CASES if p.arm == arm and p.form == 'TN'} >= {(m, k) for m in (256, 512) for k in (70, 1100)}
    for p in G.RUN_CASES:      # every view is a real view
        for v in (p.A, p.B) if not (p.a_blocked or p.b_blocked) else ((p.B,) if p.a_blocked else (p.A,)):
            assert v.ld > v.cols and v.col0 > 0 and (v.planes == 1 or v.ps > v.rows * v.ld), p.name
        assert p.C.ld > p.N and (p.R is None or p.R.ld not in (p.C.ld, p.N)) and (p.RS is None or p.RS.ld > p.RS.cols), p.name
    for arm in ('f32', 'bf16', 'f32x3'):          # a C aligned to 4 bytes only: the scalar branch through the alignment alone, split and unsplit
        odd = {p.plan()[0] > 1 for p in G.RUN_CASES if p.arm == arm and p.C.col0 % 4 and p.C.ld % 4 == 0}
        assert odd and (arm != 'f32' or odd == {False, True}), (arm, odd)
    assert any(p.R is not None and p.R.col0 % 4 for p in G.RUN_CASES)
    # the cases that name the narrow NT kernel of a plane arm also name the counter of the 64-byte-piece kernel, which must stay
    for arm, wide, mod in (('h2', 2, 32), ('b16_dma', 4, 64)):
        for p in G.RUN_CASES:
            if p.arm == arm and p.form == 'NT':
                narrow = p.K % mod != 0 or (p.switch is not None and p.switch[1] == 0)
                assert (p.quiet == (wide,) and p.counter[2] != wide) if narrow else (p.counter[2] == wide and not p.quiet), p.name
    assert any(p.rs_div == 51 and p.A.rows % 51 for p in G.RUN_CASES)          # the last row group is partial
    switches = {p.switch[0] for p in G.RUN_CASES if p.switch}
    assert switches == {'cham_gemm_set_variant', 'cham_gemm_f32x3_set_variant', 'cham_gemm_b16_set_variant', 'cham_gemm_h2_set_nt_wide',
                        'cham_gemm_b16_dma_set_nt_wide'}, switches


def test_poison_moves_an_element_by_more_than_1000_bounds():
    for p in (c for c in G.RUN_CASES if c.K and not c.a_blocked):
        d = G.data(p)
        _, S = G.reference(p)
        poison = G.POISON_F16 * float(d['rec_a'][1]) if p.arm in G.H2_ARMS else G.POISON
        b = np.abs(np.asarray(d['B'][0], np.float64)) * (float(d['rec_b'][1]) if p.arm in G.H2_ARMS else 1.0)      # one poisoned a against the median |b|
        assert poison * float(np.median(b)) > 1000 * G.bound(p) * float(np.median(S)), p.name


@pytest.mark.parametrize("slip", G.SLIPS)
def test_every_slip_breaks_a_bound_tenfold_or_touches_a_guard(slip):
    cases = sorted((p for p in G.RUN_CASES if G.applies(slip, p)), key=_cost)
    assert cases, "no case to which the slip applies"
    for p in cases[:12]:
        intact, ratio = G.judge(p, G.twin(p, slip))
        if not intact or ratio > 10 * G.bound(p):
            print("    %-28s caught by %-40s frame intact %s, %.2e against the bound %.2e" % (slip, p.name, intact, ratio, G.bound(p)))
            return
    raise AssertionError("%s passes every case it applies to" % slip)


def test_group_sum_reference_adds_up_to_the_whole_groups():
    p = next(c for c in G.RUN_CASES if c.arm == 'h2_dgrad_gs')
    ref, _ = G.reference(p)
    gs = G.group_sums(p, ref)
    per_group = np.zeros((p.M // p.group_rows, p.N))
    gsk = 127 // p.group_rows + 2
    for q in range(-(-p.M // 128)):
        for k in range(gsk):
            if not np.isnan(gs[q * gsk + k]).any():
                per_group[128 * q // p.group_rows + k] += gs[q * gsk + k]
    assert np.allclose(per_group, ref.reshape(-1, p.group_rows, p.N).sum(1), rtol=0, atol=1e-9)


# ---- catalogue ------------------------------------------------------------------------------------------------------------------------------
def _entry_points(path, start=None):
    src = open(os.path.join(ROOT, "chameleon_recsys_amd", "csrc", path)).read()
    if start is not None:
        src = src[src.index('extern "C" int %s(' % start):]
    return sorted(set(re.findall(r'extern "C" int (cham_\w+)\s*\(', src)))


def test_every_gemm_entry_point_is_named_in_a_gpu_test():
    names = sorted(set(sum((_entry_points(f) for f in GEMM_FILES), [])))
    gemms = [n for n in names if n.startswith("cham_gemm_")]
    assert len(gemms) >= 12 and set(G.ENTRY.values()) <= set(gemms), gemms
    views = open(os.path.join(ROOT, "tests", "test_gemm_views_gpu.py")).read()
    missing = [n for n in gemms if not re.search(r"\b%s\b" % n, views)]
    assert not missing, "GEMM entry points without a case in tests/test_gemm_views_gpu.py: %s" % missing
    assert {G.ENTRY[p.arm] for p in G.RUN_CASES} == set(G.ENTRY.values())
    helpers = [n for n in names if n in ("cham_split3", "cham_split2h") or n.startswith("cham_h2_scale_")]
    assert len(helpers) == 5, helpers
    text = views + "".join(open(f).read() for f in glob.glob(os.path.join(ROOT, "tests", "test_gemm_*_gpu.py")))
    missing = [n for n in helpers if not re.search(r"\b%s\b" % n, text)]
    assert not missing, "split / scale entry points without a direct GPU test: %s" % missing
