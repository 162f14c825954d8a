"""The exact-sum inputs of tests/test_backward_exact_gpu.py are exact, and its comparisons can fail (no GPU here).

  * every builder of tests/backward_reference.py, at every shape the GPU file uses, evaluated in fp32 numpy in two summation orders -
    ascending, and a seeded permutation of the k, of a position's rows, of the slot entries, of the rows of a column - equals the float64
    value bit for bit; the three bf16 planes and the two fp16 planes (under the power-of-two scale of the recorded bound) of the exact dZ2
    sum back to it exactly (the plane emulations of tests/gemm_reference.py), and both bf16 roundings of the bf16 twin are the identity;
  * the inputs have the structure the GPU file relies on (masked positions, Z2 = +-1, pred = 0; hot, cold, pad and masked slots);
  * each of the 11 slips changes an output on some case;
  * the ten entry points are named in a tests/test_*_gpu.py file.
"""
import os
import re

import numpy as np
import pytest

from tests import backward_reference as B
from tests import gemm_reference as G
from tests.test_features_reference_cpu import ROOT, _entry_points

f32, f64 = np.float32, np.float64


def _same(a32, b64):
    """an fp32 result equals the float64 one bit for bit (as numbers: widened exactly)"""
    return a32.dtype == f32 and np.array_equal(a32.astype(f64), b64)


# ---- fused scorer dgrad -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC", B.DM_NC)
def test_dm_inputs_are_exact_sum_inputs(NC):
    for (nc, BT, C) in [c for c in B.dm_cases() if c[0] == NC]:
        for b16 in (False, True):
            inp = B.dm_inputs(NC, BT, C, b16)
            ref = B.dm_reference(inp)
            for seed in (None, 7):
                got = B.dm_reference(inp, dtype=f32, perm_seed=seed)
                for k in ref:
                    assert _same(got[k], ref[k]), (NC, BT, C, b16, seed, k)
            assert np.abs(ref['b2']).max() < 2 ** 18 / 16 and np.abs(ref['dpred']).max() < 2 ** 18 / 16 and np.abs(ref['dM']).max() <= 48
            dz = B.exact32(ref['dZ2'])
            if b16:
                # both roundings of the kernel are the identity: dM and dZ2 are bf16 values (and so are the operands)
                for x in (ref['dM'], ref['dZ2'], inp['dS1'], inp['Ws1'], inp['Z2']):
                    assert np.array_equal(G.bf16_rne(x.astype(f32)).astype(f64), x)
                assert (np.count_nonzero(inp['dS1'], axis=1) <= 1).all()
                continue
            h, m, l = G.split3(dz)
            assert np.array_equal(h.astype(f64) + m.astype(f64) + l.astype(f64), ref['dZ2']) and not l.any()
            bound = B.dm_scale_bound(inp)
            assert bound >= np.abs(ref['dM']).max()
            for s in (G.h2_scale(bound), G.h2_scale(bound) / 2):          # (the kernel's bound may round into the next binade)
                hh, ll = G.split2h(dz, s)
                assert np.isfinite(hh.astype(f32)).all()
                assert np.array_equal((hh.astype(f64) + ll.astype(f64)) / s, ref['dZ2']) and not ll.any()


def test_dm_inputs_have_the_structure_the_gpu_test_relies_on():
    seen = set()
    for NC, BT, C in B.dm_cases():
        inp = B.dm_inputs(NC, BT, C)
        ref = B.dm_reference(inp)
        m = inp['masked']
        assert not m.all() and (BT < 2 or m.any())
        rows = np.repeat(m, NC)
        assert not inp['dS1'][rows].any() and not ref['dZ2'][rows].any() and not ref['dpred'][m].any() and not ref['b2'][m].any()
        assert (np.count_nonzero(inp['dS1'], axis=1) <= B.DM_NNZ).all() and np.abs(inp['dS1']).max() <= 3
        assert (np.abs(inp['Z2']) == 1).all(1).any() and ((np.abs(inp['Z2']) == 1).any(1) & ~(np.abs(inp['Z2']) == 1).all(1)).any()
        assert set(np.unique(np.abs(inp['Z2']))) <= {0.0, 0.5, 1.0} and set(np.unique(np.abs(inp['pred']))) <= {0.0, 0.5, 1.0}
        assert set(np.unique(np.abs(inp['Ws1']))) <= {0.0, 0.5, 1.0, 2.0}
        if m.any():
            seen |= {'first'} if m[0] else set()
            seen |= {'last'} if m[-1] else set()
            seen |= {'middle'} if m[1:-1].any() else set()
        if inp['pred_zero'].any():
            seen.add('pred0')
            assert not inp['pred'][inp['pred_zero']].any()
        assert np.abs(ref['dZ2']).max() > 0 and np.abs(ref['dpred']).max() > 0
    assert seen == {'first', 'last', 'middle', 'pred0'}
    assert [B.dm_pw(nc) for nc in B.DM_NC] == [8, 7, 5, 4, 3, 2, 2, 1, 1]
    assert B.dm_bts(51) == [1, 4, 5, 6, 11] and B.dm_bts(256) == [1, 2, 3] and len(B.dm_cases()) == 3 * sum(len(B.dm_bts(nc)) for nc in B.DM_NC)


def test_every_dm_slip_changes_an_output():
    tried = {}
    for NC, BT, C in [c for c in B.dm_cases() if c[2] == B.DM_C[0]]:          # (no slip depends on the width)
        for b16 in (False, True):
            inp = B.dm_inputs(NC, BT, C, b16)
            ref = B.dm_reference(inp)
            for s in B.DM_SLIPS:
                got = B.dm_reference(inp, **{s: True})
                changed = {k for k in ('dZ2', 'dpred', 'b2') if not np.array_equal(got[k], ref[k])}
                if changed:
                    tried.setdefault(s, set()).update(changed)
                if s in ('columns_swapped', 'one_minus_z') or (s == 'pred_from_neighbour' and BT >= 2):
                    assert changed, (s, NC, BT, C, b16)                  # these apply to every case
    print({s: sorted(v) for s, v in tried.items()})
    assert set(tried) == set(B.DM_SLIPS)
    assert tried['last_row_dropped'] >= {'dZ2', 'dpred', 'b2'} and tried['row_past_valid_added'] >= {'dpred', 'b2'}
    assert tried['boundary_off_by_one'] >= {'dZ2', 'dpred', 'b2'}


# ---- combine backward -------------------------------------------------------------------------------------------------------------------------
def test_combine_inputs_are_exact_sum_inputs_with_the_slot_structure():
    hot = B.kernel_constants()['slot_hot']
    seen = set()
    for case in B.combine_cases():
        inp = B.combine_inputs(*case)
        BT, N, pmax, C, plain = case
        dU, dV = B.combine_reference(inp)
        for seed in (None, 11):
            gU, gV = B.combine_reference(inp, dtype=f32, perm_seed=seed)
            assert _same(gU, dU) and _same(gV, dV), (case, seed)
        assert np.abs(dV).max() < 2 ** 22
        slot, masked = inp['slot'], inp['masked']
        assert slot.min() >= -1 and slot.max() <= pmax and (slot[masked] == -1).all() and not (slot[~masked] == -1).any()
        for p in np.flatnonzero(~masked)[:64]:                            # a click holds a real slot at most once
            real = slot[p][slot[p] < pmax]
            assert len(set(real.tolist())) == len(real)
        holders = int((slot == 0).any(1).sum())
        assert holders == BT - masked.sum() - (inp['allpad'] >= 0) - (N == 1 and inp['cold'] >= 0)
        if holders > hot:
            seen.add('hot x %d chunks' % -(-BT // hot))
        if plain and BT == hot:
            assert holders == hot
            seen.add('at the chunk size')
        if inp['cold'] >= 0:
            assert (slot == pmax - 1).sum() == 1
            seen.add('cold')
        if inp['allpad'] >= 0:
            assert (slot[inp['allpad']] == pmax).all()
            seen.add('allpad')
        if inp['loud'] >= 0:
            assert np.abs(inp['dpre'][BT + inp['loud'] * (N + 1):BT + (inp['loud'] + 1) * (N + 1)]).max() > 0
        if masked.any():
            seen |= {'m-first'} if masked[0] else set()
            seen |= {'m-last'} if masked[-1] else set()
            seen |= {'m-middle'} if masked[1:-1].any() else set()
        seen.add('pmax 1' if pmax == 1 else 'pmax > BT N' if pmax > BT * N else 'pmax')
    assert seen >= {'hot x 2 chunks', 'hot x 3 chunks', 'at the chunk size', 'cold', 'allpad', 'm-first', 'm-last', 'm-middle', 'pmax 1', 'pmax > BT N'}, seen
    assert {c[0] for c in B.combine_cases()} == set(B.COMBINE_BT) and {c[1] for c in B.combine_cases()} == set(B.COMBINE_N)
    assert {c[3] for c in B.combine_cases()} == {4, 68}


def test_group_sums_give_du_exactly():
    for NC, BT in B.GS_CASES:
        assert (BT * NC) % 128 != 0 or NC % 128 == 0                      # (a multiple of 128 rows per click cannot avoid it)
        inp = B.combine_inputs(BT, NC - 1, 40, 68)
        dU, _ = B.combine_reference(inp)
        for dt in (f64, f32):
            dpre = inp['dpre'].astype(dt)
            gs = B.group_sums(dpre[BT:], NC)
            assert gs.shape[0] == 2 * -(-BT * NC // 256) * (127 // NC + 2) and np.isnan(gs).all(1).any()
            assert np.array_equal(B.du_from_group_sums(dpre[:BT], gs, BT, NC - 1).astype(f64), dU)
        # the same layout as the GEMM reference's
        class P:
            group_rows, M, N = NC, BT * NC, 68
        assert np.array_equal(G.group_sums(P, inp['dpre'][BT:].astype(f64)), B.group_sums(inp['dpre'][BT:].astype(f64), NC), equal_nan=True)


def test_every_combine_slip_changes_an_output():
    tried = set()
    for case in B.combine_cases():
        inp = B.combine_inputs(*case)
        dU, dV = B.combine_reference(inp)
        for s in B.COMBINE_SLIPS:
            if not np.array_equal(B.combine_reference(inp, **{s: True})[1], dV):
                tried.add(s)
            elif s == 'pad_slot_dropped':
                assert not (inp['slot'] == inp['pmax']).any() or not dV[-1].any(), case
    for NC, BT in B.GS_CASES:
        inp = B.combine_inputs(BT, NC - 1, 40, 68)
        dpre = inp['dpre'].astype(f64)
        gs = np.nan_to_num(B.group_sums(dpre[BT:], NC), nan=1.0)
        if not np.array_equal(B.du_from_group_sums(dpre[:BT], gs, BT, NC - 1, piece_k_plus_1=True), B.combine_reference(inp)[0]):
            tried.add('piece_k_plus_1')
    assert tried == set(B.COMBINE_SLIPS + B.GS_SLIPS)


# ---- feature backward -------------------------------------------------------------------------------------------------------------------------
def test_feature_inputs_are_exact_sum_inputs_and_the_slip_shows():
    k = B.kernel_constants()
    assert k['sbw_chunks'] >= 2 and k['sbw_min_rows'] >= 2 and k['slot_hot'] % 32 == 0
    rs = B.feature_rs()
    m = k['sbw_min_rows']
    assert {1, 63, 64, 65, m - 1, m, m + 1} <= set(rs) and B.feature_rows_per_chunk(rs[-1]) == m + 1 and B.feature_rows_per_chunk(rs[-2]) == m
    assert {c[1] for c in B.feature_cases()} == set(B.FEATURE_F) and {c[0] for c in B.feature_cases()} == set(rs)
    tried = set()
    for R, F in B.feature_cases():
        dxs, xraw = B.feature_inputs(R, F)
        dg, db = B.feature_reference(dxs, xraw)
        for seed in (None, 3):
            g32, b32 = B.feature_reference(dxs, xraw, dtype=f32, perm_seed=seed)
            assert _same(g32, dg) and _same(b32, db), (R, F, seed)
        assert np.array_equal(dg, (dxs.astype(f64) * xraw.astype(f64)).sum(0)) and np.array_equal(db, dxs.astype(f64).sum(0))
        sg, sb = B.feature_reference(dxs, xraw, chunk_edge_row_dropped=True)
        if R > B.feature_rows_per_chunk(R):
            assert not np.array_equal(sg, dg) and not np.array_equal(sb, db), (R, F)
            tried.add('chunk_edge_row_dropped')
    assert tried == set(B.FEATURE_SLIPS)


def test_the_slip_table_is_complete():
    assert set(B.SLIPS) == set(B.DM_SLIPS) | set(B.COMBINE_SLIPS) | set(B.GS_SLIPS) | set(B.FEATURE_SLIPS) and len(B.SLIPS) == 11


# ---- the random-data bounds -------------------------------------------------------------------------------------------------------------------
def test_random_data_bounds_are_fp32_roundoff_and_a_slip_breaks_them():
    inp = B.dm_random_inputs()
    sa, sw = G.h2_scale(float(np.sqrt((inp['dS1'].astype(f64) ** 2).sum(1)).max())), G.h2_scale(float(np.sqrt((inp['Ws1'].astype(f64) ** 2).sum(1)).max()))
    for form in ('p3', 'h2h', 'b16'):
        ref, S, bound, extra = B.dm_random_reference(inp, form, sa, sw)
        print(form, {k: float('%.2e' % v) for k, v in bound.items()})
        assert all((0 < v or form == 'b16') and v < 1e-5 for v in bound.values()), bound          # (the GEMM family's: 0.2-4.6e-6)
        if form == 'b16':
            # almost every element is far from a bf16 rounding boundary: there the kernel has to store the reference's bits
            assert extra['safe'].mean() > 0.98 and bound['dZ2'] == 0.0 and bound['dpred'] > 0 and bound['b2'] > 0, (extra['safe'].mean(), bound)
        # one row given to the neighbouring position: far outside every per-element bound
        bad = ref['b2'].copy()
        bad[0] += ref['dZ2'][inp['NC']]
        assert B.ratio(bad, ref['b2'], S['b2'], extra['b2']) > 10 * bound['b2']
    for name, (ref, S, bound) in B.combine_random_reference().items():
        assert all(0 <= b < 2e-6 for b in bound), (name, bound)
    ref, S, bound = B.feature_random_reference()
    assert all(0 < b < 1e-5 for b in bound), bound


# ---- the gate ---------------------------------------------------------------------------------------------------------------------------------
def test_every_entry_point_of_the_backward_path_is_named_in_a_gpu_test():
    fused = _entry_points("dm_fused.hip")
    assert fused == sorted(['cham_dm_mulpred_p3', 'cham_dm_mulpred_h2', 'cham_dm_mulpred_h2h', 'cham_dm_mulpred_h2_blk', 'cham_dm_mulpred_b16'])
    names = fused + ['cham_combine_bwd', 'cham_combine_bwd_gs', 'cham_combine_bwd_b16', 'cham_feature_bwd', 'cham_feature_bwd_ws']
    assert all(n in _entry_points("scorer.hip") for n in names[5:8]) and all(n in _entry_points("features.hip") for n in names[8:])
    assert len(names) == 10
    tdir = os.path.join(ROOT, "tests")
    text = {f: open(os.path.join(tdir, f)).read() for f in sorted(os.listdir(tdir)) if re.fullmatch(r"test_\w+_gpu\.py", f)}
    missing = [n for n in names if not any(re.search(r"\blib\.%s\(" % n, t) for t in text.values())]
    assert not missing, "entry points without a direct GPU test: %s" % missing
    # ... and in the file that holds them to the exact references
    missing = [n for n in names if not re.search(r"\b%s\b" % n, text["test_backward_exact_gpu.py"])]
    assert not missing, "entry points tests/test_backward_exact_gpu.py does not name: %s" % missing
