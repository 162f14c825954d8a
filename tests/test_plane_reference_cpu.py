"""The host models of tests/plane_reference.py are right, and the assertions of tests/test_plane_producers_gpu.py can fail (no GPU here).

  * the models against each other, against float64 and against literal restatements: the record (frexp / ldexp against float64 logarithms),
    the loop a row of the K == 128 row-norm kernel goes through (against the kernel's two loops walked one half-wave at a time), the planted
    rows (exact sums in two orders), the tile-blocked index (against a reshaped array), both splits (against float64 and the bf16 rounding
    of tests/tail_reference.py);
  * the cases reach the branches they are named for at the caps the kernels' sources state, and still do if a cap doubles;
  * the assertions of the GPU file - the functions of tests/plane_reference.py it calls - run here on host emulations: clean ones pass, and
    each slip of plane_reference.SLIPS fails one (for the loop slips: at exactly the placements that lie in the slipped branch);
  * the nine entry points are called by the GPU file.
"""
import os
import re

import numpy as np
import pytest

from tests import features_reference as F
from tests import gemm_reference as G
from tests import plane_reference as PR
from tests.test_features_reference_cpu import ROOT

f32, f64 = np.float32, np.float64
BLK = 8192                     # cham_h2b_block_elements() of the default build (H2B_PAD 0)


def _src(name):
    return open(os.path.join(ROOT, "chameleon_recsys_amd", "csrc", name)).read()


# ---- the caps and the branches ---------------------------------------------------------------------------------------------------------------
def test_caps_are_the_ones_the_sources_state():
    h2, p3 = _src("gemm_h2.hip"), _src("gemm_p3.hip")
    body = lambda src, name: src[src.index('extern "C" int %s(' % name):].split("\n}\n")[0]
    assert "blocks > %d ? %d : blocks" % (PR.ABSMAX_CAP, PR.ABSMAX_CAP) in body(h2, "cham_h2_scale_absmax")
    assert "blocks > %d ? %d : blocks" % (PR.ROWNORM_CAP, PR.ROWNORM_CAP) in body(h2, "cham_h2_scale_rownorm2")
    assert "const long per = K == 128 ? 8 : 4;" in body(h2, "cham_h2_scale_rownorm2")
    assert "if (blocks > %d) blocks = %d;" % (PR.SPLIT_CAP, PR.SPLIT_CAP) in body(h2, "cham_split2h")
    assert "if (blocks > %d) blocks = %d;" % (PR.SPLIT_CAP, PR.SPLIT_CAP) in body(p3, "cham_split3")
    assert "for (; r + 3 * stride < R; r += 4 * stride)" in h2 and "1.0009765625f" in h2
    assert "#define H2B_ROWS 256" in _src("common.h") and "#define H2B_COLS 32" in _src("common.h")


def _walk_rownorm_loops(R, cap):
    """k_h2_scale_rownorm, K == 128, one half-wave at a time: the slot (0-3) or -1 (tail loop) that reads each row"""
    blocks = min(max((R + 7) // 8, 1), cap)
    stride = 8 * blocks
    path = np.full(R, -9)
    for r0 in range(min(stride, R)):
        r = r0
        while r + 3 * stride < R:
            for u in range(4):
                assert path[r + u * stride] == -9
                path[r + u * stride] = u
            r += 4 * stride
        while r < R:
            assert path[r] == -9
            path[r] = -1
            r += stride
    return path


@pytest.mark.parametrize("cap", [PR.ROWNORM_CAP, 2 * PR.ROWNORM_CAP])
def test_rownorm_cases_reach_every_loop_and_slot(cap, monkeypatch):
    monkeypatch.setattr(PR, "ROWNORM_CAP", cap)
    reached = set()
    for R in PR.ROWNORM_R:
        paths = PR.rownorm_paths(R)
        assert np.array_equal(paths, _walk_rownorm_loops(R, cap)), R
        rows = PR.rownorm_placements(R, 128)
        assert rows[0] == 0 and rows[-1] == R - 1
        for p in np.unique(paths):
            hit = [r for r in rows if paths[r] == p]
            assert hit, (R, p)
            if (paths == p).sum() > 4:
                assert {r % 2 for r in hit} == {0, 1}, (R, p)          # an even and an odd row: both half-waves of a wave
            reached.add(int(p))
    assert reached == {0, 1, 2, 3, -1}
    if cap == PR.ROWNORM_STRIDE // 8:
        assert [set(np.unique(PR.rownorm_paths(R))) == {-1} for R in PR.ROWNORM_R] == [True] * 7 + [False] * 3


@pytest.mark.parametrize("cap", [PR.ABSMAX_CAP, 2 * PR.ABSMAX_CAP])
def test_absmax_cases_reach_a_second_and_a_third_pass(cap, monkeypatch):
    monkeypatch.setattr(PR, "ABSMAX_CAP", cap)
    P = cap * 1024
    passes = set()
    for name, n0, n1, plants in PR.absmax_cases():
        if isinstance(n0, str):
            continue
        for which, i, v in plants:
            n = (n0, n1)[which]
            assert 0 <= i < n
            passes.add((i // 4) // (PR.absmax_blocks(n0, n1) * 256))
    assert passes >= ({0, 1, 2, 3} if cap == PR.ABSMAX_PASS // 1024 else {0, 1})
    assert P + 4 > P                                                     # (the sizes themselves are fixed by the issue)


# ---- the models ---------------------------------------------------------------------------------------------------------------------------
def test_record_model_against_float64():
    rng = np.random.default_rng(1)
    bounds = np.concatenate([np.exp2(rng.uniform(-90, 90, 500)), 2.0 ** np.arange(-94, 95), np.nextafter(f32(2.0) ** np.arange(-94, 95, dtype=f32), f32(0))]).astype(f32)
    for b in bounds:
        w = PR.record_words(b)
        assert not PR.record_failures(w, b)
        s, inv, bb = (f64(v) for v in w[:3].view(f32))
        assert bb == f64(b) and s * inv == 1.0 and s == 2.0 ** (14 - np.floor(np.log2(f64(b)))) and 2.0 ** 14 <= bb * s < 2.0 ** 15
    for b, s in ((0.0, 1.0), (-0.0, 1.0), (np.inf, 1.0), (2.0 ** -140, 2.0 ** 110), (2.0 ** -120, 2.0 ** 110), (2.0 ** 127, 2.0 ** -110)):
        w = PR.record_words(f32(b))
        assert w[:2].view(f32)[0] == f32(s) and f64(w[:2].view(f32)[1]) == 1.0 / s and not PR.record_failures(w, f32(b))
        assert PR.record_clamped(f32(b)) == (s not in (1.0,))
    assert list(PR.record_words(f32(0))[:3].view(f32)) == [1.0, 1.0, 0.0]


def test_absmax_model_against_float64():
    for case in PR.absmax_cases():
        x0, x1 = PR.absmax_inputs(case)
        got = PR.absmax_bound(x0, x1)
        a = np.nanmax(np.abs(x0.astype(f64)), initial=0.0)
        b = 0.0 if x1 is None else np.nanmax(np.abs(x1.astype(f64)), initial=0.0)
        with np.errstate(over='ignore'):
            assert PR.word32(got) == PR.word32(f32(a + b)), case[0]      # the float64 sum of two fp32 values is exact: one rounding either way
        for which, i, v in case[3]:
            if not isinstance(case[1], str):
                assert abs(v) > 1.0 and abs((x0, x1)[which][i]) == abs(v)  # above the U(-1, 1) background
    x0, x1 = PR.absmax_inputs(next(c for c in PR.absmax_cases() if c[0] == 'equal_in_both'))
    assert PR.absmax_bound(x0, x1) == 2 * PR.B_MAG


def test_planted_rows_are_exact_in_any_order():
    rng = np.random.default_rng(2)
    for K in (128,) + PR.GENERIC_K:
        for vname, cols in PR.rownorm_variants(K):
            for amp in (1.0, 2.0, 4.0, 2.0 ** 40, 2.0 ** -40):
                row = PR.planted_row(K, cols, amp, flip=int(rng.integers(3)))
                if cols is not None:
                    assert not np.delete(row, cols).any() and np.count_nonzero(row) == 4
                elif K == 128:
                    assert (np.count_nonzero(row.reshape(32, 4), axis=1) == 2).all()          # two entries in every lane's float4
                assert (row > 0).any() and ((row < 0).any() or K < 4)
                sq = (row * row).astype(f32)
                for order in (np.arange(K), rng.permutation(K)):
                    acc = f32(0)
                    for v in sq[order]:
                        acc = f32(acc + v)
                    assert f64(acc) == 1024.0 * amp * amp == PR.rownorm_row_sq(row[None], K)[0]
                assert np.sqrt(f32(acc), dtype=f32) == f32(32 * amp)
                b, plain = PR.rownorm_bounds(PR.rownorm_row_sq(row[None], K), K, 2.0 ** -3)
                assert f64(plain) == 32 * amp * (1 + 2.0 ** -10) and f64(b) == f64(plain) / 8
    X = PR.rownorm_background(50, 128, 136)
    assert np.isnan(X[:, 128:]).all() and set(np.unique(X[:, :128])) == {-1.0, 0.0, 1.0} and PR.rownorm_row_sq(X, 128).max() <= 128
    assert PR.rownorm_bounds(np.zeros(0), 128)[0] == 0 and list(PR.record_words(0)[:3].view(f32)) == [1, 1, 0]


def test_split_models_against_float64_and_the_other_bf16_rounding():
    for R, Cc in PR.SPLIT_SHAPES[:2]:
        for mode in ('absmax',) + (('rownorm',) if R > 1 else ()):
            X, bound, scale = PR.split_inputs(R, Cc, mode)
            if mode == 'absmax':
                assert bound == np.abs(X).max() == 7.5
            else:
                n = np.sqrt((X.astype(f64) ** 2).sum(1))
                assert n.argmax() == 0 and n[0] == 64 and n[1:].max() < 48 and f64(bound) == 64 * (1 + 2.0 ** -10)
            hb, lb = PR.split2h_planes(X, scale)
            assert not PR.h2_property_failures(hb, lb, X, scale)
            start = Cc if mode == 'rownorm' else 1
            k = min(len(PR.SPLIT2H_PLANTS), R * Cc - start)
            assert np.array_equal(X.reshape(-1)[start:start + k].astype(f64) * scale, np.array(PR.SPLIT2H_PLANTS[:k]))      # planted exactly
            hp, lp = hb.reshape(-1)[start:start + k], lb.reshape(-1)[start:start + k]
            assert hp[0] == 0x0001 and hp[1] == 0x8000 and hp[2] == 0x8000
            if k == len(PR.SPLIT2H_PLANTS):
                hv, lv = hp.view(np.float16).astype(f64), lp.view(np.float16).astype(f64)
                want = {2049.0: (2048, 1), 2051.0: (2052, -1), -2049.0: (-2048, -1), 1024.25 + 2.0 ** -13: (1024, 0.25),
                        1024.25 + 3 * 2.0 ** -13: (1024, 0.25 + 2.0 ** -11), 2.0 ** -25: (2.0 ** -24, 0), 2.0 ** -24: (2.0 ** -24, 0),
                        3 * 2.0 ** -24: (3 * 2.0 ** -24, 0), 2.0 ** -26: (2.0 ** -24, 0)}
                for i, v in enumerate(PR.SPLIT2H_PLANTS):
                    if v in want:
                        assert (hv[i], lv[i]) == want[v], (v, hv[i], lv[i])
    X, _, _ = PR.split_inputs(300, 264, 'p3')
    planes = PR.split3_planes(X)
    h = F.round_bf16_bits(X)
    r1 = (X.astype(f64) - G.bf16_from_bits(h).astype(f64)).astype(f32)
    m = F.round_bf16_bits(r1)
    r2 = (r1.astype(f64) - G.bf16_from_bits(m).astype(f64)).astype(f32)
    for got, want in zip(planes, (h, m, F.round_bf16_bits(r2))):
        assert np.array_equal(got, want.reshape(X.shape))
    back = sum(G.bf16_from_bits(p).astype(f64) for p in planes)
    assert np.abs(back - X.astype(f64)).max() <= 2.0 ** -23 * np.abs(X.astype(f64)).max()
    k = len(PR.SPLIT3_PLANTS)
    assert np.array_equal(X.reshape(-1)[1:1 + k], np.array(PR.SPLIT3_PLANTS, f32))
    hv = G.bf16_from_bits(planes[0]).reshape(-1)[1:1 + k]
    assert hv[2] == 1.0 and hv[3] == f32(1 + 2.0 ** -6) and G.bf16_from_bits(planes[1]).reshape(-1)[1 + 5] == f32(2.0 ** -10)


@pytest.mark.parametrize("blk", [8192, 8192 + 64])
def test_blocked_index_against_a_reshaped_array(blk):
    rows, C = 700, 96
    tiles, ncb = (rows + 255) // 256, C // 32
    flat = np.full(tiles * ncb * blk, -1, np.int64)
    blocks = flat.reshape(tiles, ncb, blk)[:, :, :8192].reshape(tiles, ncb, 256, 32)          # [row tiles][column blocks][256][32] (a view)
    r, c = np.arange(rows)[:, None], np.arange(C)[None, :]
    blocks[r // 256, c // 32, r % 256, c % 32] = r * C + c
    idx = PR.h2b_index(r, c, ncb, blk)
    assert np.array_equal(flat[idx], r * C + c) and np.unique(idx).size == rows * C and idx.max() < flat.size
    lay = PR.combine_layout(rows, C, 2, 1, blk)
    assert lay['plane'] == tiles * ncb * blk and lay['ps'] > lay['plane'] and lay['ps'] % 4 == 0


# ---- the assertions of the GPU file on emulations: clean ones pass, every slip fails ----------------------------------------------------------
def _rownorm_emulation(slip):
    """-> {(R, row, variant): failures} over the K == 128 cases of the GPU file (ld 128) and one generic case"""
    out = {}
    for R in PR.ROWNORM_R:
        K = 128
        Xh = PR.rownorm_background(R, K, K, seed=R)
        sq0c, sq0s = PR.rownorm_row_sq(Xh, K), PR.rownorm_row_sq(Xh, K, **slip)
        n = 0
        for row in PR.rownorm_placements(R, K):
            for vname, cols in PR.rownorm_variants(K):
                prow = PR.planted_row(K, cols, 2.0 ** (n % 3), flip=n)
                fac = (None, 2.0 ** -3, 2.0 ** 5)[n % 3]
                clean, slipped = sq0c.copy(), sq0s.copy()
                clean[row], slipped[row] = PR.rownorm_row_sq(prow[None], K)[0], PR.rownorm_row_sq(prow[None], K, **slip)[0]
                want, want_plain = PR.rownorm_bounds(clean, K, fac)
                got, got_plain = PR.rownorm_bounds(slipped, K, fac, **slip)
                out[(R, row, vname)] = PR.record_failures(PR.record_words(got, **slip), want) + PR.record_failures(PR.record_words(got_plain, **slip), want_plain)
                n += 1
    return out


def _absmax_emulation(slip):
    out = {}
    for case in PR.absmax_cases():
        x0, x1 = PR.absmax_inputs(case)
        out[case[0]] = PR.record_failures(PR.record_words(PR.absmax_bound(x0, x1, **slip), **slip), PR.absmax_bound(x0, x1))
    return out


def _split_emulation(slip):
    out = {}
    for R, Cc in PR.SPLIT_SHAPES[:2]:
        for layout in PR.SPLIT_LAYOUTS:
            lay = PR.split_layout(R, Cc, layout, 2)
            X, bound, scale = PR.split_inputs(R, Cc, 'absmax' if (lay['recompute'] or R == 1) else 'rownorm')
            want = PR.split_expected(PR.split2h_planes(X, scale), R, Cc, lay, PR.FILL_F16)
            hb, lb = PR.split2h_planes(X, scale, **slip)
            try:
                got = PR.split_expected([hb, lb], R, Cc, lay, PR.FILL_F16, **slip)
            except IndexError:
                out[(R, Cc, layout[0])] = ["a write outside the buffer"]
                continue
            out[(R, Cc, layout[0])] = PR.buffer_failures(got, want) + PR.h2_property_failures(hb, lb, X, scale)
            if not slip:
                x3, _, _ = PR.split_inputs(R, Cc, 'p3')
                lay3 = PR.split_layout(R, Cc, layout, 3)
                e3 = PR.split_expected(PR.split3_planes(x3), R, Cc, lay3, PR.FILL_BF16)
                inside = np.count_nonzero(e3 != PR.FILL_BF16)
                assert inside >= 3 * R * Cc * (1 if lay3['which'] != 'both' else 2) - 3 * 4 * R * Cc // 100          # (a plane value may equal the fill: none does)
    return out


def _combine_inputs():
    yield "case 1 C 64", F.combine_inputs(1, 64)
    yield "case 2 C 128", F.combine_inputs(2, 128)
    yield "case 4 C 64", F.combine_inputs(4, 64)
    for i in range(len(PR.COMBINE_EXTRA)):
        yield "extra %d" % i, PR.combine_extra_inputs(i)
    yield "pad-row bound", PR.combine_pad_large_inputs()


def _combine_emulation(slip):
    out = {}
    for name, inp in _combine_inputs():
        BT, N, C = inp['BT'], inp['N'], inp['C']
        rows = BT * (N + 1)
        scale = G.h2_scale(PR.absmax_bound(inp['U'].reshape(-1), inp['V'].reshape(-1)))
        z = PR.combine_rows(inp)
        for arm, blocked in (('p3', 0), ('h2', 0), ('h2', 1)):
            npl, fill = (3, PR.FILL_BF16) if arm == 'p3' else (2, PR.FILL_F16)
            lay = PR.combine_layout(rows, C, npl, blocked, BLK)
            want = PR.combine_expected(PR.combine_planes(inp, arm, scale), rows, C, lay, blocked, BLK, fill)
            planes = PR.combine_planes(inp, arm, scale, **slip)
            try:
                got = PR.combine_expected(planes, rows, C, lay, blocked, BLK, fill, **slip)
            except IndexError:
                out[(name, arm, blocked)] = ["a write outside the buffer"]
                continue
            bad = PR.buffer_failures(got, want)
            if arm == 'h2' and not blocked:
                bad += PR.h2_property_failures(planes[0], planes[1], z, scale, exact_sum=False)
            out[(name, arm, blocked)] = bad
            if not slip and blocked and rows % 256:
                tail = want[lay['off']:lay['off'] + lay['plane']].reshape(-1, BLK)[-1].reshape(256, 32)[rows % 256:]
                assert (tail == fill).all()                              # the rows of the last tile beyond the matrix keep the initial value
    return out


EMULATIONS = {'rownorm': _rownorm_emulation, 'absmax': _absmax_emulation, 'split': _split_emulation, 'combine': _combine_emulation}
WHERE = {'skip_u3': 'rownorm', 'drop_tail': 'rownorm', 'drop_unrolled': 'rownorm', 'no_margin': 'rownorm', 'half_reduce_16': 'rownorm',
         'drop_second_pass': 'absmax', 'ignore_x1': 'absmax', 'max_for_sum': 'absmax', 'exponent_off_by_one': 'absmax', 'scratch_armed': 'absmax',
         'no_keep_sign': 'split', 'l_unscaled': 'split', 'transposed_with_ldd': 'split', 'pad_slot_from_row_0': 'combine', 'pmax_not_pad': 'combine',
         'wrong_col_blocks': 'combine', 'row_not_mod_256': 'combine'}


@pytest.mark.parametrize("family", sorted(EMULATIONS))
def test_clean_emulations_pass_every_assertion(family):
    res = EMULATIONS[family]({})
    assert res and not {k: v for k, v in res.items() if v}


@pytest.mark.parametrize("slip", PR.SLIPS)
def test_every_slip_fails_an_assertion(slip):
    assert set(WHERE) == set(PR.SLIPS)
    res = EMULATIONS[WHERE[slip]]({slip: True})
    caught = {k for k, v in res.items() if v}
    print("\n    %-22s fails %d of %d cases" % (slip, len(caught), len(res)))
    assert caught
    if slip in ('skip_u3', 'drop_tail', 'drop_unrolled'):
        # the loop slips: caught at exactly the placements the slipped branch reads - every one of them, and nowhere else
        inside = {3: lambda p: p == 3, -1: lambda p: p == -1, 0: lambda p: p >= 0}[{'skip_u3': 3, 'drop_tail': -1, 'drop_unrolled': 0}[slip]]
        assert caught == {k for k in res if inside(PR.rownorm_paths(k[0])[k[1]])}
    if slip in ('exponent_off_by_one', 'scratch_armed'):
        assert len(caught) >= len(res) - 4                               # (not where the bound is 0 or inf: scale 1, nothing armed)
        assert all(v for v in _rownorm_emulation({slip: True}).values())
    if slip == 'no_keep_sign':
        assert ("pad-row bound", 'h2', 0) in {k for k, v in _combine_emulation({slip: True}).items() if any("int16" in m for m in v)}
        assert all(any("int16" in m for m in v) for v in res.values())   # the sign assertion itself, at every shape and layout
    if slip == 'l_unscaled':
        assert all(any("h + l" in m for m in v) for k, v in res.items() if k[:2] != (1, 4))
    if slip == 'transposed_with_ldd':
        assert caught == {k for k in res if k[2] not in ('dst_only', 'dst_recompute')}          # wherever a transposed plane is written
    if slip in ('pad_slot_from_row_0', 'pmax_not_pad'):
        assert {k[0] for k in caught} >= {"case 1 C 64", "case 2 C 128", "pad-row bound"} and all(res[k] for k in res if k[0] == "case 2 C 128")
    if slip in ('wrong_col_blocks', 'row_not_mod_256'):
        assert caught == {k for k in res if k[2] == 1 and k[0] in ("case 2 C 128", "case 4 C 64", "extra 2", "extra 3")}          # blocked, > 256 rows


# ---- the entry points -----------------------------------------------------------------------------------------------------------------------
def test_every_producer_entry_point_is_called_by_the_gpu_file():
    names = ['cham_h2_scale_absmax', 'cham_h2_scale_rownorm', 'cham_h2_scale_rownorm2', 'cham_split2h', 'cham_split3', 'cham_combine_fwd_p3',
             'cham_combine_fwd_h2', 'cham_combine_fwd_h2b', 'cham_h2b_block_elements']
    exported = re.findall(r'extern "C" int (cham_\w+)\s*\(', _src("gemm_h2.hip") + _src("gemm_p3.hip") + _src("scorer.hip"))
    assert all(n in exported for n in names)
    text = open(os.path.join(ROOT, "tests", "test_plane_producers_gpu.py")).read()
    missing = [n for n in names if not re.search(r"\blib\.%s\(" % n, text)]
    assert not missing, "entry points tests/test_plane_producers_gpu.py does not call: %s" % missing
