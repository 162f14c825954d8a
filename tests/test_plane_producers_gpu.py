"""The kernels that WRITE the fp16 / bf16 planes and their scale records, bit for bit against tests/plane_reference.py, at the sizes the
training step reaches:

    cham_h2_scale_absmax                      every grid-stride pass of the capped grid (512 workgroups: a second pass above 524 288 elements)
    cham_h2_scale_rownorm, _rownorm2          K == 128: the four-rows-in-flight loop (R > 3 x 8192 under the cap of 1024 workgroups), each of its
                                              slots, its tail loop, both half-waves; the generic row loop
    cham_split2h, cham_split3                 a wrap of the grid loop (cap 8192 workgroups: above 2 097 152 elements), strided and one-sided
                                              destinations inside NaN frames
    cham_combine_fwd_p3, _h2, _h2b            every slot table of tests/features_reference.py (pads, masked clicks), row-major and tile-blocked
    cham_h2b_block_elements                   the block pitch of the tile-blocked index restated in the reference

The maximum is PLANTED (one element, one row) and moved through the branches; the expected record has no rounding freedom, so every comparison
is exact - there is no tolerance in this file.  The assertions are functions of tests/plane_reference.py; tests/test_plane_reference_cpu.py
runs the same functions on host emulations that carry one slip each.

Found by this file: k_split2h stored h = +0, l = -0 for x = -0 (the product folded into the fp16 convert with a +0 addend) where
h = fp16(x s) is -0; fixed in the kernel.  The planted -0 of the split cases keeps it."""
import numpy as np
import pytest
import torch

from tests import features_reference as F
from tests import plane_reference as PR

pytestmark = pytest.mark.gpu
ERR = -22


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _rec(gpu):
    return torch.zeros(8, dtype=torch.int32, device=gpu)


def _words(rec):
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(np.uint32)


def _ok(failures, what):
    assert not failures, "%s: %s" % (what, "; ".join(failures))


def _frame(gpu, total, fill):
    return torch.full((total,), int(np.array(fill, np.uint16).view(np.int16)), dtype=torch.int16, device=gpu)


def _bits(buf):
    torch.cuda.synchronize()
    return buf.cpu().numpy().view(np.uint16)


def _at(buf, elements):
    return buf.data_ptr() + 2 * elements


# ---- scale records ---------------------------------------------------------------------------------------------------------------------------
def test_the_restated_caps_put_the_cases_in_their_branches():
    """no launch: the sizes of this file against the caps restated in tests/plane_reference.py (512 / 1024 / 8192 workgroups)"""
    assert PR.ABSMAX_PASS == 524288 and PR.ROWNORM_STRIDE == 8192 and PR.SPLIT_PASS == 2097152
    assert PR.ROWNORM_R == (1, 7, 8, 9, 8184, 8185, 24576, 24577, 32773, 65539)
    assert max(R * C for R, C in PR.SPLIT_SHAPES) > PR.SPLIT_PASS
    assert max(c[1] for c in PR.absmax_cases() if not isinstance(c[1], str)) > 3 * PR.ABSMAX_PASS


@pytest.mark.parametrize("case", PR.absmax_cases(), ids=lambda c: c[0])
def test_absmax_record_is_exact(gpu, case):
    lib = _lib_()
    x0, x1 = PR.absmax_inputs(case)
    want = PR.absmax_bound(x0, x1)
    d0, d1 = _dev(gpu, x0), (None if x1 is None else _dev(gpu, x1))
    rec = _rec(gpu)
    for rep in range(2):                                     # the second launch finds the scratch the first one left
        assert lib.cham_h2_scale_absmax(d0.data_ptr(), x0.size, None if d1 is None else d1.data_ptr(), 0 if x1 is None else x1.size,
                                        rec.data_ptr(), _st()) == 0
        w = _words(rec)
        print("    %-24s bound %r scale %r inv %r" % (case[0], w[2:3].view(np.float32)[0], w[0:1].view(np.float32)[0], w[1:2].view(np.float32)[0]))
        _ok(PR.record_failures(w, want), "%s, launch %d" % (case[0], rep))
    if case[0] in ('zeros', 'negative_zeros', 'overflow_sum'):
        assert list(_words(rec)[:2].view(np.float32)) == [1.0, 1.0]
        assert _words(rec)[2] == (0x7F800000 if case[0] == 'overflow_sum' else 0)


def _rownorm_check(lib, gpu, X, R, K, ld, factor, rec, plain, rec1, sq, what, base=None):
    """rownorm2 with a factor and a plain record, rownorm without: three records, each exact"""
    p = X.data_ptr() if base is None else base
    fac = None if factor is None else float(factor.cpu()[0])
    want, want_plain = PR.rownorm_bounds(sq, K, fac)
    assert lib.cham_h2_scale_rownorm2(p, R, K, ld, None if factor is None else factor.data_ptr(), rec.data_ptr(), plain.data_ptr(), _st()) == 0
    assert lib.cham_h2_scale_rownorm(p, R, K, ld, None, rec1.data_ptr(), _st()) == 0
    _ok(PR.record_failures(_words(rec), want), what + " (factor %r)" % fac)
    _ok(PR.record_failures(_words(plain), want_plain), what + " (rec_plain)")
    _ok(PR.record_failures(_words(rec1), want_plain), what + " (cham_h2_scale_rownorm, no factor)")
    assert np.array_equal(_words(plain)[:3], _words(rec1)[:3]), "rec_plain differs from the factor-free record"
    return want_plain


@pytest.mark.parametrize("R", PR.ROWNORM_R)
def test_rownorm_k128_record_is_exact(gpu, R):
    """The planted row in the first and the last row and in an even and an odd row of every in-flight slot and of the tail loop; spread over
    the 32 lanes, then confined to the first and to the last lane; ld 128 and 136 (NaN pad columns)."""
    lib = _lib_()
    K = 128
    factors = [None, _dev(gpu, np.array([2.0 ** -3], np.float32)), _dev(gpu, np.array([2.0 ** 5], np.float32))]
    rec, plain, rec1 = _rec(gpu), _rec(gpu), _rec(gpu)
    paths = PR.rownorm_paths(R)
    seen = set()
    for ld in PR.ROWNORM_LD:
        Xh = PR.rownorm_background(R, K, ld, seed=R + ld)
        sq0 = PR.rownorm_row_sq(Xh, K)
        assert sq0.max() <= K
        X = _dev(gpu, Xh)
        n = 0
        for row in PR.rownorm_placements(R, K):
            for vname, cols in PR.rownorm_variants(K):
                amp = 2.0 ** (n % 3)
                prow = PR.planted_row(K, cols, amp, flip=n)
                keep = X[row, :K].clone()
                X[row, :K] = _dev(gpu, prow)
                sq = sq0.copy()
                sq[row] = PR.rownorm_row_sq(prow[None], K)[0]
                got = _rownorm_check(lib, gpu, X, R, K, ld, factors[n % 3], rec, plain, rec1, sq,
                                     "R %d ld %d row %d (path %d) %s" % (R, ld, row, paths[row], vname))
                assert got == np.float32(32 * amp) * PR.MARGIN
                X[row, :K] = keep
                seen.add(int(paths[row]))
                n += 1
    print("    R %d: %d placements, loop paths %s" % (R, n, sorted(seen)))
    assert seen == set(int(p) for p in np.unique(paths))
    assert seen == ({-1} if R <= 3 * PR.ROWNORM_STRIDE else {0, 1, 2, 3, -1})          # (R = 3 x 8192 + 1: the unrolled loop holds rows 0, 8192, ... only)


@pytest.mark.parametrize("K", PR.GENERIC_K)
def test_rownorm_generic_record_is_exact(gpu, K):
    """K != 128: a wave per row; ld > K with NaN pad columns and a base that is aligned to 4 bytes only; one pass and three"""
    lib = _lib_()
    factor = _dev(gpu, np.array([2.0 ** -7], np.float32))
    rec, plain, rec1 = _rec(gpu), _rec(gpu), _rec(gpu)
    for R in PR.GENERIC_R:
        for ld in (K, K + 3):
            Xh = PR.rownorm_background(R, K, ld, seed=R + K)
            sq0 = PR.rownorm_row_sq(Xh, K)
            buf = torch.full((R * ld + 1,), float('nan'), device=gpu)
            X = buf[1:].view(R, ld)                          # base 4 bytes behind a 16-byte boundary
            X.copy_(_dev(gpu, Xh))
            assert X.data_ptr() % 16 == 4
            for n, row in enumerate(PR.rownorm_placements(R, K)):
                prow = PR.planted_row(K, None, 2.0 ** (n % 2), flip=n)
                keep = X[row, :K].clone()
                X[row, :K] = _dev(gpu, prow)
                sq = sq0.copy()
                sq[row] = PR.rownorm_row_sq(prow[None], K)[0]
                _rownorm_check(lib, gpu, X, R, K, ld, factor if n % 2 else None, rec, plain, rec1, sq, "K %d R %d ld %d row %d" % (K, R, ld, row))
                X[row, :K] = keep


def test_rownorm_empty_matrix_and_argument_errors(gpu):
    lib = _lib_()
    X = torch.ones(8, 128, device=gpu)
    rec = _rec(gpu)
    assert lib.cham_h2_scale_rownorm(X.data_ptr(), 0, 128, 128, None, rec.data_ptr(), _st()) == 0
    w = _words(rec)
    _ok(PR.record_failures(w, 0.0), "R = 0")
    assert list(w[:3].view(np.float32)) == [1.0, 1.0, 0.0]
    assert lib.cham_h2_scale_rownorm(X.data_ptr(), 8, 128, 130, None, rec.data_ptr(), _st()) == ERR          # K == 128: ld % 4
    assert lib.cham_h2_scale_rownorm(X.data_ptr() + 4, 7, 128, 128, None, rec.data_ptr(), _st()) == ERR      # K == 128: 16-byte base
    assert lib.cham_h2_scale_rownorm(X.data_ptr(), 8, 128, 64, None, rec.data_ptr(), _st()) == ERR           # ld < K
    assert lib.cham_h2_scale_rownorm2(X.data_ptr(), 8, 128, 128, None, rec.data_ptr(), rec.data_ptr(), _st()) == ERR
    assert lib.cham_h2_scale_absmax(X.data_ptr(), 6, None, 0, rec.data_ptr(), _st()) == ERR                  # n % 4
    assert lib.cham_h2_scale_absmax(X.data_ptr() + 4, 8, None, 0, rec.data_ptr(), _st()) == ERR
    assert np.array_equal(_words(rec), w)


@pytest.mark.parametrize("K,R,ld", [(128, 3 * PR.ROWNORM_STRIDE + 1, 128), (128, 4 * PR.ROWNORM_STRIDE + 5, 136), (264, PR.GENERIC_R[1], 267)])
def test_rownorm_record_scales_with_the_input(gpu, K, R, ld):
    """The same matrix x 2^40 and x 2^-40: the record scaled accordingly (squares of 2^90 and 2^-70: no hidden overflow or underflow).
    Beyond that range nothing is asserted; what the device gives at x 2^60 (squares overflow) and x 2^-70 (squares underflow) is printed."""
    lib = _lib_()
    Xh = PR.rownorm_background(R, K, ld, seed=K)
    row = PR.rownorm_placements(R, K)[-2]
    Xh[row, :K] = PR.planted_row(K)
    sq = PR.rownorm_row_sq(Xh, K)
    X = _dev(gpu, Xh)
    rec, plain, rec1 = _rec(gpu), _rec(gpu), _rec(gpu)
    factor = _dev(gpu, np.array([0.25], np.float32))
    for e in (0, 40, -40):
        Xs = X * 2.0 ** e
        got = _rownorm_check(lib, gpu, Xs, R, K, ld, factor, rec, plain, rec1, sq * 4.0 ** e, "x 2^%d" % e)
        assert got == np.float32(32 * 2.0 ** e) * PR.MARGIN
    for e in (60, -70):
        Xs = X * 2.0 ** e
        assert lib.cham_h2_scale_rownorm(Xs.data_ptr(), R, K, ld, None, rec1.data_ptr(), _st()) == 0
        print("    x 2^%d (outside the asserted range): scale, inv, bound = %s" % (e, list(_words(rec1)[:3].view(np.float32))))
        rec1.zero_()


def test_one_record_reused_across_kernels_and_grid_sizes(gpu):
    """absmax on 1 workgroup, absmax on the capped grid, rownorm on its capped grid, absmax again: one record, every result exact"""
    lib = _lib_()
    rec = _rec(gpu)
    small = np.array([0.5, -3.25, 1.0, 0.0], np.float32)
    big = PR.absmax_background(2 * PR.ABSMAX_PASS + 8, 9).copy()
    big[PR.ABSMAX_PASS + 5] = -PR.A_MAG
    assert PR.absmax_blocks(small.size) == 1 and PR.absmax_blocks(big.size) == PR.ABSMAX_CAP
    R = 4 * PR.ROWNORM_STRIDE + 5
    assert PR.rownorm_blocks(R, 128) == PR.ROWNORM_CAP
    Xh = PR.rownorm_background(R, 128, 128, seed=1)
    Xh[R - 3] = PR.planted_row(128)
    d_small, d_big, d_X = _dev(gpu, small), _dev(gpu, big), _dev(gpu, Xh)
    for rep in range(2):
        assert lib.cham_h2_scale_absmax(d_small.data_ptr(), 4, None, 0, rec.data_ptr(), _st()) == 0
        _ok(PR.record_failures(_words(rec), PR.absmax_bound(small)), "absmax, 1 workgroup")
        assert lib.cham_h2_scale_absmax(d_big.data_ptr(), big.size, d_small.data_ptr(), 4, rec.data_ptr(), _st()) == 0
        _ok(PR.record_failures(_words(rec), PR.absmax_bound(big, small)), "absmax, capped grid")
        assert lib.cham_h2_scale_rownorm(d_X.data_ptr(), R, 128, 128, None, rec.data_ptr(), _st()) == 0
        _ok(PR.record_failures(_words(rec), PR.rownorm_bounds(PR.rownorm_row_sq(Xh, 128), 128)[0]), "rownorm, capped grid")
        assert lib.cham_h2_scale_absmax(d_small.data_ptr(), 4, None, 0, rec.data_ptr(), _st()) == 0
        _ok(PR.record_failures(_words(rec), PR.absmax_bound(small)), "absmax again")


# ---- cham_split2h / cham_split3 ------------------------------------------------------------------------------------------------------------
def _split_call(lib, arm, src, R, Cc, lay, buf, rec, recompute):
    n = 2 if arm == 'h2' else 3
    dst = _at(buf, lay['off']) if lay['which'] != 'dstT' else None
    dstT = _at(buf, lay['offT']) if lay['which'] != 'dst' else None
    if arm == 'h2':
        return lib.cham_split2h(src.data_ptr(), R, Cc, lay['ld'], dst, lay['ps'], lay['ldd'], dstT, lay['psT'], lay['lddT'], rec.data_ptr(), recompute, _st())
    assert n == 3
    return lib.cham_split3(src.data_ptr(), R, Cc, lay['ld'], dst, lay['ps'], lay['ldd'], dstT, lay['psT'], lay['lddT'], _st())


@pytest.mark.parametrize("layout", PR.SPLIT_LAYOUTS, ids=lambda l: l[0])
@pytest.mark.parametrize("shape", PR.SPLIT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_split2h_planes_are_the_host_split(gpu, shape, layout):
    lib = _lib_()
    R, Cc = shape
    lay = PR.split_layout(R, Cc, layout, 2)
    recompute = lay['recompute']
    if recompute and lay['ld'] != Cc:
        pytest.fail("a recompute layout has no source pad")
    mode = 'absmax' if (recompute or R == 1) else 'rownorm'
    X, bound, scale = PR.split_inputs(R, Cc, mode)
    src = _dev(gpu, PR.split_source(X, lay['ld']))
    rec = _rec(gpu)
    buf = _frame(gpu, lay['total'], PR.FILL_F16)
    if recompute and (R * Cc) % 4:
        # the scale pass reads float4: refused, nothing written
        assert _split_call(lib, 'h2', src, R, Cc, lay, buf, rec, 1) == ERR
        assert (_bits(buf) == PR.FILL_F16).all() and not _words(rec).any()
        return
    if not recompute:
        # the record comes from its own kernel, as the model fills Ws1's from the row norms (a one-row matrix: from max |x|)
        if mode == 'rownorm':
            assert lib.cham_h2_scale_rownorm(src.data_ptr(), R, Cc, lay['ld'], None, rec.data_ptr(), _st()) == 0
        else:
            assert lib.cham_h2_scale_absmax(src.data_ptr(), Cc, None, 0, rec.data_ptr(), _st()) == 0
        _ok(PR.record_failures(_words(rec), bound), "record before the split")
    outs = []
    for rep in range(2):
        buf = _frame(gpu, lay['total'], PR.FILL_F16)
        assert _split_call(lib, 'h2', src, R, Cc, lay, buf, rec, recompute) == 0
        outs.append(_bits(buf))
    _ok(PR.record_failures(_words(rec), bound), "record after the split")
    assert np.array_equal(outs[0], outs[1]), "two launches differ"
    planes = PR.split2h_planes(X, scale)
    _ok(PR.buffer_failures(outs[0], PR.split_expected(planes, R, Cc, lay, PR.FILL_F16), "%dx%d %s" % (R, Cc, layout[0])), "planes and frame")
    # the consumers' contract, on the device's own planes (dst, or dstT transposed back)
    if lay['which'] != 'dstT':
        o = lay['off']
        got = [outs[0][o + q * lay['ps']:o + q * lay['ps'] + R * lay['ldd']].reshape(R, lay['ldd'])[:, :Cc] for q in range(2)]
    else:
        o = lay['offT']
        got = [outs[0][o + q * lay['psT']:o + q * lay['psT'] + Cc * lay['lddT']].reshape(Cc, lay['lddT'])[:, :R].T for q in range(2)]
    _ok(PR.h2_property_failures(got[0], got[1], X, scale), "h2 contract")
    k = min(len(PR.SPLIT2H_PLANTS), R * Cc - (Cc if mode == 'rownorm' else 1))
    hp = np.ascontiguousarray(got[0]).reshape(-1)[(Cc if mode == 'rownorm' else 1):][:k]
    assert hp[0] == 0x0001 and hp[1] == 0x8000, "underflowing values: h bits %s" % [hex(int(v)) for v in hp[:2]]


def test_split2h_argument_errors_write_nothing(gpu):
    lib = _lib_()
    R, Cc = 300, 264
    X, bound, scale = PR.split_inputs(R, Cc, 'absmax')
    lay = PR.split_layout(R, Cc, ('padded', 3, 5, 3, 24, 'both', 1), 2)
    src = _dev(gpu, PR.split_source(X, lay['ld']))
    rec = _rec(gpu)
    buf = _frame(gpu, lay['total'], PR.FILL_F16)
    assert _split_call(lib, 'h2', src, R, Cc, lay, buf, rec, 1) == ERR                                     # recompute = 1 with ld != Cc
    assert lib.cham_split2h(src.data_ptr(), R, Cc, Cc, None, 0, 0, None, 0, 0, rec.data_ptr(), 1, _st()) == ERR
    assert lib.cham_split2h(src.data_ptr(), 0, Cc, Cc, _at(buf, 64), R * Cc, Cc, None, 0, 0, rec.data_ptr(), 1, _st()) == ERR
    assert lib.cham_split2h(src.data_ptr(), R, Cc, Cc, _at(buf, 64), R * Cc, Cc, None, 0, 0, None, 1, _st()) == ERR
    assert lib.cham_split3(src.data_ptr(), R, Cc, Cc, None, 0, 0, None, 0, 0, _st()) == ERR
    assert lib.cham_split3(None, R, Cc, Cc, _at(buf, 64), R * Cc, Cc, None, 0, 0, _st()) == ERR
    assert (_bits(buf) == PR.FILL_F16).all() and not _words(rec).any()


@pytest.mark.parametrize("layout", PR.SPLIT_LAYOUTS, ids=lambda l: l[0])
@pytest.mark.parametrize("shape", PR.SPLIT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_split3_planes_are_the_host_split(gpu, shape, layout):
    lib = _lib_()
    R, Cc = shape
    lay = PR.split_layout(R, Cc, layout, 3)
    X, _, _ = PR.split_inputs(R, Cc, 'p3')
    src = _dev(gpu, PR.split_source(X, lay['ld']))
    outs = []
    for rep in range(2):
        buf = _frame(gpu, lay['total'], PR.FILL_BF16)
        assert _split_call(lib, 'p3', src, R, Cc, lay, buf, None, 0) == 0
        outs.append(_bits(buf))
    assert np.array_equal(outs[0], outs[1]), "two launches differ"
    planes = PR.split3_planes(X)
    _ok(PR.buffer_failures(outs[0], PR.split_expected(planes, R, Cc, lay, PR.FILL_BF16), "%dx%d %s" % (R, Cc, layout[0])), "planes and frame")


# ---- cham_combine_fwd_p3 / _h2 / _h2b --------------------------------------------------------------------------------------------------------
def _combine_all_arms(gpu, inp, what):
    """The four producers on one input: three bf16 planes; two fp16 planes through _h2, through _h2b row-major and - C % 32 == 0 - through
    _h2b tile-blocked, under the record cham_h2_scale_absmax(U, all rows of V) leaves (as nar/candidate_rows.py calls it).  Every destination
    is compared whole: planes, the gaps between them (ps > the plane), the frame, and the rows of the last row tile beyond the matrix."""
    lib = _lib_()
    BT, N, pmax, C = inp['BT'], inp['N'], inp['pmax'], inp['C']
    rows = BT * (N + 1)
    blk = lib.cham_h2b_block_elements()
    assert blk >= 256 * 32 and blk % 8 == 0
    U, V = _dev(gpu, inp['U']), _dev(gpu, inp['V'])
    slot = _dev(gpu, inp['slot'] if inp['slot'].size else np.zeros(1, np.int32))
    assert inp['V'].shape[0] == 2 * BT + pmax + 1
    rec = _rec(gpu)
    assert lib.cham_h2_scale_absmax(U.data_ptr(), U.numel(), V.data_ptr(), V.numel(), rec.data_ptr(), _st()) == 0
    w = _words(rec).copy()
    _ok(PR.record_failures(w, PR.absmax_bound(inp['U'].reshape(-1), inp['V'].reshape(-1))), what + ": record")
    scale = float(w[:1].view(np.float32)[0])
    z = PR.combine_rows(inp)
    got_h2 = None
    arms = [('p3', 0), ('h2', 0), ('h2b', 0)] + ([('h2b', 1)] if C % 32 == 0 else [])
    for arm, blocked in arms:
        npl, fill = (3, PR.FILL_BF16) if arm == 'p3' else (2, PR.FILL_F16)
        lay = PR.combine_layout(rows, C, npl, blocked, blk)
        outs = []
        for rep in range(2):
            buf = _frame(gpu, lay['total'], fill)
            args = (U.data_ptr(), V.data_ptr(), C, BT, N, pmax, slot.data_ptr(), _at(buf, lay['off']), lay['ps'])
            if arm == 'p3':
                rc = lib.cham_combine_fwd_p3(*args, _st())
            elif arm == 'h2':
                rc = lib.cham_combine_fwd_h2(*args, rec.data_ptr(), _st())
            else:
                rc = lib.cham_combine_fwd_h2b(*args, rec.data_ptr(), blocked, _st())
            assert rc == 0, (what, arm, blocked, rc)
            outs.append(_bits(buf))
        assert np.array_equal(outs[0], outs[1]), "%s %s: two launches differ" % (what, arm)
        planes = PR.combine_planes(inp, arm, scale)
        _ok(PR.buffer_failures(outs[0], PR.combine_expected(planes, rows, C, lay, blocked, blk, fill), "%s %s blocked %d" % (what, arm, blocked)), "planes")
        if arm == 'h2' and rows:
            o = lay['off']
            got_h2 = [outs[0][o + q * lay['ps']:o + q * lay['ps'] + rows * C].reshape(rows, C) for q in range(2)]
            _ok(PR.h2_property_failures(got_h2[0], got_h2[1], z, scale, exact_sum=False), what + ": h2 contract")
    assert np.array_equal(_words(rec), w), "a producer wrote the record"
    return z, got_h2, scale


@pytest.mark.parametrize("C", F.COMBINE_C)
@pytest.mark.parametrize("case", range(len(F.SLOT_CASES)))
def test_combine_planes_are_the_split_of_the_exact_rows(gpu, case, C):
    inp = F.combine_inputs(case, C)
    if case:
        s = inp['slot']
        assert (s == -1).any() and (s == inp['pmax']).any()          # the pad row is read: by a masked click and by a pad slot
    _combine_all_arms(gpu, inp, "case %d C %d" % (case, C))


@pytest.mark.parametrize("i", range(len(PR.COMBINE_EXTRA)))
def test_combine_planes_at_the_row_tile_edges(gpu, i):
    """N = 0; exactly 256 candidate rows; 257; a 256-row tile boundary inside a position's candidates"""
    inp = PR.combine_extra_inputs(i)
    rows = inp['BT'] * (inp['N'] + 1)
    assert rows == (6, 256, 257, 303)[i]
    _combine_all_arms(gpu, inp, "BT %d N %d" % (inp['BT'], inp['N']))


def test_combine_bound_set_by_the_pad_row_keeps_every_sign(gpu):
    """One element of V's pad row is 2^20 and sets the bound; every other z is 0 or +-2^-45 of it and underflows under the scale: the h plane
    holds 0x0001 exactly where z > 0 and +-0 elsewhere, and the large element itself arrives through the masked click and the pad slots."""
    inp = PR.combine_pad_large_inputs()
    z, (h, l), scale = _combine_all_arms(gpu, inp, "pad-row bound")
    assert scale == 2.0 ** -6                                            # bound 2^20 (+ 2^-26, rounded away) -> 2^20 x 2^-6 = 2^14
    small = np.abs(z) < 1
    assert (z[small] > 0).sum() > 100 and (z[small] < 0).sum() > 100 and (~small).sum() >= inp['N'] + 1
    assert (h[small & (z > 0)] == 0x0001).all() and (h[small & (z < 0)] == 0x8000).all() and (h[small & (z == 0)] & 0x7FFF == 0).all()
    assert (h[~small] == np.float16(2.0 ** 14).view(np.uint16)).all() and not l[~small].any()


def test_combine_argument_errors_write_nothing(gpu):
    lib = _lib_()
    inp = F.combine_inputs(1, 64)
    BT, N, pmax, C = inp['BT'], inp['N'], inp['pmax'], 64
    rows = BT * (N + 1)
    blk = lib.cham_h2b_block_elements()
    U, V, slot = _dev(gpu, inp['U']), _dev(gpu, inp['V']), _dev(gpu, inp['slot'])
    rec = _rec(gpu)
    assert lib.cham_h2_scale_absmax(U.data_ptr(), U.numel(), V.data_ptr(), V.numel(), rec.data_ptr(), _st()) == 0
    lay = PR.combine_layout(rows, C, 3, 1, blk)
    buf = _frame(gpu, lay['total'], PR.FILL_F16)
    z, ps = _at(buf, lay['off']), lay['ps']
    u, v, s, r = U.data_ptr(), V.data_ptr(), slot.data_ptr(), rec.data_ptr()
    p3 = lambda u=u, v=v, C=C, BT=BT, N=N, s=s, z=z, ps=ps: lib.cham_combine_fwd_p3(u, v, C, BT, N, pmax, s, z, ps, _st())
    h2 = lambda u=u, v=v, C=C, BT=BT, N=N, s=s, z=z, ps=ps, r=r: lib.cham_combine_fwd_h2(u, v, C, BT, N, pmax, s, z, ps, r, _st())
    h2b = lambda C=C, BT=BT, N=N, z=z, ps=ps, r=r, b=1: lib.cham_combine_fwd_h2b(u, v, C, BT, N, pmax, s, z, ps, r, b, _st())
    for f in (p3, h2):
        assert f(u=None) == ERR and f(v=None) == ERR and f(s=None) == ERR and f(z=None) == ERR and f(C=62) == ERR and f(C=0) == ERR
        assert f(BT=-1) == ERR and f(N=-1) == ERR and f(ps=ps + 2) == ERR
        assert f(BT=0) == 0                                              # nothing to do: OK, nothing written
    assert h2(r=None) == ERR and h2b(r=None) == ERR and h2b(b=0, BT=0) == 0 and h2b(BT=0) == 0
    assert h2b(C=48) == ERR                                              # blocked: C % 32
    assert h2b(ps=(rows + 255) // 256 * (C // 32) * blk - 4) == ERR      # blocked: a plane stride below whole row tiles
    assert (_bits(buf) == PR.FILL_F16).all()
