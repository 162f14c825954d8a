"""Host models, case tables and assertions of the plane producers (the kernels that WRITE the fp16 / bf16 planes and their scale records)
for tests/test_plane_producers_gpu.py and tests/test_plane_reference_cpu.py.  numpy only: neither torch nor the library is imported here.

    k_h2_scale_absmax, k_h2_scale_rownorm     csrc/gemm_h2.hip     the 32-byte H2Scale record {scale, 1 / scale, bound, -, scratch x 3, -}
    k_split2h, k_split3                       csrc/gemm_h2.hip, csrc/gemm_p3.hip
    k_combine_fwd_cand_p3, _h2                csrc/scorer.hip      (row-major and tile-blocked planes)

Everything is compared BIT FOR BIT; no tolerance appears in this file or in the two test files.

The planted maximum.  A maximum that skips an element is wrong only when the skipped element holds the maximum, so every case PLANTS the
maximum in one known place - an element (absmax) or a row (rownorm) - above a background that cannot reach it, and moves the place through
every branch of the kernel: each grid-stride pass, each of the four in-flight slots of the unrolled row loop, its tail loop, both
half-waves.  The expected record has no rounding freedom:
    absmax    bound = max |x0| + max |x1|, one fp32 addition of two fp32 values, formed here in fp32;
    rownorm   the background is {-1, 0, 1} and the planted row holds m = 64 (16, 4, 1 where K is smaller or the columns are confined)
              entries +-32 / sqrt(m) (x a power of two): every fp32 sum of squares is an exact integer whatever its order, the planted one
              is 1024 (a perfect square), sqrt = 32, x (1 + 2^-10) and x a power-of-two factor are exact.

Each model takes **slip: one wrong thing a kernel could do (SLIPS).  tests/test_plane_reference_cpu.py runs the assertions below on the
slipped models and shows that every slip fails one - which is the argument that the GPU file would see the same mistake in a kernel.

The grid caps are restated here (ABSMAX_CAP, ROWNORM_CAP, SPLIT_CAP; the CPU file pins them to the source lines); every size below is
derived from them, so the cases stay in their branches if a cap doubles.
"""
import functools

import numpy as np

from tests import features_reference as F
from tests import gemm_reference as G

f32, f64 = np.float32, np.float64

# cham_h2_scale_absmax  (csrc/gemm_h2.hip): "blocks = blocks < 1 ? 1 : (blocks > 512 ? 512 : blocks)", 256 float4 lanes per workgroup
ABSMAX_CAP = 512
# cham_h2_scale_rownorm2 (csrc/gemm_h2.hip): "blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks)", 8 rows (K == 128) or 4 per workgroup
ROWNORM_CAP = 1024
# cham_split2h (csrc/gemm_h2.hip), cham_split3 (csrc/gemm_p3.hip): "if (blocks > 8192) blocks = 8192", 256 elements per workgroup
SPLIT_CAP = 8192
ABSMAX_PASS = ABSMAX_CAP * 256 * 4          # elements of one grid-stride pass of the capped grid: 524 288
ROWNORM_STRIDE = ROWNORM_CAP * 8            # rows of one pass of the capped grid, K == 128: 8192
SPLIT_PASS = SPLIT_CAP * 256                # 2 097 152
MARGIN = f32(1.0009765625)                  # 1 + 2^-10 (k_h2_scale_rownorm)
ROOT_NORM = 32.0                            # the planted row's norm (x its power-of-two amplitude)
FILL_F16, FILL_BF16 = 0x7E00, 0x7FC0        # NaN in either format: the frame of every destination
FRONT = 64                                  # elements of frame in front of and behind a destination

SLIPS = ('skip_u3', 'drop_tail', 'drop_unrolled', 'drop_second_pass', 'ignore_x1', 'max_for_sum', 'exponent_off_by_one', 'scratch_armed', 'no_margin',
         'half_reduce_16', 'no_keep_sign', 'l_unscaled', 'pad_slot_from_row_0', 'pmax_not_pad', 'wrong_col_blocks', 'row_not_mod_256',
         'transposed_with_ldd')


def bits16(x):
    return np.ascontiguousarray(x).view(np.uint16)


def bits32(x):
    return np.ascontiguousarray(x, dtype=f32).view(np.uint32)


def word32(x):
    """the bit pattern of one fp32 value"""
    return int(bits32(x).reshape(-1)[0])


# ---- the record ---------------------------------------------------------------------------------------------------------------------------
def record_words(bound, **slip):
    """h2_finish_scale + the cleared scratch: the eight 32-bit words a scale kernel leaves in a (zero-initialised) record."""
    b = f32(bound)
    s = G.h2_scale(b)
    if slip.get('exponent_off_by_one') and b > 0 and np.isfinite(b):
        s *= 2.0
    w = np.zeros(8, np.uint32)
    w[:3] = np.array([s, 1.0 / s, b], f32).view(np.uint32)
    if slip.get('scratch_armed'):
        w[4], w[5] = word32(b), 1
    return w


def record_clamped(bound):
    """the exponent 15 - e left [-110, 110]: scale and 1 / scale stay normal numbers and bound x scale is NOT in [2^14, 2^15)"""
    b = f32(bound)
    return bool(b > 0 and np.isfinite(b) and abs(15 - int(np.frexp(b)[1])) > 110)


def record_failures(words, bound):
    """The assertions on a record.  words: 8 uint32 as read back; bound: the expected fp32 value, compared by its bits (the device's sqrtf
    of a perfect square is exact: the row-norm records need no allowance)."""
    words = np.asarray(words, np.uint32)
    got = words[:3].view(f32)
    b = f32(bound)
    bad = []
    if word32(got[2]) != word32(b):
        bad.append("bound %r (0x%08x), expected %r (0x%08x)" % (got[2], words[2], b, word32(b)))
    s = G.h2_scale(b)
    want = np.array([s, 1.0 / s], f32)
    if words[0] != want.view(np.uint32)[0] or words[1] != want.view(np.uint32)[1]:
        bad.append("scale, inv = %r, %r, expected %r, %r" % (got[0], got[1], want[0], want[1]))
    if b > 0 and np.isfinite(b) and not record_clamped(b) and not 2.0 ** 14 <= f64(got[2]) * f64(got[0]) < 2.0 ** 15:
        bad.append("bound x scale = %r outside [2^14, 2^15)" % (f64(got[2]) * f64(got[0])))
    if words[4:7].any():
        bad.append("scratch words 4-6 left at %s" % [hex(int(v)) for v in words[4:7]])
    return bad


# ---- cham_h2_scale_absmax -----------------------------------------------------------------------------------------------------------------
def absmax_blocks(n0, n1=0):
    n = max(n0, n1)
    return min(max((n // 4 + 255) // 256, 1), ABSMAX_CAP)


def _absmax_one(x, stride4, slip):
    cnt = x.size // 4
    if slip.get('drop_second_pass'):
        cnt = min(cnt, stride4)
    return f32(np.fmax.reduce(np.abs(x[:4 * cnt]), initial=f32(0)))          # fmaxf: a NaN operand is ignored


def absmax_bound(x0, x1=None, **slip):
    stride4 = absmax_blocks(x0.size, 0 if x1 is None else x1.size) * 256
    a = _absmax_one(x0, stride4, slip)
    b = f32(0) if x1 is None or slip.get('ignore_x1') else _absmax_one(x1, stride4, slip)
    with np.errstate(over='ignore'):
        return f32(max(a, b)) if slip.get('max_for_sum') else f32(a + b)


@functools.lru_cache(maxsize=None)
def absmax_background(n, seed):
    x = np.random.default_rng(7000 + seed).uniform(-1, 1, n).astype(f32)
    x.setflags(write=False)
    return x


A_MAG, B_MAG = f32(2.7182817), f32(3.1415927)      # planted magnitudes: their fp32 sums with the background's maximum round


def absmax_cases():
    """(name, n0, n1, plants): plants = [(array 0 / 1, element, value)] written over the U(-1, 1) background; n1 == 0: x1 = NULL.
    'kind' cases (n0 is a string) are built by absmax_inputs from scratch."""
    P = ABSMAX_PASS
    big = 3 * P + 4 * 77
    cs = []
    for n in (4, 1024, P, P + 4, big):
        cs += [("n%d_first" % n, n, 0, [(0, 0, A_MAG)]), ("n%d_last_negative" % n, n, 0, [(0, n - 1, -B_MAG)])]
    cs += [("pass1_last_float4", big, 0, [(0, P - 2, -A_MAG)]), ("pass2_first_float4", big, 0, [(0, P + 1, B_MAG)]),
           ("pass3_first_float4", big, 0, [(0, 2 * P + 3, -A_MAG)]), ("pass2_only_float4", P + 4, 0, [(0, P, B_MAG)]),
           ("x1_only_longer", 1024, P + 4, [(1, P + 2, -B_MAG)]), ("x1_only_longer_pass3", 1024, big, [(1, 2 * P + 1, A_MAG)]),
           ("x1_only_shorter", P + 4, 1024, [(1, 1000, A_MAG)]), ("x0_pass2_x1_short", P + 4, 1024, [(0, P + 3, A_MAG), (1, 3, -B_MAG)]),
           ("equal_in_both", big, P + 4, [(0, 2 * P, B_MAG), (1, P + 1, -B_MAG)])]
    for kind in ('zeros', 'negative_zeros', 'subnormal', 'clamp_large', 'clamp_small', 'overflow_sum', 'nans'):
        cs.append((kind, kind, 0, []))
    for k in (-20, 0, 15):
        cs += [("pow2_%d" % k, 'one', 0, [(0, 5, f32(2.0 ** k))]), ("below_pow2_%d" % k, 'one', 0, [(0, 6, -np.nextafter(f32(2.0 ** k), f32(0)))])]
    return cs


def absmax_inputs(case):
    """-> (x0, x1 or None), writable copies"""
    name, n0, n1, plants = case
    x1 = None
    if isinstance(n0, str):
        x0 = np.zeros(1024, f32)
        if n0 == 'negative_zeros':
            x0[:] = f32(-0.0)
        elif n0 == 'subnormal':
            x0[7], x0[900] = f32(2.0 ** -140), f32(-2.0 ** -141)
        elif n0 == 'clamp_large':
            x0[1023] = f32(-2.0 ** 127)
        elif n0 == 'clamp_small':
            x0[3] = f32(2.0 ** -120)                        # a normal number: 15 - e = 134 > 110
        elif n0 == 'overflow_sum':
            x0[11] = f32(1.5 * 2.0 ** 127)
            x1 = np.zeros(8, f32)
            x1[4] = f32(-1.5 * 2.0 ** 127)
        elif n0 == 'nans':
            x0 = absmax_background(ABSMAX_PASS + 1024, 3).copy()
            x0[[0, 1, 500, 501, 503, ABSMAX_PASS + 1, x0.size - 1]] = np.nan
            x0[502] = -A_MAG                                 # the maximum shares its float4 with three NaNs
            x1 = np.full(8, np.nan, f32)
            x1[5] = f32(0.5)
    else:
        x0 = absmax_background(n0, 1).copy()
        x1 = absmax_background(n1, 2).copy() if n1 else None
    for which, i, v in plants:
        (x0, x1)[which][i] = v
    return x0, x1


# ---- cham_h2_scale_rownorm / _rownorm2 ---------------------------------------------------------------------------------------------------------
ROWNORM_R = (1, 7, 8, 9, ROWNORM_STRIDE - 8, ROWNORM_STRIDE - 7, 3 * ROWNORM_STRIDE, 3 * ROWNORM_STRIDE + 1, 4 * ROWNORM_STRIDE + 5,
             8 * ROWNORM_STRIDE + 3)                          # 1, 7, 8, 9, 8184, 8185, 24 576, 24 577, 32 773, 65 539
ROWNORM_LD = (128, 136)
GENERIC_K = (1, 63, 64, 65, 100, 264)
GENERIC_R = (5, 2 * ROWNORM_CAP * 4 + 3)                      # one pass; a third pass of the capped grid (4 rows per workgroup): 8195


def rownorm_blocks(R, K):
    per = 8 if K == 128 else 4
    return min(max((R + per - 1) // per, 1), ROWNORM_CAP)


def rownorm_paths(R):
    """K == 128: which loop reads row r - 0..3: in-flight slot u of the unrolled loop; -1: the tail loop.  A half-wave starts at
    r0 = 2 wave + half and walks r0 + j stride; the unrolled loop takes four rows while r + 3 stride < R."""
    stride = 8 * rownorm_blocks(R, 128)
    r = np.arange(R, dtype=np.int64)
    r0, j = r % stride, r // stride
    cnt = (R - r0 + stride - 1) // stride
    return np.where(j < cnt // 4 * 4, j % 4, -1)


def rownorm_row_sq(X, K, **slip):
    """fp32 sum of squares of every row's first K columns (exact for this file's inputs: integers x a power of two).  half_reduce_16: the
    K == 128 half-wave reduction stops at 16 lanes, so a lane sees only its 64-column half and the maximum is over the halves."""
    Xd = np.asarray(X)[:, :K].astype(f64)
    if slip.get('half_reduce_16') and K == 128:
        return np.maximum((Xd[:, :64] ** 2).sum(1), (Xd[:, 64:] ** 2).sum(1))
    return (Xd ** 2).sum(1)


def rownorm_bounds(sq, K, factor=None, **slip):
    """sq: rownorm_row_sq.  -> (bound of rec, bound of rec_plain): sqrtf(max) x factor x (1 + 2^-10), left to right in fp32."""
    sq = np.asarray(sq, f64)
    keep = np.ones(sq.size, bool)
    if K == 128 and sq.size:
        paths = rownorm_paths(sq.size)
        if slip.get('skip_u3'):
            keep &= paths != 3
        if slip.get('drop_tail'):
            keep &= paths != -1
        if slip.get('drop_unrolled'):                          # the unrolled loop advances r and folds nothing in
            keep &= paths < 0
    with np.errstate(over='ignore'):
        m = f32(sq[keep].max()) if keep.any() else f32(0)
        root = np.sqrt(m, dtype=f32)
        margin = f32(1) if slip.get('no_margin') else MARGIN
        return f32(f32(root * f32(1 if factor is None else factor)) * margin), f32(root * margin)


def rownorm_background(R, K, ld, seed=0):
    """{-1, 0, 1} in the K columns, NaN in the pad columns"""
    X = np.full((R, ld), np.nan, f32)
    X[:, :K] = np.random.default_rng(7100 + seed).integers(-1, 2, (R, K), dtype=np.int8)
    return X


def planted_row(K, cols=None, amp=1.0, flip=0):
    """m entries +- amp 32 / sqrt(m), m the largest of 64, 16, 4, 1 that fits: sum of squares 1024 amp^2, norm 32 amp.  cols: the columns
    the non-zeros are confined to (default: spread over the row - K == 128: two per lane of the half-wave)."""
    cols = np.arange(K) if cols is None else np.asarray(cols)
    m = max(v for v in (64, 16, 4, 1) if v <= cols.size)
    pick = cols[np.arange(m) * (cols.size // m)]
    row = np.zeros(K, f32)
    row[pick] = f32(amp * ROOT_NORM / np.sqrt(m)) * np.where((np.arange(m) + flip) % 3 == 0, -1, 1).astype(f32)
    return row


def rownorm_placements(R, K):
    """rows the planted row goes to: first, last and - K == 128 - the first even and the first odd row (the two half-waves of a wave) of
    each in-flight slot of the unrolled loop and of the tail loop; generic: the middle and a row of the second pass."""
    rows = {0, R - 1}
    if K == 128:
        paths = rownorm_paths(R)
        r = np.arange(R)
        for p in (0, 1, 2, 3, -1):
            for parity in (0, 1):
                hit = r[(paths == p) & (r % 2 == parity)]
                if hit.size:
                    rows.add(int(hit[hit.size // 3]))
    else:
        rows |= {R // 2} | ({4 * ROWNORM_CAP + 1} if 4 * ROWNORM_CAP + 1 < R else set())
    return sorted(rows)


def rownorm_variants(K):
    """(name, columns of the planted row) - the confined forms catch a half-wave reduction that loses its first or last lane"""
    if K != 128:
        return [('spread', None)]
    return [('spread', None), ('cols_0_3', np.arange(0, 4)), ('cols_124_127', np.arange(124, 128))]


# ---- cham_split2h / cham_split3 -------------------------------------------------------------------------------------------------------------
SPLIT_SHAPES = ((1, 4), (300, 264), (2049, 1025))            # 2049 x 1025 > SPLIT_PASS: the grid loop wraps
# (name, source pad columns, ldd - Cc, lddT - R, plane stride - plane, destinations, recompute)
SPLIT_LAYOUTS = (('tight', 0, 0, 0, 0, 'both', 1), ('padded', 3, 5, 3, 24, 'both', 0), ('dst_only', 0, 5, 0, 40, 'dst', 0),
                 ('dstT_only', 3, 0, 7, 8, 'dstT', 0), ('dst_recompute', 0, 6, 0, 16, 'dst', 1), ('dstT_tight', 0, 0, 0, 0, 'dstT', 0))
# x scale of the planted values: +-0; underflow in both signs (h = 0x0001, 0x8000); below, at and above half the smallest fp16 subnormal;
# fp16 subnormals; ties of the h rounding (spacing 2 in [2048, 4096)); ties of the l rounding (residual 0.25 + 2^-13: spacing 2^-12)
SPLIT2H_PLANTS = (2.0 ** -30, -2.0 ** -30, -0.0, 0.0, 2.0 ** -26, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, 3 * 2.0 ** -24, -(2.0 ** -15 + 2.0 ** -24),
                  2.0 ** -14 - 2.0 ** -24, 2049.0, 2051.0, -2049.0, -2051.0, 1024.25 + 2.0 ** -13, 1024.25 + 3 * 2.0 ** -13, -(1024.25 + 2.0 ** -13),
                  2.0 ** -3, 2.0 ** -3 - 2.0 ** -27)
# ties of the three bf16 roundings: h (1 + 2^-8 down, 1 + 3 2^-8 up), m (residual 2^-10 + 2^-18), and values with a full 24-bit significand
SPLIT3_PLANTS = (0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), 1 + 2.0 ** -10 + 2.0 ** -18, 1 + 2.0 ** -10 + 3 * 2.0 ** -18,
                 1 + 2.0 ** -23, -(2 - 2.0 ** -23), 3.0e38, -1.0e-30)


@functools.lru_cache(maxsize=8)
def split_inputs(R, Cc, mode):
    """-> (X [R, Cc] fp32, expected bound of the record, scale).  mode 'absmax' (recompute = 1, or a one-row matrix): element 0 = 7.5 is
    the bound; 'rownorm' (recompute = 0, the record of cham_h2_scale_rownorm as the model takes Ws1's): row 0 is one element -64, the
    largest row norm, bound 64 (1 + 2^-10); 'p3': no scale.  Gaussian values clipped to +-6, the planted values from the second element
    (absmax, p3) or the second row (rownorm) on."""
    X = np.clip(np.random.default_rng(7200 + R + Cc).standard_normal((R, Cc)), -6, 6).astype(f32)
    if mode != 'p3':
        # two fp16 planes hold 11 + 11 significand bits: h + l == x scale can be asserted EXACTLY only of values of at most 22 (an fp32 value
        # has 24), so the low two bits of every Gaussian value are cleared; the bit-for-bit comparison does not need this, the combine tests
        # keep all 24 bits
        X = (X.view(np.uint32) & np.uint32(0xFFFFFFFC)).view(f32)
    if mode == 'p3':
        bound, scale, plants, start = None, 1.0, SPLIT3_PLANTS, 1
    elif mode == 'absmax':
        X.flat[0] = 7.5
        bound, plants, start = f32(7.5), SPLIT2H_PLANTS, 1
    else:
        assert R > 1
        X[0] = 0
        X[0, Cc // 2] = -64.0
        bound, plants, start = f32(f32(64.0) * MARGIN), SPLIT2H_PLANTS, Cc
    if mode != 'p3':
        scale = G.h2_scale(bound)
    k = min(len(plants), R * Cc - start)
    X.flat[start:start + k] = np.array(plants[:k], f64) / scale
    X.setflags(write=False)
    return X, bound, scale


def split2h_planes(X, scale, **slip):
    """[h bits, l bits] (uint16) of the two fp16 planes.  l_unscaled: the residual taken from x instead of x scale."""
    h, l = G.split2h(X, scale, keep_sign=not slip.get('no_keep_sign'))
    if slip.get('l_unscaled'):
        with np.errstate(over='ignore'):
            l = (np.asarray(X, f32) - h.astype(f32)).astype(np.float16)
    return [bits16(h), bits16(l)]


def split3_planes(X):
    return [G.bf16_bits(p) for p in G.split3(X)]


def h2_property_failures(hb, lb, X, scale, exact_sum=True):
    """What the consumers rely on: h + l == x scale exactly while l is a normal number, |h| <= 2^15, (int16) h > 0 <=> x > 0.  The sum is
    asserted (exact_sum) of the values of at most 22 significand bits - all of split_inputs' but the planted ties of the l rounding, which
    round by construction."""
    h, l = np.asarray(hb, np.uint16).view(np.float16).astype(f64), np.asarray(lb, np.uint16).view(np.float16).astype(f64)
    xs = np.asarray(X, f64) * scale
    big = (np.abs(xs) >= 2.0 ** -3) & (bits32(X).reshape(np.shape(X)) & 3 == 0)
    bad = []
    if exact_sum and not np.array_equal((h + l)[big], xs[big]):
        bad.append("h + l != x scale at %d elements" % np.count_nonzero((h + l)[big] != xs[big]))
    if not np.abs(h).max() <= 2.0 ** 15:
        bad.append("max |h| = %r" % np.abs(h).max())
    if not np.array_equal(np.asarray(hb, np.uint16).view(np.int16) > 0, np.asarray(X) > 0):
        bad.append("(int16) h > 0 differs from x > 0 at %d elements" % np.count_nonzero((np.asarray(hb, np.uint16).view(np.int16) > 0) != (np.asarray(X) > 0)))
    return bad


def split_layout(R, Cc, layout, nplanes):
    """-> dict(ld, ldd, lddT, ps, psT, off, offT, total): one flat 16-bit buffer [frame | dst planes | frame | dstT planes | frame]"""
    name, spad, dpad, tpad, gap, which, recompute = layout
    ldd, lddT = Cc + dpad, R + tpad
    ps, psT = R * ldd + gap, Cc * lddT + gap
    off = FRONT
    offT = off + (nplanes * ps if which != 'dstT' else 0) + FRONT
    total = offT + (nplanes * psT if which != 'dst' else 0) + FRONT
    return dict(ld=Cc + spad, ldd=ldd, lddT=lddT, ps=ps, psT=psT, off=off, offT=offT, total=total, which=which, recompute=recompute)


def split_source(X, ld):
    """the source with ld - Cc pad columns of NaN"""
    S = np.full((X.shape[0], ld), np.nan, f32)
    S[:, :X.shape[1]] = X
    return S


def split_expected(planes, R, Cc, lay, fill, **slip):
    """The whole destination buffer: the frame value everywhere but the planes' own elements."""
    buf = np.full(lay['total'], fill, np.uint16)
    r, c = np.arange(R, dtype=np.int64)[:, None], np.arange(Cc, dtype=np.int64)[None, :]
    for q, p in enumerate(planes):
        if lay['which'] != 'dstT':
            buf[lay['off'] + q * lay['ps'] + r * lay['ldd'] + c] = p
        if lay['which'] != 'dst':
            buf[lay['offT'] + q * lay['psT'] + c * (lay['ldd'] if slip.get('transposed_with_ldd') else lay['lddT']) + r] = p
    return buf


def buffer_failures(got, want, what=""):
    got, want = np.asarray(got, np.uint16), np.asarray(want, np.uint16)
    if got.shape == want.shape and np.array_equal(got, want):
        return []
    d = np.flatnonzero(got != want) if got.shape == want.shape else np.array([-1])
    first = ", ".join("[%d] 0x%04x for 0x%04x" % (i, got[i], want[i]) for i in d[:6]) if d[0] >= 0 else "shapes %s, %s" % (got.shape, want.shape)
    return ["%s: %d of %d elements differ: %s" % (what, d.size, want.size, first)]


# ---- cham_combine_fwd_p3 / _h2 / _h2b -----------------------------------------------------------------------------------------------------------
# (BT, N, pmax): N = 0; exactly 256 rows; 257 rows; a 256-row tile boundary inside position 2's candidates (rows 202 .. 302)
COMBINE_EXTRA = ((6, 0, 10), (32, 7, 40), (257, 0, 12), (3, 100, 300))
COMBINE_EXTRA_C = 64
PAD_LARGE = f32(2.0 ** 20)


def combine_extra_inputs(i):
    BT, N, pmax = COMBINE_EXTRA[i]
    rng = np.random.default_rng(7300 + i)
    slot = np.zeros((BT, 0), np.int32)
    if N:
        slot, _ = F.make_slots(rng, BT, N, pmax, 0.3, 1, 0.2)
        slot[BT // 2] = -1
        slot[0, N - 1] = pmax
    C = COMBINE_EXTRA_C
    U = rng.standard_normal((BT, C)).astype(f32)
    V = rng.standard_normal((2 * BT + pmax + 1, C)).astype(f32)
    U[:, :4], V[:, :4] = f32(0.0), f32(-0.0)
    return dict(BT=BT, N=N, pmax=pmax, slot=slot, U=U, V=V, C=C)


def combine_pad_large_inputs():
    """One large element in V's pad row only; it sets the bound.  Everything else is +-2^-26 or 0, so z = u + v is 0, +-2^-26 or +-2^-25 =
    2^-45 of the bound: x scale underflows (2^-31 and below) and only h2_keep_sign keeps x > 0 visible in the h plane."""
    BT, N, pmax, C = 9, 11, 30, 64
    rng = np.random.default_rng(7400)
    slot, _ = F.make_slots(rng, BT, N, pmax, 0.3, 1, 0.0)
    slot[4] = -1
    slot[0, N - 1] = pmax
    t = f32(2.0 ** -26)
    U = rng.integers(-1, 2, (BT, C)).astype(f32) * t
    V = rng.integers(-1, 2, (2 * BT + pmax + 1, C)).astype(f32) * t
    V[2 * BT + pmax] = 0
    V[2 * BT + pmax, 33] = PAD_LARGE
    U[:, 33] = 0
    return dict(BT=BT, N=N, pmax=pmax, slot=slot, U=U, V=V, C=C)


def combine_rows(inp, **slip):
    """the exact fp32 candidate rows [BT (1 + N), C]"""
    slot, pmax = inp['slot'], inp['pmax']
    if slip.get('pmax_not_pad'):
        slot = np.where(slot == pmax, pmax - 1, slot)          # a V of 2 BT + pmax rows: the pad slot clamped to the last pool slot
    kw = {'masked_slot_to_row_0': True} if slip.get('pad_slot_from_row_0') else {}
    z = F.combine_fwd(inp['U'], inp['V'], slot, inp['BT'], inp['N'], pmax, dtype=f32, **kw)
    assert z.dtype == f32
    return z[inp['BT']:]


def combine_planes(inp, arm, scale=None, **slip):
    z = combine_rows(inp, **slip)
    return split3_planes(z) if arm == 'p3' else split2h_planes(z, scale, **slip)


def h2b_index(row, col, col_blocks, blk, **slip):
    """Tile-blocked plane (csrc/common.h, "TILE-BLOCKED plane layout"): [row tiles of 256][column blocks of 32][256 rows][32 columns], one
    (256 x 32) block every `blk` = cham_h2b_block_elements() elements."""
    row, col = np.asarray(row, np.int64), np.asarray(col, np.int64)
    ncb = col_blocks + 1 if slip.get('wrong_col_blocks') else col_blocks
    rr = row if slip.get('row_not_mod_256') else row % 256
    return ((row // 256) * ncb + col // 32) * blk + rr * 32 + col % 32


def combine_layout(rows, C, nplanes, blocked, blk):
    """-> dict(ps, off, total): [frame | planes, ps apart, ps > the plane | frame].  Blocked: whole row tiles, as the header demands."""
    plane = (rows + 255) // 256 * (C // 32) * blk if blocked else rows * C
    ps = plane + 8
    return dict(ps=ps, off=FRONT, total=FRONT + nplanes * ps + FRONT, plane=plane)


def combine_expected(planes, rows, C, lay, blocked, blk, fill, **slip):
    buf = np.full(lay['total'], fill, np.uint16)
    r, c = np.arange(rows, dtype=np.int64)[:, None], np.arange(C, dtype=np.int64)[None, :]
    idx = h2b_index(r, c, C // 32, blk, **slip) if blocked else r * C + c
    for q, p in enumerate(planes):
        buf[lay['off'] + q * lay['ps'] + idx] = p
    return buf
