"""Float64 reference, fp32-CPU twin and case table of the GEMM family (csrc/gemm.hip, gemm_x3.hip, gemm_b16.hip, gemm_p3.hip, gemm_h2.hip)
for tests/test_gemm_views_gpu.py and tests/test_gemm_reference_cpu.py.  numpy only: neither torch nor the library is imported here.

A `Problem` is one call: the arm (entry point), the form (NN / NT / TN), M, N, K, the epilogue and one `View` per operand.  A `View` places an
operand inside a larger parent buffer: leading dimension larger than the width, base at a column offset, planes further apart than
rows x ld.  Input parents hold a finite poison outside the view (POISON, POISON_F16 for fp16 planes: a kernel may load a pad column
and discard it, so it must not be NaN, but USING one moves an element by ~1e3 of the data's scale); output parents are NaN everywhere
(the interior holds C0 under accumulate), with a frame of FRONT elements in front, the pad columns of every row and GUARD_ROWS whole rows
behind row M.

reference(p) -> (ref, S), float64.  The operands are the STORED values:
    f32                 A (x rowscale) and B as float64
    bf16                bf16(fp32(A x rowscale)), bf16(B)                  (round to nearest even, as the staging does)
    b16, b16_dma        the bf16 values as stored
    f32x3               split3(fp32(A x rowscale)), split3(B): three bf16 planes h, m, l each, SIX products
                            h h,  h m,  m h,  h l,  l h,  m m                 (the head comments of csrc/gemm_x3.hip and csrc/gemm_p3.hip)
    p3                  the three stored bf16 planes, the same six products
    f32x2h              split2h(fp32(A x rowscale) x scale_a), split2h(B x scale_b): two fp16 planes h, l each, THREE products
                            h h,  h l,  l h                                   (include/chameleon_nar.h, cham_gemm_h2)
    h2, h2b, h2_dgrad_gs  the two stored fp16 planes, the same three products
and ref = (float64 sum over k of exactly those plane products) / (scale_a scale_b), then the epilogue of include/chameleon_nar.h: + bias,
leaky (alpha 0.2) or tanh, x act'(dref) from the SAVED OUTPUT (leaky': y > 0 ? 1 : 0.2; tanh': 1 - y^2), (+)= C0.  Every plane product is
exact in fp32, so all that separates a kernel from ref is its fp32 summation order (and one rounding of a bf16 output).  S is the same
expression with |.| in place of every term (+ |bias|, x |act'|, + |C0|): the element's own error scale.

twin(p, **slip) is the fp32 evaluation the bounds come from: the same products in float32, added one k after the other (K rank-1 updates -
not np.dot, whose order is unknown), the K-splits of the entry point's plan added in ascending order, the same epilogue in float32, stored
into a NaN-filled output parent through the view.  It reads the operands out of the poisoned parents by index arithmetic, so that every
slip of SLIPS (a leading dimension used as a width, a K tail that takes the pad columns, ...) does what the slipped kernel would do.
judge(p, parent) -> (frame intact?, max_ij (|got - ref| - bf16 allowance) / S_ij) is shared by the CPU and the GPU test; a case's bound is
8 x the twin's ratio (tests/test_gemm_reference_cpu.py prints the table); a bf16 output is allowed 2^-8 |ref| on top of it (one
round-to-nearest-even rounding; truncation reaches 2^-7).
"""
import functools
import itertools
import zlib
from dataclasses import dataclass, replace

import numpy as np

LEAKY = 0.2
ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2
POISON = 1024.0            # bf16-exact; the data are N(0, 1)
POISON_F16 = 49152.0       # fp16 planes hold |x| scale < 2^15; finite in fp16 (< 65 504)
FRONT = 64                 # elements of frame in front of an output view (on top of its column offset)
GUARD_ROWS = 256           # whole rows of frame behind row M
MARGIN = 8.0
BF16_OUT = 2.0 ** -8       # one round-to-nearest-even rounding of a bf16 output, relative to |ref|
P3_PRODUCTS = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))       # (plane of A, plane of B); smallest terms first, as gemm_x3.hip adds them
H2_PRODUCTS = ((1, 0), (0, 0), (0, 1))                                 # gemm_h2.hip's pass order

F32_ARMS = ('f32', 'bf16', 'f32x3', 'f32x2h')                         # fp32 storage
B16_ARMS = ('b16', 'b16_dma')                                         # one bf16 array per operand
P3_ARMS = ('p3',)                                                     # three bf16 planes in memory
H2_ARMS = ('h2', 'h2b', 'h2_dgrad_gs')                                # two fp16 planes in memory
ENTRY = {'f32': 'cham_gemm_f32', 'bf16': 'cham_gemm_bf16', 'f32x3': 'cham_gemm_f32x3', 'f32x2h': 'cham_gemm_f32x2h', 'b16': 'cham_gemm_b16',
         'p3': 'cham_gemm_p3', 'b16_dma': 'cham_gemm_b16_dma', 'h2': 'cham_gemm_h2', 'h2b': 'cham_gemm_h2b', 'h2_dgrad_gs': 'cham_gemm_h2_dgrad_gs'}


# ---- number formats (the models tests/test_split3_cpu.py and tests/test_split2h_cpu.py check) --------------------------------------------
def bf16_rne(x):
    """float32 -> nearest bf16 (ties to even), returned as float32 (what v_cvt_pk_bf16_f32 does for finite inputs)."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = u + 0x7FFF + ((u >> 16) & 1)
    return ((r >> 16) << 16).astype(np.uint32).view(np.float32)


def bf16_trunc(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_bits(x):
    return (np.asarray(x, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def split3(a):
    a = np.asarray(a, np.float32)
    h = bf16_rne(a)
    r = (a - h).astype(np.float32)          # exact in fp32 (Sterbenz-like: |r| <= 2^-8 |a|, fits 16 bits of significand)
    m = bf16_rne(r)
    r2 = (r - m).astype(np.float32)
    return h, m, bf16_rne(r2)


def h2_scale(bound):
    """h2_finish_scale: bound = m 2^e (0.5 <= m < 1) -> scale = 2^(15 - e), so that bound * scale lies in [2^14, 2^15)."""
    if not (bound > 0 and np.isfinite(bound)):
        return 1.0
    _, e = np.frexp(np.float32(bound))
    k = int(np.clip(15 - int(e), -110, 110))
    return float(np.ldexp(1.0, k))


def split2h(x, scale, keep_sign=True):
    """keep_sign: h2_keep_sign of the plane producers (a positive value never stores +0); the in-kernel split of cham_gemm_f32x2h has none."""
    xs = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float32)          # exact (power of two) unless it leaves the fp32 range
    with np.errstate(over='ignore'):
        h = xs.astype(np.float16)
    r = (xs - h.astype(np.float32)).astype(np.float32)                              # exact in fp32
    l = r.astype(np.float16)
    hb = h.view(np.uint16).copy()
    if keep_sign:
        hb[(np.asarray(x) > 0) & (hb == 0)] = 1
    return hb.view(np.float16), l


def _amax(x):
    return float(np.abs(x).max()) if x.size else 1.0


def h2_record(bound):
    s = h2_scale(bound)
    return np.array([s, 1.0 / s, bound, 0, 0, 0, 0, 0], np.float32)


# ---- views and problems -------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class View:
    """`planes` matrices [rows, cols] with row stride ld, `ps` elements apart (0: one plane), the first at element `col0` of the parent."""
    rows: int
    cols: int
    ld: int
    col0: int = 0
    planes: int = 1
    ps: int = 0

    def index(self, rows=None, cols=None, ld=None, ps=None, plane=0, base=0):
        rows, cols = self.rows if rows is None else rows, self.cols if cols is None else cols
        ld, ps = self.ld if ld is None else ld, self.ps if ps is None else ps
        return base + self.col0 + plane * ps + np.arange(rows, dtype=np.int64)[:, None] * ld + np.arange(cols, dtype=np.int64)[None, :]

    def in_elems(self):
        return self.col0 + (self.planes - 1) * self.ps + max(self.rows, 1) * self.ld

    def out_elems(self):
        return FRONT + self.col0 + (self.rows + GUARD_ROWS) * self.ld


@dataclass(frozen=True)
class Problem:
    name: str
    arm: str
    form: str                    # 'NN', 'NT', 'TN' (the plane arms: NT = tn 0, TN = tn 1)
    M: int
    N: int
    K: int
    A: View
    B: View
    C: View
    R: View = None               # dref (saved output [M, N]) when dact != 0
    RS: View = None              # rowscale when rs_div > 0
    bias: bool = False
    act: int = 0
    dact: int = 0
    rs_div: int = 0
    accumulate: int = 0
    hint: int = 1                # splits_hint
    out_bf16: bool = False
    a_blocked: bool = False      # cham_gemm_h2b / _dgrad_gs: A tile-blocked (no view on it)
    b_blocked: bool = False
    group_rows: int = 0          # cham_gemm_h2_dgrad_gs
    switch: tuple = None         # (setter, value): the tile switch the case forces
    counter: tuple = None        # (launch-count function, length, index) that must advance by one
    quiet: tuple = ()            # indices of the same counters that must NOT advance: the instances the case does not name
    expect: int = 0              # return code
    seed: int = 0

    @property
    def transA(self):
        return self.form == 'TN'

    @property
    def transB(self):
        return self.form == 'NT'

    @property
    def products(self):
        return P3_PRODUCTS if self.arm in ('f32x3', 'p3') else H2_PRODUCTS if self.arm in ('f32x2h',) + H2_ARMS else ((0, 0),)

    def ws_bytes(self):
        """Workspace the harness hands over: exactly hint x M x N x 4 where a split count is asked for, 8 slabs under the automatic choice."""
        return 0 if self.hint == 1 else (self.hint if self.hint > 1 else 8) * self.M * self.N * 4

    def plan(self):
        """(K-splits, k chunk) of the entry point's host-side plan; the GPU test pins the split count through the launch counters."""
        M, N, K, hint = self.M, self.N, self.K, self.hint
        cd = lambda a, b: -(-a // b)
        maxw = self.ws_bytes() // (M * N * 4)
        if self.arm in F32_ARMS:
            splits = 1
            if hint != 1 and N % 4 == 0 and self.form == 'TN':
                bm = (256 if M * N >= (1 << 20) else 128) if N > 64 else 256
                bn = 128 if N > 64 else 64 if N > 32 else 32
                tiles = cd(M, bm) * cd(N, bn)
                want = min(hint if hint > 1 else (1 if tiles >= 384 else cd(512, tiles)), cd(K, 256), maxw)
                splits = max(want, 1)
            kchunk = cd(cd(K, splits), 64) * 64 or 64
            return max(cd(K, kchunk), 1), kchunk
        if self.arm == 'b16':
            splits = 1
            if hint != 1 and self.form == 'TN':
                tiles = cd(M, 256) * cd(N, 128 if N > 64 else 64 if N > 32 else 32)
                want = min(hint if hint > 1 else (1 if tiles >= 384 else cd(512, tiles)), cd(K, 512), maxw)
                want = want // 8 * 8 if want >= 8 else want
                splits = max(want, 1)
            kchunk = cd(cd(K, splits), 32) * 32
            return cd(K, kchunk), kchunk
        if self.form != 'TN':
            return 1, K
        per, step = (1536, 48) if self.arm == 'b16_dma' else (512, 16)
        splits = 1
        if hint != 1:
            tiles = cd(M, 256) * cd(N, 256)
            want = min(hint if hint > 1 else (1 if tiles >= 192 else cd(256, tiles)), cd(K, per), maxw)
            want = want // 8 * 8 if (hint <= 0 and want >= 8) else want
            splits = max(want, 1)
        kchunk = cd(cd(K, splits), step) * step
        return cd(K, kchunk), kchunk


def _fill_view(parent, v, planes_data):
    for q, X in enumerate(planes_data):
        parent[v.index(plane=q)] = X


@functools.lru_cache(maxsize=None)
def data(p):
    """The call's buffers.  Logical values: A / B as stored ([rows, cols] of the view; plane arms: a tuple of planes), bias, Y (dref), rs, C0;
    parents: flat arrays in the storage type (uint16 bits for bf16, float16 for fp16 planes), poisoned / NaN-framed."""
    rng = np.random.default_rng(1000 + p.seed)
    d = {}
    nrm = lambda *s: rng.standard_normal(s).astype(np.float32)
    A, B = nrm(p.A.rows, p.A.cols), nrm(p.B.rows, p.B.cols)
    d['rec_a'] = d['rec_b'] = None
    if p.rs_div:
        d['rs'] = nrm(p.RS.rows, p.RS.cols)
        d['rs_parent'] = np.full(p.RS.in_elems(), POISON, np.float32)
        _fill_view(d['rs_parent'], p.RS, [d['rs']])
    if p.arm in F32_ARMS:
        d['A'], d['B'] = (A,), (B,)
        pa, pb = np.full(p.A.in_elems(), POISON, np.float32), np.full(p.B.in_elems(), POISON, np.float32)
        if p.arm == 'f32x2h':
            As = A * d['rs'][np.arange(p.A.rows) // p.rs_div] if p.rs_div else A
            d['rec_a'], d['rec_b'] = h2_record(_amax(As)), h2_record(_amax(B))
    elif p.arm in B16_ARMS:
        d['A'], d['B'] = (bf16_rne(A),), (bf16_rne(B),)
        pa, pb = np.full(p.A.in_elems(), bf16_bits(POISON), np.uint16), np.full(p.B.in_elems(), bf16_bits(POISON), np.uint16)
    elif p.arm in P3_ARMS:
        d['A'], d['B'] = split3(A), split3(B)
        pa, pb = np.full(p.A.in_elems(), bf16_bits(POISON), np.uint16), np.full(p.B.in_elems(), bf16_bits(POISON), np.uint16)
    else:
        d['rec_a'], d['rec_b'] = h2_record(_amax(A)), h2_record(_amax(B))
        d['A'], d['B'] = split2h(A, d['rec_a'][0]), split2h(B, d['rec_b'][0])
        pa, pb = np.full(p.A.in_elems(), POISON_F16, np.float16), np.full(p.B.in_elems(), POISON_F16, np.float16)
    as_stored = (lambda X: bf16_bits(X)) if pa.dtype == np.uint16 else (lambda X: X)
    _fill_view(pa, p.A, [as_stored(X) for X in d['A']])
    _fill_view(pb, p.B, [as_stored(X) for X in d['B']])
    d['A_parent'], d['B_parent'] = pa, pb
    d['bias'] = nrm(p.N) if p.bias else None
    if p.dact:
        Y = np.tanh(nrm(p.M, p.N)) if p.dact == ACT_TANH else nrm(p.M, p.N)
        z = rng.random((p.M, p.N)) < 0.01                      # ~1 % exact zeros of either sign: leaky'(+-0) = 0.2, tanh'(0) = 1
        Y[z] = np.where(rng.random(int(z.sum())) < 0.5, np.float32(0.0), np.float32(-0.0))
        if p.arm in F32_ARMS:
            d['Y'] = Y
            d['R_parent'] = np.full(p.R.in_elems(), POISON, np.float32)
            _fill_view(d['R_parent'], p.R, [Y])
        elif p.arm in H2_ARMS:                                 # the fp16 h plane of the saved activation (sign kept by the producer)
            d['Y'] = split2h(Y, h2_scale(float(np.abs(Y).max())))[0]
            d['R_parent'] = np.full(p.R.in_elems(), POISON_F16, np.float16)
            _fill_view(d['R_parent'], p.R, [d['Y']])
        else:                                                  # bf16 activation / h plane of a three-plane one
            d['Y'] = bf16_rne(Y)
            d['R_parent'] = np.full(p.R.in_elems(), bf16_bits(POISON), np.uint16)
            _fill_view(d['R_parent'], p.R, [bf16_bits(d['Y'])])
    d['C0'] = nrm(p.M, p.N) if p.accumulate else None
    return d


def out_parent(p, d):
    """The output as the harness uploads it: NaN everywhere, C0 in the interior under accumulate (float32; a bf16 output is kept as float32
    values here and converted by the harness)."""
    c = np.full(p.C.out_elems(), np.nan, np.float32)
    if p.accumulate:
        c[p.C.index(base=FRONT)] = d['C0']
    return c


def _operand_planes(p, d, dt):
    """op(A) [M, K] and op(B) [K, N] per plane in precision dt, and 1 / (scale_a scale_b)."""
    A, B = [X.astype(dt) for X in d['A']], [X.astype(dt) for X in d['B']]
    inv = dt(1.0)
    if p.arm in F32_ARMS:
        a, b = A[0], B[0]
        if p.rs_div:
            a = a * d['rs'].astype(dt)[np.arange(p.A.rows) // p.rs_div]
        if p.arm != 'f32':                                     # the staging multiplies in fp32 and then rounds / splits
            a32 = d['A'][0] * d['rs'][np.arange(p.A.rows) // p.rs_div] if p.rs_div else d['A'][0]
            if p.arm == 'bf16':
                A, B = [bf16_rne(a32).astype(dt)], [bf16_rne(d['B'][0]).astype(dt)]
            elif p.arm == 'f32x3':
                A, B = [X.astype(dt) for X in split3(a32)], [X.astype(dt) for X in split3(d['B'][0])]
            else:
                sa, sb = d['rec_a'][0], d['rec_b'][0]
                A, B = [X.astype(dt) for X in split2h(a32, sa, keep_sign=False)], [X.astype(dt) for X in split2h(d['B'][0], sb, keep_sign=False)]
                inv = dt(d['rec_a'][1]) * dt(d['rec_b'][1])
        else:
            A, B = [a], [b]
    elif p.arm in H2_ARMS:
        inv = dt(d['rec_a'][1]) * dt(d['rec_b'][1])
    if p.transA:
        A = [X.T for X in A]
    if p.transB:
        B = [X.T for X in B]
    return A, B, inv


def _dact(Y, dact, dt, slip=()):
    Y = Y.astype(dt)
    if dact == ACT_LEAKY:
        return np.where((Y >= 0) if 'leaky_ge' in slip else (Y > 0), dt(1), dt(LEAKY))
    if 'tanh_from_pre' in slip:
        Y = np.tanh(Y)
    return dt(1) - Y * Y


@functools.lru_cache(maxsize=None)
def reference(p):
    d = data(p)
    A, B, inv = _operand_planes(p, d, np.float64)
    ref, S = np.zeros((p.M, p.N)), np.zeros((p.M, p.N))
    for qa, qb in p.products:
        ref += A[qa] @ B[qb]
        S += np.abs(A[qa]) @ np.abs(B[qb])
    ref, S = ref * inv, S * inv
    if p.bias:
        ref, S = ref + d['bias'], S + np.abs(d['bias'].astype(np.float64))
    if p.act == ACT_LEAKY:
        ref = np.where(ref > 0, ref, LEAKY * ref)
    elif p.act == ACT_TANH:
        ref = np.tanh(ref)
    if p.dact:
        g = _dact(d['Y'], p.dact, np.float64)          # |terms| of tanh' = 1 - y^2: 1 + y^2 (the fp32 subtraction cancels where |y| is near 1)
        ref, S = ref * g, S * (np.abs(g) if p.dact == ACT_LEAKY else 1.0 + d['Y'].astype(np.float64) ** 2)
    if p.accumulate:
        ref, S = ref + d['C0'], S + np.abs(d['C0'].astype(np.float64))
    ref.setflags(write=False), S.setflags(write=False)
    return ref, S


def group_sums(p, C):
    """cham_gemm_h2_dgrad_gs: per 128-row chunk q and k-th group of that chunk, the column sums of the chunk's rows of the group, at
    [(q * (127 // G + 2) + k)]; pieces no row falls into stay NaN."""
    G, gsk = p.group_rows, 127 // p.group_rows + 2
    out = np.full((2 * (-(-p.M // 256)) * gsk, p.N), np.nan, C.dtype)
    for q in range(-(-p.M // 128)):
        lo, hi = 128 * q, min(128 * q + 128, p.M)
        g0 = lo // G
        for g in range(g0, (hi - 1) // G + 1):
            r0, r1 = max(lo, g * G), min(hi, (g + 1) * G)
            acc = np.zeros(p.N, C.dtype)
            for r in range(r0, r1):
                acc = acc + C[r]
            out[q * gsk + (g - g0)] = acc
    return out


# ---- the fp32 twin, with slips -------------------------------------------------------------------------------------------------------------
SLIPS = ('lda_as_width', 'ldb_as_width', 'ldc_as_width', 'ldr_as_width', 'ldrs_as_width', 'k_tail_reads_pad', 'last_k_chunk_dropped', 'rs_mod',
         'bias_per_split', 'c0_dropped_splitk', 'c0_twice', 'leaky_ge', 'tanh_from_pre', 'bf16_out_truncated', 'h2_product_dropped',
         'p3_product_dropped', 'plane_stride_rows_x_width', 'rows_past_m_stored')


def applies(slip, p):
    if p.expect or p.K == 0:
        return False
    two, three = p.arm in ('f32x2h',) + H2_ARMS, p.arm in ('f32x3', 'p3')
    return {'lda_as_width': not p.a_blocked, 'ldb_as_width': not p.b_blocked, 'ldc_as_width': True, 'ldr_as_width': bool(p.dact),
            'ldrs_as_width': p.rs_div > 0, 'k_tail_reads_pad': p.form == 'NT' and p.K % 16 != 0, 'last_k_chunk_dropped': p.K > 16, 'rs_mod': p.rs_div > 0,
            'bias_per_split': p.bias and p.plan()[0] > 1, 'c0_dropped_splitk': p.accumulate and p.plan()[0] > 1, 'c0_twice': bool(p.accumulate),
            'leaky_ge': p.dact == ACT_LEAKY, 'tanh_from_pre': p.dact == ACT_TANH, 'bf16_out_truncated': p.out_bf16, 'h2_product_dropped': two,
            'p3_product_dropped': three, 'plane_stride_rows_x_width': p.arm in P3_ARMS + H2_ARMS and not p.a_blocked,
            'rows_past_m_stored': p.M % 32 != 0}[slip]


def _to_f32(parent, idx):
    x = parent[idx]
    return bf16_from_bits(x) if x.dtype == np.uint16 else x.astype(np.float32)


def twin(p, *slip):
    """-> the output parent (float32 values; NaN frame) as a kernel with the given slips would leave it."""
    d = data(p)
    f = np.float32
    K = p.K
    kpad = 0
    if 'k_tail_reads_pad' in slip:
        kpad = min(-(-K // 16) * 16, p.A.ld, p.B.ld) - K
    if 'last_k_chunk_dropped' in slip:
        K = (K - 1) // 16 * 16
    # operands out of the parents, as stored
    def load(v, parent, which):
        ld = v.cols if which + '_as_width' in slip else v.ld
        ps = v.rows * v.cols if ('plane_stride_rows_x_width' in slip and which == 'lda') else v.ps
        cols = v.cols + (kpad if p.form == 'NT' else 0)
        return [_to_f32(parent, v.index(ld=ld, ps=ps, plane=q, cols=cols)) for q in range(v.planes)]
    A = [X.astype(f) for X in d['A']] if p.a_blocked else load(p.A, d['A_parent'], 'lda')
    B = [X.astype(f) for X in d['B']] if p.b_blocked else load(p.B, d['B_parent'], 'ldb')
    inv = f(1)
    if p.arm in F32_ARMS:
        a = A[0]
        if p.rs_div:
            rs = _to_f32(d['rs_parent'], p.RS.index(ld=p.RS.cols if 'ldrs_as_width' in slip else None))
            r = np.arange(p.A.rows)
            a = a * rs[((r % p.rs_div) % p.RS.rows) if 'rs_mod' in slip else (r // p.rs_div)]
        if p.arm == 'bf16':
            A, B = [bf16_rne(a)], [bf16_rne(B[0])]
        elif p.arm == 'f32x3':
            A, B = list(split3(a)), list(split3(B[0]))
        elif p.arm == 'f32x2h':
            A = [X.astype(f) for X in split2h(a, d['rec_a'][0], keep_sign=False)]
            B = [X.astype(f) for X in split2h(B[0], d['rec_b'][0], keep_sign=False)]
        else:
            A = [a]
    if d['rec_a'] is not None:
        inv = f(d['rec_a'][1]) * f(d['rec_b'][1])
    if p.transA:
        A = [X.T for X in A]
    if p.transB:
        B = [X.T for X in B]
    products = list(p.products)
    if ('h2_product_dropped' in slip and len(products) == 3) or ('p3_product_dropped' in slip and len(products) == 6):
        # the smallest product that an fp32-grade bound can see: a_l b_h of two fp16 planes (2^-11 |a b|), a_m b_h of three bf16 planes (2^-8).
        # The three third-order products (a_l b_h, a_h b_l, a_m b_m: 2^-16 |a b| each, 2^-17 S in a sum) are of the size of the fp32
        # summation error itself - dropping one lands at 0.7-4 x the bound; whether the kept products approximate the fp32 product is the
        # subject of tests/test_split3_cpu.py and of the per-arm GPU tests, not of this comparison.
        drop = 0 if len(products) == 3 else 3
        products = products[:drop] + products[drop + 1:]
    splits, kchunk = p.plan()
    total, tmp = np.zeros((p.M, p.N), f), np.empty((p.M, p.N), f)
    with np.errstate(over='ignore', invalid='ignore'):
        for s in range(splits):
            acc = np.zeros((p.M, p.N), f)
            for k in range(s * kchunk, min(K + kpad, (s + 1) * kchunk) if s + 1 < splits else K + kpad):
                for qa, qb in products:
                    np.multiply(A[qa][:, k, None], B[qb][None, k, :], out=tmp)
                    acc += tmp
            total = acc if splits == 1 else total + acc
        v = total * inv if d['rec_a'] is not None else total
        if p.bias:
            v = v + d['bias'] * f(splits if 'bias_per_split' in slip else 1)
        if p.act == ACT_LEAKY:
            v = np.where(v > 0, v, f(LEAKY) * v)
        elif p.act == ACT_TANH:
            v = np.tanh(v)
        if p.dact:
            Y = _to_f32(d['R_parent'], p.R.index(ld=p.R.cols if 'ldr_as_width' in slip else None))
            v = v * _dact(Y, p.dact, f, slip)
        out = out_parent(p, d)
        if p.accumulate and not ('c0_dropped_splitk' in slip and splits > 1):
            v = v + d['C0'] * f(2 if 'c0_twice' in slip else 1)
        if p.out_bf16:
            v = bf16_trunc(v) if 'bf16_out_truncated' in slip else bf16_rne(v)
    rows = p.M
    if 'rows_past_m_stored' in slip:
        rows = -(-p.M // 32) * 32
        v = np.concatenate([v, np.zeros((rows - p.M, p.N), f)])
    out[p.C.index(rows=rows, ld=p.N if 'ldc_as_width' in slip else None, base=FRONT)] = v.astype(f)
    return out


def twin_values(p):
    """The twin's interior BEFORE a bf16 output rounding (the error the bound is taken from), float32."""
    q = replace(p, out_bf16=False) if p.out_bf16 else p
    return twin(q)[q.C.index(base=FRONT)]


def judge(p, parent, expect_c0=False):
    """parent: the downloaded output parent as float values.  -> (the frame still holds NaN everywhere, max_ij (|got - ref| - allowance) / S_ij)
    with allowance = 2^-8 |ref| for a bf16 output; an interior NaN counts as infinite."""
    parent = np.asarray(parent)
    idx = p.C.index(base=FRONT)
    frame = np.ones(parent.shape, bool)
    frame[idx] = False
    intact = bool(np.isnan(parent[frame]).all())
    ref, S = reference(p)
    got = parent[idx].astype(np.float64)
    err = np.abs(got - ref) - (BF16_OUT * np.abs(ref) if p.out_bf16 else 0.0)
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(np.isnan(got), np.inf, np.where(err > 0, err / S, 0.0))
    return intact, float(ratio.max())


@functools.lru_cache(maxsize=None)
def bound(p):
    """8 x the fp32-CPU twin's worst |twin - ref| / S over the case's elements."""
    ref, S = reference(p)
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(S > 0, np.abs(twin_values(p).astype(np.float64) - ref) / S, 0.0)
    return MARGIN * float(e.max())


# ---- the case table -------------------------------------------------------------------------------------------------------------------------
def _views(arm, form, M, N, K, ldc_pad=4, dact=0, rs_div=0, out_bf16=False, a_blocked=False, b_blocked=False, c_col0=None, r_col0=None):
    """The padding recipe: lda / ldb = width + 12 floats (fp32) or + 8 / + 24 elements (16-bit planes), base at a column offset of 4 floats /
    8 elements, planes rows x ld + 64 apart, ldc = N + ldc_pad, ldr = N + 12 (fp32) / N + 16 (16-bit): different from ldc, ldrs = width + 4."""
    ar, ac = (K, M) if form == 'TN' else (M, K)
    br, bc = (N, K) if form == 'NT' else (K, N)
    if arm in F32_ARMS:
        pads, off, planes = (12, 12), 4, 1
    else:
        pads, off, planes = (8, 24), 8, 3 if arm in P3_ARMS else 2 if arm in H2_ARMS else 1
    def v(r, c, pad, blocked):
        if blocked:
            return View(r, c, c, 0, planes, 0)
        ld = c + pad
        return View(r, c, ld, off, planes, (r * ld + 64) if planes > 1 else 0)
    out = dict(A=v(ar, ac, pads[0], a_blocked), B=v(br, bc, pads[1], b_blocked),
               C=View(M, N, N + ldc_pad, c_col0 if c_col0 is not None else 0 if ldc_pad % 4 else (8 if out_bf16 else 4)))
    if dact:
        out['R'] = View(M, N, N + (12 if arm in F32_ARMS else 16), off if r_col0 is None else r_col0)
    if rs_div:
        out['RS'] = View(-(-ar // rs_div), ac, ac + 4, off)
    return out


def _case(name, arm, form, M, N, K, ldc_pad=4, c_col0=None, r_col0=None, **kw):
    vw = _views(arm, form, M, N, K, ldc_pad, kw.get('dact', 0), kw.get('rs_div', 0), kw.get('out_bf16', False), kw.get('a_blocked', False),
                kw.get('b_blocked', False), c_col0, r_col0)
    return Problem(name=name, arm=arm, form=form, M=M, N=N, K=K, **vw, **kw)


def _f32_counter(arm, N, variant=None, small=False):
    if arm in ('f32', 'bf16'):
        i = 5 if small else ((1 if variant == 2 else 2 if variant == 4 else 0) if N > 64 else 3 if N > 32 else 4)
        return ('cham_gemm_launch_counts', 16, i + (8 if arm == 'bf16' else 0))
    if arm == 'f32x3':
        return ('cham_gemm_f32x3_launch_counts', 8, 3 if (N <= 64 or small) else (1 if variant == 2 else 0))
    return ('cham_gemm_f32x3_launch_counts', 8, 5 if variant == 2 else 4)


def _tn_matrix(ns, special):
    """The TN rows of a register-staged arm: K of 70 and 1100, unsplit (splits_hint 1) and splits_hint 0, 3 and 8, each with and without
    accumulate - 16 rows (N, K, hint, accumulate, extras), the column counts `ns` handed round so that each meets both K and both
    accumulate settings; `special` adds a view or epilogue detail to the row of a (K, hint, accumulate)."""
    rows = []
    for i, (K, hint, acc) in enumerate(itertools.product((70, 1100), (1, 0, 3, 8), (0, 1))):
        rows.append((ns[(i + i // 6) % len(ns)], K, hint, acc, special.get((K, hint, acc), {})))
    return rows


TN_SPECIAL = {(70, 1, 0): dict(ldc_pad=2), (1100, 3, 0): dict(ldc_pad=2), (1100, 3, 1): dict(ldc_pad=2), (1100, 0, 0): dict(rs_div=51), (1100, 8, 0): dict(bias=True),
              (70, 3, 1): dict(ldc_pad=8), (1100, 0, 1): dict(c_col0=1)}      # ldc % 4 != 0 unsplit and split; a C aligned to 4 bytes only


def _build_cases():
    cases = []
    def add(name, arm, form, M, N, K, **kw):
        kw.setdefault('seed', zlib.crc32(("%s-%s-%dx%dx%d-%s" % (arm, form, M, N, K, name)).encode()) % 100000)
        cases.append(_case("%s-%s-%dx%dx%d-%s" % (arm, form, M, N, K, name), arm, form, M, N, K, **kw))
    LK, TH = ACT_LEAKY, ACT_TANH
    # ---- register-staged arms with fp32 storage: M = 300 = one 256-row tile + 44 rows (two 128-row tiles + 44); every column instance full and ragged
    for arm in ('f32', 'bf16', 'f32x3'):
        ns = (260, 72, 64, 36, 32, 12) if arm != 'f32x3' else (260, 72, 64)          # (cham_gemm_f32x3 hands N <= 64 to cham_gemm_f32: one case)
        nn_epi = [dict(bias=True, act=LK, rs_div=51), dict(bias=True, act=TH), dict(bias=True), dict(), dict(bias=True, act=LK), dict(bias=True, act=TH, ldc_pad=8)]
        for i, N in enumerate(ns):
            add("nn%d" % i, arm, 'NN', 300, N, (100, 4)[i % 2], counter=_f32_counter(arm, N), **nn_epi[i])
        nt_epi = [dict(), dict(dact=LK), dict(dact=TH, accumulate=1), dict(accumulate=1), dict(dact=LK, ldc_pad=8), dict(dact=TH), dict(dact=LK)]
        for i, N in enumerate(ns + ((6,) if arm != 'f32x3' else ())):
            add("nt%d" % i, arm, 'NT', 300, N, (100, 4)[i % 2], counter=_f32_counter(arm, N), **nt_epi[i])
        tn = _tn_matrix(ns if arm != 'f32x3' else (260, 72), TN_SPECIAL) + [(260, 1100, 3, 0, dict(bias=True)), (260, 1100, 8, 1, {}), (260, 1100, 1, 0, {}), (72, 70, 0, 1, dict(ldc_pad=2))]
        if arm == 'f32x3':
            tn.append((64, 1100, 3, 1, {}))                                          # handed to cham_gemm_f32
        for i, (N, K, hint, acc, kw) in enumerate(tn):
            add("tn%d" % i, arm, 'TN', 300, N, K, hint=hint, accumulate=acc, counter=_f32_counter(arm, N), **kw)
        add("tn-xcd", arm, 'TN', 300, 72, 2048, hint=8, accumulate=1, counter=_f32_counter(arm, 72))      # 8 K-splits: one per XCD, the other partial layout
        for variant in ((2, 4) if arm == 'f32' else (2,)):                         # the 256 x 128 and 256 x 256 instances, forced at (300, 260)
            sw = ('cham_gemm_f32x3_set_variant' if arm == 'f32x3' else 'cham_gemm_set_variant', variant)
            add("nn-v%d" % variant, arm, 'NN', 300, 260, 100, bias=True, act=TH, switch=sw, counter=_f32_counter(arm, 260, variant))
            add("nt-v%d" % variant, arm, 'NT', 300, 260, 100, dact=LK, accumulate=1, switch=sw, counter=_f32_counter(arm, 260, variant))
            add("tn-v%d" % variant, arm, 'TN', 300, 260, 1100, hint=3, accumulate=1, switch=sw, counter=_f32_counter(arm, 260, variant))
    # a C and a dref aligned to 4 bytes only (an odd column offset), unsplit; TN_SPECIAL has the split one
    add("nn-c4", 'f32', 'NN', 300, 72, 100, bias=True, act=LK, c_col0=3)
    add("nt-c4", 'f32', 'NT', 300, 36, 100, dact=LK, c_col0=1, r_col0=5)
    add("nt-c4", 'bf16', 'NT', 300, 260, 100, dact=TH, accumulate=1, c_col0=1, r_col0=7)
    add("tn-c4", 'f32x3', 'TN', 300, 260, 70, accumulate=1, c_col0=3)
    # cham_gemm_f32x2h: NN and TN, N > 64
    for i, (N, K, kw) in enumerate([(260, 100, dict(bias=True, act=LK, rs_div=51)), (72, 4, dict(bias=True, act=TH)), (260, 4, dict(bias=True, ldc_pad=8))]):
        add("nn%d" % i, 'f32x2h', 'NN', 300, N, K, counter=_f32_counter('f32x2h', N), **kw)
    for i, (N, K, hint, acc, kw) in enumerate(_tn_matrix((260, 72), TN_SPECIAL) + [(72, 70, 1, 1, dict(ldc_pad=2))]):
        add("tn%d" % i, 'f32x2h', 'TN', 300, N, K, hint=hint, accumulate=acc, counter=_f32_counter('f32x2h', N), **kw)
    add("tn-xcd", 'f32x2h', 'TN', 300, 72, 2048, hint=8, counter=_f32_counter('f32x2h', 72))
    sw = ('cham_gemm_f32x3_set_variant', 2)
    add("nn-v2", 'f32x2h', 'NN', 300, 260, 100, bias=True, act=LK, switch=sw, counter=_f32_counter('f32x2h', 260, 2))
    add("tn-v2", 'f32x2h', 'TN', 300, 260, 1100, hint=3, switch=sw, counter=_f32_counter('f32x2h', 260, 2))
    # ---- the small-output TN kernel (M <= 128, K >= 512, plain), through both entry points that reach it
    for i, (M, N, K, hint, acc, arm) in enumerate([(100, 36, 1100, 0, 0, 'f32'), (100, 36, 1100, 3, 1, 'f32x3'), (36, 12, 600, 1, 1, 'f32'), (128, 200, 777, 3, 0, 'f32'),
                                                   (128, 200, 777, 1, 1, 'f32x3'), (36, 12, 600, 0, 0, 'f32')]):
        add("small%d" % i, arm, 'TN', M, N, K, hint=hint, accumulate=acc, ldc_pad=(4, 8, 2)[i % 3], counter=_f32_counter(arm, N, small=True))
    # ---- cham_gemm_b16: K % 8 == 0 (NT), M % 8 == 0 and N % 8 == 0 (TN) are the arm's own rules, so K = 104 / 8 stand for 100 / 4, M = 304 for 300 and
    # N = 264 / 40 / 16 for 260 / 36 / 12 in the TN form
    b16c = lambda N, variant=None: ('cham_gemm_b16_launch_counts', 8, (variant if variant else 0) if N > 64 else 3 if N > 32 else 4)
    nt_epi = [dict(bias=True, act=TH, out_bf16=True), dict(dact=LK, out_bf16=True), dict(out_bf16=True), dict(), dict(bias=True, act=LK, out_bf16=True), dict(dact=LK, out_bf16=True, ldc_pad=8)]
    for i, N in enumerate((260, 72, 64, 36, 32, 12)):
        add("nt%d" % i, 'b16', 'NT', 300, N, (104, 8)[i % 2], counter=b16c(N), **nt_epi[i])
    for i, (N, K, hint, acc, kw) in enumerate(_tn_matrix((264, 72, 64, 40, 32, 16), {}) + [(264, 1100, 3, 0, {}), (264, 1100, 8, 1, {}), (264, 1100, 1, 0, {})]):
        add("tn%d" % i, 'b16', 'TN', 304, N, K, hint=hint, accumulate=acc, ldc_pad=(4, 8)[i % 2], counter=b16c(N))
    add("tn-xcd", 'b16', 'TN', 304, 72, 4096, hint=8, accumulate=1, counter=b16c(72))                    # 8 K-splits: one per XCD
    for variant in (1, 2):
        sw = ('cham_gemm_b16_set_variant', variant)
        add("nt-v%d" % variant, 'b16', 'NT', 300, 260, 104, bias=True, act=TH, out_bf16=True, switch=sw, counter=b16c(260, variant))
        add("tn-v%d" % variant, 'b16', 'TN', 304, 264, 1100, hint=3, accumulate=1, switch=sw, counter=b16c(264, variant))
    # ---- plane arms, NT: K = 80 (16-k chunks, not 32), 96 (32, not 64), 192 (64)
    p3c, h2c = lambda i: ('cham_gemm_p3_launch_counts', 8, i), lambda i: ('cham_gemm_h2_launch_counts', 8, i)
    for i, K in enumerate((80, 96, 192)):
        epi = [dict(bias=True, act=TH), dict(dact=LK), dict(bias=True)][i]
        add("nt%d" % i, 'p3', 'NT', 300, 260, K, counter=p3c(0), ldc_pad=(4, 8, 4)[i], **epi)
        add("nt%d" % i, 'h2', 'NT', 300, 260, K, ldc_pad=(8, 4, 4)[i], **(dict(counter=h2c(2)) if K % 32 == 0 else dict(counter=h2c(0), quiet=(2,))), **epi)
        epi = [dict(bias=True, act=TH), dict(dact=LK), dict()][i]
        add("nt%d" % i, 'b16_dma', 'NT', 300, 260, K, out_bf16=True, ldc_pad=(4, 8, 8)[i], **(dict(counter=p3c(4)) if K % 64 == 0 else dict(counter=p3c(2), quiet=(4,))), **epi)
    add("nt-narrow", 'h2', 'NT', 300, 260, 96, dact=LK, switch=('cham_gemm_h2_set_nt_wide', 0), counter=h2c(0), quiet=(2,))
    add("nt-narrow", 'b16_dma', 'NT', 300, 260, 192, dact=LK, out_bf16=True, switch=('cham_gemm_b16_dma_set_nt_wide', 0), counter=p3c(2), quiet=(4,))
    add("nt-plain", 'p3', 'NT', 300, 260, 96, counter=p3c(0))
    add("nt-plain", 'h2', 'NT', 300, 260, 192, ldc_pad=8, counter=h2c(2))
    add("nt-blockedA0", 'h2b', 'NT', 300, 260, 96, a_blocked=True, bias=True, act=TH, counter=h2c(3))
    add("nt-blockedA1", 'h2b', 'NT', 300, 260, 192, a_blocked=True, dact=LK, ldc_pad=8, counter=h2c(3))
    # ---- plane arms, TN: whole 256 x 256 tiles only
    for i, (M, K, hint, acc) in enumerate([(256, 70, 1, 0), (512, 70, 0, 1), (256, 1100, 3, 1), (512, 1100, 0, 0), (256, 1100, 8, 0), (512, 1100, 3, 1)]):
        add("tn%d" % i, 'p3', 'TN', M, 256, K, hint=hint, accumulate=acc, ldc_pad=(4, 8)[i % 2], counter=p3c(1))
        add("tn%d" % i, 'h2', 'TN', M, 256, K, hint=hint, accumulate=acc, ldc_pad=(8, 4)[i % 2], counter=h2c(1))
        add("tn%d" % i, 'b16_dma', 'TN', M, 256, K, hint=hint, accumulate=acc, ldc_pad=(4, 8)[i % 2], counter=p3c(3))
    add("tn-xcd", 'h2', 'TN', 256, 256, 4096, hint=8, accumulate=1, counter=h2c(1))                    # 8 K-splits: one per XCD
    add("tn-xcd", 'p3', 'TN', 256, 256, 4096, hint=8, counter=p3c(1))
    add("tn-blockedA", 'h2b', 'TN', 256, 256, 1100, hint=3, a_blocked=True, counter=h2c(4))
    add("tn-blockedB", 'h2b', 'TN', 512, 256, 70, accumulate=1, b_blocked=True, ldc_pad=8, counter=h2c(4))
    # ---- the CAR dgrad with group sums: BT = 7 clicks of N + 1 = 51 rows, 256 columns, K = 64
    add("gs-rowmajor", 'h2_dgrad_gs', 'NT', 7 * 51, 256, 64, dact=LK, group_rows=51, counter=h2c(5))
    add("gs-blockedA", 'h2_dgrad_gs', 'NT', 7 * 51, 256, 64, dact=LK, group_rows=51, a_blocked=True, ldc_pad=8, counter=h2c(5))
    # ---- K = 0: the entry points built on gemm_plan admit it and give the empty sum, C = epi(bias) (C unchanged under accumulate); the others return -22
    add("k0", 'f32', 'NN', 300, 72, 0, bias=True, act=LK)
    add("k0", 'f32', 'NT', 300, 36, 0, accumulate=1)
    add("k0", 'f32', 'TN', 300, 260, 0, hint=0, accumulate=1)
    add("k0", 'bf16', 'NN', 300, 260, 0, bias=True)
    add("k0", 'f32x3', 'NN', 300, 260, 0, bias=True, act=LK)
    add("k0", 'f32x2h', 'TN', 300, 260, 0)
    for arm, form, M, N in (('b16', 'NT', 300, 72), ('p3', 'NT', 300, 260), ('b16_dma', 'TN', 256, 256), ('h2', 'NT', 300, 260), ('h2b', 'TN', 256, 256)):
        add("k0-rejected", arm, form, M, N, 0, expect=-22, out_bf16=(arm in B16_ARMS and form == 'NT'))
    add("k0-rejected", 'h2_dgrad_gs', 'NT', 7 * 51, 256, 0, expect=-22, dact=LK, group_rows=51)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return tuple(cases)


CASES = _build_cases()
RUN_CASES = tuple(c for c in CASES if c.expect == 0)
