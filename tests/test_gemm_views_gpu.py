"""Every GEMM entry point on STRIDED VIEWS with GUARDED outputs against the float64 reference of tests/gemm_reference.py, element by element.

One harness (`_run`) uploads the poisoned / NaN-framed parents of a case, calls the entry point on the views and asserts, in this order:
return code 0; the frame of C (front, the pad columns of every row, 256 whole rows behind row M) and the workspace beyond the bytes the
call was given still hold the fill's bits; every interior element is within ITS OWN bound |got - ref| <= 8 e S_ij (+ 2^-8 |ref_ij| for a
bf16 output: one round-to-nearest-even rounding - truncation would reach 2^-7), with e the fp32-CPU twin's error on the same inputs
(tests/test_gemm_reference_cpu.py prints the table and shows every slip breaking it); a second launch is bit-identical.  Where an arm has a
tile switch, the launch counters prove that the case ran on the instance it names, and the K-split count of the host-side plan is pinned
through them too.  The printed figure per case is max_ij |got - ref| / S_ij next to its bound.

What the cases cover that the per-arm files (test_gemm_gpu.py, _x3, _x2h, _b16, _b16_dma, _p3, _h2) do not: leading dimensions larger than
the width, bases at a column offset, plane strides larger than rows x ld, ldc / ldr / ldrs all different, ldc % 4 != 0 or a C aligned to 4 bytes only
(the scalar branch of the split-K reduction), 8 K-splits (one per XCD: the other layout of the partials), accumulate with split-K on the MFMA TN tiles, NT plain with accumulate, K = 0, a dref with exact +0.0 / -0.0, a row
scale whose group size does not divide the rows, and a leading dimension smaller than the extent it strides over (-22, C untouched).

K = 0: cham_gemm_f32 / _bf16 / _f32x3 / _f32x2h give the empty sum (C = epi(bias), C unchanged under accumulate); cham_gemm_b16, _p3,
_b16_dma, _h2, _h2b, _h2_dgrad_gs return -22.  Both are pinned here and stated in include/chameleon_nar.h.

The plane arms' NT cases that name the narrow kernel (K = 80; K = 96 for cham_gemm_b16_dma; the switched-off ones) also name the launch
counter of the 64-byte-piece kernel, which must stay where it was: the NT counter alone advances on either kernel.  The rejection test
keeps every other rule (alignment, the tile-blocked layout's ld % 32) and launches a control with the leading dimension at the extent,
which is taken: it is the extent that the short one fails.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import gemm_reference as G

pytestmark = pytest.mark.gpu

NAN_BITS32 = 0x7FC00000
WS_GUARD = 4096            # floats of fill behind the workspace bytes the call is given


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


# the entry point of every arm, by name (tests/test_gemm_reference_cpu.py checks that none of csrc's is missing here)
def _entry(lib, arm):
    return {'f32': lib.cham_gemm_f32, 'bf16': lib.cham_gemm_bf16, 'f32x3': lib.cham_gemm_f32x3, 'f32x2h': lib.cham_gemm_f32x2h,
            'b16': lib.cham_gemm_b16, 'p3': lib.cham_gemm_p3, 'b16_dma': lib.cham_gemm_b16_dma, 'h2': lib.cham_gemm_h2, 'h2b': lib.cham_gemm_h2b,
            'h2_dgrad_gs': lib.cham_gemm_h2_dgrad_gs}[arm]


def _switch(lib, name, value):
    """Sets a tile switch; -> the call that restores it."""
    if name in ('cham_gemm_set_variant', 'cham_gemm_f32x3_set_variant', 'cham_gemm_b16_set_variant'):
        fn = {'cham_gemm_set_variant': lib.cham_gemm_set_variant, 'cham_gemm_f32x3_set_variant': lib.cham_gemm_f32x3_set_variant,
              'cham_gemm_b16_set_variant': lib.cham_gemm_b16_set_variant}[name]
        fn(value)
        return lambda: fn(-1)
    fn = {'cham_gemm_h2_set_nt_wide': lib.cham_gemm_h2_set_nt_wide, 'cham_gemm_b16_dma_set_nt_wide': lib.cham_gemm_b16_dma_set_nt_wide}[name]
    was = fn(value)
    return lambda: fn(was)


def _counts(lib, name, n):
    out = (ctypes.c_longlong * n)()
    {'cham_gemm_launch_counts': lib.cham_gemm_launch_counts, 'cham_gemm_f32x3_launch_counts': lib.cham_gemm_f32x3_launch_counts,
     'cham_gemm_b16_launch_counts': lib.cham_gemm_b16_launch_counts, 'cham_gemm_p3_launch_counts': lib.cham_gemm_p3_launch_counts,
     'cham_gemm_h2_launch_counts': lib.cham_gemm_h2_launch_counts}[name](out, 0)
    return list(out)


def _splits_counter(p):
    """(launch-count function, length, index) holding the K-splits of the last launch of this arm."""
    if p.arm in ('f32', 'bf16') or (p.arm == 'f32x3' and p.counter and p.counter[2] == 3):
        return ('cham_gemm_launch_counts', 16, 15)
    if p.arm in ('f32x3', 'f32x2h'):
        return ('cham_gemm_f32x3_launch_counts', 8, 7)
    if p.arm == 'b16':
        return ('cham_gemm_b16_launch_counts', 8, 7)
    return ('cham_gemm_p3_launch_counts' if p.arm in ('p3', 'b16_dma') else 'cham_gemm_h2_launch_counts', 8, 7)


def _up(gpu, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(gpu)


def _blocked(planes, blk):
    """[q][rows, ld] fp16 planes -> the tile-blocked buffer of include/chameleon_nar.h (rows beyond the matrix zero), (buffer, plane stride, tiles)."""
    rows, ld = planes[0].shape
    tiles = -(-rows // 256)
    ps = tiles * (ld // 32) * blk + 64
    buf = np.zeros(len(planes) * ps, np.float16)
    r, c = np.arange(rows)[:, None], np.arange(ld)[None, :]
    idx = ((r // 256) * (ld // 32) + c // 32) * blk + (r % 256) * 32 + c % 32
    for q, X in enumerate(planes):
        buf[q * ps + idx] = X
    return buf, ps, tiles


class _Call:
    """The device buffers of one case and the argument list of its entry point."""

    def __init__(self, gpu, p):
        self.p, self.gpu, d = p, gpu, G.data(p)
        lib = _lib_()
        self.keep = []
        def view_ptr(t, v):
            self.keep.append(t)
            return t.data_ptr() + v.col0 * t.element_size()
        self.a_tiles = self.b_tiles = 0
        a_ps, b_ps = p.A.ps, p.B.ps
        if p.a_blocked:
            buf, a_ps, self.a_tiles = _blocked(d['A'], lib.cham_h2b_block_elements())
            A = view_ptr(_up(gpu, buf), G.View(0, 0, 0))
        else:
            A = view_ptr(_up(gpu, d['A_parent']), p.A)
        if p.b_blocked:
            buf, b_ps, self.b_tiles = _blocked(d['B'], lib.cham_h2b_block_elements())
            B = view_ptr(_up(gpu, buf), G.View(0, 0, 0))
        else:
            B = view_ptr(_up(gpu, d['B_parent']), p.B)
        c0 = torch.from_numpy(G.out_parent(p, d)).to(gpu)
        self.C0 = c0.to(torch.bfloat16) if p.out_bf16 else c0
        self.C = self.C0.clone()
        Cp = self.C.data_ptr() + (G.FRONT + p.C.col0) * self.C.element_size()
        bias = view_ptr(_up(gpu, d['bias']), G.View(0, 0, 0)) if p.bias else None
        R = view_ptr(_up(gpu, d['R_parent']), p.R) if p.dact else None
        rs = view_ptr(_up(gpu, d['rs_parent']), p.RS) if p.rs_div else None
        ra = view_ptr(_up(gpu, d['rec_a']), G.View(0, 0, 0)) if d['rec_a'] is not None else None
        rb = view_ptr(_up(gpu, d['rec_b']), G.View(0, 0, 0)) if d['rec_b'] is not None else None
        self.ws_bytes = p.ws_bytes()
        self.ws = torch.full((self.ws_bytes // 4 + WS_GUARD,), float('nan'), device=gpu)
        ws = self.ws.data_ptr() if self.ws_bytes else None
        self.gs = None
        tn = int(p.form == 'TN')
        a = dict(A=A, a_ps=a_ps, lda=p.A.ld, a_sc=ra, tA=int(p.transA), B=B, b_ps=b_ps, ldb=p.B.ld, b_sc=rb, tB=int(p.transB), tn=tn, C=Cp, ldc=p.C.ld,
                 out_f32=int(not p.out_bf16), M=p.M, N=p.N, K=p.K, bias=bias, act=p.act, dref=R, ldr=p.R.ld if p.dact else 0, dact=p.dact, rs=rs,
                 ldrs=p.RS.ld if p.rs_div else 0, rs_div=p.rs_div or 1, acc=p.accumulate, ws=ws, wsb=self.ws_bytes, hint=p.hint, a_tiles=self.a_tiles,
                 b_tiles=self.b_tiles, dref_blocked=0, group_rows=p.group_rows, gs=None, gsb=0)
        if p.arm == 'h2_dgrad_gs':
            a['gsb'] = int(lib.cham_gemm_h2_groupsum_bytes(p.M, p.N, p.group_rows))
            self.gs = torch.full((a['gsb'] // 4 + WS_GUARD,), float('nan'), device=gpu)
            a['gs'] = self.gs.data_ptr()
        self.args = a

    ORDER = {
        'f32': "A lda tA B ldb tB C ldc M N K bias act dref ldr dact rs ldrs rs_div acc ws wsb hint",
        'f32x2h': "A lda tA B ldb tB C ldc M N K bias act rs ldrs rs_div acc ws wsb hint a_sc b_sc",
        'b16': "A lda tA B ldb tB C ldc out_f32 M N K bias act dref ldr dact acc ws wsb hint",
        'p3': "A a_ps lda B b_ps ldb tn C ldc M N K bias act dref ldr dact acc ws wsb hint",
        'b16_dma': "A lda B ldb tn C ldc M N K bias act dref ldr dact acc ws wsb hint",
        'h2': "A a_ps lda a_sc B b_ps ldb b_sc tn C ldc M N K bias act dref ldr dact acc ws wsb hint",
        'h2b': "A a_ps lda a_sc B b_ps ldb b_sc tn C ldc M N K bias act dref ldr dact acc ws wsb hint a_tiles b_tiles dref_blocked",
        'h2_dgrad_gs': "A a_ps lda a_sc B b_ps ldb b_sc C ldc M N K dref ldr a_tiles dref_blocked group_rows gs gsb",
    }
    ORDER['bf16'] = ORDER['f32x3'] = ORDER['f32']

    def launch(self, **override):
        a = dict(self.args, **override)
        return _entry(_lib_(), self.p.arm)(*[a[k] for k in self.ORDER[self.p.arm].split()], torch.cuda.current_stream().cuda_stream)

    def reset(self):
        self.C.copy_(self.C0)
        self.ws.fill_(float('nan'))
        if self.gs is not None:
            self.gs.fill_(float('nan'))

    def download(self):
        torch.cuda.synchronize()
        bits = (self.C.view(torch.int16) if self.p.out_bf16 else self.C.view(torch.int32)).cpu().numpy()
        return bits, self.C.float().cpu().numpy()

    def frame_holds_the_fill(self, bits, whole=False):
        """whole: a rejected call - the interior too is as uploaded."""
        if whole and not torch.equal(self.C.view(torch.int16), self.C0.view(torch.int16)):
            return False
        frame = np.ones(bits.shape, bool)
        frame[self.p.C.index(base=G.FRONT)] = False
        fill = np.int16(0x7FC0) if self.p.out_bf16 else np.int32(NAN_BITS32)
        ws_tail = self.ws[self.ws_bytes // 4:].view(torch.int32)
        ok = bool((bits[frame] == fill).all()) and bool((ws_tail == NAN_BITS32).all())
        if self.gs is not None:
            ok = ok and bool((self.gs[self.args['gsb'] // 4:].view(torch.int32) == NAN_BITS32).all())
        return ok


def _note(name, ratio, k):
    print("    %-44s %.2e  = %.2f x the fp32-CPU error (bound 8 x = %.2e)" % (name, ratio, ratio / (k / G.MARGIN) if k else 0.0, k))
    assert ratio <= k, (name, ratio, k)


def _run(gpu, p):
    lib = _lib_()
    call = _Call(gpu, p)
    restore = _switch(lib, *p.switch) if p.switch else (lambda: None)
    try:
        before = _counts(lib, *p.counter[:2]) if p.counter else None
        rc = call.launch()
        assert rc == p.expect, (p.name, rc)                                                      # 1. the return code
        bits, vals = call.download()
        if p.expect:
            assert call.frame_holds_the_fill(bits, whole=True), "a rejected call wrote to C or to the workspace"
            return
        if p.counter:
            after = _counts(lib, *p.counter[:2])
            assert after[p.counter[2]] == before[p.counter[2]] + 1, (p.name, p.counter, before, after)
            assert all(after[i] == before[i] for i in p.quiet), (p.name, p.quiet, before, after)      # and not on the instance it does not name
        if p.K:
            sc = _splits_counter(p)
            assert _counts(lib, *sc[:2])[sc[2]] == p.plan()[0], (p.name, _counts(lib, *sc[:2]), p.plan())
        assert call.frame_holds_the_fill(bits), "%s wrote outside its output or its workspace" % p.name      # 2. the guards
        intact, ratio = G.judge(p, vals)
        assert intact, p.name
        _note(p.name, ratio, G.bound(p))                                                                 # 3. every element within its own bound
        gs = call.gs.cpu().numpy().copy() if call.gs is not None else None
        call.reset()
        assert call.launch() == 0
        bits2, _ = call.download()
        assert np.array_equal(bits, bits2), "%s: two launches differ" % p.name                           # 4. bit-identical twice
        if gs is not None:
            _check_group_sums(p, call, gs)
    finally:
        restore()


def _check_group_sums(p, call, gs):
    """The dgrad's group sums against float64 sums of the reference rows: the bound is 8 x the error of the fp32 twin's rows added one after
    the other, per piece, in units of the piece's own sum of S."""
    n = call.args['gsb'] // 4
    gs2 = call.gs.cpu().numpy()
    assert np.array_equal(gs.view(np.int32), gs2.view(np.int32)), "group sums of two launches differ"
    ref, S = G.reference(p)
    want, scale = G.group_sums(p, np.asarray(ref)), G.group_sums(p, np.asarray(S))
    tw = G.group_sums(p, G.twin_values(p))
    live = ~np.isnan(want)
    k = G.MARGIN * float((np.abs(tw.astype(np.float64) - want)[live] / scale[live]).max())
    got = gs[:n].reshape(-1, p.N).astype(np.float64)
    assert got.shape == want.shape and not np.isnan(got[live]).any(), "a piece the consumer reads was not written"
    _note(p.name + " group sums", float((np.abs(got - want)[live] / scale[live]).max()), k)


@pytest.mark.parametrize("p", G.CASES, ids=[c.name for c in G.CASES])
def test_view_case(gpu, p):
    _run(gpu, p)


# ---- a leading dimension smaller than the extent it strides over: -22 from every entry point, C untouched -----------------------------------
def _base_case(arm):
    pick = [c for c in G.RUN_CASES if c.arm == arm and c.K and c.N >= 64 and not c.switch]
    with_dref = [c for c in pick if c.dact]
    return (with_dref or pick)[0]


@pytest.mark.parametrize("arm", sorted(G.ENTRY))
def test_short_leading_dimension_is_rejected(gpu, arm):
    step = 4 if arm in G.F32_ARMS else 8
    cases = [_base_case(arm)]
    if arm in G.F32_ARMS:
        cases.append(next(c for c in G.RUN_CASES if c.arm == arm and c.rs_div and c.K))
    if cases[0].a_blocked:
        cases.append(next(c for c in G.RUN_CASES if c.arm == arm and not c.a_blocked))
    tried = set()
    for p in cases:
        call = _Call(gpu, p)
        a = call.args
        a_cols, b_cols = p.A.cols, p.B.cols
        # a tile-blocked operand keeps ld % 32 == 0, so that only the extent is wrong; every other short value keeps the arm's alignment rule
        short = dict(lda=a_cols - (32 if p.a_blocked else step), ldb=b_cols - (32 if p.b_blocked else step), ldc=p.N - 4)
        exact = dict(lda=a_cols, ldb=b_cols, ldc=p.N)
        if p.dact:
            short['ldr'], exact['ldr'] = p.N - 4, p.N
        if p.rs_div:
            short['ldrs'], exact['ldrs'] = p.RS.cols - 4, p.RS.cols
        if p.a_blocked and p.form == 'NT':
            short.pop('lda')          # (the tile-blocked A of the NT form has its own rule, ld == K: tests/test_gemm_h2_gpu.py)
        for name, value in short.items():
            assert name in call.ORDER[arm].split(), (arm, name)
            assert call.launch(**{name: value}) == -22, (p.name, name, value, a[name])
            bits, _ = call.download()
            assert call.frame_holds_the_fill(bits, whole=True), (p.name, name)
            # the control: the same call with the leading dimension AT the extent is taken, so it is the extent that the short one fails
            assert call.launch(**{name: exact[name]}) == 0, (p.name, name, exact[name])
            torch.cuda.synchronize()
            call.reset()
            tried.add(name)
    assert {'lda', 'ldb', 'ldc'} <= tried and ('ldrs' in tried) == (arm in G.F32_ARMS), tried
    assert 'ldr' in tried or arm == 'f32x2h', tried          # (cham_gemm_f32x2h has no dref)
