"""The backward path between the scorer's first layer and the feature tables on EXACT-SUM inputs (tests/backward_reference.py): the five
entry points of csrc/dm_fused.hip, cham_combine_bwd / _gs / _b16 and cham_feature_bwd / _ws must give the float64 reference bit for bit -
every fp32 product and sum of these inputs is exact in any order (tests/test_backward_reference_cpu.py), so no tolerance is needed and one
dropped, doubled or misplaced row fails whatever the size of its sum.  (The sign of a zero is not compared: 0 * pred is -0 where pred < 0.)

Inputs are FRAMED: NaN rows directly behind the last valid row of dS1, Z2 and pred, NaN in the pad columns of dS1 (lds1 > 128) and between
the planes of Ws1; outputs, workspaces and the gaps between output planes are NaN-filled and must come back fully written inside and
untouched outside.  Small shapes only; one Gaussian case per family holds every element to 8 e S (tests/gemm_reference.py's bound).
Largest measured max |hip - ref| / S of the Gaussian cases (MI355X; bounds 0.1-3.7e-6): fused dgrad dZ2 1.7e-7 (p3), 1.5e-7 (h2, h2_blk), 6.9e-8
(h2h, h2_blk with the fp16 records), dpred <= 6.3e-8, b2part <= 6.0e-9; combine dU / dV 1.4e-7 / 1.2e-7 (gs dU 8.3e-8, b16 2.7e-8 / 1.9e-9);
feature dgamma / dbeta 2.6e-8 / 1.5e-8 (ws 3.8e-8 / 3.3e-8)."""
import numpy as np
import pytest
import torch

from tests import backward_reference as B
from tests import gemm_reference as G
from tests.features_gpu_helpers import Out, _lib_, _st, _twice

pytestmark = pytest.mark.gpu
f32, f64 = np.float32, np.float64
NAN = float('nan')
FORMS = ('p3', 'h2', 'h2h', 'h2_blk', 'h2_blk_h', 'b16')          # h2_blk: six bf16 products inside; h2_blk_h: with the fp16 records, three


def _dev(gpu, a):
    return torch.from_numpy(np.array(a)).to(gpu)          # (a copy: the cached inputs are read-only)


def _framed(gpu, a, ld, rows_behind, dtype=torch.float32):
    """a [rows, cols] at the head of a NaN-filled [rows + rows_behind, ld] buffer."""
    buf = torch.full((a.shape[0] + rows_behind, ld), NAN, dtype=dtype, device=gpu)
    buf[:a.shape[0], :a.shape[1]] = _dev(gpu, a).to(dtype)
    return buf


def _rec(gpu):
    return torch.zeros(8, dtype=torch.float32, device=gpu)


def _as_f64(x):
    """what Out.numpy() returns -> float64 values (uint16 = bf16 bit patterns)"""
    return G.bf16_from_bits(x).astype(f64) if x.dtype == np.uint16 else x.astype(f64)


class _DmCall:
    """One input set of the fused dgrad on the device, framed, with everything the five entry points take: the three bf16 planes and the two
    fp16 planes of Ws1 (planes w_ps > C * 128 elements apart, NaN between them), the scale records of cham_h2_scale_rownorm / _rownorm2 /
    cham_split2h exactly as tests/test_dm_fused_gpu.py drives them."""

    def __init__(self, gpu, lib, inp, variant=0, framed=True):
        from chameleon_recsys_amd._lib import check, ptr
        self.gpu, self.lib, self.inp = gpu, lib, inp
        NC, BT, C = inp['NC'], inp['BT'], inp['C']
        self.NC, self.BT, self.C, self.Rc = NC, BT, C, BT * NC
        self.b16 = bool(inp.get('b16'))
        behind = 3 if framed else 0
        if self.b16:
            self.lds1 = (136, 160)[variant % 2] if framed else 128                       # % 8 == 0
            dt = torch.bfloat16
        else:
            self.lds1 = (132, 140)[variant % 2] if framed else 128                       # % 4 == 0
            dt = torch.float32
        self.w_ps = C * 128 + ((8, 72)[variant % 2] if framed else 0)                    # % 8 == 0
        self.gap = (4, 36)[variant % 2] if framed else 0                                 # out_plane_stride - plane: % 4 == 0
        self.dS1 = _framed(gpu, inp['dS1'], self.lds1, behind, dt)
        self.Z2 = _framed(gpu, inp['Z2'], C, behind, dt)
        self.pred = _framed(gpu, inp['pred'], C, behind)
        st = _st()
        if self.b16:
            self.W16 = _dev(gpu, inp['Ws1']).bfloat16()
            return
        Ws1 = _dev(gpu, inp['Ws1'])
        self.W3 = torch.full((3 * self.w_ps,), NAN, dtype=torch.bfloat16, device=gpu)
        check(lib.cham_split3(ptr(Ws1), C, 128, 128, ptr(self.W3), self.w_ps, 128, None, 0, 0, st), "cham_split3")
        self.rw, self.rout, self.rds = _rec(gpu), _rec(gpu), _rec(gpu)
        check(lib.cham_h2_scale_rownorm(ptr(Ws1), C, 128, 128, None, ptr(self.rw), st), "cham_h2_scale_rownorm")
        check(lib.cham_h2_scale_rownorm2(ptr(self.dS1), self.Rc, 128, self.lds1, self.rw.data_ptr() + 8, ptr(self.rout), ptr(self.rds), st), "cham_h2_scale_rownorm2")
        self.Wh = torch.full((2 * self.w_ps,), NAN, dtype=torch.float16, device=gpu)
        check(lib.cham_split2h(ptr(Ws1), C, 128, 128, ptr(self.Wh), self.w_ps, 128, None, 0, 0, ptr(self.rw), 0, st), "cham_split2h")
        torch.cuda.synchronize()
        self.scales = dict(out=float(self.rout[0]), out_inv=float(self.rout[1]), a=float(self.rds[0]), w=float(self.rw[0]))
        for v in self.scales.values():
            assert v > 0 and np.frexp(v)[0] == 0.5, "a scale record is not a power of two: %r" % (self.scales,)

    def run(self, form):
        """-> (dZ2 [Rc, C] float64 values, dpred, b2 [BT, C] float32) of one launch; every plane fully written in the valid rows and untouched
        behind them and between the planes (Out.numpy checks the frame around the allocation)."""
        from chameleon_recsys_amd._lib import check, ptr
        lib, gpu, C, BT, N, Rc = self.lib, self.gpu, self.C, self.BT, self.NC - 1, self.Rc
        blocked = form.startswith('h2_blk')
        nplanes, dt = {'p3': (3, torch.bfloat16), 'b16': (1, torch.bfloat16)}.get(form, (2, torch.float16))
        if blocked:
            blk, ncb = lib.cham_h2b_block_elements(), C // 32
            plane = (-(-Rc // 256) + 1) * ncb * blk                      # one row tile more: a workgroup's window spans two
            r, c = np.arange(Rc)[:, None], np.arange(C)[None, :]
            where = ((r >> 8) * ncb + (c >> 5)) * blk + (r & 255) * 32 + (c & 31)
        else:
            plane = Rc * C
            where = np.arange(Rc * C).reshape(Rc, C)
        ps = plane + self.gap
        D = Out(gpu, ((nplanes - 1) * ps + plane,), dt)
        dp, b2 = Out(gpu, (BT, C)), Out(gpu, (BT, C))
        a = (ptr(self.dS1), self.lds1, 128)
        tail = (ptr(self.Z2), ptr(self.pred), C, BT, N, D.ptr(), ps)
        st = _st()
        if form == 'p3':
            rc = lib.cham_dm_mulpred_p3(*a, ptr(self.W3), self.w_ps, *tail, dp.ptr(), b2.ptr(), st)
        elif form == 'h2':
            rc = lib.cham_dm_mulpred_h2(*a, ptr(self.W3), self.w_ps, *tail, ptr(self.rout), dp.ptr(), b2.ptr(), st)
        elif form == 'h2h':
            rc = lib.cham_dm_mulpred_h2h(*a, ptr(self.Wh), self.w_ps, ptr(self.rds), ptr(self.rw), *tail, ptr(self.rout), dp.ptr(), b2.ptr(), st)
        elif form == 'h2_blk':
            rc = lib.cham_dm_mulpred_h2_blk(*a, ptr(self.W3), self.w_ps, None, None, *tail, ptr(self.rout), dp.ptr(), b2.ptr(), st)
        elif form == 'h2_blk_h':
            rc = lib.cham_dm_mulpred_h2_blk(*a, ptr(self.Wh), self.w_ps, ptr(self.rds), ptr(self.rw), *tail, ptr(self.rout), dp.ptr(), b2.ptr(), st)
        else:
            rc = lib.cham_dm_mulpred_b16(*a, ptr(self.W16), ptr(self.Z2), ptr(self.pred), C, BT, N, D.ptr(), dp.ptr(), b2.ptr(), st)
        check(rc, "cham_dm_mulpred (%s)" % form)
        flat = _as_f64(D.numpy())
        valid = np.zeros(plane, bool)
        valid[where.reshape(-1)] = True
        total = np.zeros((Rc, C))
        for q in range(nplanes):
            reg = flat[q * ps:q * ps + plane]
            assert not np.isnan(reg[valid]).any(), "%s: plane %d is not fully written in the valid rows" % (form, q)
            assert np.isnan(reg[~valid]).all(), "%s: plane %d was written outside the valid rows" % (form, q)
            assert np.isnan(flat[q * ps + plane:(q + 1) * ps]).all(), "%s: the gap behind plane %d was written" % (form, q)
            total += reg[where]
        if nplanes == 2:
            total *= self.scales['out_inv']
        gp, gb = dp.numpy(), b2.numpy()
        assert not np.isnan(gp).any() and not np.isnan(gb).any(), "%s: dpred / b2part not fully written" % form
        return total, gp, gb


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("NC", B.DM_NC)
def test_fused_dgrad_is_exact_on_exact_sum_inputs(gpu, NC, form):
    """Every BT of {1, PW - 1, PW, PW + 1, 2 PW + 1} x C of {64, 128, 192}; lds1 > 128, plane strides larger than the planes, framed."""
    lib = _lib_()
    for i, (_, BT, C) in enumerate(c for c in B.dm_cases() if c[0] == NC):
        inp = B.dm_inputs(NC, BT, C, form == 'b16')
        ref = B.dm_reference(inp)
        call = _DmCall(gpu, lib, inp, variant=i + BT)
        dz, dp, b2 = _twice(lambda: call.run(form))
        tag = (form, NC, BT, C)
        assert np.array_equal(dz, ref['dZ2']), ("dZ2", tag, int((dz != ref['dZ2']).sum()))
        assert B.same_bits(B.pos_zero(dp), B.exact32(ref['dpred'])), ("dpred", tag)
        assert B.same_bits(B.pos_zero(b2), B.exact32(ref['b2'])), ("b2part", tag)
        m = inp['masked']
        assert not dz[np.repeat(m, NC)].any() and not dp[m].any() and not b2[m].any(), ("a masked position is not exactly zero", tag)


def _print_ratio(name, what, r, bound, raw=None):
    print("    %-30s %-6s max |hip - ref| / S = %.2e   (bound %.2e)%s" % (name, what, r, bound, "" if raw is None else "   before the bf16 allowance: %.2e" % raw))


def test_fused_dgrad_gaussian_per_element(gpu):
    """1 + N = 51, BT = 7, C = 128, Gaussian operands: every element of dZ2, dpred and b2part within 8 e S of the float64 sum of exactly the
    plane products the form makes.  On top: what the stored planes cannot hold (three bf16 planes: 2^-24 |x|; two fp16 planes: 2^-22 |x| +
    2^-24 / scale, the h plane's kept sign included - csrc/common.h).  The bf16 twin: the reference rounds dM and dZ2 where the kernel does, and
    every element far from a bf16 rounding boundary must carry the reference's BITS (tests/backward_reference.dm_random_b16)."""
    lib = _lib_()
    inp = B.dm_random_inputs()
    inp16 = dict(inp, b16=True, dS1=G.bf16_rne(inp['dS1']), Ws1=G.bf16_rne(inp['Ws1']), Z2=G.bf16_rne(inp['Z2']))
    call, call16 = _DmCall(gpu, lib, inp, framed=False), _DmCall(gpu, lib, inp16, framed=False)
    sc = call.scales
    print()
    failed = []
    for form in FORMS:
        arith = {'h2h': 'h2h', 'h2_blk_h': 'h2h', 'b16': 'b16'}.get(form, 'p3')
        ref, S, bound, extra = B.dm_random_reference(inp, arith, sc['a'], sc['w'])
        dz, dp, b2 = (call16 if form == 'b16' else call).run(form)
        if form == 'b16':
            same = G.bf16_bits(dz.astype(f32)) == extra['bits']
            print("    cham_dm_mulpred_b16: %.4f of dZ2 far from a bf16 rounding boundary, %d of them differ from the reference's bits; %d of the others do"
                  % (extra['safe'].mean(), int((~same & extra['safe']).sum()), int((~same & ~extra['safe']).sum())))
            if (~same & extra['safe']).any():
                failed.append((form, 'dZ2 bits', int((~same & extra['safe']).sum())))
        store = 0.0 if form == 'b16' else 2.0 ** -24 * np.abs(ref['dZ2']) if form == 'p3' else 2.0 ** -22 * np.abs(ref['dZ2']) + 2.0 ** -24 / sc['out']
        for what, got, ex in (('dZ2', dz, extra['dZ2'] + store), ('dpred', dp, extra['dpred']), ('b2', b2, extra['b2'])):
            r = B.ratio(got, ref[what], S[what], ex)
            _print_ratio('cham_dm_mulpred_' + form.replace('h2_blk_h', 'h2_blk (fp16)'), what, r, bound[what], B.ratio(got, ref[what], S[what]) if form == 'b16' else None)
            if not r <= bound[what]:
                failed.append((form, what, r, bound[what]))
    assert not failed, failed


# ---- combine backward -------------------------------------------------------------------------------------------------------------------------
def _combine_run(gpu, lib, which, inp, gsum=None, short=0):
    """-> (dU, dV) of one launch into NaN-filled outputs with a NaN-filled workspace (`short`: that many bytes less than asked for -> the
    return code)."""
    from chameleon_recsys_amd._lib import check, ptr
    BT, N, pmax, C = inp['BT'], inp['N'], inp['pmax'], inp['C']
    need = lib.cham_combine_bwd_workspace_bytes(C, BT, N, pmax)
    ws = torch.full(((need + 3) // 4,), NAN, dtype=torch.float32, device=gpu)
    dU, dV = Out(gpu, (BT, C)), Out(gpu, (2 * BT + pmax + 1, C))
    d_slot = _dev(gpu, inp['slot'])
    if which == 'b16':
        d_in = _dev(gpu, inp['dpre'][:BT])
        d_c = _dev(gpu, inp['dpre'][BT:]).bfloat16()
        rc = lib.cham_combine_bwd_b16(ptr(d_in), ptr(d_c), C, BT, N, pmax, ptr(d_slot), dU.ptr(), dV.ptr(), ptr(ws), need - short, _st())
    elif which == 'gs':
        d = _dev(gpu, inp['dpre'])
        rc = lib.cham_combine_bwd_gs(ptr(d), C, BT, N, pmax, ptr(d_slot), dU.ptr(), dV.ptr(), ptr(ws), need - short, ptr(gsum), gsum.numel() * 4, _st())
    else:
        d = _dev(gpu, inp['dpre'])
        rc = lib.cham_combine_bwd(ptr(d), C, BT, N, pmax, ptr(d_slot), dU.ptr(), dV.ptr(), ptr(ws), need - short, _st())
    if short:
        torch.cuda.synchronize()
        assert dU.untouched() and dV.untouched()
        return rc
    check(rc, "cham_combine_bwd (%s)" % which)
    return dU.numpy(), dV.numpy()


@pytest.mark.parametrize("BT,N,pmax,C,plain", B.combine_cases())
def test_combine_bwd_is_exact_on_exact_sum_inputs(gpu, BT, N, pmax, C, plain):
    """cham_combine_bwd and cham_combine_bwd_b16 (integers up to 8 are bf16 values) against np.add.at: BT on both sides of the position chunk
    of a hot slot (SLOT_HOT, read from the kernel), a slot in every position, a cold one, the pad slot N times in a click, masked clicks first,
    last and in the middle - one of them with a gradient, which no row of dV may see -, pmax 1 and pmax > BT N."""
    lib = _lib_()
    inp = B.combine_inputs(BT, N, pmax, C, plain)
    dU, dV = (B.exact32(x) for x in B.combine_reference(inp))
    for which in ('f32', 'b16'):
        gU, gV = _twice(lambda: _combine_run(gpu, lib, which, inp))
        assert B.same_bits(B.pos_zero(gU), dU), ("dU", which)
        assert B.same_bits(B.pos_zero(gV), dV), ("dV", which, np.flatnonzero((gV != dV).any(1))[:8] - 2 * BT)
        assert _combine_run(gpu, lib, which, inp, short=1) == -22


@pytest.mark.parametrize("NC,BT", B.GS_CASES)
def test_combine_bwd_gs_from_a_hand_built_group_sum_array(gpu, NC, BT):
    """The group-sum array built on the host from the reference in the header's layout - no GEMM involved -, NaN in every piece the layout
    leaves unused: dU and dV equal the reference and the plain entry point's bits.  (BT (1 + N) is no multiple of 128 where 1 + N allows it.)"""
    lib = _lib_()
    for C in (4, 68):
        inp = B.combine_inputs(BT, NC - 1, 40, C)
        dU, dV = (B.exact32(x) for x in B.combine_reference(inp))
        gs = B.group_sums(inp['dpre'][BT:], NC)
        assert np.isnan(gs).any() and gs.dtype == f32
        gsum = _dev(gpu, gs)
        assert gsum.numel() * 4 == lib.cham_gemm_h2_groupsum_bytes(BT * NC, C, NC)
        gU, gV = _twice(lambda: _combine_run(gpu, lib, 'gs', inp, gsum))
        pU, pV = _combine_run(gpu, lib, 'f32', inp)
        assert B.same_bits(B.pos_zero(gU), dU) and B.same_bits(B.pos_zero(gV), dV)
        assert B.same_bits(gU, pU) and B.same_bits(gV, pV)
        assert _combine_run(gpu, lib, 'gs', inp, gsum, short=1) == -22


def test_combine_bwd_gaussian_per_element(gpu):
    lib = _lib_()
    inps = dict(zip(('f32', 'b16'), B.combine_random_inputs()))
    BT, N, pmax, C = B.COMBINE_RANDOM
    gs = B.group_sums(inps['f32']['dpre'][BT:].astype(f64), N + 1).astype(f32)
    print()
    failed = []
    for which, ((dU, dV), (SU, SV), (bU, bV)) in B.combine_random_reference().items():
        got = _combine_run(gpu, lib, which, inps.get(which, inps['f32']), _dev(gpu, gs) if which == 'gs' else None)
        for what, g, ref, S, b in (('dU', got[0], dU, SU, bU), ('dV', got[1], dV, SV, bV)):
            r = B.ratio(g, ref, S)
            _print_ratio('cham_combine_bwd' + {'f32': '', 'b16': '_b16', 'gs': '_gs'}[which], what, r, b)
            if not r <= b:
                failed.append((which, what, r, b))
    assert not failed, failed


# ---- feature backward -------------------------------------------------------------------------------------------------------------------------
def _feature_run(gpu, lib, ws_form, dxs, xraw, short=0):
    from chameleon_recsys_amd._lib import check, ptr
    R, F = dxs.shape
    dg, db = Out(gpu, (F,)), Out(gpu, (F,))
    a, b = _dev(gpu, dxs), _dev(gpu, xraw)
    if ws_form:
        need = lib.cham_feature_bwd_workspace_bytes(F)
        ws = torch.full((need // 4,), NAN, dtype=torch.float32, device=gpu)
        rc = lib.cham_feature_bwd_ws(ptr(a), ptr(b), R, F, dg.ptr(), db.ptr(), ptr(ws), need - short, _st())
    else:
        rc = lib.cham_feature_bwd(ptr(a), ptr(b), R, F, dg.ptr(), db.ptr(), _st())
    if short:
        torch.cuda.synchronize()
        assert dg.untouched() and db.untouched()
        return rc
    check(rc, "cham_feature_bwd")
    return dg.numpy(), db.numpy()


@pytest.mark.parametrize("R,F", B.feature_cases())
def test_feature_bwd_is_exact_on_exact_sum_inputs(gpu, R, F):
    """Both entry points against the reference and against each other, bit for bit: R of 1, 63, 64, 65 and both sides of the row chunk of
    cham_feature_bwd_ws (read from the kernel), F of 4, 60, 64, 68, 1024 (columns that do not fill the 64-lane block)."""
    lib = _lib_()
    dxs, xraw = B.feature_inputs(R, F)
    dg, db = (B.exact32(x) for x in B.feature_reference(dxs, xraw))
    outs = [_twice(lambda: _feature_run(gpu, lib, ws_form, dxs, xraw)) for ws_form in (False, True)]
    for name, (g, b) in zip(('cham_feature_bwd', 'cham_feature_bwd_ws'), outs):
        assert B.same_bits(B.pos_zero(g), dg) and B.same_bits(B.pos_zero(b), db), name
    assert B.same_bits(outs[0][0], outs[1][0]) and B.same_bits(outs[0][1], outs[1][1])
    assert _feature_run(gpu, lib, True, dxs, xraw, short=4) == -22


def test_feature_bwd_gaussian_per_element(gpu):
    lib = _lib_()
    dxs, xraw = B.feature_random_inputs()
    ref, S, bound = B.feature_random_reference()
    print()
    failed = []
    for ws_form, name in ((False, 'cham_feature_bwd'), (True, 'cham_feature_bwd_ws')):
        got = _feature_run(gpu, lib, ws_form, dxs, xraw)
        for what, g, r_, s_, b in zip(('dgamma', 'dbeta'), got, ref, S, bound):
            r = B.ratio(g, r_, s_)
            _print_ratio(name, what, r, b)
            if not r <= b:
                failed.append((name, what, r, b))
    assert not failed, failed
