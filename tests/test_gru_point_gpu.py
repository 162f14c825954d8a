"""The four step-wise GRU kernels of csrc/rnn.hip (cham_gru_point_gates_fwd / _out_fwd / _c_bwd / _r_bwd) against the float64 BPTT
reference (tests/rnn_reference.py), driven per time step as nar_model.py drives them.  Both recurrent products per direction are computed
in float64 on the device and rounded to fp32, so that only the point kernels are under test (tests/test_gru_stepwise_cpu.py pins this
algebra on the CPU and shows that the bound catches a dropped reset path).

Per array (out, hprev, G, Cc, R, RH, dxproj) max |hip - ref| <= 2e-5 max |ref|.  Exactly zero: out and dxproj beyond a session's length
and the pad lanes (H = Hp - 17) of out, hprev, Cc, RH and dxproj.  Rows >= B of the NaN-filled, 32-row-padded buffers stay NaN, and two
runs are bit-identical.

Worst relative error observed on one MI355X, over the three shapes and all arrays:
    step-wise GRU  Hp 512 2.1e-7   Hp 640 2.0e-7   Hp 1024 2.3e-7   saturated (Hp 640) 3.3e-7
    Hp 384, same inputs:  step-wise 2.2e-7,  fused cham_rnn_fwd / _bwd 5.5e-7 (its recurrent products are fp32 MFMA sums)
"""
import numpy as np
import pytest
import torch

from tests.rnn_reference import REL_BOUND, kernel_reference, padded_inputs, rel_err

pytestmark = pytest.mark.gpu

# (B, T): one row and no recurrence; one row past a 32-row group, several blocks; Adressa's length.  The smallest shapes at which
# masking, the carry, a block tail or an offset can go wrong.
SHAPES = [(1, 1), (33, 7), (70, 30)]
POINT_HP = [512, 640, 1024]
KEYS = ('out', 'hprev', 'G', 'Cc', 'R', 'RH')


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


class _Outputs:
    """NaN-filled output arrays [B, T, width] on a buffer padded to whole 32-row groups: every element the kernels must write is checked,
    and the rows past B must come back untouched."""

    def __init__(self, gpu, B, T, widths):
        Bp = (B + 31) // 32 * 32
        self.B = B
        self.full = {k: torch.full((Bp, T, w), float('nan'), device=gpu) for k, w in widths.items()}

    def __getitem__(self, k):
        return self.full[k]

    def numpy(self):
        for k, v in self.full.items():
            assert torch.isnan(v[self.B:]).all(), "%s written beyond row B" % k
        return {k: v[:self.B].cpu().numpy() for k, v in self.full.items()}


def _run_point(gpu, Hp, inp):
    """The step-wise GRU as nar_model.py runs it: per step two products + two kernels forward, two kernels + two products backward."""
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    B, T = inp['dout'].shape[:2]
    Bp = (B + 31) // 32 * 32
    xproj, lens, dout = _dev(gpu, inp['xproj']), _dev(gpu, inp['lengths']), _dev(gpu, inp['dout'])
    Wgh64, Wch64 = _dev(gpu, inp['Wh']).double(), _dev(gpu, inp['Wch']).double()
    o = _Outputs(gpu, B, T, dict({k: Hp for k in KEYS}, dxproj=3 * Hp))
    nan = lambda w: torch.full((Bp, w), float('nan'), device=gpu)
    h = nan(Hp); h[:B] = 0
    zg, zc = nan(2 * Hp), nan(Hp)
    st = _stream()
    for t in range(T):
        zg[:B] = (h[:B].double() @ Wgh64).float()
        check(lib.cham_gru_point_gates_fwd(ptr(xproj), ptr(zg), ptr(lens), B, T, t, Hp, ptr(h), ptr(o['hprev']), ptr(o['G']), ptr(o['R']),
                                           ptr(o['RH']), st), "cham_gru_point_gates_fwd")
        zc[:B] = (o['RH'][:B, t].double() @ Wch64).float()
        check(lib.cham_gru_point_out_fwd(ptr(xproj), ptr(zc), ptr(lens), B, T, t, Hp, ptr(o['G']), ptr(o['hprev']), ptr(h), ptr(o['out']),
                                         ptr(o['Cc']), st), "cham_gru_point_out_fwd")
    carry = nan(Hp); carry[:B] = 0
    dzc, drh, dzs, direct = nan(Hp), nan(Hp), nan(2 * Hp), nan(Hp)
    for t in range(T - 1, -1, -1):
        check(lib.cham_gru_point_c_bwd(ptr(dout), ptr(carry), ptr(lens), B, T, t, Hp, ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']),
                                       ptr(o['dxproj']), ptr(dzc), ptr(dzs), ptr(direct), st), "cham_gru_point_c_bwd")
        drh[:B] = (dzc[:B].double() @ Wch64.t()).float()
        check(lib.cham_gru_point_r_bwd(ptr(drh), ptr(lens), B, T, t, Hp, ptr(o['hprev']), ptr(o['R']), ptr(o['dxproj']), ptr(dzs),
                                       ptr(direct), st), "cham_gru_point_r_bwd")
        carry[:B] = (direct[:B].double() + dzs[:B].double() @ Wgh64.t()).float()
    torch.cuda.synchronize()
    for name, a in (('h', h), ('dzc', dzc), ('dzs', dzs), ('direct', direct)):       # the per-step buffers too: nothing beyond row B
        assert torch.isnan(a[B:]).all(), "%s written beyond row B" % name
        assert torch.isfinite(a[:B]).all(), "%s not fully written" % name
    return o.numpy()


def _run_fused(gpu, Hp, inp):
    """cham_rnn_fwd / cham_rnn_bwd with cell_kind 1 on the same inputs (Hp <= 384)."""
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    B, T = inp['dout'].shape[:2]
    xproj, lens, dout = _dev(gpu, inp['xproj']), _dev(gpu, inp['lengths']), _dev(gpu, inp['dout'])
    Wh, Wch = inp['Wh'], inp['Wch']
    W = _dev(gpu, np.concatenate([Wh.ravel(), Wch.ravel()]))
    WT = _dev(gpu, np.concatenate([Wh.T.ravel(), Wch.T.ravel()]))
    o = _Outputs(gpu, B, T, dict({k: Hp for k in KEYS}, dxproj=3 * Hp))
    check(lib.cham_rnn_fwd(1, ptr(xproj), ptr(W), ptr(lens), B, T, Hp, ptr(o['out']), ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']),
                           ptr(o['R']), ptr(o['RH']), _stream()), "cham_rnn_fwd")
    check(lib.cham_rnn_bwd(1, ptr(dout), ptr(WT), ptr(lens), B, T, Hp, ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']), ptr(o['R']),
                           ptr(o['dxproj']), _stream()), "cham_rnn_bwd")
    torch.cuda.synchronize()
    return o.numpy()


def _check(Hp, inp, got, ref, what):
    """The bound per array, the exact zeros, and the worst error (printed for the record)."""
    errs = {}
    assert set(got) == set(ref)
    for k, r in ref.items():
        assert np.isfinite(got[k]).all(), "%s: %s is not finite" % (what, k)
        errs[k] = rel_err(got[k], r)
    print("%s: worst %.2e %s" % (what, max(errs.values()), {k: float('%.2e' % v) for k, v in errs.items()}))
    assert max(errs.values()) <= REL_BOUND, (what, errs)
    B, T = inp['dout'].shape[:2]
    H = inp['H']
    beyond = np.arange(T)[None, :] >= inp['lengths'][:, None]
    assert not got['out'][beyond].any(), "%s: out is not zero beyond a session's length" % what
    assert not got['dxproj'][beyond].any(), "%s: dxproj is not zero beyond a session's length" % what
    for k in ('out', 'hprev', 'Cc', 'RH'):
        assert not got[k][..., H:].any(), "%s: pad lanes of %s are not zero" % (what, k)
    assert not got['dxproj'].reshape(B, T, 3, Hp)[..., H:].any(), "%s: pad lanes of dxproj are not zero" % what
    return errs


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s differs between two runs" % (what, k)


def _reference(inp):
    return kernel_reference('gru', inp['xproj'], inp['lengths'], inp['Wh'], inp['Wch'], inp['dout'])


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("Hp", POINT_HP)
def test_gru_point_kernels_match_float64_bptt(gpu, Hp, B, T):
    inp = padded_inputs('gru', Hp, B, T, seed=5 * Hp + B + T)
    got = _run_point(gpu, Hp, inp)
    _same(got, _run_point(gpu, Hp, inp), "GRU point Hp %d" % Hp)
    _check(Hp, inp, got, _reference(inp), "GRU point Hp %d B %d T %d" % (Hp, B, T))


def test_gru_point_kernels_saturated_gates(gpu):
    """xproj x 30 with +-120 planted in every column block: the rcp / exp sigmoid and both branches of cham_tanhf far out (exp overflows
    to inf) stay finite and within the bound."""
    Hp, B, T = 640, 33, 7
    inp = padded_inputs('gru', Hp, B, T, seed=Hp + 1, x_scale=0.7 * 30)
    x = inp['xproj'].reshape(B, T, -1, Hp)
    x[..., :4], x[..., 4:8] = -120.0, 120.0
    _check(Hp, inp, _run_point(gpu, Hp, inp), _reference(inp), "GRU point Hp %d saturated" % Hp)


def test_gru_point_and_fused_kernels_agree_with_the_reference_at_hp_384(gpu):
    """Hp 384, where both paths exist: each meets the bound on the same inputs."""
    Hp, B, T = 384, 70, 30
    inp = padded_inputs('gru', Hp, B, T, seed=384)
    ref = _reference(inp)
    _check(Hp, inp, _run_point(gpu, Hp, inp), ref, "GRU point Hp 384 B %d T %d" % (B, T))
    _check(Hp, inp, _run_fused(gpu, Hp, inp), ref, "GRU fused Hp 384 B %d T %d" % (B, T))


def test_gru_point_argument_errors(gpu):
    """NULL pointers and t outside [0, T) return a negative code and launch nothing (the buffers are far too small for a launch)."""
    from chameleon_recsys_amd._lib import ptr
    lib = _lib_()
    x = torch.zeros(64, device=gpu)
    p, st = ptr(x), _stream()
    B, T, Hp = 32, 4, 512
    for t in (-1, T, T + 3):
        assert lib.cham_gru_point_gates_fwd(p, p, p, B, T, t, Hp, p, p, p, p, p, st) < 0
        assert lib.cham_gru_point_out_fwd(p, p, p, B, T, t, Hp, p, p, p, p, p, st) < 0
        assert lib.cham_gru_point_c_bwd(p, p, p, B, T, t, Hp, p, p, p, p, p, p, p, st) < 0
        assert lib.cham_gru_point_r_bwd(p, p, B, T, t, Hp, p, p, p, p, p, st) < 0
    for i in (0, 1, 2, 7, 8, 9, 10, 11):
        a = [p, p, p, B, T, 0, Hp, p, p, p, p, p]; a[i] = None
        assert lib.cham_gru_point_gates_fwd(*a, st) < 0, i
        a = [p, p, p, B, T, 0, Hp, p, p, p, p, p]; a[i] = None
        assert lib.cham_gru_point_out_fwd(*a, st) < 0, i
    for i in (0, 1, 2, 7, 8, 9, 10, 11, 12, 13):
        a = [p, p, p, B, T, 0, Hp, p, p, p, p, p, p, p]; a[i] = None
        assert lib.cham_gru_point_c_bwd(*a, st) < 0, i
    for i in (0, 1, 6, 7, 8, 9, 10):
        a = [p, p, B, T, 0, Hp, p, p, p, p, p]; a[i] = None
        assert lib.cham_gru_point_r_bwd(*a, st) < 0, i
    assert lib.cham_gru_point_gates_fwd(p, p, p, 0, T, 0, Hp, p, p, p, p, p, st) < 0          # B = 0
    assert lib.cham_gru_point_c_bwd(p, p, p, B, 0, 0, Hp, p, p, p, p, p, p, p, st) < 0        # T = 0
    torch.cuda.synchronize()
    assert not x.any()
