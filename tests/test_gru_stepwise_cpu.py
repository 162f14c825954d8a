"""The step-wise GRU (rnn_units above 384): the layout switch, and the algebra of its four per-step stages on the CPU.

`four_stage` restates in numpy float32 what the four point kernels of csrc/rnn.hip compute per time step (cham_gru_point_gates_fwd /
_out_fwd forward, _c_bwd / _r_bwd backward; include/chameleon_nar.h), with the recurrent products formed in float64 and rounded to fp32 -
exactly what tests/test_gru_point_gpu.py feeds the kernels.  It must meet the kernels' bound against the float64 BPTT reference
(tests/rnn_reference.py), and the bound must catch a dropped `drh r` term of the state gradient: this pins the algebra the GPU test
relies on.  Worst relative error of the restatement over all widths, shapes and arrays on one CPU: 2.2e-7; the mutant: 0.30 - 0.42."""
import numpy as np
import pytest

from chameleon_recsys_amd.nar import synthetic
from chameleon_recsys_amd.nar.layout import ParamLayout
from tests.rnn_reference import REL_BOUND, kernel_reference, padded_inputs, rel_err

SHAPES = [(1, 1), (33, 7), (70, 30)]
WIDTHS = [512, 640, 1024]
f32 = np.float32


def _layout(rnn_units, cell):
    p = synthetic.default_params(200, 16, C=128, H=rnn_units, rnn_cell=cell)
    return ParamLayout(p['session_features_config'], p['articles_features_config'], 200, 16, 128, rnn_units, 1, cell)


@pytest.mark.parametrize("units,Hp", [(500, 512), (600, 640), (1000, 1024)])
def test_wide_gru_layout_is_stepwise(units, Hp):
    L = _layout(units, 'gru')
    assert L.Hp == Hp and L.rnn_stepwise and L.NG == 3
    assert L.entries['rnn0/Wh'].shape == (Hp, 2 * Hp) and L.entries['rnn0/Wch'].shape == (Hp, Hp)


def test_stepwise_thresholds_per_cell():
    assert not _layout(384, 'gru').rnn_stepwise           # the fused kernels keep every width they had
    assert not _layout(512, 'ugrnn').rnn_stepwise
    assert _layout(600, 'ugrnn').rnn_stepwise
    assert _layout(385, 'gru').rnn_stepwise               # Hp 512: fused for UGRNN, step-wise for GRU


def _sig(x):
    return (f32(1) / (f32(1) + np.exp(-x, dtype=f32))).astype(f32)


def _mm(a, w):
    """The recurrent product as the GPU test forms it: float64, rounded to fp32."""
    return (a.astype(np.float64) @ w.astype(np.float64)).astype(f32)


def four_stage(inp, drop_direct_r=False):
    """out, hprev, G, Cc, R, RH, dxproj of the four stages, float32.  drop_direct_r: the mutant that leaves drh r out of `direct`."""
    xproj, Wgh, Wch, dout, lens = inp['xproj'], inp['Wh'], inp['Wch'], inp['dout'], inp['lengths']
    B, T, Hp = dout.shape
    x = xproj.reshape(B, T, 3, Hp)
    o = {k: np.full((B, T, Hp), np.nan, f32) for k in ('out', 'hprev', 'G', 'Cc', 'R', 'RH')}
    dx = np.full((B, T, 3, Hp), np.nan, f32)
    h = np.zeros((B, Hp), f32)
    for t in range(T):
        valid = (t < lens)[:, None]
        zg = _mm(h, Wgh)                                                  # GEMM 1
        r, u = _sig(zg[:, :Hp] + x[:, t, 0]), _sig(zg[:, Hp:] + x[:, t, 1])          # gates_fwd
        o['hprev'][:, t], o['R'][:, t], o['G'][:, t], o['RH'][:, t] = h, r, u, r * h
        zc = _mm(o['RH'][:, t], Wch)                                      # GEMM 2
        c = np.tanh(zc + x[:, t, 2], dtype=f32)                           # out_fwd
        hn = u * h + (f32(1) - u) * c
        o['out'][:, t], o['Cc'][:, t] = np.where(valid, hn, f32(0)), c
        h = np.where(valid, hn, h)
    carry = np.zeros((B, Hp), f32)
    for t in range(T - 1, -1, -1):
        valid = (t < lens)[:, None]
        hp, u, c, r = o['hprev'][:, t], o['G'][:, t], o['Cc'][:, t], o['R'][:, t]
        dh = dout[:, t] + carry                                           # c_bwd
        dzu = np.where(valid, dh * (hp - c) * u * (f32(1) - u), f32(0))
        dzc = np.where(valid, dh * (f32(1) - u) * (f32(1) - c * c), f32(0))
        direct = np.where(valid, dh * u, carry)
        dx[:, t, 1], dx[:, t, 2] = dzu, dzc
        drh = _mm(dzc, Wch.T)                                             # GEMM 3
        dzr = np.where(valid, drh * hp * r * (f32(1) - r), f32(0))        # r_bwd
        if not drop_direct_r:
            direct = np.where(valid, direct + drh * r, direct)
        dx[:, t, 0] = dzr
        dzs = np.concatenate([dzr, dzu], 1)
        carry = (direct.astype(np.float64) + dzs.astype(np.float64) @ Wgh.T.astype(np.float64)).astype(f32)      # copy + GEMM 4
    o['dxproj'] = dx.reshape(B, T, 3 * Hp)
    assert all(a.dtype == f32 for a in o.values())
    return o


_cases = {}


def _case(Hp, B, T):
    """Inputs and float64 reference of one (width, shape), computed once for the restatement and the mutant."""
    if (Hp, B, T) not in _cases:
        inp = padded_inputs('gru', Hp, B, T, seed=5 * Hp + B + T)
        _cases[(Hp, B, T)] = (inp, kernel_reference('gru', inp['xproj'], inp['lengths'], inp['Wh'], inp['Wch'], inp['dout']))
    return _cases[(Hp, B, T)]


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("Hp", WIDTHS)
def test_four_stage_restatement_matches_float64_bptt(Hp, B, T):
    inp, ref = _case(Hp, B, T)
    got = four_stage(inp)
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print("four-stage Hp %d B %d T %d: worst %.2e" % (Hp, B, T, max(errs.values())))
    assert set(got) == set(ref) and all(np.isfinite(a).all() for a in got.values())
    assert max(errs.values()) <= REL_BOUND, errs
    beyond = np.arange(T)[None, :] >= inp['lengths'][:, None]
    assert not got['out'][beyond].any() and not got['dxproj'][beyond].any()


@pytest.mark.parametrize("B,T", SHAPES[1:])              # (1, 1) has no recurrence: the carry is never read
@pytest.mark.parametrize("Hp", WIDTHS)
def test_bound_catches_a_dropped_reset_path(Hp, B, T):
    inp, ref = _case(Hp, B, T)
    err = rel_err(four_stage(inp, drop_direct_r=True)['dxproj'], ref['dxproj'])
    print("mutant (no drh r in direct) Hp %d B %d T %d: %.2e" % (Hp, B, T, err))
    assert err > REL_BOUND, err
