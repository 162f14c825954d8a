"""The bound of tests/test_rnn_kernels_gpu.py (max |hip - ref| <= 2e-5 max |ref| per array) can fail: at the GPU tests' shapes and inputs,
each of seven plausible kernel slips, written into a float64 restatement of the cell, moves some compared array by at least 10x the bound,
while an honest fp32 evaluation stays far inside it.

The restatement (`_direct`) is a plain torch step loop, differentiated by autograd; unmutated it equals tests/rnn_reference.py, which
also pins the identity-padded kernel mapping (xproj in, dxproj out) that the GPU tests rely on."""
import numpy as np
import pytest
import torch

from tests.rnn_reference import REL_BOUND, kernel_reference, padded_inputs, rel_err

SHAPES = [(1, 1), (33, 7), (70, 30)]          # those of tests/test_rnn_kernels_gpu.py
WIDTHS = [("ugrnn", 128), ("ugrnn", 384), ("gru", 128), ("gru", 384)]
K_DROP = 34                                   # k-pair 17 (rows 34, 35 of W_h): one skipped v_mfma_f32_32x32x2_f32 k-step
J_SHIFT = 40                                  # W_h column 40 read from column 41: a tile offset off by one

_CACHE = {}


def _inputs(cell, Hp, B, T):
    key = (cell, Hp, B, T)
    if key not in _CACHE:
        inp = padded_inputs(cell, Hp, B, T, seed=Hp + 7 * B + T)
        _CACHE[key] = inp, kernel_reference(cell, inp['xproj'], inp['lengths'], inp['Wh'], inp['Wch'], inp['dout'])
    return _CACHE[key]


def _direct(cell, inp, dtype=torch.float64, forget_bias=1.0, reset_after=False, reset_state=False, bf16_h=False, lengths=None, Wh=None):
    """The arrays the kernels write (out, hprev, G, Cc, GRU R / RH, dxproj = d sum(out * dout) / d xproj), optionally with one slip."""
    t_ = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x = t_(inp['xproj']).requires_grad_(True)
    Wh = t_(inp['Wh'] if Wh is None else Wh)
    Wch = t_(inp['Wch']) if cell == 'gru' else None
    lens = torch.tensor(inp['lengths'] if lengths is None else lengths, dtype=torch.int64)
    B, T, _ = x.shape
    Hp = Wh.shape[0]
    h = torch.zeros(B, Hp, dtype=dtype)
    keep = {k: [] for k in (['out', 'hprev', 'G', 'Cc'] + (['R', 'RH'] if cell == 'gru' else []))}
    for t in range(T):
        hm = h.to(torch.bfloat16).to(dtype) if bf16_h else h
        if cell == 'ugrnn':
            z = x[:, t] + hm @ Wh
            g, c = torch.sigmoid(z[:, :Hp] + forget_bias), torch.tanh(z[:, Hp:])
        else:
            ru = torch.sigmoid(x[:, t, :2 * Hp] + hm @ Wh)
            r, g = ru[:, :Hp], ru[:, Hp:]
            c = torch.tanh(x[:, t, 2 * Hp:] + (r * (hm @ Wch) if reset_after else (r * hm) @ Wch))
            keep['R'].append(r); keep['RH'].append(r * h)
        hn = g * h + (1 - g) * c
        v = (t < lens)[:, None]
        keep['out'].append(torch.where(v, hn, torch.zeros_like(hn)))
        keep['hprev'].append(h); keep['G'].append(g); keep['Cc'].append(c)
        h = torch.where(v, hn, torch.zeros_like(h) if reset_state else h)
    res = {k: torch.stack(v, 1) for k, v in keep.items()}
    (res['out'] * t_(inp['dout'])).sum().backward()
    res = {k: v.detach().double().numpy() for k, v in res.items()}
    res['dxproj'] = x.grad.double().numpy()
    return res


def _worst(got, ref):
    return max(rel_err(got[k], ref[k]) for k in ref)


def _mutations(cell, inp):
    """(name, needs T >= 2, keyword arguments of _direct)."""
    lens = inp['lengths'].copy(); lens[0] -= 1                      # session 0 has length T
    drop = inp['Wh'].copy(); drop[K_DROP:K_DROP + 2] = 0
    shift = inp['Wh'].copy(); shift[:, J_SHIFT] = shift[:, J_SHIFT + 1]
    m = [("length off by one", False, dict(lengths=lens)),
         ("state reset past the length", True, dict(reset_state=True)),
         ("skipped k-step", True, dict(Wh=drop)),
         ("wrong tile offset", True, dict(Wh=shift)),
         ("h rounded to bf16", True, dict(bf16_h=True))]
    if cell == 'ugrnn':
        m.append(("forget bias 0", False, dict(forget_bias=0.0)))
    else:
        m.append(("reset after the W_ch product", True, dict(reset_after=True)))
    return m


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("cell,Hp", WIDTHS)
def test_direct_restatement_equals_the_reference(cell, Hp, B, T):
    inp, ref = _inputs(cell, Hp, B, T)
    got = _direct(cell, inp)
    assert set(got) == set(ref)
    assert _worst(got, ref) < 1e-12


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("cell,Hp", WIDTHS)
def test_fp32_evaluation_is_far_inside_the_bound(cell, Hp, B, T):
    inp, ref = _inputs(cell, Hp, B, T)
    assert _worst(_direct(cell, inp, dtype=torch.float32), ref) < REL_BOUND / 10


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("cell,Hp", WIDTHS)
def test_every_mutation_breaks_the_bound_tenfold(cell, Hp, B, T):
    inp, ref = _inputs(cell, Hp, B, T)
    worst = {}
    for name, recurrent, kw in _mutations(cell, inp):
        if recurrent and T < 2:
            continue
        worst[name] = _worst(_direct(cell, inp, **kw), ref)
    assert worst and min(worst.values()) >= 10 * REL_BOUND, worst
