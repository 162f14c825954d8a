"""The two step-wise LSTM kernels of csrc/rnn.hip (cham_lstm_point_fwd / _bwd) against the float64 BPTT reference (tests/lstm_reference.py),
driven per time step as nar/recurrent.py (StepwiseLstm) drives them: zh = h W_h by cham_gemm_f32, the forward kernel; the backward kernel,
the copy carry = direct and the accumulating cham_gemm_f32 carry += dzs W_h^T.  tests/test_lstm_cpu.py pins this algebra on the CPU and
shows that the bound catches a dropped cell-state gradient.

Per array (out, hprev, cprev, Gi, Gj, Gf, Go, TC, dxproj) max |hip - ref| <= 2e-5 max |ref|.  Exactly zero: out and dxproj beyond a session's
length and the pad lanes (H = Hp - 17) of out, hprev, cprev, Gj, TC and dxproj.  Every plane is written at every t (the NaN fill is gone
everywhere in rows < B), rows >= B of the NaN-filled, 32-row-padded buffers stay NaN, and two runs are bit-identical.

Worst relative error observed on one MI355X, over all arrays:   Hp 128 B 5 T 3: 1.9e-7   Hp 384 B 37 T 6: 4.8e-7   Hp 1024 B 8 T 4: 6.8e-7
"""
import numpy as np
import pytest
import torch

from tests.lstm_reference import REL_BOUND, SAVED, kernel_reference, padded_inputs, rel_err

pytestmark = pytest.mark.gpu

# (Hp, B, T): a partial last block (5 x 128 = 2.5 blocks); a width that is no power of two, several blocks, sessions of every length; the
# widest layout.  The smallest shapes at which masking, either carry, a block tail or an offset can go wrong.
SHAPES = [(128, 5, 3), (384, 37, 6), (1024, 8, 4)]
PLANES = ('out',) + SAVED


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _run(gpu, Hp, inp):
    """One layer forward + backward.  Every buffer the kernels write is NaN-filled and padded to whole 32-row groups; returns the rows < B
    as numpy, after checking that the rows beyond came back untouched."""
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    B, T = inp['dout'].shape[:2]
    Bp = (B + 31) // 32 * 32
    st = _stream()
    xproj, lens, dout, Wh = (_dev(gpu, inp[k]) for k in ('xproj', 'lengths', 'dout', 'Wh'))
    nan = lambda *s: torch.full(s, float('nan'), device=gpu)
    o = {k: nan(Bp, T, Hp) for k in PLANES}
    o['dxproj'] = nan(Bp, T, 4 * Hp)
    step = dict(h=nan(Bp, Hp), c=nan(Bp, Hp), zh=nan(Bp, 4 * Hp), carry=nan(Bp, Hp), carry_c=nan(Bp, Hp), dzs=nan(Bp, 4 * Hp), direct=nan(Bp, Hp))
    h, c, zh, carry, carry_c, dzs, direct = (step[k] for k in ('h', 'c', 'zh', 'carry', 'carry_c', 'dzs', 'direct'))

    def gemm(A, C, N, K, transB, accumulate):      # C [B, N] (+)= A [B, K] op(W_h), W_h stored [Hp, 4Hp]
        check(lib.cham_gemm_f32(ptr(A), K, 0, ptr(Wh), 4 * Hp, transB, ptr(C), N, B, N, K, None, 0, None, 0, 0, None, 0, 1, accumulate, None, 0,
                                1, st), "cham_gemm_f32")

    h[:B] = 0; c[:B] = 0
    for t in range(T):
        gemm(h, zh, 4 * Hp, Hp, 0, 0)
        check(lib.cham_lstm_point_fwd(ptr(xproj), ptr(zh), ptr(lens), B, T, t, Hp, ptr(h), ptr(c), ptr(o['out']), ptr(o['hprev']), ptr(o['cprev']),
                                      ptr(o['Gi']), ptr(o['Gj']), ptr(o['Gf']), ptr(o['Go']), ptr(o['TC']), st), "cham_lstm_point_fwd")
    carry[:B] = 0; carry_c[:B] = 0
    for t in range(T - 1, -1, -1):
        check(lib.cham_lstm_point_bwd(ptr(dout), ptr(carry), ptr(carry_c), ptr(lens), B, T, t, Hp, ptr(o['cprev']), ptr(o['Gi']), ptr(o['Gj']),
                                      ptr(o['Gf']), ptr(o['Go']), ptr(o['TC']), ptr(o['dxproj']), ptr(dzs), ptr(direct), st), "cham_lstm_point_bwd")
        carry[:B] = direct[:B]
        gemm(dzs, carry, Hp, 4 * Hp, 1, 1)
    torch.cuda.synchronize()
    for name, a in list(step.items()) + list(o.items()):
        assert torch.isnan(a[B:]).all(), "%s written beyond row B" % name
        assert torch.isfinite(a[:B]).all(), "%s not fully written" % name          # the planes: at every t, also beyond the length
    return {k: v[:B].cpu().numpy() for k, v in o.items()}


_cases = {}


def _case(gpu, Hp, B, T):
    """Inputs, the float64 reference and one run of the kernels per shape, shared by the tests below."""
    if (Hp, B, T) not in _cases:
        inp = padded_inputs(Hp, B, T, seed=5 * Hp + B + T)
        _cases[(Hp, B, T)] = (inp, kernel_reference(inp['xproj'], inp['lengths'], inp['Wh'], inp['dout']), _run(gpu, Hp, inp))
    return _cases[(Hp, B, T)]


@pytest.mark.parametrize("Hp,B,T", SHAPES)
def test_lstm_point_kernels_match_float64_bptt(gpu, Hp, B, T):
    inp, ref, got = _case(gpu, Hp, B, T)
    what = "LSTM point Hp %d B %d T %d" % (Hp, B, T)
    assert set(got) == set(ref) == set(PLANES) | {'dxproj'}
    errs = {k: rel_err(got[k], r) for k, r in ref.items()}
    print("%s: worst %.2e %s" % (what, max(errs.values()), {k: float('%.2e' % v) for k, v in errs.items()}))
    assert max(errs.values()) <= REL_BOUND, (what, errs)


@pytest.mark.parametrize("Hp,B,T", SHAPES)
def test_lstm_point_kernels_mask_carry_and_pad_exactly(gpu, Hp, B, T):
    inp, ref, got = _case(gpu, Hp, B, T)
    lens, H = inp['lengths'], inp['H']
    beyond = np.arange(T)[None, :] >= lens[:, None]
    assert beyond.any() and (~beyond).any()
    assert not got['out'][beyond].any() and not got['dxproj'][beyond].any()
    for k in ('out', 'hprev', 'cprev', 'Gj', 'TC'):
        assert not got[k][..., H:].any(), "pad lanes of %s are not zero" % k
    assert not got['dxproj'].reshape(B, T, 4, Hp)[..., H:].any(), "pad lanes of dxproj are not zero"
    # planes are written beyond the length, from the carried states: hprev / cprev repeat there, and equal the last valid step's h' / c'
    for b in range(B):
        n = int(lens[b])
        for t in range(max(n, 1), T):
            for k in ('hprev', 'cprev'):
                assert np.array_equal(got[k][b, t], got[k][b, max(n, 1)] if n else np.zeros(Hp, np.float32)), (k, b, t)
        if 0 < n < T:
            assert np.array_equal(got['hprev'][b, n], got['out'][b, n - 1])
        assert np.isfinite(got['Go'][b]).all() and (got['Gf'][b] > 0).all()


@pytest.mark.parametrize("Hp,B,T", SHAPES)
def test_lstm_point_kernels_two_runs_are_bit_identical(gpu, Hp, B, T):
    inp, _, got = _case(gpu, Hp, B, T)
    again = _run(gpu, Hp, inp)
    for k in got:
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), "%s differs between two runs" % k


def test_lstm_point_argument_errors(gpu):
    """NULL pointers and t outside [0, T) return a negative code and launch nothing (the buffers are far too small for a launch)."""
    from chameleon_recsys_amd._lib import ptr
    lib = _lib_()
    x = torch.zeros(64, device=gpu)
    p, st = ptr(x), _stream()
    B, T, Hp = 32, 4, 128
    fwd = lambda t=0, B=B, T=T, Hp=Hp: [p, p, p, B, T, t, Hp] + [p] * 10
    bwd = lambda t=0, B=B, T=T, Hp=Hp: [p, p, p, p, B, T, t, Hp] + [p] * 9
    for t in (-1, T, T + 3):
        assert lib.cham_lstm_point_fwd(*fwd(t), st) < 0
        assert lib.cham_lstm_point_bwd(*bwd(t), st) < 0
    for i in [0, 1, 2] + list(range(7, 17)):
        a = fwd(); a[i] = None
        assert lib.cham_lstm_point_fwd(*a, st) < 0, i
    for i in [0, 1, 2, 3] + list(range(8, 17)):
        a = bwd(); a[i] = None
        assert lib.cham_lstm_point_bwd(*a, st) < 0, i
    for kw in (dict(B=0), dict(T=0), dict(Hp=0)):
        assert lib.cham_lstm_point_fwd(*fwd(**kw), st) < 0
        assert lib.cham_lstm_point_bwd(*bwd(**kw), st) < 0
    torch.cuda.synchronize()
    assert not x.any()
