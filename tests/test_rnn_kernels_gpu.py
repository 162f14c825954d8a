"""Every recurrent kernel of csrc/rnn.hip and csrc/rnn_coop.hip against the float64 BPTT reference (tests/rnn_reference.py), fed the
kernels' own layout: xproj in, out / hprev / G / Cc (GRU: R / RH) and dxproj out.

Per array max |hip - ref| <= 2e-5 max |ref| (tests/test_rnn_reference_cpu.py shows that the bound catches a forget-bias slip, a wrong
reset order, a length off by one, a dropped state carry, a skipped k-step, a wrong tile offset and bf16 rounding of h).  Exactly zero:
out and dxproj beyond a session's length and the pad lanes (H = Hp - 17) of out, hprev, Cc, RH and dxproj.  Two runs are bit-identical,
and no kernel writes the rows of a workgroup's partial group beyond B.

Worst relative error observed on one MI355X, over the three shapes and all arrays (saturated inputs in brackets).  The fp32 evaluation
of the same cells on the CPU reaches 4e-7 to 7e-7 at these shapes: the approximate sigmoid / tanh add little.
    UGRNN  Hp 128 4.2e-7 (6.0e-7)   Hp 256 7.4e-7 (1.5e-6)   Hp 384 8.7e-7 (1.3e-6)   Hp 512 1.1e-6 (2.0e-6)
    GRU    Hp 128 3.2e-7 (3.6e-7)   Hp 256 6.3e-7 (6.8e-7)   Hp 384 6.8e-7 (8.7e-7)
    cooperative UGRNN Hp 256 3.3e-7;  step-wise UGRNN Hp 512 2.4e-7, Hp 640 3.2e-7, Hp 1024 2.4e-7
"""
import numpy as np
import pytest
import torch

from tests.rnn_reference import REL_BOUND, kernel_reference, padded_inputs, rel_err

pytestmark = pytest.mark.gpu

# every (cell, Hp) instance of the switches in cham_rnn_fwd / cham_rnn_bwd (csrc/rnn.hip): must match them
FUSED = [("ugrnn", 128), ("ugrnn", 256), ("ugrnn", 384), ("ugrnn", 512), ("gru", 128), ("gru", 256), ("gru", 384)]
# (B, T): one row in a 32-row group and no recurrence; two workgroups, the second holding one row; three workgroups at Adressa's seq_len
SHAPES = [(1, 1), (33, 7), (70, 30)]
POINT_HP = [512, 640, 1024]
CELL = {"ugrnn": 0, "gru": 1}


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


class _Outputs:
    """NaN-filled output arrays [B, T, width] on a buffer padded to whole 32-row groups: every element the kernel must write is checked,
    and the rows past B (the rest of the last workgroup's group) must come back untouched."""

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


def _weights(gpu, cell, inp):
    """Wh as the kernels take it (GRU: W_ch directly behind W_gh) and WhT as nar_model.py builds it for the backward:
    transpose(W_gh), followed for GRU by transpose(W_ch)."""
    Wh, Wch = inp['Wh'], inp['Wch']
    if cell == 'ugrnn':
        return _dev(gpu, Wh), _dev(gpu, Wh.T)
    return _dev(gpu, np.concatenate([Wh.ravel(), Wch.ravel()])), _dev(gpu, np.concatenate([Wh.T.ravel(), Wch.T.ravel()]))


def _run_fused(gpu, cell, Hp, inp):
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    B, T = inp['dout'].shape[:2]
    ng = 2 if cell == 'ugrnn' else 3
    xproj, lens, dout = _dev(gpu, inp['xproj']), _dev(gpu, inp['lengths']), _dev(gpu, inp['dout'])
    Wh, WhT = _weights(gpu, cell, inp)
    keys = ['out', 'hprev', 'G', 'Cc'] + (['R', 'RH'] if cell == 'gru' else [])
    o = _Outputs(gpu, B, T, dict({k: Hp for k in keys}, dxproj=ng * Hp))
    R, RH = (o['R'], o['RH']) if cell == 'gru' else (None, None)
    check(lib.cham_rnn_fwd(CELL[cell], ptr(xproj), ptr(Wh), ptr(lens), B, T, Hp, ptr(o['out']), ptr(o['hprev']), ptr(o['G']),
                           ptr(o['Cc']), ptr(R), ptr(RH), _stream()), "cham_rnn_fwd")
    # the backward reads the forward's own saved activations, as the model does
    check(lib.cham_rnn_bwd(CELL[cell], ptr(dout), ptr(WhT), ptr(lens), B, T, Hp, ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']), ptr(R),
                           ptr(o['dxproj']), _stream()), "cham_rnn_bwd")
    torch.cuda.synchronize()
    return o.numpy()


def _run_coop(gpu, inp):
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    Hp = 256
    B, T = inp['dout'].shape[:2]
    xproj, lens, dout, Wh = (_dev(gpu, inp[k]) for k in ('xproj', 'lengths', 'dout', 'Wh'))
    o = _Outputs(gpu, B, T, dict(out=Hp, hprev=Hp, G=Hp, Cc=Hp, dxproj=2 * Hp))
    nb = lib.cham_rnn_coop_workspace_bytes(B, Hp)
    assert nb > 0
    ws = torch.zeros(nb, dtype=torch.uint8, device=gpu)
    check(lib.cham_ugrnn_fwd_coop(ptr(xproj), ptr(Wh), ptr(lens), B, T, Hp, ptr(o['out']), ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']),
                                  ptr(ws), nb, _stream()), "cham_ugrnn_fwd_coop")
    check(lib.cham_ugrnn_bwd_coop(ptr(dout), ptr(Wh), ptr(lens), B, T, Hp, ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']), ptr(o['dxproj']),
                                  ptr(ws), nb, _stream()), "cham_ugrnn_bwd_coop")
    assert lib.cham_rnn_coop_timeouts(ptr(ws), B, Hp, _stream()) == 0, "a cooperating workgroup gave up its spin"
    torch.cuda.synchronize()
    return o.numpy()


def _run_point(gpu, Hp, inp):
    """The step-wise UGRNN as nar_model.py runs it (forward ~1335, backward ~1673), with the recurrent products h W_h and dzs W_h^T
    computed in float64 on the device and rounded to fp32, so that only the gate kernels are under test."""
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    B, T = inp['dout'].shape[:2]
    xproj, lens, dout, Wh = (_dev(gpu, inp[k]) for k in ('xproj', 'lengths', 'dout', 'Wh'))
    Wh64 = Wh.double()
    o = _Outputs(gpu, B, T, dict(out=Hp, hprev=Hp, G=Hp, Cc=Hp, dxproj=2 * Hp))
    h = torch.zeros(B, Hp, device=gpu)
    zh = torch.empty(B, 2 * Hp, device=gpu)
    for t in range(T):
        zh.copy_(h.double() @ Wh64)
        check(lib.cham_ugrnn_point_fwd(ptr(xproj), ptr(zh), ptr(lens), B, T, t, Hp, ptr(h), ptr(o['out']), ptr(o['hprev']), ptr(o['G']),
                                       ptr(o['Cc']), _stream()), "cham_ugrnn_point_fwd")
    carry = torch.zeros(B, Hp, device=gpu)
    dzs = torch.full((B, 2 * Hp), float('nan'), device=gpu)
    direct = torch.full((B, Hp), float('nan'), device=gpu)
    for t in range(T - 1, -1, -1):
        check(lib.cham_ugrnn_point_bwd(ptr(dout), ptr(carry), ptr(lens), B, T, t, Hp, ptr(o['hprev']), ptr(o['G']), ptr(o['Cc']),
                                       ptr(o['dxproj']), ptr(dzs), ptr(direct), _stream()), "cham_ugrnn_point_bwd")
        carry.copy_(direct.double() + dzs.double() @ Wh64.t())
    torch.cuda.synchronize()
    return o.numpy()


def _check(cell, Hp, inp, got, ref, what):
    """The bound per array, the exact zeros, and the worst error (printed for the record)."""
    errs = {}
    for k, r in ref.items():
        assert np.isfinite(got[k]).all(), "%s: %s is not finite" % (what, k)
        errs[k] = rel_err(got[k], r)
    print("%s: worst %.2e %s" % (what, max(errs.values()), {k: float('%.2e' % v) for k, v in errs.items()}))
    assert max(errs.values()) <= REL_BOUND, (what, errs)
    B, T = inp['dout'].shape[:2]
    H, ng = inp['H'], got['dxproj'].shape[2] // Hp
    beyond = np.arange(T)[None, :] >= inp['lengths'][:, None]
    assert not got['out'][beyond].any(), "%s: out is not zero beyond a session's length" % what
    assert not got['dxproj'][beyond].any(), "%s: dxproj is not zero beyond a session's length" % what
    for k in ('out', 'hprev', 'Cc', 'RH'):
        if k in got:
            assert not got[k][..., H:].any(), "%s: pad lanes of %s are not zero" % (what, k)
    assert not got['dxproj'].reshape(B, T, ng, Hp)[..., H:].any(), "%s: pad lanes of dxproj are not zero" % what
    return errs


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), "%s: %s differs between two runs" % (what, k)


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("cell,Hp", FUSED)
def test_fused_kernels_match_float64_bptt(gpu, cell, Hp, B, T):
    inp = padded_inputs(cell, Hp, B, T, seed=Hp + 7 * B + T)
    got = _run_fused(gpu, cell, Hp, inp)
    _same(got, _run_fused(gpu, cell, Hp, inp), "%s Hp %d" % (cell, Hp))
    ref = kernel_reference(cell, inp['xproj'], inp['lengths'], inp['Wh'], inp['Wch'], inp['dout'])
    _check(cell, Hp, inp, got, ref, "%s Hp %d B %d T %d" % (cell, Hp, B, T))


@pytest.mark.parametrize("cell,Hp", FUSED)
def test_fused_kernels_saturated_gates(gpu, cell, Hp):
    """xproj x 30: the rcp / exp sigmoid and both branches of cham_tanhf far out (exp overflows to inf) stay finite and within the bound."""
    B, T = 33, 7
    inp = padded_inputs(cell, Hp, B, T, seed=Hp + 1, x_scale=0.7 * 30)
    x = inp['xproj'].reshape(B, T, -1, Hp)
    x[..., :4], x[..., 4:8] = -120.0, 120.0        # in every column block: exp(-z) of the sigmoid overflows too, not only tanh's exp(2|z|)
    got = _run_fused(gpu, cell, Hp, inp)
    ref = kernel_reference(cell, inp['xproj'], inp['lengths'], inp['Wh'], inp['Wch'], inp['dout'])
    _check(cell, Hp, inp, got, ref, "%s Hp %d saturated" % (cell, Hp))


@pytest.mark.parametrize("B,T", SHAPES)
def test_coop_ugrnn_matches_float64_bptt(gpu, B, T):
    inp = padded_inputs('ugrnn', 256, B, T, seed=11 * B + T)
    got = _run_coop(gpu, inp)
    _same(got, _run_coop(gpu, inp), "coop")
    ref = kernel_reference('ugrnn', inp['xproj'], inp['lengths'], inp['Wh'], None, inp['dout'])
    _check('ugrnn', 256, inp, got, ref, "coop B %d T %d" % (B, T))


@pytest.mark.parametrize("B,T", SHAPES)
@pytest.mark.parametrize("Hp", POINT_HP)
def test_point_kernels_match_float64_bptt(gpu, Hp, B, T):
    inp = padded_inputs('ugrnn', Hp, B, T, seed=3 * Hp + B + T)
    got = _run_point(gpu, Hp, inp)
    _same(got, _run_point(gpu, Hp, inp), "point Hp %d" % Hp)
    ref = kernel_reference('ugrnn', inp['xproj'], inp['lengths'], inp['Wh'], None, inp['dout'])
    _check('ugrnn', Hp, inp, got, ref, "point Hp %d B %d T %d" % (Hp, B, T))
    if Hp == 512:          # the fused NT = 4 kernel on the same inputs
        _check('ugrnn', Hp, inp, _run_fused(gpu, 'ugrnn', Hp, inp), ref, "fused Hp 512 B %d T %d (point inputs)" % (B, T))


@pytest.mark.parametrize("rows,cols", [(128, 256), (384, 768), (512, 1024), (640, 1280), (384, 384), (33, 70), (70, 33), (1, 1)])
def test_transpose_is_exact(gpu, rows, cols):
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    a = torch.randn(rows, cols, device=gpu)
    out = torch.full((cols, rows), float('nan'), device=gpu)
    check(lib.cham_transpose_f32(ptr(a), rows, cols, ptr(out), _stream()), "cham_transpose_f32")
    torch.cuda.synchronize()
    assert torch.equal(out, a.t())


def _rows(gpu, n, words, g):
    """n rows of `words` 32-bit words (2 words: int64 values with both halves set)."""
    if words == 2:
        return torch.randint(-2 ** 62, 2 ** 62, (n,), dtype=torch.int64, device=gpu, generator=g)
    return torch.randint(-2 ** 31, 2 ** 31 - 1, (n, words), dtype=torch.int32, device=gpu, generator=g)


@pytest.mark.parametrize("words", [1, 2, 384])
def test_rows_gather_scatter_are_exact_past_the_grid_cap(gpu, words):
    """n_rows * words above 8192 blocks x 256 threads = 2,097,152 words: the grid-stride loop covers the tail."""
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib_()
    g = torch.Generator(device=gpu).manual_seed(words)
    n = 2_300_001 // words + 3
    assert n * words > 8192 * 256
    extra = 1001
    src = _rows(gpu, n + extra, words, g)
    pos = torch.randint(0, n + extra, (n,), dtype=torch.int32, device=gpu, generator=g)      # gather: repeats allowed
    dst = torch.zeros_like(src[:n])
    check(lib.cham_rows_gather(ptr(src), ptr(pos), n, words, ptr(dst), _stream()), "cham_rows_gather")
    torch.cuda.synchronize()
    assert torch.equal(dst, src[pos.long()])
    rows = src[:n].clone()
    spos = torch.randperm(n + extra, device=gpu, generator=g)[:n].to(torch.int32)          # scatter: distinct rows
    before = _rows(gpu, n + extra, words, g)
    dst = before.clone()
    check(lib.cham_rows_scatter(ptr(rows), ptr(spos), n, words, ptr(dst), _stream()), "cham_rows_scatter")
    torch.cuda.synchronize()
    want = before.clone()
    want[spos.long()] = rows
    assert torch.equal(dst, want)                       # rows that pos does not name are untouched
    untouched = torch.ones(n + extra, dtype=torch.bool, device=gpu)
    untouched[spos.long()] = False
    assert int(untouched.sum()) == extra and torch.equal(dst[untouched], before[untouched])


def test_rnn_argument_errors(gpu):
    from chameleon_recsys_amd._lib import ptr
    lib = _lib_()
    x = torch.zeros(64, device=gpu)
    p = ptr(x)
    st = _stream()
    assert lib.cham_rnn_fwd(1, p, p, p, 32, 4, 512, p, p, p, p, p, p, st) < 0          # GRU has no Hp 512 instance
    assert lib.cham_rnn_bwd(1, p, p, p, 32, 4, 512, p, p, p, p, p, st) < 0
    assert lib.cham_rnn_fwd(0, p, p, p, 32, 4, 640, p, p, p, p, None, None, st) < 0    # fused UGRNN ends at Hp 512
    assert lib.cham_rnn_bwd(0, p, p, p, 32, 4, 640, p, p, p, None, p, st) < 0
    assert lib.cham_rnn_fwd(2, p, p, p, 32, 4, 128, p, p, p, p, p, p, st) < 0          # cell_kind 2
    assert lib.cham_rnn_bwd(2, p, p, p, 32, 4, 128, p, p, p, p, p, st) < 0
    assert lib.cham_rnn_fwd(0, p, p, p, 0, 4, 128, p, p, p, p, None, None, st) < 0     # B = 0
    assert lib.cham_rnn_bwd(0, p, p, p, 0, 4, 128, p, p, p, None, p, st) < 0
    torch.cuda.synchronize()
