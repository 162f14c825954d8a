"""Every entry point of csrc/optim.hip against the float64 references of tests/tail_reference.py: cham_adam_tf / _dev, cham_sumsq_partial,
cham_loss_finalize / _dev, cham_loss_accumulate, cham_accumulate, cham_colsum / cham_colsum_b16 (and cham_colsum_workspace_bytes),
cham_cast_b16, cham_upcast_b16; cham_step_scalars_set / cham_step_scalars_bytes are in tests/test_scorer_tail_gpu.py.

Outputs start as NaN inside guarded allocations, launches are made twice and must repeat bit for bit, and the bounds are 8 x the error of
the same formula in fp32 on the CPU at the same inputs (tests/test_tail_reference_cpu.py: `gpu_bounds`, and the slips that break them
tenfold).  Adam compares p, m AND v: m and v to k of their array's max, the weight as |dp_hip - dp_ref| <= k lr_t + ulp(p).  The scalar
arguments reach a kernel as fp32 (0.999f is 0.99900001287): the reference is evaluated at those values (tail_reference.adam_scalars).
Exact and compared with ==: casts (round-to-nearest-even, ties, signed zeros, the largest finite, denormals), cham_accumulate and
cham_loss_accumulate (one IEEE addition per element), first = 1 over NaN contents, by-value against _dev, run against run.

Float4 alignment (k_adam_tf, k_sumsq_partial, k_accumulate, k_upcast_b16 read their pointers as float4): the entry points check n % 4, not
the pointer.  Decided: no pointer check - the sub-ranges apply_gradients makes begin at rank * (total // world), a multiple of 4 whenever
the length is one, which ParamLayout's padding to 256 guarantees for every world size up to 64 and which the n % 4 check enforces beyond
(tests/test_tail_reference_cpu.py::test_adam_subranges_are_float4_aligned).  Adam runs below on such an offset pointer.

Worst error seen on one MI355X / fp32-CPU error of the same array (the bound is 8 x the latter):
    adam p 1.2e-6 / 7.9e-7 (of lr_t, beyond one ulp of p)   m 6.7e-8 / 6.6e-8   v 9.7e-8 / 8.1e-8
    sum of squares 1.7e-8, loss 1.1e-7 / 1.7e-7   colsum 3.3e-7, colsum_b16 2.1e-7 / 7.7e-6 (numpy adds 70 000 rows one after the other)
Wall time of this file on one MI355X: 5.1 s (41 tests; the n = 8.4 M Adam / accumulate / upcast cases included).
"""
import numpy as np
import pytest
import torch

from tests import tail_reference as R
from tests.test_tail_reference_cpu import bf16_edge_values, colsum_reference, gpu_bounds

pytestmark = pytest.mark.gpu

WORST = {}


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t.bfloat16() if bf16 else t


def _note(name, err, k):
    w = WORST.setdefault(name, [0.0, k])
    w[0] = max(w[0], err)
    print("    %-22s %.2e  (bound %.2e)" % (name, err, k))
    assert err <= k, (name, err, k)


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------
def _adam_run(gpu, lib, inp, n, n_reg, sc, off, dev):
    """One step on the sub-range [off, off + n) of buffers of n + 8 entries, as apply_gradients calls it on flat + 4 a."""
    from chameleon_recsys_amd._lib import check
    pad = lambda a: np.concatenate([np.full(off, 7.0, np.float32), a, np.full(8 - off, 7.0, np.float32)])
    bufs = {k: R.Guarded(gpu, (n + 8,), init=_dev(gpu, pad(inp[k]))) for k in ('p', 'g', 'm', 'v')}
    at = lambda k: bufs[k].ptr() + 4 * off
    if dev:
        rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
        check(lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, 0, 0.0, sc['lr_t'], 4, _st()), "cham_step_scalars_set")
        check(lib.cham_adam_tf_dev(at('p'), at('g'), at('m'), at('v'), n, n_reg, sc['lam'], rec.data_ptr(), sc['b1'], sc['b2'], sc['eps'], _st()),
              "cham_adam_tf_dev")
    else:
        check(lib.cham_adam_tf(at('p'), at('g'), at('m'), at('v'), n, n_reg, sc['lam'], sc['lr_t'], sc['b1'], sc['b2'], sc['eps'], _st()), "cham_adam_tf")
    torch.cuda.synchronize()
    out = {k: v.numpy() for k, v in bufs.items()}
    for k, a in out.items():
        assert (a[:off] == 7.0).all() and (a[off + n:] == 7.0).all(), "%s written outside the sub-range" % k
    assert R.same_bits(out['g'][off:off + n], inp['g']), "the gradient was modified"
    return {k: out[k][off:off + n] for k in ('p', 'm', 'v')}


@pytest.mark.parametrize("case", range(len(R.ADAM_CASES)))
def test_adam_matches_tf_adam_in_float64(gpu, case):
    lib = _lib_()
    n, n_reg, lam, t = R.ADAM_CASES[case]
    print("\nn %d n_reg %d lam %g t %d" % (n, n_reg, lam, t))
    k = gpu_bounds()
    inp, sc = R.adam_inputs(n), R.adam_scalars(R.ADAM_LR, t, lam)
    ref = R.adam_tf(inp['p'], inp['g'], inp['m'], inp['v'], n_reg, **sc)
    off = 4 * (case % 2)
    got = _adam_run(gpu, lib, inp, n, n_reg, sc, off, False)
    for how, other in (("two runs", _adam_run(gpu, lib, inp, n, n_reg, sc, off, False)), ("by value and _dev", _adam_run(gpu, lib, inp, n, n_reg, sc, off, True)),
                       ("two offsets", _adam_run(gpu, lib, inp, n, n_reg, sc, 4 - off, False))):
        for a in got:
            assert R.same_bits(got[a], other[a]), "%s differs between %s" % (a, how)
    _note('adam.p', R.adam_step_err(got['p'], inp['p'], ref['p'], sc['lr_t']), k['adam.p'])
    _note('adam.m', R.rel_err(got['m'], ref['m']), k['adam.m'])
    _note('adam.v', R.rel_err(got['v'], ref['v']), k['adam.v'])
    first = (inp['m'] == 0) & (inp['v'] == 0) & (inp['g'] == 0)
    if n_reg == 0 or lam == 0:
        assert R.same_bits(got['p'][first], inp['p'][first]), "a zero gradient on a first step moved a weight"


def test_adam_argument_errors(gpu):
    lib = _lib_()
    bufs = [R.Guarded(gpu, (16,)) for _ in range(4)]
    p, g, m, v = (b.ptr() for b in bufs)
    rec = torch.zeros(32, dtype=torch.uint8, device=gpu)
    for fn, lr in ((lib.cham_adam_tf, 1e-3), (lib.cham_adam_tf_dev, rec.data_ptr())):
        call = lambda p_, g_, m_, v_, n, n_reg: fn(p_, g_, m_, v_, n, n_reg, 1e-4, lr, 0.9, 0.999, 1e-8, _st())
        assert call(p, g, m, v, 6, 0) == -22 and call(p, g, m, v, 8, 2) == -22 and call(p, g, m, v, 8, 12) == -22
        assert call(None, g, m, v, 8, 4) == -22 and call(p, None, m, v, 8, 4) == -22 and call(p, g, None, v, 8, 4) == -22 and call(p, g, m, None, 8, 4) == -22
        assert call(p, g, m, v, 0, 0) == 0
    assert lib.cham_adam_tf_dev(p, g, m, v, 8, 4, 1e-4, None, 0.9, 0.999, 1e-8, _st()) == -22
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)


# ---- L2 sum, loss, accumulation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reg,BT", R.LOSS_CASES)
def test_sumsq_and_loss_finalize(gpu, n_reg, BT):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    print("\nn_reg %d BT %d" % (n_reg, BT))
    k = gpu_bounds()['loss.loss']
    inp = R.loss_inputs(n_reg, BT)
    lam = float(np.float32(R.LOSS_LAMBDA))
    sumsq = float((R.f64(inp['p'][:n_reg]) ** 2).sum())
    ref = R.loss_finalize(inp['nll'], inp['sum_mask'], sumsq, lam)
    assert abs(ref[2] - R.l2_loss(inp['p'], n_reg, lam)) <= 1e-15 * max(ref[2], 1e-300)
    p, nll = _dev(gpu, inp['p']), _dev(gpu, inp['nll'])
    rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
    check(lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, 0, inp['sum_mask'], 0.0, 2, _st()), "cham_step_scalars_set")
    outs = []
    for dev in (False, False, True):
        part, loss = R.Guarded(gpu, (1024,)), R.Guarded(gpu, (3,))
        check(lib.cham_sumsq_partial(p.data_ptr(), n_reg, part.ptr(), _st()), "cham_sumsq_partial")
        if dev:
            check(lib.cham_loss_finalize_dev(nll.data_ptr(), BT, rec.data_ptr(), part.ptr(), lam, loss.ptr(), _st()), "cham_loss_finalize_dev")
        else:
            check(lib.cham_loss_finalize(nll.data_ptr(), BT, inp['sum_mask'], part.ptr(), lam, loss.ptr(), _st()), "cham_loss_finalize")
        torch.cuda.synchronize()
        outs.append((part.numpy(), loss.numpy()))
    assert all(R.same_bits(outs[0][j], o[j]) for o in outs[1:] for j in (0, 1)), "two runs, or by value and _dev, differ"
    part, loss = outs[0]
    _note('sumsq', R.comp_err([part.astype(np.float64).sum()], [sumsq]), k)
    _note('loss', R.comp_err(loss, ref), k)
    assert lib.cham_loss_finalize(nll.data_ptr(), BT, 0.0, p.data_ptr(), lam, p.data_ptr(), _st()) == -22          # sum(mask) = 0
    assert lib.cham_loss_finalize(nll.data_ptr(), 0, 1.0, p.data_ptr(), lam, p.data_ptr(), _st()) == -22
    assert lib.cham_loss_finalize_dev(nll.data_ptr(), BT, None, p.data_ptr(), lam, p.data_ptr(), _st()) == -22
    assert lib.cham_sumsq_partial(p.data_ptr(), 6, p.data_ptr(), _st()) == -22 and lib.cham_sumsq_partial(None, 4, p.data_ptr(), _st()) == -22


def test_loss_accumulate(gpu):
    """acc = [xe_acc + reg, xe_acc (+)= xe, reg]: one fp32 addition each, so the expected values are exact."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    f = np.float32
    a = np.array([9.0, 2.7182817, 0.125], f)
    b = np.array([5.0, 3.1415927, 0.33333334], f)
    acc = R.Guarded(gpu, (3,))
    check(lib.cham_loss_accumulate(acc.ptr(), _dev(gpu, a).data_ptr(), 1, _st()), "cham_loss_accumulate")      # first: the NaN contents must not leak
    torch.cuda.synchronize()
    assert R.same_bits(acc.numpy(), np.array([a[1] + a[2], a[1], a[2]], f))
    check(lib.cham_loss_accumulate(acc.ptr(), _dev(gpu, b).data_ptr(), 0, _st()), "cham_loss_accumulate")
    torch.cuda.synchronize()
    xe = f(a[1] + b[1])
    assert R.same_bits(acc.numpy(), np.array([xe + b[2], xe, b[2]], f))
    assert lib.cham_loss_accumulate(None, acc.ptr(), 0, _st()) == -22 and lib.cham_loss_accumulate(acc.ptr(), None, 0, _st()) == -22


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1027, 8192 * 256 * 4 + 3])
def test_accumulate_is_one_exact_addition_per_element(gpu, n):
    """n % 4 in {0, 1, 2, 3} (float4 body + scalar tail) and a size beyond 8192 workgroups x 256 threads x 4 floats (second grid-stride trip)."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    rng = np.random.default_rng(n % 9973)
    x, a = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    xd = _dev(gpu, x)
    for first, want in ((1, x), (0, a + x)):
        for _ in range(2):
            acc = R.Guarded(gpu, (n,), init=None if first else _dev(gpu, a))          # first = 1: the old contents are NaN
            check(lib.cham_accumulate(acc.ptr(), xd.data_ptr(), n, first, _st()), "cham_accumulate")
            torch.cuda.synchronize()
            assert R.same_bits(acc.numpy(), want), "first = %d" % first
    assert lib.cham_accumulate(acc.ptr(), xd.data_ptr(), 0, 0, _st()) == -22 and lib.cham_accumulate(None, xd.data_ptr(), n, 0, _st()) == -22


# ---- column sums ----------------------------------------------------------------------------------------------------------------------
def _colsum_run(gpu, lib, fn, Xd, wd, prev, R_, F, ld, weights, acc, short=0):
    nb = lib.cham_colsum_workspace_bytes(R_, F)
    assert nb == 4 * F * -(-R_ // R.colsum_chunk_rows(R_))
    ws = R.Guarded(gpu, (nb // 4,))
    out = R.Guarded(gpu, (F,), init=_dev(gpu, prev) if acc else None)
    rc = fn(Xd.data_ptr(), ld, R_, F, wd.data_ptr() if weights else None, out.ptr(), acc, ws.ptr(), nb - short, _st())
    torch.cuda.synchronize()
    ws.numpy()
    return rc, out


@pytest.mark.parametrize("F", R.COLSUM_F)
def test_colsum_fp32_and_bf16(gpu, F):
    lib = _lib_()
    k = gpu_bounds()['colsum.out']
    for R_, F_, ld, weights, acc in R.colsum_cases():
        if F_ != F:
            continue
        print("\nR %d F %d ld %d weights %d accumulate %d" % (R_, F, ld, weights, acc))
        for b16 in (False, True):
            inp = R.colsum_inputs(R_, F, ld, b16)
            fn = lib.cham_colsum_b16 if b16 else lib.cham_colsum
            Xd, wd = _dev(gpu, inp['X'], b16), _dev(gpu, inp['w'])
            rc, out = _colsum_run(gpu, lib, fn, Xd, wd, inp['prev'], R_, F, ld, weights, acc)
            if b16 and not R.colsum_vec_ok(F, ld):
                assert rc == -22 and (out.untouched() if not acc else True), "cham_colsum_b16 took a shape its kernel cannot"
                continue
            assert rc == 0
            got = out.numpy()
            assert R.same_bits(got, _colsum_run(gpu, lib, fn, Xd, wd, inp['prev'], R_, F, ld, weights, acc)[1].numpy()), "two runs differ"
            _note('colsum_b16' if b16 else 'colsum', R.rel_err(got, colsum_reference(inp, F, weights, acc)), k)
            rc, out = _colsum_run(gpu, lib, fn, Xd, wd, inp['prev'], R_, F, ld, weights, 0, short=4)
            assert rc == -22 and out.untouched(), "an undersized workspace was accepted"
    x = torch.zeros(64, device=gpu)
    for fn in (lib.cham_colsum, lib.cham_colsum_b16):
        assert fn(x.data_ptr(), 4, 0, 4, None, x.data_ptr(), 0, x.data_ptr(), 1024, _st()) == -22
        assert fn(x.data_ptr(), 4, 4, 0, None, x.data_ptr(), 0, x.data_ptr(), 1024, _st()) == -22
        assert fn(None, 4, 4, 4, None, x.data_ptr(), 0, x.data_ptr(), 1024, _st()) == -22


# ---- casts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Rr,Cc", [(1, 1), (31, 33), (32, 32), (100, 378), (1024, 128)])
def test_cast_b16_rounds_to_nearest_even(gpu, Rr, Cc):
    """dst = bf16(W), dstT = bf16(W)^T, either or both, bit for bit against the integer rounding of tail_reference.round_bf16_bits: ties on odd
    and even mantissas, signed zeros, the largest fp32 that stays finite, denormals (bf16_edge_values) and random values."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    rng = np.random.default_rng(Rr + Cc)
    W = (rng.standard_normal(Rr * Cc) * 10.0 ** rng.integers(-3, 4, Rr * Cc)).astype(np.float32)
    edge = bf16_edge_values()
    for j in range(0, Rr * Cc, max(1, len(edge) + 17)):          # the edge values at many (row, column) positions of the 32 x 32 tiles
        W[j:j + len(edge)] = edge[:len(W[j:j + len(edge)])]
    ties = rng.integers(0, 2 ** 16, Rr * Cc // 3).astype(np.uint32) << 16 | 0x8000          # exactly half an ulp above a bf16 value
    ties = ties[(ties >> 23) & 0xFF != 0xFF]
    W[rng.choice(Rr * Cc, size=len(ties), replace=False)] = ties.view(np.float32)
    W = W.reshape(Rr, Cc)
    want = R.round_bf16_bits(W).reshape(Rr, Cc)
    Wd = _dev(gpu, W)
    for use_dst, use_T in ((True, False), (False, True), (True, True)):
        for _ in range(2):
            dst, dstT = R.Guarded(gpu, (Rr, Cc), torch.bfloat16), R.Guarded(gpu, (Cc, Rr), torch.bfloat16)
            check(lib.cham_cast_b16(Wd.data_ptr(), Rr, Cc, dst.ptr() if use_dst else None, dstT.ptr() if use_T else None, _st()), "cham_cast_b16")
            torch.cuda.synchronize()
            if use_dst:
                assert R.same_bits(dst.numpy(), want), "dst is not round-to-nearest-even"
            else:
                assert dst.untouched()
            if use_T:
                assert R.same_bits(dstT.numpy(), np.ascontiguousarray(want.T)), "dstT is not the transposed rounding"
            else:
                assert dstT.untouched()
    assert lib.cham_cast_b16(Wd.data_ptr(), Rr, Cc, None, None, _st()) == -22 and lib.cham_cast_b16(None, Rr, Cc, dst.ptr(), None, _st()) == -22
    assert lib.cham_cast_b16(Wd.data_ptr(), 0, Cc, dst.ptr(), None, _st()) == -22


@pytest.mark.parametrize("n", [0, 4, 4 * (8192 * 256) + 4])
def test_upcast_b16_is_exact(gpu, n):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    rng = np.random.default_rng(n % 1013)
    bits = rng.integers(0, 2 ** 16, max(n, 4)).astype(np.uint16)
    bits = np.where((bits >> 7) & 0xFF == 0xFF, bits & 0x807F, bits)[:max(n, 4)]          # no Inf / NaN patterns (NaN != NaN bitwise is fine, but keep it plain)
    src = torch.from_numpy(bits.view(np.int16)).to(gpu).view(torch.bfloat16)
    for _ in range(2):
        dst = R.Guarded(gpu, (n,))
        check(lib.cham_upcast_b16(src.data_ptr(), n, dst.ptr(), _st()), "cham_upcast_b16")
        torch.cuda.synchronize()
        assert R.same_bits(dst.numpy(), R.bf16_bits_to_f32(bits[:n]))
        assert dst.intact() and (n > 0 or dst.untouched())
    assert lib.cham_upcast_b16(src.data_ptr(), 6, dst.ptr(), _st()) == -22 and lib.cham_upcast_b16(None, 4, dst.ptr(), _st()) == -22


def test_zz_print_the_worst_errors(gpu):
    """(last in the file) the figures of the module docstring: worst error per array / its bound."""
    for name, (err, k) in sorted(WORST.items()):
        print("%-28s worst %.2e  bound %.2e" % (name, err, k))
