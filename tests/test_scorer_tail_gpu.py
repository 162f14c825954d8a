"""The tail of csrc/scorer.hip, entry point by entry point, against the float64 references of tests/tail_reference.py:
cham_score_softmax_fwd / _fwd_b16, cham_score_softmax_bwd / _bwd_b16 / _bwd_dev / _bwd_b16_dev, cham_rank_items, cham_mulpred_bwd / _b16 /
_p3 / _h2, cham_mul_rows_b16, and cham_step_scalars_set (csrc/optim.hip), whose record the _dev forms read.

Every output starts as NaN inside a guarded allocation (tail_reference.Guarded), every launch is made twice and must repeat bit for bit,
and the bound of every compared array is max |hip - ref| <= k max |ref| (per click for probs, ds, dS3) with k = 8 x the error of the
same formula in fp32 on the CPU at the same inputs (tests/test_tail_reference_cpu.py, which also shows that each of 17 slips breaks it tenfold).
Exact by construction and compared with ==: masked clicks (nll, ds, dS3 zero, label_rank -1), ranking order and ids, by-value against
_dev, cham_mul_rows_b16 against round_bf16(fp32 product).

bf16 outputs: dM of cham_mulpred_bwd_b16 against round_bf16(reference), one bf16 ulp allowed where the reference is within the fp32 bound
of a rounding boundary, on at most 1 % of the elements.  dS3 of the bf16 softmax backward the same way, but against round_bf16 of
(the kernel's own ds) w4 leaky'(S3): ds is held to its bound separately, and what remains are two fp32 products.  A bound relative to the
click's largest |dS3| would put most elements of a click within reach of a boundary - at tau = 0.1 they span 20 decades.

Inputs: a click whose positive leads every negative by a wide margin has p_0 -> 1 and a ds row that cancels to ~1e-40; fp32 (CPU and GPU
alike) returns 0 there and an error relative to the row's max measures nothing.  tail_reference.softmax_inputs therefore lets the
positive lead by at most 0.03 logits, except in one MASKED click per ragged case (lead >= 100 in z: the max subtraction is what keeps
expf finite), whose logits and probs are owed and whose nll / ds / dS3 are exact zeros.

Findings.  cham_rank_items admitted N <= 8191 and launched with 16 (1 + N) bytes of dynamic LDS without raising the 64 KB limit: for
N > 4095 the launch could not succeed.  Decided: the guard stays (128 KB fits the CU's 160 KB; the evaluation of a large candidate set is
what the limit was written for) and the entry point raises the limit as every other > 64 KB kernel here does; N = 8191 runs below,
N = 8192 gives -22.  NaN probabilities are not ranked: every comparison with a NaN is false, several candidates would share rank 0 and
some output slots would stay unwritten (tf.nn.top_k is total); finite logits cannot produce one, and no test feeds one.

Worst error seen on one MI355X / fp32-CPU error of the same array (the bound is 8 x the latter):
    logits 3.0e-7 / 3.9e-7   probs 2.8e-6 / 3.9e-6   nll 5.9e-7 / 5.2e-7   novterm 1.3e-6 / 9.7e-7   ds 2.8e-6 / 2.6e-6   dS3 1.7e-6 / 2.1e-6
    mulpred dZ2 9.7e-8 / 9.7e-8 (p3 planes 9.7e-8, h2 planes 1.6e-7)   dpred_pre 5.7e-7 / 5.6e-7   col_part 5.7e-7 / 4.8e-7
    bf16 dS3: no element off round_bf16; bf16 dM: at most 0.0005 % of the elements one ulp off.  No kernel needs more than 1.4 x fp32-CPU.
Wall time of this file on one MI355X: 4.2 s (32 tests).
"""
import numpy as np
import pytest
import torch

from tests import tail_reference as R
from tests.test_tail_reference_cpu import ds3_bf16_target, gpu_bounds, softmax_case

pytestmark = pytest.mark.gpu

WORST = {}


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t.bfloat16() if bf16 else t          # (exact: the inputs are bf16-representable)


def _note(name, err, k):
    w = WORST.setdefault(name, [0.0, k])
    w[0] = max(w[0], err)
    print("    %-22s %.2e  (bound %.2e)" % (name, err, k))
    assert err <= k, (name, err, k)


def _scalars(gpu, lib, sum_mask):
    """A ChamStepScalars record holding sum_mask (fields = 2: the batch scalars), everything else zero."""
    from chameleon_recsys_amd._lib import check
    rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
    check(lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, 0, float(sum_mask), 0.0, 2, _st()), "cham_step_scalars_set")
    return rec


def _forward(gpu, lib, inp, d):
    from chameleon_recsys_amd._lib import check
    BT, N, NC = inp['BT'], inp['N'], inp['N'] + 1
    o = dict(logits=R.Guarded(gpu, (BT, NC)), probs=R.Guarded(gpu, (BT, NC)), nll=R.Guarded(gpu, (BT,)), nov_aux=R.Guarded(gpu, (BT, 3)))
    fn = lib.cham_score_softmax_fwd_b16 if inp['bf16'] else lib.cham_score_softmax_fwd
    check(fn(d['S3'].data_ptr(), R.K3, d['w4'].data_ptr(), d['b4'].data_ptr(), BT, N, inp['tau'], d['mask'].data_ptr(), o['logits'].ptr(),
             o['probs'].ptr(), o['nll'].ptr(), inp['nov_factor'], d['neg_ids'].data_ptr(), d['pop_norm'].data_ptr(), o['nov_aux'].ptr(), _st()),
          "cham_score_softmax_fwd")
    torch.cuda.synchronize()
    if inp['nov_factor'] == 0:
        assert o['nov_aux'].untouched()
    return o


def _backward(gpu, lib, inp, d, fwd, scalars=None):
    from chameleon_recsys_amd._lib import check
    BT, N, NC = inp['BT'], inp['N'], inp['N'] + 1
    o = dict(ds=R.Guarded(gpu, (BT, NC)), dS3=R.Guarded(gpu, (BT, NC, R.K3), torch.bfloat16 if inp['bf16'] else torch.float32))
    head = (d['S3'].data_ptr(), R.K3, d['w4'].data_ptr(), fwd['probs'].ptr(), d['mask'].data_ptr(), BT, N, inp['tau'])
    tail = (o['ds'].ptr(), o['dS3'].ptr(), inp['nov_factor'], d['neg_ids'].data_ptr(), d['pop_norm'].data_ptr(), fwd['logits'].ptr(),
            fwd['nov_aux'].ptr(), _st())
    if scalars is None:
        fn = lib.cham_score_softmax_bwd_b16 if inp['bf16'] else lib.cham_score_softmax_bwd
        rc = fn(*head, inp['sum_mask'], *tail)
    else:
        fn = lib.cham_score_softmax_bwd_b16_dev if inp['bf16'] else lib.cham_score_softmax_bwd_dev
        rc = fn(*head, scalars.data_ptr(), *tail)
    torch.cuda.synchronize()
    if inp['sum_mask'] == 0 and scalars is None:
        assert rc == -22 and o['ds'].untouched() and o['dS3'].untouched()
        return None
    check(rc, "cham_score_softmax_bwd")
    return o


def _rank(gpu, lib, inp, d, probs_t):
    from chameleon_recsys_amd._lib import check
    BT, N, NC = inp['BT'], inp['N'], inp['N'] + 1
    o = dict(pred_ids=R.Guarded(gpu, (BT, NC), torch.int64), pred_probs=R.Guarded(gpu, (BT, NC)), label_rank=R.Guarded(gpu, (BT,), torch.int32))
    check(lib.cham_rank_items(probs_t.data_ptr(), d['label_next'].data_ptr(), d['neg_ids'].data_ptr(), d['mask'].data_ptr(), BT, N,
                              o['pred_ids'].ptr(), o['pred_probs'].ptr(), o['label_rank'].ptr(), _st()), "cham_rank_items")
    torch.cuda.synchronize()
    return {k: v.numpy() for k, v in o.items()}


def _check_rank(got, probs, inp):
    want = R.rank_items(probs, inp['label_next'], inp['neg_ids'], inp['mask'])
    for k in want:
        assert R.same_bits(got[k], want[k]), "cham_rank_items: %s differs from the stable descending order" % k
    assert (got['label_rank'][inp['mask'] == 0] == -1).all()


@pytest.mark.parametrize("i", range(len(R.SOFTMAX_CASES)))
def test_softmax_forward_backward_and_ranking(gpu, i):
    lib = _lib_()
    inp, ref = softmax_case(i)
    k = gpu_bounds()
    print("\n%s" % (R.SOFTMAX_CASES[i],))
    d = {n: _dev(gpu, inp[n]) for n in ('w4', 'b4', 'mask', 'neg_ids', 'pop_norm', 'label_next')}
    d['S3'] = _dev(gpu, inp['S3'], inp['bf16'])
    masked = inp['mask'] == 0
    assert lib.cham_set_log_bases(1.3, inp['pop_log_base']) == 0
    try:
        f1, f2 = _forward(gpu, lib, inp, d), _forward(gpu, lib, inp, d)
        fwd = {n: v.numpy() for n, v in f1.items()}
        for n, v in f2.items():
            assert R.same_bits(fwd[n], v.numpy()), "forward: %s differs between two runs" % n
        _note('softmax.logits', R.rel_err(fwd['logits'], ref['logits']), k['softmax.logits'])
        _note('softmax.probs', R.row_err(fwd['probs'], ref['probs']), k['softmax.probs'])
        _note('softmax.nll', R.rel_err(fwd['nll'], ref['nll']), k['softmax.nll'])
        assert not fwd['nll'][masked].any(), "nll of a masked click is not exactly zero"
        if inp['nov_factor'] > 0:
            _note('softmax.novterm', R.rel_err(fwd['nov_aux'][:, 2], ref['novterm']), k['softmax.novterm'])
        S3 = inp['S3']
        for bt in range(0, inp['BT'], 3):          # tied candidates get bit-identical probabilities: the stable order decides their ranks
            same = [c for c in range(1, inp['N'] + 1) if S3[bt, c].tobytes() == S3[bt, 1].tobytes()]
            assert len({fwd['probs'][bt, c].tobytes() for c in same}) == 1
        # ranking: of the kernel's own probabilities (as the model runs it) and of the reference's, rounded to fp32
        got = _rank(gpu, lib, inp, d, f1['probs'].t)
        assert all(R.same_bits(got[n], v) for n, v in _rank(gpu, lib, inp, d, f1['probs'].t).items())
        _check_rank(got, fwd['probs'], inp)
        p32 = ref['probs'].astype(np.float32)
        _check_rank(_rank(gpu, lib, inp, d, _dev(gpu, p32)), p32, inp)
        # backward, from the forward's own outputs
        b1 = _backward(gpu, lib, inp, d, f1)
        if inp['sum_mask'] == 0:
            return
        bwd = {n: v.numpy() for n, v in b1.items()}
        for how, other in (("two runs", _backward(gpu, lib, inp, d, f1)), ("by value and _dev", _backward(gpu, lib, inp, d, f1, _scalars(gpu, lib, inp['sum_mask'])))):
            for n, v in other.items():
                assert R.same_bits(bwd[n], v.numpy()), "backward: %s differs between %s" % (n, how)
        _note('softmax.ds', R.row_err(bwd['ds'], ref['ds']), k['softmax.ds'])
        dS3 = R.bf16_bits_to_f32(bwd['dS3']) if inp['bf16'] else bwd['dS3']
        assert not bwd['ds'][masked].any() and not dS3[masked].any(), "gradient of a masked click is not exactly zero"
        if inp['bf16']:
            target, tol = ds3_bf16_target(inp, bwd['ds'])
            ok, share = R.bf16_matches(bwd['dS3'], target, tol)
            print("    dS3 (bf16): %.4f %% of the elements one ulp off round_bf16" % (100 * share))
            assert ok and share <= 0.01, share
            _note('softmax.dS3(bf16)', R.row_err(R.bf16_bits_to_f32(bwd['dS3']), ref['dS3']), k['softmax.dS3'] + 2.0 ** -8)
        else:
            _note('softmax.dS3', R.row_err(bwd['dS3'], ref['dS3']), k['softmax.dS3'])
    finally:
        assert lib.cham_set_log_bases(1.3, 2.0) == 0


def test_rank_items_at_the_largest_admitted_n(gpu):
    """N = 8191: 128 KB of dynamic LDS, above the 64 KB a launch gets without hipFuncAttributeMaxDynamicSharedMemorySize.  BT = 5 leaves
    three waves of the second workgroup without a click.  A third of the candidates tie."""
    lib = _lib_()
    N, BT = 8191, 5
    rng = np.random.default_rng(8191)
    p = rng.random((BT, N + 1)).astype(np.float32)
    p[:, rng.choice(N + 1, size=N // 3, replace=False)] = np.float32(0.25)
    p[1, 0] = np.float32(0.25)
    p /= p.sum(1, keepdims=True, dtype=np.float32)
    inp = dict(BT=BT, N=N, mask=np.array([1, 1, 0, 1, 1], np.uint8), label_next=rng.integers(1, 10 ** 9, BT).astype(np.int64),
               neg_ids=rng.integers(0, 2 ** 40, (BT, N)).astype(np.int64))
    d = {n: _dev(gpu, inp[n]) for n in ('mask', 'label_next', 'neg_ids')}
    got = _rank(gpu, lib, inp, d, _dev(gpu, p))
    _check_rank(got, p, inp)
    assert all(R.same_bits(got[n], v) for n, v in _rank(gpu, lib, inp, d, _dev(gpu, p)).items())
    x = _dev(gpu, p)
    o = R.Guarded(gpu, (BT, N + 2), torch.int64)
    args = lambda n: (x.data_ptr(), d['label_next'].data_ptr(), d['neg_ids'].data_ptr(), d['mask'].data_ptr(), BT, n, o.ptr(), x.data_ptr(), x.data_ptr(), _st())
    assert lib.cham_rank_items(*args(N + 1)) == -22 and lib.cham_rank_items(*args(0)) == -22
    torch.cuda.synchronize()
    assert o.untouched()


def test_step_scalars_set_writes_only_the_fields_it_is_asked_to(gpu):
    """ChamStepScalars (csrc/common.h): {uint32 step, step_next; int64 max_ts, max_ts_next; float sum_mask, lr_t} = 32 bytes.  fields: bit 0 the
    sampler keys, bit 1 max_ts and sum_mask, bit 2 lr_t."""
    lib = _lib_()
    nb = lib.cham_step_scalars_bytes()
    assert nb == 32
    rec_t = np.dtype([('step', '<u4'), ('step_next', '<u4'), ('max_ts', '<i8'), ('max_ts_next', '<i8'), ('sum_mask', '<f4'), ('lr_t', '<f4')])
    buf = R.Guarded(gpu, (nb,), torch.uint8)
    start = np.frombuffer(np.arange(1, nb + 1, dtype=np.uint8).tobytes(), rec_t)[0]
    new = dict(step=0xDEADBEEF, step_next=0x12345678, max_ts=-(2 ** 52 + 3), sum_mask=np.float32(1234.5), lr_t=np.float32(3.25e-4))
    owns = {1: ('step', 'step_next'), 2: ('max_ts', 'sum_mask'), 4: ('lr_t',), 7: ('step', 'step_next', 'max_ts', 'sum_mask', 'lr_t'), 5: ('step', 'step_next', 'lr_t')}
    for fields, names in owns.items():
        buf.t.copy_(torch.arange(1, nb + 1, dtype=torch.uint8))
        assert lib.cham_step_scalars_set(buf.ptr(), new['step'], new['step_next'], new['max_ts'], float(new['sum_mask']), float(new['lr_t']), fields, _st()) == 0
        torch.cuda.synchronize()
        got = np.frombuffer(buf.numpy().tobytes(), rec_t)[0]
        for f in rec_t.names:
            want = new[f] if f in names else start[f]
            assert got[f] == want, (fields, f, got[f], want)
    assert lib.cham_step_scalars_set(buf.ptr(), 1, 2, 3, 1.0, 1.0, 0, _st()) == -22
    assert lib.cham_step_scalars_set(buf.ptr(), 1, 2, 3, 1.0, 1.0, 8, _st()) == -22
    assert lib.cham_step_scalars_set(None, 1, 2, 3, 1.0, 1.0, 7, _st()) == -22
    assert lib.cham_step_scalars_set(buf.ptr() + 4, 1, 2, 3, 1.0, 1.0, 7, _st()) == -22          # the record holds int64 fields


def _planes(gpu, n_planes, n, dtype):
    return R.Guarded(gpu, (n_planes, n), dtype)


@pytest.mark.parametrize("C,N,BT", R.MULPRED_CASES)
def test_mulpred_backward_all_four_forms(gpu, C, N, BT):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    k = gpu_bounds()
    print("\nC %d N %d BT %d" % (C, N, BT))
    NC, Rc = N + 1, BT * (N + 1)
    inp = R.mulpred_inputs(C, N, BT)
    ref = R.mulpred_grad(**inp)
    dM, Z, pred = (_dev(gpu, inp[n]) for n in ('dM', 'Z2c', 'pred'))

    def fp32_form():
        o = dict(dZ2=R.Guarded(gpu, (BT, NC, C), init=dM), dpred_pre=R.Guarded(gpu, (BT, C)))
        check(lib.cham_mulpred_bwd(o['dZ2'].ptr(), Z.data_ptr(), pred.data_ptr(), C, BT, N, o['dpred_pre'].ptr(), _st()), "cham_mulpred_bwd")
        torch.cuda.synchronize()
        return {n: v.numpy() for n, v in o.items()}

    def plane_form(kind, with_col):
        dt = torch.bfloat16 if kind == 'p3' else torch.float16
        o = dict(planes=_planes(gpu, 3 if kind == 'p3' else 2, Rc * C, dt), dpred_pre=R.Guarded(gpu, (BT, C)), col_part=R.Guarded(gpu, (BT, C)))
        col = o['col_part'].ptr() if with_col else None
        inv = 1.0
        if kind == 'p3':
            check(lib.cham_mulpred_bwd_p3(dM.data_ptr(), Z.data_ptr(), pred.data_ptr(), C, BT, N, o['dpred_pre'].ptr(), o['planes'].ptr(), Rc * C, col, _st()),
                  "cham_mulpred_bwd_p3")
        else:
            rec = torch.zeros(8, device=gpu)
            check(lib.cham_h2_scale_absmax(dM.data_ptr(), dM.numel(), dM.data_ptr(), dM.numel(), rec.data_ptr(), _st()), "cham_h2_scale_absmax")
            check(lib.cham_mulpred_bwd_h2(dM.data_ptr(), Z.data_ptr(), pred.data_ptr(), C, BT, N, o['dpred_pre'].ptr(), o['planes'].ptr(), Rc * C, col,
                                          rec.data_ptr(), _st()), "cham_mulpred_bwd_h2")
            inv = float(rec[1])
        torch.cuda.synchronize()
        if not with_col:
            assert o['col_part'].untouched()
        total = o['planes'].t.double().sum(0).cpu().numpy().reshape(BT, NC, C) * inv
        return dict(planes=o['planes'].numpy(), total=total, dpred_pre=o['dpred_pre'].numpy(), col_part=o['col_part'].t.cpu().numpy())

    a = fp32_form()
    assert all(R.same_bits(a[n], v) for n, v in fp32_form().items()), "cham_mulpred_bwd: two runs differ"
    _note('mulpred.dZ2', R.rel_err(a['dZ2'], ref['dZ2']), k['mulpred.dZ2'])
    _note('mulpred.dpred_pre', R.rel_err(a['dpred_pre'], ref['dpred_pre']), k['mulpred.dpred_pre'])
    # three bf16 planes hold 24 significand bits (2^-24 of the value), two fp16 planes under one scale 2^-21 of the matrix's max
    # (the resolution tests/test_gemm_h2_gpu.py grants the format)
    for kind, res in (('p3', 2.0 ** -24), ('h2', 2.0 ** -21)):
        b = plane_form(kind, True)
        again, nocol = plane_form(kind, True), plane_form(kind, False)
        for n in ('planes', 'dpred_pre', 'col_part'):
            assert R.same_bits(b[n], again[n]), "cham_mulpred_bwd_%s: %s differs between two runs" % (kind, n)
        assert R.same_bits(b['planes'], nocol['planes']) and R.same_bits(b['dpred_pre'], nocol['dpred_pre'])
        _note('mulpred.dZ2(%s)' % kind, R.rel_err(b['total'], ref['dZ2']), k['mulpred.dZ2'] + res)
        _note('mulpred.dpred_pre(%s)' % kind, R.rel_err(b['dpred_pre'], ref['dpred_pre']), k['mulpred.dpred_pre'])
        _note('mulpred.col_part(%s)' % kind, R.rel_err(b['col_part'], ref['col_part']), k['mulpred.col_part'])
        assert R.same_bits(b['dpred_pre'], a['dpred_pre']), "the plane form's dpred_pre is not the fp32 form's"

    # bf16 in place
    inb = R.mulpred_inputs(C, N, BT, True)
    refb = R.mulpred_grad(**inb)
    Zb, dMb = _dev(gpu, inb['Z2c'], True), _dev(gpu, inb['dM'], True)

    def b16_form():
        o = dict(dZ2=R.Guarded(gpu, (BT, NC, C), torch.bfloat16, init=dMb), dpred_pre=R.Guarded(gpu, (BT, C)))
        check(lib.cham_mulpred_bwd_b16(o['dZ2'].ptr(), Zb.data_ptr(), pred.data_ptr(), C, BT, N, o['dpred_pre'].ptr(), _st()), "cham_mulpred_bwd_b16")
        torch.cuda.synchronize()
        return {n: v.numpy() for n, v in o.items()}
    c = b16_form()
    assert all(R.same_bits(c[n], v) for n, v in b16_form().items()), "cham_mulpred_bwd_b16: two runs differ"
    ok, share = R.bf16_matches(c['dZ2'], refb['dZ2'], k['mulpred.dZ2'] * np.abs(refb['dZ2']).max())
    print("    dM (bf16): %.4f %% of the elements one ulp off round_bf16" % (100 * share))
    assert ok and share <= 0.01, share
    _note('mulpred.dpred_pre(b16)', R.rel_err(c['dpred_pre'], refb['dpred_pre']), k['mulpred.dpred_pre'])


@pytest.mark.parametrize("NC", [1, 2, 3, 4, 5, 51])
def test_mul_rows_b16_is_the_rounded_fp32_product(gpu, NC):
    """Mc = bf16(float(z) * p): the fp32 product (one IEEE rounding) rounded to bf16, bit for bit.  The kernel loads four candidates at a time
    and clamps the loads at NC - 1."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    BT, C = 7, 128
    rng = np.random.default_rng(NC)
    Z = R.round_bf16(np.tanh(1.5 * rng.standard_normal((BT, NC, C))).astype(np.float32)).reshape(BT, NC, C)
    pred = np.tanh(1.5 * rng.standard_normal((BT, C))).astype(np.float32)
    want = R.round_bf16_bits(Z * pred[:, None, :])                   # numpy multiplies fp32 by fp32 in fp32
    Zd, pd = _dev(gpu, Z, True), _dev(gpu, pred)
    outs = []
    for _ in range(2):
        o = R.Guarded(gpu, (BT, NC, C), torch.bfloat16)
        check(lib.cham_mul_rows_b16(Zd.data_ptr(), pd.data_ptr(), C, BT, NC, o.ptr(), _st()), "cham_mul_rows_b16")
        torch.cuda.synchronize()
        outs.append(o.numpy())
    assert R.same_bits(outs[0], outs[1]) and R.same_bits(outs[0], want)
    assert R.rel_err(R.bf16_bits_to_f32(outs[0]), R.mul_rows(Z, pred)) <= 2.0 ** -8
    assert lib.cham_mul_rows_b16(Zd.data_ptr(), pd.data_ptr(), C, BT, 0, o.ptr(), _st()) == -22
    assert lib.cham_mul_rows_b16(Zd.data_ptr(), pd.data_ptr(), C + 2, BT, NC, o.ptr(), _st()) == -22


def test_scorer_tail_argument_errors(gpu):
    lib = _lib_()
    x = torch.zeros(4096, device=gpu)
    p, st = x.data_ptr(), _st()
    fwd = lambda fn, K3, BT, N, S3=p: fn(S3, K3, p, p, BT, N, 0.1, p, p, p, p, 0.0, None, None, None, st)
    for fn in (lib.cham_score_softmax_fwd, lib.cham_score_softmax_fwd_b16):
        assert fwd(fn, 64, 2, 3) == -22 and fwd(fn, 32, 0, 3) == -22 and fwd(fn, 32, 2, 0) == -22 and fwd(fn, 32, 2, 3, None) == -22
        assert fn(p, 32, p, p, 2, 3, 0.1, p, p, p, p, 0.3, None, p, p, st) == -22           # novelty without neg_ids
    for fn in (lib.cham_score_softmax_bwd, lib.cham_score_softmax_bwd_b16):
        assert fn(p, 32, p, p, p, 2, 3, 0.1, 0.0, p, p, 0.0, None, None, None, None, st) == -22          # sum_mask = 0
        assert fn(p, 16, p, p, p, 2, 3, 0.1, 2.0, p, p, 0.0, None, None, None, None, st) == -22
        assert fn(p, 32, p, p, p, 2, 3, 0.1, 2.0, p, p, 0.3, p, p, None, p, st) == -22                   # novelty without the logits
    for fn in (lib.cham_score_softmax_bwd_dev, lib.cham_score_softmax_bwd_b16_dev):
        assert fn(p, 32, p, p, p, 2, 3, 0.1, None, p, p, 0.0, None, None, None, None, st) == -22         # no record
    assert lib.cham_mulpred_bwd(p, p, p, 6, 2, 3, p, st) == -22 and lib.cham_mulpred_bwd_b16(p, p, p, 6, 2, 3, p, st) == -22
    assert lib.cham_mulpred_bwd_p3(p, p, p, 8, 2, 3, p, p, 8 * 8 + 2, None, st) == -22                  # plane stride % 4
    assert lib.cham_mulpred_bwd_h2(p, p, p, 8, 2, 3, p, p, 64, None, None, st) == -22                   # no scale record
    torch.cuda.synchronize()


def test_zz_print_the_worst_errors(gpu):
    """(last in the file) the figures of the module docstring: worst error per array / its bound."""
    for name, (err, k) in sorted(WORST.items()):
        print("%-28s worst %.2e  bound %.2e" % (name, err, k))
