"""Cosine ranking head (--recommendations_ranking cosine) on the GPU: the kernels of csrc/cosine.hip against the float64 restatement of
tests/cosine_reference.py, the softmax kernels at K3 = 4, and the step / training / evaluation against tests/cosine_oracle.CosineOracle.

Kernel bounds are worst-case rounding, not measurements (EPS = 2^-24):
  forward   |cos - ref| <= (C + 32) EPS for fp32 rows - after normalisation the terms' absolute sum is <= 1 - plus 2^-8 for bf16-stored rows;
  backward  |got - ref| <= (C + 32) EPS x (the closed form evaluated over absolute values), + 2^-21 x (the scale record's bound) for the
            two-plane output, + 2^-8 |ref| for bf16 output.
Step bounds are the project's own (tests/test_step_gpu.py): negatives bit-exact, logits / probs / loss within 1e-3, gradients within
3e-4 max|ref| + 2e-5 on batches without a leaky-ReLU kink flip - counted over the sites this mode has, Z1 and FC1."""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from tests import cosine_oracle as CO
from tests import cosine_reference as CR
from tests import helpers as H

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
EPS = 2.0 ** -24
GUARD = 64


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


class Out:
    """An output array between two NaN guards: an element the kernel owes and does not write stays NaN, a write outside shows in the guards."""

    def __init__(self, gpu, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float('nan'), dtype=dtype, device=gpu)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)

    def ptr(self):
        return self.t.data_ptr()

    def get(self):
        torch.cuda.synchronize()
        assert bool(torch.isnan(self.buf[:GUARD].float()).all()) and bool(torch.isnan(self.buf[-GUARD:].float()).all()), "a kernel wrote outside its output"
        return self.t.clone()


def _rows(gpu, z, b16, pad):
    """z [BT, NC, C] -> device rows [R, C + pad] (NaN in the padding columns) in the arm's storage."""
    BT, NC, C = z.shape
    rows = torch.full((BT * NC, C + pad), float('nan'), dtype=torch.float32)
    rows[:, :C] = z.reshape(BT * NC, C)
    rows = rows.to(gpu)
    return rows.bfloat16() if b16 else rows


def _fwd(gpu, z, p, b16=False, pad=0):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    BT, NC, C = z.shape
    rows, pd = _rows(gpu, z, b16, pad), p.to(gpu)
    o = dict(cosq=Out(gpu, (BT * NC, 4)), rz=Out(gpu, (BT * NC,)), rp=Out(gpu, (BT,)))
    fn = lib.cham_cosine_fwd_b16 if b16 else lib.cham_cosine_fwd
    check(fn(rows.data_ptr(), C + pad, pd.data_ptr(), C, BT, NC - 1, o['cosq'].ptr(), o['rz'].ptr(), o['rp'].ptr(), _st()), "cham_cosine_fwd")
    return {k: v.get() for k, v in o.items()}


FWD_SHAPES = [(BT, N) for BT in (1, 5) for N in (1, 4, 63, 64)]


@pytest.mark.parametrize("C,b16", [(128, False), (132, False), (1024, False), (1028, False), (128, True), (1024, True)])
def test_forward_kernels_against_float64(gpu, C, b16):
    largest = 0.0
    for BT, N in FWD_SHAPES:
        NC = N + 1
        z, p, _, _ = CR.make_case(BT, NC, C, seed=2)
        ref = CR.closed_form(z, p, torch.zeros(BT, NC))
        tol = (C + 32) * EPS + (2.0 ** -8 if b16 else 0.0)
        for pad in (0, 8):
            got = _fwd(gpu, z, p, b16, pad)
            cosq = got['cosq'].cpu().double()
            assert bool(torch.isfinite(cosq).all())
            err = float((cosq[:, 0].view(BT, NC) - ref['cos']).abs().max())
            assert err <= tol, (BT, N, C, pad, err, tol)
            assert float(cosq[:, 1:].abs().max()) == 0.0 and not bool((torch.signbit(cosq) & (cosq == 0)).any())      # (no -0 either)
            rz, rp = got['rz'].cpu().double().view(BT, NC), got['rp'].cpu().double()
            assert float((rz / ref['rz'] - 1.0).abs().max()) <= tol and float((rp / ref['rp'] - 1.0).abs().max()) <= (C + 32) * EPS
            # the clamp regime is marked by exactly 1e6, and by nothing else
            assert float(rz[0, 0]) == 1e6 and float(rz[0, NC - 1]) == 1e6 and int((rz == 1e6).sum()) == (2 if NC > 1 else 1)
            assert int((rp == 1e6).sum()) == (1 if BT > 1 else 0)
            again = _fwd(gpu, z, p, b16, pad)
            assert all(torch.equal(got[k], again[k]) for k in got)
        largest = max(largest, float(ref['cos'].abs().max()))
    assert largest > 0.05          # ... and the comparison is not one of zeros


def _bwd(gpu, mode, z, p, ds, mask, fwd, with_b2=True):
    """mode 'f32' / 'h2' / 'b16' -> dict(dz [BT, NC, C] float64 as stored, dp, b2, bound)."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    BT, NC, C = z.shape
    R = BT * NC
    rows, pd, dsd, md = _rows(gpu, z, mode == 'b16', 0), p.to(gpu), ds.reshape(-1).to(gpu), mask.to(gpu)
    dp, b2 = Out(gpu, (BT, C)), Out(gpu, (BT, C))
    head = (rows.data_ptr(), pd.data_ptr(), dsd.data_ptr(), fwd['rz'].data_ptr(), fwd['rp'].data_ptr(), fwd['cosq'].data_ptr(), md.data_ptr(), C, BT, NC - 1)
    tail = (dp.ptr(), b2.ptr() if with_b2 else None, _st())
    bound = 0.0
    if mode == 'h2':
        t = Out(gpu, ((R + 3) & ~3,))
        rec = torch.zeros(8, dtype=torch.float32, device=gpu)
        check(lib.cham_cosine_bound(dsd.data_ptr(), fwd['rz'].data_ptr(), R, t.ptr(), _st()), "cham_cosine_bound")
        tv = t.get()
        want = (ds.reshape(-1).double().abs() * fwd['rz'].cpu().double())
        assert float((tv[:R].cpu().double() - want).abs().max()) <= EPS * float(want.max()) and float(tv[R:].abs().sum()) == 0.0
        check(lib.cham_h2_scale_absmax(t.ptr(), (R + 3) & ~3, None, 0, rec.data_ptr(), _st()), "cham_h2_scale_absmax")
        planes = Out(gpu, (2, R, C), torch.float16)
        check(lib.cham_cosine_bwd_h2(*head, planes.ptr(), R * C, rec.data_ptr(), *tail), "cham_cosine_bwd_h2")
        pl, rc = planes.get().cpu(), rec.cpu()
        assert bool(torch.isfinite(pl.float()).all()), "a plane holds a non-finite fp16 value"
        bound = float(rc[2])
        assert bound == float(tv.max()) and 2.0 ** 14 <= bound * float(rc[0]) < 2.0 ** 15
        dz = (pl[0].double() + pl[1].double()) * float(rc[1])
    elif mode == 'b16':
        o = Out(gpu, (R, C), torch.bfloat16)
        check(lib.cham_cosine_bwd_b16(*head, o.ptr(), *tail), "cham_cosine_bwd_b16")
        dz = o.get().cpu().double()
    else:
        o = Out(gpu, (R, C))
        check(lib.cham_cosine_bwd(*head, o.ptr(), *tail), "cham_cosine_bwd")
        dz = o.get().cpu().double()
    return dict(dz=dz.view(BT, NC, C), dp=dp.get().cpu().double(), b2=b2.get().cpu().double() if with_b2 else None, bound=bound)


@pytest.mark.parametrize("C,mode", [(128, 'f32'), (132, 'f32'), (1024, 'f32'), (1028, 'f32'), (128, 'h2'), (132, 'h2'), (1024, 'h2'), (1028, 'h2'),
                                    (128, 'b16'), (1024, 'b16')])
def test_backward_kernels_against_float64(gpu, C, mode):
    for BT, N in FWD_SHAPES:
        NC = N + 1
        z, p, ds, mask = CR.make_case(BT, NC, C, seed=3)
        if mode == 'b16':
            z = z.bfloat16().float()          # the rows as that arm stores them: the output's rounding is what its bound is about
        ref = CR.closed_form(z, p, ds)
        fwd = _fwd(gpu, z, p, mode == 'b16')
        got = _bwd(gpu, mode, z, p, ds, mask, fwd)
        k = (C + 32) * EPS
        tol_dz = k * ref['abs_dz'] + (2.0 ** -21 * got['bound'] if mode == 'h2' else 0.0) + (2.0 ** -8 * ref['dz'].abs() if mode == 'b16' else 0.0)
        over = (got['dz'] - ref['dz']).abs() - tol_dz
        assert float(over.max()) <= 0.0, (BT, N, C, mode, float(over.max()))
        over = (got['dp'] - ref['dp']).abs() - k * ref['abs_dp']
        assert float(over.max()) <= 0.0, (BT, N, C, mode, float(over.max()))
        assert float(ref['dz'].abs().max()) > 1e-3 and (BT == 1 or float(ref['dp'].abs().max()) > 1e-3)
        # b2part = the column sums of the rows as stored (fp32 sums of NC terms; the two-plane rows are stored to 2^-21 of the bound)
        sums, asum = got['dz'].sum(1), got['dz'].abs().sum(1)
        tol_b2 = NC * EPS * asum + (NC * 2.0 ** -21 * got['bound'] if mode == 'h2' else 0.0)
        assert float(((got['b2'] - sums).abs() - tol_b2).max()) <= 0.0
        # rows of a masked click are exactly zero, everywhere
        for bt in np.flatnonzero(mask.numpy() == 0):
            assert float(got['dz'][bt].abs().max()) == 0.0 and float(got['dp'][bt].abs().max()) == 0.0 and float(got['b2'][bt].abs().max()) == 0.0
        # the tiny row (rz = 1e6) is there, finite, and carries ds 1e6 p^
        assert float(got['dz'][0, NC - 1].abs().max()) > 0.0
    if mode == 'f32':      # the column sums are optional in this form; the other outputs do not depend on them
        z, p, ds, mask = CR.make_case(5, 5, C, seed=3)
        fwd = _fwd(gpu, z, p)
        a, b = _bwd(gpu, mode, z, p, ds, mask, fwd), _bwd(gpu, mode, z, p, ds, mask, fwd, with_b2=False)
        assert torch.equal(a['dz'], b['dz']) and torch.equal(a['dp'], b['dp']) and b['b2'] is None


def _softmax(gpu, S3, K3, w4, b4, mask, tau, BT, N, sum_mask):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    NC = N + 1
    o = dict(logits=Out(gpu, (BT, NC)), probs=Out(gpu, (BT, NC)), nll=Out(gpu, (BT,)), ds=Out(gpu, (BT, NC)), dS3=Out(gpu, (BT * NC, K3)))
    check(lib.cham_score_softmax_fwd(S3.data_ptr(), K3, w4.data_ptr(), b4.data_ptr(), BT, N, tau, mask.data_ptr(), o['logits'].ptr(), o['probs'].ptr(),
                                     o['nll'].ptr(), 0.0, None, None, None, _st()), "cham_score_softmax_fwd")
    check(lib.cham_score_softmax_bwd(S3.data_ptr(), K3, w4.data_ptr(), o['probs'].ptr(), mask.data_ptr(), BT, N, tau, float(sum_mask), o['ds'].ptr(),
                                     o['dS3'].ptr(), 0.0, None, None, None, None, _st()), "cham_score_softmax_bwd")
    return {k: v.get() for k, v in o.items()}


@pytest.mark.parametrize("N", [1, 4, 63, 64])
def test_softmax_at_k3_4_returns_the_cosine_bit_exactly(gpu, N):
    BT, NC, C, tau = 5, N + 1, 128, 0.1
    z, p, _, mask = CR.make_case(BT, NC, C, seed=4)
    fwd = _fwd(gpu, z, p)
    w4 = torch.tensor([1.0, 0.0, 0.0, 0.0], device=gpu)
    b4 = torch.zeros(4, device=gpu)
    md = mask.to(gpu)
    got = _softmax(gpu, fwd['cosq'], 4, w4, b4, md, tau, BT, N, float(mask.sum()))
    assert torch.equal(got['logits'].view(-1).view(torch.int32), fwd['cosq'][:, 0].contiguous().view(torch.int32)), "logits differ from cosq[:, 0] in a bit"
    # against float64.  Per click, relative to the row's max: the exponent's argument (|logit| / tau <= 10, two roundings + the max
    # subtracted) is off by <= 40 x 2^-24 absolute, expf and the division add a few ulps, the sum of NC terms NC x 2^-24: k = (NC + 48) 2^-23
    from tests import tail_reference as R
    k = (NC + 48) * 2.0 ** -23
    lg = got['logits'].cpu().double()
    pr = torch.softmax(lg / tau, -1)
    assert R.row_err(got['probs'].cpu().numpy(), pr.numpy()) <= k
    mk = mask.double()
    nll = -torch.log_softmax(lg / tau, -1)[:, 0] * mk
    assert float((got['nll'].cpu().double() - nll).abs().max()) <= k * (1.0 + float(nll.max()))
    dsr = (pr - torch.nn.functional.one_hot(torch.zeros(BT, dtype=torch.long), NC)) * mk[:, None] / (tau * mk.sum())
    assert R.row_err(got['ds'].cpu().numpy(), dsr.numpy()) <= k
    assert float(got['ds'][mask == 0].abs().max()) == 0.0 and float(got['nll'][mask == 0].abs().max()) == 0.0
    # ... and the K3 = 32 instance over the same rows padded with zeros gives the same bits: a sum that only adds exact zeros
    S32 = torch.zeros(BT * NC, 32, device=gpu)
    S32[:, 0] = fwd['cosq'][:, 0]
    w32 = torch.zeros(32, device=gpu)
    w32[0] = 1.0
    ref32 = _softmax(gpu, S32, 32, w32, b4, md, tau, BT, N, float(mask.sum()))
    for k in ('logits', 'probs', 'nll', 'ds'):
        assert torch.equal(got[k], ref32[k]), k
    assert torch.equal(got['dS3'], ref32['dS3'][:, :4]) and float(ref32['dS3'][:, 4:].abs().max()) == 0.0


def test_softmax_at_k3_32_is_what_it_was(gpu):
    """One case of tests/test_scorer_tail_gpu.py through the same entry points, in that file's bounds against its float64 reference - the K3 = 4
    instance is another template instance beside it - and two runs are bit-identical."""
    from tests import tail_reference as R
    from tests.test_scorer_tail_gpu import _backward, _dev, _forward
    from tests.test_tail_reference_cpu import gpu_bounds, softmax_case
    lib = _lib_()
    i = next(j for j, c in enumerate(R.SOFTMAX_CASES) if not softmax_case(j)[0]['bf16'] and softmax_case(j)[0]['sum_mask'] > 0)
    inp, ref = softmax_case(i)
    kb = gpu_bounds()
    d = {n: _dev(gpu, inp[n]) for n in ('w4', 'b4', 'mask', 'neg_ids', 'pop_norm', 'label_next')}
    d['S3'] = _dev(gpu, inp['S3'])
    assert lib.cham_set_log_bases(1.3, inp['pop_log_base']) == 0
    try:
        f1, f2 = _forward(gpu, lib, inp, d), _forward(gpu, lib, inp, d)
        fwd = {n: v.numpy() for n, v in f1.items()}
        assert all(R.same_bits(fwd[n], v.numpy()) for n, v in f2.items())
        assert R.rel_err(fwd['logits'], ref['logits']) <= kb['softmax.logits']
        assert R.row_err(fwd['probs'], ref['probs']) <= kb['softmax.probs']
        assert R.rel_err(fwd['nll'], ref['nll']) <= kb['softmax.nll']
        bwd = {n: v.numpy() for n, v in _backward(gpu, lib, inp, d, f1).items()}
        assert R.row_err(bwd['ds'], ref['ds']) <= kb['softmax.ds'] and R.row_err(bwd['dS3'], ref['dS3']) <= kb['softmax.dS3']
    finally:
        assert lib.cham_set_log_bases(1.3, 2.0) == 0


def test_argument_errors(gpu):
    lib = _lib_()
    x = torch.zeros(64, 128, device=gpu)
    u8 = torch.ones(8, dtype=torch.uint8, device=gpu)
    a = x.data_ptr()
    assert lib.cham_cosine_fwd(a, 128, a, 128, 2, 0, a, a, a, _st()) == -22           # no negatives
    assert lib.cham_cosine_fwd(a, 128, a, 126, 2, 3, a, a, a, _st()) == -22           # C % 4
    assert lib.cham_cosine_fwd(a, 64, a, 128, 2, 3, a, a, a, _st()) == -22            # row stride below C
    assert lib.cham_cosine_fwd(a + 4, 128, a, 128, 2, 3, a, a, a, _st()) == -22       # misaligned rows
    assert lib.cham_cosine_fwd(a, 128, a, 128, 0, 3, a, a, a, _st()) == 0             # nothing to do
    assert lib.cham_cosine_bwd(a, a, a, a, a, a, u8.data_ptr(), 128, 2, 6000, a, a, None, _st()) == -22      # more candidates than the LDS takes
    assert lib.cham_cosine_bwd_h2(a, a, a, a, a, a, u8.data_ptr(), 128, 2, 3, a, 64 * 128, None, a, None, _st()) == -22      # no scale record
    assert lib.cham_score_softmax_fwd(a, 8, a, a, 2, 3, 1.0, u8.data_ptr(), a, a, a, 0.0, None, None, None, _st()) == -22     # K3 is 32 or 4
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- the step
def _kink_flips(model, orc, mask):
    """Leaky-ReLU outputs whose sign differs between the HIP path and the oracle, over the sites this mode has: Z1 and FC1."""
    pl, taps = model._plan, orc.debug_taps
    B, T, NC, P = pl.B, pl.T, pl.NC, pl.P
    zin, zpos, zneg = taps['Z1']
    C = zin.shape[-1]
    Zin = pl.full_rows(pl.Z1[:P]).float().cpu().numpy()
    Zc = pl.full_rows(pl.cand_Z1(P), NC).float().cpu().numpy()
    n = int(((Zin.reshape(B, T, C) > 0) != (zin.numpy() > 0))[mask].sum())
    zc = torch.cat([zpos.unsqueeze(2), zneg], 2).numpy()
    n += int(((Zc.reshape(B, T, NC, C) > 0) != (zc > 0))[mask].sum())
    n += int(((pl.full_rows(pl.FC1).cpu().numpy().reshape(B, T, -1) > 0) != (taps['FC1'][0].numpy() > 0))[mask].sum())
    return n


def _compare_step(model, orc, f, l, st, loss_of=lambda ref: ref['xe_loss'], logit_tol=LOGIT_TOL):
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    model.feed_state(pop, buf)
    model.forward(model.upload_batch(f, l))
    out = model.outputs_numpy()
    for v in orc.w.values():
        v.grad = None
    orc.debug_taps = {}
    ref = orc.forward(f, l, buf, pop, 'train')
    assert np.array_equal(out['neg_items'], ref['neg_items'].numpy()), "negative samples must be bit exact"
    mask = ref['mask'].numpy()
    assert np.abs(out['logits'] - ref['logits'].detach().numpy())[mask].max() < logit_tol
    assert np.abs(out['probs'] - ref['probs'].detach().numpy())[mask].max() < logit_tol
    assert np.abs(out['logits'][mask]).max() <= 1.0 + 1e-6
    assert abs(out['loss'][2] - float(ref['reg_loss'].detach())) < 1e-5
    assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < LOGIT_TOL
    flips = _kink_flips(model, orc, mask)
    loss_of(ref).backward()
    model.backward()
    torch.cuda.synchronize()
    g = model.rt.logical_grads()
    assert set(g) == set(orc.w) and not [k for k in g if k.startswith('match')]
    tol = 3e-4 if flips == 0 else 0.25
    for k, v in orc.w.items():
        rg = v.grad.numpy() if v.grad is not None else np.zeros_like(v.detach().numpy())
        scale = max(1e-6, float(np.abs(rg).max()))
        err = float(np.abs(g[k] - rg).max())
        assert err < tol * scale + 2e-5, "grad %s: err %g scale %g (kink flips %d)" % (k, err, scale, flips)
    return flips


def _params(**over):
    return H.tiny_params(recommendations_ranking='cosine', **over)


def test_step_parity_tiny_warm_state(gpu):
    p = _params()
    batches = synthetic.make_batches(7, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:3])
    model, orc = CO.make_pair(p)
    assert model.rt.cosine and model.recommendations_ranking == 'cosine' and 'Ws1' not in model.rt.layout.entries
    flips = [_compare_step(model, orc, *batches[i], st) for i in (3, 4, 5, 6)]
    assert sum(1 for x in flips if x == 0) >= 2, "tight gradient parity needs kink-free batches: %r" % flips
    pl = model._plan
    assert not hasattr(pl, 'S1') and not hasattr(pl, 'dS3') and pl.cosq.shape == (pl.Rc, 4)


def test_step_parity_two_plane_arm_ragged_and_full_length(gpu):
    """C = 256: the default arithmetic keeps dZ2 as two fp16 planes under the record built from max |ds| rz."""
    from chameleon_recsys_amd.nar.candidate_rows import H2Rows
    p = _params(C=256, H=128, neg=12, batch_size=40)
    model, orc = CO.make_pair(p, seed=11)
    assert isinstance(model.rt.arm, H2Rows)
    flips = []
    for dist in ('g1', 'full'):
        batches = synthetic.make_batches(4 if dist == 'g1' else 3, 40, 8, 1000, p['session_features_config'], length_dist=dist)
        st = H.warm_state(p, batches[:2])
        for b in batches[2:]:
            flips.append(_compare_step(model, orc, *b, st))
            assert isinstance(model._plan.arm, H2Rows)
            rec = model._plan.sc_dz2.cpu()
            assert float(rec[2]) > 0.0 and 2.0 ** 14 <= float(rec[2]) * float(rec[0]) < 2.0 ** 15
    assert min(flips) == 0, flips


def test_step_parity_f32_native(gpu):
    p = _params(C=256, H=128, neg=12, batch_size=40, gemm_dtype='f32_native')
    batches = synthetic.make_batches(4, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    model, orc = CO.make_pair(p, seed=11)
    assert model.rt.arm is model.rt.f32_rows
    assert min(_compare_step(model, orc, *b, st) for b in batches[2:]) == 0


def test_step_parity_dropout(gpu):
    """keep_prob 0.9: the step runs on the fp32 rows of a plan built for the two-plane arm."""
    p = _params(C=256, H=96, neg=9, batch_size=40, dropout_keep_prob=0.9)
    batches = synthetic.make_batches(5, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    model, orc = CO.make_pair(p, seed=5)
    assert model.keep_prob == 0.9
    flips = []
    for b in batches[2:]:
        flips.append(_compare_step(model, orc, *b, st))
        assert model._plan.arm is model.rt.f32_rows
        model.rt.global_step += 1; orc.global_step += 1
    assert min(flips) == 0, flips


def test_step_parity_novelty_and_diversity_terms(gpu):
    from tests.diversity_oracle import clustered_ace
    for over in (dict(novelty_reg_factor=0.3), dict(diversity_reg_factor=1.0, content_article_embeddings_matrix=clustered_ace(1000, 64))):
        p = _params(**over)
        batches = synthetic.make_batches(6, 64, 8, 1000, p['session_features_config'], length_dist='g1')
        st = H.warm_state(p, batches[:3])
        model, orc = CO.make_pair(p)
        flips = []
        for b in batches[3:]:
            flips.append(_compare_step(model, orc, *b, st, loss_of=lambda ref: ref['total_loss'] - ref['reg_loss']))
        assert min(flips) == 0, (over.keys(), flips)
        with torch.no_grad():
            ref = orc.forward(*batches[5], st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy(), 'train')
        extra = abs(float(ref['total_loss']) - float(ref['xe_loss']) - float(ref['reg_loss']))
        assert extra > 0.02, "the term is meant not to be negligible here: %g" % extra


def test_padded_masked_path_equals_compacted(gpu):
    """CHAM_COMPACT=0 computes every padded position and masks it: the cosine forward still writes finite logits there, the backward writes
    zero rows, and logits at valid positions, loss and gradients equal the compacted step's (two-plane arm)."""
    p = _params(C=256, H=96, neg=9, batch_size=40)
    batches = synthetic.make_batches(3, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    mc, _ = CO.make_pair(p, seed=5)
    mp, _ = CO.make_pair(p, seed=5)
    mp.rt.compact = False
    f, l = batches[2]
    outs = []
    for m in (mc, mp):
        m.feed_state(st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer())
        d = m.upload_batch(f, l)
        m.forward(d); m.backward()
        torch.cuda.synchronize()
        outs.append((m.outputs_numpy(), m.rt.grads.clone(), d))
    (oc, gc, dc), (op, gp, dp_) = outs
    assert dc['pos'] is not None and dp_['pos'] is None and dc['P'] < dp_['P']
    mask = np.arange(f['item_clicked'].shape[1])[None, :] < (np.asarray(f['session_size']).reshape(-1, 1) - 1)
    assert np.isfinite(op['logits']).all() and np.isfinite(op['probs']).all()
    assert np.abs(oc['logits'] - op['logits'])[mask].max() < 1e-5
    assert np.abs(oc['loss'] - op['loss']).max() < 1e-5
    assert float((gc - gp).abs().max()) < 2e-5 * float(gp.abs().max()) + 1e-7
    pl = mp._plan
    dz = (pl.dZ2p[0].float() + pl.dZ2p[1].float())[:pl.PC].view(pl.BT, pl.NC, -1)
    assert float(dz[torch.from_numpy(~mask.reshape(-1)).to(gpu)].abs().max()) == 0.0 and float(dz.abs().max()) > 0.0


def test_step_parity_bf16(gpu):
    """bf16-resident candidate rows against the oracle emulating that rounding, in the bounds of test_step_parity_bf16_compute_mode: logits
    2e-3, loss 1e-3; gradients as close to the fp32 oracle's as the emulated bf16 gradients are (x 3 + 2 % of the tensor's max)."""
    p = _params(gemm_dtype='bf16')
    batches = synthetic.make_batches(5, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:3])
    model, orc = CO.make_pair(p)
    assert model.rt.gemm_dtype == 'bf16' and orc.gemm_dtype == 'bf16'
    orc32 = CO.CosineOracle(dict(p, gemm_dtype='f32'), weights=orc.weights_numpy())
    for f, l in batches[3:5]:
        buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
        model.feed_state(pop, buf)
        model.forward(model.upload_batch(f, l))
        out = model.outputs_numpy()
        grads = {}
        for name, o in (("bf16", orc), ("f32", orc32)):
            for v in o.w.values():
                v.grad = None
            ref = o.forward(f, l, buf, pop, 'train')
            if name == "bf16":
                mask = ref['mask'].numpy()
                assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
                assert np.abs(out['logits'] - ref['logits'].detach().numpy())[mask].max() < 2e-3
                assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < 1e-3
            else:
                assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < 3e-2
            ref['xe_loss'].backward()
            grads[name] = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy())) for k, v in o.w.items()}
        model.backward()
        torch.cuda.synchronize()
        g = model.rt.logical_grads()
        for k in g:
            scale = max(1e-6, float(np.abs(grads["f32"][k]).max()))
            e_hip = float(np.abs(g[k] - grads["f32"][k]).max())
            e_emu = float(np.abs(grads["bf16"][k] - grads["f32"][k]).max())
            assert e_hip < 3.0 * e_emu + 2e-2 * scale + 2e-5, (k, e_hip, e_emu, scale)
        H.update_state(st, f, l)


# ---------------------------------------------------------------------------------------------------- training, evaluation
def test_training_curve_matches_oracle(gpu):
    """Thirty optimizer steps with the state evolving: every loss within 1e-3 of CosineOracle's, then the Adam slots."""
    steps = 30
    p = _params()
    batches = synthetic.make_batches(steps, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, [])
    model, orc = CO.make_pair(p)
    sig = None
    for i, (f, l) in enumerate(batches):
        buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
        model.feed_state(pop, buf)
        loss = model.train_step(model.upload_batch(f, l)).cpu().numpy()
        ref = orc.train_step(f, l, buf, pop, return_grads=True)
        sig = H.grad_significance(ref['grads'], acc=sig)
        assert np.array_equal(model._plan.neg_ids.cpu().numpy(), ref['neg_items'].numpy())
        assert abs(loss[0] - float(ref['total_loss'])) < LOGIT_TOL, (i, loss, float(ref['total_loss']))
        H.update_state(st, f, l)
    H.assert_adam_state_close(model, orc, p['lr'], n_steps=steps, w_tol=0.2, sig_every_step=sig)


def test_training_is_bit_reproducible(gpu):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    p = _params(C=256, H=128, neg=12)
    batches = synthetic.make_batches(4, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    runs = []
    for _ in range(2):
        model, _o = CO.make_pair(p)
        st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], 1000)
        dev = [model.upload_batch(f, l) for f, l in batches]
        losses = []
        for i, d in enumerate(dev):
            model.feed_state(st, st)
            losses.append(model.train_step(d).clone())
            st.update_from_device_batch(d['aci'], d['g_event_ts'])
            if i + 1 < len(dev):
                model.presample(dev[i + 1])
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), model.rt.flat.cpu().clone(), model.rt.m.cpu().clone(), model.rt.v.cpu().clone()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    assert float(runs[0][2].abs().max()) > 0.0


def test_eval_label_rank_matches_oracle(gpu):
    """cosine_oracle.EVAL: label_rank of every valid click whose oracle probabilities separate the label from every other candidate by more than
    2 x LOGIT_TOL - at least 90 % of the valid clicks (tests/test_cosine_cpu.py checks that for the oracle alone)."""
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p, st, (f, l) = CO.eval_setup()
    w = CO.pair_weights(p, CO.EVAL['weight_seed'])
    rt = NARRuntime(p, seed=CO.EVAL['weight_seed'], weights=w)
    ev = CO.make_model(p, rt, ModeKeys.EVAL)
    orc = CO.CosineOracle(p, weights=w)
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    ev.feed_state(pop, buf)
    ev.evaluate_step(ev.upload_batch(f, l))
    with torch.no_grad():
        ref = orc.forward(f, l, buf, pop, mode='eval', step=NARModuleModel.eval_step_key(0, 0))
    out = ev.outputs_numpy()
    mask = ref['mask'].numpy()
    assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
    assert np.abs(out['probs'] - ref['probs'].numpy())[mask].max() < LOGIT_TOL
    sep = CO.separated_clicks(ref['probs'].numpy(), mask, 2 * LOGIT_TOL)
    assert 1.0 - sep.sum() / mask.sum() <= CO.EVAL['max_excluded']
    rank = ev.label_rank.eval()
    assert np.array_equal(rank[sep], CO.label_rank(ref['probs'].numpy())[sep])
    assert (rank[~mask] == -1).all() and (rank[mask] >= 0).all()


def test_graphed_step_declines_a_cosine_model(gpu):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import GraphedTrainStep
    p = _params()
    model, _ = CO.make_pair(p)
    full = synthetic.make_batches(1, 64, 8, 1000, p['session_features_config'], length_dist='full')
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], 1000)
    gs = GraphedTrainStep(model, st)
    d = model.upload_batch(*full[0])
    st.update_from_device_batch(d['aci'], d['g_event_ts'])
    model.feed_state(st, st)
    model.train_step(d)                                    # an eager step on the device-resident state: the shape is warm
    assert "cosine" in gs.supports(d)
    with pytest.raises(RuntimeError, match="GraphedTrainStep: cosine"):
        gs.step(d, d)
    assert gs.graph is None
