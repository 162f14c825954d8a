"""Pairwise ranking losses (--loss_function bpr | top1 | bpr_max | top1_max) on the GPU: the kernels of csrc/rank_loss.hip against the float64
reference of tests/rankloss_reference.py, and the step / training / evaluation against tests/rankloss_oracle.py.

Kernel bounds (tests/rankloss_reference.kernel_bounds), per click, for nll and for ds: the larger of 4 x the fp32 host restatement's own
deviation from float64 at that click and (N + 32) eps sum|terms|, + (N + 32) 2^-126 for terms below the smallest normal fp32 number.  The
logits are known exactly (w4 = e_0, b4 = 0, the values in column 0 of S3), so the reference never reads them from the kernel.
Step bounds are those of tests/test_cosine_gpu._compare_step: negatives bit-exact, logits / probs / loss within 1e-3, gradients within
3e-4 max|ref| + 2e-5 on batches without a leaky-ReLU kink flip.
profiles/rankloss_notes.md records the worst observed error / bound ratios of the kernel tests."""
import os

import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from tests import cosine_oracle as CO
from tests import helpers as H
from tests import rankloss_oracle as RO
from tests import rankloss_reference as RR
from tests.test_cosine_gpu import Out, _lib_, _st

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
EPS = 2.0 ** -24
KIND_ID = {k: i + 1 for i, k in enumerate(RR.KINDS)}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rankloss_softmax_guard.npz")


# ---------------------------------------------------------------------------------------------------- the kernels
def _s3(gpu, s, K3, b16, seed):
    """Device S3 [BT * NC, K3] with the logits s [BT, NC] in column 0 and noise of both signs in the other columns."""
    BT, NC = s.shape
    g = torch.Generator().manual_seed(seed)
    S3 = torch.randn(BT * NC, K3, generator=g)
    S3[:, 0] = s.reshape(-1)
    S3 = S3.to(gpu)
    return S3.bfloat16() if b16 else S3


def _run(gpu, kind, S3, K3, w4, b4, mask, tau, lam, BT, N, sum_mask, b16=False, dev_scalars=None):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    NC = N + 1
    o = dict(logits=Out(gpu, (BT, NC)), probs=Out(gpu, (BT, NC)), nll=Out(gpu, (BT,)), aux=Out(gpu, (BT, 8)), ds=Out(gpu, (BT, NC)),
             dS3=Out(gpu, (BT * NC, K3), torch.bfloat16 if b16 else torch.float32))
    sfx = '_b16' if b16 else ''
    check(getattr(lib, 'cham_score_rankloss_fwd' + sfx)(S3.data_ptr(), K3, w4.data_ptr(), b4.data_ptr(), BT, N, tau, mask.data_ptr(), o['logits'].ptr(),
                                                        o['probs'].ptr(), o['nll'].ptr(), 0.0, None, None, None, KIND_ID[kind], lam, o['aux'].ptr(), _st()),
          "cham_score_rankloss_fwd")
    if dev_scalars is None:
        fn, sm = getattr(lib, 'cham_score_rankloss_bwd' + sfx), float(sum_mask)
    else:
        fn, sm = getattr(lib, 'cham_score_rankloss_bwd' + sfx + '_dev'), dev_scalars.data_ptr()
    check(fn(S3.data_ptr(), K3, w4.data_ptr(), o['probs'].ptr(), mask.data_ptr(), BT, N, tau, sm, o['ds'].ptr(), o['dS3'].ptr(), 0.0, None, None,
             o['logits'].ptr(), None, KIND_ID[kind], lam, o['aux'].ptr(), _st()), "cham_score_rankloss_bwd")
    return {k: v.get() for k, v in o.items()}


def _mask(BT):
    m = torch.ones(BT, dtype=torch.uint8)
    if BT > 1:
        m[1::3] = 0          # rows set and cleared
    return m


def _e0(gpu, K3):
    w4 = torch.zeros(K3, device=gpu)
    w4[0] = 1.0
    return w4, torch.zeros(4, device=gpu)


SHAPES = [(BT, N) for BT in (1, 5, 9) for N in RR.GRID_N]


@pytest.mark.parametrize("b16", [False, True])
@pytest.mark.parametrize("K3", [32, 4])
@pytest.mark.parametrize("kind", RR.KINDS)
def test_kernels_against_float64(gpu, kind, K3, b16):
    w4, b4 = _e0(gpu, K3)
    worst_nll = worst_ds = worst_p = 0.0
    lam = 0.5
    for BT, N in SHAPES:
        NC = N + 1
        for scale in RR.GRID_SCALE:
            for tau in (1.0, 0.7):
                s = RR.make_logits(BT, N, scale, seed=5)
                if b16:
                    s = s.bfloat16().float()          # the logits as that arm stores them
                mask = _mask(BT)
                S3 = _s3(gpu, s, K3, b16, seed=BT * 131 + N)
                got = _run(gpu, kind, S3, K3, w4, b4, mask.to(gpu), tau, lam, BT, N, float(mask.sum()), b16)
                label = (kind, K3, b16, BT, N, scale, tau)
                for k, v in got.items():
                    assert bool(torch.isfinite(v.float()).all()), (label, k)
                assert torch.equal(got['logits'].cpu().view(torch.int32), s.view(torch.int32)), (label, "logits differ from column 0 of S3 in a bit")
                ref = RR.reference(kind, s, tau, lam, mask)
                nll_tol, ds_tol = RR.kernel_bounds(kind, s, tau, lam, mask)
                e_nll = (got['nll'].cpu().double() - ref['nll']).abs()
                e_ds = (got['ds'].cpu().double() - ref['ds']).abs().amax(-1)
                worst_nll, worst_ds = max(worst_nll, float((e_nll / nll_tol).max())), max(worst_ds, float((e_ds / ds_tol).max()))
                assert bool((e_nll <= nll_tol).all()), (label, "nll", float((e_nll / nll_tol).max()))
                assert bool((e_ds <= ds_tol).all()), (label, "ds", float((e_ds / ds_tol).max()))
                # probs = softmax(logits / tau) over all candidates, per click relative to the row's max (1 at most): the exponent's argument
                # r - max r is off by <= 3 eps max|r|, expf and the division add a few ulps, the sum of NC terms NC eps
                k = (NC + 48 + 6.0 * float(s.abs().max()) / tau) * 2.0 ** -23
                e_p = float((got['probs'].cpu().double() - ref['probs']).abs().max())
                worst_p = max(worst_p, e_p / k)
                assert e_p <= k, (label, "probs", e_p, k)
                # masked clicks: exactly zero
                off = mask == 0
                if bool(off.any()):
                    assert float(got['nll'].cpu()[off].abs().max()) == 0.0 and float(got['ds'].cpu()[off].abs().max()) == 0.0, label
                    assert float(got['dS3'].cpu().view(BT, NC, K3)[off].float().abs().max()) == 0.0, label
                # dS3 = ds w4 leaky'(S3): column 0 carries ds x {1, 0.2}, the other columns w4 = 0
                want = got['ds'].view(-1) * torch.where(S3[:, 0].float() > 0, 1.0, 0.2)
                d0 = got['dS3'][:, 0]
                assert torch.equal(d0, want.bfloat16() if b16 else want), label
                assert float(got['dS3'][:, 1:].float().abs().max()) == 0.0, label
                # a second launch gives the same bits
                again = _run(gpu, kind, S3, K3, w4, b4, mask.to(gpu), tau, lam, BT, N, float(mask.sum()), b16)
                assert all(torch.equal(got[n].view(torch.int16 if got[n].dtype == torch.bfloat16 else torch.int32),
                                       again[n].view(torch.int16 if again[n].dtype == torch.bfloat16 else torch.int32)) for n in got), label
        assert float(ref['ds'].abs().max()) > 0.0
    print("rankloss %s K3 %d %s: worst error / bound: nll %.3f, ds %.3f, probs %.3f" % (kind, K3, 'bf16' if b16 else 'fp32', worst_nll, worst_ds, worst_p))


@pytest.mark.parametrize("kind", RR.KINDS)
def test_kernels_with_a_general_last_layer(gpu, kind):
    """K3 = 32 with a dense w4 and a bias: logits within the dot product's bound (33 eps sum|terms|: 32 products, their sums and the bias),
    dS3 = ds w4 leaky'(S3) from the ds the kernel wrote, and the loss read from the kernel's own logits."""
    BT, N, K3, tau, lam = 9, 70, 32, 0.7, 0.5
    NC = N + 1
    g = torch.Generator().manual_seed(11)
    S3c, w4c, b4c = torch.randn(BT * NC, K3, generator=g), torch.randn(K3, generator=g), torch.randn(1, generator=g)
    mask = _mask(BT)
    S3, w4, b4 = S3c.to(gpu), w4c.to(gpu), torch.cat([b4c, torch.zeros(3)]).to(gpu)
    got = _run(gpu, kind, S3, K3, w4, b4, mask.to(gpu), tau, lam, BT, N, float(mask.sum()))
    ref_logits = (S3c.double() @ w4c.double() + b4c.double()).view(BT, NC)
    bound = 33 * EPS * ((S3c.double().abs() @ w4c.double().abs()) + b4c.double().abs()).view(BT, NC)
    assert bool(((got['logits'].cpu().double() - ref_logits).abs() <= bound).all())
    s = got['logits'].cpu()
    ref = RR.reference(kind, s, tau, lam, mask)
    nll_tol, ds_tol = RR.kernel_bounds(kind, s, tau, lam, mask)
    assert bool(((got['nll'].cpu().double() - ref['nll']).abs() <= nll_tol).all())
    assert bool(((got['ds'].cpu().double() - ref['ds']).abs().amax(-1) <= ds_tol).all())
    want = (got['ds'].view(-1, 1) * w4.view(1, -1)) * torch.where(S3 > 0, 1.0, 0.2)          # the kernel's operation order: exact
    assert torch.equal(got['dS3'], want)
    # sum(mask) from the step-scalar record: the same bits as by value
    lib = _lib_()
    rec = torch.zeros(int(lib.cham_step_scalars_bytes()), dtype=torch.uint8, device=gpu)
    assert lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, 0, float(mask.sum()), 0.0, 7, _st()) == 0
    dev = _run(gpu, kind, S3, K3, w4, b4, mask.to(gpu), tau, lam, BT, N, 0.0, dev_scalars=rec)
    assert torch.equal(dev['ds'], got['ds']) and torch.equal(dev['dS3'], got['dS3'])


def test_novelty_term_rides_on_every_loss(gpu):
    """nll and ds with novelty_reg_factor = 0.3 differ from the factor-0 run by what the softmax pair's novelty term adds on the same inputs."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    BT, N, K3, tau, f = 5, 66, 4, 0.7, 0.3
    NC = N + 1
    s = RR.make_logits(BT, N, 2.0, seed=6)
    w4, b4 = _e0(gpu, K3)
    S3 = _s3(gpu, s, K3, False, seed=3)
    mask = _mask(BT).to(gpu)
    g = torch.Generator().manual_seed(2)
    neg = torch.randint(0, 50, (BT, N), generator=g).to(gpu)
    pop = (torch.rand(50, generator=g) * 0.9 + 0.05).to(gpu)
    sm = float(mask.sum())

    def pair(fwd, bwd, extra_f, extra_b, factor):
        o = dict(logits=Out(gpu, (BT, NC)), probs=Out(gpu, (BT, NC)), nll=Out(gpu, (BT,)), nov=Out(gpu, (BT, 3)), ds=Out(gpu, (BT, NC)), dS3=Out(gpu, (BT * NC, K3)))
        check(fwd(S3.data_ptr(), K3, w4.data_ptr(), b4.data_ptr(), BT, N, tau, mask.data_ptr(), o['logits'].ptr(), o['probs'].ptr(), o['nll'].ptr(), factor,
                  neg.data_ptr(), pop.data_ptr(), o['nov'].ptr(), *extra_f, _st()), "fwd")
        check(bwd(S3.data_ptr(), K3, w4.data_ptr(), o['probs'].ptr(), mask.data_ptr(), BT, N, tau, sm, o['ds'].ptr(), o['dS3'].ptr(), factor, neg.data_ptr(),
                  pop.data_ptr(), o['logits'].ptr(), o['nov'].ptr(), *extra_b, _st()), "bwd")
        torch.cuda.synchronize()
        return {k: (v.t.clone() if k == 'nov' and factor == 0.0 else v.get()) for k, v in o.items()}
    soft = [pair(lib.cham_score_softmax_fwd, lib.cham_score_softmax_bwd, (), (), x) for x in (0.0, f)]
    for kind in RR.KINDS:
        aux = torch.zeros(BT, 8, device=gpu)
        extra = (KIND_ID[kind], 0.5, aux.data_ptr())
        rank = [pair(lib.cham_score_rankloss_fwd, lib.cham_score_rankloss_bwd, extra, extra, x) for x in (0.0, f)]
        assert torch.equal(rank[1]['nov'], soft[1]['nov']), kind          # {max, sum, q . nov}: the same arithmetic
        # each side is a difference of two fp32 values (eps of each); the exponent's argument r_n - max may be contracted into an fma in one
        # kernel and not in the other (|r| eps of the term)
        k = (8.0 + 2.0 * float(s.abs().max()) / tau) * EPS
        for name, scale in (('nll', 1.0), ('ds', 1.0 / (tau * sm))):
            a, b = rank[1][name].double() - rank[0][name].double(), soft[1][name].double() - soft[0][name].double()
            mag = torch.maximum(rank[0][name].abs(), soft[0][name].abs()).double() + b.abs()
            assert bool(((a - b).abs() <= k * mag + 1e-12).all()), (kind, name)
            assert float(b.abs().max()) > 1e-3 * scale


def test_argument_errors(gpu):
    lib = _lib_()
    x = torch.zeros(64, 32, device=gpu)
    u8 = torch.ones(8, dtype=torch.uint8, device=gpu)
    a, m = x.data_ptr(), u8.data_ptr()
    canary = torch.full((64,), 7.0, device=gpu)
    c = canary.data_ptr()
    for sfx in ('', '_b16'):
        fwd = getattr(lib, 'cham_score_rankloss_fwd' + sfx)

        def f(K3=32, BT=2, N=3, tau=1.0, kind=1, S3=a, w4=a, b4=a, mask=m, logits=c, probs=c, nll=c, aux=c, factor=0.0):
            return fwd(S3, K3, w4, b4, BT, N, tau, mask, logits, probs, nll, factor, None, None, None, kind, 0.5, aux, _st())
        assert f(kind=0) == -22 and f(kind=5) == -22 and f(N=0) == -22 and f(tau=0.0) == -22 and f(tau=-1.0) == -22 and f(K3=8) == -22 and f(BT=0) == -22
        for name in ('S3', 'w4', 'b4', 'mask', 'logits', 'probs', 'nll', 'aux'):
            assert f(**{name: None}) == -22, name
        assert f(factor=0.3) == -22          # the novelty term without its arrays
        for dev in ('', '_dev'):
            bwd = getattr(lib, 'cham_score_rankloss_bwd' + sfx + dev)
            rec = torch.zeros(64, dtype=torch.uint8, device=gpu)
            sm_ok = rec.data_ptr() if dev else 3.0

            def b(K3=32, BT=2, N=3, tau=1.0, kind=1, sm=sm_ok, S3=a, w4=a, mask=m, ds=c, dS3=c, logits=a, aux=a, factor=0.0):
                return bwd(S3, K3, w4, a, mask, BT, N, tau, sm, ds, dS3, factor, None, None, logits, None, kind, 0.5, aux, _st())
            assert b(kind=0) == -22 and b(kind=5) == -22 and b(N=0) == -22 and b(tau=0.0) == -22 and b(K3=8) == -22 and b(BT=0) == -22
            assert b(sm=None if dev else 0.0) == -22 and b(factor=0.3) == -22
            for name in ('S3', 'w4', 'mask', 'ds', 'dS3', 'logits', 'aux'):
                assert b(**{name: None}) == -22, name
    torch.cuda.synchronize()
    assert float(canary.min()) == 7.0 and float(canary.max()) == 7.0, "a refused call launched"


def softmax_guard_inputs():
    """The fixed input of the regression guard on scorer.hip (host tensors)."""
    BT, N, K3 = 6, 66, 32
    g = torch.Generator().manual_seed(20)
    return dict(S3=torch.randn(BT * (N + 1), K3, generator=g), w4=torch.randn(K3, generator=g) * 0.5, b4=torch.cat([torch.randn(1, generator=g), torch.zeros(3)]),
                mask=torch.tensor([1, 0, 1, 1, 0, 1], dtype=torch.uint8), neg_ids=torch.randint(0, 40, (BT, N), generator=g),
                pop_norm=torch.rand(40, generator=g) * 0.9 + 0.05)


def softmax_guard_run(gpu, inp):
    """cham_score_softmax_fwd + _bwd (tau 0.7, novelty factor 0.3) on `inp` -> numpy outputs."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    d = {k: torch.as_tensor(v).to(gpu) for k, v in inp.items()}
    BT, N, K3, tau, f = 6, 66, 32, 0.7, 0.3
    NC = N + 1
    o = dict(logits=Out(gpu, (BT, NC)), probs=Out(gpu, (BT, NC)), nll=Out(gpu, (BT,)), nov_aux=Out(gpu, (BT, 3)), ds=Out(gpu, (BT, NC)), dS3=Out(gpu, (BT * NC, K3)))
    check(lib.cham_score_softmax_fwd(d['S3'].data_ptr(), K3, d['w4'].data_ptr(), d['b4'].data_ptr(), BT, N, tau, d['mask'].data_ptr(), o['logits'].ptr(),
                                     o['probs'].ptr(), o['nll'].ptr(), f, d['neg_ids'].data_ptr(), d['pop_norm'].data_ptr(), o['nov_aux'].ptr(), _st()), "fwd")
    check(lib.cham_score_softmax_bwd(d['S3'].data_ptr(), K3, d['w4'].data_ptr(), o['probs'].ptr(), d['mask'].data_ptr(), BT, N, tau, 4.0, o['ds'].ptr(),
                                     o['dS3'].ptr(), f, d['neg_ids'].data_ptr(), d['pop_norm'].data_ptr(), o['logits'].ptr(), o['nov_aux'].ptr(), _st()), "bwd")
    return {k: v.get().cpu().numpy() for k, v in o.items()}


def test_softmax_entry_points_give_the_bits_they_gave(gpu):
    """tests/golden/rankloss_softmax_guard.npz: the input above and what cham_score_softmax_fwd / _bwd returned for it on an MI355X, recorded
    from csrc/scorer.hip as it stood when csrc/rank_loss.hip was added beside it (its translation unit was not changed): the default loss's
    kernels are not to be touched by work on the other losses."""
    z = np.load(GOLDEN)
    inp = {k[3:]: z[k] for k in z.files if k.startswith('in_')}
    fresh = softmax_guard_inputs()
    assert all(np.array_equal(inp[k], fresh[k].numpy()) for k in fresh)
    got = softmax_guard_run(gpu, inp)
    for k, v in got.items():
        assert np.array_equal(v.view(np.int32), z['out_' + k].view(np.int32)), k


# ---------------------------------------------------------------------------------------------------- the step
def _kink_flips(model, orc, mask):
    if model.rt.cosine:
        from tests.test_cosine_gpu import _kink_flips as flips
    else:
        from tests.test_step_gpu import _kink_flips as flips
    return flips(model, orc, mask)


def _data_loss(ref):
    return ref['total_loss'] - ref['reg_loss']          # what the HIP backward differentiates (L2 is added inside the Adam kernel)


def _compare_step(model, orc, f, l, st, logit_tol=LOGIT_TOL, probs_tol=LOGIT_TOL, loss_tol=lambda total: LOGIT_TOL):
    """tests/test_cosine_gpu._compare_step without what is particular to the cosine head."""
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
    assert np.abs(out['probs'] - ref['probs'].detach().numpy())[mask].max() < probs_tol
    assert abs(out['loss'][2] - float(ref['reg_loss'].detach())) < 1e-5
    total = float(ref['total_loss'].detach())
    assert abs(out['loss'][0] - total) < loss_tol(total), (out['loss'], total)
    flips = _kink_flips(model, orc, mask)
    _data_loss(ref).backward()
    model.backward()
    torch.cuda.synchronize()
    g = model.rt.logical_grads()
    assert set(g) == set(orc.w)
    tol = 3e-4 if flips == 0 else 0.25
    for k, v in orc.w.items():
        rg = v.grad.numpy() if v.grad is not None else np.zeros_like(v.detach().numpy())
        assert np.isfinite(g[k]).all(), k
        scale = max(1e-6, float(np.abs(rg).max()))
        err = float(np.abs(g[k] - rg).max())
        assert err < tol * scale + 2e-5, "grad %s: err %g scale %g (kink flips %d)" % (k, err, scale, flips)
    return flips, ref


def _parity(p, seed=3, n_warm=3, n=3, B=64, dist='g1', step_counter=False, check=None, weight_scale=None, clean=True, **tols):
    batches = synthetic.make_batches(n_warm + n, B, 8, 1000, p['session_features_config'], length_dist=dist)
    st = H.warm_state(p, batches[:n_warm])
    model, orc = RO.make_pair(p, seed=seed, weight_scale=weight_scale)
    assert model.loss_function == p['loss_function']
    flips = []
    for b in batches[n_warm:]:
        fl, ref = _compare_step(model, orc, *b, st, **tols)
        flips.append(fl)
        assert model._plan.rank_aux is not None
        if check is not None:
            check(model, ref)
        if step_counter:
            model.rt.global_step += 1; orc.global_step += 1
    assert not clean or min(flips) == 0, flips          # tight gradient parity needs a batch without a kink flip
    model.flips = flips
    return model, orc


@pytest.mark.parametrize("kind", RR.KINDS)
def test_step_parity_mlp_head_warm_state(gpu, kind):
    model, _ = _parity(H.tiny_params(loss_function=kind), n=4)
    assert not model.rt.cosine and model._plan.rank_aux.shape == (model._plan.BT, 8)


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_step_parity_cosine_head(gpu, kind):
    model, _ = _parity(H.tiny_params(loss_function=kind, recommendations_ranking='cosine'), n=4)
    assert model.rt.cosine


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_step_parity_two_plane_arm_ragged_and_full_length(gpu, kind):
    from chameleon_recsys_amd.nar.candidate_rows import H2Rows
    p = H.tiny_params(C=256, H=128, neg=12, batch_size=40, loss_function=kind)
    flips = []
    for dist in ('g1', 'full'):
        model, _ = _parity(p, seed=11, n_warm=2, n=2 if dist == 'g1' else 1, B=40, dist=dist, clean=False,
                           check=lambda m, ref: isinstance(m._plan.arm, H2Rows) or pytest.fail("not the two-plane arm"))
        assert isinstance(model.rt.arm, H2Rows)
        flips += model.flips
    assert min(flips) == 0, flips


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_step_parity_f32_native(gpu, kind):
    p = H.tiny_params(C=256, H=128, neg=12, batch_size=40, gemm_dtype='f32_native', loss_function=kind)
    model, _ = _parity(p, seed=11, n_warm=2, n=2, B=40)
    assert model.rt.arm is model.rt.f32_rows


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_step_parity_dropout(gpu, kind):
    p = H.tiny_params(C=256, H=96, neg=9, batch_size=40, dropout_keep_prob=0.9, loss_function=kind)
    model, _ = _parity(p, seed=5, n_warm=2, n=3, B=40, step_counter=True)
    assert model.keep_prob == 0.9 and model._plan.arm is model.rt.f32_rows


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_step_parity_novelty_and_diversity_terms(gpu, kind):
    from tests.diversity_oracle import clustered_ace
    p = H.tiny_params(loss_function=kind, novelty_reg_factor=0.3, diversity_reg_factor=0.5, content_article_embeddings_matrix=clustered_ace(1000, 64))
    extras = []
    _parity(p, check=lambda m, ref: extras.append(abs(float(ref['total_loss'].detach()) - float(ref['xe_loss'].detach()) - float(ref['reg_loss'].detach()))))
    assert max(extras) > 0.02, "the two terms are meant not to be negligible here: %r" % extras


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_step_parity_bf16(gpu, kind):
    """tests/test_cosine_gpu.test_step_parity_bf16's criterion: logits 2e-3 and loss 1e-3 against the oracle emulating the rounding; gradients
    as close to the fp32 oracle's as the emulated bf16 gradients are (x 3 + 2 % of the tensor's max)."""
    p = H.tiny_params(gemm_dtype='bf16', loss_function=kind)
    batches = synthetic.make_batches(5, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:3])
    model, orc = RO.make_pair(p)
    assert model.rt.gemm_dtype == 'bf16' and orc.gemm_dtype == 'bf16'
    orc32 = RO.make_oracle(dict(p, gemm_dtype='f32'), orc.weights_numpy())
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
            _data_loss(ref).backward()
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


def test_step_with_large_scores_on_the_two_plane_arm(gpu):
    """bpr_max with lambda = 4 and the last scorer layer scaled until |r| = |logit| / tau reaches about 30: the gradients at the logits
    grow with lambda |r|, the scale records of the two-plane arm follow them (they are measured on the device: the row norms of dS1,
    nar/candidate_rows.py H2Rows.scorer_dgrad), and every gradient stays finite and within the step bounds.  The forward bounds keep their
    RELATIVE size: the last layer is linear in its kernel, so the logits' bound grows by the factor it is scaled with; a softmax moves by at
    most half the largest change of its arguments; the loss (lambda sum q r^2 ~ 10^3) is held to 1e-3 of its magnitude."""
    from chameleon_recsys_amd.nar.candidate_rows import H2Rows
    p = H.tiny_params(C=256, H=128, neg=12, batch_size=40, loss_function='bpr_max', bpr_max_reg=4.0)
    batches = synthetic.make_batches(5, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    probe = RO.make_oracle(p, CO.pair_weights(p, 11))
    with torch.no_grad():
        out = probe.forward(*batches[2], st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy(), 'train')
    tau = p['softmax_temperature']
    b4 = float(probe.w['match4/bias'].detach().abs().max())
    factor = 30.0 * tau / float((out['logits'][out['mask']].abs().max() - b4).clamp(min=1e-6))
    seen = []

    def check(m, ref):
        assert isinstance(m._plan.arm, H2Rows)
        seen.append(float(ref['logits'].detach()[ref['mask']].abs().max()) / tau)
    logit_tol = LOGIT_TOL * max(1.0, factor)
    _parity(p, seed=11, n_warm=2, n=3, B=40, check=check, weight_scale={'match4/kernel': factor}, logit_tol=logit_tol,
            probs_tol=min(1.0, 0.5 * logit_tol / tau), loss_tol=lambda total: LOGIT_TOL * max(1.0, abs(total)))
    assert 20.0 <= max(seen) <= 45.0, seen


def test_training_curve_matches_oracle(gpu):
    """Twenty optimizer steps under bpr_max with the state evolving: every loss within 1e-3 of the oracle's, then the Adam slots."""
    steps = 20
    p = H.tiny_params(loss_function='bpr_max')
    batches = synthetic.make_batches(steps, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, [])
    model, orc = RO.make_pair(p)
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


@pytest.mark.parametrize("kind", ['bpr_max', 'top1'])
def test_training_is_bit_reproducible(gpu, kind):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    p = H.tiny_params(C=256, H=128, neg=12, loss_function=kind)
    batches = synthetic.make_batches(4, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    runs = []
    for _ in range(2):
        model, _o = RO.make_pair(p)
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


def test_eval_ranks_match_the_oracle_under_every_loss(gpu):
    """The ranked lists are the softmax's under every loss.  label_rank is compared on the valid clicks whose ORACLE probabilities separate the
    label from every other candidate by more than 2 x 1e-3, the ranked ids on those where every pair of candidates is that far apart."""
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p0 = H.tiny_params(neg=5)
    batches = synthetic.make_batches(4, 64, 8, 1000, p0['session_features_config'], length_dist='g1')
    st = H.warm_state(p0, batches[:3])
    f, l = batches[3]
    w = CO.pair_weights(p0, 6)
    rt = NARRuntime(p0, seed=6, weights=w)
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    ranks = []
    for kind in RR.KINDS:
        p = dict(p0, loss_function=kind)
        ev = RO.make_model(p, rt, ModeKeys.EVAL)
        orc = RO.make_oracle(p, w)
        ev.feed_state(pop, buf)
        ev.evaluate_step(ev.upload_batch(f, l))
        with torch.no_grad():
            ref = orc.forward(f, l, buf, pop, mode='eval', step=NARModuleModel.eval_step_key(0, 0))
        out = ev.outputs_numpy()
        mask = ref['mask'].numpy()
        pr = ref['probs'].numpy()
        assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
        assert np.abs(out['probs'] - pr)[mask].max() < LOGIT_TOL
        assert abs(out['loss'][0] - float(ref['total_loss'])) < LOGIT_TOL
        sep = CO.separated_clicks(pr, mask, 2 * LOGIT_TOL)
        gaps = np.abs(pr[..., :, None] - pr[..., None, :]) + np.eye(pr.shape[-1]) * 10.0
        full = mask & (gaps.min((-1, -2)) > 2 * LOGIT_TOL)
        assert sep.sum() >= 50 and full.sum() >= 20, (int(mask.sum()), int(sep.sum()), int(full.sum()))
        rank = ev.label_rank.eval()
        assert np.array_equal(rank[sep], CO.label_rank(pr)[sep])
        assert (rank[~mask] == -1).all() and (rank[mask] >= 0).all()
        ids = ev.predicted_item_ids.eval().reshape(ref['predicted_item_ids'].shape)
        assert np.array_equal(ids[full], ref['predicted_item_ids'].numpy()[full])
        ranks.append(rank)
    assert all(np.array_equal(ranks[0], r) for r in ranks[1:])          # the same runtime, the same lists


class _LibSpy:
    """The library with the name of every entry point called kept in one list (what tests/recording.py does for the driver modules)."""

    def __init__(self, lib):
        self._lib, self.log = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not callable(fn):
            return fn

        def call(*a):
            self.log.append(name)
            return fn(*a)
        return call


def test_default_is_the_model_without_the_argument(gpu):
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    p = H.tiny_params()
    batches = synthetic.make_batches(3, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    runs = []
    for pass_loss in (False, True):
        w = CO.pair_weights(p, 3)
        rt = NARRuntime(p, seed=3, weights=w)
        model = RO.make_model(dict(p, loss_function='softmax'), rt, pass_loss=pass_loss)
        assert model.loss_function == 'softmax' and model.bpr_max_reg == 0.5
        spy = rt.lib = _LibSpy(rt.lib)
        st = H.warm_state(p, [])
        losses = []
        for f, l in batches:
            model.feed_state(st.get_articles_recent_pop_norm().copy(), st.get_recent_clicks_buffer().copy())
            losses.append(model.train_step(model.upload_batch(f, l)).clone())
            H.update_state(st, f, l)
        torch.cuda.synchronize()
        assert model._plan.rank_aux is None
        runs.append((torch.stack(losses).cpu(), rt.flat.cpu().clone(), rt.m.cpu().clone(), rt.v.cpu().clone(), list(spy.log)))
    for a, b in zip(runs[0][:4], runs[1][:4]):
        assert torch.equal(a, b)
    assert runs[0][4] == runs[1][4] and not [n for n in runs[0][4] if 'rankloss' in n]
    assert 'cham_score_softmax_fwd' in runs[0][4] and len(runs[0][4]) > 50


def test_a_ranking_loss_launches_its_own_pair(gpu):
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    p = H.tiny_params(loss_function='bpr')
    rt = NARRuntime(p, seed=3, weights=CO.pair_weights(p, 3))
    model = RO.make_model(p, rt)
    spy = rt.lib = _LibSpy(rt.lib)
    f, l = synthetic.make_batches(1, 64, 8, 1000, p['session_features_config'], length_dist='g1')[0]
    st = H.warm_state(p, [])
    model.feed_state(st.get_articles_recent_pop_norm().copy(), st.get_recent_clicks_buffer().copy())
    model.train_step(model.upload_batch(f, l))
    torch.cuda.synchronize()
    assert 'cham_score_rankloss_fwd' in spy.log and [n for n in spy.log if n.startswith('cham_score_rankloss_bwd')]
    assert not [n for n in spy.log if 'score_softmax' in n]


def test_checkpoint_crosses_losses(gpu):
    """The loss is not part of the parameter layout: a state dict written under bpr_max loads into a runtime that trains with the softmax."""
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    p = H.tiny_params(loss_function='bpr_max')
    a = NARRuntime(p, seed=3, weights=CO.pair_weights(p, 3))
    q = H.tiny_params()
    b = NARRuntime(q, seed=4)
    assert a.layout.fingerprint() == b.layout.fingerprint()
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.flat, b.flat)


def test_graphed_step_declines_a_ranking_loss(gpu):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import GraphedTrainStep
    p = H.tiny_params(loss_function='bpr')
    model, _ = RO.make_pair(p)
    full = synthetic.make_batches(1, 64, 8, 1000, p['session_features_config'], length_dist='full')
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], 1000)
    gs = GraphedTrainStep(model, st)
    d = model.upload_batch(*full[0])
    st.update_from_device_batch(d['aci'], d['g_event_ts'])
    model.feed_state(st, st)
    model.train_step(d)                                    # an eager step on the device-resident state: the shape is warm
    assert "loss_function bpr" in gs.supports(d)
    model.loss_function = 'softmax'                        # ... which is the only thing in the way of a capture
    assert gs.supports(d) is None


_SHARD_CASE = {}


@pytest.mark.parametrize("world", [2, 3])
def test_row_shards_sum_to_the_whole_batch(gpu, world):
    """tests/test_shard_paths_gpu.py's criterion (tests/shard_paths.check_entries and what goes with it) on a bpr_max model."""
    from tests import shard_paths as SP
    from tests.test_shard_paths_gpu import _check_shards_against_whole, _evaluate, _ranges, _state_arrays
    if 'c' not in _SHARD_CASE:
        p = SP.params('default', loss_function='bpr_max')
        model, orc = RO.make_pair(p)
        bs = SP.batches(p, 4)
        st = H.warm_state(p, bs[:3])
        _SHARD_CASE['c'] = _evaluate('default', p, model, orc, *bs[3], *_state_arrays(st))
    c = _SHARD_CASE['c']
    outs, g_sum = c['shards'](_ranges('world', world))
    _check_shards_against_whole('default', c, outs, g_sum, "bpr_max world %d" % world)
