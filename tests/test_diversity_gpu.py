"""Content-diversity regulariser (--diversity_reg_factor; csrc/diversity.hip) on the GPU: the forward and backward kernels through the C ABI
against float64 references computed here from the same fp32 inputs, the training step against tests/diversity_oracle.DiversityOracle, the
effect of training with the factor, and the plumbing around it.

Kernel bounds (u = 2^-24; the recursive-summation bound n u A with A <= 2 the sum of the absolute terms: |e^| <= 1, sum p = 1, plus the
same-id subtraction; 16 for the normalisation):
    |sp - ref| <= (D + NC + 16) 2^-23        |e - ref| <= (D + 2 NC + 16) 2^-23
    |ds - (ds_before + gx_ref)| <= 4 factor scale (D + NC + 16) 2^-23 + 4 2^-24 (|ds_before| + |gx_ref|),  scale = 1 / (tau sum(mask))"""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from tests import diversity_oracle as DO
from tests import helpers as H
from tests.test_step_gpu import LOGIT_TOL, _kink_flips

pytestmark = pytest.mark.gpu
N_ITEMS = 40
ZERO_ROW, TINY_ROW = 3, 4          # an all-zero ACE row; one of norm^2 below 1e-12
U23 = 2.0 ** -23


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def kernel_case(P, N, D, ld, seed, zero_ace=False):
    """fp32 inputs of one forward launch + their float64 results.  Per click: duplicate negatives, a run of zero padding at the end of the
    list, the all-zero and the near-zero row among the candidates; every third click's label equals one of its negatives; the second click
    (and every fifth after it) is masked."""
    rng = np.random.default_rng(seed)
    NC = N + 1
    ace = np.full((N_ITEMS, ld), 7.0, np.float32)          # (the columns beyond D are not the table's: a kernel that reads them is off)
    ace[:, :D] = (rng.standard_normal((N_ITEMS, D)) * rng.uniform(0.5, 6.0, (N_ITEMS, 1))).astype(np.float32)
    ace[ZERO_ROW, :D] = 0.0
    ace[TINY_ROW, :D] = (1e-8 * rng.standard_normal(D) / np.sqrt(D)).astype(np.float32)
    if zero_ace:
        ace[:, :D] = 0.0
    label = rng.integers(1, N_ITEMS, P).astype(np.int64)
    neg = rng.integers(1, N_ITEMS, (P, N)).astype(np.int64)
    for i in range(P):
        if N >= 4:
            neg[i, 1] = neg[i, 0]                          # a duplicate inside the click
            neg[i, 2], neg[i, 3] = ZERO_ROW, TINY_ROW
            neg[i, N - max(1, N // 5):] = 0                # zero padding of a short negative list
        if i % 3 == 0:
            label[i] = neg[i, 0]                           # the label among the negatives
    mask = np.ones(P, np.uint8)
    mask[1::5] = 0
    z = rng.standard_normal((P, NC)).astype(np.float32) * np.float32(3.0)
    z -= z.max(1, keepdims=True)
    p = np.exp(z, dtype=np.float32)
    p /= p.sum(1, keepdims=True, dtype=np.float32)
    nll = rng.uniform(1.0, 5.0, P).astype(np.float32)          # (above |factor e|: the sum cannot cancel below the product's last bit)
    ids = np.concatenate([label[:, None], neg], 1)
    S = DO.similarity(torch.from_numpy(ids), torch.from_numpy(ace[:, :D].astype(np.float64))).numpy()
    sp = np.einsum('pcd,pd->pc', S, p.astype(np.float64)) * mask[:, None]
    e = (p.astype(np.float64) * sp).sum(1)
    return dict(P=P, N=N, NC=NC, D=D, ld=ld, ace=ace, label=label, neg=neg, mask=mask, p=p, nll=nll, ids=ids, sp=sp, e=e)


def run_fwd(gpu, lib, c, factor):
    from chameleon_recsys_amd._lib import check
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    d = dict(ace=t(c['ace']), label=t(c['label']), neg=t(c['neg']), mask=t(c['mask']), p=t(c['p']), nll=t(c['nll']),
             sp=torch.full((c['P'], c['NC']), float('nan'), device=gpu), e=torch.full((c['P'],), float('nan'), device=gpu))
    check(lib.cham_diversity_fwd(d['p'].data_ptr(), d['label'].data_ptr(), d['neg'].data_ptr(), d['mask'].data_ptr(), c['P'], c['N'],
                                 d['ace'].data_ptr(), c['ld'], c['D'], N_ITEMS, factor, d['sp'].data_ptr(), d['e'].data_ptr(),
                                 d['nll'].data_ptr(), _st()), "cham_diversity_fwd")
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("D", [1, 3, 64, 250, 257, 300])
def test_forward_kernel_against_float64(gpu, D):
    """P in {1, 5, 9}, N in {1, 10, 63, 64, 100} (NC = 64 and 65 straddle a wave), D of the parametrisation (300: a lane's second 16-byte
    piece) at three row strides >= D: D itself, D + 1 (no 16-byte pieces: one column per lane) and a multiple of 4 beyond D (16-byte pieces
    + the columns behind the last whole one)."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    factor = 0.37
    worst = [0.0, 0.0]
    for ld in sorted({D, D + 1, 4 * ((D + 3) // 4) + 4}):
        for P in (1, 5, 9):
            for N in (1, 10, 63, 64, 100):
                c = kernel_case(P, N, D, ld, seed=1000 * D + 10 * N + P)
                d = run_fwd(gpu, lib, c, factor)
                sp, e, nll = d['sp'].cpu().numpy(), d['e'].cpu().numpy(), d['nll'].cpu().numpy()
                masked = c['mask'] == 0
                tag = (P, N, D, ld)
                err_sp, err_e = float(np.abs(sp - c['sp']).max()), float(np.abs(e - c['e']).max())
                worst = [max(worst[0], err_sp / ((D + c['NC'] + 16) * U23)), max(worst[1], err_e / ((D + 2 * c['NC'] + 16) * U23))]
                assert err_sp <= (D + c['NC'] + 16) * U23, (tag, err_sp)
                assert err_e <= (D + 2 * c['NC'] + 16) * U23, (tag, err_e)
                assert not sp[masked].any() and not e[masked].any(), tag
                assert np.array_equal(_bits(nll[masked]), _bits(c['nll'][masked])), tag
                want = c['nll'].astype(np.float64) + np.float64(np.float32(factor)) * e.astype(np.float64)
                assert (np.abs(nll - want) <= np.spacing(np.abs(nll)))[~masked].all(), tag
                if N >= 4:                                 # the case has what it says it has
                    assert float(np.abs(c['sp'][~masked]).max()) > 1e-3
    print("D %d: worst |sp - ref| %.3f, |e - ref| %.3f of the bound" % (D, worst[0], worst[1]))


def test_forward_kernel_beyond_64_kib_of_lds(gpu):
    """D = 3 300, then 7 000, then 3 300 again: 66 and 140 KB of dynamic LDS (the limit is raised once per device, to the cap - a later,
    larger launch must not find the first one's size), same bounds."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    for D in (3300, 7000, 3300):
        c = kernel_case(5, 10, D, D, seed=D)
        d = run_fwd(gpu, lib, c, 0.37)
        sp, e = d['sp'].cpu().numpy(), d['e'].cpu().numpy()
        assert float(np.abs(sp - c['sp']).max()) <= (D + c['NC'] + 16) * U23, D
        assert float(np.abs(e - c['e']).max()) <= (D + 2 * c['NC'] + 16) * U23, D
        assert float(np.abs(c['sp']).max()) > 1e-3
    q = d['p'].data_ptr()
    assert lib.cham_diversity_fwd(q, q, q, q, 1, 10, q, 9000, 9000, 10, 0.5, q, q, q, _st()) == -22      # beyond a CU's LDS


def test_forward_kernel_rejects_bad_arguments(gpu):
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    x = torch.zeros(64, device=gpu)
    q = x.data_ptr()
    assert lib.cham_diversity_fwd(q, q, q, q, 1, 3, None, 4, 4, 10, 0.5, q, q, q, _st()) == -22       # no table
    assert lib.cham_diversity_fwd(q, q, q, q, 1, 3, q, 3, 4, 10, 0.5, q, q, q, _st()) == -22          # row stride below D
    assert lib.cham_diversity_fwd(q, q, q, q, 1, 0, q, 4, 4, 10, 0.5, q, q, q, _st()) == -22          # no negatives
    assert lib.cham_diversity_fwd(q, q, q, q, 1, 3, q, 4, 4, 10, -0.5, q, q, q, _st()) == -22         # negative factor
    assert lib.cham_diversity_bwd(q, 16, q, q, q, 1, 3, 0.1, None, 2.0, q, q, 0.5, q, q, _st()) == -22     # K3 != 32
    assert lib.cham_diversity_bwd(q, 32, q, q, q, 1, 3, 0.1, None, 0.0, q, q, 0.5, q, q, _st()) == -22     # neither a record nor sum(mask)
    torch.cuda.synchronize()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_backward_kernel_against_float64(gpu, bf16):
    """Behind the arm's softmax backward, on the forward kernel's own sp / e: ds, dS3 (the kernel expression on the downloaded ds), the record
    against sum(mask) by value, and an all-zero table (gx = 0: nothing the softmax backward wrote may change)."""
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check
    lib = _lib.load()
    factor, tau = 0.8, 0.1
    for (P, N, D), zero_ace in (((9, 10, 64), False), ((5, 64, 250), False), ((1, 1, 3), False), ((9, 100, 257), False), ((9, 10, 64), True)):
        c = kernel_case(P, N, D, D, seed=77 + P + N + D, zero_ace=zero_ace)
        NC, rows = c['NC'], P * c['NC']
        rng = np.random.default_rng(5 + N)
        sum_mask = float(c['mask'].sum()) + 3.0          # (the global batch's: other ranks' clicks count too)
        S3 = torch.from_numpy(rng.standard_normal((rows, 32)).astype(np.float32)).to(gpu)
        S3 = S3.bfloat16() if bf16 else S3
        w4 = torch.from_numpy(rng.standard_normal(32).astype(np.float32)).to(gpu)
        d = run_fwd(gpu, lib, c, factor)
        rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
        check(lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, 0, sum_mask, 0.0, 2, _st()), "cham_step_scalars_set")
        got = {}
        for how in ("value", "record"):
            ds = torch.full((rows,), float('nan'), device=gpu)
            dS3 = torch.full((rows, 32), float('nan'), device=gpu, dtype=S3.dtype)
            check((lib.cham_score_softmax_bwd_b16 if bf16 else lib.cham_score_softmax_bwd)(
                S3.data_ptr(), 32, w4.data_ptr(), d['p'].data_ptr(), d['mask'].data_ptr(), P, N, tau, sum_mask, ds.data_ptr(), dS3.data_ptr(),
                0.0, None, None, None, None, _st()), "cham_score_softmax_bwd")
            torch.cuda.synchronize()
            before = (ds.cpu().numpy().copy(), dS3.view(torch.int16 if bf16 else torch.int32).cpu().numpy().copy())
            check((lib.cham_diversity_bwd_b16 if bf16 else lib.cham_diversity_bwd)(
                S3.data_ptr(), 32, w4.data_ptr(), d['p'].data_ptr(), d['mask'].data_ptr(), P, N, tau, rec.data_ptr() if how == "record" else None,
                0.0 if how == "record" else sum_mask, d['sp'].data_ptr(), d['e'].data_ptr(), factor, ds.data_ptr(), dS3.data_ptr(), _st()),
                "cham_diversity_bwd")
            torch.cuda.synchronize()
            got[how] = (ds.cpu().numpy(), dS3.view(torch.int16 if bf16 else torch.int32).cpu().numpy(), dS3.float().cpu().numpy())
        assert np.array_equal(_bits(got["value"][0]), _bits(got["record"][0])) and np.array_equal(got["value"][1], got["record"][1])
        ds, dS3_bits, dS3 = got["value"]
        ds_before = before[0]
        if zero_ace:
            assert np.array_equal(_bits(ds), _bits(ds_before)) and np.array_equal(dS3_bits, before[1])
            continue
        scale = 1.0 / (tau * sum_mask)
        p64 = c['p'].astype(np.float64)
        gx = factor * scale * 2.0 * p64 * (c['sp'] - c['e'][:, None]) * c['mask'][:, None]
        bound = 4 * factor * scale * (D + NC + 16) * U23 + 4 * 2.0 ** -24 * (np.abs(ds_before.astype(np.float64)) + np.abs(gx).reshape(-1))
        err = np.abs(ds.astype(np.float64) - (ds_before.astype(np.float64) + gx.reshape(-1)))
        assert (err <= bound).all(), ((P, N, D), float((err / bound).max()))
        if N >= 4:                                   # the term moves ds by something a slip would show in
            assert float(np.abs(gx).max()) > 1e-3 * float(np.abs(ds_before).max())
        # dS3 = ds w4[k] leaky'(S3[row, k]) on the downloaded ds, in the kernel's order of fp32 products
        s3 = S3.float().cpu().numpy()
        expr = (ds[:, None] * w4.cpu().numpy()[None, :]) * np.where(s3 > 0, np.float32(1.0), np.float32(0.2))
        assert expr.dtype == np.float32
        if bf16:
            assert (np.abs(dS3 - expr) <= 2.0 ** -7 * np.abs(expr)).all()               # one bf16 ulp
        else:
            assert np.array_equal(_bits(dS3), _bits(expr))


# ---- the training step against DiversityOracle ------------------------------------------------------------------------------------------
FACTOR = 0.5          # with the clustered table below the oracle's term is 0.11 - 0.18 on the three batches compared (xe 2.4 - 2.8)


def _params(**over):
    return H.tiny_params(diversity_reg_factor=FACTOR, content_article_embeddings_matrix=DO.clustered_ace(1000, 64), **over)


def _term(ref):
    return float(ref['total_loss'].detach()) - float(ref['xe_loss'].detach()) - float(ref['reg_loss'].detach())


def _step_parity(p, novelty=False):
    """tests/test_step_gpu._mode_parity with the DiversityOracle pair: negatives equal, loss within LOGIT_TOL, div_e within it too, every
    parameter gradient within 3e-4 max|ref| + 2e-5 on batches without a leaky-ReLU kink flip (at least one of the three)."""
    batches = synthetic.make_batches(6, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:3])
    model, orc = DO.make_pair(p)
    clean = 0
    for f, l in batches[3:6]:
        buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
        model.feed_state(pop, buf)
        model.forward(model.upload_batch(f, l))
        out = model.outputs_numpy()
        for v in orc.w.values():
            v.grad = None
        orc.debug_taps = {}
        ref = orc.forward(f, l, buf, pop, 'train')
        mask = ref['mask'].numpy()
        assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
        div = float(ref['diversity_loss'].detach())
        assert div > 0.05 and (novelty or abs(_term(ref) - div) < 1e-5)              # the term is not negligible in this set-up
        assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < LOGIT_TOL
        assert np.abs(out['div_e'] - ref['div_e'].detach().numpy())[mask].max() < LOGIT_TOL and not out['div_e'][~mask].any()
        flips = _kink_flips(model, orc, mask)
        (ref['total_loss'] - ref['reg_loss']).backward()
        model.backward()
        torch.cuda.synchronize()
        g = model.rt.logical_grads()
        tol = 3e-4 if flips == 0 else 0.25
        clean += flips == 0
        for k, v in orc.w.items():
            rg = v.grad.numpy() if v.grad is not None else np.zeros_like(v.detach().numpy())
            scale = max(1e-6, float(np.abs(rg).max()))
            assert float(np.abs(g[k] - rg).max()) < tol * scale + 2e-5, (k, flips)
        H.update_state(st, f, l)
    assert clean >= 1


@pytest.mark.parametrize("variant", ["plain", "novelty", "dropout", "compact_0", "dev_scalars_0"])
def test_step_parity_diversity_regularised_loss(gpu, monkeypatch, variant):
    """Loss and gradients with the diversity term: alone, together with the novelty term, under dropout, on the padded + masked rows
    (CHAM_COMPACT=0) and with sum(mask) by value (CHAM_DEV_SCALARS=0)."""
    if variant == "compact_0":
        monkeypatch.setenv("CHAM_COMPACT", "0")
    if variant == "dev_scalars_0":
        monkeypatch.setenv("CHAM_DEV_SCALARS", "0")
    over = dict(novelty=dict(novelty_reg_factor=0.3), dropout=dict(dropout_keep_prob=0.8)).get(variant, {})
    _step_parity(_params(**over), novelty=variant == "novelty")


def test_step_parity_diversity_bf16_compute_mode(gpu):
    """gemm_dtype 'bf16' by the criterion of test_step_parity_bf16_compute_mode: loss within 1e-3 of the oracle emulating the rounding and
    within 3e-2 of the fp32 oracle; every gradient as close to the fp32 oracle's as the emulated bf16 gradient is (x 3 + 2 % of the max)."""
    p = _params(gemm_dtype='bf16')
    batches = synthetic.make_batches(5, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:3])
    model, orc = DO.make_pair(p)
    assert model.rt.gemm_dtype == 'bf16' and orc.gemm_dtype == 'bf16'
    orc32 = DO.DiversityOracle(dict(p, gemm_dtype='f32'), weights=orc.weights_numpy())
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
            assert float(ref['diversity_loss'].detach()) > 0.05
            if name == "bf16":
                assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
                assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < 1e-3
            else:
                assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < 3e-2
            (ref['total_loss'] - ref['reg_loss']).backward()
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


def test_eval_forward_carries_the_term(gpu):
    """An EVAL model on the trained runtime: its loss record holds xe + factor * mean(e) + reg as the oracle's eval forward does."""
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel
    p = _params()
    batches = synthetic.make_batches(4, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:3])
    model, orc = DO.make_pair(p)
    ev = NARModuleModel(ModeKeys.EVAL, None, None, p['session_features_config'], p['articles_features_config'], p['batch_size'], p['lr'], 1.0,
                        p['eval_total_negative_samples'], p['eval_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                        softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                        recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                        recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                        CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], diversity_reg_factor=FACTOR, runtime=model.rt)
    f, l = batches[3]
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    ev.feed_state(pop, buf)
    key = NARModuleModel.eval_step_key(model.rt.global_step, 0)
    ev.forward(ev.upload_batch(f, l), step=key)
    out = ev.outputs_numpy()
    with torch.no_grad():
        ref = orc.forward(f, l, buf, pop, mode='eval', step=key)
    mask = ref['mask'].numpy()
    assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
    assert float(ref['diversity_loss']) > 0.05
    assert abs(out['loss'][0] - float(ref['total_loss'])) < LOGIT_TOL
    assert abs(out['loss'][1] - float(ref['xe_loss']) - float(ref['diversity_loss'])) < LOGIT_TOL         # the xe slot carries the term
    assert np.abs(out['div_e'] - ref['div_e'].numpy())[mask].max() < LOGIT_TOL


def test_training_with_the_factor_is_bit_reproducible(gpu):
    """tests/test_step_gpu.test_training_is_bit_reproducible with the factor set: two runs of four optimizer steps end with bit-identical
    losses, weights and Adam slots (the kernels' sums have a fixed order, no atomics)."""
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    p = _params()
    batches = synthetic.make_batches(5, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    runs = []
    for _ in range(2):
        model, _o = DO.make_pair(p)
        st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'],
                                     p['recent_clicks_for_normalization'], 1000)
        dev = [model.upload_batch(f, l) for f, l in batches]
        losses = []
        for i, d in enumerate(dev):
            model.feed_state(st, st)
            losses.append(model.train_step(d).clone())
            st.update_from_device_batch(d['aci'], d['g_event_ts'])
            if i + 1 < len(dev):
                model.presample(dev[i + 1])
        torch.cuda.synchronize()
        runs.append((torch.stack(losses).cpu(), model.rt.flat.cpu().clone(), model.rt.m.cpu().clone(), model.rt.v.cpu().clone(),
                     model._plan.div_e[:model._plan.P].cpu().clone()))          # (the rows of the last step's valid positions)
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)


# ---- does what it says ------------------------------------------------------------------------------------------------------------------
def _heldout_div_e(factor):
    t = DO.TRAINED
    p, st, train, held = DO.trained_setup(factor)
    model, _ = DO.make_pair(p)
    for f, l in train:
        model.feed_state(st.get_articles_recent_pop_norm().copy(), st.get_recent_clicks_buffer().copy())
        model.train_step(model.upload_batch(f, l))
        H.update_state(st, f, l)
    model.diversity_reg_factor = t['factor']              # (the term is measured whatever the run trained with)
    model.feed_state(st.get_articles_recent_pop_norm().copy(), st.get_recent_clicks_buffer().copy())
    d = model.upload_batch(*held)
    model.forward(d)
    seq = np.asarray(held[0]['session_size']).reshape(-1) - 1
    mask = np.arange(d['T'])[None, :] < seq[:, None]
    return DO.masked_mean(model.outputs_numpy()['div_e'], mask)


def test_training_with_the_factor_lowers_the_term(gpu):
    """The same twenty tiny steps with factor 0 and with the factor: the held-out mean of p^T S p ends lower with it, by at least half the
    relative decrease DiversityOracle shows on the CPU (0.18549 -> 0.14807, 20 %: tests/diversity_oracle.TRAINED)."""
    t = DO.TRAINED
    e_plain, e_reg = _heldout_div_e(0.0), _heldout_div_e(t['factor'])
    print("held-out mean div_e: factor 0 -> %.5f, factor %g -> %.5f" % (e_plain, t['factor'], e_reg))
    oracle_drop = (t['e_plain'] - t['e_reg']) / t['e_plain']
    assert oracle_drop >= 0.10
    assert e_reg < e_plain and (e_plain - e_reg) / e_plain >= 0.5 * oracle_drop


# ---- plumbing ---------------------------------------------------------------------------------------------------------------------------
def test_negative_factor_raises(gpu):
    p = H.tiny_params(diversity_reg_factor=-0.1)
    with pytest.raises(ValueError, match="diversity_reg_factor"):
        DO.make_pair(p)


def test_factor_zero_is_the_model_without_the_argument(gpu):
    """No div_e, no buffers, and four training steps bit-identical in weights and Adam slots to a model constructed without the argument."""
    p = H.tiny_params()
    batches = synthetic.make_batches(4, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    runs = []
    for make in (H.make_pair, DO.make_pair):              # helpers.make_pair does not pass the argument
        model, _ = make(p)
        assert model.diversity_reg_factor == 0.0
        st = H.warm_state(p, [])
        for f, l in batches:
            model.feed_state(st.get_articles_recent_pop_norm().copy(), st.get_recent_clicks_buffer().copy())
            model.train_step(model.upload_batch(f, l))
            H.update_state(st, f, l)
        assert 'div_e' not in model.outputs_numpy() and model._plan.div_sp is None and model._plan.div_e is None
        runs.append((model.rt.flat.cpu().clone(), model.rt.m.cpu().clone(), model.rt.v.cpu().clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_graphed_step_declines_the_diversity_term(gpu):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import GraphedTrainStep
    p = _params()
    model, _ = DO.make_pair(p)
    full = synthetic.make_batches(1, 64, 8, 1000, p['session_features_config'], length_dist='full')
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], 1000)
    gs = GraphedTrainStep(model, st)
    d = model.upload_batch(*full[0])
    st.update_from_device_batch(d['aci'], d['g_event_ts'])
    model.feed_state(st, st)
    model.train_step(d)                                    # an eager step with the term on the device-resident state
    assert 'div_e' in model.outputs_numpy()
    assert "diversity" in gs.supports(d)
    model.diversity_reg_factor = 0.0                       # ... which is the only thing in the way of a capture
    assert gs.supports(d) is None


def test_forward_kernel_rows_beyond_4_gib(gpu):
    """The 5 M-article table (5 000 000 x 256 fp32 = 5.1 GB, left uninitialised but for the rows used): candidates whose rows start beyond
    byte 2^32 - a 32-bit row offset would read another row."""
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check
    lib = _lib.load()
    n, D, ld, P, N = 5_000_000, 250, 256, 3, 10
    rng = np.random.default_rng(9)
    used = np.unique(np.concatenate([[0, 1, 2], rng.integers(4_300_000, n, 12), [n - 1]])).astype(np.int64)
    assert int(used[-1]) * ld * 4 > 2 ** 32
    rows = (rng.standard_normal((len(used), D)) * 3.0).astype(np.float32)
    ace = torch.empty(n, ld, dtype=torch.float32, device=gpu)
    ace[torch.from_numpy(used).to(gpu), :D] = torch.from_numpy(rows).to(gpu)
    ids = used[rng.integers(3, len(used), (P, N + 1))]
    ids[:, -1] = 0
    ids[0, 1] = n - 1
    z = rng.standard_normal((P, N + 1)).astype(np.float32)
    p = np.exp(z - z.max(1, keepdims=True), dtype=np.float32)
    p /= p.sum(1, keepdims=True, dtype=np.float32)
    small = np.zeros((int(used.size), D), np.float64)
    small[:] = rows
    local = np.searchsorted(used, ids)
    S = DO.similarity(torch.from_numpy(local), torch.from_numpy(small)).numpy()
    sp_ref = np.einsum('pcd,pd->pc', S, p.astype(np.float64))
    e_ref = (p * sp_ref).sum(1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    d = dict(label=t(ids[:, 0]), neg=t(ids[:, 1:]), mask=t(np.ones(P, np.uint8)), p=t(p), nll=t(np.ones(P, np.float32)),
             sp=torch.full((P, N + 1), float('nan'), device=gpu), e=torch.full((P,), float('nan'), device=gpu))
    check(lib.cham_diversity_fwd(d['p'].data_ptr(), d['label'].data_ptr(), d['neg'].data_ptr(), d['mask'].data_ptr(), P, N, ace.data_ptr(), ld,
                                 D, n, 0.5, d['sp'].data_ptr(), d['e'].data_ptr(), d['nll'].data_ptr(), _st()), "cham_diversity_fwd")
    torch.cuda.synchronize()
    assert float(np.abs(d['sp'].cpu().numpy() - sp_ref).max()) <= (D + N + 1 + 16) * U23
    assert float(np.abs(d['e'].cpu().numpy() - e_ref).max()) <= (D + 2 * (N + 1) + 16) * U23
    assert float(np.abs(sp_ref).max()) > 1e-3
