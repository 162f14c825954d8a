"""The bounds of tests/test_scorer_tail_gpu.py and tests/test_optim_kernels_gpu.py can fail, and where they come from (no GPU here).

For every function of tests/tail_reference.py:
  * an independent restatement (torch float64 autograd for the softmax / NLL / novelty gradient and for mulpred, central differences
    for ds, a python sort for the ranking, torch for Adam) equals it to 1e-12;
  * `evaluate_*` is the same formula in a chosen precision, optionally with one slip.  Evaluated in fp32 at the GPU tests' own inputs
    it gives the fp32-CPU error per compared array; `gpu_bounds()` = 8 x the worst of them over the cases, which is the k of the GPU
    tests' max |hip - ref| <= k max |ref| (per click row for probs, ds, dS3; in units of lr_t and beyond one ulp of the weight for
    Adam's p).  8: the GPU's expf / logf / log2f and its shuffle summation order differ from numpy's by a few ulp, the recurrent
    kernels showed 2-4x between fp32 on the CPU and on the GPU, and every slip below has to stay 10x above the result;
  * each slip, evaluated in float64 (so that nothing but the slip differs), moves some compared array by at least 10 k.

fp32-CPU error per array, worst over the GPU tests' cases (k is 8 x these):
    softmax  logits 3.9e-7  probs 3.9e-6 (per click)  nll 5.2e-7  novterm 9.7e-7  ds 2.6e-6 (per click)  dS3 2.1e-6 (per click)
    mulpred  dZ2 9.7e-8  dpred_pre 5.6e-7  col_part 4.8e-7
    adam     p 7.9e-7 lr_t  m 6.6e-8  v 8.1e-8;   sumsq / loss 1.7e-7 (per component);   colsum 7.7e-6 (numpy adds the rows one after
    the other; the kernel's chunked sum is 20x better, see tests/test_optim_kernels_gpu.py)
Slips: 11 softmax / novelty, 3 ranking (exact: the output has to differ), 3 mulpred, 8 Adam, 3 column sum.
"""
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import tail_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8.0


# ---- the same formulas in a chosen precision, with optional slips ---------------------------------------------------------------------
def evaluate_softmax(inp, dt=np.float64, **slip):
    """What the forward and backward kernels owe, in precision dt: the backward from the forward's own probs / logits, as the model runs
    them.  slip: one of the keys of SOFTMAX_SLIPS."""
    c = lambda a: np.asarray(a).astype(dt)
    S3, w4, b4, tau = c(inp['S3']), c(inp['w4']), dt(inp['b4'][0]), dt(inp['tau'])
    mask = np.ones(inp['BT'], dt) if slip.get('mask_ignored') else c(inp['mask'])
    f, base = dt(inp['nov_factor']), dt(inp['pop_log_base'])
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        logits = (S3 * w4).sum(-1, dtype=dt) + b4
        z = logits * tau if slip.get('tau_multiplied') else logits / tau
        mx = z[:, 1:].max(-1, keepdims=True) if slip.get('max_over_negatives') else z.max(-1, keepdims=True)
        e = np.exp(z - mx)
        probs = e / e.sum(-1, keepdims=True, dtype=dt)
        # -log softmax_0 in its log-softmax form: the same number wherever tf.log(positive_prob) of :660 is finite, and finite where
        # fp32 lets a probability underflow (a positive 9 logits below the best candidate at tau = 0.1)
        nll = -((z[:, 0] - mx[:, 0]) - np.log(e.sum(-1, dtype=dt))) * mask
        out = dict(logits=logits, probs=probs)
        g = probs.copy()
        g[:, 1 if slip.get('minus_one_on_column_1') else 0] -= dt(1)
        if inp['nov_factor'] > 0:
            en = np.exp(z[:, 1:] - z[:, 1:].max(-1, keepdims=True))
            q = probs[:, 1:] if slip.get('q_over_all') else en / en.sum(-1, keepdims=True, dtype=dt)
            lg = np.log(c(inp['pop_norm'])[inp['neg_ids']])
            nov = -lg if slip.get('natural_log') else -lg / np.log(base)
            novterm = (q * nov).sum(-1, dtype=dt)
            nll = nll + f * novterm * mask if slip.get('novelty_sign') else nll - f * novterm * mask
            out['novterm'] = novterm
            g[:, 1:] -= f * q * (nov - novterm[:, None])
            if slip.get('novelty_gradient_to_positive'):
                q0 = np.exp(z[:, 0] - z[:, 1:].max(-1)) / en.sum(-1, dtype=dt)
                nov0 = -np.log(c(inp['pop_norm'])[inp['label_next']]) / np.log(base)
                g[:, 0] -= f * q0 * (nov0 - novterm)
        out['nll'] = nll
        if inp['sum_mask'] > 0:
            scale = dt(1) / tau if slip.get('sum_mask_dropped') else dt(1) / (tau * dt(inp['sum_mask']))
            ds = g * (mask * scale)[:, None]
            slope = np.where((S3 >= 0) if slip.get('kink_at_ge_0') else (S3 > 0), dt(1), dt(0.1 if slip.get('slope_0_1') else R.LEAKY))
            out.update(ds=ds, dS3=ds[:, :, None] * w4[None, None, :] * slope)
    return out


# name -> applies to this input set?
SOFTMAX_SLIPS = {
    'tau_multiplied': lambda i: i['tau'] != 1.0,
    'max_over_negatives': lambda i: i['tau'] == 0.1 and i['dominant'],          # fp32 only: see test_every_slip...
    'minus_one_on_column_1': lambda i: i['sum_mask'] > 0,
    'mask_ignored': lambda i: 0 < i['sum_mask'] < i['BT'],
    'sum_mask_dropped': lambda i: i['sum_mask'] > 1,
    'slope_0_1': lambda i: i['sum_mask'] > 0,
    'kink_at_ge_0': lambda i: i['sum_mask'] > 0,
    'natural_log': lambda i: i['nov_factor'] > 0 and i['sum_mask'] > 0,
    'q_over_all': lambda i: i['nov_factor'] > 0 and i['sum_mask'] > 0 and i['N'] > 1,
    'novelty_sign': lambda i: i['nov_factor'] > 0 and i['sum_mask'] > 0,
    'novelty_gradient_to_positive': lambda i: i['nov_factor'] > 0 and i['sum_mask'] > 0,
}
ROWWISE = ('probs', 'ds', 'dS3')


def softmax_reference(inp):
    ref = R.score_softmax(**R.softmax_args(inp))
    out = {k: ref[k] for k in ('logits', 'probs', 'nll')}
    if inp['nov_factor'] > 0:
        out['novterm'] = ref['novterm']
    if inp['sum_mask'] > 0:
        out.update(R.score_softmax_grad(sum_mask=inp['sum_mask'], **R.softmax_args(inp)))
    return out


def softmax_errors(got, ref):
    return {k: (R.row_err if k in ROWWISE else R.rel_err)(got[k], ref[k]) for k in ref}


def evaluate_rank(probs, label_next, neg_ids, mask, **slip):
    p = np.asarray(probs)
    NC = p.shape[1]
    idx = np.broadcast_to(np.arange(NC), p.shape)
    if slip.get('ascending'):
        order = np.argsort(p, axis=-1, kind='stable')
    elif slip.get('highest_index_first'):
        order = np.stack([np.lexsort((-idx[b], -p[b].astype(np.float64))) for b in range(len(p))])
    else:
        order = np.stack([np.array(sorted(range(NC), key=lambda c: (-float(p[b, c]), c))) for b in range(len(p))])
    ids = np.concatenate([label_next[:, None], neg_ids], 1)
    rank = np.array([int(np.where(order[b] == 0)[0][0]) for b in range(len(p))]) + (1 if slip.get('rank_off_by_one') else 0)
    return dict(pred_ids=np.take_along_axis(ids, order, 1), pred_probs=np.take_along_axis(p, order, 1),
                label_rank=np.where(mask != 0, rank, -1).astype(np.int32))


def evaluate_mulpred(inp, dt=np.float64, **slip):
    dM, Z, p = (np.asarray(inp[k]).astype(dt) for k in ('dM', 'Z2c', 'pred'))
    d = (dt(1) - Z) if slip.get('one_minus_z') else (dt(1) - Z * Z)
    dZ2 = dM * d if slip.get('pred_dropped') else dM * p[:, None, :] * d
    dMZ = dM * Z
    if slip.get('dpred_over_N'):
        dMZ = dMZ[:, :-1]
    return dict(dZ2=dZ2, dpred_pre=dMZ.sum(1, dtype=dt) * (dt(1) - p * p), col_part=dZ2.sum(1, dtype=dt))


MULPRED_SLIPS = ('one_minus_z', 'pred_dropped', 'dpred_over_N')


def evaluate_adam(inp, n_reg, sc, dt=np.float64, **slip):
    """sc: R.adam_scalars(...).  dt = float32 does every operation in fp32, as the kernel does."""
    p, g, m, v = (np.asarray(inp[k]).astype(dt) for k in ('p', 'g', 'm', 'v'))
    n = p.size
    lam, b1, b2, eps = dt(sc['lam']), dt(sc['b1']), dt(sc['b2']), dt(sc['eps'])
    if slip.get('betas_swapped'):
        b1, b2 = b2, b1
    lr_t = sc['lr_t']
    if slip.get('lr_not_lr_t'):
        lr_t = sc['lr']
    if slip.get('t_off_by_one'):
        lr_t = float(np.float32(R.adam_lr_t(sc['lr'], sc['t'] + 1)))
    lr_t = dt(lr_t)
    k = n if slip.get('l2_on_all') else 0 if slip.get('l2_on_none') else n_reg
    gr = g.copy()
    if not slip.get('decoupled_decay'):
        gr[:k] += lam * p[:k]
    m = b1 * m + (dt(1) - b1) * gr
    g2 = g if slip.get('v_without_l2') else gr
    v = b2 * v + (dt(1) - b2) * g2 * g2
    den = np.sqrt(v + eps) if slip.get('eps_inside_sqrt') else np.sqrt(v) + eps
    pn = p - lr_t * m / den
    if slip.get('decoupled_decay'):
        pn[:k] -= lr_t * lam * p[:k]
    return dict(p=pn, m=m, v=v)


ADAM_SLIPS = {
    'eps_inside_sqrt': lambda n, n_reg, lam, t: True,
    'l2_on_all': lambda n, n_reg, lam, t: lam > 0 and n_reg < n,
    'l2_on_none': lambda n, n_reg, lam, t: lam > 0 and n_reg > 0,
    'decoupled_decay': lambda n, n_reg, lam, t: lam > 0 and n_reg > 0,
    'v_without_l2': lambda n, n_reg, lam, t: lam > 0 and n_reg > 0,
    'betas_swapped': lambda n, n_reg, lam, t: True,
    'lr_not_lr_t': lambda n, n_reg, lam, t: True,
    't_off_by_one': lambda n, n_reg, lam, t: True,
}


def adam_errors(got, inp, ref, lr_t):
    return dict(p=R.adam_step_err(got['p'], inp['p'], ref['p'], lr_t), m=R.rel_err(got['m'], ref['m']), v=R.rel_err(got['v'], ref['v']))


def evaluate_colsum(inp, R_, F, weights, accumulate, dt=np.float64, **slip):
    X, w = np.asarray(inp['X'][:, :F]).astype(dt), np.asarray(inp['w']).astype(dt)
    if slip.get('last_chunk_dropped'):
        rpc = R.colsum_chunk_rows(R_)
        keep = (R_ - 1) // rpc * rpc
        X, w = X[:keep], w[:keep]
    s = (X * w[:, None]).sum(0, dtype=dt) if weights and not slip.get('weights_ignored') else X.sum(0, dtype=dt)
    return s + np.asarray(inp['prev']).astype(dt) if accumulate and not slip.get('accumulate_overwrites') else s


def colsum_reference(inp, F, weights, accumulate):
    s = R.colsum(inp['X'][:, :F], inp['w'] if weights else None)
    return s + R.f64(inp['prev']) if accumulate else s


def evaluate_loss(inp, n_reg, lam, dt=np.float64):
    p, nll = np.asarray(inp['p'][:n_reg]).astype(dt), np.asarray(inp['nll']).astype(dt)
    xe = nll.sum(dtype=dt) / dt(inp['sum_mask'])
    reg = dt(0.5) * dt(lam) * (p * p).sum(dtype=dt)
    return np.array([xe + reg, xe, reg], dt)


# ---- the bounds of the GPU tests ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def softmax_case(i):
    inp = R.softmax_inputs(*R.SOFTMAX_CASES[i])
    return inp, softmax_reference(inp)


@functools.lru_cache(maxsize=None)
def fp32_cpu_errors():
    """Worst fp32-CPU error per compared array over the GPU tests' cases."""
    worst = {}

    def note(group, errs):
        for k, e in errs.items():
            worst[group + '.' + k] = max(worst.get(group + '.' + k, 0.0), e)
    for i in range(len(R.SOFTMAX_CASES)):
        inp, ref = softmax_case(i)
        note('softmax', softmax_errors(evaluate_softmax(inp, np.float32), ref))
    for C, N, BT in R.MULPRED_CASES:
        for b16 in (False, True):
            inp = R.mulpred_inputs(C, N, BT, b16)
            ref = R.mulpred_grad(**inp)
            got = evaluate_mulpred(inp, np.float32)
            note('mulpred', {k: R.rel_err(got[k], ref[k]) for k in ref})
    for n, n_reg, lam, t in R.ADAM_CASES:
        if n > 10 ** 6:
            continue                       # (the elementwise error does not depend on n: the large case reuses the small cases' bound)
        inp, sc = R.adam_inputs(n), R.adam_scalars(R.ADAM_LR, t, lam)
        ref = R.adam_tf(inp['p'], inp['g'], inp['m'], inp['v'], n_reg, **sc)
        note('adam', adam_errors(evaluate_adam(inp, n_reg, sc, np.float32), inp, ref, sc['lr_t']))
    for R_, F, ld, weights, acc in R.colsum_cases():
        inp = R.colsum_inputs(R_, F, ld)
        note('colsum', dict(out=R.rel_err(evaluate_colsum(inp, R_, F, weights, acc, np.float32), colsum_reference(inp, F, weights, acc))))
    for n_reg, BT in R.LOSS_CASES:
        inp = R.loss_inputs(n_reg, BT)
        ref = R.loss_finalize(inp['nll'], inp['sum_mask'], (R.f64(inp['p'][:n_reg]) ** 2).sum(), float(np.float32(R.LOSS_LAMBDA)))
        note('loss', dict(loss=R.comp_err(evaluate_loss(inp, n_reg, float(np.float32(R.LOSS_LAMBDA)), np.float32), ref)))
    return worst


def gpu_bounds():
    """k per compared array: MARGIN x the worst fp32-CPU error of the same formula at the same inputs."""
    return {k: MARGIN * e for k, e in fp32_cpu_errors().items()}


# ---- the references against independent restatements ---------------------------------------------------------------------------------
def _torch_softmax(inp):
    """Autograd through leaky_relu, the last layer, log_softmax and the novelty term, all in float64."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    S3 = t(inp['S3'])
    pre = torch.where(S3 > 0, S3, S3 / R.LEAKY).requires_grad_(True)
    act = torch.nn.functional.leaky_relu(pre, R.LEAKY)
    logits = act @ t(inp['w4']) + float(inp['b4'][0])
    logits.retain_grad()
    z = logits / inp['tau']
    per = -torch.log_softmax(z, -1)[:, 0]
    if inp['nov_factor'] > 0:
        nov = -torch.log(t(inp['pop_norm'])[torch.tensor(inp['neg_ids'])]) / np.log(inp['pop_log_base'])
        per = per - inp['nov_factor'] * (torch.softmax(z[:, 1:], -1) * nov).sum(-1)
    nll = per * t(inp['mask'])
    out = dict(logits=logits.detach().numpy(), probs=torch.softmax(z, -1).detach().numpy(), nll=nll.detach().numpy())
    if inp['sum_mask'] > 0:
        (nll.sum() / inp['sum_mask']).backward()
        out.update(ds=logits.grad.numpy(), dS3=pre.grad.numpy())
    return out


@pytest.mark.parametrize("i", range(len(R.SOFTMAX_CASES)))
def test_softmax_reference_equals_autograd(i):
    inp, ref = softmax_case(i)
    got = _torch_softmax(inp)
    for k in got:
        assert (R.row_err if k in ROWWISE else R.rel_err)(got[k], ref[k]) < 1e-12, (k, R.SOFTMAX_CASES[i])
    ev = evaluate_softmax(inp)
    for k in ref:
        assert (R.row_err if k in ROWWISE else R.rel_err)(ev[k], ref[k]) < 1e-12, (k, R.SOFTMAX_CASES[i])


def test_ds_equals_central_differences():
    """d(sum(nll) / sum_mask) / d logit by central differences of score_softmax in float64, through the last layer's bias-free input:
    the logits are shifted directly by perturbing b4 per candidate (S3 gets one extra column that selects the candidate)."""
    inp = R.softmax_inputs(9, 5, 0.2, 0.3, 10.0, 'ragged', False)
    a = R.softmax_args(inp)
    ds = R.score_softmax_grad(sum_mask=inp['sum_mask'], **a)['ds']
    S3x = np.concatenate([R.f64(inp['S3']), np.zeros((5, 10, 1))], -1)
    w4x = np.concatenate([R.f64(inp['w4']), [1.0]])
    h = 1e-5
    for bt in range(5):
        for c in range(10):
            tot = []
            for s in (h, -h):
                S = S3x.copy()
                S[bt, c, -1] = s
                tot.append(R.score_softmax(**dict(a, S3=S, w4=w4x))['nll'].sum() / inp['sum_mask'])
            fd = (tot[0] - tot[1]) / (2 * h)
            assert abs(fd - ds[bt, c]) < 1e-7 * max(1.0, np.abs(ds).max()), (bt, c, fd, ds[bt, c])


def test_softmax_inputs_follow_the_input_rules():
    seen = dict(tiny_p=False, sure_p=False, big_z=False, small_z=False, dominant=False)
    for i, case in enumerate(R.SOFTMAX_CASES):
        inp, ref = softmax_case(i)
        S3, BT, N = inp['S3'], inp['BT'], inp['N']
        bits = S3.view(np.uint32)
        for pattern in (0x00000000, 0x80000000, 0x00800000, 0x80800000):        # +0.0, -0.0, the smallest normals
            assert (bits == pattern).any(), (case, hex(pattern))
        if inp['bf16']:
            assert np.array_equal(R.round_bf16(S3).reshape(S3.shape), S3)
        tied = sum(1 for bt in range(BT) if len({S3[bt, c].tobytes() for c in range(1, N + 1)}) < N)
        if N >= 2:
            assert 3 * tied >= BT, case
            assert any(S3[0, 0].tobytes() == S3[0, c].tobytes() for c in range(1, N + 1))
        assert (inp['neg_ids'] == 0).any() and (inp['pop_norm'] > 0).all()
        z = ref['logits'] / inp['tau']
        if inp['tau'] == 0.1 and inp['dominant']:
            seen['tiny_p'] |= bool(ref['probs'][1, 0] < 1e-20 and 40 < ref['nll'][1] + 20 and inp['mask'][1])
            seen['sure_p'] |= bool(ref['probs'][2, 0] > 1 - 1e-9)
            seen['dominant'] |= bool(z[2, 0] - z[2, 1:].max() > 89.0)          # expf overflows fp32 above 88.7
            seen['big_z'] |= bool(np.abs(z).max() > 55)
            seen['small_z'] |= bool((np.abs(z).max(-1) < 5).any())
    assert all(seen.values()), seen


@pytest.mark.parametrize("i", range(len(R.SOFTMAX_CASES)))
def test_rank_reference_equals_a_python_sort(i):
    inp, ref = softmax_case(i)
    probs = ref['probs'].astype(np.float32)
    want = evaluate_rank(probs, inp['label_next'], inp['neg_ids'], inp['mask'])
    got = R.rank_items(probs, inp['label_next'], inp['neg_ids'], inp['mask'])
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    # ranking is exact: a slip has to change some output outright
    for slip in ('highest_index_first', 'ascending', 'rank_off_by_one'):
        if (slip == 'rank_off_by_one' and not inp['mask'].any()) or (slip == 'ascending' and (probs.max(1) == probs.min(1)).all()):
            continue                          # (nothing to tell them apart by: all clicks masked / every candidate tied)
        bad = evaluate_rank(probs, inp['label_next'], inp['neg_ids'], inp['mask'], **{slip: True})
        assert any(not np.array_equal(bad[k], want[k]) for k in want), (slip, R.SOFTMAX_CASES[i])


def _torch_mulpred(inp):
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    a, b = torch.atanh(t(inp['Z2c'])).requires_grad_(True), torch.atanh(t(inp['pred'])).requires_grad_(True)
    (torch.tanh(a) * torch.tanh(b)[:, None, :] * t(inp['dM'])).sum().backward()
    return dict(dZ2=a.grad.numpy(), dpred_pre=b.grad.numpy(), col_part=a.grad.sum(1).numpy())


@pytest.mark.parametrize("C,N,BT", R.MULPRED_CASES)
def test_mulpred_reference_equals_autograd(C, N, BT):
    inp = R.mulpred_inputs(C, N, BT)
    ref = R.mulpred_grad(**inp)
    got, ev = _torch_mulpred(inp), evaluate_mulpred(inp)
    for k in ref:
        assert R.rel_err(got[k], ref[k]) < 1e-12 and R.rel_err(ev[k], ref[k]) < 1e-12, k
    assert R.rel_err(R.mul_rows(inp['Z2c'], inp['pred']), (torch.tensor(inp['Z2c']).double() * torch.tensor(inp['pred']).double()[:, None]).numpy()) < 1e-12


@pytest.mark.parametrize("n,n_reg,lam,t", [c for c in R.ADAM_CASES if c[0] < 10 ** 6])
def test_adam_reference_equals_a_torch_step(n, n_reg, lam, t):
    inp, sc = R.adam_inputs(n), R.adam_scalars(R.ADAM_LR, t, lam)
    ref = R.adam_tf(inp['p'], inp['g'], inp['m'], inp['v'], n_reg, **sc)
    p, g, m, v = (torch.tensor(inp[k], dtype=torch.float64) for k in ('p', 'g', 'm', 'v'))
    reg = torch.arange(n) < n_reg
    gr = g + torch.where(reg, sc['lam'] * p, torch.zeros_like(p))
    m = sc['b1'] * m + (1 - sc['b1']) * gr
    v = sc['b2'] * v + (1 - sc['b2']) * gr ** 2
    p = p - sc['lr_t'] * m / (v.sqrt() + sc['eps'])
    for k, x in (('p', p), ('m', m), ('v', v)):
        assert R.rel_err(x.numpy(), ref[k]) < 1e-12, k
    ev = evaluate_adam(inp, n_reg, sc)
    assert all(R.rel_err(ev[k], ref[k]) < 1e-12 for k in ref)
    # torch.optim.Adam differs from TF's (epsilon next to the bias-corrected root); at t = 1 from zero moments both reduce to
    # p - lr g / (|g| + eps') and agree where |g| >> eps
    assert abs(R.adam_lr_t(1e-3, 1) - 1e-3 * np.sqrt(1 - 0.999) / (1 - 0.9)) < 1e-18


def test_model_adam_lr_t_is_the_tf_step_size():
    from chameleon_recsys_amd.nar.nar_model import NARModuleModel

    class _Stub:
        lr = 3e-4
    for t in (1, 2, 10, 1000, 10 ** 6):
        want = R.adam_lr_t(3e-4, t)
        assert abs(NARModuleModel.adam_lr_t(_Stub(), t) - want) <= 1e-15 * want
        assert abs(R.adam_lr_t(3e-4, t + 1) - want) > 1e-9 * want or t == 10 ** 6        # t off by one is a different number


def test_reductions_equal_their_restatements():
    for R_, F, ld, weights, acc in R.colsum_cases()[::5]:
        inp = R.colsum_inputs(R_, F, ld)
        X = torch.tensor(inp['X'][:, :F], dtype=torch.float64)
        want = (torch.tensor(inp['w'], dtype=torch.float64) @ X if weights else X.sum(0)).numpy() + (R.f64(inp['prev']) if acc else 0.0)
        assert R.rel_err(colsum_reference(inp, F, weights, acc), want) < 1e-12
    inp = R.loss_inputs(1000, 257)
    p = torch.tensor(inp['p'][:1000], dtype=torch.float64)
    assert abs(R.l2_loss(inp['p'], 1000, 1e-4) - float(1e-4 * (p ** 2).sum() / 2)) < 1e-18
    tot = R.loss_finalize(inp['nll'], inp['sum_mask'], float((p ** 2).sum()), 1e-4)
    assert abs(tot[1] - float(torch.tensor(inp['nll']).double().sum()) / inp['sum_mask']) < 1e-12 and abs(tot[0] - tot[1] - tot[2]) < 1e-15


def test_round_bf16_matches_torch_and_the_hand_cases():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(10.0) ** rng.integers(-40, 38, 4096).astype(np.float32),
                        bf16_edge_values()])
    want = torch.tensor(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.round_bf16_bits(x), want)
    one = np.array([0x3F800000, 0x3F808000, 0x3F818000, 0x3F808001], np.uint32).view(np.float32)
    # 1.0; 1 + half an ulp with an even mantissa (down); odd mantissa + half an ulp (up, to even); just above the tie (up)
    assert R.round_bf16_bits(one).tolist() == [0x3F80, 0x3F80, 0x3F82, 0x3F81]


def bf16_edge_values():
    """fp32 values where a bf16 rounding goes wrong first: ties on odd and even mantissas, +-0, the largest fp32 that still rounds to a
    finite bf16 (0x7F7F7FFF; 0x7F7F8000 ties to even = infinity), denormals, the smallest normal."""
    u = np.array([0x00000000, 0x80000000, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F807FFF, 0x3F808001, 0x7F7F7FFF, 0xFF7F7FFF,
                  0x7F7F0000, 0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000, 0x00400000, 0x0000C000],
                 np.uint32)
    return u.view(np.float32)


# ---- the bound can fail ---------------------------------------------------------------------------------------------------------------
def test_fp32_evaluation_gives_the_bounds():
    e = fp32_cpu_errors()
    print({k: float('%.2e' % v) for k, v in e.items()})
    assert all(0 < v < 1e-4 for v in e.values()), e          # fp32 roundoff class: the bounds are 8 x these
    assert set(gpu_bounds()) == set(e)


@pytest.mark.parametrize("i", range(len(R.SOFTMAX_CASES)))
def test_every_softmax_slip_breaks_the_bound_tenfold(i):
    """In float64, so that only the slip differs - except the max taken over the negatives, which is invisible in exact arithmetic (softmax is
    shift-invariant): its damage is the fp32 overflow of exp(z_0 - max) where the positive leads by more than 88.7, so it is evaluated in fp32."""
    inp, ref = softmax_case(i)
    k = gpu_bounds()
    worst = {}
    for name, applies in SOFTMAX_SLIPS.items():
        if not applies(inp):
            continue
        got = evaluate_softmax(inp, np.float32 if name == 'max_over_negatives' else np.float64, **{name: True})
        worst[name] = max(e / k['softmax.' + a] for a, e in softmax_errors(got, ref).items())
    print(R.SOFTMAX_CASES[i], {a: float('%.3g' % b) for a, b in worst.items()})
    assert all(v >= 10 for v in worst.values()), worst


def test_every_softmax_slip_is_tried_somewhere():
    for name, applies in SOFTMAX_SLIPS.items():
        assert any(applies(softmax_case(i)[0]) for i in range(len(R.SOFTMAX_CASES))), name


@pytest.mark.parametrize("C,N,BT", R.MULPRED_CASES)
def test_every_mulpred_slip_breaks_the_bound_tenfold(C, N, BT):
    inp = R.mulpred_inputs(C, N, BT)
    ref, k = R.mulpred_grad(**inp), gpu_bounds()
    worst = {s: max(R.rel_err(v, ref[a]) / k['mulpred.' + a] for a, v in evaluate_mulpred(inp, **{s: True}).items()) for s in MULPRED_SLIPS}
    assert min(worst.values()) >= 10, worst


@pytest.mark.parametrize("n,n_reg,lam,t", [c for c in R.ADAM_CASES if c[0] < 10 ** 6])
def test_every_adam_slip_breaks_the_bound_tenfold(n, n_reg, lam, t):
    inp, sc = R.adam_inputs(n), R.adam_scalars(R.ADAM_LR, t, lam)
    ref, k = R.adam_tf(inp['p'], inp['g'], inp['m'], inp['v'], n_reg, **sc), gpu_bounds()
    worst = {}
    for name, applies in ADAM_SLIPS.items():
        if applies(n, n_reg, lam, t):
            worst[name] = max(e / k['adam.' + a] for a, e in adam_errors(evaluate_adam(inp, n_reg, sc, **{name: True}), inp, ref, sc['lr_t']).items())
    print((n, n_reg, lam, t), {a: float('%.3g' % b) for a, b in worst.items()})
    assert min(worst.values()) >= 10, worst


def test_every_adam_slip_is_tried_somewhere():
    for name, applies in ADAM_SLIPS.items():
        assert any(applies(*c) for c in R.ADAM_CASES if c[0] < 10 ** 6), name


def test_every_colsum_slip_breaks_the_bound_tenfold():
    k = gpu_bounds()['colsum.out']
    tried = set()
    for R_, F, ld, weights, acc in R.colsum_cases():
        inp = R.colsum_inputs(R_, F, ld)
        ref = colsum_reference(inp, F, weights, acc)
        slips = (['weights_ignored'] if weights else []) + (['accumulate_overwrites'] if acc else []) + (['last_chunk_dropped'] if R_ > 1 else [])
        for s in slips:
            assert R.rel_err(evaluate_colsum(inp, R_, F, weights, acc, **{s: True}), ref) >= 10 * k, (s, R_, F)
            tried.add(s)
    assert tried == {'weights_ignored', 'accumulate_overwrites', 'last_chunk_dropped'}


def test_bf16_allowance_stays_under_its_cap_in_fp32():
    """The bf16 outputs of the GPU tests (dS3 of the bf16 softmax backward, dM of cham_mulpred_bwd_b16) against round_bf16(reference): the
    fp32-CPU evaluation, rounded to bf16, needs the one-ulp allowance at no more than 1 % of the elements."""
    k = gpu_bounds()
    for C, N, BT in R.MULPRED_CASES:
        inp = R.mulpred_inputs(C, N, BT, True)
        ref = R.mulpred_grad(**inp)['dZ2']
        ok, share = R.bf16_matches(R.round_bf16_bits(evaluate_mulpred(inp, np.float32)['dZ2']), ref, k['mulpred.dZ2'] * np.abs(ref).max())
        assert ok and share <= 0.01, (C, N, BT, share)
    for i, case in enumerate(R.SOFTMAX_CASES):
        inp, ref = softmax_case(i)
        if inp['bf16'] and inp['sum_mask'] > 0:
            got = evaluate_softmax(inp, np.float32)
            ok, share = R.bf16_matches(R.round_bf16_bits(got['dS3']), *ds3_bf16_target(inp, got['ds']))
            assert ok and share <= 0.01, (case, share)


def ds3_bf16_target(inp, ds):
    """The bf16 dS3 is compared with round_bf16(ds w4 leaky'(S3)) taken from the ds the same evaluation produced (itself held to the
    fp32 bound): what is left between them are two fp32 products, so the allowance is 4 fp32 ulps of the element.  A bound relative
    to the click's largest |dS3| would put most elements within reach of a rounding boundary: at tau = 0.1 they span 20 decades."""
    ref = R.f64(ds)[:, :, None] * R.f64(inp['w4'])[None, None, :] * R.leaky_grad_from_output(inp['S3'])
    return ref, np.abs(ref) * 2.0 ** -21


# ---- housekeeping ---------------------------------------------------------------------------------------------------------------------
def _entry_points(path, start=None):
    src = open(os.path.join(ROOT, "chameleon_recsys_amd", "csrc", path)).read()
    if start is not None:
        src = src[src.index('extern "C" int %s(' % start):]
    return sorted(set(re.findall(r'extern "C" int (cham_\w+)\s*\(', src)))


def test_every_entry_point_of_the_tail_is_named_in_a_gpu_test():
    names = _entry_points("optim.hip") + _entry_points("scorer.hip", start="cham_mulpred_bwd")
    # (the plane forms of the combine forward sit among them in the file; they belong to the combine family and are tested with it)
    combine = [n for n in names if n.startswith("cham_combine_")]
    h2 = open(os.path.join(ROOT, "tests", "test_gemm_h2_gpu.py")).read()
    assert all(re.search(r"\b%s\b" % n, h2) for n in combine), combine
    names = [n for n in names if n not in combine]
    assert len(names) >= 25 and 'cham_rank_items' in names and 'cham_adam_tf_dev' in names, names
    text = "".join(open(os.path.join(ROOT, "tests", f)).read() for f in ("test_scorer_tail_gpu.py", "test_optim_kernels_gpu.py"))
    missing = [n for n in names if not re.search(r"\b%s\b" % n, text)]
    assert not missing, "entry points without a direct GPU test: %s" % missing


def test_adam_subranges_are_float4_aligned():
    """k_adam_tf reads its pointers as float4, and parallel._sharded_step calls it on flat + 4 a with a = rank * (total // world).  The
    entry point checks n % 4, not the pointer.  Decided: no pointer check (an unaligned dwordx4 access is legal on gfx950, only slow);
    the guarantee is pinned here instead.  ParamLayout pads total to a multiple of 256 and every entry to a multiple of 4, so for every
    world size up to 64 that divides total, each rank's begin and length and its share of n_reg are multiples of 4; beyond 64 a split
    that is not has n % 4 != 0, which the entry point does reject (tests/test_optim_kernels_gpu.py)."""
    from chameleon_recsys_amd.nar.layout import ParamLayout
    from tests import helpers as H
    for over in (dict(), dict(n_items=1001, ace_dim=63), dict(C=132, H=100), dict(n_items=7, ace_dim=5, C=4, H=1)):
        p = H.tiny_params(**over)
        ace = p['content_article_embeddings_matrix']
        L = ParamLayout(p['session_features_config'], p['articles_features_config'], ace.shape[0], ace.shape[1], p['CAR_embedding_size'],
                        p['rnn_units'])
        assert L.total % 256 == 0 and L.n_reg % 4 == 0 and all(e.offset % 4 == 0 and e.size % 4 == 0 for e in L.entries.values())
        for world in range(1, 1025):
            if L.total % world:
                continue                                   # DataParallel refuses to shard
            n = L.total // world
            if world <= 64:
                assert n % 4 == 0, (L.total, world)
            if n % 4 == 0:
                for rank in range(world):
                    a = rank * n
                    assert a % 4 == 0 and min(max(L.n_reg - a, 0), n) % 4 == 0      # apply_gradients' adam(a, b, ...)
