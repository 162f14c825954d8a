"""ACR module on the GPU: the conv + max-over-time kernels, the weighted softmax cross-entropy, the padding rule, one training step and a
short training run against the float64 restatement of tests/acr_oracle.py, and the trainer end to end on the synthetic corpus.

Bounds.  Conv forward: per element |got - ref| <= gamma_(kE+2) (|bias| + sum |x||w|) (a fixed-order fp32 fma chain of kE products plus
the bias add), gamma_n = n u / (1 - n u), u = 2^-24; for the pooled value the bound is the largest over the article's positions (the max of
values that each lie within their bound lies within the largest).  Conv backward: gamma_(B+1) sum_b |g||x|.  Whole steps: the GPU's
deviation from the float64 oracle may be at most 4 x the float32 oracle's own deviation (the factor covers the different summation order),
floor 8 u, per tensor in max-norm relative to the tensor's largest magnitude."""
import ctypes
import logging
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import check, ptr
from chameleon_recsys_amd.acr import acr_datasets, acr_model, acr_trainer_gcom, synthetic
from chameleon_recsys_amd.nar import nar_trainer_adressa, nar_trainer_gcom
from tests import acr_oracle as AO

pytestmark = pytest.mark.gpu
U = AO.U
V = 50
GUARD = 777.0


# ---------------------------------------------------------------------------------------------------- conv-pool cases
def _case(B, L, E, F, sizes, ldE=None, row_offset=0, seed=0):
    """Inputs of one conv-pool case: fp32-valued float64 arrays.  Tokens hold 0, V-1 and repeats; article 1 is all pad except two tokens;
    every 7th filter (f % 7 == 3) has a bias so negative that its ReLU is off everywhere (pool exactly 0, argmax 0, g = 0)."""
    rng = np.random.RandomState(seed)
    ldE = ldE or (E + 3) // 4 * 4
    table = np.full((V + row_offset, ldE), 1000.0, np.float32)          # pad columns / rows in front of the view: NaN-free sentinels
    table[row_offset:, :E] = (0.5 * rng.randn(V, E)).astype(np.float32)
    tok = rng.randint(0, V, size=(B, L)).astype(np.int32)
    tok[0, 0], tok[0, L - 1] = 0, V - 1
    if L > 2:
        tok[0, 1] = tok[0, 2] = tok[0, 0]                                # repeats
    if B > 1:
        tok[1, :] = 0
        tok[1, 0], tok[1, min(1, L - 1)] = 7, V - 1
    Ws = [(rng.randn(k, E, F) / np.sqrt(k * E)).astype(np.float32) for k in sizes]
    bs = [rng.uniform(0.2, 1.0, size=F).astype(np.float32) for _ in sizes]
    for b in bs:
        b[3::7] = -100.0
    return dict(B=B, L=L, E=E, F=F, sizes=list(sizes), ldE=ldE, row_offset=row_offset, table=table, tok=tok, W=Ws, bias=bs)


def _reference(c):
    """Per size: float64 conv [B, T', F] and the bound factor |bias| + sum |x||w|, evaluated ONCE per distinct token window, so that identical
    windows (the pad tail) have literally the same reference value."""
    x = c['table'][c['row_offset']:, :c['E']].astype(np.float64)
    out = []
    for k, W, bias in zip(c['sizes'], c['W'], c['bias']):
        T = c['L'] - k + 1
        win = np.stack([c['tok'][:, j:j + T] for j in range(k)], axis=2).reshape(-1, k)          # [B T', k] token windows
        uniq, inv = np.unique(win, axis=0, return_inverse=True)
        xw = x[uniq].reshape(len(uniq), -1)                                                     # [U, k E]
        W2 = W.astype(np.float64).reshape(-1, c['F'])
        conv = np.maximum(xw @ W2 + bias.astype(np.float64), 0.0)
        bnd = AO.gamma(k * c['E'] + 2) * (np.abs(xw) @ np.abs(W2) + np.abs(bias.astype(np.float64)))
        inv = inv.reshape(-1)
        out.append((conv[inv].reshape(c['B'], T, c['F']), bnd[inv].reshape(c['B'], T, c['F'])))
    return out


def _expectations(c):
    """pool_ref [B, PW], pool bound [B, PW], first argmax [B, PW], qualifies [B, PW] (the best two distinct values lie further apart than
    twice the bound: the argmax must then be the reference's first), conv_ref / bound per size."""
    ref = _reference(c)
    pools, bnds, args, quals = [], [], [], []
    for conv, bnd in ref:
        m = conv.max(axis=1)
        b = bnd.max(axis=1)
        lower = np.where(conv < m[:, None, :], conv, -np.inf).max(axis=1)                       # the second distinct value (or -inf)
        pools.append(m); bnds.append(b); args.append(conv.argmax(axis=1)); quals.append(m - lower > 2 * b)
    cat = lambda xs: np.concatenate(xs, axis=1)
    return cat(pools), cat(bnds), cat(args), cat(quals), ref


CONV_CASES = OrderedDict([
    ("L5_E6_F5", dict(B=3, L=5, E=6, F=5, sizes=(3, 4, 5))),            # a single output position for k = 5
    ("L6_E1_F1", dict(B=3, L=6, E=1, F=1, sizes=(3, 4, 5))),
    ("L37_E12_F130", dict(B=3, L=37, E=12, F=130, sizes=(3, 4, 5))),    # two position tiles, two filter tiles, the second partial
    ("L300_E300_F128", dict(B=3, L=300, E=300, F=128, sizes=(3, 4, 5))),
    ("L37_E6_F5_wide_ld", dict(B=3, L=37, E=6, F=5, sizes=(3, 4, 5), ldE=16)),
    ("L37_E6_F5_row_offset", dict(B=3, L=37, E=6, F=5, sizes=(3, 4, 5), row_offset=3)),
    ("L7_size1", dict(B=3, L=7, E=6, F=5, sizes=(1,))),
    ("L7_sizes2_7", dict(B=3, L=7, E=12, F=5, sizes=(2, 7))),
    ("L37_E330_F5", dict(B=3, L=37, E=330, F=5, sizes=(3, 4, 5))),      # E above the 320 columns staged per pass: the multi-pass path
    ("L33_E12_F128", dict(B=3, L=33, E=12, F=128, sizes=(2, 3))),      # 32 positions for k = 2 -> exactly one tile; 31 for k = 3
])


class _Conv:
    """Device buffers and the two kernel calls of one case; the gradient slices sit inside a guarded flat buffer."""

    def __init__(self, c, dev):
        self.c, self.lib = c, _lib.load()
        n, F, E = len(c['sizes']), c['F'], c['E']
        self.PW, self.ldP = n * F, (n * F + 3) // 4 * 4 + 4
        self.table_full = torch.from_numpy(c['table']).to(dev)
        self.table = self.table_full[c['row_offset']:]
        self.tok = torch.from_numpy(c['tok']).to(dev)
        self.W = [torch.from_numpy(w).to(dev) for w in c['W']]
        self.b = [torch.from_numpy(b).to(dev) for b in c['bias']]
        self.sizes = (ctypes.c_int * n)(*c['sizes'])
        arr = ctypes.c_void_p * n
        self.pW, self.pb = arr(*[w.data_ptr() for w in self.W]), arr(*[b.data_ptr() for b in self.b])
        self.pool = torch.full((c['B'], self.ldP), GUARD, device=dev)
        self.argmax = torch.full((c['B'], self.PW), -5, dtype=torch.int32, device=dev)
        need = self.lib.cham_acr_conv_pool_workspace_bytes(c['B'], c['L'], self.sizes, n, F)
        self.ws = torch.empty(max(1, need // 4), device=dev)
        # flat gradient buffer: [guard 8][dW_0][guard 8][db_0][guard 8] ...
        self.slices, off = [], 8
        for k in c['sizes']:
            w0 = off; off += (k * E * F + 3) // 4 * 4 + 8
            b0 = off; off += (F + 3) // 4 * 4 + 8
            self.slices.append((w0, k * E * F, b0, F))
        self.flat = torch.full((off,), GUARD, device=dev)
        self.pdW = arr(*[self.flat.data_ptr() + 4 * s[0] for s in self.slices])
        self.pdb = arr(*[self.flat.data_ptr() + 4 * s[2] for s in self.slices])

    def fwd(self, L=None):
        c = self.c
        return self.lib.cham_acr_conv_pool_fwd(ptr(self.tok), c['B'], c['L'] if L is None else L, ptr(self.table), V, c['E'], c['ldE'], self.sizes,
                                               len(c['sizes']), c['F'], self.pW, self.pb, ptr(self.pool), self.ldP, ptr(self.argmax), ptr(self.ws),
                                               self.ws.numel() * 4, None)

    def bwd(self, dpool):
        c = self.c
        check(self.lib.cham_acr_conv_pool_bwd(ptr(self.tok), c['B'], c['L'], ptr(self.table), V, c['E'], c['ldE'], self.sizes, len(c['sizes']),
                                              c['F'], ptr(dpool), ptr(self.pool), self.ldP, ptr(self.argmax), self.pdW, self.pdb, None),
              "cham_acr_conv_pool_bwd")
        torch.cuda.synchronize()
        return self.flat.cpu().numpy().copy()


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_pool_forward_against_float64(gpu, name):
    c = _case(**CONV_CASES[name])
    pool_ref, bnd, arg_ref, qual, ref = _expectations(c)
    k = _Conv(c, gpu)
    check(k.fwd(), "cham_acr_conv_pool_fwd")
    torch.cuda.synchronize()
    pool, arg = k.pool.cpu().numpy(), k.argmax.cpu().numpy()
    assert np.all(pool[:, k.PW:] == GUARD)                                       # columns beyond n_sizes F are not written
    pool = pool[:, :k.PW].astype(np.float64)
    err = np.abs(pool - pool_ref)
    print("%s: max |pool - ref| / bound = %.3g, exact-argmax share %.3f" % (name, (err / bnd).max(), qual.mean()))
    assert np.all(err <= bnd), (err / bnd).max()
    F = c['F']
    for s, (conv, b) in enumerate(ref):
        a = arg[:, s * F:(s + 1) * F]
        assert a.min() >= 0 and a.max() <= c['L'] - c['sizes'][s]
        at = np.take_along_axis(conv, a[:, None, :].astype(np.int64), axis=1)[:, 0, :]
        assert np.all(at >= pool_ref[:, s * F:(s + 1) * F] - 2 * bnd[:, s * F:(s + 1) * F])        # the position attains the maximum
        if F > 3:                                                                # filters 3, 10, .. are ReLU-off: exactly 0, first position
            assert np.all(pool[:, s * F:(s + 1) * F][:, 3::7] == 0.0) and np.all(a[:, 3::7] == 0)
    assert qual.mean() >= 0.9
    assert np.array_equal(arg[qual], arg_ref[qual])
    # two runs are bit-identical
    p1, a1 = k.pool.clone(), k.argmax.clone()
    check(k.fwd(), "cham_acr_conv_pool_fwd")
    torch.cuda.synchronize()
    assert torch.equal(p1, k.pool) and torch.equal(a1, k.argmax)


def test_conv_pool_refuses_a_batch_shorter_than_the_largest_filter(gpu):
    c = _case(B=3, L=5, E=6, F=5, sizes=(3, 4, 5))
    k = _Conv(c, gpu)
    assert k.fwd(L=4) == -22
    torch.cuda.synchronize()
    assert torch.all(k.pool == GUARD) and torch.all(k.argmax == -5)


BWD_CASES = [(n, 3) for n in CONV_CASES] + [("L6_E1_F1", 1), ("L37_E12_F130", 1), ("L6_E1_F1", 64), ("L37_E12_F130", 64), ("L7_sizes2_7", 64)]


@pytest.mark.parametrize("name,B", BWD_CASES)
def test_conv_pool_backward_against_float64(gpu, name, B):
    c = _case(**dict(CONV_CASES[name], B=B))
    k = _Conv(c, gpu)
    check(k.fwd(), "cham_acr_conv_pool_fwd")
    rng = np.random.RandomState(11)
    dpool = rng.randn(B, k.ldP).astype(np.float32)
    dpool[rng.rand(B, k.ldP) < 0.2] = 0.0                                        # some g exactly zero beside the ReLU-off filters
    d_dev = torch.from_numpy(dpool).to(gpu)
    flat = k.bwd(d_dev)
    assert np.array_equal(flat, k.bwd(d_dev))                                    # two runs are bit-identical
    pool, arg = k.pool.cpu().numpy()[:, :k.PW], k.argmax.cpu().numpy()
    g = np.where(pool > 0, dpool[:, :k.PW], 0.0).astype(np.float64)
    assert (g == 0).any() and (g != 0).any()
    x = c['table'][c['row_offset']:, :c['E']].astype(np.float64)[c['tok']]
    F, E = c['F'], c['E']
    touched = np.zeros(flat.shape, bool)
    worst = 0.0
    for s, (ksz, (w0, wn, b0, bn)) in enumerate(zip(c['sizes'], k.slices)):
        sl = slice(s * F, (s + 1) * F)
        dW, db = AO.first_index_conv_grads(x, arg[:, sl], g[:, sl], ksz)
        aW, ab = AO.first_index_conv_abs(x, arg[:, sl], g[:, sl], ksz)
        gW, gb = flat[w0:w0 + wn].reshape(ksz, E, F).astype(np.float64), flat[b0:b0 + bn].astype(np.float64)
        tW, tb = AO.gamma(B + 1) * aW, AO.gamma(B + 1) * ab
        assert np.all(np.abs(gW - dW) <= tW) and np.all(np.abs(gb - db) <= tb)
        worst = max(worst, float((np.abs(gW - dW) / np.where(tW > 0, tW, 1)).max()))
        touched[w0:w0 + wn] = True; touched[b0:b0 + bn] = True
    print("%s B=%d: max |dW - ref| / bound = %.3g" % (name, B, worst))
    assert np.all(flat[~touched] == GUARD)                                       # nothing outside the kernel's slices is written


# ---------------------------------------------------------------------------------------------------- softmax cross-entropy
@pytest.mark.parametrize("C", [2, 7, 461])
@pytest.mark.parametrize("weights", ["none", "random", "some_zero", "all_zero"])
def test_softmax_xent_against_float64(gpu, C, weights):
    lib, rng, B = _lib.load(), np.random.RandomState(C), 9
    ld = (C + 3) // 4 * 4 + 4
    logits = np.full((B, ld), 1.0e4, np.float32)                                  # padded columns: large values that must be ignored
    logits[:, :C] = (3.0 * rng.randn(B, C)).astype(np.float32)
    logits[2, C - 1] = logits[2, 0] = logits[2, :C].max() + 1.0                  # tied maxima: the first index wins
    if C > 5:
        logits[5, 3] = logits[5, 5] = logits[5, :C].max() + 0.5
    labels = rng.randint(0, C, size=B).astype(np.int32)
    labels[0], labels[1] = 0, C - 1
    cw = None
    if weights != "none":
        cw = rng.uniform(0.5, 2.0, size=C).astype(np.float32)
        if weights == "some_zero":
            cw[labels[0]] = 0.0; cw[labels[3]] = 0.0
        if weights == "all_zero":
            cw[:] = 0.0
    d = lambda a: None if a is None else torch.from_numpy(a).to(gpu)
    lg, lb, cwd = d(logits), d(labels), d(cw)
    loss = torch.full((3,), GUARD, device=gpu)
    dl = torch.full((B, ld), GUARD, device=gpu)
    pred = torch.full((B,), -1, dtype=torch.int32, device=gpu)
    row_ws = torch.zeros(B, device=gpu)
    check(lib.cham_acr_softmax_xent(ptr(lg), ld, B, C, ptr(lb), ptr(cwd), ptr(loss), ptr(dl), ptr(pred), ptr(row_ws), None), "cham_acr_softmax_xent")
    torch.cuda.synchronize()
    # float64 reference through autograd
    x = torch.tensor(logits[:, :C].astype(np.float64), requires_grad=True)
    ref = AO.weighted_ce(x, torch.tensor(labels.astype(np.int64)), None if cw is None else torch.tensor(cw.astype(np.float64)))
    ref.backward()
    dref, ref = x.grad.numpy(), ref.detach()
    # bounds: x - m (1 rounding, carried into exp as a relative error <= R u, R = the row's range), expf and logf within 2 u, a sum of C
    # positive terms (C u), the final adds: per row (C + R + 8) u of (1 + |m| + |log s| + |x_y|); the weighted mean adds B + 2 roundings
    xs = logits[:, :C].astype(np.float64)
    m = xs.max(axis=1); s = np.exp(xs - m[:, None]).sum(axis=1); R = (m - xs.min(axis=1))
    xy = xs[np.arange(B), labels]
    ce = m + np.log(s) - xy
    wb = np.ones(B) if cw is None else cw.astype(np.float64)[labels]
    nnz = (wb != 0).sum()
    tol_row = (C + R + 8) * U * (1 + np.abs(m) + np.abs(np.log(s)) + np.abs(xy))
    tol_loss = (np.abs(wb) * (tol_row + (B + 2) * U * np.abs(ce))).sum() / max(nnz, 1)
    got = loss.cpu().numpy()
    print("C=%d %s: loss %.7g ref %.7g (|diff| %.3g, bound %.3g)" % (C, weights, got[0], float(ref), abs(got[0] - float(ref)), tol_loss))
    assert got[1] == GUARD and got[2] == GUARD
    assert abs(float(got[0]) - float(ref)) <= tol_loss
    if weights == "all_zero":
        assert got[0] == 0.0
    p = np.exp(xs - m[:, None]) / s[:, None]
    scale = np.abs(wb) / max(nnz, 1)
    tol_d = scale[:, None] * ((C + R[:, None] + 8) * U * p + 2 * U)
    gd = dl.cpu().numpy()
    assert np.all(gd[:, C:] == 0.0)                                              # padded columns of dlogits are written 0
    assert np.all(np.abs(gd[:, :C].astype(np.float64) - dref) <= tol_d)
    if weights == "all_zero":
        assert not gd.any()
    want = xs.argmax(axis=1)                                                      # numpy: the first index on ties
    assert want[2] == 0 and (C <= 5 or want[5] == 3)
    assert np.array_equal(pred.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- the model
def _tiny_model(gpu, F=4, lr=1e-3, seed=42, E=8, sizes="2,3", A=6, n_vocab=30):
    rng = np.random.RandomState(100)
    table = rng.uniform(-0.5, 0.5, size=(n_vocab, E)).astype(np.float32)
    heads = OrderedDict([('category_id', {'classification_type': 'multiclass', 'cardinality': 5}),
                         ('publisher_id', {'classification_type': 'multiclass', 'cardinality': 3})])
    cw = {'publisher_id': np.array([0.5, 2.0, 1.25], np.float32)}
    params = dict(word_embeddings_matrix=table, cnn_filter_sizes=sizes, cnn_num_filters=F, acr_embeddings_size=A, dropout_keep_prob=1.0,
                  l2_reg_lambda=1e-3, learning_rate=lr, labels_class_weights=cw)
    return acr_model.ACR_Model('metadata_classification', 'CNN', heads, params, device=gpu, seed=seed), table, heads, cw


def _tiny_batch(seed, B=4, L=9, n_vocab=30):
    rng = np.random.RandomState(seed)
    text = rng.randint(1, n_vocab, size=(B, L))
    text[1, 4:] = 0                                                                # a short article: its pad tail repeats one window
    return {'text': text}, {'category_id': rng.randint(0, 5, size=B), 'publisher_id': rng.randint(0, 3, size=B)}


def _oracles(model, table, heads, cw, lr):
    w = model.logical_weights()
    mk = lambda dt: AO.ACROracle(table, len(model.layout.sizes), OrderedDict((n, h['cardinality']) for n, h in heads.items()), w,
                                 model.l2_reg_lambda, lr, class_weights=cw, dtype=dt)
    return mk(torch.float64), mk(torch.float32)


def _allowed(dev32):
    return max(4.0 * dev32, 8 * U)


def test_padding_stays_exactly_zero_under_adam_with_l2(gpu):
    model, _, _, _ = _tiny_model(gpu, F=5, A=6)                                    # PW = 10 -> 12, A = 6 -> 8, C = 5 -> 8, 3 -> 4
    L = model.layout
    assert (L.ldP, L.ldA, list(L.ldC.values())) == (12, 8, [8, 4])
    pad = L.padding_mask()
    assert pad.any()
    init = model.params.cpu().numpy().copy()
    for i in range(5):
        model.train_step(*_tiny_batch(i))
    for t in (model.params, model.grads, model.m, model.v):
        assert not t.cpu().numpy()[pad].any()
    after = model.params.cpu().numpy()
    assert (after != init).mean() > 0.3 and after[L.offset('fc2/bias'):L.offset('fc2/bias') + 6].any()      # (the logical entries did move)


def test_one_training_step_against_the_oracle(gpu):
    lr = 1e-3
    model, table, heads, cw = _tiny_model(gpu, F=4, lr=lr)
    o64, o32 = _oracles(model, table, heads, cw, lr)
    w0 = model.logical_weights()
    f, l = _tiny_batch(0)
    loss = model.train_step(f, l).cpu().numpy()
    r64, r32 = o64.train_step(f['text'], l), o32.train_step(f['text'], l)
    g, p = model.logical_grads(), model.logical_weights()
    rows = [("loss", abs(float(loss[0]) - r64['loss']) / abs(r64['loss']), abs(r32['loss'] - r64['loss']) / abs(r64['loss']))]
    for n in g:
        gg = g[n].astype(np.float64) + (model.l2_reg_lambda * w0[n].astype(np.float64) if n.endswith('/kernel') else 0.0)   # Adam adds the L2 term
        rows.append(("grad " + n, AO.max_rel_dev(gg, r64['grads'][n]), AO.max_rel_dev(r32['grads'][n], r64['grads'][n])))
    for n in p:
        rows.append(("param " + n, AO.max_rel_dev(p[n], r64['params'][n]), AO.max_rel_dev(r32['params'][n], r64['params'][n])))
    for name, dev_gpu, dev32 in rows:
        print("%-36s gpu %.3e   float32 oracle %.3e   allowed %.3e" % (name, dev_gpu, dev32, _allowed(dev32)))
    bad = [(n, a, b) for n, a, b in rows if a > _allowed(b)]
    assert not bad, bad
    assert abs(float(loss[1]) + float(loss[2]) - float(loss[0])) <= 2 * U * abs(float(loss[0]))


@pytest.fixture(scope="module")
def train_corpus(tmp_path_factory):
    return synthetic.make_corpus(str(tmp_path_factory.mktemp("acr_train")), n_articles=160, n_categories=5, vocab_size=60, embedding_size=12,
                                 articles_by_file=40, seed=0, min_len=6)


def _train_run(gpu, corpus, steps=40):
    cfg = corpus['features_config']
    params = dict(word_embeddings_matrix=corpus['word_embeddings_matrix'], cnn_filter_sizes="3,4,5", cnn_num_filters=8, acr_embeddings_size=10,
                  dropout_keep_prob=1.0, l2_reg_lambda=1e-3, learning_rate=1e-2)
    model = acr_model.ACR_Model('metadata_classification', 'CNN', cfg['label_features'], params, device=gpu)
    batches = list(acr_datasets.prepare_dataset(corpus['files'], cfg, batch_size=16, epochs=4, shuffle_dataset=True, shuffle_buffer_size=8,
                                                truncate_tokens_length=30))[:steps]
    assert len(batches) == steps
    w0 = model.logical_weights()
    losses = [float(model.train_step(f, l).cpu().numpy()[0]) for f, l in batches]
    return model, batches, w0, losses, params


def test_training_run_learns_is_reproducible_and_tracks_the_oracle(gpu, train_corpus):
    model, batches, w0, losses, params = _train_run(gpu, train_corpus)
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    correct = total = 0
    for f, l in acr_datasets.prepare_dataset(train_corpus['files'], train_corpus['features_config'], 16, 1, False, 1, 30):
        _, preds = model.eval_step(f, l)
        correct += int((preds['category_id'] == l['category_id']).sum()); total += len(l['category_id'])
    print("loss %.5f -> %.5f, training-set accuracy %.3f" % (losses[0], losses[-1], correct / total))
    assert correct / total > 1.5 / 5
    model2, _, _, losses2, _ = _train_run(gpu, train_corpus)
    assert losses2 == losses and torch.equal(model2.params, model.params)          # bit-identical from the same seed
    heads = OrderedDict([('category_id', 5)])
    mk = lambda dt: AO.ACROracle(params['word_embeddings_matrix'], 3, heads, w0, 1e-3, 1e-2, dtype=dt)
    o64, o32 = mk(torch.float64), mk(torch.float32)
    bad = []
    for i, (f, l) in enumerate(batches[:10]):
        a, b = o64.train_step(f['text'], l)['loss'], o32.train_step(f['text'], l)['loss']
        dev_gpu, dev32 = abs(losses[i] - a) / abs(a), abs(b - a) / abs(a)
        print("step %2d: loss %.7f oracle %.7f  gpu dev %.3e  float32 oracle dev %.3e  allowed %.3e" % (i + 1, losses[i], a, dev_gpu, dev32, _allowed(dev32)))
        if dev_gpu > _allowed(dev32):
            bad.append((i + 1, dev_gpu, dev32))
    assert not bad, bad


class _NoLaunch:
    def __getattr__(self, name):
        raise AssertionError("kernel entry point %s reached with an out-of-range id" % name)


def test_out_of_range_ids_raise_before_any_launch(gpu):
    model, _, _, _ = _tiny_model(gpu)
    f, l = _tiny_batch(0)
    before = model.params.clone()
    model.lib = _NoLaunch()
    bad_f = {'text': f['text'].copy()}
    bad_f['text'][2, 3] = 30                                                        # == V
    with pytest.raises(ValueError, match="token"):
        model.train_step(bad_f, l)
    bad_f['text'][2, 3] = -1
    with pytest.raises(ValueError, match="token"):
        model.predict(bad_f)
    bad_l = dict(l, category_id=l['category_id'].copy())
    bad_l['category_id'][0] = 5
    with pytest.raises(ValueError, match="label"):
        model.train_step(f, bad_l)
    with pytest.raises(ValueError, match="label"):
        model.eval_step(f, bad_l)
    assert model.global_step == 0 and torch.equal(before, model.params)


# ---------------------------------------------------------------------------------------------------- end to end
def test_trainer_end_to_end_on_the_synthetic_corpus(gpu, tmp_path, caplog):
    corpus = synthetic.make_corpus(str(tmp_path / "corpus"), n_articles=200, n_categories=5, vocab_size=60, embedding_size=12,
                                   articles_by_file=50, seed=1, min_len=6)
    assert len(corpus['files']) == 4
    pk, csv, mat = str(tmp_path / "acr.pickle"), str(tmp_path / "articles.csv"), str(tmp_path / "ace.pickle")
    with caplog.at_level(logging.INFO, logger=acr_trainer_gcom.log.name):
        out = acr_trainer_gcom.main([
            '--train_set_path_regex', corpus['train_set_path_regex'], '--model_dir', str(tmp_path / "model"),
            '--input_word_vocab_embeddings_path', corpus['word_vocab_embeddings_path'], '--input_label_encoders_path', corpus['label_encoders_path'],
            '--output_acr_metadata_embeddings_path', pk, '--output_articles_metadata_csv_path', csv,
            '--output_articles_content_embeddings_pickle_path', mat, '--cnn_num_filters', '8', '--acr_embeddings_size', '10', '--batch_size', '16',
            '--truncate_tokens_length', '30', '--training_epochs', '1', '--learning_rate', '0.01'], device=gpu)
    assert any('accuracy-category_id' in r.getMessage() for r in caplog.records)
    assert 0.0 <= out['eval_results']['accuracy-category_id'] <= 1.0 and out['eval_results']['global_step'] == 13
    sd = torch.load(str(tmp_path / "model" / "acr_model.ckpt.pt"), map_location="cpu", weights_only=True)       # the final checkpoint
    assert sd['global_step'] == 13 and torch.equal(sd['params'], out['estimator'].model.params.cpu())
    # the three loaders
    with open(pk, 'rb') as fh:
        enc, df, ace = pickle.load(fh)
    enc2, df2, ace2 = nar_trainer_adressa.load_acr_module_resources(pk)
    df3, ace3 = nar_trainer_gcom.load_acr_module_resources(csv, mat)
    assert ace.shape == (200, 10) and ace.dtype == np.float32 and np.isfinite(ace).all() and np.abs(ace).max() < 1.0
    assert np.array_equal(ace2, ace) and np.array_equal(ace3, ace) and df2.equals(df) and np.array_equal(df3.values, df.values)
    assert set(enc) == {'article_id', 'category_id', 'publisher_id'}
    assert list(df['article_id']) == list(range(200)) and 'predictions-category_id' in df.columns
    arts = corpus['articles']
    assert list(df['category_id']) == [a['category_id'] for a in arts] and list(df['text_length']) == [a['text_length'] for a in arts]
    # row i belongs to article i, embedded at the padded length of ITS predict batch (16 articles in file order)
    model = out['estimator'].model
    w = model.logical_weights()
    mk = lambda dt: AO.ACROracle(corpus['word_embeddings_matrix'], 3, OrderedDict([('category_id', 5)]), w, 1e-3, 1e-2, dtype=dt)
    o64, o32 = mk(torch.float64), mk(torch.float32)
    first = arts[:16]
    Lb = max(min(len(a['text']), 30) for a in first)
    text = np.zeros((16, Lb), np.int64)
    for i, a in enumerate(first):
        text[i, :min(len(a['text']), 30)] = a['text'][:30]
    with torch.no_grad():
        r64, r32 = o64.forward(text)[2].numpy(), o32.forward(text)[2].numpy()
    dev, dev32 = AO.max_rel_dev(ace[:16], r64), AO.max_rel_dev(r32, r64)
    print("exported rows 0-15 vs oracle at the batch's L=%d: gpu %.3e, float32 oracle %.3e" % (Lb, dev, dev32))
    assert dev <= _allowed(dev32)
    # one article alone, at its own L
    i = next(j for j, a in enumerate(first) if 5 <= len(a['text']) < Lb)
    own = np.asarray(first[i]['text'][:30])[None, :]
    alone, _ = model.predict({'text': own})
    with torch.no_grad():
        a64, a32 = o64.forward(own)[2].numpy(), o32.forward(own)[2].numpy()
    dev, dev32 = AO.max_rel_dev(alone, a64), AO.max_rel_dev(a32, a64)
    print("article %d alone at L=%d: gpu %.3e, float32 oracle %.3e" % (i, own.shape[1], dev, dev32))
    assert alone.shape == (1, 10) and dev <= _allowed(dev32)
    # a new estimator on the same model_dir restores the checkpoint before its first step
    est2 = acr_trainer_gcom.build_acr_estimator(str(tmp_path / "model"), corpus['word_embeddings_matrix'], corpus['features_config'], None,
                                                flags=acr_trainer_gcom.FLAGS, device=gpu)
    res2 = est2.evaluate(lambda: acr_datasets.prepare_dataset(corpus['files'][-1:], corpus['features_config'], 16, 1, False, 1, 30))
    assert res2['global_step'] == 13 and torch.equal(est2.model.params, model.params) and est2.model is not model
