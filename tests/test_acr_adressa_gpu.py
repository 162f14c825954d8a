"""ACR module on Adressa, on the GPU: the multilabel head's kernel against float64, one training step and a short run of the two-head
model against the float64 restatement of tests/acr_multilabel_oracle.py, and acr_trainer_adressa end to end on the synthetic corpus.

Bounds of the kernel test (u = 2^-24, gamma_n = n u / (1 - n u); expf and log1pf are taken at 2 u, as tests/test_acr_gpu.py takes expf and
logf).  Per element, term = (max(x,0) - x z) + log1p(exp(-|x|)) with z a small integer:
  * e^ = expf(-|x|) carries 2 u (|x| is exact); through log1p it becomes 2 u e / (1 + e) <= 2 u log1p(e), log1pf adds 2 u of its own, and
    l = log1p(e) <= ln 2 < 1: at most 4 u for the logarithm;
  * the product x z, the subtraction and the final addition round once each, each on a quantity of at most |x| (1 + z) + 1: 3 u.
  That is 7 u (|x| (1 + z) + 1) = tol_t, an operation count times u with no fitted constant.
The mean sums n = B C computed terms in a fixed tree: gamma_n sum |term^| for any order, and sum |term^| <= sum (|term| + tol_t); the
factor 1 / n is rounded once on the host and multiplied once: 2 u.  So
  tol_loss = (sum tol_t + (gamma_n + 2 u) sum (|term| + tol_t)) / n.
dlogits = (sigmoid(x) - z) / n with sigmoid = (x >= 0 ? 1 : e^) / (1 + e^): e^ 2 u, the denominator 2 u (from e^) + 1 u, the division 1 u:
6 u sigmoid; the subtraction, the rounded 1 / n and the product one u each on |sigmoid - z|:
  tol_d = (6 u sigmoid + 3 u |sigmoid - z|) / n + 2^-126,
the last term because a result below fp32's smallest normal number (sigmoid(-80) / n is one) has no relative accuracy.
pred = x > 0 and the three counts are exact: the test keeps |x| >= 1e-3 and asserts it on its own inputs, far outside the band
0 < x < 2.4e-7 in which TF's sigmoid(x) > 0.5 in fp32 reports 0.

Whole steps: the rule of tests/test_acr_gpu.py - the GPU's deviation from the float64 oracle may be at most 4 x the float32 oracle's own
deviation, floor 8 u, per tensor in max-norm relative to the tensor's largest magnitude."""
import logging
from collections import OrderedDict

import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import check, ptr
from chameleon_recsys_amd.acr import acr_datasets, acr_model, acr_trainer_adressa, synthetic
from chameleon_recsys_amd.nar import nar_trainer_adressa
from tests import acr_multilabel_oracle as MO
from tests import acr_oracle as AO

pytestmark = pytest.mark.gpu
U = AO.U
GUARD = 777.0
EINVAL = -22
ML_CHUNK = 1024                  # ACR_ML_CHUNK of csrc/acr.hip: the columns one workgroup stages in LDS; C = 1027 needs a second chunk


# ---------------------------------------------------------------------------------------------------- the kernel
def _ml_case(B, C, K, ld, ldK):
    """Logits [B, ld] (1e4 in the padded columns, 3 randn with +-80 planted, |x| >= 1e-3) and id lists [B, ldK] whose columns beyond K
    hold the VALID id C - 1, so that reading them would change the result.  Row 0 has a duplicated id in the last column and id 0 inside
    the list (K >= 3; K = 1: the last column alone), row 1 is all padding, row 2 starts with id 0."""
    rng = np.random.RandomState(100000 * B + 10 * C + K)
    logits = np.full((B, ld), 1.0e4, np.float32)
    x = (3.0 * rng.randn(B, C)).astype(np.float32)
    x[np.abs(x) < 1e-3] = 0.5
    x[0, 0], x[0, C - 1], x[B - 1, C // 2], x[B - 1, 1] = 80.0, -80.0, -80.0, 80.0
    logits[:, :C] = x
    ids = np.full((B, ldK), C - 1, np.int32)
    ids[:, :K] = rng.randint(0, C, size=(B, K))
    if K >= 3:
        ids[0, 0] = ids[0, K - 1] = C - 1
        ids[0, 1] = 0
    elif K:
        ids[0, 0] = C - 1
    if B > 1:
        ids[1, :K] = 0
    if B > 2 and K:
        ids[2, 0] = 0
    return logits, ids


class _Guarded:
    """A device buffer with 8 guard elements on either side of the view the kernel gets (a 32-byte offset keeps 16-byte alignment;
    ``skew`` elements more break it on purpose)."""

    def __init__(self, shape, dtype, guard, dev, skew=0):
        n = int(np.prod(shape))
        self.flat = torch.full((n + 16 + skew,), guard, dtype=dtype, device=dev)
        self.view = self.flat[8 + skew:8 + skew + n].view(*shape)
        self.guard, self.lo, self.hi = guard, 8 + skew, 8 + skew + n

    def outside_untouched(self):
        f = self.flat.cpu()
        return bool((f[:self.lo] == self.guard).all() and (f[self.hi:] == self.guard).all())


def _run_ml_case(gpu, B, C, K, ld, skew=0):
    lib = _lib.load()
    ldK, ldp = K + 3, C + 5
    logits, ids = _ml_case(B, C, K, ld, ldK)
    x32 = logits[:, :C]
    assert np.abs(x32).min() >= 1e-3 and np.abs(x32).max() == 80.0          # no element is excused from the exact prediction
    lg = _Guarded((B, ld), torch.float32, GUARD, gpu, skew)
    lg.view.copy_(torch.from_numpy(logits))
    idd = torch.from_numpy(ids).to(gpu) if K else None
    loss = _Guarded((1,), torch.float32, GUARD, gpu)
    dl = _Guarded((B, ld), torch.float32, GUARD, gpu, skew)
    pred = _Guarded((B, ldp), torch.uint8, 99, gpu)
    counts = _Guarded((3,), torch.int32, -5, gpu)
    need = lib.cham_acr_sigmoid_xent_workspace_bytes(B, C)
    assert need == B * ((C + ML_CHUNK - 1) // ML_CHUNK) * 16
    ws = _Guarded((need // 4,), torch.float32, GUARD, gpu)

    def run():
        check(lib.cham_acr_sigmoid_xent(ptr(lg.view), ld, B, C, ptr(idd), K, ldK, ptr(loss.view), ptr(dl.view), ptr(pred.view), ldp,
                                        ptr(counts.view), ptr(ws.view), need, None), "cham_acr_sigmoid_xent")
        torch.cuda.synchronize()
        return [t.view.cpu().numpy().copy() for t in (loss, dl, pred, counts)]

    got_loss, got_dl, got_pred, got_counts = run()
    again = run()
    for a, b in zip((got_loss, got_dl, got_pred, got_counts), again):       # two runs are bit-identical
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    for t in (lg, loss, dl, pred, counts, ws):
        assert t.outside_untouched()
    assert np.array_equal(lg.view.cpu().numpy(), logits)                    # (the input is not written)

    # float64 reference: autograd of binary_cross_entropy_with_logits against the count-valued target
    x = x32.astype(np.float64)
    z = MO.multi_hot(ids[:, :K], C)
    if K >= 3:
        assert z[0, C - 1] >= 2.0                                           # the duplicate counts twice (more if the draw hit it again)
    assert not z[:, 0].any() and (B < 2 or not z[1].any())
    ref_loss, ref_dl = MO.autograd_loss_and_dlogits(x, z)
    term, _, _ = MO.closed_form(x, z)
    n = B * C
    tol_t = 7 * U * (np.abs(x) * (1 + z) + 1)
    tol_loss = (tol_t.sum() + (AO.gamma(n) + 2 * U) * (np.abs(term) + tol_t).sum()) / n
    e = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1.0, e) / (1.0 + e)
    tol_d = (6 * U * sig + 3 * U * np.abs(sig - z)) / n + 2.0 ** -126
    err_l = abs(float(got_loss[0]) - ref_loss)
    err_d = np.abs(got_dl[:, :C].astype(np.float64) - ref_dl)
    print("B=%d C=%d K=%d ld=%d skew=%d: loss %.7g ref %.7g (|diff| / bound %.3g), max |ddl| / bound %.3g"
          % (B, C, K, ld, skew, got_loss[0], ref_loss, err_l / tol_loss, (err_d / tol_d).max()))
    assert np.isfinite(got_loss).all() and np.isfinite(got_dl).all()
    assert err_l <= tol_loss
    assert np.all(err_d <= tol_d)
    assert np.all(got_dl[:, C:] == 0.0)                                     # the padded columns are written 0
    want_pred, want_counts = MO.counts(x32, z)
    assert np.array_equal(got_pred[:, :C], want_pred) and np.all(got_pred[:, C:] == 99)
    assert tuple(int(v) for v in got_counts) == want_counts


@pytest.mark.parametrize("K", [0, 1, 7])
@pytest.mark.parametrize("C", [3, 67, 461, ML_CHUNK + 3])
@pytest.mark.parametrize("B", [1, 5, 9])
def test_sigmoid_xent_against_float64(gpu, B, C, K):
    _run_ml_case(gpu, B, C, K, ld=(C + 3) // 4 * 4 + 4)


@pytest.mark.parametrize("C,ld,skew", [(67, 70, 0), (67, 72, 1), (ML_CHUNK + 3, ML_CHUNK + 9, 0), (ML_CHUNK, ML_CHUNK + 12, 0)])
def test_sigmoid_xent_unaligned_rows_and_a_tail_beyond_the_last_chunk(gpu, C, ld, skew):
    """ld % 4 != 0 or a pointer off the 16-byte grid: the kernel's one-column path; C = 1024, ld = 1036: the padded columns lie beyond
    the last workgroup's chunk."""
    _run_ml_case(gpu, 5, C, 7, ld=ld, skew=skew)


def test_sigmoid_xent_refuses_bad_arguments_and_launches_nothing(gpu):
    lib, B, C, K = _lib.load(), 5, 67, 7
    ld, ldK, ldp = 72, K + 3, C + 5
    logits, ids = _ml_case(B, C, K, ld, ldK)
    lg, idd = torch.from_numpy(logits).to(gpu), torch.from_numpy(ids).to(gpu)
    loss = torch.full((3,), GUARD, device=gpu)
    dl = torch.full((B, ld), GUARD, device=gpu)
    pred = torch.full((B, ldp), 99, dtype=torch.uint8, device=gpu)
    counts = torch.full((3,), -5, dtype=torch.int32, device=gpu)
    need = lib.cham_acr_sigmoid_xent_workspace_bytes(B, C)
    ws = torch.full((need // 4,), GUARD, device=gpu)
    good = dict(logits=ptr(lg), ld=ld, B=B, C=C, ids=ptr(idd), K=K, ldK=ldK, loss=ptr(loss), dl=ptr(dl), pred=ptr(pred), ldp=ldp,
                counts=ptr(counts), ws=ptr(ws), wsb=need)
    order = ['logits', 'ld', 'B', 'C', 'ids', 'K', 'ldK', 'loss', 'dl', 'pred', 'ldp', 'counts', 'ws', 'wsb']
    bad = [dict(logits=None), dict(loss=None), dict(pred=None), dict(counts=None), dict(ws=None), dict(B=0), dict(B=-1), dict(C=0),
           dict(ld=C - 1), dict(K=-1), dict(ldK=K - 1), dict(ids=None), dict(wsb=need - 4), dict(ldp=C - 1)]
    for change in bad:
        a = dict(good, **change)
        assert lib.cham_acr_sigmoid_xent(*[a[k] for k in order], None) == EINVAL, change
    torch.cuda.synchronize()
    assert torch.all(loss == GUARD) and torch.all(dl == GUARD) and torch.all(pred == 99) and torch.all(counts == -5) and torch.all(ws == GUARD)
    assert lib.cham_acr_sigmoid_xent_workspace_bytes(0, C) == 0 and lib.cham_acr_sigmoid_xent_workspace_bytes(B, 0) == 0


# ---------------------------------------------------------------------------------------------------- the model
CW = {'category0': np.array([0.5, 2.0, 1.25, 1.0, 0.75], np.float32)}


def _tiny_model(gpu, F=4, lr=1e-3, seed=42, E=8, sizes="2,3", A=6, n_vocab=30):
    rng = np.random.RandomState(100)
    table = rng.uniform(-0.5, 0.5, size=(n_vocab, E)).astype(np.float32)
    heads = OrderedDict([('category0', {'classification_type': 'multiclass', 'cardinality': 5}),
                         ('keywords', {'classification_type': 'multilabel', 'cardinality': 9})])
    params = dict(word_embeddings_matrix=table, cnn_filter_sizes=sizes, cnn_num_filters=F, acr_embeddings_size=A, dropout_keep_prob=1.0,
                  l2_reg_lambda=1e-3, learning_rate=lr, labels_class_weights=CW)
    return acr_model.ACR_ModelMultilabel('metadata_classification', 'CNN', heads, params, device=gpu, seed=seed), table


def _tiny_batch(seed, B=4, L=9, n_vocab=30, K=3):
    rng = np.random.RandomState(seed)
    text = rng.randint(1, n_vocab, size=(B, L))
    text[1, 4:] = 0
    kw = rng.randint(1, 9, size=(B, K))
    if K:
        kw[0, 1] = kw[0, 0]                                                 # a duplicate
        kw[1, :] = 0                                                        # an empty list
        kw[2, K - 1] = 0                                                    # a shorter list
    return {'text': text}, {'category0': rng.randint(0, 5, size=B), 'keywords': kw}


def _allowed(dev32):
    return max(4.0 * dev32, 8 * U)


def test_one_training_step_of_the_two_head_model_against_the_oracle(gpu):
    lr = 1e-3
    model, table = _tiny_model(gpu, lr=lr)
    assert model.multilabel == ('keywords',)
    o64, o32 = MO.make_pair(model, table, CW, lr)
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
    assert any(n == "grad output_keywords/kernel" for n, _, _ in rows) and np.abs(r64['grads']['output_keywords/kernel']).max() > 0
    bad = [(n, a, b) for n, a, b in rows if a > _allowed(b)]
    assert not bad, bad
    assert abs(float(loss[1]) + float(loss[2]) - float(loss[0])) <= 2 * U * abs(float(loss[0]))


def test_padding_stays_exactly_zero_and_eval_and_predict_report_the_multilabel_head(gpu):
    model, _ = _tiny_model(gpu)
    L = model.layout
    assert (L.ldA, list(L.ldC.values())) == (8, [8, 12])
    pad = L.padding_mask()
    assert pad.any()
    init = model.params.cpu().numpy().copy()
    for i in range(5):
        model.train_step(*_tiny_batch(i, K=0 if i == 3 else 3))             # (one batch without any keyword list: [B, 0])
    for t in (model.params, model.grads, model.m, model.v):
        assert not t.cpu().numpy()[pad].any()
    assert (model.params.cpu().numpy() != init).mean() > 0.3
    # eval_step: the multi-hot and the three counts follow from the logits the GPU holds
    f, l = _tiny_batch(9)
    loss, preds = model.eval_step(f, l)
    x = model._last['logits_keywords'][:, :9].cpu().numpy()
    want_pred, want_counts = MO.counts(x, MO.multi_hot(l['keywords'], 9))
    assert preds['keywords'].dtype == np.uint8 and preds['keywords'].shape == (4, 9) and np.array_equal(preds['keywords'], want_pred)
    assert preds['category0'].shape == (4,) and model.multilabel_counts() == {'keywords': want_counts}
    assert np.isfinite(loss).all() and loss[0] > 0
    # predict: no labels, so no true positive and no false negative
    ace, preds2 = model.predict(f)
    tp, fp, fn = model.multilabel_counts()['keywords']
    assert ace.shape == (4, 6) and np.array_equal(preds2['keywords'], want_pred) and (tp, fp, fn) == (0, int(want_pred.sum()), 0)


@pytest.fixture(scope="module")
def train_corpus(tmp_path_factory):
    return synthetic.make_corpus_adressa(str(tmp_path_factory.mktemp("acr_adressa_train")), n_articles=160, vocab_size=60, embedding_size=12,
                                         articles_by_file=40, seed=0, min_len=6)


def _train_run(gpu, corpus, steps=40):
    cfg = corpus['features_config']
    params = dict(word_embeddings_matrix=corpus['word_embeddings_matrix'], cnn_filter_sizes="3,4,5", cnn_num_filters=8, acr_embeddings_size=10,
                  dropout_keep_prob=1.0, l2_reg_lambda=1e-3, learning_rate=1e-2, labels_class_weights=corpus['labels_class_weights'])
    model = acr_model.ACR_ModelMultilabel('metadata_classification', 'CNN', cfg['label_features'], params, device=gpu)
    batches = list(acr_datasets.prepare_dataset(corpus['files'], cfg, batch_size=16, epochs=4, shuffle_dataset=True, shuffle_buffer_size=8))[:steps]
    assert len(batches) == steps
    table = corpus['word_embeddings_matrix']
    oracles = MO.make_pair(model, table, corpus['labels_class_weights'], 1e-2)
    losses = [float(model.train_step(f, l).cpu().numpy()[0]) for f, l in batches]
    return model, batches, oracles, losses


def test_training_run_learns_is_reproducible_and_tracks_the_oracle(gpu, train_corpus):
    model, batches, (o64, o32), losses = _train_run(gpu, train_corpus)
    assert any(l['keywords'].shape[1] == 0 for _, l in batches[:10])        # a batch without any keyword list is among the compared steps
    print("loss %.5f -> %.5f" % (losses[0], losses[-1]))
    assert losses[-1] < losses[0], (losses[0], losses[-1])
    model2, _, _, losses2 = _train_run(gpu, train_corpus)
    assert losses2 == losses and torch.equal(model2.params, model.params)   # bit-identical from the same seed
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


def test_out_of_range_keyword_ids_raise_before_any_launch(gpu):
    model, _ = _tiny_model(gpu)
    f, l = _tiny_batch(0)
    before = model.params.clone()
    model.lib = _NoLaunch()
    for bad in (9, -1):
        kw = l['keywords'].copy()
        kw[3, 2] = bad
        with pytest.raises(ValueError, match="label 'keywords'"):
            model.train_step(f, dict(l, keywords=kw))
        with pytest.raises(ValueError, match="label 'keywords'"):
            model.eval_step(f, dict(l, keywords=kw))
    with pytest.raises(ValueError, match="rows"):
        model.train_step(f, dict(l, keywords=np.zeros((3, 2), np.int64)))
    assert model.global_step == 0 and torch.equal(before, model.params)


# ---------------------------------------------------------------------------------------------------- end to end
def test_trainer_end_to_end_on_the_synthetic_corpus(gpu, tmp_path, caplog, monkeypatch):
    n = 120
    corpus = synthetic.make_corpus_adressa(str(tmp_path / "corpus"), n_articles=n, vocab_size=60, embedding_size=12, articles_by_file=40,
                                           seed=1, min_len=6)
    assert len(corpus['files']) == 3
    pk = str(tmp_path / "acr_adressa.pickle")
    with caplog.at_level(logging.INFO, logger=acr_trainer_adressa.log.name):
        out = acr_trainer_adressa.main([
            '--train_set_path_regex', corpus['train_set_path_regex'], '--model_dir', str(tmp_path / "model"),
            '--input_word_vocab_embeddings_path', corpus['word_vocab_embeddings_path'], '--input_label_encoders_path', corpus['label_encoders_path'],
            '--output_acr_metadata_embeddings_path', pk, '--cnn_num_filters', '8', '--acr_embeddings_size', '10', '--batch_size', '16',
            '--training_epochs', '2', '--learning_rate', '0.01'], device=gpu)
    res = out['eval_results']
    assert any('precision-keywords' in r.getMessage() for r in caplog.records)
    for k in ('accuracy-category0', 'precision-keywords', 'recall-keywords'):
        assert 0.0 <= res[k] <= 1.0, (k, res[k])
    assert res['global_step'] == 16 and np.isfinite(res['loss'])
    model = out['estimator'].model
    assert type(model) is acr_model.ACR_ModelMultilabel
    # the pickle, as nar_trainer_adressa reads it: n + 1 rows everywhere, the padding row first
    enc, df, ace = nar_trainer_adressa.load_acr_module_resources(pk)
    assert ace.shape == (n + 1, 10) and ace.dtype == np.float32 and np.isfinite(ace).all() and np.abs(ace).max() < 1.0
    assert np.array_equal(ace, out['content_article_embeddings']) and np.array_equal(ace[0], np.mean(ace[1:], axis=0))
    assert list(df['article_id']) == list(range(1, n + 1))
    assert list(df.columns) == ['article_id', 'category0', 'category1', 'author', 'keywords', 'concepts', 'entities', 'locations', 'persons',
                                'created_at_ts', 'text_length', 'input_text', 'predictions-category0', 'predictions-keywords']
    monkeypatch.setattr(nar_trainer_adressa.base.FLAGS, 'enabled_articles_input_features_groups', [nar_trainer_adressa.ALL_FEATURES])
    acfg = nar_trainer_adressa.get_articles_features_config(enc)
    meta = nar_trainer_adressa.process_articles_metadata(df, acfg)
    arts = corpus['articles']
    assert list(meta) == ['article_id', 'created_at_ts', 'category0', 'category1', 'author']
    for name, col in meta.items():
        assert len(col) == ace.shape[0] and col[0] == 0 and list(col[1:]) == [a[name] for a in arts]
    # row i belongs to article i: a fresh predict of every batch, as the trainer formed it, gives the exported rows bit for bit
    cfg = corpus['features_config']
    first = None
    for f, _ in acr_datasets.prepare_dataset(corpus['files'], cfg, batch_size=16, epochs=1, shuffle_dataset=False):
        emb, preds = model.predict(f)
        first = first or (f, emb)
        ids = f['article_id']
        assert np.array_equal(ace[ids], emb)
        for r, i in enumerate(ids):
            row = df.iloc[int(i) - 1]
            assert row['article_id'] == i and np.array_equal(row['predictions-keywords'], np.nonzero(preds['keywords'][r])[0])
            assert row['predictions-category0'] == preds['category0'][r]
            k = len(arts[int(i) - 1]['keywords'])
            assert np.array_equal(row['keywords'][:k], arts[int(i) - 1]['keywords']) and not np.asarray(row['keywords'][k:]).any()
    # ... and the first batch agrees with the float64 oracle at the trained weights
    o64, o32 = MO.make_pair(model, corpus['word_embeddings_matrix'], corpus['labels_class_weights'], 1e-2)
    with torch.no_grad():
        r64, r32 = o64.forward(first[0]['text'])[2].numpy(), o32.forward(first[0]['text'])[2].numpy()
    dev, dev32 = AO.max_rel_dev(first[1], r64), AO.max_rel_dev(r32, r64)
    print("exported rows 1-16 vs oracle: gpu %.3e, float32 oracle %.3e" % (dev, dev32))
    assert dev <= _allowed(dev32)
