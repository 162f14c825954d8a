"""ACR module, host side (no GPU): flags and refusals, the flat layout and its padding, the article reader, the gradient rule of the
max (first index vs. TF's even split), the weighted cross-entropy reduction and the export formats."""
import math
import pickle
from collections import OrderedDict

import numpy as np
import pytest
import torch

from chameleon_recsys_amd.acr import acr_datasets, acr_model, acr_trainer_gcom, synthetic
from chameleon_recsys_amd.nar import nar_trainer_adressa, nar_trainer_gcom
from tests import acr_oracle as AO
from tests import test_acr_gpu as G         # (its case builders only: the GPU tests' inputs are qualified here, without a GPU)

# acr_module/acr/acr_trainer_gcom.py:25-61: every flag of the reference with its default
REFERENCE_FLAGS = OrderedDict([
    ('train_set_path_regex', '/train*.tfrecord'), ('model_dir', './tmp'), ('input_word_vocab_embeddings_path', ''),
    ('input_label_encoders_path', ''), ('output_acr_metadata_embeddings_path', ''), ('text_feature_extractor', 'CNN'),
    ('training_task', 'metadata_classification'), ('autoencoder_noise', 0.0), ('cnn_filter_sizes', '3,4,5'), ('cnn_num_filters', 128),
    ('rnn_units', 250), ('rnn_layers', 1), ('rnn_direction', 'unidirectional'), ('acr_embeddings_size', 250), ('batch_size', 64),
    ('truncate_tokens_length', 300), ('training_epochs', 10), ('learning_rate', 1e-3), ('dropout_keep_prob', 1.0), ('l2_reg_lambda', 1e-3),
])
EXTRA_FLAGS = {'output_articles_metadata_csv_path': '', 'output_articles_content_embeddings_pickle_path': ''}

HEADS = {'category_id': {'classification_type': 'multiclass', 'cardinality': 5}}


# ---------------------------------------------------------------------------------------------------- flags and layout
def test_flags_are_the_references_with_its_defaults():
    got = vars(acr_trainer_gcom.build_parser().parse_args([]))
    for name, default in REFERENCE_FLAGS.items():
        assert name in got, name
        assert got[name] == default and type(got[name]) is type(default), (name, got[name], default)
    assert {k: got[k] for k in got if k not in REFERENCE_FLAGS} == EXTRA_FLAGS
    with pytest.raises(SystemExit) as e:
        acr_trainer_gcom.build_parser().parse_args(['--help'])
    assert e.value.code == 0


@pytest.mark.parametrize("kw,exc,word", [
    (dict(text_feature_extractor='LSTM'), NotImplementedError, 'text_feature_extractor'),
    (dict(text_feature_extractor='gru'), NotImplementedError, 'text_feature_extractor'),
    (dict(text_feature_extractor='MLP'), ValueError, 'text_feature_extractor'),
    (dict(training_task='autoencoder'), NotImplementedError, 'training_task'),
    (dict(training_task='other'), ValueError, 'training_task'),
    (dict(dropout_keep_prob=0.9), NotImplementedError, 'dropout_keep_prob'),
    (dict(heads={'keywords': {'classification_type': 'multilabel', 'cardinality': 9}}), NotImplementedError, 'multilabel'),
])
def test_out_of_scope_arms_are_refused_by_name(kw, exc, word):
    args = dict(training_task='metadata_classification', text_feature_extractor='CNN', heads=HEADS, dropout_keep_prob=1.0)
    args.update(kw)
    params = {'dropout_keep_prob': args['dropout_keep_prob']}
    with pytest.raises(exc, match=word):
        acr_model.check_supported(args['training_task'], args['text_feature_extractor'], args['heads'], params)
    with pytest.raises(exc, match=word):       # the model's constructor refuses before it touches the GPU library
        acr_model.ACR_Model(args['training_task'], args['text_feature_extractor'], args['heads'], params)
    acr_model.check_supported('metadata_classification', 'cnn', HEADS, {'dropout_keep_prob': 1.0})


@pytest.mark.parametrize("argv,exc,word", [
    (['--text_feature_extractor', 'GRU'], NotImplementedError, 'text_feature_extractor'),
    (['--training_task', 'autoencoder'], NotImplementedError, 'training_task'),
    (['--dropout_keep_prob', '0.5'], NotImplementedError, 'dropout_keep_prob'),
])
def test_trainer_refuses_unbuilt_flags_before_reading_anything(argv, exc, word):
    with pytest.raises(exc, match=word):           # (the asset paths are empty: reaching them would be a FileNotFoundError)
        acr_trainer_gcom.main(argv)


def test_layout_kernels_first_and_padded_widths():
    L = acr_model.ACRLayout(E=6, filter_sizes=[3, 4, 5], F=5, acr_embeddings_size=250, heads=OrderedDict([('category_id', 461), ('p', 3)]))
    assert (L.PW, L.ldP, L.ldA) == (15, 16, 252) and dict(L.ldC) == {'category_id': 464, 'p': 4}
    names = list(L.entries)
    kernels = [n for n in names if n.endswith('/kernel')]
    assert names[:len(kernels)] == kernels and all(n.endswith('/bias') for n in names[len(kernels):])
    assert L.n_reg == L.offset('conv_0/bias') and L.n_reg % 4 == 0 and L.n_params % 4 == 0
    assert L.n_reg == sum((int(np.prod(L.entries[n][2])) + 3) // 4 * 4 for n in kernels)
    assert all(off % 4 == 0 for off, _, _ in L.entries.values())
    assert L.entries['fc2/kernel'][1:] == ((15, 250), (16, 252)) and L.entries['output_category_id/kernel'][1:] == ((250, 461), (252, 464))
    assert L.entries['conv_1/kernel'][1] == (4, 6, 5) and L.entries['ace/bias'][1:] == ((250,), (252,))


def test_xavier_bounds_zero_biases_zero_padding_and_seed():
    L = acr_model.ACRLayout(E=6, filter_sizes=[2, 3], F=5, acr_embeddings_size=7, heads=OrderedDict([('c', 5), ('p', 3)]))
    flat = L.init(42)
    assert flat.dtype == np.float32 and np.array_equal(flat, L.init(42)) and not np.array_equal(flat, L.init(43))
    assert not flat[L.padding_mask()].any()
    for n in L.entries:
        w = L.gather(flat, n)
        if n.endswith('/bias'):
            assert not w.any()
            continue
        fi, fo = L.fan(n)
        lim = math.sqrt(6.0 / (fi + fo))
        assert np.abs(w).max() <= lim and np.abs(w).max() > 0.5 * lim, n
    assert L.fan('conv_1/kernel') == (3 * 6, 3 * 5) and L.fan('fc2/kernel') == (10, 7)


def test_host_validation_raises_before_any_upload():
    heads = OrderedDict([('c', 5)])
    ok = np.array([[0, 49, 3], [1, 1, 0]])
    acr_model.validate_batch(ok, {'c': np.array([0, 4])}, 50, heads)
    with pytest.raises(ValueError, match="token"):
        acr_model.validate_batch(np.array([[0, 50, 3]]), None, 50, heads)
    with pytest.raises(ValueError, match="token"):
        acr_model.validate_batch(np.array([[0, -1, 3]]), None, 50, heads)
    with pytest.raises(ValueError, match="label"):
        acr_model.validate_batch(ok, {'c': np.array([0, 5])}, 50, heads)
    with pytest.raises(ValueError, match="label"):
        acr_model.validate_batch(ok, {'c': np.array([-1, 0])}, 50, heads)


# ---------------------------------------------------------------------------------------------------- reader
@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return synthetic.make_corpus(str(tmp_path_factory.mktemp("acr_corpus")), n_articles=23, n_categories=5, vocab_size=40, embedding_size=4,
                                 articles_by_file=10, seed=3)


def test_reader_truncates_pads_keeps_order_and_partial_batch(corpus):
    arts, cfg = corpus['articles'], corpus['features_config']
    assert len(corpus['files']) == 3 and max(a['text_length'] for a in arts) > 30
    batches = list(acr_datasets.prepare_dataset(corpus['files'], cfg, batch_size=5, epochs=1, shuffle_dataset=False, truncate_tokens_length=30))
    assert [len(f['article_id']) for f, _ in batches] == [5, 5, 5, 5, 3]                 # batches run across file borders; the last is partial
    i = 0
    for f, lab in batches:
        B = len(f['article_id'])
        want_L = max(min(len(a['text']), 30) for a in arts[i:i + B])
        assert f['text'].shape == (B, want_L) and f['text'].dtype == np.int64
        assert set(lab) == {'category_id'} and lab['category_id'].shape == (B,)
        for r in range(B):
            a = arts[i + r]
            n = min(len(a['text']), 30)
            assert np.array_equal(f['text'][r, :n], a['text'][:n]) and not f['text'][r, n:].any()      # first N tokens, no shift, zero pad
            for name in cfg['single_features']:
                assert f[name][r] == a[name]
            assert lab['category_id'][r] == a['category_id']
        i += B
    assert i == len(arts)


def test_reader_epochs_and_seeded_shuffle(corpus):
    cfg = corpus['features_config']
    ids = lambda ds: [tuple(f['article_id']) for f, _ in ds]
    one = ids(acr_datasets.prepare_dataset(corpus['files'], cfg, 4, 1, False, 10, 30))
    assert ids(acr_datasets.prepare_dataset(corpus['files'], cfg, 4, 3, False, 10, 30)) == one * 3
    a = ids(acr_datasets.prepare_dataset(corpus['files'], cfg, 4, 3, True, 5, 30, seed=7))
    b = ids(acr_datasets.prepare_dataset(corpus['files'], cfg, 4, 3, True, 5, 30, seed=7))
    c = ids(acr_datasets.prepare_dataset(corpus['files'], cfg, 4, 3, True, 5, 30, seed=8))
    assert a == b and a != c and a != one * 3 and sorted(a) == sorted(one * 3)


# ---------------------------------------------------------------------------------------------------- gradient of the max
def _autograd_vs_first_index(x, W, bias, dpool):
    """(float64 autograd of the even-split max, closed form under the first-index rule) for dW and dbias."""
    xt = torch.tensor(x, dtype=torch.float64)
    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(bias, dtype=torch.float64, requires_grad=True)
    conv = AO.conv_relu(xt, Wt, bt)
    (conv.amax(dim=1) * torch.tensor(dpool)).sum().backward()
    c = conv.detach().numpy()
    pool, arg = c.max(axis=1), c.argmax(axis=1)              # numpy's argmax: the first index
    g = np.where(pool > 0, dpool, 0.0)
    dW, db = AO.first_index_conv_grads(x, arg, g, W.shape[0])
    ties = (c == pool[:, None, :]).sum(axis=1)
    return Wt.grad.numpy(), bt.grad.numpy(), dW, db, pool, arg, ties


def test_max_gradient_random_data_matches_autograd():
    rng = np.random.RandomState(0)
    x, W, bias, dpool = rng.randn(4, 11, 6), rng.randn(3, 6, 5), rng.randn(5), rng.randn(4, 5)
    aW, ab, dW, db, pool, _, _ = _autograd_vs_first_index(x, W, bias, dpool)
    assert (pool > 0).any()
    np.testing.assert_allclose(dW, aW, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, ab, rtol=1e-12, atol=1e-12)


def test_max_gradient_pad_tail_ties_are_identical_windows():
    """Short articles in a long batch: the pad tail repeats one window, which here attains the max - tied, identical windows."""
    rng = np.random.RandomState(1)
    table = rng.randn(9, 4)
    table[0] = 2.0                                            # the <PAD> row is an ordinary row, and a strong one
    text = np.zeros((3, 12), np.int64)
    text[0, :3] = [3, 4, 5]; text[1, :12] = rng.randint(1, 9, size=12); text[2, :2] = [7, 8]
    W = rng.randn(2, 4, 5); W[:, :, 0] = np.abs(W[:, :, 0]) + 0.5      # filter 0 likes the pad window
    bias, dpool = rng.randn(5), rng.randn(3, 5)
    aW, ab, dW, db, pool, arg, ties = _autograd_vs_first_index(table[text], W, bias, dpool)
    assert ties[0, 0] >= 8 and arg[0, 0] == 3 and ties[2, 0] >= 9 and pool[0, 0] > 0       # the max sits in the pad tail, many times over
    np.testing.assert_allclose(dW, aW, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(db, ab, rtol=1e-12, atol=1e-12)


def test_max_gradient_coincidental_ties_differ_by_design():
    """Two DIFFERENT windows with the same conv value: TF splits the gradient evenly, the kernels give it to the first.  This is the
    only case in which the rules differ; documented here by asserting the difference."""
    x = np.array([[[1.0, 0.0], [0.0, 1.0]]])                 # B = 1, L = 2, E = 2
    W, bias, dpool = np.ones((1, 2, 1)), np.zeros(1), np.ones((1, 1))
    aW, ab, dW, db, _, arg, ties = _autograd_vs_first_index(x, W, bias, dpool)
    assert ties[0, 0] == 2 and arg[0, 0] == 0
    assert np.array_equal(aW[0, :, 0], [0.5, 0.5]) and np.array_equal(dW[0, :, 0], [1.0, 0.0])
    assert np.array_equal(ab, db)                             # the bias gradient is the same under both rules


@pytest.mark.parametrize("name", list(G.CONV_CASES))
def test_gpu_conv_cases_admit_the_exact_argmax_comparison(name):
    """The inputs of the GPU conv tests, checked with the oracle alone: in at least 90 % of the (b, f) pairs the best two distinct values
    lie further apart than twice the rounding bound, so the kernel's argmax must equal the reference's first argmax there."""
    _, _, _, qual, _ = G._expectations(G._case(**G.CONV_CASES[name]))
    assert qual.mean() >= 0.9, qual.mean()


# ---------------------------------------------------------------------------------------------------- weighted CE
def _ce_numpy(logits, labels, w):
    z = logits - logits.max(axis=1, keepdims=True)
    ce = np.log(np.exp(z).sum(axis=1)) - z[np.arange(len(labels)), labels]
    if w is None:
        return ce.mean()
    wb = w[labels]
    return (wb * ce).sum() / (wb != 0).sum() if (wb != 0).any() else 0.0


@pytest.mark.parametrize("weights", [None, [1.0, 2.0, 0.5, 1.5], [0.0, 2.0, 0.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
def test_weighted_ce_reduction_sum_by_nonzero_weights(weights):
    rng = np.random.RandomState(5)
    logits, labels = rng.randn(9, 4), np.array([0, 1, 2, 3, 0, 0, 2, 1, 3])
    w = None if weights is None else np.array(weights)
    got = AO.weighted_ce(torch.tensor(logits), torch.tensor(labels), None if w is None else torch.tensor(w))
    assert abs(float(got) - _ce_numpy(logits, labels, w)) < 1e-12
    if weights == [0.0, 2.0, 0.0, 1.0]:                       # the denominator counts the 4 rows of classes 1 and 3, not all 9
        wb = w[labels]
        assert (wb != 0).sum() == 4 and abs(float(got) * 4 - (wb * (-np.log(np.exp(logits)[np.arange(9), labels] / np.exp(logits).sum(1)))).sum()) < 1e-12
    if weights == [0.0, 0.0, 0.0, 0.0]:
        assert float(got) == 0.0


# ---------------------------------------------------------------------------------------------------- export
def test_export_formats_load_in_both_nar_trainers(tmp_path, corpus):
    rng = np.random.RandomState(2)
    n, D = 7, 6
    preds = [{'acr_embedding': rng.uniform(-1, 1, D).astype(np.float32), 'article_id': np.int64(i), 'category_id': np.int64(i % 3),
              'publisher_id': np.int64(1), 'created_at_ts': np.int64(1000 + i), 'text_length': np.int64(5 + i),
              'predictions-category_id': np.int64(i % 2), 'not_exported': 1} for i in rng.permutation(n)]
    df, ace = acr_trainer_gcom.get_articles_metadata_embeddings(preds)
    assert list(df['article_id']) == list(range(n)) and ace.shape == (n, D) and ace.dtype == np.float32
    assert list(df.columns) == ['article_id', 'category_id', 'created_at_ts', 'publisher_id', 'text_length', 'predictions-category_id']
    by_id = {int(p['article_id']): p for p in preds}
    for i in range(n):
        assert np.array_equal(ace[i], by_id[i]['acr_embedding'])
    with pytest.raises(AssertionError):                        # ids must start at 0 ...
        acr_trainer_gcom.get_articles_metadata_embeddings([p for p in preds if p['article_id'] != 0])
    with pytest.raises(AssertionError):                        # ... and be contiguous
        acr_trainer_gcom.get_articles_metadata_embeddings([p for p in preds if p['article_id'] != 3])

    enc = corpus['acr_label_encoders']
    pk, csv, mat = str(tmp_path / "acr.pickle"), str(tmp_path / "articles.csv"), str(tmp_path / "ace.pickle")
    acr_trainer_gcom.export_acr_metadata_embeddings(enc, df, ace, pk)
    with open(pk, 'rb') as fh:
        assert len(pickle.load(fh)) == 3
    enc2, df2, ace2 = nar_trainer_adressa.load_acr_module_resources(pk)
    assert set(enc2) == set(enc) and df2.equals(df) and np.array_equal(ace2, ace)
    acr_trainer_gcom.export_articles_csv_and_matrix(df, ace, csv, mat)
    df3, ace3 = nar_trainer_gcom.load_acr_module_resources(csv, mat)
    assert np.array_equal(ace3, ace) and list(df3.columns) == list(df.columns) and np.array_equal(df3.values, df.values)


def test_features_config_and_assets(corpus):
    enc, emb = acr_trainer_gcom.load_acr_preprocessing_assets(corpus['label_encoders_path'], corpus['word_vocab_embeddings_path'])
    assert emb.shape == (40, 4) and emb[0].any()              # the <PAD> row is not zero
    cfg = acr_trainer_gcom.get_session_features_config(enc)
    assert list(cfg['single_features']) == ['article_id', 'publisher_id', 'category_id', 'created_at_ts', 'text_length']
    assert cfg['label_features']['category_id'] == {'type': 'categorical', 'dtype': 'int', 'classification_type': 'multiclass', 'cardinality': 5}
    assert cfg['single_features']['article_id']['cardinality'] == 23 and 'cardinality' not in cfg['single_features']['text_length']
