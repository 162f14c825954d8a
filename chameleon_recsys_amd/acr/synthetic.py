"""A small synthetic article corpus in the ACR module's input formats (what acr_module/acr/preprocessing produces for the trainer):
GZIP TFRecord files of SequenceExample (article_id, publisher_id, category_id, created_at_ts, text_length; text), the
(word_vocab, word_embeddings_matrix) pickle and the label-encoders pickle.

Tokens are drawn from category-dependent distributions - each category prefers its own slice of the vocabulary - so that the
category classifier has something to learn.  Lengths are ragged and some exceed ``long_len`` (pick truncate_tokens_length below it)."""
import os
import pickle

import numpy as np

from ..nar.tf_records_management import export_sessions_to_tf_records
from .acr_trainer_gcom import get_session_features_config


def make_articles(n_articles=200, n_categories=5, n_publishers=3, vocab_size=60, min_len=4, max_len=24, long_len=40, long_share=0.1,
                  own_token_prob=0.7, seed=0):
    """List of article dicts; ids are 0 .. n_articles-1 (contiguous, as the exporter asserts).  Token 0 = <PAD> never occurs in a text."""
    rng = np.random.RandomState(seed)
    per_cat = max(1, (vocab_size - 1) // n_categories)
    rows = []
    for i in range(n_articles):
        cat = int(rng.randint(n_categories))
        n = int(rng.randint(long_len, long_len + 10)) if rng.rand() < long_share else int(rng.randint(min_len, max_len + 1))
        own = rng.rand(n) < own_token_prob
        lo = 1 + (cat * per_cat) % (vocab_size - 1)
        tok_own = lo + rng.randint(per_cat, size=n)
        tok_any = rng.randint(1, vocab_size, size=n)
        text = np.minimum(np.where(own, tok_own, tok_any), vocab_size - 1).astype(np.int64)
        rows.append(dict(article_id=i, publisher_id=int(rng.randint(n_publishers)), category_id=cat,
                         created_at_ts=1500000000000 + 3600000 * i, text_length=n, text=text))
    return rows


def make_corpus(out_dir, n_articles=200, n_categories=5, n_publishers=3, vocab_size=60, embedding_size=12, articles_by_file=50, seed=0,
                **kw):
    """Writes the corpus under out_dir; returns dict(files, train_set_path_regex, word_vocab_embeddings_path, label_encoders_path,
    articles, word_embeddings_matrix, acr_label_encoders)."""
    from sklearn.preprocessing import LabelEncoder
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.RandomState(seed + 1)
    articles = make_articles(n_articles, n_categories, n_publishers, vocab_size, seed=seed, **kw)
    word_vocab = {('<PAD>' if i == 0 else 'w%d' % i): i for i in range(vocab_size)}
    emb = rng.uniform(-0.5, 0.5, size=(vocab_size, embedding_size)).astype(np.float32)     # the <PAD> row is non-zero, as in the reference
    encoders = {}
    for name, n in (('article_id', n_articles), ('category_id', n_categories), ('publisher_id', n_publishers)):
        encoders[name] = LabelEncoder().fit(np.arange(n))
    vocab_path = os.path.join(out_dir, 'acr_word_vocab_embeddings.pickle')
    enc_path = os.path.join(out_dir, 'acr_label_encoders.pickle')
    with open(vocab_path, 'wb') as fh:
        pickle.dump((word_vocab, emb), fh)
    with open(enc_path, 'wb') as fh:
        pickle.dump(encoders, fh)
    cfg = get_session_features_config(encoders)
    files = export_sessions_to_tf_records(articles, cfg, os.path.join(out_dir, 'articles_tfrecords_*.tfrecord.gz'),
                                          examples_by_file=articles_by_file)
    return dict(files=files, train_set_path_regex=os.path.join(out_dir, 'articles_tfrecords_*.tfrecord.gz'),
                word_vocab_embeddings_path=vocab_path, label_encoders_path=enc_path, articles=articles, word_embeddings_matrix=emb,
                acr_label_encoders=encoders, features_config=cfg)
