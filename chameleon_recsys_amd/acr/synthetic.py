"""A small synthetic article corpus in the ACR module's input formats (what acr_module/acr/preprocessing produces for the trainer):
GZIP TFRecord files of SequenceExample (article_id, publisher_id, category_id, created_at_ts, text_length; text), the
(word_vocab, word_embeddings_matrix) pickle and the label-encoders pickle.

Tokens are drawn from category-dependent distributions - each category prefers its own slice of the vocabulary - so that the
category classifier has something to learn.  Lengths are ragged and some exceed ``long_len`` (pick truncate_tokens_length below it).

``make_corpus_adressa`` writes the same in the Adressa trainer's formats: ids from 1, category0 / category1 / author, five ragged id
lists per article (keywords depend on the category), and the (label encoders, class weights) pickle."""
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


# ---------------------------------------------------------------------------------------------------- Adressa
ADRESSA_LISTS = ('keywords', 'concepts', 'entities', 'locations', 'persons')


def make_articles_adressa(n_articles=200, n_categories=5, n_subcategories=7, n_authors=4, n_keywords=41, n_list_values=12, max_keywords=6,
                          empty_keywords_share=0.15, empty_keywords_run=(16, 16), own_keyword_prob=0.8, seed=0, **kw):
    """make_articles with the Adressa columns: ids are 1 .. n_articles (0 is the padding article), category0 / category1 / author
    instead of category_id / publisher_id, and five ragged id lists.  Keyword ids lie in 1 .. n_keywords-1 (0 = <PAD> never occurs) and
    prefer the category's own slice, so that the multilabel head has something to learn; a share of the lists is empty, and so is every
    list of the ``empty_keywords_run`` = (first index, count) articles, so that whole batches of the unshuffled stream have none."""
    rng = np.random.RandomState(seed + 7)
    rows = []
    per_cat = max(1, (n_keywords - 1) // n_categories)
    for i, a in enumerate(make_articles(n_articles, n_categories, 1, seed=seed, **kw)):
        cat = a['category_id']
        nk = int(rng.randint(1, max_keywords + 1))
        own = rng.rand(nk) < own_keyword_prob
        lo = 1 + (cat * per_cat) % (n_keywords - 1)
        ids = np.minimum(np.where(own, lo + rng.randint(per_cat, size=nk), rng.randint(1, n_keywords, size=nk)), n_keywords - 1)
        keywords = np.unique(ids).astype(np.int64)
        empty = rng.rand() < empty_keywords_share
        if empty or empty_keywords_run[0] <= i < empty_keywords_run[0] + empty_keywords_run[1]:
            keywords = keywords[:0]
        row = dict(article_id=i + 1, category0=cat, category1=int(rng.randint(n_subcategories)), author=int(rng.randint(n_authors)),
                   created_at_ts=a['created_at_ts'], text_length=a['text_length'], text=a['text'], keywords=keywords)
        for name in ADRESSA_LISTS[1:]:
            row[name] = rng.randint(1, n_list_values, size=int(rng.randint(0, 4))).astype(np.int64)
        rows.append(row)
    return rows


def _pb_varint(v):
    v &= (1 << 64) - 1
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _pb_field(no, payload):
    """One length-delimited protobuf field."""
    return _pb_varint(no << 3 | 2) + _pb_varint(len(payload)) + payload


def _pb_int64_feature(values):
    """tf.train.Feature(int64_list=...) with the packed encoding TensorFlow writes."""
    return _pb_field(3, _pb_field(1, b''.join(_pb_varint(int(v)) for v in values)) if len(values) else b'')


def sequence_example(row, features_config):
    """tf.train.SequenceExample of one article: int64 context scalars, and per sequence feature a FeatureList with one int64 Feature per
    element (what the reference's preprocessing writes).  The lists of one article have different lengths, which the session writer of
    nar/tf_records_management.py does not express."""
    ctx = b''.join(_pb_field(1, _pb_field(1, n.encode()) + _pb_field(2, _pb_int64_feature([row[n]])))
                   for n in features_config['single_features'])
    seq = b''.join(_pb_field(1, _pb_field(1, n.encode()) + _pb_field(2, b''.join(_pb_field(1, _pb_int64_feature([v])) for v in row[n])))
                   for n in features_config['sequence_features'])
    return _pb_field(1, ctx) + _pb_field(2, seq)


def export_articles_to_tf_records(articles, features_config, output_path, examples_by_file=1000):
    """GZIP TFRecord files of sequence_example records through the C++ codec's raw record writer; '*' -> 4-digit chunk index."""
    from .. import _tfrecord
    lib = _tfrecord.load()
    out = []
    for i in range(0, len(articles), examples_by_file):
        path = output_path.replace('*', '%04d' % (i // examples_by_file))
        h = lib.cham_tfw_open(path.encode(), 6)
        if not h:
            raise _tfrecord.TFRecordError("cannot open %s for writing" % path)
        try:
            for row in articles[i:i + examples_by_file]:
                rec = sequence_example(row, features_config)
                _tfrecord.check(lib.cham_tfw_write_record(h, rec, len(rec)), "cham_tfw_write_record")
        finally:
            _tfrecord.check(lib.cham_tfw_close(h), "cham_tfw_close")
        out.append(path)
    return out


def make_corpus_adressa(out_dir, n_articles=200, n_categories=5, n_subcategories=7, n_authors=4, n_keywords=41, n_list_values=12,
                        vocab_size=60, embedding_size=12, articles_by_file=50, seed=0, **kw):
    """make_corpus for acr_trainer_adressa: the label-encoders pickle is the (encoders, labels_class_weights) tuple, encoders are the
    reference's value -> id dicts (article_id with a <PAD> entry: n_articles + 1 values) and category0 has balanced class weights of
    full cardinality.  Returns make_corpus's dict plus labels_class_weights."""
    from .acr_trainer_adressa import get_session_features_config as adressa_features_config
    os.makedirs(out_dir, exist_ok=True)
    rng = np.random.RandomState(seed + 1)
    articles = make_articles_adressa(n_articles, n_categories, n_subcategories, n_authors, n_keywords, n_list_values,
                                     vocab_size=vocab_size, seed=seed, **kw)
    word_vocab = {('<PAD>' if i == 0 else 'w%d' % i): i for i in range(vocab_size)}
    emb = rng.uniform(-0.5, 0.5, size=(vocab_size, embedding_size)).astype(np.float32)
    padded = lambda prefix, n: {('<PAD>' if i == 0 else '%s%d' % (prefix, i)): i for i in range(n)}
    encoders = {'article_id': padded('a', n_articles + 1), 'category0': {'c%d' % i: i for i in range(n_categories)},
                'category1': {'s%d' % i: i for i in range(n_subcategories)}, 'author': {'u%d' % i: i for i in range(n_authors)},
                'keywords': padded('k', n_keywords)}
    for name in ADRESSA_LISTS[1:]:
        encoders[name] = padded(name[0], n_list_values)
    counts = np.bincount([a['category0'] for a in articles], minlength=n_categories)
    class_weights = {'category0': np.where(counts > 0, len(articles) / (n_categories * np.maximum(counts, 1)), 1.0)}     # "balanced"
    vocab_path = os.path.join(out_dir, 'acr_word_vocab_embeddings.pickle')
    enc_path = os.path.join(out_dir, 'acr_label_encoders.pickle')
    with open(vocab_path, 'wb') as fh:
        pickle.dump((word_vocab, emb), fh)
    with open(enc_path, 'wb') as fh:
        pickle.dump((encoders, class_weights), fh)
    cfg = adressa_features_config(encoders)
    regex = os.path.join(out_dir, 'articles_tfrecords_*.tfrecord.gz')
    files = export_articles_to_tf_records(articles, cfg, regex, examples_by_file=articles_by_file)
    return dict(files=files, train_set_path_regex=regex, word_vocab_embeddings_path=vocab_path, label_encoders_path=enc_path,
                articles=articles, word_embeddings_matrix=emb, acr_label_encoders=encoders, labels_class_weights=class_weights,
                features_config=cfg)
