"""ACR trainer for the G1 (globo.com) article corpus: acr_module/acr/acr_trainer_gcom.py on the HIP kernels.

    python -m chameleon_recsys_amd.acr.acr_trainer_gcom --train_set_path_regex '.../articles_tfrecords_*.tfrecord.gz' \
        --input_word_vocab_embeddings_path ... --input_label_encoders_path ... --output_acr_metadata_embeddings_path acr.pickle

Takes the reference's flags with the reference's defaults (:25-61; the model flags of the arms that are not built are accepted and
refused by value, see acr_model.check_supported), trains for training_epochs, evaluates accuracy-<label> on the last 10 files, predicts
every article and exports the (label encoders, articles metadata DataFrame, ACE matrix) pickle that nar_trainer_adressa reads.  Two
flags beyond the reference write the CSV + bare-matrix pair that nar_trainer_gcom reads.  Not carried over: GCS / ML-Engine plumbing
(TF_CONFIG trials), TensorBoard summaries, the profiler hook."""
import argparse
import logging
import os
import pickle
from time import time

import numpy as np

from ..nar.utils import resolve_files
from .acr_datasets import prepare_dataset
from .acr_model import ACR_Model, RANDOM_SEED, check_flags, check_supported

log = logging.getLogger(__name__)

PREDICT_BATCH_SIZE = 16      # :330 "Limits batch size to avoid OOM ..."; an article's embedding depends on its batch's padded length


class ModeKeys:
    TRAIN, EVAL, PREDICT = 'train', 'eval', 'infer'


def build_parser():
    p = argparse.ArgumentParser(prog='acr_trainer_gcom', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # Control params (:25-35)
    p.add_argument('--train_set_path_regex', default='/train*.tfrecord', help='Train set regex')
    p.add_argument('--model_dir', default='./tmp', help='Directory where save model checkpoints')
    p.add_argument('--input_word_vocab_embeddings_path', default='',
                   help='Input path for a pickle with words vocabulary and corresponding word embeddings')
    p.add_argument('--input_label_encoders_path', default='',
                   help='Input path for a pickle with label encoders (article_id, category_id, publisher_id)')
    p.add_argument('--output_acr_metadata_embeddings_path', default='',
                   help='Output path for a pickle with articles metadata and content embeddings')
    # Model params (:38-52)
    p.add_argument('--text_feature_extractor', default='CNN', help='Feature extractor of articles text: (CNN | LSTM | GRU); only CNN is built')
    p.add_argument('--training_task', default='metadata_classification',
                   help='Training task: (metadata_classification | autoencoder); only metadata_classification is built')
    p.add_argument('--autoencoder_noise', type=float, default=0.0, help='(autoencoder task only: unused)')
    p.add_argument('--cnn_filter_sizes', default='3,4,5', help='CNN layers filter sizes (sliding window over words)')
    p.add_argument('--cnn_num_filters', type=int, default=128, help='Number of filters of CNN layers')
    p.add_argument('--rnn_units', type=int, default=250, help='(RNN extractors only: unused)')
    p.add_argument('--rnn_layers', type=int, default=1, help='(RNN extractors only: unused)')
    p.add_argument('--rnn_direction', default='unidirectional', help='(RNN extractors only: unused)')
    p.add_argument('--acr_embeddings_size', type=int, default=250, help='Embedding size of output ACR embeddings')
    # Training params (:56-61)
    p.add_argument('--batch_size', type=int, default=64, help='Batch size')
    p.add_argument('--truncate_tokens_length', type=int, default=300, help='Truncate the sequence of tokens (words) to this limit')
    p.add_argument('--training_epochs', type=int, default=10, help='Training epochs')
    p.add_argument('--learning_rate', type=float, default=1e-3, help='Learning Rate')
    p.add_argument('--dropout_keep_prob', type=float, default=1.0, help='Dropout (keep prob.); only 1.0 is built')
    p.add_argument('--l2_reg_lambda', type=float, default=1e-3, help='L2 regularization')
    # beyond the reference: the form nar_trainer_gcom.load_acr_module_resources reads
    p.add_argument('--output_articles_metadata_csv_path', default='', help='Output path for the articles metadata as CSV')
    p.add_argument('--output_articles_content_embeddings_pickle_path', default='',
                   help='Output path for a pickle with the bare ACE matrix [n_articles, acr_embeddings_size]')
    return p


FLAGS = build_parser().parse_args([])


def serialize(filename, obj):
    with open(filename, 'wb') as fh:
        pickle.dump(obj, fh)


def deserialize(filename):
    with open(filename, 'rb') as fh:
        return pickle.load(fh)


def _cardinality(encoder):
    return len(encoder.classes_) if hasattr(encoder, 'classes_') else len(encoder)


def get_session_features_config(acr_label_encoders):
    """:69-95."""
    features_config = {
        'single_features': {
            'article_id': {'type': 'categorical', 'dtype': 'int'},
            'publisher_id': {'type': 'categorical', 'dtype': 'int'},
            'category_id': {'type': 'categorical', 'dtype': 'int'},
            'created_at_ts': {'type': 'numerical', 'dtype': 'int'},
            'text_length': {'type': 'numerical', 'dtype': 'int'},
        },
        'sequence_features': {
            'text': {'type': 'numerical', 'dtype': 'int'},
        },
        'label_features': {
            'category_id': {'type': 'categorical', 'dtype': 'int', 'classification_type': 'multiclass'},
        },
    }
    for group in features_config.values():
        for name, cfg in group.items():
            if name in acr_label_encoders and cfg['type'] == 'categorical':
                cfg['cardinality'] = _cardinality(acr_label_encoders[name])
    log.info('Session Features: %s', features_config)
    return features_config


def load_acr_preprocessing_assets(acr_label_encoders_path, word_vocab_embeddings_path):
    """:98-105."""
    acr_label_encoders = deserialize(acr_label_encoders_path)
    log.info("Read article id label encoder: %d", _cardinality(acr_label_encoders['article_id']))
    (word_vocab, word_embeddings_matrix) = deserialize(word_vocab_embeddings_path)
    log.info("Read word embeddings: %s", (word_embeddings_matrix.shape,))
    return acr_label_encoders, word_embeddings_matrix


class EstimatorSpec:
    def __init__(self, mode, predictions=None, loss=None, train_op=None, eval_metric_ops=None):
        self.mode, self.predictions, self.loss, self.train_op = mode, predictions, loss, train_op
        self.eval_metric_ops = eval_metric_ops or {}


PREDICT_METADATA = ('article_id', 'category_id', 'publisher_id', 'created_at_ts', 'text_length')


def _variables(params):
    """The model of params['variable_store'], created on first use (the graph's variables of the reference).  params['model_class']
    (default ACR_Model) is the class to construct: acr_trainer_adressa passes ACR_ModelMultilabel."""
    store = params.setdefault('variable_store', {})
    if store.get('model') is None:
        cls = params.get('model_class', ACR_Model)
        store['model'] = cls(params['training_task'], params['text_feature_extractor'], params['features_config']['label_features'],
                             params, device=params.get('device'), seed=params.get('tf_random_seed', RANDOM_SEED))
    return store['model']


def acr_model_fn(features, labels, mode, params):
    """:108-173 without a graph: called once per batch with numpy ``features`` / ``labels``; the variables are the ACR_Model kept in
    params['variable_store'] between calls.  TRAIN runs the step (train_op is done when this returns); EVAL returns per-batch
    (number correct, number of rows) pairs per accuracy-<label>; PREDICT the per-batch arrays of :136-153."""
    model = _variables(params)
    if mode == ModeKeys.TRAIN:
        return EstimatorSpec(mode, loss=model.train_step(features, labels), train_op=True)
    if mode == ModeKeys.EVAL:
        loss, preds = model.eval_step(features, labels)
        metrics = {"accuracy-%s" % n: (int((preds[n] == np.asarray(labels[n]).reshape(-1)).sum()), len(preds[n])) for n in preds}
        return EstimatorSpec(mode, loss=loss, eval_metric_ops=metrics)
    ace, preds = model.predict(features)
    predictions = {'acr_embedding': ace}
    for n in PREDICT_METADATA:
        if n in features:
            predictions[n] = np.asarray(features[n])
    for n, v in preds.items():
        predictions["predictions-%s" % n] = v
    return EstimatorSpec(mode, predictions=predictions)


class ACREstimator:
    """tf.estimator.Estimator's train / evaluate / predict around ``model_fn`` (style of nar/estimator.py): one model_fn call per batch of
    ``input_fn()``, an implicit restore from model_dir, a checkpoint at the end of train."""

    def __init__(self, model_fn, model_dir=None, params=None, tf_random_seed=RANDOM_SEED):
        self._model_fn, self.model_dir = model_fn, model_dir
        self.params = dict(params or {})
        self.params.setdefault('variable_store', {})
        self.params.setdefault('tf_random_seed', tf_random_seed)
        self._restored = False
        if model_dir:
            os.makedirs(model_dir, exist_ok=True)

    @property
    def model(self):
        return self.params['variable_store'].get('model')

    def _ckpt_path(self):
        return os.path.join(self.model_dir, "acr_model.ckpt.pt") if self.model_dir else None

    def _maybe_restore(self):
        if self._restored or self.model is None:
            return
        self._restored = True
        p = self._ckpt_path()
        if p and os.path.exists(p):
            import torch
            self.model.load_state_dict(torch.load(p, map_location="cpu", weights_only=True))
            log.info("Restored %s (global_step %d)", p, self.model.global_step)

    def _call(self, features, labels, mode):
        _variables(self.params)             # the first call creates the variables: restore them before the first step runs
        self._maybe_restore()
        return self._model_fn(features, labels, mode, self.params)

    def save_checkpoint(self):
        p = self._ckpt_path()
        if p and self.model is not None:
            import torch
            torch.save(self.model.state_dict(), p + ".tmp")
            os.replace(p + ".tmp", p)
        return p

    def train(self, input_fn, steps=None):
        n, t0, loss = 0, time(), None
        for features, labels in input_fn():
            if steps is not None and n >= steps:
                break
            loss = self._call(features, labels, ModeKeys.TRAIN).loss
            n += 1
            if n % 100 == 0:
                log.info("step %d: loss %.6f (%.1f steps/s)", self.model.global_step, float(loss[0]), n / max(1e-9, time() - t0))
        if loss is not None:
            log.info("Finished %d training steps: loss %.6f", n, float(loss[0]))
        self.save_checkpoint()
        return self

    def evaluate(self, input_fn, steps=None):
        totals, loss_sum, n = {}, 0.0, 0
        for features, labels in input_fn():
            if steps is not None and n >= steps:
                break
            spec = self._call(features, labels, ModeKeys.EVAL)
            for k, (s, c) in spec.eval_metric_ops.items():
                a = totals.setdefault(k, [0, 0])
                a[0] += s; a[1] += c
            loss_sum += float(spec.loss[0]); n += 1
        out = {k: (s / c if c else 0.0) for k, (s, c) in totals.items()}
        out['loss'] = loss_sum / max(1, n)
        out['global_step'] = self.model.global_step if self.model is not None else 0
        return out

    def predict(self, input_fn):
        """Yields one dict per ARTICLE, as tf.estimator.Estimator.predict does."""
        for features, _ in input_fn():
            pred = self._call(features, None, ModeKeys.PREDICT).predictions
            for i in range(len(pred['acr_embedding'])):
                yield {k: v[i] for k, v in pred.items()}


def build_acr_estimator(model_output_dir, word_embeddings_matrix, features_config, special_token_embedding_vector, flags=None,
                        labels_class_weights=None, device=None):
    """:175-213."""
    F = flags or FLAGS
    params = {'training_task': F.training_task,
              'text_feature_extractor': F.text_feature_extractor,
              'word_embeddings_matrix': word_embeddings_matrix,
              'vocab_size': word_embeddings_matrix.shape[0],
              'word_embedding_size': word_embeddings_matrix.shape[1],
              'cnn_filter_sizes': F.cnn_filter_sizes,
              'rnn_units': F.rnn_units,
              'rnn_layers': F.rnn_layers,
              'rnn_direction': F.rnn_direction,
              'cnn_num_filters': F.cnn_num_filters,
              'dropout_keep_prob': F.dropout_keep_prob,
              'l2_reg_lambda': F.l2_reg_lambda,
              'learning_rate': F.learning_rate,
              'acr_embeddings_size': F.acr_embeddings_size,
              'features_config': features_config,
              'special_token_embedding_vector': special_token_embedding_vector,
              'autoencoder_noise': F.autoencoder_noise,
              'enable_profiler_hook': False,
              'device': device}
    if labels_class_weights:
        params['labels_class_weights'] = labels_class_weights
    return ACREstimator(model_fn=acr_model_fn, model_dir=model_output_dir, params=params, tf_random_seed=RANDOM_SEED)


def export_acr_metadata_embeddings(acr_label_encoders, articles_metadata_df, content_article_embeddings, output_path):
    """:216-219: the (label encoders, articles metadata DataFrame, ACE matrix) pickle."""
    log.info('Exporting ACR Label Encoders, Article metadata and embeddings to %s', output_path)
    serialize(output_path, (acr_label_encoders, articles_metadata_df, content_article_embeddings))


def export_articles_csv_and_matrix(articles_metadata_df, content_article_embeddings, csv_path, matrix_path):
    """The pair nar_trainer_gcom.load_acr_module_resources reads: the metadata as CSV, the bare ACE matrix as a pickle."""
    articles_metadata_df.to_csv(csv_path, index=False)
    serialize(matrix_path, np.asarray(content_article_embeddings, dtype=np.float32))


def get_articles_metadata_embeddings(article_metadata_with_pred_embeddings, ace_column='acr_embedding',
                                     training_task='metadata_classification'):
    """:222-245."""
    import pandas as pd
    articles_metadata_df = pd.DataFrame(article_metadata_with_pred_embeddings).sort_values(by='article_id')

    # Checking whether article ids are sorted and contiguous
    assert (articles_metadata_df['article_id'].head(1).values[0] == 0)
    assert (len(articles_metadata_df) == articles_metadata_df['article_id'].tail(1).values[0] + 1)

    content_article_embeddings = np.vstack(articles_metadata_df[ace_column].values)

    cols_to_export = ['article_id', 'category_id', 'created_at_ts', 'publisher_id', 'text_length']
    if training_task == 'autoencoder':
        cols_to_export.extend(['input_text', 'predicted_word_ids'])
    elif training_task == 'metadata_classification':
        cols_to_export.extend([col for col in articles_metadata_df.columns if col.startswith('predictions-')])
    articles_metadata_df = articles_metadata_df[cols_to_export]
    return articles_metadata_df, content_article_embeddings


def main(argv=None, predict_batch_size=PREDICT_BATCH_SIZE, device=None):
    """:247-346.  Returns dict(eval_results, articles_metadata_df, content_article_embeddings, estimator)."""
    global FLAGS
    FLAGS = build_parser().parse_args(argv)
    check_flags(FLAGS.training_task, FLAGS.text_feature_extractor, FLAGS.dropout_keep_prob)      # refuse what is not built before any work
    np.random.seed(RANDOM_SEED)
    start_train = time()
    log.info('Starting training job')
    log.info('Saving model outputs to %s', FLAGS.model_dir)

    log.info('Loading ACR preprocessing assets')
    acr_label_encoders, word_embeddings_matrix = load_acr_preprocessing_assets(FLAGS.input_label_encoders_path,
                                                                               FLAGS.input_word_vocab_embeddings_path)
    features_config = get_session_features_config(acr_label_encoders)
    check_supported(FLAGS.training_task, FLAGS.text_feature_extractor, features_config['label_features'],
                    {'dropout_keep_prob': FLAGS.dropout_keep_prob})
    input_tfrecords = FLAGS.train_set_path_regex
    log.info('Defining input data (TFRecords): %s', input_tfrecords)

    # (drawn as in the reference, so that numpy's stream stays in step; only the autoencoder would use it)
    special_token_embedding_vector = np.random.uniform(low=-0.04, high=0.04, size=[1, word_embeddings_matrix.shape[1]])
    acr_model = build_acr_estimator(FLAGS.model_dir, word_embeddings_matrix, features_config, special_token_embedding_vector, flags=FLAGS,
                                    device=device)

    log.info('Training model')
    train_files = resolve_files(input_tfrecords)
    if not train_files:
        raise FileNotFoundError("--train_set_path_regex %r matches no file" % input_tfrecords)
    files_to_train = train_files
    log.info("Training articles on TFRecords from %s to %s", files_to_train[0], files_to_train[-1])
    acr_model.train(input_fn=lambda: prepare_dataset(files=files_to_train, features_config=features_config,
                                                     batch_size=FLAGS.batch_size, epochs=FLAGS.training_epochs,
                                                     shuffle_dataset=True, shuffle_buffer_size=5000,
                                                     truncate_tokens_length=FLAGS.truncate_tokens_length))

    eval_results = None
    if FLAGS.training_task == 'metadata_classification':
        # The objective is to overfit this network, so that the ACR embedding represents the articles' content well
        log.info('Evaluating model')
        files_to_eval = train_files[-10:]
        eval_results = acr_model.evaluate(input_fn=lambda: prepare_dataset(files=files_to_eval, features_config=features_config,
                                                                           batch_size=FLAGS.batch_size, epochs=1, shuffle_dataset=False,
                                                                           truncate_tokens_length=FLAGS.truncate_tokens_length))
        log.info('Evaluation results with TRAIN SET (objective is to overfit): %s', eval_results)

    log.info('Predicting ACR embeddings')
    article_metadata_with_pred_embeddings = list(acr_model.predict(
        input_fn=lambda: prepare_dataset(files=train_files, features_config=features_config, batch_size=predict_batch_size, epochs=1,
                                         shuffle_dataset=False, truncate_tokens_length=FLAGS.truncate_tokens_length)))
    articles_metadata_df, content_article_embeddings = get_articles_metadata_embeddings(
        article_metadata_with_pred_embeddings, ace_column='acr_embedding', training_task=FLAGS.training_task)
    log.info('Generated ACR embeddings (shape): %s', (content_article_embeddings.shape,))
    log.info('Generated ACR metadata (qtde): %d', len(articles_metadata_df))

    if FLAGS.output_acr_metadata_embeddings_path:
        export_acr_metadata_embeddings(acr_label_encoders, articles_metadata_df, content_article_embeddings,
                                       FLAGS.output_acr_metadata_embeddings_path)
    if FLAGS.output_articles_metadata_csv_path or FLAGS.output_articles_content_embeddings_pickle_path:
        if not (FLAGS.output_articles_metadata_csv_path and FLAGS.output_articles_content_embeddings_pickle_path):
            raise ValueError("--output_articles_metadata_csv_path and --output_articles_content_embeddings_pickle_path go together")
        export_articles_csv_and_matrix(articles_metadata_df, content_article_embeddings, FLAGS.output_articles_metadata_csv_path,
                                       FLAGS.output_articles_content_embeddings_pickle_path)
    log.info('Finalized TRAINING in %.1f s', time() - start_train)
    return dict(eval_results=eval_results, articles_metadata_df=articles_metadata_df,
                content_article_embeddings=content_article_embeddings, estimator=acr_model)


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(levelname)s:%(message)s')
    main()
