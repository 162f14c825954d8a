"""ACR trainer for the Adressa article corpus: acr_module/acr/acr_trainer_adressa.py on the HIP kernels.

    python -m chameleon_recsys_amd.acr.acr_trainer_adressa --train_set_path_regex '.../articles_tfrecords_*.tfrecord.gz' \
        --input_word_vocab_embeddings_path ... --input_label_encoders_path ... --output_acr_metadata_embeddings_path acr.pickle

Takes the reference's flags with the reference's defaults (:23-57; there is no --truncate_tokens_length: prepare_dataset's default of
300 applies; the model flags of the arms that are not built are accepted and refused by value before any file is read, see
acr_model.check_flags).  Label heads: category0 (multiclass, with the class weights of the label-encoders pickle) and keywords
(multilabel, the sigmoid cross-entropy head of ACR_ModelMultilabel).  Trains for training_epochs on all files, evaluates
accuracy-category0, precision-keywords and recall-keywords on all files, predicts every article at --batch_size and exports the
(label encoders, articles metadata DataFrame, ACE matrix) pickle that nar_trainer_adressa reads: article ids start at 1, and row 0 of
the ACE matrix is the padding article, the mean embedding (:257-297).  The estimator, its checkpointing and the pickle writer are
acr_trainer_gcom's.  Not carried over: GCS / ML-Engine plumbing (TF_CONFIG trials), TensorBoard summaries, the profiler hook, and the
concepts / entities / locations / persons input columns that the reference's model_fn builds and its model leaves unused."""
import argparse
import logging
from time import time

import numpy as np

from ..nar.utils import resolve_files
from .acr_datasets import prepare_dataset
from .acr_model import ACR_ModelMultilabel, RANDOM_SEED, check_flags, check_supported
from .acr_trainer_gcom import (ACREstimator, EstimatorSpec, ModeKeys, _cardinality, _variables, deserialize,
                               export_acr_metadata_embeddings)

log = logging.getLogger(__name__)

PREDICTIONS_PREFIX = "predictions-"


def build_parser():
    p = argparse.ArgumentParser(prog='acr_trainer_adressa', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    # Control params (:23-33)
    p.add_argument('--train_set_path_regex', default='/train*.tfrecord', help='Train set regex')
    p.add_argument('--model_dir', default='./tmp', help='Directory where save model checkpoints')
    p.add_argument('--input_word_vocab_embeddings_path', default='',
                   help='Input path for a pickle with words vocabulary and corresponding word embeddings')
    p.add_argument('--input_label_encoders_path', default='',
                   help='Input path for a pickle with (label encoders, labels class weights)')
    p.add_argument('--output_acr_metadata_embeddings_path', default='',
                   help='Output path for a pickle with articles metadata and content embeddings')
    # Model params (:36-49)
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
    # Training params (:53-57)
    p.add_argument('--batch_size', type=int, default=64, help='Batch size')
    p.add_argument('--training_epochs', type=int, default=10, help='Training epochs')
    p.add_argument('--learning_rate', type=float, default=1e-3, help='Learning Rate')
    p.add_argument('--dropout_keep_prob', type=float, default=1.0, help='Dropout (keep prob.); only 1.0 is built')
    p.add_argument('--l2_reg_lambda', type=float, default=1e-3, help='L2 regularization')
    return p


FLAGS = build_parser().parse_args([])


def get_session_features_config(acr_label_encoders):
    """:65-100."""
    features_config = {
        'single_features': {
            'article_id': {'type': 'categorical', 'dtype': 'int'},
            'category0': {'type': 'categorical', 'dtype': 'int'},
            'category1': {'type': 'categorical', 'dtype': 'int'},
            'author': {'type': 'categorical', 'dtype': 'int'},
            'created_at_ts': {'type': 'numerical', 'dtype': 'int'},
            'text_length': {'type': 'numerical', 'dtype': 'int'},
        },
        'sequence_features': {
            'text': {'type': 'numerical', 'dtype': 'int'},
            'keywords': {'type': 'categorical', 'dtype': 'int'},
            'concepts': {'type': 'categorical', 'dtype': 'int'},
            'entities': {'type': 'categorical', 'dtype': 'int'},
            'locations': {'type': 'categorical', 'dtype': 'int'},
            'persons': {'type': 'categorical', 'dtype': 'int'},
        },
        'label_features': {
            # feature_weight_on_loss is what the reference's config carries; its model reads the key from the wrong dict, so every head
            # enters the loss with weight 1.0 whatever stands here (acr_model.py:219, kept: acr_model.ACR_Model)
            'category0': {'type': 'categorical', 'dtype': 'int', 'classification_type': 'multiclass', 'feature_weight_on_loss': 1.0},
            'keywords': {'type': 'categorical', 'dtype': 'int', 'classification_type': 'multilabel', 'feature_weight_on_loss': 1.0},
        },
    }
    for group in features_config.values():
        for name, cfg in group.items():
            if name in acr_label_encoders and cfg['type'] == 'categorical':
                cfg['cardinality'] = _cardinality(acr_label_encoders[name])
    log.info('Session Features: %s', features_config)
    return features_config


def load_acr_preprocessing_assets(acr_label_encoders_path, word_vocab_embeddings_path):
    """:103-113: the label-encoders pickle is the (encoders, labels_class_weights) tuple."""
    (acr_label_encoders, labels_class_weights) = deserialize(acr_label_encoders_path)
    log.info("Read article id label encoder: %d", _cardinality(acr_label_encoders['article_id']))
    log.info("Classes weights available for: %s", list(labels_class_weights.keys()))
    (word_vocab, word_embeddings_matrix) = deserialize(word_vocab_embeddings_path)
    log.info("Read word embeddings: %s", (word_embeddings_matrix.shape,))
    return acr_label_encoders, labels_class_weights, word_embeddings_matrix


# what PREDICT returns beside acr_embedding and the heads' predictions (:166-177); 'input_text' is features['text']
PREDICT_METADATA = ('article_id', 'category0', 'category1', 'author', 'keywords', 'concepts', 'entities', 'locations', 'persons',
                    'created_at_ts', 'text_length')


def acr_model_fn(features, labels, mode, params):
    """:122-208 without a graph (see acr_trainer_gcom.acr_model_fn).  EVAL returns per-batch (numerator, denominator) pairs:
    accuracy-<head> = (correct, rows) for a multiclass head, precision-<head> = (tp, tp + fp) and recall-<head> = (tp, tp + fn) for
    a multilabel one; ACREstimator.evaluate sums the pairs and divides (0 for an empty denominator, as tf.metrics)."""
    model = _variables(params)
    if mode == ModeKeys.TRAIN:
        return EstimatorSpec(mode, loss=model.train_step(features, labels), train_op=True)
    if mode == ModeKeys.EVAL:
        loss, preds = model.eval_step(features, labels)
        counts = model.multilabel_counts()
        metrics = {}
        for n in preds:
            if n in counts:
                tp, fp, fn = counts[n]
                metrics["precision-%s" % n] = (tp, tp + fp)
                metrics["recall-%s" % n] = (tp, tp + fn)
            else:
                metrics["accuracy-%s" % n] = (int((preds[n] == np.asarray(labels[n]).reshape(-1)).sum()), len(preds[n]))
        return EstimatorSpec(mode, loss=loss, eval_metric_ops=metrics)
    ace, preds = model.predict(features)
    predictions = {'acr_embedding': ace}
    for n in PREDICT_METADATA:
        predictions[n] = np.asarray(features[n])
    predictions['input_text'] = np.asarray(features['text'])
    for n, v in preds.items():
        predictions["%s%s" % (PREDICTIONS_PREFIX, n)] = v
    return EstimatorSpec(mode, predictions=predictions)


def build_acr_estimator(model_output_dir, word_embeddings_matrix, features_config, labels_class_weights, special_token_embedding_vector,
                        flags=None, device=None):
    """:210-247."""
    F = flags or FLAGS
    params = {'training_task': F.training_task,
              'text_feature_extractor': F.text_feature_extractor,
              'word_embeddings_matrix': word_embeddings_matrix,
              'vocab_size': word_embeddings_matrix.shape[0],
              'word_embedding_size': word_embeddings_matrix.shape[1],
              'cnn_filter_sizes': F.cnn_filter_sizes,
              'cnn_num_filters': F.cnn_num_filters,
              'rnn_units': F.rnn_units,
              'rnn_layers': F.rnn_layers,
              'rnn_direction': F.rnn_direction,
              'dropout_keep_prob': F.dropout_keep_prob,
              'l2_reg_lambda': F.l2_reg_lambda,
              'learning_rate': F.learning_rate,
              'acr_embeddings_size': F.acr_embeddings_size,
              'features_config': features_config,
              'labels_class_weights': labels_class_weights,
              'special_token_embedding_vector': special_token_embedding_vector,
              'autoencoder_noise': F.autoencoder_noise,
              'enable_profiler_hook': False,
              'model_class': ACR_ModelMultilabel,
              'device': device}
    return ACREstimator(model_fn=acr_model_fn, model_dir=model_output_dir, params=params, tf_random_seed=RANDOM_SEED)


def get_articles_metadata_embeddings(article_metadata_with_pred_embeddings, training_task='metadata_classification'):
    """:257-297: ids start at 1 (0 is the padding article) and are contiguous; the ACE matrix gets the padding article's row in front,
    the mean embedding, so that it has n + 1 rows."""
    import pandas as pd
    articles_metadata_df = pd.DataFrame(article_metadata_with_pred_embeddings).sort_values(by='article_id')
    log.info("First article id: %s", articles_metadata_df['article_id'].head(1).values[0])
    log.info("Last article id: %s", articles_metadata_df['article_id'].tail(1).values[0])

    # Checking whether article ids are sorted and contiguous
    assert (articles_metadata_df['article_id'].head(1).values[0] == 1)  # 0 is reserved for padding
    assert (len(articles_metadata_df) == articles_metadata_df['article_id'].tail(1).values[0])

    content_article_embeddings = np.vstack(articles_metadata_df['acr_embedding'].values)

    # Creating an embedding for the padding article
    embedding_for_padding_article = np.mean(content_article_embeddings, axis=0)
    content_article_embeddings_with_padding = np.vstack([embedding_for_padding_article, content_article_embeddings])
    assert content_article_embeddings_with_padding.shape[0] == articles_metadata_df['article_id'].tail(1).values[0] + 1

    # Converting the keywords multi-label predictions from the multi-hot representation back to lists of keyword ids
    preds_keywords_column_name = "%s%s" % (PREDICTIONS_PREFIX, "keywords")
    if preds_keywords_column_name in articles_metadata_df.columns:
        articles_metadata_df[preds_keywords_column_name] = articles_metadata_df[preds_keywords_column_name].apply(lambda x: x.nonzero()[0])

    cols_to_export = ['article_id', 'category0', 'category1', 'author', 'keywords', 'concepts', 'entities', 'locations', 'persons',
                      'created_at_ts', 'text_length', 'input_text']
    if training_task == 'autoencoder':
        cols_to_export.extend(['predicted_word_ids'])
    elif training_task == 'metadata_classification':
        cols_to_export.extend([col for col in articles_metadata_df.columns if col.startswith(PREDICTIONS_PREFIX)])
    articles_metadata_df = articles_metadata_df[cols_to_export]
    return articles_metadata_df, content_article_embeddings_with_padding


def main(argv=None, device=None):
    """:299-406.  Returns dict(eval_results, articles_metadata_df, content_article_embeddings, estimator)."""
    global FLAGS
    FLAGS = build_parser().parse_args(argv)
    check_flags(FLAGS.training_task, FLAGS.text_feature_extractor, FLAGS.dropout_keep_prob)      # refuse what is not built before any work
    np.random.seed(RANDOM_SEED)
    start_train = time()
    log.info('Starting training job')
    log.info('Saving model outputs to %s', FLAGS.model_dir)

    log.info('Loading ACR preprocessing assets')
    acr_label_encoders, labels_class_weights, word_embeddings_matrix = load_acr_preprocessing_assets(
        FLAGS.input_label_encoders_path, FLAGS.input_word_vocab_embeddings_path)
    features_config = get_session_features_config(acr_label_encoders)
    check_supported(FLAGS.training_task, FLAGS.text_feature_extractor, features_config['label_features'],
                    {'dropout_keep_prob': FLAGS.dropout_keep_prob}, multilabel=True)
    input_tfrecords = FLAGS.train_set_path_regex
    log.info('Defining input data (TFRecords): %s', input_tfrecords)

    # (drawn as in the reference, so that numpy's stream stays in step; only the autoencoder would use it)
    special_token_embedding_vector = np.random.uniform(low=-0.04, high=0.04, size=[1, word_embeddings_matrix.shape[1]])
    acr_model = build_acr_estimator(FLAGS.model_dir, word_embeddings_matrix, features_config, labels_class_weights,
                                    special_token_embedding_vector, flags=FLAGS, device=device)

    log.info('Training model')
    train_files = resolve_files(input_tfrecords)
    if not train_files:
        raise FileNotFoundError("--train_set_path_regex %r matches no file" % input_tfrecords)
    log.info("Training articles on TFRecords from %s to %s", train_files[0], train_files[-1])
    acr_model.train(input_fn=lambda: prepare_dataset(files=train_files, features_config=features_config, batch_size=FLAGS.batch_size,
                                                     epochs=FLAGS.training_epochs, shuffle_dataset=True, shuffle_buffer_size=10000))

    # The objective is to overfit this network, so that the ACR embedding represents the articles' content well
    log.info('Evaluating model - TRAIN SET')
    eval_results = acr_model.evaluate(input_fn=lambda: prepare_dataset(files=train_files, features_config=features_config,
                                                                       batch_size=FLAGS.batch_size, epochs=1, shuffle_dataset=False))
    log.info('Evaluation results with TRAIN SET (objective is to overfit): %s', eval_results)

    log.info('Predicting ACR embeddings')
    article_metadata_with_pred_embeddings = list(acr_model.predict(
        input_fn=lambda: prepare_dataset(files=train_files, features_config=features_config, batch_size=FLAGS.batch_size, epochs=1,
                                         shuffle_dataset=False)))
    articles_metadata_df, content_article_embeddings = get_articles_metadata_embeddings(article_metadata_with_pred_embeddings,
                                                                                        training_task=FLAGS.training_task)
    log.info('Generated ACR embeddings: %s', (content_article_embeddings.shape,))

    if FLAGS.output_acr_metadata_embeddings_path:
        export_acr_metadata_embeddings(acr_label_encoders, articles_metadata_df, content_article_embeddings,
                                       FLAGS.output_acr_metadata_embeddings_path)
    log.info('Finalized TRAINING in %.1f s', time() - start_train)
    return dict(eval_results=eval_results, articles_metadata_df=articles_metadata_df,
                content_article_embeddings=content_article_embeddings, estimator=acr_model)


if __name__ == '__main__':
    logging.basicConfig(level=logging.INFO, format='%(levelname)s:%(message)s')
    main()
