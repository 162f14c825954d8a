"""Beyond-accuracy evaluation metrics on the GPU (csrc/eval_metrics.hip): cham_eval_beyond_accuracy against the host metric classes
(themselves pinned against the reference by tests/test_beyond_accuracy_metrics.py), exact coverage counts (a table whose row offsets
pass 2^31 bytes included), and --eval_beyond_accuracy_metrics end to end through nar_trainer_gcom.main with the device and the host
recent-clicks state.  Tolerances: rtol 2e-5, atol 1e-6 (fp32 on the device; ESI is fp64 on the host)."""
import os

import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import check, ptr
from chameleon_recsys_amd.nar import evaluation, metrics, nar_trainer_gcom as T, synthetic
from chameleon_recsys_amd.nar.estimator import Estimator, SessionRunArgs, SessionRunHook

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-5, 1e-6
PER_CLICK = metrics.BEYOND_ACCURACY_PER_CLICK
SIX = ('ndcg_at_n', 'item_coverage_at_n', 'esi-r_at_n', 'esi-rr_at_n', 'content_eild-r_at_n', 'content_eild-rr_at_n')


def _run_kernel(lib, dev, preds, labels, clicked, ace_d, pop_d, topn, rel_neg, maps=None):
    B, T_, NC = preds.shape
    p = torch.from_numpy(np.ascontiguousarray(preds)).to(dev)
    lab = torch.from_numpy(np.ascontiguousarray(labels)).to(dev)
    clk = torch.from_numpy(np.ascontiguousarray(clicked)).to(dev)
    out = torch.full((B * T_, 4), 7.0, dtype=torch.float32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    rec_map, clk_map = maps if maps is not None else (None, None)
    check(lib.cham_eval_beyond_accuracy(ptr(p), NC, ptr(lab), ptr(clk), B * T_, ptr(ace_d), ace_d.shape[1], ace_d.shape[0], ptr(pop_d),
                                        topn, 1.0, rel_neg, ptr(out), ptr(rec_map), ptr(clk_map), s), "cham_eval_beyond_accuracy")
    return out.view(B, T_, 4).cpu().numpy()


def _host_values(preds, labels, ace, pop64, topn, rel_neg):
    ms = [metrics.ExpectedRankSensitiveNovelty(topn), metrics.ExpectedRankRelevanceSensitiveNovelty(topn, 1.0, rel_neg),
          metrics.ContentExpectedRankRelativeSensitiveIntraListDiversity(topn, ace),
          metrics.ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity(topn, ace, 1.0, rel_neg)]
    evaluation.update_metrics(preds, labels, None, pop64[preds], None, ms)
    return np.stack([np.array(m.results) for m in ms], axis=-1)


def _inputs(rng, n_items, B, T_, NC, zero_row=7):
    preds = np.stack([np.stack([rng.choice(np.arange(1, n_items), NC, replace=False) for _ in range(T_)]) for _ in range(B)])
    labels = rng.integers(1, n_items, size=(B, T_))
    inside = rng.random((B, T_)) < 0.5
    labels = np.where(inside, np.take_along_axis(preds, rng.integers(0, min(NC, 5), size=(B, T_, 1)), -1)[..., 0], labels)
    labels[1, :] = 0                                      # an all-padded session
    labels[2, 3:] = 0                                     # a ragged one
    preds[0, 0, 1] = preds[0, 0, 0]                       # duplicate ids in a list
    preds[0, 1, 0] = zero_row                             # a zero-norm ACE row ranked first ...
    preds[0, 2, 1] = zero_row                             # ... and second
    preds[3, 0, 2] = 0                                    # id 0 ranked
    clicked = rng.integers(0, n_items, size=(B, T_))
    clicked[:, -1] = 0
    return preds.astype(np.int64), labels.astype(np.int64), clicked.astype(np.int64)


@pytest.mark.parametrize("topn,NC", [(2, 5), (3, 13), (10, 6), (10, 51), (64, 67)])
@pytest.mark.parametrize("D", [64, 128, 250])
def test_kernel_matches_the_host_classes(gpu, topn, NC, D):
    lib = _lib.load()
    rng = np.random.default_rng(1000 * topn + D + NC)
    n_items, B, T_ = 400, 5, 6
    ace = rng.normal(size=(n_items, D)).astype(np.float32)
    ace[7] = 0.0
    pop = np.maximum(rng.random(n_items) ** 3, 1.0 / 200).astype(np.float32)
    pop[rng.integers(0, n_items, 30)] = np.float32(1.0 / 200)
    preds, labels, clicked = _inputs(rng, n_items, B, T_, NC)
    ace_d, pop_d = torch.from_numpy(ace).to(gpu), torch.from_numpy(pop).to(gpu)
    for rel_neg in (0.1, 0.5):
        got = _run_kernel(lib, gpu, preds, labels, clicked, ace_d, pop_d, topn, rel_neg)
        again = _run_kernel(lib, gpu, preds, labels, clicked, ace_d, pop_d, topn, rel_neg)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two launches differ"
        valid = labels != 0
        assert (got[~valid] == 0).all()
        ref = _host_values(preds, labels, ace, pop.astype(np.float64), topn, rel_neg)
        np.testing.assert_allclose(got[valid], ref, rtol=RTOL, atol=ATOL)


def test_kernel_nan_at_relevance_zero_matches_the_host(gpu):
    lib = _lib.load()
    rng = np.random.default_rng(5)
    ace = rng.normal(size=(50, 32)).astype(np.float32)
    pop = np.full(50, 0.25, np.float32)
    preds = np.array([[[1, 2, 3, 4], [5, 6, 7, 8]]], np.int64)
    labels = np.array([[30, 7]], np.int64)                # not in the top 3 -> EILD-RR 0/0; positive third -> finite
    got = _run_kernel(lib, gpu, preds, labels, np.zeros_like(labels), torch.from_numpy(ace).to(gpu), torch.from_numpy(pop).to(gpu), 3, 0.0)
    assert np.isnan(got[0, 0, 3]) and np.isfinite(got[0, 1, 3]) and np.isfinite(got[0, :, :3]).all()
    with np.errstate(invalid='ignore'):
        ref = _host_values(preds, labels, ace, pop.astype(np.float64), 3, 0.0)
    np.testing.assert_allclose(got[0], ref, rtol=RTOL, atol=ATOL)        # (NaN == NaN for assert_allclose)


def _coverage(lib, dev, n_items, buffer, batches, ace_d, pop_d, topn):
    rec_map = torch.full((n_items,), 9, dtype=torch.uint8, device=dev)     # the seed zeroes both maps
    clk_map = torch.full((n_items,), 9, dtype=torch.uint8, device=dev)
    buf = torch.from_numpy(buffer).to(dev)
    s = torch.cuda.current_stream().cuda_stream
    check(lib.cham_eval_coverage_seed(ptr(buf), buf.numel(), n_items, ptr(rec_map), ptr(clk_map), s), "seed")
    ws = torch.empty(lib.cham_eval_coverage_workspace_bytes(n_items), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    out, per_click = [], []
    for preds, labels, clicked in batches:
        per_click.append(_run_kernel(lib, dev, preds, labels, clicked, ace_d, pop_d, topn, 0.2, maps=(rec_map, clk_map)))
        check(lib.cham_eval_coverage_count(ptr(rec_map), ptr(clk_map), n_items, ptr(ws), ws.numel(), ptr(counts), s), "count")
        out.append(tuple(counts.cpu().tolist()))
    return out, per_click


def test_coverage_counts_are_exact(gpu):
    lib = _lib.load()
    rng = np.random.default_rng(3)
    n_items, D, topn = 1003, 40, 5
    ace_d = torch.from_numpy(rng.normal(size=(n_items, D)).astype(np.float32)).to(gpu)
    pop_d = torch.full((n_items,), 0.01, dtype=torch.float32, device=gpu)
    buffer = np.concatenate([rng.integers(1, n_items, 300), np.zeros(50, np.int64)]).astype(np.int64)
    batches = [_inputs(rng, n_items, 6, 7, 12) for _ in range(3)]
    counts, _ = _coverage(lib, gpu, n_items, buffer, batches, ace_d, pop_d, topn)
    cov = metrics.ItemCoverage(topn, buffer)
    for (preds, labels, clicked), got in zip(batches, counts):
        cov.add(preds, labels, clicked)
        assert got == (len(cov.recommended_items), len(cov.clicked_items))
    assert 0 in cov.clicked_items and 0 in cov.recommended_items


def test_coverage_and_values_past_2gb_of_rows(gpu):
    """2.2 M rows of D 250 (2.2 GB): rows past 2^31 / 1000 need 64-bit offsets; the counts cover a non-multiple-of-16 table."""
    lib = _lib.load()
    n_items, D, topn = 2_200_003, 250, 10
    g = torch.Generator(device=gpu)
    g.manual_seed(11)
    ace_d = torch.randn(n_items, D, generator=g, device=gpu, dtype=torch.float32)
    pop_d = torch.rand(n_items, generator=g, device=gpu, dtype=torch.float32).clamp_(min=1e-3)
    rng = np.random.default_rng(17)
    preds, labels, clicked = _inputs(rng, 5000, 4, 5, 20)
    far = n_items - 1 - rng.integers(0, 50_000, size=preds.shape)           # row offsets > 2^31 bytes
    preds = np.where(rng.random(preds.shape) < 0.7, far, preds).astype(np.int64)
    labels = np.where(labels != 0, np.where(rng.random(labels.shape) < 0.5, preds[..., 1], labels), 0).astype(np.int64)
    clicked[0, 0] = n_items - 1
    buffer = np.array([0, 0, 5, n_items - 2, 2_150_000], np.int64)
    counts, per_click = _coverage(lib, gpu, n_items, buffer, [(preds, labels, clicked)], ace_d, pop_d, topn)
    cov = metrics.ItemCoverage(topn, buffer)
    cov.add(preds, labels, clicked)
    assert counts[0] == (len(cov.recommended_items), len(cov.clicked_items))
    # per-click values: the host classes on the gathered rows (ids remapped into a small table)
    u = np.unique(np.concatenate([[0], preds.ravel(), labels.ravel()]))
    idx = torch.from_numpy(u).to(gpu)
    ace_h, pop_h = ace_d[idx].cpu().numpy(), pop_d[idx].cpu().numpy().astype(np.float64)
    remap = lambda a: np.searchsorted(u, a)
    ref = _host_values(remap(preds), remap(labels), ace_h, pop_h, topn, 0.2)
    np.testing.assert_allclose(per_click[0][labels != 0], ref, rtol=RTOL, atol=ATOL)
    del ace_d
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- end to end: nar_trainer_gcom.main --eval_beyond_accuracy_metrics
ARGS = ['--batch_size', '24', '--truncate_session_length', '10', '--learning_rate', '1e-3', '--reg_l2', '1e-5',
        '--softmax_temperature', '0.2', '--recent_clicks_buffer_max_size', '600', '--recent_clicks_for_normalization', '100',
        '--eval_metrics_top_n', '5', '--CAR_embedding_size', '64', '--rnn_units', '40', '--train_total_negative_samples', '7',
        '--train_negative_samples_from_buffer', '50', '--eval_total_negative_samples', '12',
        '--eval_negative_samples_from_buffer', '60', '--content_embedding_scale_factor', '6.0',
        '--training_hours_for_each_eval', '2', '--disable_eval_benchmarks', '--eval_negative_sample_relevance', '0.3']


class CaptureEval(SessionRunHook):
    """What the metrics of each eval batch are computed from: ranked ids, labels, clicked items, and the normalised popularity the
    batch is fed (read in before_run, i.e. before the batch's state update); the recent-clicks buffer at begin()."""

    def __init__(self):
        self.evals = []

    def begin(self):
        self.evals.append(dict(buffer=T.clicked_items_state.get_recent_clicks_buffer().copy(), batches=[]))

    def before_run(self, ctx):
        self._pop = np.asarray(T.clicked_items_state.get_articles_recent_pop_norm(), dtype=np.float64).copy()
        m = ctx.model
        return SessionRunArgs(fetches={'ids': m.predicted_item_ids, 'labels': m.next_item_label, 'clicked': m.item_clicked})

    def after_run(self, ctx, vals):
        r = vals.results
        self.evals[-1]['batches'].append((r['ids'].copy(), r['labels'].copy(), r['clicked'].copy(), self._pop))


def _main_with_capture(monkeypatch, argv):
    cap = CaptureEval()
    orig = Estimator.evaluate

    def evaluate(self, input_fn, steps=None, hooks=None, name=None):
        return orig(self, input_fn, steps=steps, hooks=list(hooks or []) + [cap], name=name)
    monkeypatch.setattr(Estimator, 'evaluate', evaluate)
    est = T.main(argv)
    return est, cap


def _dataset(tmp_path):
    files, csv, pkl = synthetic.write_dataset(str(tmp_path / "data"), 5, 40, 300, 16, seq_len=10, seed=5)
    return ARGS + ['--train_set_path_regex', str(tmp_path / "data" / "sessions_hour_*.tfrecord.gz"),
                   '--acr_module_articles_metadata_csv_path', csv, '--acr_module_articles_content_embeddings_pickle_path', pkl,
                   '--model_dir', str(tmp_path / "model"), '--save_results_each_n_evals', '1']


@pytest.mark.parametrize("state", ["device", "host"])
def test_trainer_reports_the_beyond_accuracy_metrics(gpu, tmp_path, monkeypatch, state):
    argv = _dataset(tmp_path) + ['--eval_beyond_accuracy_metrics', '--clicked_items_state', state]
    est, cap = _main_with_capture(monkeypatch, argv)
    log = T.eval_sessions_metrics_log
    assert len(log) == 2 == len(cap.evals)
    header = open(os.path.join(str(tmp_path / "model"), "eval_stats_benchmarks.csv")).readline().strip().split(',')
    for k in SIX:
        assert k + '_chameleon' in header and k + '_chameleon' in log[-1], k
    ace = np.asarray(est.params['content_article_embeddings_matrix'])
    ragged = 0
    for entry, ev in zip(log, cap.evals):
        ms = [metrics.HitRate(5), metrics.MRR(5)] + metrics.create_beyond_accuracy_metrics(5, 0.3, ace, ev['buffer'])
        for ids, labels, clicked, pop in ev['batches']:
            evaluation.update_metrics(ids, labels, None, pop[ids], clicked, ms, recommender='chameleon')
            ragged += int(((labels == 0).any(axis=1) & (labels != 0).any(axis=1)).any())
        host = evaluation.compute_metrics_results(ms, recommender='chameleon')
        assert entry['item_coverage_at_n_chameleon'] == host['item_coverage_at_n_chameleon']      # exact counts
        for k in SIX:
            np.testing.assert_allclose(entry[k + '_chameleon'], host[k + '_chameleon'], rtol=RTOL, atol=ATOL, err_msg=k)
        assert entry['hitrate_at_n_chameleon'] == host['hitrate_at_n_chameleon']
    assert ragged > 0, "no ragged eval batch"


def test_flag_off_keeps_the_metrics_log_keys(gpu, tmp_path):
    T.main(_dataset(tmp_path))
    log = T.eval_sessions_metrics_log
    assert len(log) == 2
    assert set(log[-1]) == {'hitrate_at_n', 'mrr_at_n', 'hitrate_at_n_chameleon', 'mrr_at_n_chameleon', 'clicks_count', 'sessions_count'}
