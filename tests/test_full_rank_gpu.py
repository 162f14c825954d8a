"""Full-candidate evaluation on the GPU: NARModuleModel.enable_full_candidate_ranking / evaluate_step against the CPU
oracle's bracket and, exactly, against the numpy model on the path's own scores; no side effects on the sampled evaluation; the trainer.

Batch (tests/full_rank_reference.case): B 8, T 7, 29 valid clicks, K 16 candidates.  chunk_candidates 5, block_rows 8: four chunks with
the last ragged (one column), four row blocks with the last padded (5 rows + 3).  Bounds: the arms' logit bounds of
tests/test_predict_gpu.py (1e-3, 1e-3, 4e-3); a rank may lie anywhere in [#(z_c - z_l > 2 beta), #(z_c - z_l >= -2 beta)] of the oracle's
logits and must equal the oracle's where that is one rank - at least half the clicks on the two fp32 arms (tests/test_full_rank_cpu.py);
on bf16 the bracket is rarely one rank, and exactness comes from the second test."""
import functools
import os

import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from tests import helpers as H
from tests import full_rank_reference as R

SCALE_FREE = ('f32_native', 'bf16')          # no content-derived operand scale: neither chunking nor row blocks can change a bit
TOPN = 3


@functools.lru_cache(maxsize=None)
def hip_model(arm, C):
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p = R.params(arm, C)
    rt = NARRuntime(p, seed=3, weights=H.pair_weights(p))
    ev = NARModuleModel(ModeKeys.EVAL, None, None, p['session_features_config'], p['articles_features_config'], p['batch_size'], p['lr'], 1.0,
                        p['eval_total_negative_samples'], p['eval_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                        softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                        recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                        recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                        CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], runtime=rt, gemm_dtype=arm)
    return ev, p


def _snapshot(ev):
    out = dict(sampled=ev.outputs_numpy(), eval={k: v.cpu().numpy() for k, v in ev._eval.items() if torch.is_tensor(v)},
               hist=ev.rank_histogram(), flat=ev.rt.flat.cpu().numpy().copy(), global_step=ev.rt.global_step, eval_iter=ev._eval_iter,
               loss=ev.total_loss.cpu().numpy().copy())
    return out


def _evaluate(ev, state, full, **kw):
    """One evaluate_step of the shared batch from a fresh pair of records, sampler key 0.  state: (pop_norm, buffer) arrays or a device state."""
    f, l = R.case()[:2]
    ev._fr = None
    ev.enable_rank_histogram(TOPN, 32)
    if full:
        ev.enable_full_candidate_ranking(TOPN, 32, **kw)
    ev._eval_iter = 0
    ev.feed_state(*state)
    before = ev.rt.plans_created
    ev.evaluate_step(ev.upload_batch(f, l))
    out = _snapshot(ev)
    out['plans'] = ev.rt.plans_created - before
    if full:
        out['full'], out['full_hist'] = ev.full_rank_outputs(), ev.full_rank_histogram()
    ev._fr = ev._rh = None
    return out


@functools.lru_cache(maxsize=None)
def evaluated(arm, C, chunk, block):
    ev, _ = hip_model(arm, C)
    _, _, buf, pop, _, _ = R.case()
    return _evaluate(ev, (pop, buf), True, chunk_candidates=chunk, block_rows=block, return_scores=True)


def labels():
    return np.asarray(R.case()[1]['label_next_item'], np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("arm,C", R.ARMS)
def test_ranks_lie_in_the_oracle_bracket(gpu, arm, C):
    _, _, _, _, cand, aci = R.case()
    out = evaluated(arm, C, 5, 8)['full']
    assert (out['K'], out['Nc'], out['chunks'], out['blocks']) == (16, 5, 4, 4)
    lab, rank, comp = labels(), out['label_rank'], out['competitors']
    valid = lab != 0
    assert valid.sum() == 29 and (rank[~valid] == -1).all() and (rank[valid] >= 0).all() and not comp[~valid].any()
    lo, hi = R.oracle_brackets(arm, C)
    want_comp = np.array([[R.competitors(cand, aci[b], lab[b, t]).sum() if lab[b, t] else 0 for t in range(lab.shape[1])] for b in range(lab.shape[0])])
    assert np.array_equal(comp, want_comp)
    err = np.nanmax(np.abs(np.concatenate([out['label_logit'][..., :1], out['scores']], -1) - R.oracle_logits(arm, C)))
    single = valid & (lo == hi)
    print("%s: max |logit - oracle| %.3g (bound %g); %d of %d brackets are one rank" % (arm, err, R.BOUND[arm], single.sum(), valid.sum()))
    assert err < R.BOUND[arm]
    assert ((rank >= lo) & (rank <= hi))[valid].all(), (rank, lo, hi)
    assert np.array_equal(rank[single], lo[single])


@pytest.mark.gpu
@pytest.mark.parametrize("arm,C", R.ARMS)
def test_numpy_model_on_the_paths_own_scores_gives_every_rank(gpu, arm, C):
    _, _, _, _, cand, aci = R.case()
    for chunk, block in ((5, 8), (16, 8), (5, 3)):
        out = evaluated(arm, C, chunk, block)['full']
        assert np.array_equal(out['candidates'], cand) and out['scores'].shape == (8, 7, 16) and out['label_logit'].shape == (8, 7, out['chunks'])
        valid = labels() != 0
        assert np.isfinite(out['scores'][valid]).all() and np.isnan(out['scores'][~valid]).all()
        rank, comp = R.full_ranks(out['scores'], out['label_logit'], out['Nc'], cand, aci, labels())
        assert np.array_equal(out['label_rank'], rank) and np.array_equal(out['competitors'], comp), (chunk, block)


@pytest.mark.gpu
@pytest.mark.parametrize("arm,C", R.ARMS)
def test_ranks_do_not_depend_on_chunks_and_row_blocks(gpu, arm, C):
    a, b, c = (evaluated(arm, C, ch, bl)['full'] for ch, bl in ((5, 8), (16, 8), (5, 3)))
    assert (b['chunks'], b['blocks']) == (1, 4) and (c['chunks'], c['blocks']) == (4, 10)
    assert np.array_equal(a['competitors'], b['competitors']) and np.array_equal(a['competitors'], c['competitors'])
    if arm in SCALE_FREE:
        assert np.array_equal(a['label_rank'], b['label_rank']) and np.array_equal(a['label_rank'], c['label_rank'])
        assert a['scores'].tobytes() == b['scores'].tobytes() == c['scores'].tobytes()
    else:      # a chunk's operand scale comes from the chunk's own rows: the logits move within the bound, the ranks within the bracket
        lo, hi = R.oracle_brackets(arm, C)
        valid = labels() != 0
        for o in (b, c):
            assert ((o['label_rank'] >= lo) & (o['label_rank'] <= hi))[valid].all()


@pytest.mark.gpu
@pytest.mark.parametrize("arm,C", R.ARMS[:1] + R.ARMS[2:])
def test_histogram_and_result_keys(gpu, arm, C):
    from chameleon_recsys_amd.nar import full_eval
    from chameleon_recsys_amd.nar.metrics import HitRate, MRR, NDCG, accuracy_from_rank_hist
    ev, _ = hip_model(arm, C)
    res = evaluated(arm, C, 5, 8)
    rank, (hist, pop_sum) = res['full']['label_rank'], res['full_hist']
    assert hist.shape == (32, TOPN + 1)
    for t in range(32):
        col = rank[:, t][rank[:, t] >= 0] if t < rank.shape[1] else np.zeros(0, np.int64)
        assert np.array_equal(hist[t], np.bincount(np.minimum(col, TOPN), minlength=TOPN + 1)), t
    pop = R.case()[3]
    lab = labels()
    pop32 = np.asarray(pop, np.float32)      # the fed array is float32 on the device; the record sums it in fp64
    assert np.allclose(pop_sum[:7], np.where(lab != 0, pop32[lab], np.float32(0)).astype(np.float64).sum(0), rtol=1e-12, atol=0)
    # the result keys of the hook's end(): from the record of two batches (the same batch twice: K counted twice, the rates unchanged)
    ev.enable_full_candidate_ranking(TOPN, 32, chunk_candidates=5, block_rows=8)
    f, l, buf, pop, _, _ = R.case()
    for _ in range(2):
        ev.feed_state(pop, buf)
        ev.evaluate_step(ev.upload_batch(f, l))
    got = full_eval.results(ev, by_session_position=True)
    h2 = ev.full_rank_histogram()
    ev._fr = None
    assert np.array_equal(h2[0], 2 * hist)
    acc = accuracy_from_rank_hist(hist, pop_sum, TOPN)
    r = rank[rank >= 0]
    assert got['full_candidates_mean'] == 16.0
    assert got['hitrate_at_n_chameleon_full'] == acc[HitRate.name] == (r < TOPN).mean()
    assert got['mrr_at_n_chameleon_full'] == acc[MRR.name] and abs(acc[MRR.name] - np.where(r < TOPN, 1.0 / (1.0 + r), 0.0).mean()) < 1e-12
    assert got['ndcg_at_n_chameleon_full'] == acc[NDCG.name]
    assert any(k.startswith('hitrate_at_n_by_pos_chameleon_full') for k in got), sorted(got)


@pytest.mark.gpu
def test_no_side_effects_on_the_sampled_evaluation(gpu):
    """Device-resident state (the candidate set is built on the device): the same evaluate_step with the feature off, on, and off again."""
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState, batch_clicks_for_state
    arm, C = 'f32', 256
    ev, p = hip_model(arm, C)
    batches = synthetic.make_batches(3, 8, 8, R.N_ITEMS, p['session_features_config'], length_dist='g1', seed=R.SEED)
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], R.N_ITEMS)
    for f, l in batches[:2]:
        st.update_items_state(*batch_clicks_for_state(f['item_clicked'], l['label_last_item'], f['event_timestamp']))
    snap = {k: getattr(st, k).clone() for k in ('buf_ids', 'buf_ts', 'recent_pop', 'articles_pop', 'pop_norm', 'n_valid')}
    off = _evaluate(ev, (st, st), False)
    on = _evaluate(ev, (st, st), True, chunk_candidates=5, block_rows=8)
    assert on['plans'] <= 1 and off['plans'] <= 1
    again = _evaluate(ev, (st, st), True, chunk_candidates=5, block_rows=8)
    assert again['plans'] == 0
    assert all(torch.equal(getattr(st, k), v) for k, v in snap.items()) and st.n_updates == 2
    for other in (on, again):
        for k in off['sampled']:
            assert off['sampled'][k].tobytes() == other['sampled'][k].tobytes(), k
        for k in off['eval']:
            assert off['eval'][k].tobytes() == other['eval'][k].tobytes(), k
        assert all(np.array_equal(a, b) for a, b in zip(off['hist'], other['hist']))
        assert off['flat'].tobytes() == other['flat'].tobytes() and off['loss'].tobytes() == other['loss'].tobytes()
        assert (off['global_step'], off['eval_iter']) == (other['global_step'], other['eval_iter']) == (off['global_step'], 1)
    # the device-built candidate set gives the ranks of the host-fed one, bit for bit on repetition
    host = evaluated(arm, C, 5, 8)['full']
    assert np.array_equal(on['full']['label_rank'], again['full']['label_rank']) and on['full']['K'] == host['K'] == 16
    assert np.array_equal(on['full']['competitors'], host['competitors'])


@pytest.mark.gpu
def test_empty_state_ranks_every_click_first_and_builds_no_plan(gpu):
    from chameleon_recsys_amd.nar.clicked_items_state import ClickedItemsState
    ev, p = hip_model('f32_native', 128)
    st = ClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], R.N_ITEMS)
    _evaluate(ev, (st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer()), False)
    out = _evaluate(ev, (st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer()), True)
    valid = labels() != 0
    full = out['full']
    assert out['plans'] == 0 and (full['K'], full['chunks'], full['blocks']) == (0, 0, 0)
    assert (full['label_rank'][valid] == 0).all() and (full['label_rank'][~valid] == -1).all() and not full['competitors'].any()
    assert out['full_hist'][0][:, 0].sum() == valid.sum() and not out['full_hist'][0][:, 1:].any()


@pytest.mark.gpu
def test_session_length_limit(gpu):
    ev, _ = hip_model('f32_native', 128)
    ev.enable_full_candidate_ranking(TOPN, 32)
    try:
        ev.reserve_full_candidate_ranking(127)
        assert ev._fr['t_cap'] == 127
        with pytest.raises(ValueError, match="128"):
            ev.reserve_full_candidate_ranking(128)
    finally:
        ev._fr = None


def _trainer_args(tmp_path, tag):
    files, csv, pkl = synthetic.write_dataset(str(tmp_path / "data"), 3, 30, 300, 16, seq_len=10, seed=5)
    return ['--batch_size', '16', '--truncate_session_length', '10', '--recent_clicks_buffer_max_size', '600',
            '--recent_clicks_for_normalization', '100', '--CAR_embedding_size', '64', '--rnn_units', '40', '--train_total_negative_samples', '7',
            '--train_negative_samples_from_buffer', '50', '--eval_total_negative_samples', '12', '--eval_negative_samples_from_buffer', '60',
            '--training_hours_for_each_eval', '1', '--disable_eval_benchmarks', '--softmax_temperature', '0.2', '--eval_metrics_top_n', '5',
            '--eval_metrics_by_session_position', '--save_results_each_n_evals', '1',
            '--train_set_path_regex', str(tmp_path / "data" / "sessions_hour_*.tfrecord.gz"),
            '--acr_module_articles_metadata_csv_path', csv, '--acr_module_articles_content_embeddings_pickle_path', pkl,
            '--model_dir', str(tmp_path / ("model_" + tag))]


NEW_KEYS = ('hitrate_at_n_chameleon_full', 'mrr_at_n_chameleon_full', 'ndcg_at_n_chameleon_full', 'full_candidates_mean')


@pytest.mark.gpu
@pytest.mark.parametrize("ranking", ['mlp', 'cosine'])
def test_through_the_trainer(gpu, tmp_path, ranking):
    from chameleon_recsys_amd.nar import nar_trainer_gcom as T
    head = ['--recommendations_ranking', ranking]
    T.main(_trainer_args(tmp_path, 'full') + head + ['--eval_full_candidates'])
    log = [dict(e) for e in T.eval_sessions_metrics_log]
    header = open(os.path.join(str(tmp_path / "model_full"), "eval_stats_benchmarks.csv")).readline().strip().split(',')
    assert len(log) == 2
    for e in log:
        assert all(k in e and k in header for k in NEW_KEYS), sorted(e)
        assert any(k.startswith('hitrate_at_n_by_pos_chameleon_full') for k in e)
        assert 0.0 <= e['mrr_at_n_chameleon_full'] <= e['hitrate_at_n_chameleon_full'] <= 1.0 and 12 < e['full_candidates_mean'] < 300
    if ranking == 'mlp':      # the run without the flag: none of the new keys or columns, every other number as it was
        T.main(_trainer_args(tmp_path, 'plain') + head)
        plain = T.eval_sessions_metrics_log
        plain_header = open(os.path.join(str(tmp_path / "model_plain"), "eval_stats_benchmarks.csv")).readline().strip().split(',')
        assert len(plain) == len(log) and not any('full' in k for k in plain_header)
        assert [k for k in header if 'full' not in k] == plain_header
        for a, b in zip(log, plain):
            assert not any('full' in k for k in b)
            assert {k: v for k, v in a.items() if k in b} == dict(b)
