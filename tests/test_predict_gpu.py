"""NARModuleModel.predict_step / Estimator.predict on the GPU against the CPU oracle and the numpy model.

Bounds: 1e-3 on logits (tests/test_golden.py, tests/test_g1shape_parity_gpu.py), 4e-3 for the bf16 arm (test_g1shape_parity_gpu.py: "logits
4e-3").  The top-n list must equal the oracle's for every session whose oracle gaps (between ranks n and n + 1 and between neighbours inside
the list) exceed twice the bound; SEED was picked on the CPU, with the oracle alone, so that at most a quarter of the sessions is exempt
(`exempt_share` below recomputes it and the test asserts it)."""
import functools
import json

import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from chameleon_recsys_amd.nar.clicked_items_state import ClickedItemsState
from tests import helpers as H
from tests import predict_reference as R

ARMS = [('f32', 256), ('f32_native', 128), ('bf16', 128)]          # (gemm_dtype, CAR width): two-fp16-plane rows, native fp32 rows, bf16 rows
BOUND = {'f32': 1e-3, 'f32_native': 1e-3, 'bf16': 4e-3}
SCALE_FREE = ('f32_native', 'bf16')                                 # no content-derived operand scale: chunking cannot change a bit
SEED, N_ITEMS = 13, 1000                                           # seeds 11 and 12 exempt 2-5 of the 7 sessions, 13 at most one per arm
TOPN = {'f32': 3, 'f32_native': 3, 'bf16': 1}                       # (the bf16 bound is four times wider: gaps of 8e-3 between all of three ranks are rare)


def params(arm, C):
    return H.tiny_params(C=C, gemm_dtype=arm, batch_size=8)


@functools.lru_cache(maxsize=None)
def case(seed=SEED):
    """Host-only inputs: features of 8 sessions with 1 .. 7 clicks and one all-padding row (T = 7), the oracle's labelled twin (dummy
    non-zero labels at the valid positions), a state fed with 14 recent clicks on 10 distinct ids (4 of them clicked in the batch)."""
    p = params('f32', 128)
    scfg = p['session_features_config']
    f, _ = synthetic.make_batches(1, 8, 8, N_ITEMS, scfg, length_dist='full', seed=seed)[0]
    B, T = f['item_clicked'].shape
    assert (B, T) == (8, 7)
    lens = np.array([1, 2, 3, 4, 5, 6, 7, 0])
    valid = np.arange(T)[None, :] < lens[:, None]
    f = {k: (np.where(valid, v, np.zeros_like(v)) if np.asarray(v).shape == (B, T) else v) for k, v in f.items()}
    f_orc = dict(f, session_size=lens + 1)
    l_orc = dict(label_next_item=np.where(valid, 1, 0).astype(np.int64), label_last_item=np.ones((B, 1), np.int64))
    rng = np.random.default_rng(seed)
    ic = f['item_clicked']
    own = np.unique(ic[ic != 0])[:4]
    other = np.setdiff1d(rng.choice(np.arange(1, N_ITEMS), 12, replace=False), ic)[:6]
    ids = np.concatenate([own, other, own[:2], other[:2]])
    ts = np.full(ids.shape, int(f['event_timestamp'].max()) - 60000, np.int64) + np.arange(ids.shape[0])
    st = ClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], N_ITEMS)
    st.update_items_state(ids, ts)
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    cand = R.candidate_set(buf, N_ITEMS)
    assert cand.shape[0] == 10
    return f, f_orc, l_orc, buf, pop, cand


@functools.lru_cache(maxsize=None)
def oracle_scores(arm, C, seed=SEED):
    """Oracle logits [B, K] of every candidate as a negative sample of each session's last click (NaN row: the session without a click)."""
    from oracle.nar_oracle import NAROracle
    f, f_orc, l_orc, buf, pop, cand = case(seed)
    p = params(arm, C)
    orc = NAROracle(p, weights=H.pair_weights(p))
    B, T = f['item_clicked'].shape
    neg = np.broadcast_to(cand, (B, T, cand.shape[0])).copy()
    with torch.no_grad():
        ref = orc.forward(f_orc, l_orc, buf, pop, mode='eval', neg_items=neg)
    lg = ref['logits'].numpy()
    t_last = R.last_click(f['item_clicked'])
    out = np.full((B, cand.shape[0]), np.nan)
    for b in range(B):
        if t_last[b] >= 0:
            out[b] = lg[b, t_last[b], 1:]
    return out


def exempt_share(arm, C, seed=SEED, topn=None):
    """(exempt sessions, sessions with a click, the oracle's lists): a session is exempt when an oracle gap that decides its top-n list is
    within twice the bound."""
    topn = TOPN[arm] if topn is None else topn
    f, _, _, _, _, cand = case(seed)
    sc = oracle_scores(arm, C, seed)
    ids, s, _ = R.topn(np.nan_to_num(sc), cand, f['item_clicked'], topn + 1)
    has = R.last_click(f['item_clicked']) >= 0
    with np.errstate(invalid='ignore'):
        gaps = s[:, :-1].astype(np.float64) - s[:, 1:].astype(np.float64)      # neighbours inside the list and ranks n / n + 1
    exempt = has & ~(np.nan_to_num(gaps, nan=np.inf, posinf=np.inf) > 2 * BOUND[arm]).all(1)
    return exempt, has, ids[:, :topn]


@functools.lru_cache(maxsize=None)
def hip_model(arm, C):
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p = params(arm, C)
    rt = NARRuntime(p, seed=3, weights=H.pair_weights(p))
    ev = NARModuleModel(ModeKeys.EVAL, None, None, p['session_features_config'], p['articles_features_config'], p['batch_size'], p['lr'], 1.0,
                        p['eval_total_negative_samples'], p['eval_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                        softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                        recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                        recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                        CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], runtime=rt, gemm_dtype=arm)
    return ev, p


@functools.lru_cache(maxsize=None)
def predicted(arm, C, topn, chunk):
    ev, p = hip_model(arm, C)
    f, _, _, buf, pop, cand = case()
    ev.feed_state(pop, buf)
    out = ev.predict_step(ev.upload_predict_batch(f), topn=topn, chunk_candidates=chunk)
    out['plan_fields'] = (ev._predict_plan.P, ev._predict_plan.NC, ev._predict_plan.PC, ev._predict_plan.B, ev._predict_plan.T)
    return out


def score_matrix(out, cand):
    """[B, K] scores by candidate from a topn = K result (NaN where the candidate is not listed: excluded, or a session without a click)."""
    m = np.full((out['item_ids'].shape[0], cand.shape[0]), np.nan)
    for b in range(m.shape[0]):
        for i, s in zip(out['item_ids'][b], out['scores'][b]):
            if i != 0:
                m[b, np.searchsorted(cand, i)] = s
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("arm,C", ARMS)
def test_scores_and_lists_match_the_oracle(gpu, arm, C):
    f, _, _, buf, pop, cand = case()
    K = cand.shape[0]
    out = predicted(arm, C, K, 4)
    assert np.array_equal(out['candidates'], cand) and out['K'] == K and out['Nc'] == 4 and out['chunks'] == 3      # 4 + 4 + 2: a ragged last chunk
    # row count of a chunk's plan: one position per session with a click, 1 + Nc candidate rows each
    P, NC, PC, Bp, Tp = out['plan_fields']
    assert (P, NC, Bp, Tp) == (7, 5, 7, 1) and PC == out['P_last'] * (1 + out['Nc']) == 35
    ref = oracle_scores(arm, C)
    got = score_matrix(out, cand)
    ic = f['item_clicked']
    for b in range(ic.shape[0]):
        listed = ~np.isnan(got[b])
        want = ~np.isin(cand, ic[b][ic[b] != 0]) if (ic[b] != 0).any() else np.zeros(K, bool)
        assert np.array_equal(listed, want), (b, listed, want)                  # exactly the non-excluded candidates; none for the empty row
    err = np.nanmax(np.abs(got - ref))
    print("%s: max |score - oracle logit| %.3g (bound %g)" % (arm, err, BOUND[arm]))
    assert err < BOUND[arm]
    assert not out['item_ids'][7].any() and np.isneginf(out['scores'][7]).all() and not out['probs'][7].any()
    # ranking rule, padding and softmax: the numpy model on the HIP scores themselves
    tau = hip_model(arm, C)[1]['softmax_temperature']
    r_ids, r_sc, r_pr = R.topn(np.nan_to_num(got, nan=-np.inf), cand, ic, K, temperature=tau)
    assert np.array_equal(out['item_ids'], r_ids) and out['scores'].tobytes() == r_sc.tobytes()
    bound = R.softmax_rel_bound(K, 3, 3, 2 * float(np.nanmax(np.abs(got))) / tau)
    assert np.all(np.abs(out['probs'] - r_pr) <= bound * r_pr + 1e-45)
    # the top-n lists against the oracle's
    exempt, has, o_ids = exempt_share(arm, C)
    assert exempt.sum() * 4 <= has.sum(), "seed %d: %d of %d sessions exempt" % (SEED, exempt.sum(), has.sum())
    n = TOPN[arm]
    top = predicted(arm, C, n, 4)
    for b in np.flatnonzero(has & ~exempt):
        assert np.array_equal(top['item_ids'][b], o_ids[b]), (b, top['item_ids'][b], o_ids[b])
    assert np.array_equal(top['item_ids'], out['item_ids'][:, :n]) and top['scores'].tobytes() == out['scores'][:, :n].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("arm,C", ARMS)
def test_scores_do_not_depend_on_the_chunking(gpu, arm, C):
    cand = case()[5]
    K = cand.shape[0]
    a, b = predicted(arm, C, K, 4), predicted(arm, C, K, K)
    assert b['chunks'] == 1 and b['plan_fields'][2] == 7 * (1 + K)
    ma, mb = score_matrix(a, cand), score_matrix(b, cand)
    assert np.array_equal(np.isnan(ma), np.isnan(mb))
    err = np.nanmax(np.abs(ma - mb))
    print("%s: chunks of 4 vs one chunk: max |d score| %.3g" % (arm, err))
    assert err <= 2 * BOUND[arm]
    if arm in SCALE_FREE:
        assert np.array_equal(np.nan_to_num(ma), np.nan_to_num(mb)), err
        assert a['probs'].tobytes() != b'' and np.array_equal(a['item_ids'], b['item_ids'])


@pytest.mark.gpu
def test_consistent_with_evaluation_and_without_side_effects(gpu):
    """evaluate_step, then predict_step on the same features with the union of the batch's last-position candidates, on a device-resident
    state: shared (session, id) logits agree, each side within the bound of the oracle; the evaluation repeats bit for bit afterwards."""
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState, batch_clicks_for_state
    from chameleon_recsys_amd.nar.nar_model import NARModuleModel
    from oracle.nar_oracle import NAROracle
    arm, C = 'f32', 256
    ev, p = hip_model(arm, C)
    batches = synthetic.make_batches(3, 5, 8, N_ITEMS, p['session_features_config'], length_dist='g1', seed=29)
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], N_ITEMS)
    for f, l in batches[:2]:
        st.update_items_state(*batch_clicks_for_state(f['item_clicked'], l['label_last_item'], f['event_timestamp']))
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    f, l = batches[2]
    ev.enable_rank_histogram(3, 32)
    it0, step0 = ev._eval_iter, ev.rt.global_step
    ev.feed_state(st, st)
    ev.evaluate_step(ev.upload_batch(f, l))
    first = ev.outputs_numpy()
    first_eval = {k: v.clone() for k, v in ev._eval.items() if torch.is_tensor(v)}
    hist = [x.copy() for x in ev.rank_histogram()]
    snap = {k: getattr(st, k).clone() for k in ('buf_ids', 'buf_ts', 'recent_pop', 'articles_pop', 'pop_norm', 'n_valid')}
    flat = ev.rt.flat.clone()
    # ---- predict on the features alone
    t_last = R.last_click(f['item_clicked'])
    negs = first['neg_items']
    union = np.unique(np.concatenate([negs[b, t_last[b]] for b in range(negs.shape[0]) if t_last[b] >= 0]))
    union = union[union != 0]
    assert 10 <= union.shape[0] <= 64
    ev.feed_state(st, st)
    out = ev.predict_step(ev.upload_predict_batch({k: v for k, v in f.items() if k != 'session_size'}), topn=int(union.shape[0]),
                          candidates=union, chunk_candidates=16)
    assert np.array_equal(out['candidates'], union)
    assert all(torch.equal(getattr(st, k), v) for k, v in snap.items()) and st.n_updates == 2
    assert torch.equal(ev.rt.flat, flat) and ev.rt.global_step == step0 and ev._eval_iter == it0 + 1
    assert all(np.array_equal(a, b) for a, b in zip(hist, ev.rank_histogram()))
    with torch.no_grad():
        ref = NAROracle(p, weights=H.pair_weights(p)).forward(f, l, buf, pop, mode='eval', neg_items=negs)
    o_lg = ref['logits'].numpy()
    got = score_matrix(out, union)
    pairs = 0
    for b in range(negs.shape[0]):
        for c, nid in enumerate(negs[b, t_last[b]]):
            if nid == 0:
                continue
            e, o, q = first['logits'][b, t_last[b], 1 + c], o_lg[b, t_last[b], 1 + c], got[b, np.searchsorted(union, nid)]
            assert abs(e - o) < BOUND[arm] and abs(q - o) < BOUND[arm] and abs(e - q) < 2 * BOUND[arm], (b, nid, e, q, o)
            pairs += 1
    assert pairs >= 20
    # ---- the default candidate set of a device-resident state: the distinct ids of its buffer, built on the device
    dflt = ev.predict_step(ev.upload_predict_batch(f), topn=5)
    assert np.array_equal(dflt['candidates'], R.candidate_set(buf, N_ITEMS)) and dflt['chunks'] >= 1
    assert all(torch.equal(getattr(st, k), v) for k, v in snap.items())
    # ---- the same evaluation again: bit-identical
    ev._eval_iter = it0
    ev.feed_state(st, st)
    ev.evaluate_step(ev.upload_batch(f, l))
    second = ev.outputs_numpy()
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    for k, v in first_eval.items():
        assert torch.equal(ev._eval[k], v), k
    ev._rh = None


@pytest.mark.gpu
def test_empty_state_launches_nothing_and_covered_sessions_get_padding(gpu):
    from chameleon_recsys_amd.nar.nar_model import NARRuntime, _launch_counts
    ev, p = hip_model('f32_native', 128)
    f, _, _, buf, pop, cand = case()
    st = ClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], N_ITEMS)
    ev.feed_state(st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer())
    d = ev.upload_predict_batch(f)
    before = (_launch_counts(ev.rt.lib.cham_gemm_launch_counts), NARRuntime.plans_created)
    ev.rt.profile = []
    out = ev.predict_step(d, topn=4)
    assert ev.rt.profile == [] and (_launch_counts(ev.rt.lib.cham_gemm_launch_counts), NARRuntime.plans_created) == before
    ev.rt.profile = None
    assert out['K'] == 0 and not out['item_ids'].any() and np.isneginf(out['scores']).all() and not out['probs'].any()
    with pytest.raises(ValueError, match="recent-clicks state"):
        ev.predict_step(d, topn=4, candidates=[3, 4])
    # ... a fed state; the clicks of session 6 (7 clicks) cover every explicit candidate: its list is all padding, the others are not
    ev.feed_state(pop, buf)
    ic = f['item_clicked']
    mine = np.unique(ic[6][ic[6] != 0])
    out = ev.predict_step(ev.upload_predict_batch(f), topn=4, candidates=mine, chunk_candidates=4)
    assert not out['item_ids'][6].any() and not out['probs'][6].any()
    assert out['item_ids'][0].any() and out['K'] == mine.shape[0]
    with pytest.raises(ValueError, match=r"\[1, 1000\)"):
        ev.predict_step(ev.upload_predict_batch(f), topn=4, candidates=[5, 1000])
    with pytest.raises(ValueError, match="predict_top_n"):
        ev.predict_step(ev.upload_predict_batch(f), topn=65)


@pytest.mark.gpu
def test_through_the_trainer(gpu, tmp_path):
    """--predict_set_path_regex / --predict_output_jsonl: one JSON line per session of the matching files, the ids Estimator.predict yields."""
    from chameleon_recsys_amd.nar import datasets, nar_trainer_gcom as T
    files, csv, pkl = synthetic.write_dataset(str(tmp_path / "data"), 4, 30, 300, 16, seq_len=10, seed=5)
    out_path = str(tmp_path / "pred.jsonl")
    argv = ['--batch_size', '16', '--truncate_session_length', '10', '--recent_clicks_buffer_max_size', '600',
            '--recent_clicks_for_normalization', '100', '--CAR_embedding_size', '64', '--rnn_units', '40', '--train_total_negative_samples', '7',
            '--train_negative_samples_from_buffer', '50', '--eval_total_negative_samples', '12', '--eval_negative_samples_from_buffer', '60',
            '--training_hours_for_each_eval', '1', '--disable_eval_benchmarks', '--softmax_temperature', '0.2',
            '--train_set_path_regex', str(tmp_path / "data" / "sessions_hour_*.tfrecord.gz"),
            '--acr_module_articles_metadata_csv_path', csv, '--acr_module_articles_content_embeddings_pickle_path', pkl,
            '--model_dir', str(tmp_path / "model"), '--predict_set_path_regex', files[3], '--predict_top_n', '5',
            '--predict_output_jsonl', out_path]
    est = T.main(argv)
    lines = [json.loads(x) for x in open(out_path)]
    assert len(lines) == 30 and len({r['session_id'] for r in lines}) == 30
    scfg = T.get_session_features_config()
    again = list(est.predict(lambda: datasets.prepare_dataset_iterator(files[3], scfg, batch_size=16, truncate_session_length=10), predict_top_n=5))
    assert len(again) == 30
    for r, a in zip(lines, again):
        assert r['session_id'] == int(a['session_id'])
        assert r['item_ids'] == a['item_ids'][a['item_ids'] != 0].tolist() and 1 <= len(r['item_ids']) <= 5
        assert len(r['probs']) == len(r['scores']) == len(r['item_ids']) and all(0.0 <= x <= 1.0 for x in r['probs'])
        assert r['scores'] == sorted(r['scores'], reverse=True)
