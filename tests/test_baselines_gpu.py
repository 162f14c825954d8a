"""csrc/baselines.hip and nar/baselines.py on the device against the numpy model (tests/baselines_reference.py): the pair table
(insert, growth, rehash, export), the co-occurrence and sequential-rules inserts, scores and ranking of the four baselines, and the
trainer end to end with --eval_benchmarks.  Integer baselines are compared exactly; cb within eps = 4 (D + 8) 2^-24 of the float64
cosine (fp32 dot-product error on unit rows), its label rank exactly where the float64 gap to every competitor exceeds eps."""
import os

import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import check, ptr
from chameleon_recsys_amd.nar import baselines as BL
from chameleon_recsys_amd.nar import nar_trainer_gcom as T, synthetic
from chameleon_recsys_amd.nar.estimator import Estimator, SessionRunArgs, SessionRunHook
from tests import baselines_reference as R

pytestmark = pytest.mark.gpu


def _s():
    return torch.cuda.current_stream().cuda_stream


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _insert(table, kind, aci, n_items, gpu, max_dist=10):
    """The insert kernels on a table of FIXED capacity (no host growth rule)."""
    lib = _lib.load()
    d = _dev(np.asarray(aci, np.int64), gpu)
    B, T1 = d.shape
    if kind == 'cooc':
        check(lib.cham_pairs_insert_cooc(ptr(d), B, T1, n_items, ptr(table.keys), ptr(table.vals), table.cap, ptr(table.meta), _s()), "cooc")
    else:
        check(lib.cham_pairs_insert_sr(ptr(d), B, T1, max_dist, n_items, ptr(table.keys), ptr(table.vals), table.cap, ptr(table.meta), _s()), "sr")


def _counters(table):
    return tuple(table.meta.cpu().tolist())


# ------------------------------------------------------------------------------------------------------------------ pair table
def test_eight_slots_three_entries(gpu):
    t = BL.PairTable(gpu, capacity=8)
    _insert(t, 'sr', [[1, 2, 3]], 10, gpu)
    assert t.export() == {(1, 2): 2520, (2, 3): 2520, (1, 3): 1260} == R.learn_sr({}, [[1, 2, 3]], 10)
    assert _counters(t) == (0, 3) and t.cap == 8


def test_growth_from_eight_slots(gpu):
    """40 distinct pairs in batches of 5 sessions [a, b]: 8 -> 16 -> 32 -> ... slots by the host rule, nothing lost in a rehash."""
    t = BL.PairTable(gpu, capacity=8)
    rng = np.random.default_rng(0)
    pairs = rng.permutation(np.arange(1, 41))
    want, caps = {}, [t.cap]
    for k in range(8):
        aci = np.stack([pairs[5 * k:5 * k + 5], pairs[5 * k:5 * k + 5] % 7 + 41], axis=1)
        t.insert_sr(_dev(aci, gpu), 60)
        R.learn_sr(want, aci, 60)
        caps.append(t.cap)
        assert t.export() == want
    assert len(want) == 40 and _counters(t) == (0, 40)
    assert caps[1] == 16 and 32 in caps and caps[-1] == 128 and caps == sorted(caps)
    assert 2 * 40 <= t.cap                                       # the load the host allows


def test_half_load_of_1024_slots(gpu):
    t = BL.PairTable(gpu, capacity=1024)
    a = np.arange(1, 513)
    aci = np.stack([a, (a * 7) % 511 + 1], axis=1)
    _insert(t, 'sr', aci, 600, gpu)
    want = R.learn_sr({}, aci, 600)
    assert len(want) == 512 and t.export() == want and _counters(t) == (0, 512)


def test_keys_colliding_on_their_first_slot(gpu):
    cap = 64
    same = [(a, b) for a in range(1, 60) for b in range(1, 60) if a != b and BL.pair_slot(a, b, cap) == 5][:6]
    assert len(same) == 6
    t = BL.PairTable(gpu, capacity=cap)
    _insert(t, 'sr', np.array(same), 100, gpu)
    assert t.export() == {k: 2520 for k in same} and _counters(t) == (0, 6)
    keys = t.keys.cpu().numpy()
    assert sorted(np.flatnonzero(keys).tolist()) == list(range(5, 11))          # one probe chain from the shared first slot


def test_many_threads_one_key_and_skipped_ids(gpu):
    n_items = 50
    aci = np.array([[7, 9, 0]] * 300 + [[0, 3, n_items], [4, -1, 5], [n_items + 7, 0, 0]])
    for kind, learn in (('cooc', R.learn_cooc), ('sr', R.learn_sr)):
        t = BL.PairTable(gpu, capacity=64)
        _insert(t, kind, aci, n_items, gpu)
        want = learn({}, aci, n_items)
        got = t.export()
        assert got == want and _counters(t)[0] == 0
        assert got[(7, 9)] == (300 if kind == 'cooc' else 300 * 2520) and (4, 5) in got and all(0 < a < n_items and 0 < b < n_items for a, b in got)


def test_two_runs_export_equal_sets(gpu):
    rng = np.random.default_rng(3)
    aci = rng.integers(0, 40, size=(200, 9))
    out = []
    for _ in range(2):
        t = BL.PairTable(gpu, capacity=1 << 15)
        _insert(t, 'cooc', aci, 40, gpu)
        out.append(t.export())
    assert out[0] == out[1] == R.learn_cooc({}, aci, 40)


def test_ceiling_names_the_flag(gpu):
    t = BL.PairTable(gpu, capacity=8, max_pairs=16)
    t.insert_sr(_dev(np.array([[1, 2], [3, 4]]), gpu), 50)
    with pytest.raises(ValueError, match="--eval_benchmarks_max_pairs"):
        t.insert_sr(_dev(np.arange(1, 41).reshape(20, 2), gpu), 50)


# ---------------------------------------------------------------------------------------------------- co-occurrence / SR inserts
def _sessions(rng, B, T1, n_ids):
    aci = rng.integers(1, n_ids, size=(B, T1))
    aci[rng.random((B, T1)) < 0.3] = 0                           # zeros anywhere, the middle of a row included
    special = [[3], [3, 5], [1, 2, 1, 3], [4, 4, 4, 4], [0, 6, 0, 7]]
    for r, s in enumerate(special[:B]):
        s = s[:T1]
        aci[r] = 0
        aci[r, :len(s)] = s
    return aci


@pytest.mark.parametrize("T1", [2, 6, 21, 65])
@pytest.mark.parametrize("B", [1, 3, 65])
def test_cooccurrence_insert(gpu, B, T1):
    rng = np.random.default_rng(100 * B + T1)
    n_ids = 12 if T1 < 65 else 90                                # repeats within a session at every width
    aci = _sessions(rng, B, T1, n_ids)
    t = BL.PairTable(gpu, capacity=1 << 14)
    _insert(t, 'cooc', aci, n_ids, gpu)
    want = R.learn_cooc({}, aci, n_ids)
    assert t.export() == want and _counters(t) == (0, len(want))
    _insert(t, 'cooc', aci, n_ids, gpu)                          # a second batch adds to the same entries
    assert t.export() == {k: 2 * v for k, v in want.items()}


def test_cooccurrence_documented_example(gpu):
    t = BL.PairTable(gpu, capacity=64)
    _insert(t, 'cooc', [[1, 2, 1, 3]], 10, gpu)
    got = t.export()
    assert got[(1, 1)] == got[(1, 2)] == got[(1, 3)] == 1 and len(got) == 7


def test_sequential_rules_insert(gpu):
    """Sessions of 1, 2, 11 and 12 clicks: the window of 10 cuts in at 12; exact integer weights 2520 / distance."""
    aci = np.zeros((4, 13), np.int64)
    aci[0, 0] = 30
    aci[1, :2] = [31, 32]
    aci[2, :11] = np.arange(1, 12)
    aci[3, 1:13] = np.arange(1, 13)                              # (a leading zero: compaction)
    t = BL.PairTable(gpu, capacity=1 << 10)
    _insert(t, 'sr', aci, 40, gpu)
    got, want = t.export(), R.learn_sr({}, aci, 40)
    assert got == want and _counters(t)[0] == 0
    assert got[(1, 11)] == 2 * 252 and (1, 12) not in got and got[(2, 12)] == 252 and got[(31, 32)] == 2520 and got[(9, 12)] == 840
    assert not any(30 in k for k in got)
    t2 = BL.PairTable(gpu, capacity=1 << 10)
    _insert(t2, 'sr', aci, 40, gpu, max_dist=3)
    assert t2.export() == R.learn_sr({}, aci, 40, max_dist=3)


# ------------------------------------------------------------------------------------------------------------ scores and ranking
SHAPES = {(1, 1, 1): 5, (3, 2, 4): 5, (65, 3, 20): 64, (33, 20, 70): 250}        # (B, T, N) -> D of the cb case
N_ITEMS = 200
_CASES = {}


def _case(gpu, shape):
    """Inputs of one shape + the model's scores, built once and shared by the tests of that shape."""
    if shape in _CASES:
        return _CASES[shape]
    B, Tn, N = shape
    D = SHAPES[shape]
    rng = np.random.default_rng(B * 1000 + N)
    recent_pop = rng.integers(0, 4, size=N_ITEMS).astype(np.int32)               # small counts: ties, and zeros: unscored
    recent_pop[:100] = 0
    ace = rng.normal(size=(N_ITEMS, D)).astype(np.float32)
    ace[5] = 0.0                                                                 # a zero row
    ace[9] = ace[8]                                                              # two bit-identical rows
    ic = rng.integers(1, N_ITEMS, size=(B, Tn)).astype(np.int64)
    ln = rng.integers(1, N_ITEMS, size=(B, Tn)).astype(np.int64)
    neg = np.zeros((B, Tn, N), np.int64)
    for b in range(B):
        for t in range(Tn):
            neg[b, t] = rng.permutation(np.setdiff1d(np.arange(1, N_ITEMS), [ln[b, t]]))[:N]
    if B > 1:
        lengths = rng.integers(0, Tn + 1, size=B)
        lengths[:3] = np.maximum(lengths[:3], 1)
        lengths[0], lengths[B - 1] = Tn, Tn - 1                                  # a full row, and at least one padded position
        for b in range(B):                                                       # padded positions: item, label and negatives 0
            ic[b, lengths[b]:] = 0; ln[b, lengths[b]:] = 0; neg[b, lengths[b]:] = 0
        ln[0, 0] = 3                                                             # label unscored by pop_recent (count 0)
        neg[1, 0] = np.arange(10, 10 + N)                                        # no candidate scored by pop_recent (counts 0) ...
        ln[1, 0], ic[1, 0] = 90, 6                                               # ... nor by the tables: item 6 is in no learned session
        if N >= 4:
            neg[2, 0, :4] = [8, 9, 5, 8]                                         # identical rows, the zero row, a duplicated candidate
            neg[0, 0, 1] = ln[0, 0]                                              # a negative equal to the label
        neg[0, 0, 0] = N_ITEMS + 3                                               # ids outside the table: never an index
        recent_pop[150] = recent_pop[151] = 2                                    # equal counts, the label the larger id
        ln[0, 1], neg[0, 1, 0] = 151, 150
    sessions = np.concatenate([ic, rng.integers(1, N_ITEMS, size=(B, 1))], axis=1)
    extra = rng.integers(1, N_ITEMS, size=(40, Tn + 1))
    sessions[sessions == 6] = 7
    extra[extra == 6] = 7
    # sessions that make the tables answer for this batch's (item, candidate) pairs, equal weights included
    seeded = np.array([[ic[b, t], c] for b in range(B) for t in range(Tn) if ln[b, t] and ic[b, t] != 6 for c in neg[b, t, :3].tolist() + [ln[b, t]]][:400])
    seeded = np.clip(seeded, 0, N_ITEMS - 1)
    tables = {}
    for name, kind in (('coocurrent', 'cooc'), ('sr', 'sr')):
        tab = BL.PairTable(gpu, capacity=1 << 14)
        for aci in (sessions, extra, seeded, seeded[::2]):
            _insert(tab, kind, aci, N_ITEMS, gpu)
        assert _counters(tab)[0] == 0
        tables[name] = tab
    bl = BL.DeviceBaselines(R.NAMES, N_ITEMS, ace, device=gpu)
    bl.tables = tables
    dicts = {n: t.export() for n, t in tables.items()}
    ref = {n: R.scores(n, ic, ln, neg, N_ITEMS, recent_pop=recent_pop, ace=ace, table=dicts.get(n)) for n in R.NAMES}
    c = _CASES[shape] = dict(ic=ic, ln=ln, neg=neg, recent_pop=recent_pop, ace=ace, bl=bl, ref=ref, D=D,
                             dev=tuple(_dev(x, gpu) for x in (ic, ln, neg, recent_pop)))
    return c


def _run(c, name, topn):
    bl = c['bl']
    bl.begin_evaluation(topn)
    ic, ln, neg, pop = c['dev']
    b = bl.score_and_rank(name, ic, ln, neg, pop)
    B, Tn, N = c['neg'].shape
    return (b['score'].cpu().numpy().reshape(B, Tn, N + 1), b['scored'].cpu().numpy().reshape(B, Tn, N + 1).astype(bool),
            b['label_rank'].cpu().numpy().reshape(B, Tn), b['pred_ids'].cpu().numpy().reshape(B, Tn, topn))


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("name", ['pop_recent', 'coocurrent', 'sr'])
def test_integer_baselines_match_the_model_exactly(gpu, shape, name):
    c = _case(gpu, shape)
    want_score, want_scored = c['ref'][name]
    valid = c['ln'] != 0
    for topn in (1, 3, 64):
        score, scored, label_rank, pred_ids = _run(c, name, topn)
        assert np.array_equal(scored, want_scored) and np.array_equal(score, want_score)
        lr, pi = R.rank(want_score, want_scored, c['ln'], c['neg'], topn)
        assert np.array_equal(label_rank, lr) and np.array_equal(pred_ids, pi)
    if shape[0] > 1:                                             # the edge rows are in the batch
        NC = shape[2] + 1
        assert (label_rank[valid] == max(NC, 64)).any() and (want_scored[valid].sum(axis=-1) == 0).any() and not valid.all()
        lo, hi = R.rank_bracket(want_score, want_scored, c['ln'], c['neg'])
        assert (valid & (lo != hi)).any()                        # equal integer scores: the id rule decided


@pytest.mark.parametrize("shape", list(SHAPES))
def test_content_based_matches_the_float64_cosine(gpu, shape):
    c = _case(gpu, shape)
    D = c['D']
    eps = 4.0 * (D + 8) * 2.0 ** -24
    want_score, want_scored = c['ref']['cb']
    valid = c['ln'] != 0
    NC = shape[2] + 1
    for topn in (1, 3, 64):
        score, scored, label_rank, pred_ids = _run(c, 'cb', topn)
        assert np.array_equal(scored, want_scored)
        err = np.abs(score.astype(np.float64) - want_score)[want_scored]
        print("cb %s D %d topn %d: max |score - float64 cosine| %.3e (eps %.3e)" % (shape, D, topn, err.max(), eps))
        assert err.max() <= eps
        # the ranking kernel against the model on the device's OWN scores: exact, ties by id included
        lr, pi = R.rank(score.astype(np.float64), scored, c['ln'], c['neg'], topn)
        assert np.array_equal(label_rank, lr) and np.array_equal(pred_ids, pi)
        # the label's rank against the float64 model wherever its gap to every live competitor exceeds eps
        lr64, _ = R.rank(want_score, want_scored, c['ln'], c['neg'], topn)
        clear = np.zeros(valid.shape, bool)
        cand = R.candidates(c['ln'], c['neg'])
        for b, t in zip(*np.nonzero(valid)):
            live = R.live_mask(cand[b, t], want_scored[b, t])
            others = np.flatnonzero(live)[1:] if live[0] else np.flatnonzero(live)
            clear[b, t] = (not live[0]) or (np.abs(want_score[b, t, others] - want_score[b, t, 0]) > eps).all()
        left_out = 1.0 - clear[valid].mean()
        print("cb %s: %.2f %% of %d valid clicks left out" % (shape, 100 * left_out, valid.sum()))
        assert np.array_equal(label_rank[clear], lr64[clear])
        assert left_out <= 0.05
    if shape[0] > 2 and shape[2] >= 4:
        # bit-identical ACE rows (ids 8 and 9) in different columns: bit-identical scores, id 8 first; the zero row scores exactly 0
        row, cands = score[2, 0], cand[2, 0]
        assert row[cands == 8][0] == row[cands == 9][0]
        assert (row[cands == 5] == 0).all()
        ids = pred_ids[2, 0].tolist()
        if 8 in ids and 9 in ids:
            assert ids.index(9) == ids.index(8) + 1
        assert ids.count(8) <= 1                                  # the duplicated candidate is recommended once


def test_content_based_zero_row_as_the_current_item(gpu):
    """sklearn's convention: a zero row normalises to zero - every similarity is exactly 0, every candidate scored, ids ascending."""
    c = _case(gpu, (3, 2, 4))
    ic = c['ic'].copy()
    ic[0, 0] = 5
    bl = c['bl']
    bl.begin_evaluation(3)
    b = bl.score_and_rank('cb', _dev(ic, gpu), c['dev'][1], c['dev'][2])
    score, scored = b['score'].cpu().numpy()[0], b['scored'].cpu().numpy()[0]
    cand = R.candidates(c['ln'], c['neg'])[0, 0]
    inside = (cand >= 0) & (cand < N_ITEMS)
    assert (score == 0).all() and np.array_equal(scored.astype(bool), inside)
    live = sorted(set(cand[inside].tolist()))
    assert b['pred_ids'].cpu().numpy()[0].tolist() == live[:3] and int(b['label_rank'].cpu()[0]) == live.index(int(cand[0]))


def test_evaluate_accumulates_one_histogram_per_baseline(gpu):
    c = _case(gpu, (65, 3, 20))
    bl = c['bl']
    bl.begin_evaluation(3, t_cap=2)                               # (the record grows to the batch's T)
    ic, ln, neg, pop = c['dev']
    bl.evaluate(ic, ln, neg, pop)
    bl.evaluate(ic, ln, neg, pop)
    res = bl.results(3, by_session_position=True)
    model = R.Model(N_ITEMS, ace=c['ace'])
    model.tables = {n: t.export() for n, t in bl.tables.items()}
    for _ in range(2):
        model.evaluate(c['ic'], c['ln'], c['neg'], 3, recent_pop=c['recent_pop'])
    want = model.results()
    for n in ('pop_recent', 'coocurrent', 'sr'):
        assert res['hitrate_at_n_' + n] == want['hitrate_at_n_' + n]
        assert abs(res['mrr_at_n_' + n] - want['mrr_at_n_' + n]) < 1e-12
        assert 'hitrate_at_n_by_pos_%s_01' % n in res and 'clicks_at_pos_%s_01' % n not in res
    assert 0.0 <= res['hitrate_at_n_cb'] <= 1.0


def test_snapshot_and_restore_swap_the_tables(gpu):
    bl = BL.DeviceBaselines(['coocurrent', 'sr'], 50, None, device=gpu, table_capacity=8)
    rng = np.random.default_rng(5)
    bl.learn(_dev(rng.integers(0, 50, size=(6, 5)), gpu))
    before = {n: t.export() for n, t in bl.tables.items()}
    bl.save_state_checkpoint()
    bl.learn(_dev(rng.integers(0, 50, size=(40, 9)), gpu))        # grows and rehashes inside the "evaluation"
    assert all(len(t.export()) > len(before[n]) for n, t in bl.tables.items())
    bl.restore_state_checkpoint()
    assert {n: t.export() for n, t in bl.tables.items()} == before
    bl.check_tables()


# ------------------------------------------------------------------------------------ end to end: nar_trainer_gcom.main --eval_benchmarks
ARGS = ['--batch_size', '24', '--truncate_session_length', '10', '--learning_rate', '1e-3', '--reg_l2', '1e-5',
        '--softmax_temperature', '0.2', '--recent_clicks_buffer_max_size', '600', '--recent_clicks_for_normalization', '100',
        '--eval_metrics_top_n', '5', '--CAR_embedding_size', '64', '--rnn_units', '40', '--train_total_negative_samples', '7',
        '--train_negative_samples_from_buffer', '50', '--eval_total_negative_samples', '12',
        '--eval_negative_samples_from_buffer', '60', '--content_embedding_scale_factor', '6.0',
        '--training_hours_for_each_eval', '2', '--eval_metrics_by_session_position']
FOUR = 'pop_recent,cb,coocurrent,sr'


class CaptureBatches(SessionRunHook):
    """Every batch the hook saw, in order, with what the baselines were given: the batch's ids, in EVAL the negatives and the recent
    popularity counts before the batch's state update; the tables at begin() (after the snapshot) and at end() (after the restore)."""

    def __init__(self, log, mode):
        self.log, self.mode = log, mode

    def _tables(self):
        st = T.eval_benchmarks_state
        return None if st is None else {n: t.export() for n, t in st.tables.items()}

    def begin(self):
        self.log.append(dict(mode=self.mode, batches=[], tables_begin=self._tables()))

    def before_run(self, ctx):
        m = ctx.model
        self._pop = np.asarray(T.clicked_items_state.get_articles_recent_pop()).copy() if self.mode == 'eval' else None
        f = {'clicked': m.item_clicked, 'labels': m.next_item_label, 'last': m.label_last_item}
        if self.mode == 'eval':
            f['neg'] = m.batch_negative_items
        return SessionRunArgs(fetches=f)

    def after_run(self, ctx, vals):
        r = {k: np.array(v) for k, v in vals.results.items()}
        r['pop'] = self._pop
        self.log[-1]['batches'].append(r)

    def end(self, session=None):
        self.log[-1]['tables_end'] = self._tables()


def _main_with_capture(monkeypatch, argv):
    log = []
    train, evaluate = Estimator.train, Estimator.evaluate
    monkeypatch.setattr(Estimator, 'train', lambda self, input_fn, hooks=None, steps=None, max_steps=None:
                        train(self, input_fn, hooks=list(hooks or []) + [CaptureBatches(log, 'train')], steps=steps, max_steps=max_steps))
    monkeypatch.setattr(Estimator, 'evaluate', lambda self, input_fn, steps=None, hooks=None, name=None:
                        evaluate(self, input_fn, steps=steps, hooks=list(hooks or []) + [CaptureBatches(log, 'eval')], name=name))
    est = T.main(argv)
    return est, log


def _dataset(tmp_path, tag):
    files, csv, pkl = synthetic.write_dataset(str(tmp_path / "data"), 5, 40, 300, 16, seq_len=10, seed=5)
    return ARGS + ['--train_set_path_regex', str(tmp_path / "data" / "sessions_hour_*.tfrecord.gz"),
                   '--acr_module_articles_metadata_csv_path', csv, '--acr_module_articles_content_embeddings_pickle_path', pkl,
                   '--model_dir', str(tmp_path / ("model_" + tag)), '--save_results_each_n_evals', '1']


def _check_against_model(est, log, entries, tmp_path, tag):
    header = open(os.path.join(str(tmp_path / ("model_" + tag)), "eval_stats_benchmarks.csv")).readline().strip().split(',')
    for n in R.NAMES:
        assert 'hitrate_at_n_' + n in header and 'mrr_at_n_' + n in header, n
    assert 'hitrate_at_n_chameleon' in header and 'mrr_at_n_chameleon' in header
    ace = np.asarray(est.params['content_article_embeddings_matrix'])
    n_items = ace.shape[0]
    eps = 4.0 * (ace.shape[1] + 8) * 2.0 ** -24
    tables = {'coocurrent': {}, 'sr': {}}
    evals = [p for p in log if p['mode'] == 'eval']
    assert len(evals) == len(entries) == 2
    ev = iter(entries)
    for phase in log:
        if phase['mode'] == 'eval':
            assert phase['tables_begin'] == tables                # what training learned so far, nothing else
        model = R.Model(n_items, ace=ace)
        model.tables = {n: dict(t) for n, t in tables.items()}
        lo_hits = hi_hits = 0
        for r in phase['batches']:
            if phase['mode'] == 'eval':
                out = model.evaluate(r['clicked'], r['labels'], r['neg'], 5, recent_pop=r['pop'])
                sc, sd = out['cb']['score'], out['cb']['scored']
                # cb's bracket: a competitor within eps of the label may fall on either side in fp32
                cand = R.candidates(r['labels'], r['neg'])
                for b, t in zip(*np.nonzero(r['labels'])):
                    live = R.live_mask(cand[b, t], sd[b, t])
                    others = np.flatnonzero(live)[1:]
                    above = int((sc[b, t, others] > sc[b, t, 0] + eps).sum())
                    near = int((np.abs(sc[b, t, others] - sc[b, t, 0]) <= eps).sum())
                    hi_hits += above < 5
                    lo_hits += above + near < 5
            model.learn(np.concatenate([r['clicked'], r['last']], axis=1))
        if phase['mode'] == 'eval':
            entry, want = next(ev), model.results()
            for n in ('pop_recent', 'coocurrent', 'sr'):
                assert entry['hitrate_at_n_' + n] == want['hitrate_at_n_' + n], n
                assert abs(entry['mrr_at_n_' + n] - want['mrr_at_n_' + n]) < 1e-12, n
                assert 'hitrate_at_n_by_pos_%s_01' % n in entry
            clicks = float(model.clicks)
            assert lo_hits / clicks - 1e-12 <= entry['hitrate_at_n_cb'] <= hi_hits / clicks + 1e-12
            assert phase['tables_end'] == tables                  # the evaluation's learning is gone after the restore
            assert model.tables != tables
        else:
            tables = model.tables
            assert phase['tables_end'] == tables
    assert max(tables['coocurrent'].values()) > 1 and len(tables['sr']) > 100


@pytest.mark.parametrize("state", ["device", "host"])
def test_trainer_reports_the_four_baselines(gpu, tmp_path, monkeypatch, state):
    est, log = _main_with_capture(monkeypatch, _dataset(tmp_path, state) + ['--eval_benchmarks', FOUR, '--clicked_items_state', state])
    entries = [dict(e) for e in T.eval_sessions_metrics_log]
    _check_against_model(est, log, entries, tmp_path, state)
    if state == 'host':                                           # the model's own columns do not move when the flag is on
        T.main(_dataset(tmp_path, 'plain'))
        plain = T.eval_sessions_metrics_log
        assert T.eval_benchmarks_state is None
        assert len(plain) == len(entries)
        for a, b in zip(entries, plain):
            assert not any(k.endswith(('_pop_recent', '_cb', '_coocurrent', '_sr')) or '_sr_' in k or '_cb_' in k for k in b)
            assert {k: v for k, v in a.items() if k in b} == dict(b)
