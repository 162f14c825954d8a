"""csrc/vsknn.hip and nar/baselines.SessionRing on the device against the numpy model (tests/vsknn_reference.py), and the trainer end to
end with --eval_benchmarks v-sknn.

Expected agreement: the ring's contents and order exactly; sim and n bit-equal (the model performs the same float64 operations in the
same order); scores within 1e-12 relative (at most ~600 terms and operations at 2^-53 each: < 1e-13); scored exactly; label_rank and
pred_ids exactly against the ranking model on the device's own scores, and against the model's scores at every click whose live
candidates' model scores are pairwise further apart than that tolerance or exactly equal."""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import baselines as BL
from chameleon_recsys_amd.nar import nar_trainer_gcom as T
from chameleon_recsys_amd.nar.estimator import Estimator, SessionRunArgs, SessionRunHook
from tests import baselines_reference as R
from tests import vsknn_reference as V

pytestmark = pytest.mark.gpu
TOL = 1e-12


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int64))).to(gpu)


class Pair:
    """DeviceBaselines(['v-sknn']) and the model side by side."""

    def __init__(self, gpu, S, sample, knn, n_items):
        self.gpu, self.n_items, self.sample, self.knn = gpu, n_items, sample, knn
        self.bl = BL.DeviceBaselines(['v-sknn'], n_items, None, device=gpu, sessions_buffer_size=S, candidate_sessions_sample_size=sample,
                                     nearest_neighbor_session_for_scoring=knn)
        self.model = V.Ring(S, n_items)

    def learn(self, aci, sid):
        self.bl.learn(_dev(aci, self.gpu), _dev(sid, self.gpu))
        self.model.append(np.asarray(aci), np.asarray(sid))
        return self

    def check_ring(self):
        ring = self.bl.ring
        assert ring.export() == self.model.sessions()
        assert ring.order.cpu().numpy().tolist() == self.model.order()

    def run(self, ic, ln, neg, topn=3):
        self.bl.begin_evaluation(topn)
        b = self.bl.score_and_rank('v-sknn', _dev(ic, self.gpu), _dev(ln, self.gpu), _dev(neg, self.gpu), neighbours=True)
        B, Tn, N = np.asarray(neg).shape
        S = self.model.S
        return dict(score=b['score'].cpu().numpy().reshape(B, Tn, N + 1), scored=b['scored'].cpu().numpy().reshape(B, Tn, N + 1).astype(bool),
                    label_rank=b['label_rank'].cpu().numpy().reshape(B, Tn), pred_ids=b['pred_ids'].cpu().numpy().reshape(B, Tn, topn),
                    sim=b['sim'].cpu().numpy().reshape(B, Tn, S), n=b['n'].cpu().numpy().reshape(B, Tn, S))

    def check(self, ic, ln, neg, topn=3):
        """Runs the batch on both sides and asserts the module docstring's agreement; returns (device outputs, model details)."""
        ic, ln, neg = (np.asarray(x, np.int64) for x in (ic, ln, neg))
        self.check_ring()
        got = self.run(ic, ln, neg, topn)
        score, scored, info = V.scores(self.model, ic, ln, neg, self.sample, self.knn, details=True)
        B, Tn = ic.shape
        for b in range(B):
            for t in range(Tn):
                if (b, t) in info:
                    assert got['sim'][b, t].tobytes() == info[(b, t)]['sim'].tobytes(), (b, t)
                    assert np.array_equal(got['n'][b, t], info[(b, t)]['n']), (b, t)
                else:
                    assert not got['sim'][b, t].any() and not got['n'][b, t].any() and not got['scored'][b, t].any()
        assert np.array_equal(got['scored'], scored)
        err = np.abs(got['score'] - score)
        print("max relative score error %.3e" % (err / np.maximum(np.abs(score), 1e-300)).max())
        assert (err <= TOL * np.abs(score)).all()
        lr, pi = R.rank(got['score'], got['scored'], ln, neg, topn)
        assert np.array_equal(got['label_rank'], lr) and np.array_equal(got['pred_ids'], pi)
        lr64, pi64 = R.rank(score, scored, ln, neg, topn)
        cand = R.candidates(ln, neg)
        for b, t in zip(*np.nonzero(ln)):
            live = R.live_mask(cand[b, t], scored[b, t])
            s = score[b, t][live]
            gap = np.abs(s[:, None] - s[None, :])
            if ((gap == 0) | (gap > TOL * np.maximum(np.abs(s[:, None]), np.abs(s[None, :])))).all():
                assert got['label_rank'][b, t] == lr64[b, t] and np.array_equal(got['pred_ids'][b, t], pi64[b, t]), (b, t)
        return got, info


def _batch(rng, B, Tn, N, n_items, min_len=1):
    """Left-aligned session rows with repeats: (item_clicked, label_next, last label [B, 1], neg_ids); padded positions all zero."""
    ic, ln = np.zeros((B, Tn), np.int64), np.zeros((B, Tn), np.int64)
    neg, last = np.zeros((B, Tn, N), np.int64), np.zeros((B, 1), np.int64)
    for r in range(B):
        length = int(rng.integers(min_len, Tn + 1))
        s = rng.integers(1, n_items, size=length + 1)
        ic[r, :length], ln[r, :length], last[r, 0] = s[:-1], s[1:], s[-1]
        neg[r, :length] = rng.integers(1, n_items, size=(length, N))
    return ic, ln, last, neg


def _aci(ic, last):
    return np.concatenate([ic, last], axis=1)


def test_empty_ring_scores_nothing(gpu):
    p = Pair(gpu, 8, 5, 3, 20)
    ic, ln, last, neg = _batch(np.random.default_rng(0), 3, 4, 5, 20)
    got, _ = p.check(ic, ln, neg, topn=9)
    assert not got['scored'].any() and not got['score'].any() and not got['pred_ids'].any()
    assert (got['label_rank'][ln != 0] == 9).all() and (got['label_rank'][ln == 0] == -1).all()          # max(1 + N, topn) = 9
    got, _ = p.check(ic, ln, neg, topn=2)
    assert (got['label_rank'][ln != 0] == 6).all()


def test_wrap_around_and_small_cuts(gpu):
    """S 8 with three batches of 3 (the ninth session overwrites slot 0), then sample 5 / knn 3 over 12 item ids: both cuts fall inside a
    session's copies and inside groups of equal similarity."""
    rng = np.random.default_rng(1)
    p = Pair(gpu, 8, 5, 3, 12)
    for k in range(3):
        ic, ln, last, neg = _batch(rng, 3, 5, 4, 12, min_len=2)
        p.learn(_aci(ic, last), 100 * (k + 1) + np.arange(3))
        p.check_ring()
    assert p.bl.ring.appended == 9 and p.bl.ring.export()[-1][0] == 302 and p.bl.ring.ids.cpu().numpy()[0] == 302
    ic, ln, last, neg = _batch(rng, 7, 5, 6, 12, min_len=3)
    got, info = p.check(ic, ln, neg)
    ds = list(info.values())
    assert any(d['sampled'] and ((d['k'] > 0) & (d['k'] < d['m'])).any() for d in ds)             # the sample cut splits a session's copies
    assert any(d['cut'] and ((d['n'] > 0) & (d['n'] < d['k'])).any() for d in ds)                 # ... and so does the neighbour cut
    tie_cut = False                                                                              # the cut inside a group of equal sim:
    for d in ds:                                                                                 # one session kept, ANOTHER one cut
        kept, dropped = np.flatnonzero(d['n'] > 0), np.flatnonzero((d['k'] > 0) & (d['n'] < d['k']) & (d['sim'] < 1))
        tie_cut = tie_cut or any(d['sim'][x] == d['sim'][y] and x != y for x in kept for y in dropped)
    assert tie_cut
    assert got['scored'].any()


def test_batch_larger_than_the_ring_and_an_all_zero_row(gpu):
    rng = np.random.default_rng(2)
    p = Pair(gpu, 8, 16, 8, 15)
    ic, ln, last, neg = _batch(rng, 10, 4, 5, 15)
    aci = _aci(ic, last)
    aci[8] = 0                                                     # no valid id: still a slot
    aci[9, 1] = 15                                                 # ids outside [1, n_items) are dropped
    aci[9, 2] = -4
    p.learn(aci, 50 + np.arange(10))                               # rows 2..9 remain, row 8 in slot 0, row 9 in slot 1
    p.check_ring()
    sessions = p.bl.ring.export()
    assert len(sessions) == 8 and sessions[0][0] == 52 and sessions[-2] == (58, []) and all(0 < x < 15 for x in sessions[-1][1])
    ic2, ln2, last2, neg2 = _batch(rng, 4, 4, 5, 15, min_len=2)
    got, _ = p.check(ic2, ln2, neg2)
    assert got['scored'].any()
    p.learn(_aci(ic2, last2), np.array([7, 900, 3, 400]))          # non-ascending arrival
    got, info = p.check(ic, ln, neg)
    assert got['scored'].any()


def test_one_position_and_sixty_four(gpu):
    rng = np.random.default_rng(3)
    p = Pair(gpu, 8, 16, 8, 30)
    p.learn(np.array([[5, 6, 7], [5, 9, 0], [28, 29, 0], [6, 6, 6]]), np.arange(4) + 10)
    ic, ln, neg = np.array([[5], [6], [0]]), np.array([[6], [7], [0]]), rng.integers(1, 30, size=(3, 1, 4))
    p.check(ic, ln, neg)
    ic = np.zeros((2, 64), np.int64)
    ic[0] = 1 + (np.arange(64) % 4)                                # ids 1..4: in no buffered session ...
    ic[0, 63] = 28                                                 # ... but the last position hits {28, 29}
    ic[1, :40] = 5                                                 # a repeated id: 40 copies of two sessions, sim > 1 early on
    ln = np.where(ic != 0, 29, 0)
    neg = np.where(ic[..., None] != 0, rng.integers(10, 28, size=(2, 64, 4)), 0)
    got, info = p.check(ic, ln, neg)
    assert info[(0, 63)]['m'][2] == 1 and got['scored'][0, 63, 0] and not got['scored'][0, :63].any()
    assert got['label_rank'][0, 63] == 0 and got['sim'][0, 63, 2] == 1.0 / (np.sqrt(5.0) * np.sqrt(2.0))
    assert info[(1, 39)]['m'][0] == 40 and info[(1, 39)]['sim'][0] > 1.0 and not got['n'][1, 39].any()
    with pytest.raises(ValueError, match="64"):
        p.bl.score_and_rank('v-sknn', _dev(np.ones((1, 65)), gpu), _dev(np.ones((1, 65)), gpu), _dev(np.ones((1, 65, 2)), gpu))


def test_the_two_exclusions_on_the_device(gpu):
    p = Pair(gpu, 4, 16, 8, 20).learn(np.array([[5, 0, 0], [5, 6, 0]]), np.array([10, 11]))
    ic, ln, neg = np.array([[5, 5]]), np.array([[6, 6]]), np.array([[[5, 7], [5, 7]]])
    got, _ = p.check(ic, ln, neg)
    assert got['sim'][0, 0, 0] == 1.0 and got['n'][0, 0].tolist() == [0, 1, 0, 0]                   # sim == 1 is no neighbour
    assert got['sim'][0, 1, 0] == 1.5 and got['sim'][0, 1, 1] > 1.0 and not got['n'][0, 1].any()    # nor is sim > 1
    assert got['scored'][0].tolist() == [[True, True, False], [False, False, False]]
    assert got['pred_ids'][0, 0].tolist() == [5, 6, 0] and got['label_rank'][0].tolist() == [1, 3]


def test_seventy_candidates_with_duplicates_and_zeros(gpu):
    rng = np.random.default_rng(4)
    p = Pair(gpu, 16, 12, 6, 40)
    for k in range(2):
        ic, ln, last, neg = _batch(rng, 8, 6, 3, 40, min_len=3)
        p.learn(_aci(ic, last), 10 * k + np.arange(8))
    ic, ln, last, neg = _batch(rng, 5, 6, 69, 40, min_len=2)
    neg[:, :, 5] = 0
    neg[:, :, 7] = neg[:, :, 6]
    neg[:, :, 9] = ln
    neg[0, 0, 11] = 40 + 3                                         # ids outside the item table, beyond int32 too: never matched
    neg[0, 0, 12] = (1 << 32) + int(ic[0, 0])
    neg[ic == 0] = 0
    got, _ = p.check(ic, ln, neg, topn=64)
    assert got['scored'].any() and not got['scored'][0, 0, 12:14].any()
    for b, t in zip(*np.nonzero(ln)):
        ids = got['pred_ids'][b, t][got['pred_ids'][b, t] != 0].tolist()
        assert len(ids) == len(set(ids))


def test_full_size_ring_with_forty_sessions(gpu):
    rng = np.random.default_rng(5)
    p = Pair(gpu, 3000, 1000, 500, 60)
    for k in range(2):
        ic, ln, last, neg = _batch(rng, 20, 8, 3, 60, min_len=2)
        p.learn(_aci(ic, last), 1000 * (k + 1) + np.arange(20))
    ic, ln, last, neg = _batch(rng, 6, 8, 10, 60, min_len=2)
    got, _ = p.check(ic, ln, neg)
    assert got['scored'].any() and not got['n'][:, :, 40:].any()


def test_limits_are_refused(gpu):
    with pytest.raises(ValueError, match="4096"):
        BL.DeviceBaselines(['v-sknn'], 10, None, device=gpu, sessions_buffer_size=4097)
    p = Pair(gpu, 4, 16, 8, 20)
    one = lambda *shape: _dev(np.ones(shape), gpu)
    with pytest.raises(ValueError, match="1024"):
        p.bl.begin_evaluation(3)
        p.bl.score_and_rank('v-sknn', one(1, 2), one(1, 2), one(1, 2, 1024))
    with pytest.raises(ValueError, match="65"):
        p.bl.learn(one(1, 66), one(1))
    with pytest.raises(ValueError, match="session ids"):
        p.bl.learn(one(1, 3))
    assert BL.DeviceBaselines(['sr'], 10, None, device=gpu, table_capacity=8).ring is None        # nothing allocated without the name


def test_snapshot_restore_and_two_runs_bit_identical(gpu):
    rng = np.random.default_rng(6)
    batches = [_batch(rng, 6, 5, 6, 14, min_len=2) for _ in range(4)]
    outs = []
    for _ in range(2):
        p = Pair(gpu, 8, 6, 4, 14)
        for k in (0, 1):
            p.learn(_aci(batches[k][0], batches[k][2]), 10 * k + np.arange(6))
        before = p.bl.ring.export()
        p.bl.save_state_checkpoint()
        snap = p.model.snapshot()
        p.learn(_aci(batches[2][0], batches[2][2]), 100 + np.arange(6))
        assert p.bl.ring.export() != before
        p.bl.restore_state_checkpoint()
        p.model.restore(snap)
        assert p.bl.ring.export() == before and p.bl.ring.appended == 12
        ic, ln, last, neg = batches[3]
        got, _ = p.check(ic, ln, neg)
        outs.append(got)
    for key in outs[0]:
        assert outs[0][key].tobytes() == outs[1][key].tobytes(), key


# --------------------------------------------------------------------------------- end to end: nar_trainer_gcom.main --eval_benchmarks v-sknn
class CaptureSessions(SessionRunHook):
    """Every batch the hook saw with what 'v-sknn' was given, and the ring at begin() (after the snapshot) and at end() (after the
    restore)."""

    def __init__(self, log, mode):
        self.log, self.mode = log, mode

    def _ring(self):
        st = T.eval_benchmarks_state
        return None if st is None else (st.ring.export(), st.ring.appended)

    def begin(self):
        self.log.append(dict(mode=self.mode, batches=[], ring_begin=self._ring()))

    def before_run(self, ctx):
        m = ctx.model
        f = {'clicked': m.item_clicked, 'labels': m.next_item_label, 'last': m.label_last_item, 'sid': m.session_id}
        if self.mode == 'eval':
            f['neg'] = m.batch_negative_items
        return SessionRunArgs(fetches=f)

    def after_run(self, ctx, vals):
        self.log[-1]['batches'].append({k: np.array(v) for k, v in vals.results.items()})

    def end(self, session=None):
        self.log[-1]['ring_end'] = self._ring()


def test_trainer_reports_v_sknn(gpu, tmp_path, monkeypatch):
    from tests.test_baselines_gpu import _dataset
    log = []
    train, evaluate = Estimator.train, Estimator.evaluate
    monkeypatch.setattr(Estimator, 'train', lambda self, input_fn, hooks=None, steps=None, max_steps=None:
                        train(self, input_fn, hooks=list(hooks or []) + [CaptureSessions(log, 'train')], steps=steps, max_steps=max_steps))
    monkeypatch.setattr(Estimator, 'evaluate', lambda self, input_fn, steps=None, hooks=None, name=None:
                        evaluate(self, input_fn, steps=steps, hooks=list(hooks or []) + [CaptureSessions(log, 'eval')], name=name))
    est = T.main(_dataset(tmp_path, 'vsknn') + ['--eval_benchmarks', 'v-sknn'])
    entries = [dict(e) for e in T.eval_sessions_metrics_log]
    n_items = np.asarray(est.params['content_article_embeddings_matrix']).shape[0]
    ring = V.Ring(BL.VSKNN_SESSIONS_BUFFER_SIZE, n_items)
    evals = [ph for ph in log if ph['mode'] == 'eval']
    assert len(evals) == len(entries) == 2
    ev = iter(entries)
    scored_clicks = 0
    for phase in log:
        if phase['mode'] == 'eval':
            assert phase['ring_begin'] == (ring.sessions(), ring.appended)
            snap = ring.snapshot()
        lo_hits = hi_hits = clicks = 0
        lo_rr = hi_rr = 0.0
        for r in phase['batches']:
            if phase['mode'] == 'eval':
                score, scored = V.scores(ring, r['clicked'], r['labels'], r['neg'], BL.VSKNN_CANDIDATE_SESSIONS_SAMPLE_SIZE,
                                         BL.VSKNN_NEAREST_NEIGHBOR_SESSIONS)
                cand = R.candidates(r['labels'], r['neg'])
                for b, t in zip(*np.nonzero(r['labels'])):          # the label's rank bracket under the score tolerance
                    clicks += 1
                    live = R.live_mask(cand[b, t], scored[b, t])
                    if not live[0]:
                        continue
                    scored_clicks += 1
                    others = np.flatnonzero(live)[1:]
                    s, s0, ids = score[b, t, others], score[b, t, 0], cand[b, t, others]
                    near = (np.abs(s - s0) <= TOL * np.maximum(np.abs(s), abs(s0))) & (s != s0)
                    above = int((((s > s0) | ((s == s0) & (ids < cand[b, t, 0]))) & ~near).sum())
                    lo, hi = above, above + int(near.sum())
                    hi_hits += lo < 5
                    lo_hits += hi < 5
                    hi_rr += 1.0 / (1 + lo) if lo < 5 else 0.0
                    lo_rr += 1.0 / (1 + hi) if hi < 5 else 0.0
            ring.append(np.concatenate([r['clicked'], r['last']], axis=1), np.asarray(r['sid']).reshape(-1))
        if phase['mode'] == 'eval':
            entry = next(ev)
            assert lo_hits / clicks - 1e-12 <= entry['hitrate_at_n_v-sknn'] <= hi_hits / clicks + 1e-12
            assert lo_rr / clicks - 1e-12 <= entry['mrr_at_n_v-sknn'] <= hi_rr / clicks + 1e-12
            assert 'hitrate_at_n_by_pos_v-sknn_01' in entry and 'hitrate_at_n_chameleon' in entry
            assert ring.sessions() != phase['ring_begin'][0]
            ring.restore(snap)
        assert phase['ring_end'] == (ring.sessions(), ring.appended)    # after an evaluation: the ring before begin()
    assert scored_clicks > 50 and ring.appended > 100
