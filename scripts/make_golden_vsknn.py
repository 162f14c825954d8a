#!/usr/bin/env python
"""Generates tests/golden/vsknn.npz by EXECUTING the reference's own SessionBasedKNNRecommender (nar_module/nar/benchmarks/session_knn.py),
unmodified, in the trainers' V-SkNN configuration (cosine, 'div' decay, 'recent' sampling) with shrunk sizes, over its own
ClickedItemsState and in the order of the reference's hook (nar_model.py:1607-1650): evaluate (EVAL), then train; snapshot / restore
around an evaluation; the recommender rebuilt per train / evaluate phase as the hook is.

  CHAMELEON_REFERENCE=<reference checkout> python scripts/make_golden_vsknn.py

The reference is imported at generation time only (stubs for its unused imports: scripts/make_golden_baselines.py).  The stream is that
script's recipe: 8 batches of B=8 sessions, T=6 click positions, N=8 negatives over 30 item ids with a skewed popularity (repeated ids
within a session occur), session ids 1000 (k + 1) + row (ascending, as the reference's lookup assumes): TRAIN 0-2, EVAL 3-4 (snapshot,
restore), TRAIN 5, EVAL 6-7 (snapshot, restore).  Buffer 24 sessions, sample 16, 8 neighbours: both cuts are at work.
Stored: the inputs, the recommender's full ranking (predict with topk = 1 + N) and the rank of the label in it per eval batch, and the
sessions buffer (ids, 0-padded sorted item rows) inside each evaluation, after its restore and after each training phase.  Arrays only."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden_baselines import PHASES, ROOT, _ref, label_rank_of, make_stream            # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vsknn.npz")
N_ITEMS, B, T, N = 30, 8, 6, 8
BUFFER, SAMPLE, KNN = 24, 16, 8
PARAMS = {'sessions_buffer_size': BUFFER, 'candidate_sessions_sample_size': SAMPLE, 'sampling_strategy': 'recent',
          'nearest_neighbor_session_for_scoring': KNN, 'similarity': 'cosine', 'first_session_clicks_decay': 'div'}


def buffer_of(state):
    buf = state.benchmarks_states.get('v-sknn', {'last_sessions_buffer': []})['last_sessions_buffer']
    ids = np.array([s.session_id for s in buf], np.int64)
    items = np.zeros((len(buf), T + 1), np.int64)
    for r, s in enumerate(buf):
        row = sorted(int(x) for x in s.item_ids)
        items[r, :len(row)] = row
    return dict(ids=ids, items=items)


def main():
    benchmarks, cis, metrics = _ref()
    rng = np.random.default_rng(7)
    stream = make_stream(rng, 8, n_items=N_ITEMS, b=B, t=T, n=N)
    state = cis.ClickedItemsState(1.0, 120, 120, N_ITEMS)
    out = dict(n_items=np.int64(N_ITEMS), buffer_size=np.int64(BUFFER), sample_size=np.int64(SAMPLE), neighbours=np.int64(KNN),
               phases=np.array([[0 if m == 'train' else 1, ids[0], ids[-1]] for m, ids in PHASES], np.int64))
    for k, (ic, ln, last, neg, ts) in enumerate(stream):
        out.update({'b%d_item_clicked' % k: ic, 'b%d_label_next' % k: ln, 'b%d_last_label' % k: last, 'b%d_neg_ids' % k: neg,
                    'b%d_session_id' % k: 1000 * (k + 1) + np.arange(B, dtype=np.int64)})
    for pi, (mode, ids) in enumerate(PHASES):
        clf = benchmarks.SessionBasedKNNRecommender(state, dict(PARAMS), [metrics.HitRate(3), metrics.MRR(3)])     # a new hook per phase
        assert clf.get_clf_suffix() == 'v-sknn'
        if mode == 'eval':
            state.save_state_checkpoint()
        for k in ids:
            ic, ln, last, neg, ts = stream[k]
            if mode == 'eval':
                preds = clf.predict(None, ic, topk=N + 1, valid_items=np.concatenate([ln[..., None], neg], axis=2))
                out['b%d_preds' % k] = preds
                out['b%d_label_rank' % k] = label_rank_of(preds, ln)
            clf.train(None, out['b%d_session_id' % k], ic, ln)
        if mode == 'eval':
            for key, v in buffer_of(state).items():
                out['p%d_inside_%s' % (pi, key)] = v
            state.restore_state_checkpoint()
        for key, v in buffer_of(state).items():
            out['p%d_after_%s' % (pi, key)] = v
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
