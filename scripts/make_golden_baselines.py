#!/usr/bin/env python
"""Generates tests/golden/baselines.npz by EXECUTING the reference's own baseline recommenders (nar_module/nar/benchmarks:
RecentlyPopularRecommender, ContentBasedRecommender, ItemCooccurrenceRecommender, SequentialRulesRecommender), unmodified, over its own
ClickedItemsState, in the order of the reference's hook (nar_model.py:1607-1650): evaluate (EVAL), train, state update, co-occurrence
update; snapshot / restore around an evaluation; the recommenders rebuilt per train / evaluate phase as the hook is.

  CHAMELEON_REFERENCE=<reference checkout> python scripts/make_golden_baselines.py            # writes the fixture
  CHAMELEON_REFERENCE=<reference checkout> python scripts/make_golden_baselines.py --time_g1  # times the four classes on one G1-shaped batch

benchmarks.py and utils.py import TensorFlow (and utils.py ua_parser) without using them on this path: empty stub modules of this
script's own stand in for them.  The stream: 8 batches of B=8 sessions, T=5 click positions, N=6 negatives over 60 item ids with a
skewed popularity (repeated ids within a session occur): TRAIN 0-2, EVAL 3-4 (snapshot, restore), TRAIN 5, EVAL 6-7 (snapshot, restore).
Stored: the inputs, each recommender's full ranking (predict with topk = 1 + N) and the rank of the label in it, its streaming
HitRate@3 / MRR@3 after every eval batch, the recent-clicks buffer each eval batch saw, and the learned maps after batch 4 (inside the
first evaluation), after its restore, and at the end.  Arrays only (loads without pickle)."""
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CHAMELEON_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))     # a checkout of the reference
OUT = os.path.join(ROOT, "tests", "golden", "baselines.npz")

N_ITEMS, D, B, T, N, TOPN = 60, 12, 8, 5, 6, 3
PHASES = (('train', (0, 1, 2)), ('eval', (3, 4)), ('train', (5,)), ('eval', (6, 7)))
NAMES = ('pop_recent', 'cb', 'coocurrent', 'sr')


def _ref():
    for name in ('tensorflow', 'ua_parser', 'ua_parser.user_agent_parser', 'pytz'):
        try:
            __import__(name)
        except ImportError:
            sys.modules[name] = types.ModuleType(name)                            # imported by the reference, unused on this path
    if 'ua_parser' in sys.modules and not hasattr(sys.modules['ua_parser'], 'user_agent_parser'):
        sys.modules['ua_parser'].user_agent_parser = sys.modules.get('ua_parser.user_agent_parser')
    sys.path.insert(0, os.path.join(REF, "nar_module"))
    from nar import benchmarks, clicked_items_state, metrics                       # noqa: E402  (reference modules, unmodified)
    return benchmarks, clicked_items_state, metrics


def make_stream(rng, n_batches, n_items=N_ITEMS, b=B, t=T, n=N, min_len=2):
    """Batches of sessions with a skewed item popularity: (item_clicked [b, t], label_next [b, t], last_label [b, 1], neg_ids [b, t, n],
    timestamps [b, t])."""
    p = 1.0 / np.arange(1, n_items) ** 0.8
    p /= p.sum()
    out = []
    for k in range(n_batches):
        ic = np.zeros((b, t), np.int64); ln = np.zeros((b, t), np.int64); neg = np.zeros((b, t, n), np.int64)
        ts = np.zeros((b, t), np.int64); last = np.zeros((b, 1), np.int64)
        for r in range(b):
            length = int(rng.integers(min_len, t + 2))                             # clicks of the session, the last label included
            s = rng.choice(np.arange(1, n_items), size=length, p=p)                # with replacement: an id may repeat
            ic[r, :length - 1], ln[r, :length - 1], last[r, 0] = s[:-1], s[1:], s[-1]
            ts[r, :length - 1] = 1_500_000_000_000 + 60_000 * k + 1000 * np.arange(length - 1)
            others = np.setdiff1d(np.arange(1, n_items), s)
            for c in range(length - 1):
                neg[r, c] = rng.permutation(others)[:n]
        out.append((ic, ln, last, neg, ts))
    return out


def build_recommenders(benchmarks, metrics, state, ace, topn):
    mk = lambda: [metrics.HitRate(topn), metrics.MRR(topn)]
    return [benchmarks.RecentlyPopularRecommender(state, {}, mk()),
            benchmarks.ContentBasedRecommender(state, {'articles_metadata': {}, 'content_article_embeddings_matrix': ace}, mk()),
            benchmarks.ItemCooccurrenceRecommender(state, {}, mk()),
            benchmarks.SequentialRulesRecommender(state, {'max_clicks_dist': 10, 'dist_between_clicks_decay': 'div'}, mk())]


def learn_batch(clfs, state, batch):
    """The reference hook's after_run behind the evaluation (nar_model.py:1627-1650)."""
    ic, ln, last, neg, ts = batch
    for clf in clfs:
        clf.train(None, None, ic, ln)
    items = np.concatenate([ic, last], axis=1)
    flat = items.reshape(-1)
    stamps = np.concatenate([ts, ts.max(axis=1).reshape(-1, 1)], axis=1).reshape(-1)
    state.update_items_state(flat[np.nonzero(flat)], stamps[np.nonzero(flat)])
    state.update_items_coocurrences(items)


def maps_of(state):
    c = state.items_coocurrences.tocoo()
    keep = c.data != 0
    rules = state.benchmarks_states.get('sr', {'rules': {}})['rules']
    sr = [(a, b, w) for a, row in rules.items() for b, w in row.items()]
    return dict(cooc_rows=c.row[keep].astype(np.int64), cooc_cols=c.col[keep].astype(np.int64), cooc_vals=c.data[keep].astype(np.int64),
                sr_a=np.array([x[0] for x in sr], np.int64), sr_b=np.array([x[1] for x in sr], np.int64),
                sr_w=np.array([x[2] for x in sr], np.float64))


def label_rank_of(preds, ln):
    """Position of the label in a recommender's full ranking of the candidates; 1 + N when it is not recommended; -1 at padding."""
    rank = np.full(ln.shape, -1, np.int64)
    for b, t in zip(*np.nonzero(ln)):
        at = np.flatnonzero(preds[b, t] == ln[b, t])
        rank[b, t] = int(at[0]) if len(at) else preds.shape[2]
    return rank


def main():
    benchmarks, cis, metrics = _ref()
    rng = np.random.default_rng(7)
    ace = rng.normal(size=(N_ITEMS, D)).astype(np.float32)
    ace[11] = 0.0                                                                  # a zero row
    ace[23] = ace[17]                                                              # two bit-identical rows
    stream = make_stream(rng, 8)
    state = cis.ClickedItemsState(1.0, 120, 120, N_ITEMS)
    out = dict(ace=ace, topn=np.int64(TOPN), n_items=np.int64(N_ITEMS),
               phases=np.array([[0 if m == 'train' else 1, ids[0], ids[-1]] for m, ids in PHASES], np.int64))
    for k, (ic, ln, last, neg, ts) in enumerate(stream):
        out.update({'b%d_item_clicked' % k: ic, 'b%d_label_next' % k: ln, 'b%d_last_label' % k: last, 'b%d_neg_ids' % k: neg,
                    'b%d_timestamps' % k: ts})
    for pi, (mode, ids) in enumerate(PHASES):
        clfs = build_recommenders(benchmarks, metrics, state, ace, TOPN)          # a new hook per train / evaluate call
        if mode == 'eval':
            state.save_state_checkpoint()
            for clf in clfs:
                clf.reset_eval_metrics()
        for k in ids:
            ic, ln, last, neg, ts = stream[k]
            if mode == 'eval':
                out['b%d_buffer' % k] = np.array(state.get_recent_clicks_buffer(), np.int64)
                valid = np.concatenate([ln[..., None], neg], axis=2)
                for clf in clfs:
                    name = clf.get_clf_suffix()
                    preds = clf.predict(None, ic, topk=N + 1, valid_items=valid)
                    res = clf.evaluate(None, ic, ln, topk=TOPN, eval_negative_items=neg)
                    out['b%d_%s_preds' % (k, name)] = preds
                    out['b%d_%s_label_rank' % (k, name)] = label_rank_of(preds, ln)
                    out['b%d_%s_metrics' % (k, name)] = np.array([res['hitrate_at_n_' + name], res['mrr_at_n_' + name]], np.float64)
            learn_batch(clfs, state, stream[k])
        if mode == 'eval':
            for key, v in maps_of(state).items():
                out['p%d_inside_%s' % (pi, key)] = v
            state.restore_state_checkpoint()
        for key, v in maps_of(state).items():
            out['p%d_after_%s' % (pi, key)] = v
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


def time_g1(batches=3):
    """Seconds per eval batch of the reference's four classes at the G1 eval shape (B 256, T 20, 1 + N = 51, D 250, topn 10) on this
    host's CPU, after `batches` G1-shaped batches were learned."""
    benchmarks, cis, metrics = _ref()
    rng = np.random.default_rng(11)
    n_items, d, b, t, n, topn = 5000, 250, 256, 20, 50, 10
    ace = rng.normal(size=(n_items, d)).astype(np.float32)
    stream = make_stream(rng, batches + 1, n_items=n_items, b=b, t=t, n=n)
    state = cis.ClickedItemsState(1.0, 5000, 5000, n_items)
    clfs = build_recommenders(benchmarks, metrics, state, ace, topn)
    for k in range(batches):
        learn_batch(clfs, state, stream[k])
    ic, ln, last, neg, ts = stream[batches]
    total = 0.0
    for clf in clfs:
        t0 = time.perf_counter()
        clf.evaluate(None, ic, ln, topk=topn, eval_negative_items=neg)
        dt = time.perf_counter() - t0
        total += dt
        print("%-12s evaluate %.3f s" % (clf.get_clf_suffix(), dt))
    t0 = time.perf_counter()
    learn_batch(clfs, state, stream[batches])
    print("learn (train x4 + state + co-occurrences) %.3f s" % (time.perf_counter() - t0))
    print("four baselines, one eval batch: %.3f s" % total)


if __name__ == "__main__":
    time_g1() if "--time_g1" in sys.argv else main()
