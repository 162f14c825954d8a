#!/usr/bin/env python
"""Generates tests/golden/beyond_accuracy.npz by EXECUTING the reference's own metric classes (nar_module/nar/metrics.py:
NDCG, ItemCoverage, ExpectedRankSensitiveNovelty, ExpectedRankRelevanceSensitiveNovelty,
ContentExpectedRankRelativeSensitiveIntraListDiversity, ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity) and its
evaluation.update_metrics / compute_metrics_results, unmodified.  The only addition is a local ``np.asfarray`` shim (removed in
NumPy 2; NDCG calls it).

  CHAMELEON_REFERENCE=<reference checkout> python scripts/make_golden_beyond_accuracy.py

Cases: topn in {2, 3, 5, 10} x K in {6, 13}, relevance of the negatives 0.1 / 0.5, padded labels, id 0 and duplicate ids inside
prediction lists, an ACE row of zero norm, items at the minimum normalised popularity, a coverage seed buffer with empty (0) slots,
two batches streamed into one metric object.  Arrays only (loads without pickle).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("CHAMELEON_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))     # a checkout of the reference
OUT = os.path.join(ROOT, "tests", "golden", "beyond_accuracy.npz")

N_ITEMS, D, B, T, FOR_NORM = 40, 16, 3, 4, 50
CASES = [(topn, K) for topn in (2, 3, 5, 10) for K in (6, 13)]
KEYS = (('ndcg', 'ndcg_results'), ('esi_r', 'results'), ('esi_rr', 'results'), ('eild_r', 'results'), ('eild_rr', 'results'))


def _ref():
    if not hasattr(np, 'asfarray'):
        np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)       # NumPy 2 removed it
    sys.path.insert(0, os.path.join(REF, "nar_module"))
    from nar import evaluation, metrics                                          # noqa: E402  (reference modules, unmodified)
    return metrics, evaluation


def shared_inputs(rng):
    ace = rng.normal(size=(N_ITEMS, D)).astype(np.float32)
    ace[5] = 0.0                                                                  # zero-norm row
    counts = rng.integers(0, 6, size=N_ITEMS)
    counts[[3, 7, 11, 19]] = 0                                                   # -> the minimum normalised popularity
    pop = np.maximum(counts / (counts.sum() + 1), [1.0 / FOR_NORM])              # ClickedItemsState._update_recent_pop_norm
    buffer = np.concatenate([rng.integers(1, N_ITEMS, size=14), np.zeros(6, np.int64)]).astype(np.int64)   # 6 empty slots
    return ace, pop, buffer


def case_batches(rng, K):
    preds = np.stack([np.stack([np.stack([rng.permutation(N_ITEMS)[:K] for _ in range(T)]) for _ in range(B)]) for _ in range(2)])
    labels = rng.integers(1, N_ITEMS, size=(2, B, T))
    hit = rng.random((2, B, T)) < 0.5                                            # half of the labels inside the list
    pos = rng.integers(0, K, size=(2, B, T))
    labels = np.where(hit, np.take_along_axis(preds, pos[..., None], -1)[..., 0], labels)
    labels[:, 0, 3] = 0                                                          # padded positions
    labels[1, 2, 2:] = 0
    preds[0, 1, 0, 1] = preds[0, 1, 0, 0]                                        # duplicate ids in one list
    preds[1, 0, 1, 2] = preds[1, 0, 1, 0]
    labels[0, 1, 0] = preds[0, 1, 0, 0]                                          # ... one of them the label (counts twice in NDCG)
    preds[0, 2, 1, 1] = 0                                                        # id 0 ranked inside a list
    preds[1, 1, 3, 0] = 0
    preds[0, 0, 2, 0] = 5                                                        # the zero-norm ACE row ranked first
    clicked = rng.integers(0, N_ITEMS, size=(2, B, T))
    clicked[:, :, -1] = 0
    return preds.astype(np.int64), labels.astype(np.int64), clicked.astype(np.int64)


def main():
    metrics, evaluation = _ref()
    rng = np.random.default_rng(2024)
    ace, pop, buffer = shared_inputs(rng)
    out = dict(ace=ace, pop=pop, buffer=buffer)
    for ci, (topn, K) in enumerate(CASES):
        rel_neg = 0.1 if ci % 2 == 0 else 0.5
        preds, labels, clicked = case_batches(rng, K)
        ms = [metrics.HitRate(topn), metrics.MRR(topn), metrics.NDCG(topn),
              metrics.ItemCoverage(topn, buffer), metrics.ExpectedRankSensitiveNovelty(topn),
              metrics.ExpectedRankRelevanceSensitiveNovelty(topn, 1.0, rel_neg),
              metrics.ContentExpectedRankRelativeSensitiveIntraListDiversity(topn, ace),
              metrics.ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity(topn, ace, 1.0, rel_neg)]
        cov = []
        for bi in range(2):
            evaluation.update_metrics(preds[bi], labels[bi], pop[labels[bi]], pop[preds[bi]], clicked[bi], ms, recommender='chameleon')
            cov.append([ms[3].result(), len(ms[3].recommended_items), len(ms[3].clicked_items)])
        res = evaluation.compute_metrics_results(ms, recommender='chameleon')
        p = "c%d_" % ci
        out.update({p + 'cfg': np.array([topn, K, rel_neg], np.float64), p + 'preds': preds, p + 'labels': labels,
                    p + 'clicked': clicked, p + 'cov': np.array(cov, np.float64)})
        for (key, attr), m in zip(KEYS, [ms[2]] + ms[4:]):
            out[p + key + '_per_click'] = np.array(getattr(m, attr), np.float64)
            out[p + key + '_result'] = np.float64(m.result())
        if ci == 0:
            out['result_keys'] = np.array(sorted(res.keys()))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
