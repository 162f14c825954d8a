"""metrics.accuracy_from_rank_hist against the host streaming classes: HitRate@n, MRR@n, NDCG@n and HitRate-by-session-position are
functions of ONE integer histogram - valid clicks by (session position, rank of the positive) - when the label occurs exactly once in
its candidate row, which the sampler guarantees (it removes every id of a session, labels included, from that session's negatives).
The histogram here is numpy's; csrc/eval_metrics.hip's is pinned against the same numpy in tests/test_rank_hist_gpu.py."""
import numpy as np
import pytest

from chameleon_recsys_amd.nar import metrics as M
from chameleon_recsys_amd.nar import parallel

B, T, NC = 37, 6, 11


def _ranked_lists(seed):
    """pred_ids [B, T, NC] with the label exactly once per valid row, labels [B, T] (0 = padding), ragged lengths, column T-1 all padded."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, T, size=B)              # 0 .. T-1 valid clicks: the last column is padded in every row
    lengths[0], lengths[1] = T - 1, 0
    labels = rng.integers(1, 500, size=(B, T)).astype(np.int64)
    labels[np.arange(T)[None, :] >= lengths[:, None]] = 0
    pred = np.zeros((B, T, NC), np.int64)
    rank = np.full((B, T), -1, np.int32)
    for b in range(B):
        for t in range(T):
            if labels[b, t] == 0:
                continue
            others = rng.choice(np.setdiff1d(np.arange(1, 600), [labels[b, t]]), NC - 1, replace=False)
            r = int(rng.integers(0, NC))
            pred[b, t] = np.insert(others, r, labels[b, t])
            rank[b, t] = r
    pop = rng.random(600)
    return pred, labels, rank, pop


def _hist(rank, labels, pop, topn, t_cap):
    hist = np.zeros((t_cap, topn + 1), np.int64)
    pop_sum = np.zeros(t_cap, np.float64)
    for t in range(rank.shape[1]):
        for b in range(rank.shape[0]):
            if rank[b, t] >= 0:
                hist[t, min(rank[b, t], topn)] += 1
                pop_sum[t] += pop[labels[b, t]]
    return hist, pop_sum


@pytest.mark.parametrize("topn", [1, 5, 10])
def test_accuracy_from_rank_hist_equals_the_streaming_classes(topn):
    halves = [_ranked_lists(seed) for seed in (3, 4)]              # two batches: the histogram accumulates, the classes stream
    host = [M.HitRate(topn), M.MRR(topn), M.NDCG(topn), M.HitRateBySessionPosition(topn)]
    hist, pop_sum = np.zeros((T + 2, topn + 1), np.int64), np.zeros(T + 2)
    for pred, labels, rank, pop in halves:
        assert ((pred == labels[..., None]).sum(-1)[labels != 0] == 1).all()
        for m in host[:3]:
            m.add(pred, labels)
        host[3].add(pred, labels, pop[labels])
        h, s = _hist(rank, labels, pop, topn, T + 2)
        hist += h
        pop_sum += s
    n_clicks = int(hist.sum())
    assert n_clicks == sum(int((l != 0).sum()) for _, l, _, _ in halves) and n_clicks > 50
    assert not hist[T - 1:].any()                                  # the all-padded column and the rows beyond T
    got = M.accuracy_from_rank_hist(hist, pop_sum, topn)
    assert set(got) == {m.name for m in host}
    rel = n_clicks * 2.0 ** -52
    assert got['hitrate_at_n'] == host[0].result()                 # a ratio of two equal integers
    for m in host[1:3]:
        want = float(m.result())
        assert abs(float(got[m.name]) - want) <= rel * abs(want), (m.name, got[m.name], want)
    hr, avg_pop, tot = host[3].result()
    g_hr, g_pop, g_tot = got['hitrate_at_n_by_pos']
    assert g_tot == tot and set(g_hr) == set(hr) == set(g_pop) == set(avg_pop) and T not in tot and max(tot) == T - 1
    assert g_hr == hr
    for k in tot:
        assert abs(g_pop[k] - avg_pop[k]) <= rel * abs(avg_pop[k]), (k, g_pop[k], avg_pop[k])


def test_rank_bins_beyond_topn_count_as_misses():
    hist = np.zeros((2, 4), np.int64)
    hist[0] = [2, 0, 1, 5]                       # topn = 3: 3 hits, 5 clicks ranked 3 or worse
    got = M.accuracy_from_rank_hist(hist, None, 3)
    assert got['hitrate_at_n'] == 3 / 8
    assert got['mrr_at_n'] == (2 + 1 / 3) / 8
    assert abs(got['ndcg_at_n'] - (2 + 1 / np.log2(4)) / 8) < 1e-15
    assert got['hitrate_at_n_by_pos'] == ({1: 3 / 8}, {1: 0.0}, {1: 8})


def test_a_shard_can_be_empty():
    assert parallel.shard_rows(1, 0, 2) == (0, 1)
    b, e = parallel.shard_rows(1, 1, 2)
    assert b == e
    for n, w in ((1, 3), (2, 3), (5, 8)):
        spans = [parallel.shard_rows(n, r, w) for r in range(w)]
        assert sum(e - b for b, e in spans) == n and sum(e == b for b, e in spans) == w - n
