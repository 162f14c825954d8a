"""cham_eval_rank_hist (csrc/eval_metrics.hip) alone against numpy: hist[t][min(r, topn)] and the fp64 popularity sums by session
position, accumulated over launches, one workgroup per position.  Shapes: one click; fewer rows than a wave; more rows than a wave;
more rows than the workgroup's 256 threads (a second stride per thread) by one and by many; topn + 1 bins within and beyond a wave."""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import ptr

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 2, 5), (65, 3, 5), (257, 20, 10), (300, 20, 64)]
N_ITEMS = 500
CANARY_I, CANARY_F = -0x0123456789ABCDEF, -12345.678
EINVAL = 22


def _inputs(B, T, topn, seed):
    """label_rank [B, T]: -1, 0, topn - 1, topn and NC - 1 all occur (where B has rows for them), one column all -1 when T > 1; labels
    with one id of n_items and one of -1 at valid positions."""
    rng = np.random.default_rng(seed)
    NC = topn + 7
    special = np.array([-1, 0, topn - 1, topn, NC - 1], np.int32)
    rank = special[rng.integers(0, 5, size=(B, T))]
    other = rng.random((B, T)) < 0.5
    rank = np.where(other, rng.integers(-1, NC, size=(B, T)), rank).astype(np.int32)
    k = min(B, 4)
    rank[:k, 0] = special[1:1 + k]                 # the four non-negative edge values, as far as column 0 has rows for them
    if T > 1:
        rank[:, T - 1] = -1
    labels = rng.integers(1, N_ITEMS, size=(B, T)).astype(np.int64)
    labels[rank < 0] = 0
    valid = np.argwhere(rank >= 0)
    if len(valid) >= 3:
        labels[tuple(valid[1])] = N_ITEMS          # outside the table: counted in hist, never read from pop_norm
        labels[tuple(valid[2])] = -1
    return rank, labels


def _reference(rank, labels, pop, topn, t_cap):
    B, T = rank.shape
    hist, pop_sum, abs_sum = np.zeros((t_cap, topn + 1), np.int64), np.zeros(t_cap), np.zeros(t_cap)
    for t in range(T):
        r = rank[:, t]
        v = r >= 0
        hist[t] = np.bincount(np.minimum(r[v], topn), minlength=topn + 1)
        ok = v & (labels[:, t] >= 0) & (labels[:, t] < len(pop))
        x = pop[labels[ok, t]].astype(np.float64)
        pop_sum[t], abs_sum[t] = x.sum(), np.abs(x).sum()
    return hist, pop_sum, abs_sum


def _launch(lib, rank_d, labels_d, topn, pop_d, hist_d, pop_sum_d, t_cap, T=None):
    B, T_ = rank_d.shape
    return lib.cham_eval_rank_hist(ptr(rank_d), ptr(labels_d), B, T_ if T is None else T, topn, ptr(pop_d), N_ITEMS, ptr(hist_d),
                                   ptr(pop_sum_d), t_cap, torch.cuda.current_stream().cuda_stream)


def _run(lib, gpu, rank, labels, pop_d, topn, t_cap, launches=2):
    """`launches` launches of the same batch into records followed by canary words; -> (hist, pop_sum) after each launch."""
    T = rank.shape[1]
    hist = torch.zeros(t_cap * (topn + 1) + 4, dtype=torch.int64, device=gpu)
    pop_sum = torch.zeros(t_cap + 4, dtype=torch.float64, device=gpu)
    hist[T * (topn + 1):] = CANARY_I                  # rows >= T and the words behind the record
    pop_sum[T:] = CANARY_F
    rank_d, labels_d = torch.from_numpy(rank).to(gpu), torch.from_numpy(labels).to(gpu)
    out = []
    for _ in range(launches):
        assert _launch(lib, rank_d, labels_d, topn, pop_d, hist, pop_sum, t_cap) == 0
        out.append((hist.cpu().numpy().copy(), pop_sum.cpu().numpy().copy()))
    return out


@pytest.mark.parametrize("B,T,topn", SHAPES)
def test_histogram_and_popularity_sums_match_numpy(gpu, B, T, topn):
    lib = _lib.load()
    rank, labels = _inputs(B, T, topn, seed=B * 1000 + T)
    if B >= 4 and T > 1:
        assert {-1, 0, topn - 1, topn, topn + 6} <= set(rank.reshape(-1).tolist())
    pop = np.random.default_rng(7).random(N_ITEMS).astype(np.float32)
    pop_d = torch.from_numpy(pop).to(gpu)
    t_cap = T + 3
    want_h, want_s, abs_s = _reference(rank, labels, pop, topn, t_cap)
    first, second = _run(lib, gpu, rank, labels, pop_d, topn, t_cap)
    n = T * (topn + 1)
    for k, (h, s) in enumerate((first, second), start=1):            # two successive launches accumulate
        assert np.array_equal(h[:n].reshape(T, topn + 1), k * want_h[:T])
        assert (h[n:] == CANARY_I).all() and (s[T:] == CANARY_F).all()          # rows >= T and the words behind both arrays
        assert (np.abs(s[:T] - k * want_s[:T]) <= B * 2.0 ** -52 * k * abs_s[:T]).all(), (s[:T], k * want_s[:T])
    assert int(first[0][:n].sum()) == int((rank >= 0).sum())
    again = _run(lib, gpu, rank, labels, pop_d, topn, t_cap)
    for (h0, s0), (h1, s1) in zip((first, second), again):            # bit-identical between two runs
        assert np.array_equal(h0, h1) and np.array_equal(s0.view(np.uint64), s1.view(np.uint64))


def test_without_pop_norm_the_sums_are_untouched(gpu):
    lib = _lib.load()
    rank, labels = _inputs(65, 3, 5, seed=1)
    (h, s), = _run(lib, gpu, rank, labels, None, 5, 4, launches=1)
    want_h, _, _ = _reference(rank, labels, np.zeros(N_ITEMS, np.float32), 5, 4)
    assert np.array_equal(h[:18].reshape(3, 6), want_h[:3]) and (h[18:] == CANARY_I).all()
    assert (s[:3] == 0.0).all() and (s[3:] == CANARY_F).all()


def test_argument_errors(gpu):
    lib = _lib.load()
    B, T, topn, t_cap = 4, 3, 5, 3
    rank = torch.zeros(B, T, dtype=torch.int32, device=gpu)
    labels = torch.ones(B, T, dtype=torch.int64, device=gpu)
    pop = torch.ones(N_ITEMS, dtype=torch.float32, device=gpu)
    hist = torch.zeros(t_cap, 257, dtype=torch.int64, device=gpu)
    pop_sum = torch.zeros(t_cap, dtype=torch.float64, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    call = lambda rank=rank, labels=labels, B=B, T=T, topn=topn, hist=hist, pop_sum=pop_sum, t_cap=t_cap: lib.cham_eval_rank_hist(
        ptr(rank), ptr(labels), B, T, topn, ptr(pop), N_ITEMS, ptr(hist), ptr(pop_sum), t_cap, s)
    for bad in (dict(rank=None), dict(labels=None), dict(hist=None), dict(pop_sum=None), dict(B=0), dict(T=0), dict(topn=0), dict(topn=257),
                dict(t_cap=T - 1)):
        assert call(**bad) == -EINVAL, bad
    torch.cuda.synchronize()
    assert not hist.any() and not pop_sum.any()                       # nothing was launched
    assert call(topn=256) == 0
    torch.cuda.synchronize()
    assert int(hist.view(-1)[:T * 257].sum()) == B * T                 # (topn 256: rows of 257 bins)
