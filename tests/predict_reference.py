"""numpy model of top-n prediction, from a score matrix: candidate set, exclusion, ranking rule, padding and the
softmax over the non-excluded candidates.  float64 throughout; scores are taken as given (the caller passes the float32 values)."""
import numpy as np


def candidate_set(buffer_ids, n_items):
    """Distinct ids in [1, n_items) of the recent-clicks buffer, ascending."""
    b = np.asarray(buffer_ids, dtype=np.int64).reshape(-1)
    return np.unique(b[(b >= 1) & (b < n_items)])


def last_click(item_clicked):
    """t_b = last non-zero position of each row, -1 for a row without a click."""
    nz = np.asarray(item_clicked) != 0
    T = nz.shape[1]
    return np.where(nz.any(1), T - 1 - np.argmax(nz[:, ::-1], axis=1), -1)


def topn(scores, cand, item_clicked, n, temperature=1.0):
    """scores [B, K] of the candidates `cand` [K] (distinct ids) for each session, item_clicked [B, T] (0 = padding).
    Returns (ids int64 [B, n], scores float32 [B, n], probs float64 [B, n]): per session the non-excluded candidates - those that are not
    among the session's own clicks - by score descending, the smaller id first among equal scores, cut at n and padded with (0, -inf, 0);
    probs = softmax(score / temperature) over ALL the session's non-excluded candidates.  A session without a click: all padding."""
    scores = np.asarray(scores, dtype=np.float64)
    cand = np.asarray(cand, dtype=np.int64)
    ic = np.asarray(item_clicked, dtype=np.int64)
    B = ic.shape[0]
    ids = np.zeros((B, n), np.int64)
    sc = np.full((B, n), -np.inf, np.float32)
    pr = np.zeros((B, n), np.float64)
    t_last = last_click(ic)
    for b in range(B):
        if t_last[b] < 0 or cand.size == 0:
            continue
        keep = ~np.isin(cand, ic[b][ic[b] != 0]) & np.isfinite(scores[b])
        if not keep.any():
            continue
        c, s = cand[keep], scores[b][keep]
        z = s / temperature
        p = np.exp(z - z.max())
        p /= p.sum()
        order = np.lexsort((c, -s))[:n]          # primary: score descending; ties: id ascending
        k = order.shape[0]
        ids[b, :k], sc[b, :k], pr[b, :k] = c[order], s[order].astype(np.float32), p[order]
    return ids, sc, pr


def softmax_rel_bound(K, chunks, tiles, spread):
    """Relative error bound of the kernels' float32 probs against the float64 softmax above, in units of 1 (derivation: docstring of
    tests/test_predict_kernels_gpu.py): u = 2^-24; every exponent score / tau - m carries one rounding of the product, one of the
    difference (absolute error <= 2 u max(|score / tau|, spread) -> relative error of exp about 2 u (spread + |m|) ... bounded here by
    4 u (1 + spread)); expf itself 2 ulp = 4 u; the K-term sum in a fixed tree adds at most K u; each of the `tiles` rescales of the running
    sum (one per tile of 64 columns, `chunks` chunks) one exp (4 u + its exponent's 4 u (1 + spread)) and one multiply-add (2 u); the final
    division and the numerator's own exp the same again."""
    u = 2.0 ** -24
    per_exp = 4 * u * (1 + spread) + 4 * u
    return K * u + tiles * (per_exp + 2 * u) + 2 * per_exp + 2 * u
