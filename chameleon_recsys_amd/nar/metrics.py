"""Streaming metrics of the NAR evaluation path: HitRate@N, MRR@N, NDCG@N and the beyond-accuracy metrics (item coverage,
rank-sensitive novelty ESI-R / ESI-RR, content intra-list diversity EILD-R / EILD-RR).

Same classes / method names / results as nar_module/nar/metrics.py of the reference (StreamingMetric, MRR :23-66, NDCG :69-106,
HitRate :109-134, ExpectedRankSensitiveNovelty :226-266, ExpectedRankRelevanceSensitiveNovelty :269-314, ItemCoverage :317-343,
ContentExpectedRankRelativeSensitiveIntraListDiversity :513-569, ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity
:573-641), vectorised over the [B, T, K] prediction tensor instead of the reference's Python double loop.  ``predictions[b, t]`` =
item ids ranked by predicted probability (nar_model.py:777-794), ``labels[b, t]`` = next clicked item (0 = padding, skipped).
Pinned against the reference classes: tests/golden/metrics_hitrate_mrr.npz, tests/golden/beyond_accuracy.npz.

The novelty and diversity metrics also accept per-click values computed on the GPU (``add_values``, csrc/eval_metrics.hip), and
ItemCoverage the two set sizes counted there (``add_counts``); ``result()`` is the same fp64 mean / ratio either way.
"""
import numpy as np


class StreamingMetric:
    name = 'undefined'

    def __init__(self, topn):
        self.topn = topn
        self.reset()

    def reset(self):
        pass

    def add(self, predictions, labels):
        pass

    def result(self):
        pass


def _first_hit_rank(predictions, labels, topn):
    """rank (0-based) of the first position within the top-n where prediction == label, -1 if none; valid = label != 0."""
    predictions = np.asarray(predictions)[..., :topn]
    labels = np.asarray(labels)
    hit = predictions == labels[..., None]
    any_hit = hit.any(axis=-1)
    rank = np.where(any_hit, hit.argmax(axis=-1), -1)
    return rank, labels != 0


class HitRate(StreamingMetric):
    name = 'hitrate_at_n'

    def reset(self):
        self.hitrate_total = 0
        self.hitrate_matches = 0

    def add(self, predictions, labels):
        rank, valid = _first_hit_rank(predictions, labels, self.topn)
        self.hitrate_total += int(valid.sum())
        self.hitrate_matches += int(((rank >= 0) & valid).sum())

    def result(self):
        return self.hitrate_matches / float(self.hitrate_total)


class MRR(StreamingMetric):
    name = 'mrr_at_n'

    def reset(self):
        self.mrr_results = []

    def add(self, predictions, labels):
        rank, valid = _first_hit_rank(predictions, labels, self.topn)
        rr = np.where(rank >= 0, 1.0 / (1.0 + np.maximum(rank, 0)), 0.0)
        self.mrr_results.extend(rr[valid].tolist())       # row-major == the reference's loop order

    def result(self):
        return np.mean(self.mrr_results)


class HitRateBySessionPosition(StreamingMetric):
    """HitRate@N per session position (nar_module/nar/metrics.py:136-168): key = 1-based click column; also the average recent
    normalised popularity of the labels at that position and the number of clicks counted there."""
    name = 'hitrate_at_n_by_pos'

    def reset(self):
        self.hitrate_matches_by_session_pos = {}
        self.hitrate_total_by_session_pos = {}
        self.norm_pop_by_pos = {}

    def add(self, predictions, labels, labels_norm_pop):
        rank, valid = _first_hit_rank(predictions, labels, self.topn)
        labels_norm_pop = np.asarray(labels_norm_pop, dtype=np.float64)
        for col in np.flatnonzero(valid.any(axis=0)):
            v = valid[:, col]
            key = int(col) + 1
            self.hitrate_total_by_session_pos[key] = self.hitrate_total_by_session_pos.get(key, 0) + int(v.sum())
            self.norm_pop_by_pos[key] = self.norm_pop_by_pos.get(key, 0) + float(labels_norm_pop[:, col][v].sum())
            hits = int(((rank[:, col] >= 0) & v).sum())
            if hits:
                self.hitrate_matches_by_session_pos[key] = self.hitrate_matches_by_session_pos.get(key, 0) + hits

    def result(self):
        tot = self.hitrate_total_by_session_pos
        hitrate = {k: self.hitrate_matches_by_session_pos.get(k, 0) / float(tot[k]) for k in tot}
        avg_pop = {k: self.norm_pop_by_pos.get(k, 0) / float(tot[k]) for k in tot}
        return hitrate, avg_pop, tot


def _log_rank_discount(k):
    """1 / log2(k + 2) for 0-based ranks k (the reference's log_rank_discount), elementwise, fp64."""
    return 1.0 / np.log2(np.asarray(k, dtype=np.float64) + 2.0)


class NDCG(StreamingMetric):
    """The label is compared with the WHOLE prediction row to build the ideal DCG (a label listed twice counts twice); the
    DCG itself is over the first topn positions (gains 2^r - 1 = r for binary relevance)."""
    name = 'ndcg_at_n'

    def reset(self):
        self.ndcg_results = []

    def add(self, predictions, labels):
        predictions, labels = np.asarray(predictions), np.asarray(labels)
        valid = labels != 0
        hit = (predictions == labels[..., None])[valid]                      # [V, K], row-major == the reference's loop order
        k = min(self.topn, hit.shape[-1])
        disc = _log_rank_discount(np.arange(k))
        dcg = (hit[:, :k] * disc).sum(axis=-1)
        ideal = np.concatenate([[0.0], np.cumsum(disc)])[np.minimum(hit.sum(axis=-1), k)]
        with np.errstate(invalid='ignore', divide='ignore'):
            ndcg = np.where(ideal > 0, dcg / np.where(ideal > 0, ideal, 1.0), 0.0)
        self.ndcg_results.extend(ndcg.tolist())

    def result(self):
        return np.mean(self.ndcg_results)


def accuracy_from_rank_hist(hist, pop_sum, topn):
    """HitRate@n, MRR@n, NDCG@n and HitRate-by-session-position from the rank histogram of cham_eval_rank_hist: ``hist[t, r]`` =
    valid clicks at session position t whose positive ranked r (0-based; ranks >= topn share bin ``topn``), ``pop_sum[t]`` = fp64 sum
    of the labels' recent normalised popularity at t (or None).  Same keys and result shapes as the streaming classes above, all
    arithmetic fp64.  Equal to them because the sampler removes every id of a session, its labels included, from that session's
    negatives: the label occurs exactly once in its candidate row, so its rank decides every one of these metrics (the ideal DCG of
    a single relevant item is 1)."""
    hist = np.asarray(hist, dtype=np.int64)[:, :topn + 1]
    by_rank = hist.sum(axis=0)
    total = int(by_rank.sum())
    ranks = np.arange(topn, dtype=np.float64)
    top = by_rank[:topn].astype(np.float64)
    per_pos = hist.sum(axis=1)
    hits_pos = hist[:, :topn].sum(axis=1)
    pop = np.zeros(hist.shape[0], np.float64) if pop_sum is None else np.asarray(pop_sum, dtype=np.float64)
    cols = [int(t) for t in np.flatnonzero(per_pos)]
    tot = {t + 1: int(per_pos[t]) for t in cols}
    hitrate = {t + 1: int(hits_pos[t]) / float(per_pos[t]) for t in cols}
    avg_pop = {t + 1: float(pop[t]) / float(per_pos[t]) for t in cols}
    with np.errstate(invalid='ignore', divide='ignore'):
        return {HitRate.name: int(by_rank[:topn].sum()) / float(total) if total else float('nan'),
                MRR.name: (top / (ranks + 1.0)).sum() / np.float64(total),
                NDCG.name: (top * _log_rank_discount(ranks)).sum() / np.float64(total),
                HitRateBySessionPosition.name: (hitrate, avg_pop, tot)}


class ItemCoverage(StreamingMetric):
    """|recommended items| / |clicked items|.  The clicked set is seeded with the recent-clicks buffer given at construction (a 0
    included while the buffer has empty slots), then grows by the non-zero labels and clicked items of each batch; the
    recommended set holds the top-n ids of the valid clicks (id 0 included if it is ranked there).
    ``add_counts`` takes the two set sizes from the device-side maps instead (they are cumulative: the last call wins)."""
    name = 'item_coverage_at_n'

    def __init__(self, topn, recent_clicks_buffer):
        self.recent_clicks_buffer = recent_clicks_buffer
        super().__init__(topn)

    def reset(self):
        self.clicked_items = set(np.asarray(self.recent_clicks_buffer).reshape(-1).tolist())
        self.recommended_items = set()
        self.counts = None

    def add(self, predictions, labels, clicked_items):
        predictions, labels, clicked_items = np.asarray(predictions), np.asarray(labels), np.asarray(clicked_items)
        self.recommended_items.update(np.unique(predictions[..., :self.topn][labels != 0]).tolist())
        self.clicked_items.update(np.unique(labels[labels != 0]).tolist())
        self.clicked_items.update(np.unique(clicked_items[clicked_items != 0]).tolist())

    def add_counts(self, recommended_count, clicked_count):
        self.counts = (int(recommended_count), int(clicked_count))

    def result(self):
        rec, clk = self.counts if self.counts is not None else (len(self.recommended_items), len(self.clicked_items))
        return rec / float(clk)


class _PerClickMean(StreamingMetric):
    """Mean over the valid clicks of a per-click value (fp64 on the host).  topn < 2 is rejected: the reference divides by a sum
    over ranks [0, n - 1), which is empty for n = 1."""

    def __init__(self, topn):
        if topn < 2:
            raise ValueError("%s needs eval_metrics_top_n >= 2 (got %d)" % (self.name, topn))
        super().__init__(topn)

    def reset(self):
        self.results = []

    def add_values(self, values):
        """Per-click values of the VALID clicks, in row-major click order (e.g. from cham_eval_beyond_accuracy)."""
        self.results.extend(np.asarray(values, dtype=np.float64).reshape(-1).tolist())

    def result(self):
        return np.mean(self.results)

    def _top(self, predictions, labels):
        predictions, labels = np.asarray(predictions), np.asarray(labels)
        valid = labels != 0
        top = predictions[..., :self.topn][valid]                            # [V, n]
        if top.shape[-1] < 2:
            raise ValueError("%s needs at least 2 ranked items per click (got %d)" % (self.name, top.shape[-1]))
        return top, labels[valid], valid

    def _relevance(self, ids, labels):
        return np.where(ids == labels[:, None], float(self.relevance_positive_sample), float(self.relevance_negative_samples))


class _Novelty(_PerClickMean):
    """sum_{i < n-1} -log2(pop_i) * disc(i) [* rel_i] / sum_{i < n-1} disc(i)  (the last ranked item never contributes)."""
    relevance = False

    def add(self, predictions, labels, predictions_norm_pop):
        top, lab, valid = self._top(predictions, labels)
        m = top.shape[-1] - 1
        pop = np.asarray(predictions_norm_pop, dtype=np.float64)[..., :m][valid]
        w = _log_rank_discount(np.arange(m))
        terms = -np.log2(pop) * w
        if self.relevance:
            terms = terms * self._relevance(top[:, :m], lab)
        self.add_values(terms.sum(axis=-1) / w.sum())


class ExpectedRankSensitiveNovelty(_Novelty):
    name = 'esi-r_at_n'


class ExpectedRankRelevanceSensitiveNovelty(_Novelty):
    name = 'esi-rr_at_n'
    relevance = True

    def __init__(self, topn, relevance_positive_sample, relevance_negative_samples):
        self.relevance_positive_sample = relevance_positive_sample
        self.relevance_negative_samples = relevance_negative_samples
        super().__init__(topn)


def cosine_distances_halved(rows):
    """sklearn.metrics.pairwise.cosine_distances(X, X') / 2 per list, rows [V, n, D] -> [V, n, n] in the rows' dtype: L2-normalised
    rows (a zero row stays zero: distance 0.5 to anything), clip(1 - sim, 0, 2) / 2, the diagonal NOT forced to 0."""
    rows = np.asarray(rows)
    norms = np.sqrt(np.einsum('vnd,vnd->vn', rows, rows))
    norms[norms == 0.0] = 1.0
    xn = rows / norms[..., None]
    sim = np.matmul(xn, np.swapaxes(xn, -1, -2))
    return np.clip(1 - sim, 0, 2) / 2


class _IntraListDiversity(_PerClickMean):
    """Content EILD with a relative rank discount disc(max(0, j - i - 1)), averaged over i < n-1 with disc(i).
    EILD-R: j over all n items but i (so every j < i weighs 1).  EILD-RR: j over i+1 .. n-1, relevance in the inner numerator
    and weights and in the outer numerator, not in the outer denominator (rel 0 with no positive at j > i: 0/0 = NaN, kept)."""
    relevance = False

    def add(self, predictions, labels):
        top, lab, _ = self._top(predictions, labels)
        n = top.shape[-1]
        ace = np.asarray(self.content_article_embeddings_matrix)
        dist = cosine_distances_halved(ace[top]).astype(np.float64)[:, :n - 1, :]      # rows i < n-1
        i, j = np.arange(n - 1)[:, None], np.arange(n)[None, :]
        rel_w = _log_rank_discount(np.maximum(0, j - i - 1))                            # [n-1, n]
        outer = _log_rank_discount(np.arange(n - 1))
        with np.errstate(invalid='ignore', divide='ignore'):
            if not self.relevance:
                rel_w = np.where(j == i, 0.0, rel_w)
                avg = np.einsum('vij,ij->vi', dist, rel_w) / rel_w.sum(axis=-1)
                terms = avg * outer
            else:
                rel = self._relevance(top, lab)                                         # [V, n]
                w = np.where(j > i, rel_w, 0.0)[None] * rel[:, None, :]                 # [V, n-1, n]
                avg = (dist * w).sum(axis=-1) / w.sum(axis=-1)
                terms = avg * outer * rel[:, :n - 1]
        self.add_values(terms.sum(axis=-1) / outer.sum())


class ContentExpectedRankRelativeSensitiveIntraListDiversity(_IntraListDiversity):
    name = 'content_eild-r_at_n'

    def __init__(self, topn, content_article_embeddings_matrix):
        self.content_article_embeddings_matrix = content_article_embeddings_matrix
        super().__init__(topn)


class ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity(_IntraListDiversity):
    name = 'content_eild-rr_at_n'
    relevance = True

    def __init__(self, topn, content_article_embeddings_matrix, relevance_positive_sample, relevance_negative_samples):
        self.content_article_embeddings_matrix = content_article_embeddings_matrix
        self.relevance_positive_sample = relevance_positive_sample
        self.relevance_negative_samples = relevance_negative_samples
        super().__init__(topn)


# the beyond-accuracy classes, in the order of the reference's create_eval_metrics (nar_model.py:1709-1719), and the four whose
# per-click values cham_eval_beyond_accuracy computes (its per_click columns)
BEYOND_ACCURACY_PER_CLICK = (ExpectedRankSensitiveNovelty, ExpectedRankRelevanceSensitiveNovelty,
                             ContentExpectedRankRelativeSensitiveIntraListDiversity,
                             ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity)


def create_beyond_accuracy_metrics(topn, relevance_negative_samples, content_article_embeddings_matrix, recent_clicks_buffer,
                                   relevance_positive_sample=1.0):
    """NDCG, ItemCoverage, ESI-R, ESI-RR, EILD-R, EILD-RR as the reference's create_eval_metrics builds them after HitRate, MRR."""
    return [NDCG(topn), ItemCoverage(topn, recent_clicks_buffer), ExpectedRankSensitiveNovelty(topn),
            ExpectedRankRelevanceSensitiveNovelty(topn, relevance_positive_sample, relevance_negative_samples),
            ContentExpectedRankRelativeSensitiveIntraListDiversity(topn, content_article_embeddings_matrix),
            ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity(topn, content_article_embeddings_matrix,
                                                                            relevance_positive_sample, relevance_negative_samples)]
