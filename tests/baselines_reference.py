"""Plain numpy / dict model of the four baseline recommenders of the evaluation (pop_recent, cb, coocurrent, sr): what
csrc/baselines.hip and nar/baselines.py must compute.  Integer scores are exact; cb runs in float64.  Ties: among equal scores the
smaller item id ranks first.  A candidate is live if it is scored and no earlier column holds the same id (the reference walks a
ranking of unique items and keeps those that are candidates)."""
import numpy as np

SR_SCALE = 2520          # lcm(1..10): the 'div' decay 1 / (i - j), i - j <= 10, as exact integers
NAMES = ('pop_recent', 'cb', 'coocurrent', 'sr')


def sessions_of(aci, n_items):
    """Rows of aci [B, T1] -> lists of their ids in [1, n_items), in order."""
    return [[int(x) for x in row if 1 <= int(x) < n_items] for row in np.asarray(aci)]


def learn_cooc(table, aci, n_items):
    """+1 for every distinct ordered id pair of two different positions of a session, once per session."""
    for s in sessions_of(aci, n_items):
        pairs = set((s[p], s[q]) for p in range(len(s)) for q in range(len(s)) if p != q)
        for k in pairs:
            table[k] = table.get(k, 0) + 1
    return table


def learn_sr(table, aci, n_items, max_dist=10):
    """rules[s_j][s_i] += 2520 / (i - j) for 1 <= i - j <= max_dist."""
    for s in sessions_of(aci, n_items):
        for i in range(1, len(s)):
            for j in range(max(0, i - max_dist), i):
                k = (s[j], s[i])
                table[k] = table.get(k, 0) + SR_SCALE // (i - j)
    return table


def candidates(label_next, neg_ids):
    label_next, neg_ids = np.asarray(label_next, np.int64), np.asarray(neg_ids, np.int64)
    return np.concatenate([label_next[..., None], neg_ids], axis=-1)          # [B, T, 1 + N], column 0 = the label


def cosine64(x, y):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx, ny = np.sqrt((x * x).sum()), np.sqrt((y * y).sum())
    return float((x / (nx if nx else 1.0)) @ (y / (ny if ny else 1.0)))


def scores(name, item_clicked, label_next, neg_ids, n_items, recent_pop=None, ace=None, table=None):
    """(score [B, T, NC] int64 | float64, scored [B, T, NC] bool); nothing is scored at a padded position (label 0)."""
    cand = candidates(label_next, neg_ids)
    B, T, NC = cand.shape
    score = np.zeros(cand.shape, np.float64 if name == 'cb' else np.int64)
    scored = np.zeros(cand.shape, bool)
    item_clicked = np.asarray(item_clicked)
    for b in range(B):
        for t in range(T):
            if cand[b, t, 0] == 0:
                continue
            item = int(item_clicked[b, t])
            for c in range(NC):
                i = int(cand[b, t, c])
                if name == 'pop_recent':
                    if 0 <= i < n_items and recent_pop[i] > 0:
                        score[b, t, c], scored[b, t, c] = int(recent_pop[i]), True
                elif name == 'cb':
                    if 0 <= i < n_items and 0 <= item < n_items:
                        score[b, t, c], scored[b, t, c] = cosine64(ace[item], ace[i]), True
                elif (item, i) in table and 1 <= i < n_items and 1 <= item < n_items:
                    score[b, t, c], scored[b, t, c] = table[(item, i)], True
    return score, scored


def live_mask(cand_row, scored_row):
    live = np.array(scored_row, bool)
    for c in range(len(cand_row)):
        if live[c] and (cand_row[:c] == cand_row[c]).any():
            live[c] = False
    return live


def rank(score, scored, label_next, neg_ids, topn):
    """(label_rank [B, T] int32: -1 at padding, max(NC, topn) for an unscored label; pred_ids [B, T, topn] int64, 0-padded)."""
    cand = candidates(label_next, neg_ids)
    B, T, NC = cand.shape
    label_rank = np.full((B, T), -1, np.int32)
    pred_ids = np.zeros((B, T, topn), np.int64)
    for b in range(B):
        for t in range(T):
            if cand[b, t, 0] == 0:
                continue
            live = live_mask(cand[b, t], scored[b, t])
            order = sorted(np.flatnonzero(live).tolist(), key=lambda c: (-score[b, t, c], cand[b, t, c]))
            label_rank[b, t] = order.index(0) if live[0] else max(NC, topn)
            for r, c in enumerate(order[:topn]):
                pred_ids[b, t, r] = cand[b, t, c]
    return label_rank, pred_ids


def rank_bracket(score, scored, label_next, neg_ids):
    """Per click (lo, hi): the label's rank lies in [lo, hi] under ANY order of equal scores - lo = live candidates strictly above the
    label, hi = lo + live candidates tied with it.  (-1, -1) at padding; (None) handled by the caller for an unscored label: lo = hi = NC."""
    cand = candidates(label_next, neg_ids)
    B, T, NC = cand.shape
    lo = np.full((B, T), -1, np.int64)
    hi = np.full((B, T), -1, np.int64)
    for b in range(B):
        for t in range(T):
            if cand[b, t, 0] == 0:
                continue
            live = live_mask(cand[b, t], scored[b, t])
            if not live[0]:
                lo[b, t] = hi[b, t] = NC
                continue
            others = np.flatnonzero(live)[1:]
            lo[b, t] = int((score[b, t, others] > score[b, t, 0]).sum())
            hi[b, t] = lo[b, t] + int((score[b, t, others] == score[b, t, 0]).sum())
    return lo, hi


class Model:
    """The four baselines over a stream of batches, with the hook's order: evaluate (EVAL), then learn (both modes)."""

    def __init__(self, n_items, ace=None, names=NAMES):
        self.n_items, self.ace, self.names = n_items, ace, tuple(names)
        self.tables = {'coocurrent': {}, 'sr': {}}
        self.hits = {n: 0 for n in self.names}
        self.rr = {n: 0.0 for n in self.names}
        self.clicks = 0

    def learn(self, aci):
        if 'coocurrent' in self.names:
            learn_cooc(self.tables['coocurrent'], aci, self.n_items)
        if 'sr' in self.names:
            learn_sr(self.tables['sr'], aci, self.n_items)

    def save_state_checkpoint(self):
        self._chkp = {k: dict(v) for k, v in self.tables.items()}

    def restore_state_checkpoint(self):
        self.tables = self._chkp
        del self._chkp

    def evaluate(self, item_clicked, label_next, neg_ids, topn, recent_pop=None):
        out = {}
        for n in self.names:
            sc, sd = scores(n, item_clicked, label_next, neg_ids, self.n_items, recent_pop=recent_pop, ace=self.ace,
                            table=self.tables.get(n))
            lr, pi = rank(sc, sd, label_next, neg_ids, topn)
            out[n] = dict(score=sc, scored=sd, label_rank=lr, pred_ids=pi)
            hit = (lr >= 0) & (lr < topn)
            self.hits[n] += int(hit.sum())
            self.rr[n] += float((1.0 / (1.0 + lr[hit])).sum())
        self.clicks += int((np.asarray(label_next) != 0).sum())
        return out

    def results(self):
        res = {}
        for n in self.names:
            res['hitrate_at_n_' + n] = self.hits[n] / float(self.clicks) if self.clicks else float('nan')
            res['mrr_at_n_' + n] = self.rr[n] / float(self.clicks) if self.clicks else float('nan')
        return res
