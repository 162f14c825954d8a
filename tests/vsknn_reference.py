"""Plain numpy / Python model of the V-SkNN baseline (reference nar/benchmarks/session_knn.py in the trainers' configuration: cosine,
'div' decay, 'recent' sampling): what csrc/vsknn.hip and nar/baselines.SessionRing must compute.  float64 in the reference's order of
operations, so sim is the same IEEE value; a session's copies MULTIPLY its sim (the reference adds sim once per copy).

Rules that differ from the reference on purpose: a buffered session is always found and 'recent' means larger session id (the
reference's binary search assumes ids arrive ascending); a session id that arrives twice is two sessions; equal similarities at the knn
cut are broken by session id descending always (the reference: only after sampling; otherwise by set-iteration order); equal final
scores rank the smaller item id first."""
import math

import numpy as np


class Ring:
    """FIFO of the last S sessions as (session id, list of distinct valid ids in order of first occurrence), in SLOT order: row r of a
    batch goes to slot (appended + r) mod S."""

    def __init__(self, S, n_items):
        self.S, self.n_items = int(S), int(n_items)
        self.slots = [None] * self.S
        self.appended = 0

    def append(self, aci, session_ids):
        for r, (row, sid) in enumerate(zip(np.asarray(aci), np.asarray(session_ids))):
            items = []
            for x in row.tolist():
                if 1 <= x < self.n_items and x not in items:
                    items.append(int(x))
            self.slots[(self.appended + r) % self.S] = (int(sid), items)
        self.appended += len(aci)

    def sessions(self):
        """The buffered sessions oldest first: [(session id, sorted item ids)] - the reference's last_sessions_buffer."""
        n = min(self.appended, self.S)
        first = self.appended - n
        return [(self.slots[i % self.S][0], sorted(self.slots[i % self.S][1])) for i in range(first, self.appended)]

    def snapshot(self):
        return (list(self.slots), self.appended)

    def restore(self, snap):
        self.slots, self.appended = list(snap[0]), snap[1]

    def order(self):
        """Slots by session id descending, slot ascending among equal ids; never-written slots count as id 0."""
        ids = [s[0] if s is not None else 0 for s in self.slots]
        return sorted(range(self.S), key=lambda s: (-ids[s], s))


def click(ring, partial, sample, knn):
    """One click: partial = item_clicked[b, 0..t] (a list that may repeat ids).  Returns dict(sim [S], m [S], k [S], n [S] by slot,
    sampled, cut, ambiguous)."""
    S = ring.S
    partial = [int(x) for x in partial]
    t = len(partial) - 1
    a = len(set(partial))
    sim, m = np.zeros(S, np.float64), np.zeros(S, np.int64)
    for s, sess in enumerate(ring.slots):
        if sess is None or not sess[1]:
            continue
        items = set(sess[1])
        decay = 0
        for pos, item in enumerate(reversed(partial)):            # from p = t downwards
            if item in items:
                decay += 1 / (pos + 1)
                m[s] += 1
        if m[s]:
            sim[s] = decay / (math.sqrt(a) * math.sqrt(len(items)))
    order = ring.order()
    k = m.copy()
    sampled = int(m.sum()) > sample
    if sampled:
        kept = 0
        for s in order:
            k[s] = min(m[s], sample - kept)
            kept += k[s]
    elig = [s for s in order if k[s] > 0 and 0.0 < sim[s] < 1.0]
    ranked = sorted(elig, key=lambda s: -sim[s])                   # stable: session id descending among equal sim
    n = np.zeros(S, np.int64)
    kept = 0
    cut = sum(int(k[s]) for s in elig) > knn
    ambiguous = False
    for s in ranked:
        n[s] = min(k[s], knn - kept)
        kept += n[s]
    if cut and not sampled:
        # the knn cut falls inside a group of equal sim that spans more than one session: the reference's set order decides
        group = {}
        for s in ranked:
            group.setdefault(sim[s], []).append(s)
        for g in group.values():
            if len(g) > 1 and any(n[s] < k[s] for s in g) and any(n[s] > 0 for s in g):
                ambiguous = True                                   # (a cut between two whole groups is not ambiguous)
    return dict(sim=sim, m=m, k=k, n=n, sampled=sampled, cut=cut, ambiguous=ambiguous)


def scores(ring, item_clicked, label_next, neg_ids, sample, knn, details=False):
    """(score float64 [B, T, NC], scored bool [B, T, NC]) (+ per-click details {(b, t): click()}) of a batch: scored iff some
    session with n > 0 holds the candidate; sum in session-id-descending order."""
    item_clicked = np.asarray(item_clicked)
    cand = np.concatenate([np.asarray(label_next)[..., None], np.asarray(neg_ids)], axis=-1)
    B, T, NC = cand.shape
    score, scored = np.zeros(cand.shape, np.float64), np.zeros(cand.shape, bool)
    info = {}
    order = ring.order()
    sets = [set(s[1]) if s is not None else set() for s in ring.slots]
    for b in range(B):
        for t in range(T):
            if item_clicked[b, t] == 0:
                continue
            d = click(ring, item_clicked[b, :t + 1], sample, knn)
            info[(b, t)] = d
            for s in order:
                if d['n'][s] > 0:
                    w = float(d['n'][s]) * d['sim'][s]
                    for c in range(NC):
                        if int(cand[b, t, c]) in sets[s]:
                            score[b, t, c] += w
                            scored[b, t, c] = True
    return (score, scored, info) if details else (score, scored)
