"""Baseline recommenders of the evaluation on the device (reference nar_module/nar/benchmarks): 'pop_recent' (most popular of the
recent-clicks buffer), 'cb' (content cosine to the current item), 'coocurrent' (session co-occurrence counts), 'sr' (sequential rules,
'div' decay over at most 10 clicks) and 'v-sknn' (session kNN with the 'div' decay of the active session's clicks: cosine, the last 3000
sessions, 1000 sampled candidates, 500 neighbours).  Each scores the SAME candidate rows the model ranks - {label} + the click's
negatives - with the kernels of csrc/baselines.hip and csrc/vsknn.hip; the rank of the positive goes into one cham_eval_rank_hist record
per baseline, from which HitRate@n, MRR@n and HitRate by position follow (metrics.accuracy_from_rank_hist).  Ties: among equal scores the
smaller item id ranks first.  ItemKNN ('item_knn') and SessionKNN without the decay ('sknn') are not available.

The two learned baselines keep their (item, item) -> weight maps in one open-addressing table each (integer weights: SR stores
2520 / distance).  The tables grow on the host without a read-back per step: see PairTable.
'v-sknn' keeps the last sessions in a ring in HBM: see SessionRing."""
import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr

BASELINE_NAMES = ('pop_recent', 'cb', 'coocurrent', 'sr', 'v-sknn')
SR_SCALE = 2520
SR_MAX_CLICKS_DIST = 10
DEFAULT_MAX_PAIRS = 1 << 25
VSKNN_SESSIONS_BUFFER_SIZE = 3000           # the reference trainers' hard-wired V-SkNN sizes
VSKNN_CANDIDATE_SESSIONS_SAMPLE_SIZE = 1000
VSKNN_NEAREST_NEIGHBOR_SESSIONS = 500
VSKNN_MAX_T, VSKNN_MAX_SESSIONS, VSKNN_ROW, MAX_CANDIDATES = 64, 4096, 65, 1024       # limits of csrc/vsknn.hip (VS_MAX_*, BL_MAX_NC)
_KIND = {'pop_recent': 0, 'cb': 1, 'coocurrent': 2, 'sr': 2, 'v-sknn': 3}
_SCORE_DTYPE = {'cb': torch.float32, 'v-sknn': torch.float64}
_MASK64 = (1 << 64) - 1


def parse_eval_benchmarks(value):
    """'--eval_benchmarks' value (comma list or list) -> tuple of names in the reference's order; ValueError for an unknown name."""
    names = [x.strip() for x in (value.split(',') if isinstance(value, str) else list(value or [])) if str(x).strip()]
    for n in names:
        if n not in BASELINE_NAMES:
            raise ValueError("--eval_benchmarks: unknown baseline %r (available: %s)" % (n, ', '.join(BASELINE_NAMES)))
    return tuple(n for n in BASELINE_NAMES if n in names)


def pair_slot(a, b, cap):
    """First probe slot of key (a, b) in a table of `cap` slots (the splitmix64 finaliser of csrc/baselines.hip)."""
    x = ((a << 32) | b) & _MASK64
    x ^= x >> 30; x = (x * 0xBF58476D1CE4E5B9) & _MASK64
    x ^= x >> 27; x = (x * 0x94D049BB133111EB) & _MASK64
    x ^= x >> 31
    return x & (cap - 1)


def _stream():
    return torch.cuda.current_stream().cuda_stream


class PairTable:
    """(a, b) -> int64 weight in HBM (include/chameleon_nar.h "PAIR TABLE").  Growth: the caller announces an upper bound of the entries a
    batch can add (reserve); the running bound never lets the load pass 1/2.  Only when the bound would pass it, the true entry count is
    read (one 16-byte read-back, which also checks the dropped-insert counter), and if that is still too high the table doubles and is
    rehashed.  ``max_pairs`` caps the entries; beyond it reserve raises a ValueError naming ``flag``."""

    def __init__(self, device, capacity=1 << 16, max_pairs=DEFAULT_MAX_PAIRS, flag='--eval_benchmarks_max_pairs', name='pairs'):
        if capacity < 2 or capacity & (capacity - 1):
            raise ValueError("capacity must be a power of two >= 2")
        self.lib, self.device, self.max_pairs, self.flag, self.name = _lib.load(), torch.device(device), int(max_pairs), flag, name
        self._alloc(int(capacity))
        self.bound = 0

    def _alloc(self, cap):
        self.cap = cap
        self.keys = torch.zeros(cap, dtype=torch.int64, device=self.device)
        self.vals = torch.zeros(cap, dtype=torch.int64, device=self.device)
        self.meta = torch.zeros(2, dtype=torch.int64, device=self.device)

    def counters(self):
        """(dropped inserts, entries): one small read-back; a dropped insert is an error (the growth rule makes it unreachable)."""
        dropped, entries = self.meta.cpu().tolist()
        if dropped:
            raise RuntimeError("%s pair table: %d inserts found no free slot (capacity %d)" % (self.name, dropped, self.cap))
        return dropped, entries

    def reserve(self, new_entries):
        if self.bound + new_entries > self.cap // 2:
            self.bound = self.counters()[1]
            cap = self.cap
            while self.bound + new_entries > cap // 2:
                cap *= 2
            if cap != self.cap:
                if self.bound + new_entries > self.max_pairs:
                    raise ValueError("the %s baseline's table would pass %d entries: raise %s" % (self.name, self.max_pairs, self.flag))
                old = (self.keys, self.vals, self.cap)
                self._alloc(cap)
                check(self.lib.cham_pairs_rehash(ptr(old[0]), ptr(old[1]), old[2], ptr(self.keys), ptr(self.vals), self.cap, ptr(self.meta),
                                                 _stream()), "cham_pairs_rehash")
        self.bound += new_entries

    def insert_cooc(self, aci, n_items):
        B, T1 = aci.shape
        self.reserve(B * T1 * max(T1 - 1, 1))
        check(self.lib.cham_pairs_insert_cooc(ptr(aci), B, T1, n_items, ptr(self.keys), ptr(self.vals), self.cap, ptr(self.meta), _stream()),
              "cham_pairs_insert_cooc")

    def insert_sr(self, aci, n_items, max_dist=SR_MAX_CLICKS_DIST):
        B, T1 = aci.shape
        self.reserve(B * (T1 - 1) * min(T1 - 1, max_dist))
        check(self.lib.cham_pairs_insert_sr(ptr(aci), B, T1, max_dist, n_items, ptr(self.keys), ptr(self.vals), self.cap, ptr(self.meta),
                                            _stream()), "cham_pairs_insert_sr")

    def export(self):
        """{(a, b): weight} of the table (tests, checkpoints)."""
        ko, vo = torch.empty_like(self.keys), torch.empty_like(self.vals)
        n = torch.zeros(1, dtype=torch.int64, device=self.device)
        check(self.lib.cham_pairs_export(ptr(self.keys), ptr(self.vals), self.cap, ptr(ko), ptr(vo), self.cap, ptr(n), _stream()),
              "cham_pairs_export")
        n = int(n.cpu()[0])
        k, v = ko[:n].cpu().numpy().view(np.uint64), vo[:n].cpu().numpy()
        order = np.argsort(k)
        return {(int(x) >> 32, int(x) & 0xFFFFFFFF): int(w) for x, w in zip(k[order].tolist(), v[order].tolist())}

    def snapshot(self):
        return (self.keys.clone(), self.vals.clone(), self.meta.clone(), self.cap, self.bound)

    def restore(self, snap):
        self.keys, self.vals, self.meta, self.cap, self.bound = snap


class SessionRing:
    """The last `size` sessions of 'v-sknn' in HBM (include/chameleon_nar.h "SESSION RING"): items int32 [size, 65], lens, session ids and
    the slots' order by session id descending.  Row r of a batch goes to slot (appended + r) mod size; `appended` is counted here, on the
    host, so an append needs no read-back.  size * 65 * 4 bytes of items (0.78 MB at 3000) + 16 bytes per slot."""

    def __init__(self, device, size=VSKNN_SESSIONS_BUFFER_SIZE):
        if not 1 <= size <= VSKNN_MAX_SESSIONS:
            raise ValueError("v-sknn: the sessions buffer holds 1 .. %d sessions (got %d)" % (VSKNN_MAX_SESSIONS, size))
        self.lib, self.device, self.size = _lib.load(), torch.device(device), int(size)
        self.items = torch.zeros(self.size, VSKNN_ROW, dtype=torch.int32, device=self.device)
        self.lens = torch.zeros(self.size, dtype=torch.int32, device=self.device)
        self.ids = torch.zeros(self.size, dtype=torch.int64, device=self.device)
        self.order = torch.arange(self.size, dtype=torch.int32, device=self.device)
        self.appended = 0

    def append(self, aci, session_ids, n_items):
        B, T1 = aci.shape
        if T1 > VSKNN_ROW:
            raise ValueError("v-sknn: a session row holds at most %d ids (got %d)" % (VSKNN_ROW, T1))
        if session_ids.dtype != torch.int64 or session_ids.numel() != B or not session_ids.is_contiguous():
            raise ValueError("v-sknn: session_ids int64 [B] expected")
        check(self.lib.cham_vsknn_append(ptr(aci), ptr(session_ids), B, T1, n_items, self.appended, self.size, VSKNN_ROW, ptr(self.items),
                                         ptr(self.lens), ptr(self.ids), ptr(self.order), _stream()), "cham_vsknn_append")
        self.appended += B

    def export(self):
        """[(session id, sorted item ids)] of the buffered sessions, oldest first (tests)."""
        items, lens, ids = self.items.cpu().numpy(), self.lens.cpu().numpy(), self.ids.cpu().numpy()
        n = min(self.appended, self.size)
        slots = [i % self.size for i in range(self.appended - n, self.appended)]
        return [(int(ids[s]), sorted(items[s, :lens[s]].tolist())) for s in slots]

    def snapshot(self):
        return (self.items.clone(), self.lens.clone(), self.ids.clone(), self.order.clone(), self.appended)

    def restore(self, snap):
        self.items, self.lens, self.ids, self.order, self.appended = snap


class DeviceBaselines:
    """The enabled baselines' state (pair tables, the session ring) and evaluation records (one rank histogram each).  Lives across the Estimator's
    train / evaluate calls like the clicked-items state; the hook calls evaluate (EVAL) and learn (both modes) per batch.
    ``table_capacity``: the slots each table starts with (2^22 = 64 MB: half of it is ~20 G1 batches' worth of the per-batch bound, so
    the growth rule reads the entry count back every ~20 steps at the earliest, not every step)."""

    def __init__(self, names, n_items, ace, device='cuda:0', max_pairs=DEFAULT_MAX_PAIRS, sr_decay='div', table_capacity=1 << 22,
                 sessions_buffer_size=VSKNN_SESSIONS_BUFFER_SIZE, candidate_sessions_sample_size=VSKNN_CANDIDATE_SESSIONS_SAMPLE_SIZE,
                 nearest_neighbor_session_for_scoring=VSKNN_NEAREST_NEIGHBOR_SESSIONS):
        self.names = parse_eval_benchmarks(names)
        if sr_decay != 'div':
            raise ValueError("sequential rules: only the 'div' decay (the trainer's configuration) is available, not %r" % (sr_decay,))
        self.lib, self.device, self.n_items = _lib.load(), torch.device(device), int(n_items)
        self.ace = None
        if ace is not None:
            self.attach_ace(ace)
        self.tables = {n: PairTable(self.device, table_capacity, max_pairs, name=n) for n in self.names if _KIND[n] == 2}
        self.ring = None
        if 'v-sknn' in self.names:
            if candidate_sessions_sample_size < 1 or nearest_neighbor_session_for_scoring < 1:
                raise ValueError("v-sknn: the sample size and the number of neighbours are >= 1")
            self.ring = SessionRing(self.device, sessions_buffer_size)
            self.sample, self.knn = int(candidate_sessions_sample_size), int(nearest_neighbor_session_for_scoring)
        self.records = None
        self._buf = {}

    def attach_ace(self, ace):
        """The content embeddings 'cb' reads: the runtime's device matrix (not copied), or a host array."""
        self.ace = ace if isinstance(ace, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ace, dtype=np.float32)).to(self.device)
        if self.ace.dtype != torch.float32 or self.ace.dim() != 2 or self.ace.stride(1) != 1 or self.ace.shape[0] != self.n_items:
            raise ValueError("content embeddings: float32 [n_items, D] rows expected")

    # ---- learning (TRAIN and EVAL)
    def learn(self, aci, session_ids=None):
        """aci int64 [B, T + 1] device tensor = concat(item_clicked, label_last_item) of the (global) batch; session_ids int64 [B] device
        tensor (needed by 'v-sknn' only)."""
        if self.ring is not None:
            if session_ids is None:
                raise ValueError("the 'v-sknn' baseline needs the batch's session ids")
            self.ring.append(aci, session_ids.reshape(-1), self.n_items)
        if 'coocurrent' in self.tables:
            self.tables['coocurrent'].insert_cooc(aci, self.n_items)
        if 'sr' in self.tables:
            self.tables['sr'].insert_sr(aci, self.n_items)

    def check_tables(self):
        for t in self.tables.values():
            t.counters()

    def save_state_checkpoint(self):
        self._chkp = {n: t.snapshot() for n, t in self.tables.items()}
        self._ring_chkp = self.ring.snapshot() if self.ring is not None else None

    def restore_state_checkpoint(self):
        for n, t in self.tables.items():
            t.restore(self._chkp[n])
        del self._chkp
        if self.ring is not None:
            self.ring.restore(self._ring_chkp)
        del self._ring_chkp

    # ---- evaluation
    def begin_evaluation(self, topn, t_cap=32):
        if not 1 <= topn <= 256:
            raise ValueError("the baselines' rank histogram needs 1 <= eval_metrics_top_n <= 256 (got %d)" % topn)
        self.topn = int(topn)
        self.records = {n: dict(hist=torch.zeros(t_cap, self.topn + 1, dtype=torch.int64, device=self.device),
                                pop_sum=torch.zeros(t_cap, dtype=torch.float64, device=self.device)) for n in self.names}
        self.t_cap = t_cap

    def _reserve(self, T):
        if T > self.t_cap:
            t_cap = max(T, 2 * self.t_cap)
            for r in self.records.values():
                hist = torch.zeros(t_cap, self.topn + 1, dtype=torch.int64, device=self.device)
                hist[:self.t_cap].copy_(r['hist'])
                r.update(hist=hist, pop_sum=torch.zeros(t_cap, dtype=torch.float64, device=self.device))
            self.t_cap = t_cap

    def _buffers(self, name, BT, NC):
        key = (name, BT, NC, self.topn)
        b = self._buf.get(name)
        if b is None or b['key'] != key:
            dev = self.device
            b = self._buf[name] = dict(key=key, score=torch.empty(BT, NC, dtype=_SCORE_DTYPE.get(name, torch.int64), device=dev),
                                       scored=torch.empty(BT, NC, dtype=torch.uint8, device=dev),
                                       label_rank=torch.empty(BT, dtype=torch.int32, device=dev),
                                       pred_ids=torch.empty(BT, self.topn, dtype=torch.int64, device=dev))
        return b

    def score_and_rank(self, name, item_clicked, label_next, neg_ids, recent_pop=None, neighbours=False):
        """Scores + ranking of one baseline over device tensors item_clicked / label_next [B, T] and neg_ids [B, T, N] (int64);
        recent_pop int32 [n_items] for 'pop_recent'.  Returns the buffers dict (score, scored, label_rank [BT], pred_ids [BT, topn]);
        neighbours=True ('v-sknn', tests): also sim float64 / n int32 [BT, ring size] by ring slot."""
        B, T, N = neg_ids.shape
        BT = B * T
        kind = _KIND[name]
        if kind == 3 and N + 1 > MAX_CANDIDATES:
            raise ValueError("v-sknn: at most %d candidates per click (got 1 + %d)" % (MAX_CANDIDATES, N))
        b = self._buffers(name, BT, N + 1)
        if kind == 3:
            ring = self.ring
            if T > VSKNN_MAX_T:
                raise ValueError("v-sknn: at most %d click positions per session row (got %d)" % (VSKNN_MAX_T, T))
            sim = n = None
            if neighbours:
                sim = b['sim'] = torch.empty(BT, ring.size, dtype=torch.float64, device=self.device)
                n = b['n'] = torch.empty(BT, ring.size, dtype=torch.int32, device=self.device)
            check(self.lib.cham_vsknn_scores(ptr(item_clicked), ptr(label_next), ptr(neg_ids), B, T, N, ptr(ring.items), ptr(ring.lens),
                                             ptr(ring.order), ring.size, VSKNN_ROW, self.sample, self.knn, ptr(b['score']), ptr(b['scored']),
                                             ptr(sim) if neighbours else None, ptr(n) if neighbours else None, _stream()),
                  "cham_vsknn_scores")
            check(self.lib.cham_baseline_rank(ptr(b['score']), 2, ptr(b['scored']), ptr(label_next), ptr(neg_ids), BT, N, self.topn,
                                              ptr(b['label_rank']), ptr(b['pred_ids']), _stream()), "cham_baseline_rank")
            return b
        tab = self.tables.get(name)
        if kind == 1 and self.ace is None:
            raise ValueError("the 'cb' baseline needs the content embeddings matrix (attach_ace)")
        if kind == 0 and (recent_pop is None or recent_pop.dtype != torch.int32 or recent_pop.numel() != self.n_items):
            raise ValueError("pop_recent: recent_pop int32 [n_items] expected")
        check(self.lib.cham_baseline_scores(kind, ptr(item_clicked), ptr(label_next), ptr(neg_ids), BT, N, self.n_items,
                                            ptr(recent_pop) if kind == 0 else None, ptr(self.ace) if kind == 1 else None,
                                            self.ace.shape[1] if kind == 1 else 0, self.ace.stride(0) if kind == 1 else 0,
                                            ptr(tab.keys) if tab else None, ptr(tab.vals) if tab else None, tab.cap if tab else 0,
                                            ptr(b['score']), ptr(b['scored']), _stream()), "cham_baseline_scores")
        check(self.lib.cham_baseline_rank(ptr(b['score']), 1 if kind == 1 else 0, ptr(b['scored']), ptr(label_next), ptr(neg_ids), BT, N,
                                          self.topn, ptr(b['label_rank']), ptr(b['pred_ids']), _stream()), "cham_baseline_rank")
        return b

    def evaluate(self, item_clicked, label_next, neg_ids, recent_pop=None):
        """One EVAL batch in the [B, T] layout: every enabled baseline's label ranks into its histogram record.  No read-back."""
        B, T, N = neg_ids.shape
        self._reserve(T)
        for name in self.names:
            b = self.score_and_rank(name, item_clicked, label_next, neg_ids, recent_pop)
            r = self.records[name]
            check(self.lib.cham_eval_rank_hist(ptr(b['label_rank']), ptr(label_next), B, T, self.topn, None, self.n_items, ptr(r['hist']),
                                               ptr(r['pop_sum']), self.t_cap, _stream()), "cham_eval_rank_hist")

    def results(self, topn=None, by_session_position=False):
        """{'hitrate_at_n_<name>': ..., 'mrr_at_n_<name>': ...} (+ the per-position hit rates) of the evaluation so far."""
        from .evaluation import compute_metrics_results
        from .metrics import HitRate, HitRateBySessionPosition, MRR, accuracy_from_rank_hist
        topn = self.topn if topn is None else int(topn)
        if topn != self.topn:
            raise ValueError("results(topn=%d): the evaluation was begun with topn %d" % (topn, self.topn))
        out = {}
        for name in self.names:
            acc = accuracy_from_rank_hist(self.records[name]['hist'].cpu().numpy(), None, topn)

            class _Value:
                def __init__(self, metric):
                    self.name = metric

                def result(self, acc=acc):
                    return acc[self.name]
            metrics = [_Value(HitRate.name), _Value(MRR.name)] + ([_Value(HitRateBySessionPosition.name)] if by_session_position else [])
            out.update(compute_metrics_results(metrics, recommender=name))
        return out
