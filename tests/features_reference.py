"""float64 numpy references of the head of a training step: the feature front end (csrc/features.hip: raw recency / novelty, the
normalisation statistics, the user-context and item rows, the first-batch row weights, the integer row sets, dropout, the dense PreCAR
input rows) and the PreCAR combine forward (top of csrc/scorer.hip), written from the reference's nar_model.py (:28-34 log_base / log_1p,
:217-248 inputs and mask, :730-773 get_features, :887-907 scale / center, :921-994 item features, :996-1039 normalize_values /
min_max_normalization, :1055-1089 recency, :1147-1186 novelty, :356-405 PreCAR over [user context ; item]) and from TF 1.12's
tf.nn.dropout - not from the kernels and not from oracle/nar_oracle.py.  Only oracle/philox.py is shared: it is the definition of the
dropout mask.

Every function takes `dtype`: float64 is the reference, float32 is the same formula as a CPU would evaluate it in the kernels' precision
(the sums one element after the other).  `slip` keywords plant one mistake each; tests/test_features_reference_cpu.py shows that each
moves some compared array by ten bounds.  Also here, shared by the CPU file and the GPU files so that all see the same numbers: the input
generators, the case lists and the error measures."""
import functools

import numpy as np

from oracle import philox
from tests.tail_reference import f64, rel_err, round_bf16_bits, same_bits  # noqa: F401  (re-exported: the GPU tests take them from here)

COL_ZERO, COL_OHE, COL_EMB, COL_NUM, COL_ACE, COL_ITEMEMB, COL_RECENCY, COL_NOVELTY = range(8)     # include/chameleon_nar.h, K1
MS_PER_DAY = 86400000.0
LEAKY = 0.2
EPS = 1e-24                   # nar_model.py:1001, 1007, 1025
DEFAULT_BASES = (1.3, 2.0)    # elapsed_days_smooth_log_base, popularity_smooth_log_base (nar_model.py:122-123)
OTHER_BASES = (1.7, 3.0)
T0 = 1500000000000            # ms since the epoch: July 2017, where an fp32 holds a time stamp to 131 072 ms


# ---- raw recency and novelty -------------------------------------------------------------------------------------------------------
def recency_raw(ref_ts, created, base, dtype=np.float64, **slip):
    """nar_model.py:1055-1060, 1071-1075: log_base(1 + relu((f32(ref_ts) - f32(created)) / 86.4e6)).  The two int64 -> fp32 conversions
    are the graph's own and part of the operation: they are done in fp32 whatever `dtype` is, everything after them in `dtype`."""
    dt = dtype
    ref_ts, created = np.asarray(ref_ts, np.int64), np.asarray(created, np.int64)
    if slip.get('int64_subtraction'):
        d = (ref_ts - created).astype(np.float32).astype(dt)
    else:
        d = ref_ts.astype(np.float32).astype(dt) - created.astype(np.float32).astype(dt)
    d = d / dt(MS_PER_DAY)
    if not slip.get('relu_dropped'):
        d = np.maximum(d, dt(0))
    with np.errstate(divide='ignore', invalid='ignore'):
        lg = np.log(d) if slip.get('log_x') else np.log(d + dt(1))
        return lg if slip.get('natural_log') else lg / np.log(dt(base))


def novelty_raw(pop_norm, base, dtype=np.float64, **slip):
    """nar_model.py:1147-1148: -log_base(pop_norm); no epsilon, pop_norm is positive (its floor is 1 / recent_clicks_for_normalization)."""
    dt = dtype
    lg = np.log(np.asarray(pop_norm).astype(dt))
    return -lg if slip.get('natural_log') else -(lg / np.log(dt(base)))


# ---- normalisation statistics ------------------------------------------------------------------------------------------------------
def _sum(a, dt):
    """Sum of a 1-d array in dt: pairwise-or-better in float64, strictly one element after the other in float32 (np.cumsum)."""
    a = np.asarray(a, dt)
    if a.size == 0:
        return dt(0)
    return a.sum(dtype=dt) if dt == np.float64 else np.cumsum(a, dtype=dt)[-1]


def norm_stats(vals, weights=None, dtype=np.float64, **slip):
    """[mean, sd, zmin, zmax] of a weighted population (nar_model.py:1014-1025 tf.nn.moments + :1001-1008): weighted mean and POPULATION
    variance, sd = sqrt(var + 1e-24), zmin / zmax = the extremes of (x - mean) / sd over the entries with weight > 0.  A weight is a
    repetition count (the first batch's population is "this call's non-pad ids WITH repetition", :1078-1084); None = all ones."""
    dt = dtype
    x = np.asarray(vals).astype(dt)
    w = np.ones(x.shape, dt) if weights is None else np.asarray(weights).astype(dt)
    live = w > 0
    sw = _sum(w[live], dt)
    mean = _sum(x[live], dt) / dt(live.sum()) if slip.get('weights_ignored_in_mean') else _sum(w[live] * x[live], dt) / sw
    d = x[live] - mean
    with np.errstate(divide='ignore', invalid='ignore'):
        var = _sum(w[live] * d * d, dt) / ((sw - dt(1)) if slip.get('sample_variance') else sw)
        sd = np.sqrt(var) if slip.get('sd_without_epsilon') else np.sqrt(var + dt(EPS))
        pool = x if slip.get('minmax_over_zero_weights') else x[live]
        return np.array([mean, sd, (pool.min() - mean) / sd, (pool.max() - mean) / sd], dt)


def norm_apply(x, stats, dtype=np.float64):
    """nar_model.py:1031-1037 with min_max_normalization :1007-1008: z = (x - mean) / sd, (z - zmin + 1e-24) / max(zmax - zmin, 2e-24)
    scaled to [-1, 1].  stats [..., 4] broadcasts against x."""
    dt = dtype
    x, st = np.asarray(x).astype(dt), np.asarray(stats).astype(dt)
    z = (x - st[..., 0]) / st[..., 1]
    scaled = (z - st[..., 2] + dt(EPS)) / np.maximum(st[..., 3] - st[..., 2], dt(2 * EPS))
    return scaled * dt(2) - dt(1)


def stats_summary(st):
    """What is compared of one [mean, sd, zmin, zmax]: mean, sd and the de-normalised extremes mean + sd zmin, mean + sd zmax (the
    population's own min and max: well conditioned whatever sd is), then zmin and zmax."""
    st = f64(st)
    return np.array([st[0], st[1], st[0] + st[1] * st[2], st[0] + st[1] * st[3]]), st[2:4].copy()


def stats_errors(got, ref, scale, constant):
    """moments: worst |got - ref| of (mean, sd, de-normalised extremes) over `scale` = the population's largest |value|; z: worst error of
    (zmin, zmax) over the larger |z| of the reference.  A constant population (one value, however many times) has sd = 1e-12 and
    z = 0 / 1e-12 in exact arithmetic and roundoff / roundoff in fp32: there sd and z are left out (the GPU test bounds sd separately)."""
    gm, gz = stats_summary(got)
    rm, rz = stats_summary(ref)
    if not (np.isfinite(gm).all() and np.isfinite(gz).all()):
        return dict(moments=float('inf')) if constant else dict(moments=float('inf'), z=float('inf'))
    if constant:
        return dict(moments=float(np.abs(gm - rm)[[0, 2, 3]].max() / scale))
    return dict(moments=float(np.abs(gm - rm).max() / scale), z=float(np.abs(gz - rz).max() / np.abs(rz).max()))


# ---- feature rows ------------------------------------------------------------------------------------------------------------------
def float_bits_to_f32(m):
    """A float-valued numerical metadata column: the low 32 bits of the int64 table entry are a float32 bit pattern."""
    return (np.asarray(m, np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.float32)


def f32_to_float_bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)


def _table(params, idx, slip):
    # (a planted wrong pitch may run past the end of params: wrapped, any other number serves)
    return np.take(params, idx, mode='wrap') if slip.get('wrong_dim') else np.asarray(params)[idx]


def _scale_center(xraw, gamma, beta, dt, slip):
    """nar_model.py:887-907: x * gamma + beta per column."""
    x = xraw.astype(dt) * np.asarray(gamma).astype(dt)[None, :]
    return x if slip.get('beta_dropped') else x + np.asarray(beta).astype(dt)[None, :]


def ctx_rows(cat, num, desc, params, gamma, beta, dtype=np.float64, **slip):
    """User-context rows (nar_model.py:730-773 through :315-317) from the raw descriptor array [F, 5] int64 {kind, feat, sub, dim, offset of
    the table in params}: cat [n_cat, R] int64, num [n_num, R] float32.  Returns (xraw, xs): the gathered values - exact, whatever dtype
    is - and xraw * gamma + beta in dtype."""
    desc = np.asarray(desc, np.int64)
    R = (cat if cat is not None and len(cat) else num).shape[1]
    xraw = np.zeros((R, len(desc)), np.float32)
    for c, (kind, feat, sub, dim, off) in enumerate(desc):
        if kind == COL_OHE:
            xraw[:, c] = cat[feat] == sub
        elif kind == COL_EMB:
            xraw[:, c] = _table(params, off + cat[feat] * (dim + 1 if slip.get('wrong_dim') else dim) + sub, slip)
        elif kind == COL_NUM:
            xraw[:, c] = num[feat]
    return xraw, _scale_center(xraw, gamma, beta, dtype, slip)


def item_rows(ids, g1_begin, g2_begin, meta_cat, ace, rec_raw, nov_raw, stats, desc, params, gamma, beta, dtype=np.float64, **slip):
    """Item rows (nar_model.py:921-994): metadata one-hot bits / embedding rows / numerics (integer-valued, or - descriptor sub-field 1 - a
    float32 bit pattern), the article's content-embedding row, its trainable embedding row, normalised recency and novelty.  Row groups
    [0, g1_begin), [g1_begin, g2_begin), rest take stats[0], stats[1], stats[2] ([3, 8] = {recency, novelty} x {mean, sd, zmin, zmax}).
    Returns (xraw, xs, dyn): xraw in dtype (its gathered columns are exact fp32 values), xs = xraw * gamma + beta, dyn = the mask of
    the two normalised columns."""
    dt = dtype
    desc, ids = np.asarray(desc, np.int64), np.asarray(ids, np.int64)
    R = len(ids)
    grp = np.where(np.arange(R) < g1_begin, 0, np.where(np.arange(R) < g2_begin, 1, 2))
    if slip.get('neighbour_group'):
        grp = (grp + 1) % 3
    st = np.asarray(stats).reshape(3, 8)
    xraw = np.zeros((R, len(desc)), dt)
    for c, (kind, feat, sub, dim, off) in enumerate(desc):
        d = dim + 1 if slip.get('wrong_dim') else dim
        if kind == COL_OHE:
            xraw[:, c] = meta_cat[feat, ids] == sub
        elif kind == COL_EMB:
            xraw[:, c] = _table(params, off + meta_cat[feat, ids] * d + sub, slip)
        elif kind == COL_NUM:
            m = meta_cat[feat, ids]
            xraw[:, c] = float_bits_to_f32(m) if sub == 1 and not slip.get('float_bits_as_integer') else m.astype(np.float32)
        elif kind == COL_ACE:
            xraw[:, c] = ace[ids, sub]
        elif kind == COL_ITEMEMB:
            xraw[:, c] = _table(params, off + ids * d + sub, slip)
        elif kind == COL_RECENCY:
            xraw[:, c] = norm_apply(rec_raw, st[grp, 0:4], dt)
        elif kind == COL_NOVELTY:
            xraw[:, c] = norm_apply(nov_raw, st[grp, 0:4] if slip.get('novelty_stats_at_0') else st[grp, 4:8], dt)
    return xraw, _scale_center(xraw, gamma, beta, dt, slip), np.isin(desc[:, 0], (COL_RECENCY, COL_NOVELTY))


def item_segments(desc):
    """(segs [n, 6] int64, singles int32) of cham_item_assemble_lds from a descriptor array: runs of columns that come from one contiguous
    source row as {kind 0 ACE / 1 item embedding / 2 metadata embedding, first column, length, table offset, row pitch, feature}, the
    other columns in `singles`."""
    segs, singles, c = [], [], 0
    while c < len(desc):
        kind, feat, sub, dim, off = (int(v) for v in desc[c])
        if kind in (COL_ACE, COL_ITEMEMB, COL_EMB) and sub == 0:
            segs.append(((0, 1, 2)[(COL_ACE, COL_ITEMEMB, COL_EMB).index(kind)], c, dim, off, dim, feat if kind == COL_EMB else 0))
            c += dim
        else:
            singles.append(c)
            c += 1
    return np.asarray(segs, np.int64).reshape(-1, 6), np.asarray(singles, np.int32)


# ---- pure index arithmetic ---------------------------------------------------------------------------------------------------------
def row_weights(ids, neg_slot, pmax, pool):
    """The first batch's normalisation population (nar_model.py:1078-1084): w_ids[i] = 1 where ids[i] is not the pad item 0;
    w_slots[s] = how often pool slot s was sampled, s < pmax, where pool[s] is not the pad item.  Slots < 0 (masked click), == pmax (the
    zero-padding slot) and slots of a pad pool entry count for nothing; w_slots has pmax + 1 entries and the last stays 0."""
    w_ids = None if ids is None else (np.asarray(ids) != 0).astype(np.float32)
    w_slots = None
    if neg_slot is not None:
        s = np.asarray(neg_slot).reshape(-1)
        s = s[(s >= 0) & (s < pmax)]
        s = s[np.asarray(pool)[s] != 0]
        w_slots = np.bincount(s, minlength=pmax + 1).astype(np.float32)
    return w_ids, w_slots


def step_ints(ic, ln, pool, ets, max_ts, BT, pmax, seq_len, mask):
    """nar_model.py:217-248, 343, 356: ids_all = [clicked | positives | pool | pad item 0], ref_ts = [click time stamps | max_ts ...]."""
    ids_all = np.concatenate([ic[:BT], ln[:BT], pool[:pmax], [0]]).astype(np.int64)
    ref_ts = np.concatenate([ets[:BT], np.full(BT + pmax + 1, max_ts)]).astype(np.int64)
    return ids_all, ref_ts, np.asarray(seq_len, np.int32).copy(), np.asarray(mask, np.uint8)[:BT].copy()


def car_rows(neg_slot, BT, N, pmax, **slip):
    """(u, v) of every CAR row - BT clicked inputs, then BT (1 + N) candidates ordered (position, candidate), candidate 0 the positive:
    u = the position's row of U / Xc, v = the row of the item row set [clicked (BT) | positives (BT) | pool slots (pmax) | pad]."""
    slot = np.asarray(neg_slot).reshape(BT, N).astype(np.int64)
    s = np.where(slot < 0, 0 if slip.get('masked_slot_to_row_0') else pmax, slot)
    v = np.concatenate([(BT + np.arange(BT))[:, None], 2 * BT + s], 1)
    if slip.get('positive_from_pool'):
        v[:, 0] = 2 * BT + s[:, 0]
    u = np.repeat(np.arange(BT), N + 1)
    return np.concatenate([np.arange(BT), u]), np.concatenate([np.arange(BT), v.reshape(-1)])


def dense_rows(Xc, Xi, neg_slot, BT, N, pmax):
    u, v = car_rows(neg_slot, BT, N, pmax)
    return np.concatenate([np.asarray(Xc)[u], np.asarray(Xi)[v]], 1)


def combine_fwd(U, V, neg_slot, BT, N, pmax, dtype=np.float64, **slip):
    """PreCAR output in the CAR row order (nar_model.py:356-405, factorised): leaky_0.2(U[u] + V[v]); a slot of -1 (masked click) reads
    the pad row 2 BT + pmax."""
    dt = dtype
    u, v = car_rows(neg_slot, BT, N, pmax, **slip)
    z = np.asarray(U).astype(dt)[u] + np.asarray(V).astype(dt)[v]
    return np.where(z > 0, z, dt(0.01 if slip.get('slope_0_01') else LEAKY) * z)


# ---- dropout -----------------------------------------------------------------------------------------------------------------------
def dropout(x, keep, seed, step, site_first, site_rest, group, pos, T, row_begin, col_split, col_shift, **slip):
    """tf.nn.dropout of TF 1.12, y = x / keep_prob * mask, with the counter-based mask of include/chameleon_nar.h: element (row r, column
    c) belongs to position index r // group and sub = r % group; the position is q = pos[index] (or the index itself), session row
    b = row_begin + q // T and step t = q % T; logical column cl = c if c < col_split else c - col_shift; it is kept iff
        philox.rand32(cl, t, b, site, seed, step) < int(float64(float32(keep)) * 2**32),
    site = site_first for sub 0, site_rest + 256 (sub - 1) otherwise.  Kept: float32(x) / float32(keep) in fp32; dropped: +0.0.
    x [rows, cols]; returns (y float32, kept bool)."""
    x = np.asarray(x, np.float32)
    rows, cols = x.shape
    k32 = np.float32(keep)
    thr = int(np.float64(k32) * 4294967296.0)
    r = np.arange(rows, dtype=np.int64)
    pi, sub = r // group, r % group
    q = pi if pos is None else np.asarray(pos, np.int64)[pi]
    b = (0 if slip.get('row_begin_ignored') else row_begin) + q // T
    t = q % T
    n = np.where(sub == 0, 0, sub - 1)
    site = np.where(sub == 0, site_first, site_rest + (0 if slip.get('site_rest_without_n') else 256) * n)
    c = np.arange(cols, dtype=np.int64)
    cl = np.where(c < col_split, c, c - (0 if slip.get('col_shift_ignored') else col_shift))
    if slip.get('t_and_b_swapped'):
        t, b = b, t
    u = lambda a: np.asarray(a, np.int64).astype(np.uint64)
    kept = philox.rand32(u(cl)[None, :], u(t)[:, None], u(b)[:, None], u(site)[:, None], seed, step) < np.uint64(thr)
    y = np.where(kept, x * k32 if slip.get('times_keep') else x / k32, np.float32(0.0)).astype(np.float32)
    return y, kept


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
N_ITEMS, FOR_NORM = 5000, 20000


def catalog(seed=0, n_items=N_ITEMS, for_norm=FOR_NORM):
    """created [n_items] int64 ms: up to 60 days before T0, one item in eight up to 2 days AFTER it (an article newer than the reference
    time: relu); the pad item 0 created at 0.  pop_norm [n_items] float32 = float32(max(count / (sum + 1), 1 / for_norm)) of Zipf counts,
    as ClickedItemsState computes it: most of the catalog sits on the floor 1 / for_norm."""
    rng = np.random.default_rng(77 + seed)
    created = T0 - (rng.uniform(0.0, 60.0, n_items) * MS_PER_DAY).astype(np.int64)
    late = rng.random(n_items) < 0.125
    created[late] = T0 + (rng.uniform(0.0, 2.0, int(late.sum())) * MS_PER_DAY).astype(np.int64)
    created[0] = 0
    counts = np.floor(3.0e5 / np.arange(1, n_items + 1) ** 1.2)
    rng.shuffle(counts)
    pop = np.maximum(counts / (counts.sum() + 1.0), 1.0 / for_norm).astype(np.float32)
    return created, pop


DYN_R = (1, 255, 256, 257, 16411)
DYN_CASES = [(R, DEFAULT_BASES) for R in DYN_R] + [(257, OTHER_BASES), (16411, OTHER_BASES)]


def dyn_inputs(R, seed=0):
    """ids [R] with the pad id 0 in it, per-row reference time stamps within two hours after T0."""
    rng = np.random.default_rng(1000 + R + seed)
    created, pop = catalog(seed)
    ids = rng.integers(1, N_ITEMS, R).astype(np.int64)
    ids[rng.random(R) < 0.1] = 0
    if R > 1:
        ids[0], ids[-1] = 0, int(np.argmax(created))
    ref_ts = (T0 + rng.integers(0, 7200000, R)).astype(np.int64)
    return dict(ids=ids, ref_ts=ref_ts, created=created, pop_norm=pop)


STATS_N = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2000, 20000)
# population kinds of the buffer forms: the valid ids are a prefix and the rest zeros (the contract of the recent-clicks buffer)
BUFFER_KINDS = ('suffix_zeros', 'all_valid', 'single_valid')
# weight kinds of cham_norm_stats_from_rows
ROWS_KINDS = ('zero_one', 'repetition', 'single_positive')
MAX_TS = T0 + 3600000 + 12345


def buffer_inputs(n, kind, seed=0):
    """The first n slots of a recent-clicks buffer: ids >= 1, then zeros ('suffix_zeros': a third of the slots; 'single_valid': all but
    slot 0).  The buffer's articles were created before MAX_TS and are drawn by popularity, as clicks are: the population has
    real spread (sd above a twentieth of its largest value) and is not a run of one number (most of the CATALOG sits on the popularity floor)."""
    rng = np.random.default_rng(2000 + n + seed)
    created, pop = catalog(seed)
    old = np.flatnonzero(created[1:] < T0 - MS_PER_DAY / 4) + 1
    # a click lands on an article in proportion to its popularity: ~1000 distinct novelty values, a few per cent of the slots on the floor.
    # (Drawn uniformly from the catalog, four slots in five would hold the floor value; adding ONE number 16 000 times one after the
    # other in fp32 drifts by the same rounding error each time - 1.4e-4 of the sum - which says nothing about a reduction tree.)
    p = pop[old].astype(np.float64)
    ids = old[rng.choice(len(old), n, p=p / p.sum())].astype(np.int64)
    if kind == 'suffix_zeros':
        ids[n - n // 3:] = 0
    elif kind == 'single_valid':
        ids[1:] = 0
    return dict(ids=ids, created=created, pop_norm=pop, max_ts=MAX_TS)


def buffer_reference(inp, bases, dtype=np.float64, **slip):
    """[8] = stats of recency then of novelty over the valid (non-zero) slots."""
    ids = inp['ids']
    w = (ids != 0).astype(np.float32)
    rec = recency_raw(np.full(len(ids), inp['max_ts']), inp['created'][ids], bases[0], dtype)
    nov = novelty_raw(inp['pop_norm'][ids], bases[1], dtype)
    return np.concatenate([norm_stats(rec, w, dtype, **slip), norm_stats(nov, w, dtype, **slip)])


def rows_inputs(n, kind, seed=0, BTN=6400):
    """rec / nov [n] float32 raw values as cham_item_dynamic_raw leaves them, weights [n] float32.  'zero_one': a fifth of the rows are
    pads (weight 0) in the MIDDLE of the population, and they hold its extremes (the pad item: created at 0, popularity at the floor);
    'repetition': integer counts up to BTN (pool slots sampled many times), zeros among them; 'single_positive': one weight of 7."""
    rng = np.random.default_rng(3000 + n + seed)
    rec = rng.uniform(2.0, 16.0, n).astype(np.float32)
    nov = rng.uniform(0.5, 10.9, n).astype(np.float32)
    if kind == 'zero_one':
        w = (rng.random(n) >= 0.2).astype(np.float32)
    elif kind == 'repetition':
        w = np.floor(BTN ** rng.random(n)).astype(np.float32) * (rng.random(n) >= 0.2)
        w[rng.integers(0, n)] = BTN
    else:
        w = np.zeros(n, np.float32)
        w[n // 2] = 7.0
    if kind != 'single_positive':
        if not (w > 0).any():
            w[0] = 1.0
        if n > 2:
            w[n // 2], w[n // 2 - 1] = 0.0, 0.0
            rec[n // 2], rec[n // 2 - 1] = 37.2, 0.0
            nov[n // 2], nov[n // 2 - 1] = 10.97, 0.0
            if not (w > 0).any():
                w[0] = 1.0
    return dict(rec=rec, nov=nov, w=w)


CONST_VALUE = np.float32(7.3)
CONST_N = (1, 2000)


def constant_inputs(n):
    """The constant population: every value the same fp32 number, weights 1."""
    return dict(rec=np.full(n, CONST_VALUE, np.float32), nov=np.full(n, np.float32(10.965784)), w=np.ones(n, np.float32))


def is_constant(vals, w):
    x = np.asarray(vals)[np.asarray(w) > 0]
    return bool(x.min() == x.max())


def make_slots(rng, BT, N, pmax, pad_frac, hot, masked_frac):
    """[BT, N] int32 slot table as the sampler leaves it: per position N distinct pool slots (popularity-skewed; slots < hot sit in every
    position), a tail of ~pad_frac N entries replaced by the zero-padding slot pmax, masked_frac of the positions all -1."""
    slot = np.empty((BT, N), np.int32)
    w = 1.0 / np.arange(1, pmax + 1) ** 1.1
    w /= w.sum()
    for p in range(BT):
        s = rng.choice(pmax, size=N, replace=False, p=w)
        rest = s[~np.isin(s, np.arange(hot))]
        s = np.concatenate([np.arange(hot), rest])[:N].astype(np.int32)
        rng.shuffle(s)
        npad = int(round(pad_frac * N * rng.uniform(0.5, 1.5))) if pad_frac > 0 else 0
        if npad:
            s[N - min(npad, N):] = pmax
        slot[p] = s
    masked = rng.random(BT) < masked_frac
    slot[masked] = -1
    return slot, masked


# (BT, N, pmax, pad_frac, hot, masked_frac): N + 1 a multiple of 4 (3) and not (1, 9, 50, 200); masked clicks and pads in all but the first
SLOT_CASES = [(5, 1, 20, 0.0, 0, 0.0), (33, 3, 60, 0.3, 1, 0.2), (90, 9, 180, 0.6, 1, 0.2), (40, 50, 1000, 0.3, 2, 0.1), (7, 200, 4000, 0.05, 0, 0.3)]
COMBINE_C = (64, 128, 1024, 1280)
DENSE_F = (4, 72, 408, 1028)


def slot_inputs(case):
    BT, N, pmax, pad_frac, hot, masked_frac = SLOT_CASES[case]
    rng = np.random.default_rng(4000 + case)
    slot, masked = make_slots(rng, BT, N, pmax, pad_frac, hot, masked_frac)
    if masked_frac > 0:
        slot[BT // 2] = -1                       # at least one masked click ...
        slot[0, :] = np.arange(N) % pmax          # ... and a first position that is not, with a real slot first
        slot[0, N - 1] = pmax if pad_frac > 0 else slot[0, N - 1]
    pool = rng.integers(1, N_ITEMS, pmax).astype(np.int64)
    pool[pmax - max(1, pmax // 10):] = 0          # a pool shorter than pmax is zero padded (nar_model.py:1252)
    return dict(BT=BT, N=N, pmax=pmax, slot=slot, pool=pool)


def combine_inputs(case, C):
    s = slot_inputs(case)
    rng = np.random.default_rng(4100 + case + C)
    RV = 2 * s['BT'] + s['pmax'] + 1
    U = rng.standard_normal((s['BT'], C)).astype(np.float32)
    V = rng.standard_normal((RV, C)).astype(np.float32)
    V[rng.random(V.shape) < 0.01] = 0.0
    U[:, :4], V[:, :4] = np.float32(0.0), np.float32(-0.0)       # z = +-0 meets the kink
    U[:, 4:8] = -V[:s['BT'], 4:8]                                 # exact cancellation on the clicked-input rows
    return dict(s, U=U, V=V, C=C)


# (name, R): hand-built context schema: every kind cham_ctx_assemble takes, embedding widths 3, 6 and 7 (none divides 4), zero padding
CTX_R = (1, 257, 50000)


def ctx_schema():
    """(desc [F, 5], cardinalities of the categorical features, number of numerics, params length): one-hot (5), embedding dim 6 (card
    40), numeric, embedding dim 3 (card 11), one-hot (2), numeric, embedding dim 7 (card 300), then zero padding to a multiple of 4."""
    cols, off, cards = [], 16, []                       # (the tables do not start at params[0])
    def ohe(card):
        cards.append(card)
        cols.extend((COL_OHE, len(cards) - 1, s, card, 0) for s in range(card))
    def emb(card, dim):
        nonlocal off
        cards.append(card)
        cols.extend((COL_EMB, len(cards) - 1, s, dim, off) for s in range(dim))
        off += card * dim
    ohe(5); emb(40, 6); cols.append((COL_NUM, 0, 0, 1, 0)); emb(11, 3); ohe(2); cols.append((COL_NUM, 1, 0, 1, 0)); emb(300, 7)
    while len(cols) % 4:
        cols.append((COL_ZERO, 0, 0, 1, 0))
    return np.asarray(cols, np.int64), cards, 2, off + 8


def ctx_inputs(R, seed=0):
    desc, cards, n_num, n_params = ctx_schema()
    rng = np.random.default_rng(5000 + R + seed)
    cat = np.stack([rng.integers(0, c, R) for c in cards]).astype(np.int64)
    if R > 1:
        cat[:, 0], cat[:, -1] = 0, np.asarray(cards) - 1           # the first and the last row of every table
    num = rng.standard_normal((n_num, R)).astype(np.float32)
    return dict(cat=cat, num=num, desc=desc, params=rng.standard_normal(n_params).astype(np.float32), **gamma_beta(rng, len(desc)))


def gamma_beta(rng, F):
    return dict(gamma=(1.0 + 0.1 * rng.standard_normal(F)).astype(np.float32), beta=(0.05 * rng.standard_normal(F)).astype(np.float32))


ITEM_R = (7, 517, 1003)
ITEM_N, ITEM_D, ITEM_E = 900, 12, 9


def item_schema(n_items=ITEM_N, D=ITEM_D, E=ITEM_E):
    """(desc, cards, params length): one-hot (4), metadata embedding dim 6 (card 40), an INTEGER numeric, a FLOAT-BITS numeric (sub-field
    1), the ACE row (D), the item embedding (E), recency, novelty, zero padding.  cards: per metadata feature, 0 for a numeric."""
    cols, off = [(COL_OHE, 0, s, 4, 0) for s in range(4)], 8
    cols += [(COL_EMB, 1, s, 6, off) for s in range(6)]
    off += 40 * 6
    cols += [(COL_NUM, 2, 0, 1, 0), (COL_NUM, 3, 1, 1, 0)]
    cols += [(COL_ACE, 0, s, D, 0) for s in range(D)]
    cols += [(COL_ITEMEMB, 0, s, E, off) for s in range(E)]
    off += n_items * E
    cols += [(COL_RECENCY, 0, 0, 1, 0), (COL_NOVELTY, 0, 0, 1, 0)]
    while len(cols) % 4:
        cols.append((COL_ZERO, 0, 0, 1, 0))
    return np.asarray(cols, np.int64), off + 4


def item_inputs(R, seed=0):
    desc, n_params = item_schema()
    rng = np.random.default_rng(6000 + R + seed)
    fl = (rng.standard_normal(ITEM_N) * np.exp(rng.uniform(-8, 8, ITEM_N))).astype(np.float32)        # both signs, 1e-4 .. 1e4
    fl[:4] = [0.0, -0.0, 0.37, -2.5]
    meta = np.stack([rng.integers(0, 4, ITEM_N), rng.integers(0, 40, ITEM_N), rng.integers(-50, 3000, ITEM_N), f32_to_float_bits(fl)]).astype(np.int64)
    ids = rng.integers(0, ITEM_N, R).astype(np.int64)
    ids[:min(R, 4)] = np.arange(min(R, 4))
    rec = rng.uniform(0.0, 16.0, R).astype(np.float32)
    nov = rng.uniform(0.5, 10.97, R).astype(np.float32)
    # three DIFFERENT groups; within a group recency and novelty differ too (a neighbour's stats or offset 0 give other numbers)
    stats = np.array([[8.0, 3.5, -1.9, 2.2, 6.0, 2.5, -2.1, 1.9], [9.0, 3.0, -2.5, 2.4, 5.0, 2.0, -2.2, 2.9], [7.0, 4.0, -1.6, 2.1, 6.5, 3.0, -1.9, 1.4]],
                     np.float32)
    return dict(ids=ids, g1=R // 3, g2=2 * R // 3, meta_cat=meta, ace=rng.standard_normal((ITEM_N, ITEM_D)).astype(np.float32), rec=rec, nov=nov,
                stats=stats, desc=desc, params=rng.standard_normal(n_params).astype(np.float32), **gamma_beta(rng, len(desc)))


def item_args(inp):
    return (inp['ids'], inp['g1'], inp['g2'], inp['meta_cat'], inp['ace'], inp['rec'], inp['nov'], inp['stats'], inp['desc'], inp['params'],
            inp['gamma'], inp['beta'])


# (B, T, N, f_ctx, Fc, Fi, keep, compacted): the dense PreCAR input [ctx (Fc, f_ctx of them real) | item (Fi)] as the model drops it out
DROPOUT_KEEPS = (0.5, 0.8, 0.9)
DROPOUT_CASES = [(6, 5, 3, 10, 12, 16, 0.8, True), (6, 5, 3, 10, 12, 16, 0.5, False), (4, 3, 9, 7, 8, 20, 0.9, True), (8, 7, 2, 3, 4, 8, 0.8, False)]
DROPOUT_SEED, DROPOUT_STEP = 42, 1234567


def dropout_inputs(case, seed=0):
    """x of both launches of the model (nar_model forward: the BT clicked-input rows with group 1 and sites 16 / 16, the BT (1 + N)
    candidate rows with group N + 1 and sites 17 / 18), pos = the valid positions of ragged sessions when compacted (it drops positions)."""
    B, T, N, f_ctx, Fc, Fi, keep, compacted = DROPOUT_CASES[case]
    rng = np.random.default_rng(7000 + case + seed)
    if compacted:
        lens = rng.integers(1, T + 1, B)
        lens[0], lens[-1] = T, 1
        pos = np.concatenate([b * T + np.arange(lens[b]) for b in range(B)]).astype(np.int32)
    else:
        pos = None
    P = B * T if pos is None else len(pos)
    x_in = rng.standard_normal((P, Fc + Fi)).astype(np.float32)
    x_cand = rng.standard_normal((P * (N + 1), Fc + Fi)).astype(np.float32)
    x_in[0, :4] = [0.0, -0.0, 2e-38, -1e38]
    return dict(B=B, T=T, N=N, f_ctx=f_ctx, Fc=Fc, Fi=Fi, keep=keep, pos=pos, P=P, x_in=x_in, x_cand=x_cand)


def dropout_launches(inp, row_begin=0):
    """The keyword arguments of `dropout` for the two launches: (x, kwargs)."""
    common = dict(keep=inp['keep'], seed=DROPOUT_SEED, step=DROPOUT_STEP, pos=inp['pos'], T=inp['T'], row_begin=row_begin, col_split=inp['Fc'],
                  col_shift=inp['Fc'] - inp['f_ctx'])
    return [(inp['x_in'], dict(common, site_first=16, site_rest=16, group=1)), (inp['x_cand'], dict(common, site_first=17, site_rest=18, group=inp['N'] + 1))]


MARGIN = 8.0


# ---- the bounds of the GPU tests ------------------------------------------------------------------------------------------------------
def stats_cases():
    """(name, inputs, bases, constant): every population the GPU tests run the statistics on.  inputs: dict(rec, nov, w) - raw values
    given (cham_norm_stats_from_rows) - or dict(ids, created, pop_norm, max_ts) - the buffer forms."""
    out = []
    for n in STATS_N:
        for kind in BUFFER_KINDS:
            out.append(('buffer %s n=%d' % (kind, n), buffer_inputs(n, kind), DEFAULT_BASES if n != 1025 else OTHER_BASES))
        for kind in ROWS_KINDS:
            out.append(('rows %s n=%d' % (kind, n), rows_inputs(n, kind), None))
    for n in CONST_N:
        out.append(('rows constant n=%d' % n, constant_inputs(n), None))
    return out


def stats_eval(inp, bases, dt=np.float64, **slip):
    """[8] (recency then novelty), the populations' scales [2] and whether each is constant."""
    if 'ids' in inp:
        st = buffer_reference(inp, bases, dt, **slip)
        ids = inp['ids']
        w = (ids != 0).astype(np.float32)
        vals = [recency_raw(np.full(len(ids), inp['max_ts']), inp['created'][ids], bases[0]), novelty_raw(inp['pop_norm'][ids], bases[1])]
    else:
        w, vals = inp['w'], [inp['rec'], inp['nov']]
        st = np.concatenate([norm_stats(v, w, dt, **slip) for v in vals])
    return st, [float(np.abs(f64(v)[w > 0]).max()) for v in vals], [is_constant(v, w) for v in vals]


def stats_case_errors(got8, ref8, scales, consts):
    worst = {}
    for h in range(2):
        for k, e in stats_errors(got8[4 * h:4 * h + 4], ref8[4 * h:4 * h + 4], scales[h], consts[h]).items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


def item_errors(got, ref):
    """got, ref = (xraw, xs, dyn) of item_rows: the normalised columns and xs relative to their array's max; the gathered columns exact."""
    (gr, gs, dyn), (rr, rs, _) = got, ref
    return {'dyn': rel_err(gr[:, dyn], rr[:, dyn]), 'xs': rel_err(gs, rs),
            'static': 0.0 if np.array_equal(f64(gr[:, ~dyn]), f64(rr[:, ~dyn])) else float('inf')}


@functools.lru_cache(maxsize=None)
def fp32_cpu_errors():
    """Worst fp32-CPU error per compared array over the GPU tests' cases."""
    worst = {}

    def note(group, errs):
        for k, e in errs.items():
            worst[group + '.' + k] = max(worst.get(group + '.' + k, 0.0), e)
    for R, bases in DYN_CASES:
        inp = dyn_inputs(R)
        cr, pn = inp['created'][inp['ids']], inp['pop_norm'][inp['ids']]
        note('dyn', dict(rec=rel_err(recency_raw(inp['ref_ts'], cr, bases[0], np.float32), recency_raw(inp['ref_ts'], cr, bases[0])),
                         nov=rel_err(novelty_raw(pn, bases[1], np.float32), novelty_raw(pn, bases[1]))))
    for name, inp, bases in stats_cases():
        ref, scales, consts = stats_eval(inp, bases)
        note('stats', stats_case_errors(stats_eval(inp, bases, np.float32)[0], ref, scales, consts))
    for R in CTX_R:
        inp = ctx_inputs(R)
        note('ctx', dict(xs=rel_err(ctx_rows(dtype=np.float32, **inp)[1], ctx_rows(**inp)[1])))
    for R in ITEM_R:
        inp = item_inputs(R)
        e = item_errors(item_rows(*item_args(inp), dtype=np.float32), item_rows(*item_args(inp)))
        assert e.pop('static') == 0.0
        note('item', e)
    return worst


def gpu_bounds():
    """k per compared array: MARGIN x the worst fp32-CPU error of the same formula at the same inputs."""
    return {k: MARGIN * e for k, e in fp32_cpu_errors().items()}
