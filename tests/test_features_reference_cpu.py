"""The bounds of tests/test_feature_frontend_gpu.py, tests/test_combine_gpu.py and the float-bits case of tests/test_features_gpu.py can
fail, and where they come from (no GPU here).

For every function of tests/features_reference.py:
  * an independent restatement equals it to 1e-12: the oracle's _recency / _novelty / _normalize_values (recency_raw, novelty_raw, norm_stats
    and norm_apply chained) and _dropout, evaluated in float64; np.average / np.cov over the population repeated by its integer weights;
    concatenations of one-hot / table / numeric blocks for the feature rows; python loops for the index arithmetic;
  * evaluated in fp32 at the GPU tests' own inputs (the sums of norm_stats one element after the other) it gives the fp32-CPU error per
    compared array; `gpu_bounds()` = 8 x the worst of them over the cases, the k of the GPU tests' max |hip - ref| <= k max |ref|;
  * each slip, evaluated in float64 (so that nothing but the slip differs), moves some compared array by at least 10 k; where the
    arithmetic leaves no freedom (gathers, index arithmetic, the dropout mask and its one fp32 division, the combine's one addition and
    one multiplication) the comparison is bit-exact and a slip has to change the output outright.

fp32-CPU error per array, worst over the GPU tests' cases (k is 8 x these):
    dyn      recency 2.5e-7  novelty 1.1e-7
    stats    moments (mean, sd, de-normalised extremes over the largest |value|) 1.9e-5  zmin / zmax 4.0e-5  (up to 20 000 terms added
             one after the other; the kernel's 1024-way tree is far better)
    rows     context xs 6.1e-8   item: normalised columns 2.5e-7  xs 6.4e-8
Slips: 4 raw recency / novelty (natural log on both), 4 statistics, 5 item / context rows, 5 dropout, 3 combine.
"""
import os
import re

import numpy as np
import pytest
import torch

from oracle import philox
from oracle.nar_oracle import NAROracle
from tests import features_reference as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the bounds of the GPU tests: features_reference.fp32_cpu_errors / gpu_bounds --------------------------------------------------------
stats_cases, stats_eval, stats_case_errors, item_errors = F.stats_cases, F.stats_eval, F.stats_case_errors, F.item_errors
fp32_cpu_errors, gpu_bounds = F.fp32_cpu_errors, F.gpu_bounds


def test_fp32_evaluation_gives_the_bounds():
    e = fp32_cpu_errors()
    print({k: float('%.2e' % v) for k, v in e.items()})
    assert all(0 < v < 1e-4 for v in e.values()), e          # fp32 roundoff class: the bounds are 8 x these
    assert set(gpu_bounds()) == set(e) == {'dyn.rec', 'dyn.nov', 'stats.moments', 'stats.z', 'ctx.xs', 'item.dyn', 'item.xs'}


def test_exact_operations_are_exact_in_fp32():
    """The gathers and the index arithmetic have error 0 (the GPU comparison is array_equal): evaluated in fp32 they equal float64."""
    for R in F.CTX_R[:2]:
        inp = F.ctx_inputs(R)
        assert np.array_equal(F.ctx_rows(dtype=np.float32, **inp)[0], F.ctx_rows(**inp)[0])
    inp = F.combine_inputs(1, 64)
    # the combine: one addition and one multiplication per element - correctly rounded operations have one result, so the GPU test asks
    # for the bits of the fp32 evaluation (which is within half an ulp per operation of float64)
    a = (inp['U'], inp['V'], inp['slot'], inp['BT'], inp['N'], inp['pmax'])
    got, ref = F.combine_fwd(*a, dtype=np.float32), F.combine_fwd(*a)
    assert got.dtype == np.float32 and F.rel_err(got, ref) < 2.0 ** -22


# ---- inputs look like the real ones ---------------------------------------------------------------------------------------------------
def test_inputs_follow_the_input_rules():
    created, pop = F.catalog()
    assert (created[1:] > 1.49e12).all() and (created > F.T0).mean() > 0.05 and created[0] == 0
    assert pop.min() == np.float32(1.0 / F.FOR_NORM) and (pop == pop.min()).mean() > 0.5 and pop.max() > 0.05
    for R, _ in F.DYN_CASES:
        inp = F.dyn_inputs(R)
        assert inp['ref_ts'].min() >= F.T0 and (R == 1 or ((inp['ids'] == 0).any() and (inp['created'][inp['ids']] > inp['ref_ts']).any()))
    for name, inp, bases in stats_cases():
        ref, scales, consts = stats_eval(inp, bases)
        if 'ids' in inp:
            ids = inp['ids']
            nv = int((ids != 0).sum())
            assert nv >= 1 and (ids[:nv] != 0).all() and not ids[nv:].any(), name          # valid entries are a prefix
        for h in range(2):
            if not consts[h] and len(inp.get('w', inp.get('ids'))) >= 63:          # (two numbers have the spread they have)
                assert ref[4 * h + 1] > 0.02 * scales[h], (name, ref)          # real spread: 1 / sd does not amplify roundoff
    seen = set()
    for n in F.STATS_N:
        for kind in F.ROWS_KINDS:
            w = F.rows_inputs(n, kind)['w']
            assert (w > 0).any() and np.array_equal(w, np.round(w))
            if kind == 'zero_one' and n > 2:
                mid = np.flatnonzero(w == 0)
                assert ((mid > 0) & (mid < n - 1)).any()          # zero weights in the MIDDLE
            if kind == 'repetition':
                seen.add(float(w.max()))
            if kind == 'single_positive':
                assert (w > 0).sum() == 1
    assert seen == {6400.0}
    for case in range(len(F.SLOT_CASES)):
        s = F.slot_inputs(case)
        if F.SLOT_CASES[case][5] > 0:
            assert (s['slot'] == -1).any() and (s['slot'] == s['pmax']).any()
        assert (s['pool'] == 0).any() and (s['pool'][s['slot'][(s['slot'] >= 0) & (s['slot'] < s['pmax'])]] == 0).any() or s['N'] == 1
    assert {c[1] + 1 for c in F.SLOT_CASES} == {2, 4, 10, 51, 201}


# ---- the references against independent restatements ---------------------------------------------------------------------------------
def _oracle(created, bases, for_norm, keep=1.0, dt=torch.float64):
    o = object.__new__(NAROracle)
    o.p = dict(elapsed_days_smooth_log_base=bases[0], popularity_smooth_log_base=bases[1], recent_clicks_for_normalization=for_norm,
               dropout_keep_prob=keep)
    o.dt, o.seed, o._train = dt, F.DROPOUT_SEED, True
    o.meta = dict(created_at_ts=torch.from_numpy(created))
    return o


@pytest.mark.parametrize("bases", [F.DEFAULT_BASES, F.OTHER_BASES])
@pytest.mark.parametrize("n_valid", [0, 1, 700])
def test_dynamic_features_equal_the_oracle_in_float64(bases, n_valid):
    """recency_raw / novelty_raw -> norm_stats -> norm_apply against NAROracle._recency / _novelty: with a buffer (the population is its
    valid prefix, at the batch's max time stamp) and without (the call's own non-pad ids with repetition = 0 / 1 weights)."""
    inp = F.dyn_inputs(257)
    ids, ref_ts, created, pop = inp['ids'], inp['ref_ts'], inp['created'], inp['pop_norm']
    buf = np.zeros(1000, np.int64)
    buf[:n_valid] = F.buffer_inputs(1000, 'all_valid')['ids'][:n_valid]
    o = _oracle(created, bases, 500)
    t = torch.from_numpy
    want_r = o._recency(t(ids), t(ref_ts)[:, None], t(buf)).numpy()[:, 0]
    want_n = o._novelty(t(ids), t(buf), t(pop).double()).numpy()[:, 0]
    rec, nov = F.recency_raw(ref_ts, created[ids], bases[0]), F.novelty_raw(pop[ids], bases[1])
    if n_valid == 0:
        w = (ids != 0).astype(np.float32)
        st_r, st_n = F.norm_stats(rec, w), F.norm_stats(nov, w)
    else:
        last = buf[:min(n_valid, 500)]
        st_r = F.norm_stats(F.recency_raw(np.full(len(last), ref_ts.max()), created[last], bases[0]))
        st_n = F.norm_stats(F.novelty_raw(pop[last], bases[1]))
    if n_valid == 1:
        # one element: sd = 1e-12 and z = (x - mean) / 1e-12 ~ 1e13; the scaled value is z / 2e-24: compare what is finite in both
        assert st_r[1] == 1e-12 and st_r[2] == 0.0 and st_r[3] == 0.0
        return
    assert F.rel_err(F.norm_apply(rec, st_r), want_r) < 1e-12 and F.rel_err(F.norm_apply(nov, st_n), want_n) < 1e-12
    # ... and NAROracle._normalize_values alone, on the statistics' own population: its extremes map to -1 and 1
    live = ids != 0
    if n_valid == 0:
        got = F.norm_apply(rec[live], st_r)
        assert abs(got.min() + 1) < 1e-12 and abs(got.max() - 1) < 1e-12
        assert F.rel_err(got, NAROracle._normalize_values(t(rec[live]), t(rec[live])).numpy()) < 1e-12


@pytest.mark.parametrize("kind", ['repetition', 'zero_one'])
@pytest.mark.parametrize("n", [2, 65, 1025])
def test_norm_stats_equal_moments_of_the_repeated_population(kind, n):
    inp = F.rows_inputs(n, kind, BTN=40)
    x, w = F.f64(inp['rec']), inp['w'].astype(np.int64)
    rep = np.repeat(x, w)
    st = F.norm_stats(inp['rec'], inp['w'])
    assert abs(st[0] - np.average(x, weights=w)) < 1e-12 * abs(st[0]) and abs(st[0] - rep.mean()) < 1e-12 * abs(st[0])
    var = float(np.cov(rep, bias=True)) if len(rep) > 1 else 0.0
    assert abs(st[1] - np.sqrt(var + 1e-24)) < 1e-12 * st[1]
    if rep.std() > 0:
        assert abs(st[2] - (rep.min() - rep.mean()) / rep.std()) < 1e-10 and abs(st[3] - (rep.max() - rep.mean()) / rep.std()) < 1e-10
    if len(rep) >= 2:
        assert F.rel_err(F.norm_stats(inp['rec'], inp['w'], sample_variance=True)[1], np.sqrt(float(np.cov(rep)))) < 1e-12


def test_feature_rows_equal_a_concatenation_of_blocks():
    """get_features (nar_model.py:730-773) builds a row by concatenating one_hot(x, cardinality), table[x] and the numeric column per
    feature; the references walk raw descriptors column by column."""
    inp = F.ctx_inputs(257)
    cat, num, P = inp['cat'], inp['num'], torch.from_numpy(inp['params']).double()
    oh = lambda x, c: torch.nn.functional.one_hot(torch.from_numpy(x), c).double()
    tab = lambda off, card, dim, x: P[off:off + card * dim].view(card, dim)[torch.from_numpy(x)]
    blocks = [oh(cat[0], 5), tab(16, 40, 6, cat[1]), torch.from_numpy(num[0]).double()[:, None], tab(256, 11, 3, cat[2]), oh(cat[3], 2),
              torch.from_numpy(num[1]).double()[:, None], tab(289, 300, 7, cat[4])]
    want = torch.cat(blocks, 1)
    want = torch.cat([want, torch.zeros(257, len(inp['desc']) - want.shape[1]).double()], 1).numpy()
    xraw, xs = F.ctx_rows(**inp)
    assert len(inp['desc']) % 4 == 0 and np.array_equal(F.f64(xraw), want)
    assert F.rel_err(xs, want * F.f64(inp['gamma']) + F.f64(inp['beta'])) < 1e-12
    it = F.item_inputs(517)
    ids, meta, P = it['ids'], it['meta_cat'], torch.from_numpy(it['params']).double()
    grp = np.where(np.arange(517) < it['g1'], 0, np.where(np.arange(517) < it['g2'], 1, 2))
    st = F.f64(it['stats'])[grp]
    z = lambda x, s: (((F.f64(x) - s[:, 0]) / s[:, 1] - s[:, 2] + 1e-24) / np.maximum(s[:, 3] - s[:, 2], 2e-24)) * 2 - 1
    fl = meta[3, ids].astype(np.int32).view(np.float32)               # the stored bit pattern read back
    blocks = [oh(meta[0, ids], 4), tab(8, 40, 6, meta[1, ids]), torch.from_numpy(meta[2, ids]).double()[:, None], torch.from_numpy(F.f64(fl))[:, None],
              torch.from_numpy(it['ace']).double()[ids], tab(248, F.ITEM_N, F.ITEM_E, ids), torch.from_numpy(z(it['rec'], st[:, :4]))[:, None],
              torch.from_numpy(z(it['nov'], st[:, 4:]))[:, None]]
    want = torch.cat(blocks, 1)
    want = torch.cat([want, torch.zeros(517, len(it['desc']) - want.shape[1]).double()], 1).numpy()
    xraw, xs, dyn = F.item_rows(*F.item_args(it))
    assert dyn.sum() == 2 and F.rel_err(xraw, want) < 1e-12 and np.array_equal(xraw[:, ~dyn], want[:, ~dyn])
    assert F.rel_err(xs, want * F.f64(it['gamma']) + F.f64(it['beta'])) < 1e-12
    assert not np.array_equal(fl, np.round(fl)) and (np.abs(fl) < 1e-3).any() and (fl < 0).any()
    # the segment form of the same descriptors covers every column once
    segs, singles = F.item_segments(it['desc'])
    cover = np.concatenate([np.arange(s[1], s[1] + s[2]) for s in segs] + [singles])
    assert sorted(cover.tolist()) == list(range(len(it['desc']))) and [int(s[0]) for s in segs] == [2, 0, 1]


def test_index_arithmetic_equals_python_loops():
    for case in range(len(F.SLOT_CASES)):
        s = F.slot_inputs(case)
        BT, N, pmax, slot, pool = s['BT'], s['N'], s['pmax'], s['slot'], s['pool']
        ids = np.concatenate([pool[:BT] if BT <= pmax else np.resize(pool, BT), np.zeros(3, np.int64)])
        w_ids, w_slots = F.row_weights(ids, slot, pmax, pool)
        want = np.zeros(pmax + 1, np.float32)
        for v in slot.reshape(-1):
            if 0 <= v < pmax and pool[v] != 0:
                want[v] += 1
        assert np.array_equal(w_slots, want) and want[pmax] == 0 and np.array_equal(w_ids, [1.0 if i else 0.0 for i in ids])
        assert F.row_weights(None, slot, pmax, pool)[0] is None and F.row_weights(ids, None, pmax, pool)[1] is None
        inp = F.combine_inputs(case, 64)
        U, V = F.f64(inp['U']), F.f64(inp['V'])
        rows = []
        for r in range(BT):
            rows.append(U[r] + V[r])
        for bt in range(BT):
            for c in range(N + 1):
                sl = pmax if c and slot[bt, c - 1] < 0 else (slot[bt, c - 1] if c else None)
                rows.append(U[bt] + (V[BT + bt] if c == 0 else V[2 * BT + sl]))
        z = np.stack(rows)
        assert np.array_equal(F.combine_fwd(inp['U'], inp['V'], slot, BT, N, pmax), np.where(z > 0, z, 0.2 * z))
        Xc, Xi = inp['U'][:, :8], inp['V'][:, :12]
        u, v = F.car_rows(slot, BT, N, pmax)
        assert np.array_equal(F.dense_rows(Xc, Xi, slot, BT, N, pmax), np.stack([np.concatenate([Xc[a], Xi[b]]) for a, b in zip(u, v)]))
        assert v.max() <= 2 * BT + pmax and (v[BT:].reshape(BT, N + 1)[:, 0] == BT + np.arange(BT)).all()
    ic, ln, pool, ets = np.arange(10, 15), np.arange(20, 25), np.arange(30, 37), np.arange(40, 45)
    ids_all, ref_ts, sl, mk = F.step_ints(ic, ln, pool, ets, 99, 5, 7, np.array([3, 2], np.int32), np.array([1, 0, 1, 1, 0], np.uint8))
    assert ids_all.tolist() == list(range(10, 15)) + list(range(20, 25)) + list(range(30, 37)) + [0]
    assert ref_ts.tolist() == list(range(40, 45)) + [99] * 13 and sl.tolist() == [3, 2] and mk.tolist() == [1, 0, 1, 1, 0]
    assert [a.tolist() for a in F.step_ints(ic, ln, pool, ets, 99, 0, 0, np.zeros(0, np.int32), np.zeros(0, np.uint8))[:2]] == [[0], [99]]


@pytest.mark.parametrize("keep", F.DROPOUT_KEEPS)
def test_dropout_equals_the_oracle(keep):
    """[B, T, F] with one site and [B, T, N, F] with site + 256 n through NAROracle._dropout in fp32 (one correctly rounded division: the
    same bits), against the flat [rows, cols] form with group 1 / group N + 1."""
    B, T, N, Fw = 5, 4, 3, 11
    rng = np.random.default_rng(int(keep * 100))
    x3 = rng.standard_normal((B, T, Fw)).astype(np.float32)
    x4 = rng.standard_normal((B, T, N, Fw)).astype(np.float32)
    o = _oracle(np.zeros(1, np.int64), F.DEFAULT_BASES, 1, keep, torch.float32)
    want3 = o._dropout(torch.from_numpy(x3), 17, F.DROPOUT_STEP).numpy()
    want4 = o._dropout(torch.from_numpy(x4), 18, F.DROPOUT_STEP).numpy()
    cand = np.concatenate([x3[:, :, None, :], x4], 2).reshape(B * T * (N + 1), Fw)
    y, kept = F.dropout(cand, keep, F.DROPOUT_SEED, F.DROPOUT_STEP, 17, 18, N + 1, None, T, 0, Fw, 0)
    y = y.reshape(B, T, N + 1, Fw)
    # (the oracle's x / keep * 0 keeps the sign of x on a dropped element; tf.nn.dropout's and the kernel's zero is +0.0: equal as numbers)
    assert np.array_equal(y[:, :, 0], want3) and np.array_equal(y[:, :, 1:], want4)
    assert not y.reshape(-1, Fw)[~kept].view(np.uint32).any(), "a dropped element is not +0.0"
    assert abs(kept.mean() - keep) < 0.05 and F.same_bits(y[kept.reshape(y.shape)], (cand / np.float32(keep))[kept])
    # compaction, a row shard and the padded [ctx | item] column layout are relabellings of the same coordinates
    pos = np.array([0, 1, 5, 8, 9, 10, 17], np.int32)
    sub = np.concatenate([np.arange(p * (N + 1), (p + 1) * (N + 1)) for p in pos])
    y2, _ = F.dropout(cand[sub], keep, F.DROPOUT_SEED, F.DROPOUT_STEP, 17, 18, N + 1, pos, T, 0, Fw, 0)
    assert F.same_bits(y2, y.reshape(-1, Fw)[sub])
    half = (B // 2) * T * (N + 1)
    y3, _ = F.dropout(cand[half:], keep, F.DROPOUT_SEED, F.DROPOUT_STEP, 17, 18, N + 1, None, T, B // 2, Fw, 0)
    assert F.same_bits(y3, y.reshape(-1, Fw)[half:])
    padded = np.concatenate([cand[:, :4], np.zeros((len(cand), 2), np.float32), cand[:, 4:]], 1)
    y4, _ = F.dropout(padded, keep, F.DROPOUT_SEED, F.DROPOUT_STEP, 17, 18, N + 1, None, T, 0, 6, 2)
    assert F.same_bits(y4[:, :4], y.reshape(-1, Fw)[:, :4]) and F.same_bits(y4[:, 6:], y.reshape(-1, Fw)[:, 4:])
    assert int(np.float64(np.float32(keep)) * 2 ** 32) == int(float(np.float32(keep)) * 4294967296.0)
    r = philox.rand32(np.uint64(3), np.uint64(2), np.uint64(1), np.uint64(18 + 256 * 2), F.DROPOUT_SEED, F.DROPOUT_STEP)
    assert bool(r < np.uint64(int(np.float64(np.float32(keep)) * 2 ** 32))) == bool(kept.reshape(B, T, N + 1, Fw)[1, 2, 3, 3])


# ---- the bounds can fail --------------------------------------------------------------------------------------------------------------
DYN_SLIPS = {
    # (the one-row case: one article, older than its reference time, whose age may be a multiple of the fp32 spacing of a time stamp)
    'int64_subtraction': lambda R, bases: R > 1,
    'natural_log': lambda R, bases: True,
    'log_x': lambda R, bases: R > 1,
    'relu_dropped': lambda R, bases: R > 1,
}


@pytest.mark.parametrize("R,bases", F.DYN_CASES)
def test_every_dynamic_slip_breaks_the_bound_tenfold(R, bases):
    inp, k = F.dyn_inputs(R), gpu_bounds()
    cr, pn = inp['created'][inp['ids']], inp['pop_norm'][inp['ids']]
    ref = F.recency_raw(inp['ref_ts'], cr, bases[0])
    worst = {s: F.rel_err(F.recency_raw(inp['ref_ts'], cr, bases[0], **{s: True}), ref) / k['dyn.rec'] for s, ok in DYN_SLIPS.items() if ok(R, bases)}
    worst['natural_log (novelty)'] = F.rel_err(F.novelty_raw(pn, bases[1], natural_log=True), F.novelty_raw(pn, bases[1])) / k['dyn.nov']
    # another base than the one asked for is the same kind of slip: the defaults where 1.7 / 3.0 were set
    if bases != F.DEFAULT_BASES:
        worst['default bases'] = F.rel_err(F.recency_raw(inp['ref_ts'], cr, F.DEFAULT_BASES[0]), ref) / k['dyn.rec']
    print((R, bases), {a: float('%.3g' % b) for a, b in worst.items()})
    assert min(worst.values()) >= 10, worst


# name -> applies to this population (name of the case, weights, constant)?
STATS_SLIPS = {
    # sd grows by 1 / (2 sum w) of itself: visible against a bound of ~1e-4 of the population's max where sum w is small
    'sample_variance': lambda name, w, const: not const and 1 < float(w.sum()) <= 64,
    'sd_without_epsilon': lambda name, w, const: const and 'constant' in name,
    'minmax_over_zero_weights': lambda name, w, const: not const and 'zero_one' in name and len(w) > 2,
    'weights_ignored_in_mean': lambda name, w, const: not const and 'repetition' in name and (w > 0).sum() > 1 and w[w > 0].min() != w.max(),
}


def test_every_stats_slip_breaks_the_bound_tenfold():
    k, tried = gpu_bounds(), {}
    for name, inp, bases in stats_cases():
        ref, scales, consts = stats_eval(inp, bases)
        w = inp['w'] if 'w' in inp else (inp['ids'] != 0).astype(np.float32)
        for s, applies in STATS_SLIPS.items():
            if applies(name, w, all(consts)):
                e = stats_case_errors(stats_eval(inp, bases, **{s: True})[0], ref, scales, consts)
                ratio = max(e[a] / k['stats.' + a] for a in e)
                tried[s] = min(tried.get(s, float('inf')), ratio)
                assert ratio >= 10, (s, name, e)
    print({a: float('%.3g' % b) for a, b in tried.items()})
    assert set(tried) == set(STATS_SLIPS)


ROW_SLIPS = ('neighbour_group', 'novelty_stats_at_0', 'beta_dropped', 'wrong_dim', 'float_bits_as_integer')


@pytest.mark.parametrize("R", F.ITEM_R)
def test_every_row_slip_breaks_the_bound_tenfold(R):
    inp, k = F.item_inputs(R), gpu_bounds()
    ref = F.item_rows(*F.item_args(inp))
    for s in ROW_SLIPS:
        e = item_errors(F.item_rows(*F.item_args(inp), **{s: True}), ref)
        assert max(e['dyn'] / k['item.dyn'], e['xs'] / k['item.xs']) >= 10, (s, e)
        if s in ('wrong_dim', 'float_bits_as_integer'):
            assert e['static'] == float('inf'), s              # the exact comparison of the gathered columns fails too
    ci = F.ctx_inputs(257)
    cref = F.ctx_rows(**ci)
    for s in ('beta_dropped', 'wrong_dim'):
        got = F.ctx_rows(**ci, **{s: True})
        assert F.rel_err(got[1], cref[1]) >= 10 * k['ctx.xs'], s
        assert s == 'beta_dropped' or not np.array_equal(got[0], cref[0])


DROPOUT_SLIPS = ('site_rest_without_n', 't_and_b_swapped', 'row_begin_ignored', 'col_shift_ignored', 'times_keep')


@pytest.mark.parametrize("case", range(len(F.DROPOUT_CASES)))
def test_every_dropout_slip_changes_the_output(case):
    """Exact comparison: a slip has to change the mask (or the kept values) outright - in the candidate launch (group N + 1, two sites)
    of a row shard that does not begin at session 0."""
    inp = F.dropout_inputs(case)
    x, kw = F.dropout_launches(inp, row_begin=3)[1]
    y, kept = F.dropout(x, **kw)
    for s in DROPOUT_SLIPS:
        y2, kept2 = F.dropout(x, **kw, **{s: True})
        assert not F.same_bits(y, y2), s
        assert s == 'times_keep' or (kept != kept2).mean() > 0.05, s
    assert inp['Fc'] > inp['f_ctx'] and inp['N'] >= 2


COMBINE_SLIPS = {
    'masked_slot_to_row_0': lambda s: (s['slot'] < 0).any(),
    'positive_from_pool': lambda s: True,
    'slope_0_01': lambda s: True,
}


def test_every_combine_slip_changes_the_output():
    tried = set()
    for case in range(len(F.SLOT_CASES)):
        inp = F.combine_inputs(case, 64)
        a = (inp['U'], inp['V'], inp['slot'], inp['BT'], inp['N'], inp['pmax'])
        ref = F.combine_fwd(*a, dtype=np.float32)
        for s, applies in COMBINE_SLIPS.items():
            if applies(inp):
                assert not F.same_bits(F.combine_fwd(*a, dtype=np.float32, **{s: True}), ref), (s, case)
                tried.add(s)
    assert tried == set(COMBINE_SLIPS)


# ---- housekeeping ---------------------------------------------------------------------------------------------------------------------
# entry points that no test calls by name: reached through a wrapper class of the package, which a GPU test file drives
THROUGH_A_WRAPPER = {'cham_state_update': ('DeviceClickedItemsState', 'test_state_gpu.py')}


def _entry_points(path, stop=None):
    src = open(os.path.join(ROOT, "chameleon_recsys_amd", "csrc", path)).read()
    if stop is not None:
        src = src[:src.index('extern "C" int %s(' % stop)]
    return sorted(set(re.findall(r'extern "C" int (cham_\w+)\s*\(', src)))


def _class_source(path, cls):
    src = open(path).read()
    m = re.search(r"^class %s\b.*?(?=^class |\Z)" % cls, src, re.S | re.M)
    assert m, "%s has no class %s" % (path, cls)
    return m.group(0)


def test_every_entry_point_of_the_front_end_is_named_in_a_gpu_test():
    names = _entry_points("features.hip") + _entry_points("sampler.hip") + _entry_points("state.hip") + _entry_points("scorer.hip", stop="cham_mulpred_bwd")
    assert len(names) >= 25 and all(n in names for n in ('cham_dropout', 'cham_combine_fwd_b16', 'cham_neg_sample_dev', 'cham_state_update')), names
    tdir = os.path.join(ROOT, "tests")
    files = sorted(f for f in os.listdir(tdir) if re.fullmatch(r"test_\w+_gpu\.py", f)) + ["test_sampler.py"]
    text = {f: open(os.path.join(tdir, f)).read() for f in files}
    for n, (cls, tfile) in THROUGH_A_WRAPPER.items():            # checked whether or not a test also names the entry point itself
        assert n in names, n
        body = _class_source(os.path.join(ROOT, "chameleon_recsys_amd", "nar", "clicked_items_state.py"), cls)
        assert re.search(r"\blib\.%s\(" % n, body), "%s does not call %s" % (cls, n)
        assert re.search(r"\b%s\(" % cls, text[tfile]), "%s does not use %s" % (tfile, cls)
    missing = [n for n in names if n not in THROUGH_A_WRAPPER and not any(re.search(r"\b%s\b" % n, t) for t in text.values())]
    assert not missing, "entry points without a direct GPU test: %s" % missing
    assert len(THROUGH_A_WRAPPER) == 1
