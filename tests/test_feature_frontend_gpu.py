"""The head of a training step against the float64 references of tests/features_reference.py: cham_item_dynamic_raw (and
cham_set_log_bases), cham_norm_stats_from_recent / _from_buffer / _from_buffer_dev / _from_rows, cham_row_weights, cham_step_ints / _dev,
cham_ctx_assemble, cham_dropout and cham_dense_rows.  (cham_item_assemble / _lds with a float-bits numeric column are next to their
schema tests in tests/test_features_gpu.py, the combine forward in tests/test_combine_gpu.py.)

Every output starts as NaN (integers: -7) inside an allocation with at least one row of the same fill on either side, which must come
back unchanged; every launch is made twice and must repeat bit for bit.  Bounds are 8 x the error of the same formula in fp32 on the CPU
at the same inputs (tests/features_reference.py: `gpu_bounds`; tests/test_features_reference_cpu.py: the slips that break them tenfold), relative to the array's
max; every bounded comparison prints kernel error / fp32-CPU error.  Exact, compared with array_equal: gathers, counts, index
arithmetic, the dropout mask and its kept values (one correctly rounded fp32 division), by-value against _dev.

"""
import numpy as np
import pytest
import torch

from tests import features_reference as F
from tests.features_gpu_helpers import Out, _dev, _lib_, _note, _st, _twice
from tests.features_reference import gpu_bounds, stats_eval

pytestmark = pytest.mark.gpu


# ---- raw recency / novelty ------------------------------------------------------------------------------------------------------------
def _dyn_run(gpu, lib, inp):
    from chameleon_recsys_amd._lib import check
    R = len(inp['ids'])
    d = {k: _dev(gpu, inp[k]) for k in ('ids', 'ref_ts', 'created', 'pop_norm')}

    def run():
        rec, nov = Out(gpu, (R,)), Out(gpu, (R,))
        check(lib.cham_item_dynamic_raw(d['ids'].data_ptr(), d['ref_ts'].data_ptr(), R, d['created'].data_ptr(), d['pop_norm'].data_ptr(), rec.ptr(),
                                        nov.ptr(), _st()), "cham_item_dynamic_raw")
        return rec.numpy(), nov.numpy()
    return _twice(run)


@pytest.mark.parametrize("R,bases", F.DYN_CASES)
def test_item_dynamic_raw_matches_float64(gpu, R, bases):
    lib, k = _lib_(), gpu_bounds()
    inp = F.dyn_inputs(R)
    print("\nR %d bases %s" % (R, bases))
    try:
        assert lib.cham_set_log_bases(*bases) == 0
        rec, nov = _dyn_run(gpu, lib, inp)
    finally:
        assert lib.cham_set_log_bases(*F.DEFAULT_BASES) == 0
    _note('dyn.rec', F.rel_err(rec, F.recency_raw(inp['ref_ts'], inp['created'][inp['ids']], bases[0])), k['dyn.rec'])
    _note('dyn.nov', F.rel_err(nov, F.novelty_raw(inp['pop_norm'][inp['ids']], bases[1])), k['dyn.nov'])
    late = inp['created'][inp['ids']].astype(np.float32) >= inp['ref_ts'].astype(np.float32)
    assert not rec[late].view(np.uint32).any(), "an article newer than its reference time has recency +0.0"


def test_invalid_log_bases_are_refused_and_leave_the_previous_ones(gpu):
    lib, k = _lib_(), gpu_bounds()
    inp = F.dyn_inputs(257)
    try:
        assert lib.cham_set_log_bases(*F.OTHER_BASES) == 0
        for bad in ((1.0, 2.0), (1.3, 1.0), (0.0, 2.0), (1.3, 0.0), (-1.3, 2.0), (1.3, -2.0), (float('nan'), 2.0), (1.3, float('nan'))):
            assert lib.cham_set_log_bases(*bad) == -22, bad
        rec, nov = _dyn_run(gpu, lib, inp)
    finally:
        assert lib.cham_set_log_bases(*F.DEFAULT_BASES) == 0
    assert F.rel_err(rec, F.recency_raw(inp['ref_ts'], inp['created'][inp['ids']], F.OTHER_BASES[0])) <= k['dyn.rec']
    assert F.rel_err(nov, F.novelty_raw(inp['pop_norm'][inp['ids']], F.OTHER_BASES[1])) <= k['dyn.nov']
    rec, nov = _dyn_run(gpu, lib, inp)
    assert F.rel_err(rec, F.recency_raw(inp['ref_ts'], inp['created'][inp['ids']], F.DEFAULT_BASES[0])) <= k['dyn.rec']
    bad = Out(gpu, (4,))
    assert lib.cham_item_dynamic_raw(None, bad.ptr(), 4, bad.ptr(), bad.ptr(), bad.ptr(), bad.ptr(), _st()) == -22
    assert lib.cham_item_dynamic_raw(bad.ptr(), bad.ptr(), 0, bad.ptr(), bad.ptr(), bad.ptr(), bad.ptr(), _st()) == -22


# ---- normalisation statistics ---------------------------------------------------------------------------------------------------------
def _check_stats(name, got8, inp, bases, k):
    """mean, sd, the de-normalised extremes and - where the population is not constant - zmin and zmax, per half (recency, novelty)."""
    ref, scales, consts = stats_eval(inp, bases)
    for h, half in enumerate(('rec', 'nov')):
        g, r = got8[4 * h:4 * h + 4], ref[4 * h:4 * h + 4]
        e = F.stats_errors(g, r, scales[h], consts[h])
        _note('%s stats.moments %s' % (name, half), e['moments'], k['stats.moments'])
        if consts[h]:
            # sd = sqrt(var + 1e-24) with var = the mean's own roundoff squared: no larger than the mean's allowed error (+ the 1e-12)
            assert 0 < float(g[1]) <= k['stats.moments'] * scales[h] + 1e-12, (name, half, g)
        else:
            _note('%s stats.z %s' % (name, half), e['z'], k['stats.z'])


@pytest.mark.parametrize("kind", F.BUFFER_KINDS)
@pytest.mark.parametrize("n", F.STATS_N)
def test_norm_stats_of_the_buffer_forms_match_float64(gpu, n, kind):
    """cham_norm_stats_from_buffer, _from_buffer_dev (bit-equal, max_ts through the step-scalars record) and _from_recent (the valid prefix
    handed over as a list) on a recent-clicks buffer whose valid ids are a prefix: zeros as a suffix, none, or all but one slot.  A
    single valid slot is a constant population: sd is 1e-12 and z = 0 / 1e-12 in exact arithmetic; zmin and zmax are not compared
    there (see test_norm_stats_of_a_constant_population)."""
    from chameleon_recsys_amd._lib import check
    lib, k = _lib_(), gpu_bounds()
    bases = F.DEFAULT_BASES if n != 1025 else F.OTHER_BASES
    inp = F.buffer_inputs(n, kind)
    ids, created, pop = _dev(gpu, inp['ids']), _dev(gpu, inp['created']), _dev(gpu, inp['pop_norm'])
    nv = int((inp['ids'] != 0).sum())
    rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
    check(lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, inp['max_ts'], 0.0, 0.0, 2, _st()), "cham_step_scalars_set")
    print("\nn %d %s (%d valid) bases %s" % (n, kind, nv, bases))

    def run(form):
        def go():
            scratch = Out(gpu, ((2 * nv if form == 'recent' else 3 * n),))
            stats = Out(gpu, (3, 8))
            if form == 'recent':
                check(lib.cham_norm_stats_from_recent(ids.data_ptr(), nv, inp['max_ts'], created.data_ptr(), pop.data_ptr(), scratch.ptr(), stats.ptr(),
                                                      _st()), "cham_norm_stats_from_recent")
            elif form == 'buffer':
                check(lib.cham_norm_stats_from_buffer(ids.data_ptr(), n, inp['max_ts'], created.data_ptr(), pop.data_ptr(), scratch.ptr(), stats.ptr(),
                                                      _st()), "cham_norm_stats_from_buffer")
            else:
                check(lib.cham_norm_stats_from_buffer_dev(ids.data_ptr(), n, rec.data_ptr(), created.data_ptr(), pop.data_ptr(), scratch.ptr(),
                                                          stats.ptr(), _st()), "cham_norm_stats_from_buffer_dev")
            out = stats.numpy()
            scratch.numpy()
            return (out,)
        return _twice(go)[0]
    try:
        assert lib.cham_set_log_bases(*bases) == 0
        got = {form: run(form) for form in ('buffer', 'dev', 'recent')}
    finally:
        assert lib.cham_set_log_bases(*F.DEFAULT_BASES) == 0
    assert F.same_bits(got['buffer'], got['dev']), "_dev differs from the by-value form"
    for form in ('buffer', 'recent'):
        st = got[form]
        assert F.same_bits(st[0], st[1]) and F.same_bits(st[0], st[2]), "the three copies of the statistics differ"
        _check_stats(form, st[0], inp, bases, k)
    s8 = Out(gpu, (3, 8))
    assert lib.cham_norm_stats_from_buffer_dev(ids.data_ptr(), n, None, created.data_ptr(), pop.data_ptr(), s8.ptr(), s8.ptr(), _st()) == -22
    assert lib.cham_norm_stats_from_buffer(ids.data_ptr(), 0, 0, created.data_ptr(), pop.data_ptr(), s8.ptr(), s8.ptr(), _st()) == -22
    assert lib.cham_norm_stats_from_recent(None, n, 0, created.data_ptr(), pop.data_ptr(), s8.ptr(), s8.ptr(), _st()) == -22
    assert s8.untouched()


def _rows_run(gpu, lib, inp, group):
    from chameleon_recsys_amd._lib import check
    n = len(inp['w'])
    rec, nov, w = _dev(gpu, inp['rec']), _dev(gpu, inp['nov']), _dev(gpu, inp['w'])

    def run():
        stats = Out(gpu, (3, 8))
        check(lib.cham_norm_stats_from_rows(rec.data_ptr(), nov.data_ptr(), w.data_ptr(), n, stats.ptr(8 * group), _st()), "cham_norm_stats_from_rows")
        return (stats.numpy(),)
    st = _twice(run)[0]
    others = [g for g in range(3) if g != group]
    assert np.isnan(st[others]).all(), "cham_norm_stats_from_rows wrote another group's statistics"
    return st[group]


@pytest.mark.parametrize("kind", F.ROWS_KINDS)
@pytest.mark.parametrize("n", F.STATS_N)
def test_norm_stats_from_rows_match_float64(gpu, n, kind):
    """0 / 1 weights with the zeros in the middle of the population (and holding its extremes), integer repetition counts up to BT N, and
    exactly one positive weight (a constant population: sd and the z values as in test_norm_stats_of_a_constant_population)."""
    lib, k = _lib_(), gpu_bounds()
    inp = F.rows_inputs(n, kind)
    print("\nn %d %s" % (n, kind))
    _check_stats('rows', _rows_run(gpu, lib, inp, n % 3), inp, None, k)


@pytest.mark.parametrize("n", F.CONST_N)
def test_norm_stats_of_a_constant_population(gpu, n):
    """Every value the same fp32 number.  mean and the de-normalised extremes mean + sd zmin, mean + sd zmax are held to the bound; sd to
    the mean's allowed error + 1e-12 (it is sqrt(roundoff^2 + 1e-24)).  zmin and zmax themselves are NOT compared: they are
    (x - mean) / sd = roundoff / roundoff - anything between -1 and 1 - in the reference's own fp32 graph too, which is ill-conditioned
    at this point; what the model uses is norm_apply of them, and max(zmax - zmin, 2e-24) keeps that finite."""
    lib, k = _lib_(), gpu_bounds()
    inp = F.constant_inputs(n)
    print("\nconstant n %d" % n)
    st = _rows_run(gpu, lib, inp, 1)
    _check_stats('constant', st, inp, None, k)
    assert np.isfinite(st).all() and (np.abs(st[[2, 3, 6, 7]]) <= 1.0 + 1e-5).all()          # |x - mean| <= sqrt((x - mean)^2 + 1e-24)
    got = F.norm_apply(inp['rec'][:1], st[:4], np.float32)
    assert np.isfinite(got).all()


def test_norm_stats_of_an_empty_population_touch_nothing_else(gpu):
    """No positive weight: the formula is 0 / 0, as TF's moments of an empty tensor are.  Owed: the other groups' statistics and the
    guards stay as they were (and -22 for the argument errors)."""
    lib = _lib_()
    inp = F.rows_inputs(65, 'zero_one')
    inp['w'][:] = 0.0
    _rows_run(gpu, lib, inp, 1)
    s8, x = Out(gpu, (3, 8)), Out(gpu, (8,))
    for a in ((None, x.ptr(), x.ptr(), 8, s8.ptr()), (x.ptr(), None, x.ptr(), 8, s8.ptr()), (x.ptr(), x.ptr(), None, 8, s8.ptr()),
              (x.ptr(), x.ptr(), x.ptr(), 0, s8.ptr()), (x.ptr(), x.ptr(), x.ptr(), 8, None)):
        assert lib.cham_norm_stats_from_rows(*a, _st()) == -22
    torch.cuda.synchronize()
    assert s8.untouched()


# ---- first-batch weights --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(F.SLOT_CASES)))
def test_row_weights_are_exact_counts(gpu, case):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    s = F.slot_inputs(case)
    BT, N, pmax = s['BT'], s['N'], s['pmax']
    rng = np.random.default_rng(case)
    ids = rng.integers(0, 4, 2 * BT + 3).astype(np.int64) * rng.integers(1, F.N_ITEMS, 2 * BT + 3)
    want_ids, want_slots = F.row_weights(ids, s['slot'], pmax, s['pool'])
    assert (want_ids == 0).any() and want_slots.max() >= 1 and want_slots[pmax] == 0
    d_ids, d_slot, d_pool = _dev(gpu, ids), _dev(gpu, s['slot']), _dev(gpu, s['pool'])
    n_ids, n_neg = len(ids), BT * N

    def run(use_ids, use_slots):
        def go():
            w_ids, w_slots = Out(gpu, (n_ids,)), Out(gpu, (pmax + 1,))
            check(lib.cham_row_weights(d_ids.data_ptr() if use_ids else None, n_ids, d_slot.data_ptr() if use_slots else None, n_neg, pmax,
                                       d_pool.data_ptr(), w_ids.ptr(), w_slots.ptr(), _st()), "cham_row_weights")
            torch.cuda.synchronize()
            assert use_ids or w_ids.untouched()
            assert use_slots or w_slots.untouched()
            return w_ids.numpy(), w_slots.numpy()
        return _twice(go)
    both = run(True, True)
    assert np.array_equal(both[0], want_ids) and np.array_equal(both[1], want_slots)
    assert np.array_equal(run(True, False)[0], want_ids) and np.array_equal(run(False, True)[1], want_slots)
    # a half that is asked for needs its output, the slot half its pool; a half that is not asked for needs nothing
    w_ids, w_slots = Out(gpu, (n_ids,)), Out(gpu, (pmax + 1,))
    i, sl, pl = d_ids.data_ptr(), d_slot.data_ptr(), d_pool.data_ptr()
    assert lib.cham_row_weights(i, n_ids, sl, n_neg, pmax, pl, None, w_slots.ptr(), _st()) == -22
    assert lib.cham_row_weights(i, n_ids, sl, n_neg, pmax, pl, w_ids.ptr(), None, _st()) == -22
    assert lib.cham_row_weights(i, n_ids, sl, n_neg, pmax, None, w_ids.ptr(), w_slots.ptr(), _st()) == -22
    assert lib.cham_row_weights(None, n_ids, sl, n_neg, pmax, None, None, w_slots.ptr(), _st()) == -22
    torch.cuda.synchronize()
    assert w_ids.untouched() and w_slots.untouched()
    assert lib.cham_row_weights(i, n_ids, None, n_neg, pmax, None, w_ids.ptr(), None, _st()) == 0
    assert lib.cham_row_weights(None, n_ids, sl, n_neg, pmax, pl, None, w_slots.ptr(), _st()) == 0
    assert np.array_equal(w_ids.numpy(), want_ids) and np.array_equal(w_slots.numpy(), want_slots)


# ---- the integer row sets -------------------------------------------------------------------------------------------------------------
# (BT, pmax, B): B > 2 BT + pmax + 1 sizes the grid by B (the last two)
STEP_INT_CASES = [(1, 0, 1), (257, 1, 40), (257, 4000, 257), (1, 4000, 1), (0, 0, 3), (0, 1, 0), (1, 0, 700), (257, 1, 1031)]


@pytest.mark.parametrize("BT,pmax,B", STEP_INT_CASES)
def test_step_ints_are_exact(gpu, BT, pmax, B):
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    rng = np.random.default_rng(BT + pmax + B)
    ic, ln = rng.integers(0, F.N_ITEMS, BT + 2).astype(np.int64), rng.integers(0, F.N_ITEMS, BT + 2).astype(np.int64)
    pool = rng.integers(0, F.N_ITEMS, pmax + 2).astype(np.int64)
    ets = (F.T0 + rng.integers(0, 7200000, BT + 2)).astype(np.int64)
    seq_len, mask = rng.integers(1, 20, B + 2).astype(np.int32), (rng.random(BT + 2) < 0.7).astype(np.uint8)
    max_ts = F.MAX_TS
    want = F.step_ints(ic, ln, pool, ets, max_ts, BT, pmax, seq_len[:B], mask)
    d = [_dev(gpu, a) for a in (ic, ln, pool, ets, seq_len, mask)]
    rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
    check(lib.cham_step_scalars_set(rec.data_ptr(), 0, 0, max_ts, 0.0, 0.0, 2, _st()), "cham_step_scalars_set")
    RV = 2 * BT + pmax + 1

    def run(dev):
        def go():
            outs = [Out(gpu, (RV,), torch.int64), Out(gpu, (RV,), torch.int64), Out(gpu, (B,), torch.int32), Out(gpu, (BT,), torch.uint8)]
            a = (d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr())
            b = (BT, pmax, d[4].data_ptr(), B, d[5].data_ptr(), outs[0].ptr(), outs[1].ptr(), outs[2].ptr(), outs[3].ptr(), _st())
            if dev:
                check(lib.cham_step_ints_dev(*a, rec.data_ptr(), *b), "cham_step_ints_dev")
            else:
                check(lib.cham_step_ints(*a, max_ts, *b), "cham_step_ints")
            return tuple(o.numpy() for o in outs)
        return _twice(go)
    got, got_dev = run(False), run(True)
    for g, gd, w, name in zip(got, got_dev, want, ('ids_all', 'ref_ts', 'seq_len', 'mask')):
        assert g.dtype == w.dtype and np.array_equal(g, w), name
        assert F.same_bits(g, gd), "%s: _dev differs from the by-value form" % name
    o = Out(gpu, (RV,), torch.int64)
    p = o.ptr()
    assert lib.cham_step_ints_dev(p, p, p, p, None, BT, pmax, p, B, p, p, p, p, p, _st()) == -22
    assert lib.cham_step_ints(None, p, p, p, 0, BT, pmax, p, B, p, p, p, p, p, _st()) == -22
    assert lib.cham_step_ints(p, p, p, p, 0, -1, pmax, p, B, p, p, p, p, p, _st()) == -22
    torch.cuda.synchronize()
    assert o.untouched()


# ---- user-context rows ----------------------------------------------------------------------------------------------------------------
def _ctx_check(gpu, lib, inp, k, name):
    from chameleon_recsys_amd._lib import check
    R, Fc = inp['cat'].shape[1] if len(inp['cat']) else inp['num'].shape[1], len(inp['desc'])
    d = {a: _dev(gpu, inp[a]) for a in ('cat', 'num', 'desc', 'params', 'gamma', 'beta')}

    def run():
        xraw, xs = Out(gpu, (R, Fc)), Out(gpu, (R, Fc))
        check(lib.cham_ctx_assemble(d['cat'].data_ptr(), d['num'].data_ptr(), R, d['desc'].data_ptr(), Fc, d['params'].data_ptr(), d['gamma'].data_ptr(),
                                    d['beta'].data_ptr(), xraw.ptr(), xs.ptr(), _st()), "cham_ctx_assemble")
        return xraw.numpy(), xs.numpy()
    xraw, xs = _twice(run)
    want_raw, want_s = F.ctx_rows(inp['cat'], inp['num'], inp['desc'], inp['params'], inp['gamma'], inp['beta'])
    assert np.array_equal(xraw, want_raw), "gathered context columns differ"
    _note(name, F.rel_err(xs, want_s), k['ctx.xs'])            # (v * gamma + beta is one FMA on the device: not the CPU's two roundings)
    return xraw


@pytest.mark.parametrize("R", F.CTX_R)
def test_ctx_assemble_hand_built_schema(gpu, R):
    """Every kind the kernel takes - zero pad, one-hot, embedding (widths 3, 6 and 7: none divides 4), numeric - from raw descriptors."""
    lib, k = _lib_(), gpu_bounds()
    print("\nR %d" % R)
    inp = F.ctx_inputs(R)
    xraw = _ctx_check(gpu, lib, inp, k, 'ctx.xs')
    kinds = inp['desc'][:, 0]
    assert set(kinds.tolist()) == {F.COL_ZERO, F.COL_OHE, F.COL_EMB, F.COL_NUM} and not xraw[:, kinds == F.COL_ZERO].view(np.uint32).any()
    x = Out(gpu, (8,))
    p = x.ptr()
    assert lib.cham_ctx_assemble(p, p, 2, None, 4, p, p, p, p, p, _st()) == -22 and lib.cham_ctx_assemble(p, p, 0, p, 4, p, p, p, p, p, _st()) == -22
    assert lib.cham_ctx_assemble(p, p, 2, p, 4, p, p, p, None, p, _st()) == -22 and lib.cham_ctx_assemble(p, p, 2, p, 4, p, p, p, p, None, _st()) == -22


@pytest.mark.parametrize("R", F.CTX_R)
@pytest.mark.parametrize("dataset", ["gcom", "adressa"])
def test_ctx_assemble_runtime_schemas(gpu, dataset, R):
    """The G1 and Adressa context schemas as NARRuntime lays them out (descriptors and tables of its flat parameter buffer)."""
    from chameleon_recsys_amd.nar import synthetic
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    lib, k = _lib_(), gpu_bounds()
    p = synthetic.default_params(2000, 64, C=128, H=64, dataset=dataset, buffer_size=500, for_norm=100)
    rt = NARRuntime(p, seed=3)
    L = rt.layout
    scfg = p['session_features_config']['sequence_features']
    rng = np.random.default_rng(len(dataset) + R)
    cat = np.stack([rng.integers(0, scfg[n]['cardinality'], R) for n in L.ctx_cat_names]).astype(np.int64)
    if R > 1:
        cat[:, 0], cat[:, -1] = 0, [scfg[n]['cardinality'] - 1 for n in L.ctx_cat_names]
    num = rng.standard_normal((max(1, len(L.ctx_num_names)), R)).astype(np.float32)
    desc = L.ctx_descriptors()
    assert np.array_equal(desc, rt.ctx_desc.cpu().numpy()) and len(desc) == L.Fc
    print("\n%s R %d: Fc %d, kinds %s" % (dataset, R, L.Fc, sorted(set(desc[:, 0].tolist()))))
    inp = dict(cat=cat, num=num, desc=desc, params=rt.flat.cpu().numpy(), **F.gamma_beta(rng, L.Fc))
    _ctx_check(gpu, lib, inp, k, 'ctx.xs ' + dataset)


# ---- dropout --------------------------------------------------------------------------------------------------------------------------
def _dropout_run(gpu, lib, x, kw, ld, in_place, expect=0):
    """cham_dropout on x [rows, cols] stored with row pitch ld (the pad columns hold 7.0 and must keep it); y = a fresh NaN matrix or x
    itself."""
    rows, cols = x.shape
    full = np.full((rows, ld), 7.0, np.float32)
    full[:, :cols] = x
    src = Out(gpu, (rows, ld), init=_dev(gpu, full))
    dst = src if in_place else Out(gpu, (rows, ld))
    pos = None if kw['pos'] is None else _dev(gpu, kw['pos'])
    rc = lib.cham_dropout(src.ptr(), dst.ptr(), rows, cols, ld, kw['keep'], kw['seed'], kw['step'], kw['site_first'], kw['site_rest'], kw['group'],
                          None if pos is None else pos.data_ptr(), kw['T'], kw['row_begin'], kw['col_split'], kw['col_shift'], _st())
    assert rc == expect, rc
    out = dst.numpy()
    if expect == 0:
        if in_place:
            assert (out[:, cols:] == 7.0).all(), "the pad columns were written"
        else:
            assert np.isnan(out[:, cols:]).all(), "the pad columns were written"
            assert F.same_bits(src.numpy(), full), "the input was modified"
    return out[:, :cols]


def _shard(inp, lo, hi):
    """The sessions [lo, hi) of a dropout input set as a row shard: its rows of both launches and its own position map."""
    T, N = inp['T'], inp['N']
    if inp['pos'] is None:
        sel = np.arange(lo * T, hi * T)
        pos = None
    else:
        sel = np.flatnonzero((inp['pos'] // T >= lo) & (inp['pos'] // T < hi))
        pos = (inp['pos'][sel] - lo * T).astype(np.int32)
    cand = (sel[:, None] * (N + 1) + np.arange(N + 1)[None, :]).reshape(-1)
    return dict(inp, pos=pos, P=len(sel), x_in=inp['x_in'][sel], x_cand=inp['x_cand'][cand]), sel, cand


@pytest.mark.parametrize("case", range(len(F.DROPOUT_CASES)))
def test_dropout_mask_and_values_are_exact(gpu, case):
    """Both launches of the model - the clicked-input rows (group 1) and the candidate rows (group N + 1, site_first != site_rest) of the
    dense [ctx | item] matrix, col_split = Fc, col_shift = Fc - f_ctx - with and without the position map of a compaction, out of place
    and in place, with ld == cols and ld > cols, as a whole and as the row shard that begins at session B / 2 (and both shards
    together equal the whole).  The mask is the reference's bit for bit; a kept value is float32(x) / float32(keep) bit for bit
    (hipcc's fp32 division is correctly rounded under this build's flags), a dropped one +0.0."""
    lib = _lib_()
    inp = F.dropout_inputs(case)
    B, cols = inp['B'], inp['Fc'] + inp['Fi']
    print("\n%s" % (F.DROPOUT_CASES[case],))
    whole = []
    for li, (x, kw) in enumerate(F.dropout_launches(inp)):
        want, kept = F.dropout(x, **kw)
        assert 0 < kept.mean() < 1 and abs(kept.mean() - inp['keep']) < 0.1
        for ld in (cols, cols + 4):
            for in_place in (False, True):
                got = _twice(lambda: (_dropout_run(gpu, lib, x, kw, ld, in_place),))[0]
                assert np.array_equal(got != 0, kept & (x != 0)), "mask differs (launch %d, ld %d, in place %s)" % (li, ld, in_place)
                assert not got[~kept].view(np.uint32).any(), "a dropped element is not +0.0"
                assert F.same_bits(got[kept], want[kept]), "a kept value is not float32(x) / float32(keep)"
        assert F.same_bits(got, _dropout_run(gpu, lib, x, kw, cols, False)), "in place with ld > cols differs from out of place with ld == cols"
        whole.append(got)
    assert any((x.size % 256) for x, _ in F.dropout_launches(inp))
    # row shards: sessions [0, B / 2) with row_begin 0 and [B / 2, B) with row_begin B / 2
    parts = [[], []]
    for lo, hi in ((0, B // 2), (B // 2, B)):
        sh, sel, cand = _shard(inp, lo, hi)
        for li, (x, kw) in enumerate(F.dropout_launches(sh, row_begin=lo)):
            got = _twice(lambda: (_dropout_run(gpu, lib, x, kw, cols, True),))[0]
            assert F.same_bits(got, F.dropout(x, **kw)[0])
            assert F.same_bits(got, whole[li][cand if li else sel]), "a row shard differs from its rows of the whole batch"
            parts[li].append(got)
    assert all(F.same_bits(np.concatenate(parts[li]), whole[li]) for li in range(2))


def test_dropout_argument_errors(gpu):
    lib = _lib_()
    x, kw = F.dropout_launches(F.dropout_inputs(0))[0]
    cols = x.shape[1]
    for bad in (dict(keep=0.0), dict(keep=-0.5), dict(keep=1.0), dict(keep=1.5), dict(keep=float('nan')), dict(group=0), dict(T=0)):
        _dropout_run(gpu, lib, x, dict(kw, **bad), cols, False, expect=-22)
    o = Out(gpu, x.shape)
    a = (kw['keep'], kw['seed'], kw['step'], 16, 16, 1, None, kw['T'], 0, cols, 0, _st())
    assert lib.cham_dropout(o.ptr(), o.ptr(), x.shape[0], cols, cols - 1, *a) == -22
    assert lib.cham_dropout(None, o.ptr(), x.shape[0], cols, cols, *a) == -22 and lib.cham_dropout(o.ptr(), None, x.shape[0], cols, cols, *a) == -22
    assert lib.cham_dropout(o.ptr(), o.ptr(), 0, cols, cols, *a) == -22
    torch.cuda.synchronize()
    assert o.untouched()


# ---- dense PreCAR input rows ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,Fc,Fi", [(0, 4, 1028), (1, 72, 408), (2, 408, 72), (3, 1028, 4), (4, 72, 72), (1, 1028, 1028)])
def test_dense_rows_are_an_exact_gather(gpu, case, Fc, Fi):
    """The slot tables of the combine tests (pads, masked clicks); Fc and Fi of {4, 72, 408, 1028}: 1028 floats are 257 float4, one more
    than a workgroup's 256 threads take in one trip."""
    from chameleon_recsys_amd._lib import check
    lib = _lib_()
    s = F.slot_inputs(case)
    BT, N, pmax = s['BT'], s['N'], s['pmax']
    rng = np.random.default_rng(Fc + Fi + case)
    Xc = rng.standard_normal((BT, Fc)).astype(np.float32)
    Xi = rng.standard_normal((2 * BT + pmax + 1, Fi)).astype(np.float32)
    want = F.dense_rows(Xc, Xi, s['slot'], BT, N, pmax)
    d_c, d_i, d_s = _dev(gpu, Xc), _dev(gpu, Xi), _dev(gpu, s['slot'])

    def run():
        X = Out(gpu, (BT + BT * (N + 1), Fc + Fi))
        check(lib.cham_dense_rows(d_c.data_ptr(), Fc, d_i.data_ptr(), Fi, BT, N, pmax, d_s.data_ptr(), X.ptr(), _st()), "cham_dense_rows")
        return (X.numpy(),)
    got = _twice(run)[0]
    assert F.same_bits(got, want)
    X = Out(gpu, (8,))
    a, b, c = d_c.data_ptr(), d_i.data_ptr(), d_s.data_ptr()
    assert lib.cham_dense_rows(a, Fc + 2, b, Fi, BT, N, pmax, c, X.ptr(), _st()) == -22 and lib.cham_dense_rows(a, Fc, b, Fi + 1, BT, N, pmax, c, X.ptr(), _st()) == -22
    assert lib.cham_dense_rows(a, Fc, b, Fi, 0, N, pmax, c, X.ptr(), _st()) == -22 and lib.cham_dense_rows(a, Fc, b, Fi, BT, 0, pmax, c, X.ptr(), _st()) == -22
    assert lib.cham_dense_rows(None, Fc, b, Fi, BT, N, pmax, c, X.ptr(), _st()) == -22 and lib.cham_dense_rows(a, Fc, b, Fi, BT, N, pmax, None, X.ptr(), _st()) == -22
    torch.cuda.synchronize()
    assert X.untouched()
