"""Row shards and micro-batches on every model variant, and on the very first batch.

The step scales through two paths that both run it on ROW SHARDS with global ids and denominators: NARModuleModel.train_step_microbatched
and DataParallelNAR.  Here every variant merged after those paths were written - stacked and wide GRU, LSTM, novelty and diversity terms,
the cosine head, dropout's dense input rows, the plane-resident CAR GEMMs at C = 256 and the bf16 configuration - goes through them at
B = 48 ragged sessions (seq_len 8, 8 negatives, 1000 items): row shards of a world of 2 and 3 (24 + 24, 16 + 16 + 16 sessions of unequal
valid positions), micro-batches of 20 (20 + 20 + 8) and 47 (47 + 1) sessions, against the whole-batch step of the same model; three
variants start from an EMPTY recent-clicks state, where the first step takes its normalisation statistics from the batch itself
(FeatureRows.norm_stats_first_batch_of_shard: from the GLOBAL batch on a shard); two of them also run as two data-parallel processes.

Bounds (tests/shard_paths.py states the per-entry one):
  negatives       bit-equal;
  logits, loss    shard against whole batch 1e-5 (tests/test_step_gpu.py::test_row_shards_sum_to_full_batch) - at C = 256 and in bf16 the
                  plane scale records are maxima over the call's rows, shard and whole batch round differently:
                  max(1e-5, 4 x |oracle32 - oracle64|_max of the same quantity on the same batch); every variant 1e-3 against the float32
                  oracle (bf16: loss 1e-3 and logits 2e-3 against the oracle that emulates the bf16 rounding, as
                  tests/test_step_gpu.py::test_step_parity_bf16_compute_mode);
  div_e           the logits' bound (1e-5: both variants that have it run at C = 128, a row-independent fp32 forward);
  gradients       per layout entry max|g_sum - g_full| <= max(4 x max|g_oracle32 - g_oracle64|, 8 u x max|g_oracle64|), both oracles on the
                  leaky-ReLU branches of the HIP whole-batch run; whole buffer 2e-5 x max|g_full| + 1e-7.  An entry whose true gradient
                  is identically zero (bs4, asserted to be the only one) holds roundoff only, both oracle figures are ~0: it is held
                  to the ceiling of any raised factor, 3e-4 x max|ref| + 2e-5 = 2e-5;
  bf16            loss 1e-3 against the emulating oracle; the shard SUM as close to the fp32 oracle as the emulation is
                  (3 x e_emu + 2e-2 x scale + 2e-5, tests/test_step_gpu.py::test_step_parity_bf16_compute_mode); no per-entry bound;
                  whole buffer one bf16 ulp, 2^-8 x max|g_full| (dU / dV are rounded after the sum over the call's rows);
  micro-batched   losses 1e-5, helpers.assert_runtimes_close (bf16: m_tol 5e-2, w_tol 0.5, floor 0.25 as tests/test_dp_gpu.py).

Measured on an MI355X (row shards of a world of 2 and 3, batch 3 on a warm state; `cold`: step 1 of test_cold_start_on_shards).  `ratio`: the
worst per-entry max|g_sum - g_full| against max(max|g_oracle32 - g_oracle64|, 2 u max|g_oracle64|) - the bound is 4; `buffer`: the whole
flat buffer's max|g_sum - g_full| over max|g_full|.  No entry's factor had to be raised (ENTRY_FACTOR is empty).  The zero-gradient entry
bs4 deviates by 3e-9 ... 5e-8 (bound 2e-5).
    variant          ratio (entry)        |dlogit| shard vs whole   |dloss|    buffer
    gru2             2.22 (beta_item)     0                         1.2e-07    9.7e-08
    gru_wide         1.20 (W1i)           0                         1.8e-07    1.6e-07
    lstm2            1.71 (beta_item)     0                         1.8e-07    1.2e-07
    novelty          1.42 (W1i)           0                         2.2e-08    1.5e-07
    diversity        2.40 (W1i)           0  (div_e 0)              3.6e-07    2.1e-07
    cosine           1.59 (Wf2)           0                         6.0e-08    2.4e-07
    cosine_all       1.79 (W1i)           0  (div_e 0)              3.0e-08    2.4e-07
    dropout          1.60 (W1i)           0                         1.8e-07    1.8e-07
    planes           1.33 (W1i)           0                         3.6e-07    1.3e-07
    planes_cosine    1.40 (W1i)           0                         1.2e-07    2.6e-07
    bf16             -                    0                         1.2e-07    2.4e-04   (logits 1.3e-3, loss 1.8e-4 from the emulating oracle)
    default cold     0.95 (gamma_item)    0                         0          9.8e-08     steps 2, 3: ratio 1.55 (W1i), 1.22 (Wf1)
    cosine_all cold  1.49 (rnn0/Wx)       0                         3.7e-09    2.0e-07     steps 2, 3: ratio 1.07 (W1i), 1.60 (W1i)
    lstm2 cold       1.56 (gamma_item)    0                         0          2.0e-07     steps 2, 3: ratio 2.48 (gamma_item), 2.94 (beta_item)
The forward of a shard is bit-equal to the whole batch's rows in every variant, the plane-resident ones included (their power-of-two scale
records came out equal on these batches); micro-batched against whole-batch losses: at most 2.4e-7; two ranks against one process: 2.4e-7.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from chameleon_recsys_amd.nar import parallel
from tests import helpers as H
from tests import shard_paths as SP

pytestmark = pytest.mark.gpu
LOGIT_TOL = 1e-3
ROW_VARIANTS = [v for v in SP.VARIANTS if v != 'default']
COLD_VARIANTS = ['default', 'cosine_all', 'lstm2']
COLD = dict(for_norm=500)          # recent_clicks_for_normalization above the 206 clicks of the first batch: step 2 normalises on a short buffer
DIVERSITY_VARIANTS = ('diversity', 'cosine_all')          # outputs_numpy() carries div_e for these and for no other
ENTRY_FACTOR = {}          # variant -> {entry: factor}: entries whose factor had to be raised above 4 (twice the measured worst ratio)


def _leaky_signs(model, mask):
    """tests.test_step_gpu.hip_leaky_signs; the cosine head has no scorer layers: its sites are Z1 and FC1."""
    from tests.test_step_gpu import hip_leaky_signs
    if not model.rt.cosine:
        return hip_leaky_signs(model, mask)
    pl = model._plan
    B, T, NC, P = pl.B, pl.T, pl.NC, pl.P
    valid = torch.from_numpy(np.asarray(mask, bool))
    zin = pl.full_rows(pl.Z1[:P]).float().cpu().reshape(B, T, -1) > 0
    zc = pl.full_rows(pl.cand_Z1(P), NC).float().cpu().reshape(B, T, NC, -1) > 0
    return {'Z1': [(zin, valid[:, :, None]), (zc[:, :, 0], valid[:, :, None]), (zc[:, :, 1:], valid[:, :, None, None])],
            'FC1': [(pl.full_rows(pl.FC1).float().cpu().reshape(B, T, -1) > 0, valid[:, :, None])]}


def _state_arrays(st):
    return st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()


def _hip_whole(model, f, l):
    model.forward(model.upload_batch(f, l)); model.backward()
    torch.cuda.synchronize()
    return model.outputs_numpy(), model.rt.grads.clone()


def _hip_shards(model, f, l, ranges):
    """The step on the row ranges `ranges` of (f, l), each with the global batch beside it -> (outputs per shard, summed flat gradients)."""
    outs, g_sum = [], torch.zeros_like(model.rt.grads)
    for b, e in ranges:
        fl, ll = parallel.slice_batch(f, l, b, e)
        model.forward(model.upload_batch(fl, ll, f, l, row_begin=b)); model.backward()
        torch.cuda.synchronize()
        outs.append(model.outputs_numpy()); g_sum += model.rt.grads
    return outs, g_sum


def _ranges(kind, n_or_world, B=SP.B):
    if kind == 'world':
        return [parallel.shard_rows(B, r, n_or_world) for r in range(n_or_world)]
    return [(b, min(B, b + n_or_world)) for b in range(0, B, n_or_world)]


_CASES = {}


def _case(variant, batch_index, **more):
    """One (variant, batch): the model fed with the state warmed on the batches before `batch_index`, the whole-batch HIP result
    (outputs_numpy(), a clone of rt.grads) and the whole-batch oracle in float32 and float64 on the same weights, both on the leaky-ReLU
    branches of that HIP run (a kink flip cannot loosen anything); bf16: `emu`, the oracle that emulates the rounding, beside the fp32
    pair.  Computed once and shared; shards(ranges) runs a split on the same model."""
    key = (variant, batch_index) + tuple(sorted(more.items()))
    if key in _CASES:
        return _CASES[key]
    p, model, orc = SP.make_pair(variant, **more)
    bs = SP.batches(p, batch_index + 1)
    st = H.warm_state(p, bs[:batch_index])
    c = _CASES[key] = _evaluate(variant, p, model, orc, *bs[batch_index], *_state_arrays(st))
    return c


def _evaluate(variant, p, model, orc, f, l, buf, pop):
    """The whole-batch HIP step of `model` on (f, l) with the state (buf, pop), and `orc` (same weights, same step counter) with its float32
    / float64 twins on that run's leaky-ReLU branches."""
    model.feed_state(pop, buf)
    out, g_full = _hip_whole(model, f, l)
    mask = SP.valid_mask(f)
    c = dict(p=p, model=model, orc=orc, f=f, l=l, mask=mask, out=out, g_full=g_full, L=model.rt.layout)
    signs_record = _leaky_signs(model, mask)
    signs = lambda: {k: list(v) for k, v in signs_record.items()}
    b16 = p.get('gemm_dtype', 'f32') == 'bf16'
    o32 = SP.twin(orc, torch.float32, gemm_dtype='f32') if b16 else orc
    o64 = SP.twin(o32, torch.float64)
    c['o32'], c['o64'] = SP.oracle_pass(o32, f, l, buf, pop, signs), SP.oracle_pass(o64, f, l, buf, pop, signs)
    c['emu'] = SP.oracle_pass(orc, f, l, buf, pop, signs) if b16 else None
    # forward tolerances of shard against whole batch
    plane = variant in SP.PLANE_VARIANTS
    c['logit_tol'] = max(1e-5, 4.0 * float(np.abs(c['o32']['logits'] - c['o64']['logits'])[mask].max())) if plane else 1e-5
    c['loss_tol'] = max(1e-5, 4.0 * abs(c['o32']['loss'] - c['o64']['loss'])) if plane else 1e-5
    c['shards'] = lambda ranges: _hip_shards(model, f, l, ranges)
    return c


def _check_forward_against_oracle(c, logits, loss_data, negs, label):
    """tests/test_step_gpu._compare_step's forward criterion on (concatenated) HIP results; bf16: against the oracle that emulates the
    rounding, loss 1e-3 and logits at the 2e-3 of tests/test_step_gpu.py::test_step_parity_bf16_compute_mode."""
    ref = c['emu'] if c['emu'] is not None else c['o32']
    # bf16 logits: 2e-3, not LOGIT_TOL - the project's figure for bf16 against the emulating oracle (test_step_parity_bf16_compute_mode: a
    # value that lands on the other side of a bf16 rounding boundary moves by 2^-8 relative); measured here 1.3e-3, whole batch and shards alike
    logit_tol = 2e-3 if c['emu'] is not None else LOGIT_TOL
    assert np.array_equal(negs, ref['neg_items']), "%s: negative samples must be bit exact" % label
    e = float(np.abs(logits - ref['logits'])[c['mask']].max())
    print("%s: |logits - float32 oracle| %.2e, |loss - oracle| %.2e" % (label, e, abs(loss_data - ref['loss'])))
    assert e < logit_tol and abs(loss_data - ref['loss']) < LOGIT_TOL, (label, e, loss_data, ref['loss'])


def _check_shards_against_whole(variant, c, outs, g_sum, label, step_parity=False):
    """Everything test_row_shards_sum_to_the_whole_batch asserts of one split (also used on the first batch); step_parity: the summed
    gradients also under _compare_step's criterion against the float32 oracle."""
    full, mask, L = c['out'], c['mask'], c['L']
    negs, logits = np.concatenate([o['neg_items'] for o in outs]), np.concatenate([o['logits'] for o in outs])
    assert np.array_equal(negs, full['neg_items']), label
    e_logit = float(np.abs(logits - full['logits'])[mask].max())
    share = float(sum(float(o['loss'][1]) for o in outs))
    e_loss = abs(share - float(full['loss'][1]))
    print("%s: shard against whole batch |dlogit| %.2e (bound %.1e), |dloss| %.2e (bound %.1e)" % (label, e_logit, c['logit_tol'], e_loss, c['loss_tol']))
    assert e_logit < c['logit_tol'], (label, e_logit, c['logit_tol'])
    assert e_loss < c['loss_tol'], (label, share, full['loss'], c['loss_tol'])
    _check_forward_against_oracle(c, logits, share, negs, label)
    _check_forward_against_oracle(c, full['logits'], float(full['loss'][1]), full['neg_items'], label + " (whole batch)")
    assert ('div_e' in full) == (variant in DIVERSITY_VARIANTS) and all(('div_e' in o) == ('div_e' in full) for o in outs), label
    if variant in DIVERSITY_VARIANTS:          # p^T S p per click, a row-independent fp32 function of the row's probabilities: the logits' bound
        e_div = float(np.abs(np.concatenate([o['div_e'] for o in outs]) - full['div_e'])[mask].max())
        print("%s: |d div_e| %.2e" % (label, e_div))
        assert e_div < c['logit_tol'], (label, e_div)
        assert float(np.abs(full['div_e'] - c['o32']['div_e'])[mask].max()) < LOGIT_TOL
    g_full = c['g_full']
    ratios = None
    if c['emu'] is None:
        ratios = SP.check_entries(L, g_sum, g_full, c['o32']['grads'], c['o64']['grads'], ENTRY_FACTOR.get(variant), label)
    else:          # bf16: the shard sum is as accurate against the fp32 oracle as the emulated bf16 gradient is
        g = L.unpack(g_sum.cpu().numpy())
        for k, r32 in c['o32']['grads'].items():
            scale = max(1e-6, float(np.abs(r32).max()))
            e_hip, e_emu = float(np.abs(g[k] - r32).max()), float(np.abs(c['emu']['grads'][k] - r32).max())
            assert e_hip < 3.0 * e_emu + 2e-2 * scale + 2e-5, (label, k, e_hip, e_emu, scale)
    if step_parity and c['emu'] is None:
        g = L.unpack(g_sum.cpu().numpy())
        for k, rg in c['o32']['grads'].items():
            scale = max(1e-6, float(np.abs(rg).max()))
            err = float(np.abs(g[k] - rg).max())
            assert err < 3e-4 * scale + 2e-5, "%s: grad %s against the oracle: err %g scale %g" % (label, k, err, scale)
    # whole buffer.  bf16: the backward rounds dU / dV to bf16 AFTER summing them over the call's rows, so a shard's partial sums round
    # differently from the whole batch's - one bf16 ulp (2^-8) of the largest gradient bounds what that can move
    e_buf, g_max = float((g_sum - g_full).abs().max()), float(g_full.abs().max())
    print("%s: whole buffer |g_sum - g_full| %.2e of max" % (label, e_buf / g_max))
    assert e_buf < (2.0 ** -8 * g_max if c['emu'] is not None else 2e-5 * g_max + 1e-7), (label, e_buf, g_max)
    return e_logit, ratios


@pytest.mark.parametrize("world", SP.WORLDS)
@pytest.mark.parametrize("variant", ROW_VARIANTS)
def test_row_shards_sum_to_the_whole_batch(gpu, variant, world):
    c = _case(variant, 3)
    outs, g_sum = c['shards'](_ranges('world', world))
    _check_shards_against_whole(variant, c, outs, g_sum, "%s world %d" % (variant, world))


@pytest.mark.parametrize("micro", SP.MICRO)
@pytest.mark.parametrize("variant", ROW_VARIANTS)
def test_microbatched_step_equals_the_whole_batch_step(gpu, variant, micro):
    """Two models from one make_pair seed: train_step against train_step_microbatched."""
    p, m1, _ = SP.make_pair(variant)
    _, m2, _ = SP.make_pair(variant)
    bs = SP.batches(p, 4)
    st = H.warm_state(p, bs[:3])
    f, l = bs[3]
    for m in (m1, m2):
        m.feed_state(st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer())
    a = m1.train_step(m1.upload_batch(f, l)).cpu().numpy()
    b = m2.train_step_microbatched(f, l, micro).cpu().numpy()
    print("%s micro %d: losses apart by %.2e" % (variant, micro, float(np.abs(a - b).max())))
    assert np.abs(a - b).max() < 1e-5, (a, b)
    assert m1.rt.global_step == m2.rt.global_step == 1
    kw = dict(m_tol=5e-2, w_tol=0.5, floor=0.25) if variant == 'bf16' else {}
    H.assert_runtimes_close(m1.rt, m2.rt, p['lr'], **kw)


@pytest.mark.parametrize("variant", COLD_VARIANTS)
def test_cold_start_on_shards(gpu, variant):
    """Three optimizer steps from an EMPTY recent-clicks state, the state updated between them: the first step takes the normalisation
    statistics from the batch (on a shard: from the GLOBAL batch - every shard the same ones as the whole-batch step), the second from a
    buffer shorter than recent_clicks_for_normalization.  The micro-batched trajectory (20 sessions) and the row-shard sums (world 3) against
    the whole-batch trajectory, step by step, at the bounds of the warm tests (every step: the per-entry bound from the oracles rebuilt on
    the weights reached); step 1 also against the oracle under the step-parity criterion.

    Before the fix (statistics of the shard's own rows) the first step of the default model on three row shards was off by logits 3.0e-3, loss 2.7e-3 and the
    whole gradient buffer 4.2e-2 of its largest entry (cosine_all: 2.0e-3 / 1.9e-3 / 1.3e-2; lstm2: 6.2e-4 / 1.5e-3 / 1.9e-2), the worst
    entries (the context embeddings, gamma_item, bs1) 3e4 ... 7e4 times their bound."""
    c = _case(variant, 0, **COLD)
    p, model, orc = c['p'], c['model'], c['orc']
    assert model._dev_state['n_last'] == 0          # the batch-statistics path
    bs = SP.batches(p, 3)
    st = H.warm_state(p, [])
    _, micro, _ = SP.make_pair(variant, **COLD)
    for i, (f, l) in enumerate(bs):
        buf, pop = _state_arrays(st)
        if i > 0:          # the oracles on the weights the whole-batch trajectory has reached, pinned to this step's HIP branches
            n_valid = int((buf != 0).sum())
            assert 0 < n_valid and (i > 1 or n_valid < p['recent_clicks_for_normalization'])          # step 2: a buffer shorter than the population asked for
            orc.global_step = model.rt.global_step
            c = _evaluate(variant, p, model, SP.twin(orc, torch.float32, weights=model.rt.logical_weights()), f, l, buf, pop)
        outs, g_sum = c['shards'](_ranges('world', 3))
        _check_shards_against_whole(variant, c, outs, g_sum, "%s cold step %d world 3" % (variant, i + 1), step_parity=(i == 0))
        # the optimizer step: whole batch on `model` (its own gradient), micro-batched on the twin
        model.rt.grads.copy_(c['g_full'])
        whole_loss = c['out']['loss']
        model.apply_gradients()
        micro.feed_state(pop, buf)
        mb_loss = micro.train_step_microbatched(f, l, 20).cpu().numpy()
        print("%s cold step %d: micro-batched loss apart by %.2e" % (variant, i + 1, float(np.abs(mb_loss - whole_loss).max())))
        assert np.abs(mb_loss - whole_loss).max() < 1e-5, (i, mb_loss, whole_loss)
        assert model.rt.global_step == micro.rt.global_step == i + 1
        H.assert_runtimes_close(model.rt, micro.rt, p['lr'], n_steps=i + 1)
        H.update_state(st, f, l)
    _CASES.clear()          # (the cached model has been trained)


# ---- two data-parallel processes on the model variants, from a cold device state -------------------------------------------------------
DP_VARIANTS = ('lstm2', 'cosine_all')
DP_MODES = ('allreduce', 'sparse_rs')
STEPS = 3


def _dp_run(variant, mode):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    p, model, _ = SP.make_pair(variant, seed=7)
    dp = parallel.DataParallelNAR(model, mode=mode)
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], SP.N_ITEMS)
    losses = []
    for f, l in SP.batches(p, STEPS):          # no warm-up batches: the first step is the batch-statistics path
        model.feed_state(st, st)
        d = dp.upload(f, l)
        model.train_step(d)
        losses.append(dp.global_loss().cpu().numpy())
        st.update_from_device_batch(d['aci'], d['g_event_ts'])
    torch.cuda.synchronize()
    rt = model.rt
    info = dict(early=int(dp._early is not None), bytes=int(dp.last_exchange_bytes), total=int(rt.layout.total),
                touched=int(getattr(dp, 'last_touched_rows', 0)))
    return np.stack(losses), rt.flat.cpu().numpy(), rt.m.cpu().numpy(), info


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), CHAM_DP_GRAD_DTYPE="f32")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    for variant in DP_VARIANTS:
        for mode in DP_MODES:
            losses, flat, m, info = _dp_run(variant, mode)
            k = "%s/%s/" % (variant, mode)
            out[k + 'losses'], out[k + 'flat'], out[k + 'm'] = losses, flat, m
            for n, v in info.items():
                out[k + n] = np.int64(v)
    np.savez(os.path.join(out_dir, "shard_rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def test_two_ranks_equal_one_process_on_model_variants(gpu, tmp_path):
    """tests/test_dp_gpu.py on the LSTM and on the cosine head with both regularisers, allreduce and sparse_rs, three optimizer steps from a
    cold DeviceClickedItemsState: replicas bit-identical, losses and weights equal to the single-process run.  The cosine layout has no
    [Wf1 .. Ws4] range: no early bucket is installed, and every gradient still goes through the exchange."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(str(tmp_path / "shard_rank0.npz")), np.load(str(tmp_path / "shard_rank1.npz"))
    for variant in DP_VARIANTS:
        p = SP.params(variant)
        L = SP.layout_of(p)
        for mode in DP_MODES:
            k = "%s/%s/" % (variant, mode)
            losses, flat, m, _ = _dp_run(variant, mode)          # (one process: DataParallelNAR is inactive, the plain step)
            assert np.array_equal(r0[k + 'flat'], r1[k + 'flat']), k          # replicas stay bit-identical
            assert np.array_equal(r0[k + 'm'], r1[k + 'm']), k
            assert np.allclose(r0[k + 'losses'], r1[k + 'losses'], atol=1e-7), k
            print("%s losses apart by %.2e" % (k, float(np.abs(losses - r0[k + 'losses']).max())))
            assert np.abs(losses - r0[k + 'losses']).max() < 2e-5, (k, losses, r0[k + 'losses'])
            H.assert_flat_close(L, r0[k + 'flat'], r0[k + 'm'], flat, m, p['lr'], n_steps=STEPS, m_tol=1e-4)
            total = int(r0[k + 'total'])
            assert total == L.total
            assert int(r0[k + 'early']) == (0 if variant == 'cosine_all' else 1), k          # dp._early is None on the cosine layout
            if mode == 'allreduce':          # ... and the whole flat gradient buffer goes through the collective(s), fp32
                assert int(r0[k + 'bytes']) == 4 * total, (k, int(r0[k + 'bytes']), total)
            else:          # everything but the item table densely + its touched rows
                e = L.entries['items_embedding']
                rows = int(r0[k + 'touched'])
                assert rows > 0 and int(r0[k + 'bytes']) == 4 * (total - e.shape[0] * e.shape[1]) + 4 * rows * e.shape[1], k
