"""Evaluation sharded by session rows, reduced once (nar/parallel.py reduce_eval_records) - on ONE GPU, two processes over gloo as in
tests/test_dp_gpu.py.  (a) one process: the device-side rank histogram gives the host streaming classes' numbers; (b) two ranks: the
reduced records are identical on both ranks and EQUAL to those of one process that evaluates the same two row shards one after the
other (same kernels at the same shapes); (c) a global batch of ONE session: the rank without rows completes the training step and
the evaluation."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from chameleon_recsys_amd.nar import metrics as M
from chameleon_recsys_amd.nar import parallel, synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu
TOPN, N_EVAL, T_CAP = 5, 3, 8


def _params():
    return H.tiny_params(C=128, H=100, neg=8, batch_size=48)


def _batches(p):
    return synthetic.make_batches(2 + N_EVAL, 48, 8, 1000, p['session_features_config'], length_dist='g1', seed=6)


def _models(p):
    """(TRAIN model, EVAL model) around one runtime, the weights of tests/test_dp_gpu.py."""
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel
    train, _ = H.make_pair(p, seed=7)
    ev = NARModuleModel(ModeKeys.EVAL, None, None, p['session_features_config'], p['articles_features_config'], p['batch_size'], p['lr'], 1.0,
                        p['eval_total_negative_samples'], p['eval_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                        softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                        recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                        recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                        CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], runtime=train.rt)
    return train, ev


def _warm_state(p, batches):
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'],
                                 p['recent_clicks_for_normalization'], 1000)
    for f, l in batches[:2]:
        aci = np.concatenate([f['item_clicked'], l['label_last_item']], 1)
        st.update_from_device_batch(torch.from_numpy(aci).cuda(), torch.from_numpy(f['event_timestamp']).cuda())
    return st


def _one_session(batch):
    f, l = batch
    return {k: np.asarray(v)[:1] for k, v in f.items()}, {k: np.asarray(v)[:1] for k, v in l.items()}


# ---------------------------------------------------------------------------------------------------------------- (a) one process
def test_rank_histogram_equals_the_host_classes(gpu):
    p = _params()
    batches = _batches(p)
    _, ev = _models(p)
    st = _warm_state(p, batches)
    ev.enable_rank_histogram(TOPN, T_CAP + 2)
    host = [M.HitRate(TOPN), M.MRR(TOPN), M.NDCG(TOPN), M.HitRateBySessionPosition(TOPN)]
    for f, l in batches[2:]:
        pop = st.get_articles_recent_pop_norm()                  # what this batch is fed (read before its state update)
        ev.feed_state(st, st)
        d = ev.upload_batch(f, l)
        ev.evaluate_step(d)
        pred, labels = ev.predicted_item_ids.eval(), l['label_next_item']
        assert ((pred == labels[..., None]).sum(-1)[labels != 0] == 1).all()      # the label occurs once in its candidate row
        for m in host[:3]:
            m.add(pred, labels)
        host[3].add(pred, labels, pop[labels])
        st.update_from_device_batch(d['aci'], d['g_event_ts'])
    hist, pop_sum = ev.rank_histogram()
    n_clicks = sum(int((l['label_next_item'] != 0).sum()) for _, l in batches[2:])
    assert int(hist.sum()) == n_clicks and hist.shape == (T_CAP + 2, TOPN + 1) and not hist[T_CAP:].any()
    got = M.accuracy_from_rank_hist(hist, pop_sum, TOPN)
    rel = n_clicks * 2.0 ** -52
    assert got['hitrate_at_n'] == host[0].result() and 0.0 < got['hitrate_at_n'] < 1.0
    for m in host[1:3]:
        assert abs(float(got[m.name]) - float(m.result())) <= rel * abs(float(m.result())), m.name
    hr, avg_pop, tot = host[3].result()
    assert got['hitrate_at_n_by_pos'][2] == tot and got['hitrate_at_n_by_pos'][0] == hr
    for k in tot:
        assert abs(got['hitrate_at_n_by_pos'][1][k] - avg_pop[k]) <= rel * abs(avg_pop[k]), k


# ---------------------------------------------------------------------------------------------------------------- (b), (c) two ranks
def _evaluate(ev, st, batches, upload, shards, dp=None):
    """N_EVAL evaluate_steps per shard with the histogram and the beyond-accuracy records enabled; `upload(f, l, shard)` -> device batch.
    The state is fed once per global batch; every shard of a batch runs under that batch's sampler key."""
    ev.enable_rank_histogram(TOPN, T_CAP)
    ev.enable_beyond_accuracy_metrics(TOPN, 1.0, 0.02, st.buf_ids)
    ba_sums, ba_clicks, loss = np.zeros(4), 0, 0.0
    ev._eval_iter = 0
    for i, (f, l) in enumerate(batches):
        ev.feed_state(st, st)
        for s in shards:
            ev._eval_iter = i
            d = upload(f, l, s)
            ev.evaluate_step(d)
            loss += float(ev.total_loss[1])
            if dp is None and not d.get('empty'):
                per_click, _ = ev.beyond_accuracy_outputs()
                ba_sums += per_click.astype(np.float64).reshape(-1, 4).sum(0)
                ba_clicks += int((np.asarray(d['label_next'].cpu()) != 0).sum())
        st.update_from_device_batch(d['aci'], d['g_event_ts'])
    return ba_sums, ba_clicks, loss


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      CHAM_DIST_BACKEND="gloo")
    assert parallel.init_from_env() == (rank, world)
    p = _params()
    batches = _batches(p)
    train, ev = _models(p)
    dp = parallel.DataParallelNAR(ev)
    assert parallel.attach_data_parallel(ev) is dp and ev.dp is dp and train.rt.dp is dp       # one wrapper per runtime
    st = _warm_state(p, batches)
    before = dict(dp.collective_calls)
    _, _, loss = _evaluate(ev, st, batches[2:], lambda f, l, s: dp.upload(f, l), [rank], dp=dp)
    ba = ev._ba_buffers
    sums = torch.cat([torch.tensor([loss], dtype=torch.float64, device=ba['sums'].device), ba['sums']])
    red = dp.reduce_eval_records(ev._rh['hist'], ev._rh['pop_sum'], counts=ba['clicks'], sums=sums, rec_map=ba['rec'], clk_map=ba['clk'])
    torch.cuda.synchronize()
    out = dict(hist=red['hist'].cpu().numpy(), pop_sum=red['pop_sum'].cpu().numpy(), clicks=red['counts'].cpu().numpy(),
               sums=red['sums'].cpu().numpy(), cov=np.asarray(red['coverage_counts']),
               reductions=dp.collective_calls['eval_reduce'] - before.get('eval_reduce', 0))
    # ---- (c) a global batch of ONE session: rank 1 has no rows
    f1, l1 = _one_session(batches[-1])
    assert parallel.attach_data_parallel(train) is dp and train.dp is dp
    train.feed_state(st, st)
    d = dp.upload(f1, l1)
    assert bool(d.get('empty')) == (rank == 1) and (d['B'], d['Bg']) == (1 - rank, 1)
    train.train_step(d)
    out['one_loss'] = dp.global_loss().cpu().numpy()
    st.update_from_device_batch(d['aci'], d['g_event_ts'])
    dp.attach(ev)
    ev.enable_rank_histogram(TOPN, T_CAP)
    ev._ba = None
    ev.feed_state(st, st)
    ev.evaluate_step(dp.upload(f1, l1))
    red1 = dp.reduce_eval_records(ev._rh['hist'], ev._rh['pop_sum'])
    torch.cuda.synchronize()
    out.update(one_hist=red1['hist'].cpu().numpy(), one_own=ev.rank_histogram()[0], one_flat=train.rt.flat.cpu().numpy(),
               one_m=train.rt.m.cpu().numpy(), one_step=train.rt.global_step)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), **out)
    dist.destroy_process_group()


def test_two_rank_evaluation_equals_the_sequential_shards(gpu, tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(str(tmp_path / "rank0.npz")), np.load(str(tmp_path / "rank1.npz"))
    for k in r0.files:
        if k != 'one_own':
            assert np.array_equal(r0[k], r1[k]), k                                    # every rank holds the same numbers
    assert int(r0['reductions']) == 1
    # ---- one process, the same two row shards one after the other
    p = _params()
    batches = _batches(p)
    train, ev = _models(p)
    st = _warm_state(p, batches)

    def shard(f, l, r):
        b, e = parallel.shard_rows(48, r, 2)
        fs, ls = parallel.slice_batch(f, l, b, e)
        return ev.upload_batch(fs, ls, f, l, row_begin=b)
    ba_sums, ba_clicks, loss = _evaluate(ev, st, batches[2:], shard, [0, 1])
    hist, pop_sum = ev.rank_histogram()
    n_clicks = sum(int((l['label_next_item'] != 0).sum()) for _, l in batches[2:])
    assert int(hist.sum()) == n_clicks == ba_clicks == int(r0['clicks'][0])
    assert np.array_equal(r0['hist'], hist)
    # (pop_sum: each rank's sum is the sequential run's partial sum of that shard; the two are added in the other association)
    assert np.array_equal(r0['pop_sum'], pop_sum) or np.abs(r0['pop_sum'] - pop_sum).max() <= n_clicks * 2.0 ** -52 * np.abs(pop_sum).max()
    assert tuple(r0['cov']) == ev.coverage_counts() and r0['cov'][0] > 0
    rel = n_clicks * 2.0 ** -52
    assert abs(r0['sums'][0] - loss) <= 1e-6 * abs(loss)
    with np.errstate(invalid='ignore'):
        got, want = r0['sums'][1:] / n_clicks, ba_sums / n_clicks
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert ok[:3].all() and (np.abs(got - want)[ok] <= rel * np.abs(want)[ok]).all(), (got, want)
    # ---- not asserted: the UNsharded evaluation of the same batches (is a row's probability bit-independent of the batch's row count?)
    _, ev_u = _models(p)
    st_u = _warm_state(p, batches)
    _evaluate(ev_u, st_u, batches[2:], lambda f, l, s: ev_u.upload_batch(f, l), [0])
    hist_u, _ = ev_u.rank_histogram()
    a, b = M.accuracy_from_rank_hist(hist, None, TOPN)['hitrate_at_n'], M.accuracy_from_rank_hist(hist_u, None, TOPN)['hitrate_at_n']
    print("sharded vs unsharded evaluation: %d of %d histogram bins differ, HitRate@%d %.6f vs %.6f (difference %.3g); %d clicks by rank bin %s"
          % (int((hist != hist_u).sum()), hist.size, TOPN, a, b, a - b, n_clicks, hist.sum(0).tolist()))
    # ---- (c) the batch of one session: the single-process step and evaluation
    f1, l1 = _one_session(batches[-1])
    train.feed_state(st, st)
    d = train.upload_batch(f1, l1)
    train.train_step(d)
    one_loss = train.total_loss.cpu().numpy()
    st.update_from_device_batch(d['aci'], d['g_event_ts'])
    ev.enable_rank_histogram(TOPN, T_CAP)
    ev._ba = None
    ev._eval_iter = N_EVAL
    ev.feed_state(st, st)
    ev.evaluate_step(ev.upload_batch(f1, l1))
    assert int(r0['one_step']) == train.rt.global_step == 1
    assert not r1['one_own'].any() and np.array_equal(r0['one_own'], r0['one_hist'])      # the rank without rows added nothing
    assert np.array_equal(r0['one_hist'], ev.rank_histogram()[0]) and int(r0['one_hist'].sum()) == int((l1['label_next_item'] != 0).sum())
    assert np.abs(r0['one_loss'] - one_loss).max() < 2e-5, (r0['one_loss'], one_loss)
    H.assert_flat_close(train.rt.layout, r0['one_flat'], r0['one_m'], train.rt.flat, train.rt.m, p['lr'], n_steps=1, m_tol=1e-4)
