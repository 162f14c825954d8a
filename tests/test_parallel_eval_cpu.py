"""DataParallelNAR.reduce_eval_records on CPU tensors with the gloo backend, worlds 2 and 3: the evaluation's per-rank records - int64
rank histogram and counts, fp64 sums, uint8 coverage maps - become global records, identical on every rank, in ONE reduction per
evaluation.  (The records themselves come from HIP kernels: tests/test_rank_hist_gpu.py, tests/test_dp_eval_gpu.py.)"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from chameleon_recsys_amd.nar import parallel

T_CAP, TOPN, N_ITEMS = 7, 5, 203


def _records(rank):
    """A rank's records: large int64 counts (sums beyond 2^53 must stay exact), fp64 sums, sparse maps."""
    rng = np.random.default_rng(40 + rank)
    hist = rng.integers(0, 1 << 40, size=(T_CAP, TOPN + 1)).astype(np.int64)
    hist[0, 0] = (1 << 61) + rank                                  # not representable in fp64
    return dict(hist=hist, pop_sum=rng.random(T_CAP), counts=rng.integers(0, 1000, size=2).astype(np.int64), sums=rng.random(7) * 100,
                rec=(rng.random(N_ITEMS) < 0.1).astype(np.uint8), clk=(rng.random(N_ITEMS) < 0.2).astype(np.uint8))


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), CHAM_DIST_BACKEND="gloo")
    assert parallel.init_from_env() == (rank, world)
    assert parallel.init_from_env() == (rank, world)               # idempotent: the group exists
    torch.set_num_threads(1)

    class _RT:
        flat = torch.full((4,), float(rank))
        dp_rank = dp_world = dp_allreduce = None

    class _Model:
        rt = _RT()
    dp = parallel.DataParallelNAR(_Model())
    assert dp.active and _Model.rt.dp is dp and float(_RT.flat[0]) == 0.0    # one wrapper per runtime; rank 0's weights everywhere
    before = dict(dp.collective_calls)
    r = {k: torch.from_numpy(v.copy()) for k, v in _records(rank).items()}
    red = dp.reduce_eval_records(r['hist'], r['pop_sum'], counts=r['counts'], sums=r['sums'], rec_map=r['rec'], clk_map=r['clk'])
    assert torch.equal(r['hist'], torch.from_numpy(_records(rank)['hist']))    # the rank's own record is not modified
    calls = {k: dp.collective_calls[k] - before.get(k, 0) for k in dp.collective_calls}
    # ... and without the optional parts
    red2 = dp.reduce_eval_records(r['hist'], r['pop_sum'])
    assert red2['counts'] is None and red2['sums'] is None and torch.equal(red2['hist'], red['hist'])
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), hist=red['hist'].numpy(), pop_sum=red['pop_sum'].numpy(),
             counts=red['counts'].numpy(), sums=red['sums'].numpy(), rec=r['rec'].numpy(), clk=r['clk'].numpy(),
             calls=np.asarray([calls['eval_reduce'], calls['all_reduce'], calls['reduce_scatter'], calls['all_gather'], calls['broadcast']]))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_reduce_eval_records(tmp_path, world):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    got = [np.load(str(tmp_path / ("rank%d.npz" % r))) for r in range(world)]
    mine = [_records(r) for r in range(world)]
    # int64 sums exact (Python integers as the reference)
    want_hist = np.asarray([sum(int(m['hist'].reshape(-1)[i]) for m in mine) for i in range(T_CAP * (TOPN + 1))], dtype=np.int64)
    assert np.array_equal(got[0]['hist'].reshape(-1), want_hist) and got[0]['hist'].shape == (T_CAP, TOPN + 1)
    assert np.array_equal(got[0]['counts'], sum(m['counts'] for m in mine))
    # fp64 sums: `world` terms in some order - within (world - 1) roundings of the exact sum
    for k in ('pop_sum', 'sums'):
        want = sum(m[k] for m in mine)
        assert np.abs(got[0][k] - want).max() <= (world - 1) * 2.0 ** -52 * np.abs(want).max()
    # the maps: union
    assert np.array_equal(got[0]['rec'], np.maximum.reduce([m['rec'] for m in mine]))
    assert np.array_equal(got[0]['clk'], np.maximum.reduce([m['clk'] for m in mine]))
    # every rank ends with identical records, bit for bit
    for g in got[1:]:
        for k in ('hist', 'pop_sum', 'counts', 'sums', 'rec', 'clk'):
            assert np.array_equal(g[k], got[0][k]), k
    # ONE reduction: one packed int64 SUM, one packed fp64 SUM, a MAX per map - and nothing else
    for g in got:
        assert g['calls'].tolist() == [1, 4, 0, 0, 0]


def test_world_of_one_needs_no_group(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert parallel.init_from_env() == (0, 1)
    assert not dist.is_initialized()
