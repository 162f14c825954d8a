"""The NAR trainer data-parallel: nar_trainer_gcom's hourly train -> evaluate loop on two ranks (both on the one GPU of a test box, gloo
transport: CHAM_DIST_BACKEND=gloo) against the same loop in one process.  33 sessions per hour at a GLOBAL batch of 16: every hour ends in
a batch of ONE session, so the second rank has no rows there - in training and in evaluation.  Also the launch line of the README,
executed: `python -m torch.distributed.run ... -m chameleon_recsys_amd.nar.nar_trainer_gcom`."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from chameleon_recsys_amd.nar import nar_trainer_gcom as T
from chameleon_recsys_amd.nar import parallel, synthetic
from tests import helpers as H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARGS = ['--batch_size', '16', '--truncate_session_length', '8', '--learning_rate', '1e-3', '--reg_l2', '1e-5',
        '--softmax_temperature', '0.2', '--recent_clicks_buffer_max_size', '600', '--recent_clicks_for_normalization', '100',
        '--eval_metrics_top_n', '5', '--CAR_embedding_size', '128', '--rnn_units', '100', '--train_total_negative_samples', '8',
        '--train_negative_samples_from_buffer', '300', '--eval_total_negative_samples', '8', '--eval_negative_samples_from_buffer', '300',
        '--training_hours_for_each_eval', '1', '--save_results_each_n_evals', '1', '--clicked_items_state', 'device',
        '--disable_eval_benchmarks', '--eval_beyond_accuracy_metrics', '--eval_metrics_by_session_position']


def _argv(data_dir, model_dir):
    return ARGS + ['--train_set_path_regex', os.path.join(data_dir, "sessions_hour_*.tfrecord.gz"),
                   '--acr_module_articles_metadata_csv_path', os.path.join(data_dir, 'articles_metadata.csv'),
                   '--acr_module_articles_content_embeddings_pickle_path', os.path.join(data_dir, 'articles_embeddings.pickle'),
                   '--model_dir', model_dir]


def _dataset(tmp_path):
    d = str(tmp_path / "data")
    synthetic.write_dataset(d, 3, 33, 1000, 16, seq_len=8)
    return d


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _plain(log):
    """The metrics log as JSON-comparable values."""
    conv = lambda v: {str(k): conv(x) for k, x in v.items()} if isinstance(v, dict) else (v.item() if hasattr(v, 'item') else v)
    return [conv(e) for e in log]


def _worker(rank, world, port, data_dir, model_dir, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      CHAM_DIST_BACKEND="gloo")
    writes = dict(ckpt=0, csv=0)
    save, csv = torch.save, T.save_eval_benchmark_metrics_csv

    def counted_save(*a, **k):
        writes['ckpt'] += 1
        return save(*a, **k)

    def counted_csv(*a, **k):
        writes['csv'] += 1
        return csv(*a, **k)
    torch.save, T.save_eval_benchmark_metrics_csv = counted_save, counted_csv
    est = T.main(_argv(data_dir, model_dir))
    assert not torch.distributed.is_initialized()                  # the loop created the group: it destroyed it on the way out
    rt = est._store['runtime']
    assert rt.dp.world == world and rt.dp.rank == rank
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as fh:
        json.dump(dict(log=_plain(T.eval_sessions_metrics_log), global_step=est.global_step, writes=writes,
                       broadcasts=rt.dp.collective_calls['broadcast'], eval_reduce=rt.dp.collective_calls['eval_reduce']), fh)
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), flat=rt.flat.cpu().numpy(), m=rt.m.cpu().numpy(), v=rt.v.cpu().numpy())


def test_two_rank_trainer_equals_the_single_process_trainer(gpu, tmp_path):
    data = _dataset(tmp_path)
    dp_dir, one_dir = str(tmp_path / "model_dp"), str(tmp_path / "model_one")
    mp.spawn(_worker, args=(2, _free_port(), data, dp_dir, str(tmp_path)), nprocs=2, join=True)
    r = [json.load(open(str(tmp_path / ("rank%d.json" % k)))) for k in range(2)]
    w = [np.load(str(tmp_path / ("rank%d.npz" % k))) for k in range(2)]
    est = T.main(_argv(data, one_dir))
    log = _plain(T.eval_sessions_metrics_log)
    assert r[0]['global_step'] == r[1]['global_step'] == est.global_step == 6         # 2 training hours x (16 + 16 + 1 sessions)
    # checkpoint and CSV are written once: by rank 0
    assert r[0]['writes']['ckpt'] >= 1 and r[0]['writes']['csv'] >= 1 and r[1]['writes'] == dict(ckpt=0, csv=0)
    assert sorted(os.listdir(dp_dir)) == sorted(os.listdir(one_dir)) == ['eval_stats_benchmarks.csv', 'model.ckpt.pt']
    assert r[0]['broadcasts'] == 1 and r[0]['eval_reduce'] == 2                        # one wrapper per runtime; one reduction per evaluation
    # every rank holds the same numbers
    assert json.dumps(r[0]['log'], sort_keys=True) == json.dumps(r[1]['log'], sort_keys=True)      # (as text: a NaN equals itself)
    assert len(log) == len(r[0]['log']) == 2
    for k in ('flat', 'm', 'v'):
        assert np.array_equal(w[0][k], w[1][k]), k
    for got, want in zip(r[0]['log'], log):
        assert set(got) == set(want)
        assert got['clicks_count'] == want['clicks_count'] and got['sessions_count'] == want['sessions_count'] == 33
        assert sum(v for k, v in got.items() if k.startswith('clicks_at_pos_chameleon_')) == \
            sum(v for k, v in want.items() if k.startswith('clicks_at_pos_chameleon_'))
        assert 0.0 < got['hitrate_at_n_chameleon'] <= 1.0 and got['hitrate_at_n'] == got['hitrate_at_n_chameleon']
    sd = torch.load(os.path.join(dp_dir, 'model.ckpt.pt'), map_location='cpu', weights_only=True)
    assert np.array_equal(sd['flat'].numpy(), w[0]['flat']) and sd['global_step'] == 6
    rt = est._store['runtime']
    H.assert_flat_close(rt.layout, w[0]['flat'], w[0]['m'], rt.flat, rt.m, 1e-3, n_steps=6, m_tol=1e-4)


@pytest.mark.parametrize("flag", ['--eval_cold_start', '--save_eval_sessions_negative_samples', '--save_eval_sessions_recommendations'])
def test_flags_that_need_one_hosts_ranked_lists_are_refused(gpu, tmp_path, monkeypatch, flag):
    monkeypatch.setattr(parallel, 'init_from_env', lambda: (0, 2))
    data = str(tmp_path / "data")
    os.makedirs(data)
    import pickle
    with open(os.path.join(data, 'articles_embeddings.pickle'), 'wb') as fh:
        pickle.dump(np.ones((4, 3), np.float32), fh)
    with open(os.path.join(data, 'articles_metadata.csv'), 'w') as fh:
        fh.write("article_id,created_at_ts,category_id\n" + "".join("%d,0,1\n" % i for i in range(4)))
    with pytest.raises(ValueError, match=flag):
        T.main(_argv(data, str(tmp_path / "model")) + [flag])
    assert not os.path.exists(str(tmp_path / "model"))


def test_the_trainer_under_the_launch_line(gpu, tmp_path):
    data, model_dir = _dataset(tmp_path), str(tmp_path / "model")
    env = dict(os.environ, CHAM_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "-m", "chameleon_recsys_amd.nar.nar_trainer_gcom"] + _argv(data, model_dir)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "rc %d\n%s" % (r.returncode, r.stderr[-3000:])
    assert sorted(os.listdir(model_dir)) == ['eval_stats_benchmarks.csv', 'model.ckpt.pt']
    assert sum(line.startswith("INFO:eval ") for line in r.stdout.splitlines()) == 2              # rank 0 speaks for both
    rows = open(os.path.join(model_dir, 'eval_stats_benchmarks.csv')).read().strip().splitlines()
    assert len(rows) == 3 and 'hitrate_at_n_chameleon' in rows[0] and 'sessions_count' in rows[0]
