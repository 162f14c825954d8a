#!/usr/bin/env python
"""Per-batch cost of the baseline recommenders of the evaluation (nar/baselines.py, csrc/baselines.hip, csrc/vsknn.hip) at the G1 eval
shape (B 256, T 20, 1 + N = 51 candidates, D 250, topn 10, 46 000 articles, G1-like session lengths), with pair tables and the V-SkNN
session ring (3000 sessions: full after 12 batches) learned from --learn-batches batches first:

  * score + rank + histogram of all baselines together, and of the four without 'v-sknn' (device events around
    DeviceBaselines.evaluate); score + rank of each baseline alone;
  * learn (the co-occurrence and sequential-rules inserts, host growth rule included, and the ring append), and the ring append alone;
  * the model's own evaluate_step on the same batches, from the same run - what the baselines are measured against;
  * the eager train_step without and with learn() behind it (learn also runs in TRAIN mode).

  python scripts/bench_eval_baselines.py [--iters 30] [--learn-batches 200] [--length-dist g1|full] [--out DIR]

One JSON line.  The reference's four Python classes on a batch of the same shape are timed on the host by
scripts/make_golden_baselines.py --time_g1."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chameleon_recsys_amd.nar import synthetic                                              # noqa: E402
from chameleon_recsys_amd.nar.baselines import BASELINE_NAMES, DeviceBaselines              # noqa: E402
from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState            # noqa: E402
from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime          # noqa: E402

N_ITEMS, B, T = 46000, 256, 20


def timed(fn, iters, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(iters):
        e0.record(); fn(warmup + i); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def make_model(mode, p, rt):
    neg, from_buf = ('train_total_negative_samples', 'train_negative_samples_from_buffer') if mode == ModeKeys.TRAIN else \
        ('eval_total_negative_samples', 'eval_negative_samples_from_buffer')
    return NARModuleModel(mode, None, None, p['session_features_config'], p['articles_features_config'], B, p['lr'], 1.0,
                          p[neg], p[from_buf], p['content_article_embeddings_matrix'],
                          softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                          recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                          recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                          CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], metrics_top_n=10, runtime=rt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--learn-batches', type=int, default=200)
    ap.add_argument('--length-dist', default='g1', choices=['g1', 'full'], help="session lengths: G1-like, or full (bench.py's headline batch)")
    ap.add_argument('--out', default=None, help='also append the JSON line to DIR/bench_eval_baselines.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_baselines.py needs a ROCm device")
    dev = torch.device('cuda:0')
    p = synthetic.default_params(N_ITEMS, 250, seq_len=T, batch_size=B, neg=50, neg_from_buffer=3000, buffer_size=20000, for_norm=2000,
                                 C=1024, H=255)
    rt = NARRuntime(p, seed=3)
    train, evalm = make_model(ModeKeys.TRAIN, p, rt), make_model(ModeKeys.EVAL, p, rt)
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'],
                                 N_ITEMS)
    bl = DeviceBaselines(BASELINE_NAMES, N_ITEMS, rt.ace, device=dev)
    n_b = 8
    batches = synthetic.make_batches(n_b, B, T, N_ITEMS, p['session_features_config'], length_dist=args.length_dist, sessions_per_hour=4 * B)
    dev_b = [train.upload_batch(f, l) for f, l in batches]
    # tables of a realistic size: sessions drawn like the batches' (fresh ids every pass, so the maps keep growing)
    rng = np.random.default_rng(0)
    sid = {'next': 0}

    def session_ids(rows):                       # ascending session ids, as a stream has them
        sid['next'] += rows
        return torch.arange(sid['next'] - rows, sid['next'], dtype=torch.int64, device=dev)
    for k in range(args.learn_batches):
        aci = dev_b[k % n_b]['aci']
        shift = torch.from_numpy(rng.integers(0, N_ITEMS - 1, size=(aci.shape[0], 1))).to(dev)
        bl.learn(torch.where(aci != 0, (aci + shift) % (N_ITEMS - 1) + 1, aci), session_ids(aci.shape[0]))
    bl.check_tables()
    entries = {n: t.counters()[1] for n, t in bl.tables.items()}
    caps = {n: t.cap for n, t in bl.tables.items()}

    def train_step(i, learn=False):
        d = dev_b[i % n_b]
        train.feed_state(st, st)
        train.train_step(d)
        if learn:
            bl.learn(d['aci'], session_ids(B))
        st.update_from_device_batch(d['aci'], d['g_event_ts'])
    out = dict(shape=dict(B=B, T=T, NC=51, D=250, topn=10, n_items=N_ITEMS), length_dist=args.length_dist, valid_clicks=int(dev_b[0]['P']), table_entries=entries,
               table_slots=caps)
    out['train_step_ms_median'], out['train_step_ms_min'] = timed(lambda i: train_step(i), args.iters, warmup=6)
    out['train_step_with_learn_ms_median'], out['train_step_with_learn_ms_min'] = timed(lambda i: train_step(i, True), args.iters)
    bl.begin_evaluation(10)
    state = {}

    def eval_step(i):
        d = state['d'] = dev_b[i % n_b]
        evalm.feed_state(st, st)
        evalm.evaluate_step(d)
    out['evaluate_step_ms_median'], out['evaluate_step_ms_min'] = timed(eval_step, args.iters)
    d, pl = state['d'], evalm._plan

    def baselines(i):
        bl.evaluate(d['item_clicked'], d['label_next'], pl.neg_ids, st.recent_pop)
    out['baselines_evaluate_ms_median'], out['baselines_evaluate_ms_min'] = timed(baselines, args.iters)
    bl.names = BASELINE_NAMES[:4]                # the four without the neighbour search
    out['four_baselines_evaluate_ms_median'], out['four_baselines_evaluate_ms_min'] = timed(baselines, args.iters)
    bl.names = BASELINE_NAMES
    for name in BASELINE_NAMES:
        med, mn = timed(lambda i: bl.score_and_rank(name, d['item_clicked'], d['label_next'], pl.neg_ids, st.recent_pop), args.iters)
        out['score_rank_%s_ms_median' % name] = med
    out['learn_ms_median'], out['learn_ms_min'] = timed(lambda i: bl.learn(dev_b[i % n_b]['aci'], session_ids(B)), args.iters)
    out['learn_v-sknn_ms_median'], out['learn_v-sknn_ms_min'] = timed(lambda i: bl.ring.append(dev_b[i % n_b]['aci'], session_ids(B), N_ITEMS),
                                                                      args.iters)
    out['ring_sessions'] = min(bl.ring.appended, bl.ring.size)
    bl.check_tables()
    out['results'] = {k: float(v) for k, v in bl.results(10).items()}
    out['baselines_vs_evaluate_step'] = out['baselines_evaluate_ms_median'] / out['evaluate_step_ms_median']
    out['four_baselines_vs_evaluate_step'] = out['four_baselines_evaluate_ms_median'] / out['evaluate_step_ms_median']
    out['v-sknn_vs_evaluate_step'] = out['score_rank_v-sknn_ms_median'] / out['evaluate_step_ms_median']
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_eval_baselines.jsonl'), 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
