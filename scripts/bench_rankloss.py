#!/usr/bin/env python
"""Cost of the loss kernels under each --loss_function (csrc/rank_loss.hip beside the softmax pair of csrc/scorer.hip) at the G1 bench shape.

  rocprofv3 --kernel-trace --output-format csv -d DIR -o rl -- python scripts/bench_rankloss.py --steps 10     # the run
  python scripts/bench_rankloss.py --summarise DIR --steps 10                                                  # per-loss kernel times from its trace

The run: one eager training model per loss at the G1 model shape (synthetic.default_params: 256 full-length sessions x 19 clicks, 50
negatives, C 1024), softmax first, --warmup + --steps train_step calls each; one JSON line per loss with the step time under device events.
The four ranking losses share one kernel pair (the loss kind is a launch argument), so --summarise attributes the dispatches of
k_score_rankloss_fwd / _bwd to the losses by their order in the trace: (warmup + steps) dispatches per loss, the last `steps` of each timed."""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOSSES = ('softmax', 'bpr', 'top1', 'bpr_max', 'top1_max')


def run(loss, steps, warmup, B=256):
    import torch
    from chameleon_recsys_amd.nar import synthetic
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p = synthetic.default_params(46000, 250, seq_len=20, batch_size=B, neg=50, neg_from_buffer=3000, buffer_size=20000, for_norm=2000, C=1024, H=255)
    rt = NARRuntime(p, seed=3)
    model = NARModuleModel(ModeKeys.TRAIN, None, None, p['session_features_config'], p['articles_features_config'], B, p['lr'], 1.0,
                           p['train_total_negative_samples'], p['train_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                           softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                           recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                           recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                           CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], runtime=rt, loss_function=loss)
    batches = synthetic.make_batches(4, B, 20, 46000, p['session_features_config'], length_dist='full', sessions_per_hour=4 * B)
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], 46000)
    dev_b = [model.upload_batch(f, l) for f, l in batches]

    def step(i):
        d = dev_b[i % len(dev_b)]
        model.feed_state(st, st)
        model.train_step(d)
        st.update_from_device_batch(d['aci'], d['g_event_ts'])
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for i in range(steps):
        e0.record(); step(warmup + i); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    loss_v = [float(x) for x in model.total_loss.cpu()]
    assert all(np.isfinite(loss_v)), loss_v
    out = dict(loss_function=loss, clicks=int(dev_b[0]['P']), step_ms_median=float(np.median(ms)), step_ms_min=float(np.min(ms)), last_loss=loss_v)
    del model, rt
    torch.cuda.empty_cache()
    return out


def summarise(directory, steps, warmup):
    files = glob.glob(os.path.join(directory, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % directory)
    rows = []
    for f in files:
        with open(f, newline='') as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']))
    rows.sort()
    per = warmup + steps
    for tag in ('fwd', 'bwd'):
        soft = [(e - s) / 1e3 for s, e, n in rows if 'k_score_softmax_' + tag in n]
        rank = [(e - s) / 1e3 for s, e, n in rows if 'k_score_rankloss_' + tag in n]
        assert len(soft) == per and len(rank) == per * (len(LOSSES) - 1), (tag, len(soft), len(rank))
        groups = [soft] + [rank[i * per:(i + 1) * per] for i in range(len(LOSSES) - 1)]
        for loss, g in zip(LOSSES, groups):
            t = g[warmup:]
            print(json.dumps(dict(kernel='k_score_%s_%s' % ('softmax' if loss == 'softmax' else 'rankloss', tag), loss_function=loss, dispatches=len(t),
                                  us_median=float(np.median(t)), us_min=float(np.min(t)), us_max=float(np.max(t)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--summarise', default=None, metavar='DIR', help='read the kernel trace under DIR instead of running')
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.steps, args.warmup)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rankloss.py needs a ROCm device")
    for loss in LOSSES:
        print(json.dumps(run(loss, args.steps, args.warmup)), flush=True)


if __name__ == '__main__':
    main()
