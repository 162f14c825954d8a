#!/usr/bin/env python
"""Per-batch cost of the full-candidate evaluation (--eval_full_candidates; nar/full_eval.py, csrc/eval_full.hip) at the
G1 eval shape (B 256, T 20, 46 000 articles, C 1024, 50 sampled negatives), for G1-like and full session lengths and K = 500 / 2 000
synthetic recent ids.  Per case: wall time of one evaluate_step with the feature on and, on the same batches in the same run, with it off
(host clock around the call + a device synchronisation), the chunk width, chunk and row-block counts it chose, and the device-event time of
the new kernels alone - as many cham_eval_full_rank_merge / _scatter launches as the step makes, on the step's own buffers.

  python scripts/bench_eval_full.py [--iters 10] [--out DIR]

One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chameleon_recsys_amd._lib import check, ptr                                            # noqa: E402
from chameleon_recsys_amd.nar import predict, synthetic                                      # noqa: E402
from chameleon_recsys_amd.nar.nar_model import NARRuntime                                    # noqa: E402
from scripts.bench_predict import B, N_ITEMS, T, make_model, state_with                      # noqa: E402


def median_wall(fn, iters, warmup=2):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        t0 = time.perf_counter(); fn(warmup + i); torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), float(np.min(ms))


def new_kernels_ms(model, d, last):
    """Device time of blocks x chunks merges + blocks scatters at the step's shapes (the plan's logits as they stand)."""
    rt, lib, dev = model.rt, model.rt.lib, model.rt.device
    Rb, Nc, blocks, chunks = d['B'], last['Nc'], last['blocks'], last['chunks']
    cand, K_dev, K, _ = predict._candidates(model, None)
    plc = rt.plan(Rb, 1, Nc, model.negative_sample_from_buffer, Rb)
    labels = d['ln_rows'][:Rb].contiguous()
    sess = torch.arange(Rb, dtype=torch.int32, device=dev)
    flat = (sess * d['T']).contiguous()
    beat, comp = torch.zeros(Rb, dtype=torch.int32, device=dev), torch.zeros(Rb, dtype=torch.int32, device=dev)
    rank, n_comp = torch.zeros(Rb * d['T'], dtype=torch.int32, device=dev), torch.zeros(Rb * d['T'], dtype=torch.int32, device=dev)
    s = rt.stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(blocks):
        for j in range(chunks):
            check(lib.cham_eval_full_rank_merge(ptr(plc.logits), ptr(cand), ptr(K_dev), j, Nc, ptr(labels), ptr(sess), ptr(d['aci']), d['T'] + 1,
                                                Rb, ptr(beat), ptr(comp), s), "merge")
        check(lib.cham_eval_full_rank_scatter(ptr(beat), ptr(comp), ptr(flat), Rb, ptr(rank), ptr(n_comp), s), "scatter")
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None, help='also append the JSON line to DIR/bench_eval_full.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_full.py needs a ROCm device")
    p = synthetic.default_params(N_ITEMS, 250, seq_len=T, batch_size=B, neg=50, neg_from_buffer=3000, buffer_size=20000, for_norm=2000,
                                 C=1024, H=255)
    rt = NARRuntime(p, seed=3)
    model = make_model(p, rt)
    n_b = 4
    res = dict(bench='eval_full', B=B, iters=args.iters, cases=[])
    for dist in ('g1', 'full'):
        batches = synthetic.make_batches(n_b, B, T, N_ITEMS, p['session_features_config'], length_dist=dist, sessions_per_hour=4 * B)
        ts = int(batches[0][0]['event_timestamp'].max())
        dev_b = [model.upload_batch(f, l) for f, l in batches]
        valid = int(sum((l['label_next_item'] != 0).sum() for _, l in batches) / n_b)
        for K in (500, 2000):
            st = state_with(p, K, ts)

            def run(i):
                model.feed_state(st, st)
                model.evaluate_step(dev_b[i % n_b])
            model._fr = None
            off_med, off_min = median_wall(run, args.iters)
            model.enable_full_candidate_ranking(10, 32)
            on_med, on_min = median_wall(run, args.iters)
            last = model.full_rank_outputs()
            assert last['K'] == K, (last['K'], K)
            model.feed_state(st, st)
            nk = new_kernels_ms(model, dev_b[(args.iters + 1) % n_b], last)
            model._fr = None
            res['cases'].append(dict(length_dist=dist, T=batches[0][0]['item_clicked'].shape[1], valid_clicks=valid, K=K, Nc=last['Nc'],
                                     chunks=last['chunks'], blocks=last['blocks'], evaluate_step_full_ms=round(on_med, 3),
                                     evaluate_step_full_min_ms=round(on_min, 3), evaluate_step_ms=round(off_med, 3),
                                     evaluate_step_min_ms=round(off_min, 3), ratio=round(on_med / off_med, 2), new_kernels_ms=round(nk, 4),
                                     new_kernels_share=round(nk / max(on_med - off_med, 1e-9), 4)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_eval_full.jsonl'), 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
