#!/usr/bin/env python
"""Per-batch cost of NARModuleModel.predict_step (nar/predict.py, csrc/predict.hip) at the G1 eval shape (B 256, T 20, 46 000 articles,
C 1024, topn 10) over K = 500 / 2 000 / 5 000 synthetic recent ids, with the model's own evaluate_step on the same batches from the same run
beside it.  Per K: wall time of one predict_step (host clock around the call - it ends with the read-back of the lists), the chunk width Nc
it chose and the number of chunks, and device-event times of its parts on the last batch: the candidate set, the input-click stages, and per
chunk the reused forward (fill excluded) and the new kernels (chunk fill + top-n merge).

  python scripts/bench_predict.py [--iters 30] [--length-dist g1|full] [--out DIR]

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
from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState            # noqa: E402
from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime          # noqa: E402

N_ITEMS, B, T, TOPN = 46000, 256, 20, 10


def make_model(p, rt):
    m = NARModuleModel(ModeKeys.EVAL, None, None, p['session_features_config'], p['articles_features_config'], B, p['lr'], 1.0,
                       p['eval_total_negative_samples'], p['eval_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                       softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                       recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                       recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                       CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], metrics_top_n=10, runtime=rt)
    m.predict_train_negative_samples = p['train_total_negative_samples']
    return m


def state_with(p, K, ts):
    """A device-resident state whose buffer holds K distinct recent ids (1.5 K clicks, Zipf-like repeats)."""
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], N_ITEMS)
    rng = np.random.default_rng(K)
    ids = rng.choice(np.arange(1, N_ITEMS), K, replace=False)
    clicks = np.concatenate([ids, rng.choice(ids, K // 2)])
    st.update_items_state(clicks, np.full(clicks.shape, ts, np.int64))
    return st


def median_wall(fn, iters, warmup=3):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        t0 = time.perf_counter(); fn(warmup + i); torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ms)), float(np.min(ms))


def parts(model, d, out):
    """Device-event times of the parts of one predict_step on batch d (the chunk width and count of `out`)."""
    rt, lib = model.rt, model.rt.lib
    ev = lambda: torch.cuda.Event(enable_timing=True)
    marks = []

    def mark(name):
        e = ev(); e.record(); marks.append((name, e))
    torch.cuda.synchronize()
    mark('start')
    cand, K_dev, K, _ = predict._candidates(model, None)
    mark('candidates')
    pl = predict._input_clicks(model, d)
    mark('input_clicks')
    P_last, d2, Nc = d['P_last'], d['last'], out['Nc']
    plc = rt.plan(P_last, 1, Nc, model.negative_sample_from_buffer, P_last)
    plc.pos, plc.P, plc.PC = None, P_last, P_last * plc.NC
    s = rt.stream()
    check(lib.cham_rows_gather(ptr(pl.pred), ptr(d2['rows']), P_last, rt.layout.C, ptr(plc.pred), s), "cham_rows_gather")
    plc.cur_neg_ids, plc.cur_neg_slot = plc.neg_ids, plc.neg_slot
    top_id = torch.zeros(P_last, TOPN, dtype=torch.int64, device=rt.device)
    top_score = torch.full((P_last, TOPN), float('-inf'), dtype=torch.float32, device=rt.device)
    ms = torch.zeros(P_last, 2, dtype=torch.float32, device=rt.device); ms[:, 0] = float('-inf')
    tau = float(model.softmax_temperature)
    for j in range(out['chunks']):
        mark('_')
        check(lib.cham_predict_fill_chunk(ptr(cand), ptr(K_dev), j, Nc, P_last, plc.pmax, ptr(plc.neg_ids), ptr(plc.neg_slot), ptr(plc.pool), s), "fill")
        mark('new_kernels')
        predict._score_chunk(model, plc, d2, s)
        mark('reused_forward')
        check(lib.cham_predict_topn_merge(ptr(plc.logits), ptr(cand), ptr(K_dev), j, Nc, ptr(d2['excl']), d['T'], P_last, TOPN, tau, ptr(top_id),
                                          ptr(top_score), ptr(ms), s), "merge")
        mark('new_kernels')
    torch.cuda.synchronize()
    acc = {}
    for (_, a), (name, b) in zip(marks[:-1], marks[1:]):
        if name != '_':
            acc[name] = acc.get(name, 0.0) + a.elapsed_time(b)
    return {k: round(v, 4) for k, v in acc.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--length-dist', default='g1', choices=['g1', 'full'])
    ap.add_argument('--out', default=None, help='also append the JSON line to DIR/bench_predict.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_predict.py needs a ROCm device")
    p = synthetic.default_params(N_ITEMS, 250, seq_len=T, batch_size=B, neg=50, neg_from_buffer=3000, buffer_size=20000, for_norm=2000,
                                 C=1024, H=255)
    rt = NARRuntime(p, seed=3)
    model = make_model(p, rt)
    n_b = 8
    batches = synthetic.make_batches(n_b, B, T, N_ITEMS, p['session_features_config'], length_dist=args.length_dist, sessions_per_hour=4 * B)
    ts = int(batches[0][0]['event_timestamp'].max())
    res = dict(bench='predict', length_dist=args.length_dist, B=B, T=batches[0][0]['item_clicked'].shape[1], topn=TOPN, iters=args.iters,
               valid_clicks=int(sum((f['item_clicked'] != 0).sum() for f, _ in batches) / n_b), K={})
    for K in (500, 2000, 5000):
        st = state_with(p, K, ts)
        dev_e = [model.upload_batch(f, l) for f, l in batches]
        dev_p = [model.upload_predict_batch(f) for f, _ in batches]
        last = {}

        def run_eval(i):
            model.feed_state(st, st)
            model.evaluate_step(dev_e[i % n_b])

        def run_predict(i):
            model.feed_state(st, st)
            last['out'] = model.predict_step(dev_p[i % n_b], topn=TOPN)
        e_med, e_min = median_wall(run_eval, args.iters)
        p_med, p_min = median_wall(run_predict, args.iters)
        out = last['out']
        assert out['K'] == K, (out['K'], K)
        model.feed_state(st, st)
        res['K'][str(K)] = dict(predict_step_ms=round(p_med, 4), predict_step_min_ms=round(p_min, 4), evaluate_step_ms=round(e_med, 4),
                                evaluate_step_min_ms=round(e_min, 4), Nc=out['Nc'], chunks=out['chunks'], P_last=out['P_last'],
                                candidate_rows_per_chunk=out['P_last'] * (1 + out['Nc']), parts_ms=parts(model, dev_p[(args.iters + 2) % n_b], out))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_predict.jsonl'), 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
