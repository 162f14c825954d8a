#!/usr/bin/env python
"""Cost of the cosine ranking head (--recommendations_ranking cosine; csrc/cosine.hip): its kernels alone under device events, beside
k_mulpred_bwd_h2 (the MLP head's kernel of the same access pattern) in the same run, and the eager training step of both heads.

  python scripts/bench_cosine.py [--shapes g1,adressa] [--iters 30] [--step-iters 20] [--heads mlp,cosine,mlp,cosine] [--out DIR]

Kernel shapes: g1 = 4 864 clicks (256 sessions x 19 steps) x 51 candidates, C 1024; adressa = the same clicks x 101 candidates.  One JSON
line per shape: median / min ms of the forward (fp32 and bf16 rows), of the bound pass and of each backward form, the bytes each must move
(rows read once + rows written) and the rate that makes; cham_mulpred_bwd_h2 on the same shape (reads dM and Z2c, writes two planes: 3 x R C 4
bytes where the cosine backward moves 2 x).  Step: the G1 model shape (synthetic.default_params) on full-length sessions, eager
train_step, one JSON line per entry of --heads (alternating: the spread between equal runs is part of the answer)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chameleon_recsys_amd import _lib                     # noqa: E402
from chameleon_recsys_amd._lib import check, ptr         # noqa: E402

SHAPES = {'g1': dict(P=4864, N=50, C=1024), 'adressa': dict(P=4864, N=100, C=1024)}


def timed(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms))


def bench_kernels(lib, s, dev, iters):
    P, N, C = s['P'], s['N'], s['C']
    NC = N + 1
    R = P * NC
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    z = torch.tanh(torch.randn(R, C, generator=g, device=dev))
    zb = z.bfloat16()
    pred = torch.tanh(torch.randn(P, C, generator=g, device=dev))
    ds = torch.randn(R, generator=g, device=dev) / R
    mask = torch.ones(P, dtype=torch.uint8, device=dev)
    cosq, rz, rp = torch.empty(R, 4, device=dev), torch.empty(R, device=dev), torch.empty(P, device=dev)
    t, rec = torch.empty((R + 3) & ~3, device=dev), torch.zeros(8, device=dev)
    dpred, b2 = torch.empty(P, C, device=dev), torch.empty(P, C, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    out = dict(s, rows=R)

    def note(name, fn, nbytes):
        med, mn = timed(fn, iters)
        out.update({name + '_ms_median': med, name + '_ms_min': mn, name + '_bytes': nbytes, name + '_gbps': nbytes / (med * 1e-3) / 1e9})

    note('fwd_f32', lambda: check(lib.cham_cosine_fwd(ptr(z), C, ptr(pred), C, P, N, ptr(cosq), ptr(rz), ptr(rp), st), "cham_cosine_fwd"), R * C * 4)
    note('fwd_b16', lambda: check(lib.cham_cosine_fwd_b16(ptr(zb), C, ptr(pred), C, P, N, ptr(cosq), ptr(rz), ptr(rp), st), "cham_cosine_fwd_b16"), R * C * 2)
    check(lib.cham_cosine_fwd(ptr(z), C, ptr(pred), C, P, N, ptr(cosq), ptr(rz), ptr(rp), st), "cham_cosine_fwd")

    def bound():
        check(lib.cham_cosine_bound(ptr(ds), ptr(rz), R, ptr(t), st), "cham_cosine_bound")
        check(lib.cham_h2_scale_absmax(ptr(t), (R + 3) & ~3, None, 0, ptr(rec), st), "cham_h2_scale_absmax")
    note('bound', bound, R * 16)
    head = (ptr(pred), ptr(ds), ptr(rz), ptr(rp), ptr(cosq), ptr(mask), C, P, N)
    o32 = torch.empty(R, C, device=dev)
    note('bwd_f32', lambda: check(lib.cham_cosine_bwd(ptr(z), *head, ptr(o32), ptr(dpred), None, st), "cham_cosine_bwd"), 2 * R * C * 4)
    planes = torch.empty(2, R, C, dtype=torch.float16, device=dev)
    note('bwd_h2', lambda: check(lib.cham_cosine_bwd_h2(ptr(z), *head, ptr(planes), R * C, ptr(rec), ptr(dpred), ptr(b2), st), "cham_cosine_bwd_h2"),
         2 * R * C * 4)
    ob = torch.empty(R, C, dtype=torch.bfloat16, device=dev)
    note('bwd_b16', lambda: check(lib.cham_cosine_bwd_b16(ptr(zb), *head, ptr(ob), ptr(dpred), ptr(b2), st), "cham_cosine_bwd_b16"), 2 * R * C * 2)
    # the MLP head's kernel of the same shape: dM (here: any fp32 matrix) and Z2c in, two planes out
    dM = o32
    check(lib.cham_h2_scale_absmax(ptr(dM), R * C, None, 0, ptr(rec), st), "cham_h2_scale_absmax")
    note('mulpred_bwd_h2', lambda: check(lib.cham_mulpred_bwd_h2(ptr(dM), ptr(z), ptr(pred), C, P, N, ptr(dpred), ptr(planes), R * C, ptr(b2), ptr(rec), st),
                                         "cham_mulpred_bwd_h2"), 3 * R * C * 4)
    return out


def bench_step(head, iters, dev, B=256, gemm_dtype='f32'):
    """Eager train_step at the G1 model shape on full-length sessions (256 x 19 = 4 864 clicks) with a device-resident recent-clicks state."""
    from chameleon_recsys_amd.nar import synthetic
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p = synthetic.default_params(46000, 250, seq_len=20, batch_size=B, neg=50, neg_from_buffer=3000, buffer_size=20000, for_norm=2000,
                                 C=1024, H=255, recommendations_ranking=head, gemm_dtype=gemm_dtype)
    rt = NARRuntime(p, seed=3)
    model = NARModuleModel(ModeKeys.TRAIN, None, None, p['session_features_config'], p['articles_features_config'], B, p['lr'], 1.0,
                           p['train_total_negative_samples'], p['train_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                           softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                           recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                           recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                           CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], runtime=rt, gemm_dtype=gemm_dtype,
                           recommendations_ranking=head)
    batches = synthetic.make_batches(8, B, 20, 46000, p['session_features_config'], length_dist='full', sessions_per_hour=4 * B)
    st = DeviceClickedItemsState(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'], p['recent_clicks_for_normalization'], 46000)
    dev_b = [model.upload_batch(f, l) for f, l in batches]

    def step(i):
        d = dev_b[i % len(dev_b)]
        model.feed_state(st, st)
        model.train_step(d)
        st.update_from_device_batch(d['aci'], d['g_event_ts'])
    for i in range(6):
        step(i)
    torch.cuda.synchronize()
    ms = []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(iters):
        e0.record(); step(6 + i); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    loss = float(model.total_loss.cpu()[0])
    del model, rt
    torch.cuda.empty_cache()
    return dict(step_head=head, gemm_dtype=gemm_dtype, B=B, clicks=int(dev_b[0]['P']), step_ms_median=float(np.median(ms)), step_ms_min=float(np.min(ms)),
                last_loss=loss)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='g1,adressa', help="'' : no kernel leg")
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--step-iters', type=int, default=20, help='0: kernels only')
    ap.add_argument('--heads', default='mlp,cosine,mlp,cosine')
    ap.add_argument('--gemm-dtype', default='f32')
    ap.add_argument('--out', default=None, help='also append the JSON lines to DIR/bench_cosine.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cosine.py needs a ROCm device")
    lib, dev = _lib.load(), torch.device('cuda:0')
    lines = []
    for name in [n for n in args.shapes.split(',') if n]:
        lines.append(json.dumps(dict(shape=name, **bench_kernels(lib, SHAPES[name], dev, args.iters))))
        print(lines[-1], flush=True)
        torch.cuda.empty_cache()
    if args.step_iters > 0:
        for head in args.heads.split(','):
            lines.append(json.dumps(bench_step(head, args.step_iters, dev, gemm_dtype=args.gemm_dtype)))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_cosine.jsonl'), 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
