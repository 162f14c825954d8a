#!/usr/bin/env python
"""Cost of the content-diversity regulariser (--diversity_reg_factor; csrc/diversity.hip): the two kernels alone, under device events,
and the training step with and without the term.

  python scripts/bench_diversity.py [--shapes g1,adressa] [--iters 30] [--step-iters 20] [--out DIR]

Kernel shapes: g1 = 4 864 clicks (256 sessions x 19 steps), 50 negatives, D 250, 46 000 articles; adressa = the same clicks with
100 negatives over 73 000 articles.  Candidate ids are uniform over the table (every row comes from the Infinity Cache / L2, none is
shared inside a click - the sampler's popular items would make it cheaper).  One JSON line per shape: median and min ms of the forward and
of the fp32 / bf16 backward, the bytes each must move and the rate that makes.  Step: the G1 model shape (synthetic.default_params)
at factor 0 and at --factor, eager train_step, median and min ms over --step-iters steps after warm-up."""
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

SHAPES = {'g1': dict(P=4864, N=50, D=250, n_items=46_000), 'adressa': dict(P=4864, N=100, D=250, n_items=73_000)}


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
    P, N, D, n = s['P'], s['N'], s['D'], s['n_items']
    NC = N + 1
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    ace = torch.randn(n, D, generator=g, device=dev)
    label = torch.randint(1, n, (P,), generator=g, device=dev)
    neg = torch.randint(1, n, (P, N), generator=g, device=dev)
    mask = torch.ones(P, dtype=torch.uint8, device=dev)
    probs = torch.softmax(torch.randn(P, NC, generator=g, device=dev) * 3.0, -1)
    nll = torch.ones(P, device=dev)
    sp, e = torch.empty(P, NC, device=dev), torch.empty(P, device=dev)
    w4 = torch.randn(32, generator=g, device=dev)
    ds = torch.zeros(P * NC, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def fwd():
        check(lib.cham_diversity_fwd(ptr(probs), ptr(label), ptr(neg), ptr(mask), P, N, ptr(ace), ace.stride(0), D, n, 0.5, ptr(sp), ptr(e),
                                     ptr(nll), st), "cham_diversity_fwd")
    out = dict(s)
    med, mn = timed(fwd, iters)
    row_bytes = P * NC * D * 4
    out.update(fwd_ms_median=med, fwd_ms_min=mn, fwd_row_bytes=row_bytes, fwd_row_gbps_one_read=row_bytes / (med * 1e-3) / 1e9,
               fwd_row_gbps_two_reads=2 * row_bytes / (med * 1e-3) / 1e9)
    # the same table with its row stride padded to whole 16-byte pieces (D = 250 -> 252): the float4 path instead of one column per lane
    ld4 = 4 * ((D + 3) // 4)
    pad = torch.zeros(n, ld4, device=dev)
    pad[:, :D] = ace

    def fwd_padded():
        check(lib.cham_diversity_fwd(ptr(probs), ptr(label), ptr(neg), ptr(mask), P, N, ptr(pad), ld4, D, n, 0.5, ptr(sp), ptr(e), ptr(nll), st),
              "cham_diversity_fwd")
    med, mn = timed(fwd_padded, iters)
    out.update(fwd_padded_ld=ld4, fwd_padded_ms_median=med, fwd_padded_ms_min=mn)
    for name, dt, fn in (('f32', torch.float32, lib.cham_diversity_bwd), ('b16', torch.bfloat16, lib.cham_diversity_bwd_b16)):
        S3 = torch.randn(P * NC, 32, generator=g, device=dev).to(dt)
        dS3 = torch.empty_like(S3)

        def bwd():
            check(fn(ptr(S3), 32, ptr(w4), ptr(probs), ptr(mask), P, N, 0.1, None, float(P), ptr(sp), ptr(e), 0.5, ptr(ds), ptr(dS3), st),
                  "cham_diversity_bwd")
        med, mn = timed(bwd, iters)
        nbytes = P * NC * (2 * 32 * S3.element_size() + 4 * 4)
        out.update({'bwd_%s_ms_median' % name: med, 'bwd_%s_ms_min' % name: mn, 'bwd_%s_bytes' % name: nbytes,
                    'bwd_%s_gbps' % name: nbytes / (med * 1e-3) / 1e9})
    return out


def bench_step(factor, iters, dev, B=256):
    """Eager train_step at the G1 model shape on full-length sessions (256 x 19 = 4 864 clicks) with a device-resident recent-clicks state."""
    from chameleon_recsys_amd.nar import synthetic
    from chameleon_recsys_amd.nar.clicked_items_state import DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    p = synthetic.default_params(46000, 250, seq_len=20, batch_size=B, neg=50, neg_from_buffer=3000, buffer_size=20000, for_norm=2000,
                                 C=1024, H=255, diversity_reg_factor=factor)
    rt = NARRuntime(p, seed=3)
    model = NARModuleModel(ModeKeys.TRAIN, None, None, p['session_features_config'], p['articles_features_config'], B, p['lr'], 1.0,
                           p['train_total_negative_samples'], p['train_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                           softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                           recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                           recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                           CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'], diversity_reg_factor=factor, runtime=rt)
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
    return dict(step_factor=factor, B=B, clicks=int(dev_b[0]['P']), step_ms_median=float(np.median(ms)), step_ms_min=float(np.min(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='g1,adressa')
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--step-iters', type=int, default=20, help='0: kernels only')
    ap.add_argument('--factor', type=float, default=0.5)
    ap.add_argument('--out', default=None, help='also append the JSON lines to DIR/bench_diversity.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_diversity.py needs a ROCm device")
    lib, dev = _lib.load(), torch.device('cuda:0')
    lines = []
    for name in args.shapes.split(','):
        lines.append(json.dumps(dict(shape=name, **bench_kernels(lib, SHAPES[name], dev, args.iters))))
        print(lines[-1], flush=True)
    if args.step_iters > 0:
        for factor in (0.0, args.factor, 0.0, args.factor):          # alternating: the spread between equal runs is part of the answer
            lines.append(json.dumps(bench_step(factor, args.step_iters, dev)))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_diversity.jsonl'), 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
