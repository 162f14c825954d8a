#!/usr/bin/env python
"""Cost of the ACR module (csrc/acr.hip, chameleon_recsys_amd/acr) at the G1 shape: B 64 articles x L 300 tokens, E 300, filter sizes
3/4/5, F 128, vocabulary 45 000, acr_embeddings_size 250, one head of 461 classes.

  python scripts/bench_acr.py [--iters 30] [--rounds 3] [--articles 1024] [--legs conv,step,multilabel,pipeline] [--out DIR]

One JSON line per leg, device events around each call, every shape warmed up first:
  conv_fwd   cham_acr_conv_pool_fwd (both launches) beside torch conv1d + relu + amax in fp32 on the same inputs - what a user would
             run without the kernel - ALTERNATING, `rounds` times; FLOPs = 2 B F E sum_k k (L-k+1) = 17.7 G, share of the 157.3 TFLOP/s
             fp32-matrix peak; the two results are compared at the timed size
  conv_bwd   cham_acr_conv_pool_bwd
  step       ACR_Model.train_step (upload, forward, loss, backward, Adam) on resident numpy batches
  multilabel cham_acr_sigmoid_xent alone (B 64, K 20, C 1 000 and 6 500) and the Adressa-shaped train_step (L 300, E 300, sizes 3/4/5,
             F 128, embedding 250, category0 of 41 classes) with and without the keywords head of 6 500 classes
  pipeline   articles/s through prepare_dataset -> train_step on a synthetic corpus of --articles articles of ~300 tokens, and of
             prepare_dataset alone (the record decoder is host-side Python)"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chameleon_recsys_amd import _lib                     # noqa: E402
from chameleon_recsys_amd._lib import check, ptr         # noqa: E402

G1 = dict(B=64, L=300, E=300, F=128, sizes=(3, 4, 5), V=45000, A=250, C=461)
PEAK_F32_MATRIX = 157.3e12


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


def conv_flops(s):
    return 2.0 * s['B'] * s['F'] * s['E'] * sum(k * (s['L'] - k + 1) for k in s['sizes'])


def bench_conv(lib, s, dev, iters, rounds):
    B, L, E, F, V, sizes = s['B'], s['L'], s['E'], s['F'], s['V'], s['sizes']
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    n, PW = len(sizes), len(sizes) * F
    table = 0.5 * torch.randn(V, E, generator=g, device=dev)
    tok = torch.randint(0, V, (B, L), generator=g, device=dev, dtype=torch.int32)
    W = [torch.randn(k, E, F, generator=g, device=dev) / (k * E) ** 0.5 for k in sizes]
    bias = [torch.rand(F, generator=g, device=dev) for _ in sizes]
    c_sizes = (ctypes.c_int * n)(*sizes)
    arr = ctypes.c_void_p * n
    pW, pb = arr(*[w.data_ptr() for w in W]), arr(*[b.data_ptr() for b in bias])
    pool, argmax = torch.zeros(B, PW, device=dev), torch.zeros(B, PW, dtype=torch.int32, device=dev)
    ws = torch.empty(lib.cham_acr_conv_pool_workspace_bytes(B, L, c_sizes, n, F) // 4 + 1, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def ours():
        check(lib.cham_acr_conv_pool_fwd(ptr(tok), B, L, ptr(table), V, E, E, c_sizes, n, F, pW, pb, ptr(pool), PW, ptr(argmax), ptr(ws),
                                         ws.numel() * 4, st), "cham_acr_conv_pool_fwd")

    Wt = [w.permute(2, 1, 0).contiguous() for w in W]          # conv1d wants [F, E, k]
    tok64 = tok.long()

    def eager():
        x = table[tok64].transpose(1, 2)                        # [B, E, L]: the gather is part of what the kernel replaces
        return torch.cat([torch.relu(torch.nn.functional.conv1d(x, w, b)).amax(dim=2) for w, b in zip(Wt, bias)], dim=1)

    ours()
    ref = eager()
    torch.cuda.synchronize()
    diff = float((pool - ref).abs().max())
    out = dict(leg='conv_fwd', **{k: v for k, v in s.items() if k != 'sizes'}, sizes=list(sizes), gflop=conv_flops(s) / 1e9,
               max_abs_diff_vs_torch=diff, rounds=[])
    for _ in range(rounds):
        a, b = timed(ours, iters), timed(eager, iters)
        out['rounds'].append(dict(ours_ms_median=a[0], ours_ms_min=a[1], torch_ms_median=b[0], torch_ms_min=b[1]))
    med = float(np.median([r['ours_ms_median'] for r in out['rounds']]))
    out.update(ours_ms=med, torch_ms=float(np.median([r['torch_ms_median'] for r in out['rounds']])),
               ours_tflops=conv_flops(s) / (med * 1e-3) / 1e12, share_of_f32_matrix_peak=conv_flops(s) / (med * 1e-3) / PEAK_F32_MATRIX)
    print(json.dumps(out), flush=True)

    dpool = torch.randn(B, PW, generator=g, device=dev)
    dW = [torch.empty_like(w) for w in W]
    db = [torch.empty_like(b) for b in bias]
    pdW, pdb = arr(*[w.data_ptr() for w in dW]), arr(*[b.data_ptr() for b in db])

    def bwd():
        check(lib.cham_acr_conv_pool_bwd(ptr(tok), B, L, ptr(table), V, E, E, c_sizes, n, F, ptr(dpool), ptr(pool), PW, ptr(argmax), pdW, pdb, st),
              "cham_acr_conv_pool_bwd")
    med, mn = timed(bwd, iters)
    out2 = dict(leg='conv_bwd', ms_median=med, ms_min=mn)
    print(json.dumps(out2), flush=True)
    return [out, out2]


def bench_step(s, dev, iters):
    from chameleon_recsys_amd.acr.acr_model import ACR_Model
    rng = np.random.RandomState(0)
    table = (0.5 * rng.randn(s['V'], s['E'])).astype(np.float32)
    heads = {'category_id': {'classification_type': 'multiclass', 'cardinality': s['C']}}
    params = dict(word_embeddings_matrix=table, cnn_filter_sizes=','.join(map(str, s['sizes'])), cnn_num_filters=s['F'],
                  acr_embeddings_size=s['A'], dropout_keep_prob=1.0, l2_reg_lambda=1e-3, learning_rate=1e-3)
    model = ACR_Model('metadata_classification', 'CNN', heads, params, device=dev)
    batches = [({'text': rng.randint(0, s['V'], size=(s['B'], s['L']))}, {'category_id': rng.randint(0, s['C'], size=s['B'])}) for _ in range(4)]
    i = [0]

    def step():
        f, l = batches[i[0] % 4]; i[0] += 1
        model.train_step(f, l)
    med, mn = timed(step, iters)
    out = dict(leg='step', ms_median=med, ms_min=mn, articles_per_s=s['B'] / (med * 1e-3), last_loss=float(model.loss.cpu()[0]))
    print(json.dumps(out), flush=True)
    return [out]


ADRESSA = dict(B=64, L=300, E=300, F=128, sizes=(3, 4, 5), V=45000, A=250, C0=41, CK=6500, K=20)


def bench_multilabel(lib, s, dev, iters):
    """The multilabel head: cham_acr_sigmoid_xent alone at B 64, K 20 and C in {1 000, 6 500} (with dlogits), and the Adressa-shaped
    train_step (category0 of 41 classes) with and without the keywords head of 6 500 classes."""
    from chameleon_recsys_amd.acr.acr_model import ACR_ModelMultilabel
    B, K = s['B'], s['K']
    g = torch.Generator(device=dev)
    g.manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    lines = []
    for C in (1000, s['CK']):
        ld = (C + 3) // 4 * 4
        logits = 3.0 * torch.randn(B, ld, generator=g, device=dev)
        ids = torch.randint(1, C, (B, K), generator=g, device=dev, dtype=torch.int32)
        loss, dl = torch.zeros(1, device=dev), torch.zeros(B, ld, device=dev)
        pred, counts = torch.zeros(B, ld, dtype=torch.uint8, device=dev), torch.zeros(3, dtype=torch.int32, device=dev)
        ws = torch.zeros(lib.cham_acr_sigmoid_xent_workspace_bytes(B, C) // 4, device=dev)

        def head():
            check(lib.cham_acr_sigmoid_xent(ptr(logits), ld, B, C, ptr(ids), K, K, ptr(loss), ptr(dl), ptr(pred), ld, ptr(counts), ptr(ws),
                                            ws.numel() * 4, st), "cham_acr_sigmoid_xent")
        med, mn = timed(head, iters)
        lines.append(dict(leg='sigmoid_xent', B=B, K=K, C=C, ms_median=med, ms_min=mn, bytes_moved=B * ld * 9, loss=float(loss.cpu()[0])))
        print(json.dumps(lines[-1]), flush=True)
    rng = np.random.RandomState(0)
    table = (0.5 * rng.randn(s['V'], s['E'])).astype(np.float32)
    params = dict(word_embeddings_matrix=table, cnn_filter_sizes=','.join(map(str, s['sizes'])), cnn_num_filters=s['F'],
                  acr_embeddings_size=s['A'], dropout_keep_prob=1.0, l2_reg_lambda=1e-3, learning_rate=1e-3)
    for with_keywords in (False, True):
        heads = {'category0': {'classification_type': 'multiclass', 'cardinality': s['C0']}}
        if with_keywords:
            heads['keywords'] = {'classification_type': 'multilabel', 'cardinality': s['CK']}
        model = ACR_ModelMultilabel('metadata_classification', 'CNN', heads, params, device=dev)
        batches = [({'text': rng.randint(0, s['V'], size=(B, s['L']))},
                    {'category0': rng.randint(0, s['C0'], size=B), 'keywords': rng.randint(1, s['CK'], size=(B, K))}) for _ in range(4)]
        i = [0]

        def step():
            f, l = batches[i[0] % 4]; i[0] += 1
            model.train_step(f, l)
        med, mn = timed(step, iters)
        lines.append(dict(leg='step_adressa', keywords_head=with_keywords, ms_median=med, ms_min=mn, articles_per_s=B / (med * 1e-3),
                          last_loss=float(model.loss.cpu()[0])))
        print(json.dumps(lines[-1]), flush=True)
    return lines


def bench_pipeline(s, dev, n_articles):
    from chameleon_recsys_amd.acr import acr_datasets, acr_trainer_gcom, synthetic
    with tempfile.TemporaryDirectory() as d:
        c = synthetic.make_corpus(d, n_articles=n_articles, n_categories=s['C'], vocab_size=s['V'], embedding_size=s['E'], articles_by_file=256,
                                  min_len=250, max_len=330, long_len=340, seed=0)
        cfg = c['features_config']
        ds = lambda: acr_datasets.prepare_dataset(c['files'], cfg, s['B'], 1, True, 5000, s['L'])
        t0 = time.time()
        n_read = sum(len(f['article_id']) for f, _ in ds())
        t_read = time.time() - t0
        est = acr_trainer_gcom.build_acr_estimator(None, c['word_embeddings_matrix'], cfg, None, device=dev)
        est.train(ds, steps=2)                                  # warm-up: model creation, code objects
        torch.cuda.synchronize()
        t0 = time.time()
        est.train(ds)
        torch.cuda.synchronize()
        t_train = time.time() - t0
    out = dict(leg='pipeline', articles=n_read, reader_alone_articles_per_s=n_read / t_read, reader_and_train_articles_per_s=n_read / t_train)
    print(json.dumps(out), flush=True)
    return [out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--articles', type=int, default=1024, help='0: no pipeline leg')
    ap.add_argument('--legs', default='conv,step,multilabel,pipeline', help='comma-separated subset of conv,step,multilabel,pipeline')
    ap.add_argument('--out', default=None, help='also append the JSON lines to DIR/bench_acr.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_acr.py needs a ROCm device")
    lib, dev = _lib.load(), torch.device('cuda:0')
    legs, lines = args.legs.split(','), []
    if 'conv' in legs:
        lines += bench_conv(lib, G1, dev, args.iters, args.rounds)
    if 'step' in legs:
        lines += bench_step(G1, dev, args.iters)
    if 'multilabel' in legs:
        lines += bench_multilabel(lib, ADRESSA, dev, args.iters)
    if 'pipeline' in legs and args.articles > 0:
        lines += bench_pipeline(G1, dev, args.articles)
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_acr.jsonl'), 'a') as fh:
            fh.write('\n'.join(json.dumps(x) for x in lines) + '\n')


if __name__ == '__main__':
    main()
