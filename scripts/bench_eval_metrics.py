#!/usr/bin/env python
"""Per-eval-batch cost of the beyond-accuracy metrics: the device chain (cham_eval_beyond_accuracy + cham_eval_coverage_count, then
the two reads the hook makes: per-click values and the two counts) against the vectorised host classes of nar/metrics.py on the
same data (ItemCoverage, ESI-R, ESI-RR, EILD-R, EILD-RR fed through evaluation.update_metrics; the host path also needs
articles_recent_pop_norm on the host, whose download is timed separately).

  python scripts/bench_eval_metrics.py [--shapes g1,cfg5] [--iters 20] [--out DIR]

Shapes: g1 = B 256, T 20, NC 51, D 250, topn 10, 46 000 articles (bench.py's G1 catalogue); cfg5 = B 4096, T 19, NC 201, D 128,
topn 10, 5 M articles.  About 35 % of the positions are valid clicks (G1-like session lengths).  One JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chameleon_recsys_amd import _lib                     # noqa: E402
from chameleon_recsys_amd._lib import check, ptr         # noqa: E402
from chameleon_recsys_amd.nar import evaluation, metrics  # noqa: E402

SHAPES = {'g1': dict(B=256, T=20, NC=51, D=250, topn=10, n_items=46_000),
          'cfg5': dict(B=4096, T=19, NC=201, D=128, topn=10, n_items=5_000_000)}
REL_NEG = 0.1


def make_data(s, dev, seed=0):
    rng = np.random.default_rng(seed)
    B, T, NC, n = s['B'], s['T'], s['NC'], s['n_items']
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    ace_d = torch.randn(n, s['D'], generator=g, device=dev, dtype=torch.float32)
    pop_d = torch.rand(n, generator=g, device=dev, dtype=torch.float32).clamp_(min=1e-4)
    lengths = np.minimum(rng.geometric(1.0 / (0.35 * T), size=B), T)
    valid = np.arange(T)[None, :] < lengths[:, None]
    preds = rng.integers(1, n, size=(B, T, NC), dtype=np.int64)
    labels = np.where(valid, np.where(rng.random((B, T)) < 0.3, preds[..., 0], rng.integers(1, n, size=(B, T))), 0).astype(np.int64)
    clicked = np.where(valid, rng.integers(1, n, size=(B, T)), 0).astype(np.int64)
    buffer = rng.integers(0, n, size=20_000, dtype=np.int64)
    return ace_d, pop_d, preds, labels, clicked, buffer


def bench_device(lib, s, dev, ace_d, pop_d, preds, labels, clicked, buffer, iters):
    B, T, NC, n = s['B'], s['T'], s['NC'], s['n_items']
    p, lab, clk = (torch.from_numpy(a).to(dev) for a in (preds, labels, clicked))
    buf = torch.from_numpy(buffer).to(dev)
    rec_map = torch.empty(n, dtype=torch.uint8, device=dev)
    clk_map = torch.empty(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(lib.cham_eval_coverage_workspace_bytes(n), dtype=torch.uint8, device=dev)
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    per_click = torch.empty(B * T, 4, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    check(lib.cham_eval_coverage_seed(ptr(buf), buf.numel(), n, ptr(rec_map), ptr(clk_map), stream), "seed")

    def chain():
        check(lib.cham_eval_beyond_accuracy(ptr(p), NC, ptr(lab), ptr(clk), B * T, ptr(ace_d), s['D'], n, ptr(pop_d), s['topn'], 1.0,
                                            REL_NEG, ptr(per_click), ptr(rec_map), ptr(clk_map), stream), "eval")
        check(lib.cham_eval_coverage_count(ptr(rec_map), ptr(clk_map), n, ptr(ws), ws.numel(), ptr(counts), stream), "count")

    for _ in range(3):
        chain()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(iters):                      # kernels only: device events around the two launches
        e0.record(); chain(); e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    wall = []
    for _ in range(iters):                      # what the hook pays per batch: launches + the two device-to-host reads
        t0 = time.perf_counter()
        chain()
        pc, cn = per_click.cpu().numpy(), counts.cpu().tolist()
        wall.append((time.perf_counter() - t0) * 1e3)
    return dict(kernel_ms_mean=float(np.mean(ms)), kernel_ms_min=float(np.min(ms)), with_reads_ms_mean=float(np.mean(wall)),
                with_reads_ms_min=float(np.min(wall))), pc.reshape(B, T, 4), tuple(cn)


def bench_host(s, ace_h, pop_d, preds, labels, clicked, buffer, iters):
    topn = s['topn']
    t0 = time.perf_counter()
    for _ in range(iters):
        pop = pop_d.cpu().numpy()
    pop_ms = (time.perf_counter() - t0) * 1e3 / iters
    pop64 = pop.astype(np.float64)
    times = []
    for _ in range(iters):
        ms = [metrics.ItemCoverage(topn, buffer), metrics.ExpectedRankSensitiveNovelty(topn),
              metrics.ExpectedRankRelevanceSensitiveNovelty(topn, 1.0, REL_NEG),
              metrics.ContentExpectedRankRelativeSensitiveIntraListDiversity(topn, ace_h),
              metrics.ContentExpectedRankRelativeRelevanceSensitiveIntraListDiversity(topn, ace_h, 1.0, REL_NEG)]
        t0 = time.perf_counter()
        evaluation.update_metrics(preds, labels, None, pop64[preds[..., :topn]], clicked, ms)
        ms[0].result()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(host_ms_mean=float(np.mean(times)), host_ms_min=float(np.min(times)), pop_download_ms=pop_ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='g1,cfg5')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--out', default=None, help='also append the JSON lines to DIR/bench_eval_metrics.jsonl')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval_metrics.py needs a ROCm device")
    lib, dev = _lib.load(), torch.device('cuda:0')
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    lines = []
    for name in args.shapes.split(','):
        s = SHAPES[name]
        ace_d, pop_d, preds, labels, clicked, buffer = make_data(s, dev)
        valid = int((labels != 0).sum())
        n = min(s['topn'], s['NC'])
        dres, pc, counts = bench_device(lib, s, dev, ace_d, pop_d, preds, labels, clicked, buffer, args.iters)
        ace_h = ace_d.cpu().numpy()
        hres, ms = bench_host(s, ace_h, pop_d, preds, labels, clicked, buffer, args.host_iters)
        # the two paths agree on this data
        host_vals = np.stack([np.array(m.results) for m in ms[1:]], -1)
        agree = bool(np.allclose(pc[labels != 0], host_vals, rtol=2e-5, atol=1e-6))
        cov_ok = counts == (len(ms[0].recommended_items), len(ms[0].clicked_items))
        out = dict(shape=name, **s, valid_clicks=valid, row_bytes_read=valid * n * s['D'] * 4, **dres, **hres,
                   speedup_vs_host=hres['host_ms_mean'] / dres['with_reads_ms_mean'], values_agree=agree, coverage_counts_agree=cov_ok)
        line = json.dumps(out)
        print(line, flush=True)
        lines.append(line)
        del ace_d, pop_d, ace_h
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, 'bench_eval_metrics.jsonl'), 'a') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
