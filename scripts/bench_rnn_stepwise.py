#!/usr/bin/env python
"""Time of the recurrent stack alone, forward + backward of one layer, through the model's own launch paths (nar/recurrent.py): the
step-wise GRU (rnn_units above 384) and the step-wise LSTM (every width) next to the step-wise UGRNN and the fused GRU.  Full-length sessions; the x W_x projection and the
weight gradients are not part of it (they are the same GEMMs for every path).

  python scripts/bench_rnn_stepwise.py [--batch 256] [--seq 20] [--warmup 5] [--iters 20] [--rounds 3] [--out FILE]

Each case is warmed up, then timed with device events around one forward + backward, `iters` times per round; the rounds go through the
cases in turn, so that a drift of the machine touches all of them.  Reported per case: median / min / max over all timed iterations
(ms), launches per time step, and the same median at a batch of 32 sessions: where that is about the time at the full batch, the path
is bound by its launches and their latency, not by its arithmetic.  One JSON line per case, then a markdown table."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from chameleon_recsys_amd import _lib                     # noqa: E402
from chameleon_recsys_amd._lib import check, ptr         # noqa: E402
from chameleon_recsys_amd.nar import recurrent            # noqa: E402
from chameleon_recsys_amd.nar.layout import rnn_stepwise  # noqa: E402

CASES = [('gru', 512), ('gru', 1024), ('ugrnn', 640), ('ugrnn', 1024), ('gru', 384), ('lstm', 256), ('lstm', 512), ('lstm', 640), ('lstm', 1024)]


class Stack:
    """One recurrent layer as nar/recurrent.py sees it: the stub HOST of a launch path (lib, gemm, p) and its PLAN (the buffers, under
    StepPlan's names) in one object, driving the path class the model's own selection picks for the width."""

    def __init__(self, lib, cell, Hp, B, T, dev, seed=0):
        self.lib, self.cell, self.Hp, self.B, self.T, self.BT = lib, cell, Hp, B, T, B * T
        gru, four = cell == 'gru', cell in ('gru', 'lstm')
        ng = {'ugrnn': 2, 'gru': 3, 'lstm': 4}[cell]
        nh = 4 if cell == 'lstm' else 2      # column blocks of W_h
        L = types.SimpleNamespace(cell=cell, Hp=Hp, NG=ng, rnn_stepwise=rnn_stepwise(cell, Hp))
        g = torch.Generator(device=dev)
        g.manual_seed(seed + Hp)
        rnd = lambda *s: torch.randn(*s, generator=g, device=dev, dtype=torch.float32)
        f32 = lambda *s: torch.zeros(*s, device=dev, dtype=torch.float32)
        # W_gh [Hp, 2Hp] directly followed by W_ch [Hp, Hp], as the flat parameter buffer holds them (LSTM: one W_h [Hp, 4Hp])
        W = rnd(Hp * ng * Hp) * Hp ** -0.5
        self.weights = {'rnn0/Wh': W[:nh * Hp * Hp].view(Hp, nh * Hp), 'rnn0/Wch': W[2 * Hp * Hp:].view(Hp, Hp) if gru else None}
        self.p = self.weights.__getitem__
        self.xproj, self.drnn = [0.7 * rnd(B * T, ng * Hp)], rnd(B * T, Hp)
        self.seq_len = torch.full((B,), T, dtype=torch.int32, device=dev)
        self.rnn_out, self.hprev, self.G, self.Cc = ([f32(B * T, Hp)] for _ in range(4))
        self.R, self.RH = ([f32(B * T, Hp) if four else None] for _ in range(2))
        self.dxproj = f32(B * T, ng * Hp)
        # (PC 0: a step without candidate rows - never the cooperative path, which is not a case here)
        self.path = recurrent.path_class(L, 0, B, recurrent.default_coop_rows(L))(self, L)
        self.path.alloc(self, f32)
        self.step, self.launches = L.rnn_stepwise, self.path.launches_per_step or (0, 0)

    def gemm(self, A, Bm, C, M, N, K, lda, ldb, ldc, transB=0, accumulate=0, force_f32=True):
        check(self.lib.cham_gemm_f32(ptr(A), lda, 0, ptr(Bm), ldb, transB, ptr(C), ldc, M, N, K, None, 0, None, 0, 0, None, 0, 1, accumulate,
                                     None, 0, 1, torch.cuda.current_stream().cuda_stream), "cham_gemm_f32")

    def timed(self, iters):
        """Device-event times (ms) of `iters` forward + backward passes."""
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
        for a, b in ev:
            a.record()
            st = torch.cuda.current_stream().cuda_stream
            self.path.forward(self, 0, st); self.path.backward(self, 0, st)
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--seq', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--small_batch', type=int, default=32)
    ap.add_argument('--out', default=None, help="also write the JSON lines and the table to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rnn_stepwise.py needs a ROCm device: a time taken elsewhere says nothing")
    dev = torch.device('cuda:0')
    lib = _lib.load()
    stacks = {(c, Hp, B): Stack(lib, c, Hp, B, a.seq, dev) for c, Hp in CASES for B in (a.batch, a.small_batch)}
    for s in stacks.values():
        s.timed(a.warmup)
        assert torch.isfinite(s.dxproj).all() and torch.isfinite(s.rnn_out[0]).all() and float(s.dxproj.abs().max()) > 0
    times = {k: [] for k in stacks}
    for _ in range(a.rounds):
        for k, s in stacks.items():
            times[k] += s.timed(a.iters)
    lines, rows = [], []
    for c, Hp in CASES:
        t, ts = np.asarray(times[(c, Hp, a.batch)]), np.asarray(times[(c, Hp, a.small_batch)])
        s = stacks[(c, Hp, a.batch)]
        rec = dict(cell=c, Hp=Hp, path='step-wise' if s.step else 'fused', B=a.batch, T=a.seq, n=len(t), median_ms=round(float(np.median(t)), 4),
                   min_ms=round(float(t.min()), 4), max_ms=round(float(t.max()), 4), launches_per_step_fwd=s.launches[0],
                   launches_per_step_bwd=s.launches[1], small_B=a.small_batch, small_B_median_ms=round(float(np.median(ts)), 4))
        if s.step:
            rec['us_per_launch'] = round(1e3 * rec['median_ms'] / (a.seq * sum(s.launches)), 2)
        lines.append(json.dumps(rec))
        rows.append(rec)
    table = ["| cell | Hp | path | launches / step (fwd + bwd) | median ms | min | max | median ms at B %d |" % a.small_batch,
             "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        table.append("| %s | %d | %s | %s | %.3f | %.3f | %.3f | %.3f |" % (
            r['cell'], r['Hp'], r['path'], ("%d + %d" % (r['launches_per_step_fwd'], r['launches_per_step_bwd'])) if r['path'] == 'step-wise' else '-',
            r['median_ms'], r['min_ms'], r['max_ms'], r['small_B_median_ms']))
    text = "\n".join(lines + [""] + table + ["", "device: %s; B %d, T %d, %d warm-up + %d x %d timed passes per case" % (
        torch.cuda.get_device_name(0), a.batch, a.seq, a.warmup, a.rounds, a.iters)])
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
