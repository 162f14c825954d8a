"""The recording host of the driver-module tests (test_recurrent_cpu.py, test_lstm_recurrent_cpu.py, test_input_rows_cpu.py): a library, a gemm and
a colsum whose every call lands in ONE log, over small CPU tensors."""
import types

import torch

from chameleon_recsys_amd import _lib

S = 7          # the stream handle the driver passes


class Recorder:
    """Host of a path (lib, gemm, p, g, colsum) whose every call lands in ONE log; pointers are logged as the name of the buffer they
    point into (+ the element offset, if any)."""

    def __init__(self, L, layers=1):
        self.log, self.names = [], {}
        Hp, NG = L.Hp, L.NG
        self.weights, self.grads = {}, {}
        for l in range(layers):
            for d, tag in ((self.weights, ''), (self.grads, 'd')):
                d['rnn%d/Wh' % l] = self.name(torch.zeros(Hp, 2 * Hp), '%sWh%d' % (tag, l))
                d['rnn%d/b' % l] = self.name(torch.zeros(NG * Hp), '%sb%d' % (tag, l))
                if L.cell == 'gru':
                    d['rnn%d/Wch' % l] = self.name(torch.zeros(Hp, Hp), '%sWch%d' % (tag, l))
        self.p, self.g = self.weights.__getitem__, self.grads.__getitem__
        self.lib = types.SimpleNamespace()
        for fn, sig in _lib._SIGNATURES.items():
            setattr(self.lib, fn, self._entry(fn, [a.__name__ == 'c_void_p' for a in sig[1]]))

    def name(self, t, name):
        self.names[name] = t
        return t

    def tag(self, a):
        if a is None or a == 0:
            return None
        if a == S:
            return 'stream'
        for name, t in self.names.items():
            if t.numel() and t.data_ptr() <= a < t.data_ptr() + t.numel() * t.element_size():
                off = (a - t.data_ptr()) // t.element_size()
                return name if off == 0 else '%s+%d' % (name, off)
        raise AssertionError("pointer into no buffer of the plan")

    def _entry(self, fn, is_ptr):
        def call(*args):
            assert len(args) == len(is_ptr), fn
            self.log.append((fn,) + tuple(self.tag(a) if p else a for a, p in zip(args, is_ptr)))
            return 0
        return call

    def gemm(self, A, Bm, C, M, N, K, lda, ldb, ldc, **kw):
        self.log.append(('gemm', self.tag(A.data_ptr()), self.tag(Bm.data_ptr()), self.tag(C.data_ptr()), M, N, K, lda, ldb, ldc, self.kw(kw)))

    def colsum(self, X, ld, R, F, out, **kw):
        self.log.append(('colsum', self.tag(X.data_ptr()), ld, R, F, self.tag(out.data_ptr()), self.kw(kw)))

    def kw(self, kw):          # tensor keyword arguments (bias=, dref=, ...) by the name of their buffer, like the positional ones
        return {k: self.tag(v.data_ptr()) if torch.is_tensor(v) else v for k, v in kw.items()}
