"""What the GPU tests of the feature front end and of the PreCAR combine share (tests/test_feature_frontend_gpu.py,
tests/test_combine_gpu.py, tests/test_features_gpu.py): guarded outputs, the launch-twice rule, the printed error ratio."""
import numpy as np
import torch

from tests import features_reference as F


def _lib_():
    from chameleon_recsys_amd import _lib
    return _lib.load()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(gpu, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _note(name, err, k):
    print("    %-26s %.2e  = %.2f x the fp32-CPU error (bound 8 x = %.2e)" % (name, err, err / (k / 8.0), k))
    assert err <= k, (name, err, k)


class Out:
    """An output of `shape` in the middle of a flat allocation: max(64, one row) elements of fill (rounded up to 16 bytes' worth) on
    either side, the output itself filled too - NaN for floats, -7 for integers (249 for bytes)."""

    def __init__(self, gpu, shape, dtype=torch.float32, init=None):
        n = int(np.prod(shape))
        row = int(shape[-1]) if len(shape) else 1
        self.pad = (max(64, row + 1) + 7) // 8 * 8
        self.fp = dtype.is_floating_point
        self.fill = float('nan') if self.fp else (249 if dtype == torch.uint8 else -7)
        self.buf = torch.full((n + 2 * self.pad,), self.fill, dtype=dtype, device=gpu)
        self.t = self.buf[self.pad:self.pad + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self, offset=0):
        return self.buf.data_ptr() + (self.pad + offset) * self.buf.element_size()

    def _is_fill(self, x):
        return bool(torch.isnan(x.float()).all()) if self.fp else bool((x == self.fill).all())

    def untouched(self):
        return self._is_fill(self.buf)

    def numpy(self):
        torch.cuda.synchronize()
        assert self._is_fill(self.buf[:self.pad]) and self._is_fill(self.buf[self.buf.numel() - self.pad:]), "a kernel wrote outside its output"
        t = self.t
        if t.dtype == torch.bfloat16:
            return t.view(torch.int16).cpu().numpy().view(np.uint16)
        return t.cpu().numpy()


def _twice(run):
    """run() -> tuple of numpy arrays; made twice, bit-identical."""
    a, b = run(), run()
    for x, y in zip(a, b):
        assert F.same_bits(x, y), "two launches differ"
    return a
