"""The split-K summation order of the register-staged GEMM families (csrc/gemm.hip, gemm_x3.hip, gemm_b16.hip), pinned against the
partial slabs themselves.  After a TN split-K call the workspace still holds `splits` dense [M, N] fp32 slabs (slab s = the product over
the s-th K chunk); the reduction kernel adds them in a documented, fixed order:

  plain  the slabs in ascending order, starting from 0
  wide   (M N / 4 <= the family's threshold and >= 32 splits) 16 running sums, sum g = 0 + slab g + slab g+16 + slab g+32 ... in ascending
         order; then sum 0 + sum 1 + ... + sum 15 in ascending g
  accumulate = 1: the old C is added last

The test reads the slabs back, adds them on the CPU in float32 (numpy: adds only, nothing to contract) in that order and asks for the
device's C bit for bit.  The wide threshold is 32768 for cham_gemm_f32 / _bf16 / _f32x3 and 65536 for cham_gemm_b16."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

WS_FLOATS = 32 * 1032 * 256          # the largest case: 32 slabs of [1032, 256]


def _counts(lib, name, n):
    out = (ctypes.c_longlong * n)()
    getattr(lib, name)(out, 0)
    return list(out)


def _expected(slabs, wide, old):
    """slabs [splits, M, N] float32 -> the documented sum, float32 adds only."""
    zero = np.zeros(slabs.shape[1:], dtype=np.float32)
    if wide:
        sums = []
        for g in range(16):
            v = zero.copy()
            for s in range(g, slabs.shape[0], 16):
                v = v + slabs[s]
            sums.append(v)
        v = sums[0]
        for g in range(1, 16):
            v = v + sums[g]
    else:
        v = zero.copy()
        for s in range(slabs.shape[0]):
            v = v + slabs[s]
    if old is not None:
        v = v + old
    assert v.dtype == np.float32
    return v


def _case(gpu, entry, M, N, K, hint, splits, wide, accumulate):
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    g = torch.Generator().manual_seed(1000 * M + N + hint)
    # asymmetric data: every slab, row and column differs, the magnitudes spread over a few binades so that the order of the adds shows
    A = torch.randn(K, M, generator=g) * (1.0 + torch.arange(M, dtype=torch.float32) / M)
    B = torch.randn(K, N, generator=g) * (0.5 + torch.arange(K, dtype=torch.float32)[:, None] / K)
    C0 = torch.randn(M, N, generator=g) * 50.0
    ws = torch.full((WS_FLOATS,), float('nan'), device=gpu)
    dC = C0.to(gpu)
    st = torch.cuda.current_stream().cuda_stream
    if entry == 'cham_gemm_b16':
        dA, dB = A.bfloat16().to(gpu), B.bfloat16().to(gpu)
        rc = lib.cham_gemm_b16(ptr(dA), M, 1, ptr(dB), N, 0, ptr(dC), N, 1, M, N, K, None, 0, None, 0, 0, accumulate, ptr(ws), WS_FLOATS * 4, hint, st)
        got_splits = _counts(lib, 'cham_gemm_b16_launch_counts', 8)[7]
    else:
        dA, dB = A.to(gpu), B.to(gpu)
        rc = getattr(lib, entry)(ptr(dA), M, 1, ptr(dB), N, 0, ptr(dC), N, M, N, K, None, 0, None, 0, 0, None, 0, 1, accumulate, ptr(ws),
                                 WS_FLOATS * 4, hint, st)
        if entry == 'cham_gemm_f32x3':
            got_splits = _counts(lib, 'cham_gemm_f32x3_launch_counts', 8)[7]
        else:
            got_splits = _counts(lib, 'cham_gemm_launch_counts', 16)[15]
    check(rc, entry)
    torch.cuda.synchronize()
    assert got_splits == splits, (entry, M, N, K, hint, got_splits)          # no silent fall-back to one split
    slabs = ws[:splits * M * N].cpu().numpy().reshape(splits, M, N)
    assert np.isfinite(slabs).all()                                           # every slab element was written
    assert np.isnan(ws[splits * M * N:splits * M * N + 4].cpu().numpy()).all()     # ... and there are no more slabs than `splits`
    want = _expected(slabs, wide, C0.numpy() if accumulate else None)
    assert torch.equal(dC.cpu(), torch.from_numpy(want)), (entry, M, N, K, hint, accumulate,
                                                            float(np.abs(dC.cpu().numpy() - want).max()))
    if splits > 16:          # the two documented orders really differ on this data: the case tells them apart (up to 16 splits they coincide)
        other = _expected(slabs, not wide, C0.numpy() if accumulate else None)
        assert not np.array_equal(other, want)


TILE_ENTRIES = ['cham_gemm_f32', 'cham_gemm_bf16', 'cham_gemm_f32x3']


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("entry", TILE_ENTRIES)
@pytest.mark.parametrize("M,N,K,hint,splits,wide", [
    (256, 128, 8192, 32, 32, True),            # n4 = 8192
    (256, 128, 8192, 5, 5, False),             # too few splits for the wide form
    (1028, 128, 8192, 32, 32, False),          # n4 = 32896, just over 32768
])
def test_tile_families(gpu, entry, M, N, K, hint, splits, wide, accumulate):
    _case(gpu, entry, M, N, K, hint, splits, wide, accumulate)


@pytest.mark.parametrize("accumulate", [0, 1])
def test_small_output_tn_kernel(gpu, accumulate):
    """M <= 128: cham_gemm_f32 runs gemm_tn_small_kernel ([5] of its launch counters), the same slabs and reduction."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    before = _counts(lib, 'cham_gemm_launch_counts', 16)[5]
    _case(gpu, 'cham_gemm_f32', 128, 64, 8192, 32, 32, True, accumulate)     # n4 = 2048
    assert _counts(lib, 'cham_gemm_launch_counts', 16)[5] == before + 1


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("M,N,K,hint,splits,wide", [
    (1024, 128, 16384, 32, 32, True),          # n4 = 32768
    (1024, 256, 16384, 32, 32, True),          # n4 = 65536: wide only under cham_gemm_b16's 65536 threshold
    (1032, 256, 16384, 32, 32, False),         # n4 = 66048
    (1024, 256, 16384, 5, 5, False),
])
def test_b16(gpu, M, N, K, hint, splits, wide, accumulate):
    _case(gpu, 'cham_gemm_b16', M, N, K, hint, splits, wide, accumulate)
