"""PreCAR combine (csrc/scorer.hip).  Backward (cham_combine_bwd, cham_combine_bwd_b16): dU / dV against a float64 index_add reference.
Forward (cham_combine_fwd: the row-per-workgroup kernel and the per-position kernel of the candidate rows; cham_combine_fwd_b16): bit-exact
against tests/features_reference.combine_fwd evaluated in fp32 - one addition and one multiplication per element leave nothing to contract.

Covers what the step-parity tests reach only by luck: hot pool slots referenced by (almost) every position (split over position
chunks), cold slots, the zero-padding slot held MANY times per click (fewer than N unique candidates: first batches, small
catalogs - nar_model.py:1252 zero-pads; the round-1 kernel truncated its match list there), masked clicks (slot -1),
and bit-reproducibility (no float atomics: two runs are bit-identical)."""
import numpy as np
import pytest
import torch

from tests import features_reference as F
from tests.features_gpu_helpers import Out, _dev, _st, _twice

pytestmark = pytest.mark.gpu


def _make_slots(rng, BT, N, pmax, pad_frac, hot, masked_frac):
    """[BT, N] int32: per position N DISTINCT pool slots (popularity-skewed; slots < hot sit in every position), then a tail of
    ~pad_frac * N entries replaced by the zero-padding slot pmax; masked_frac of the positions are all -1."""
    slot = np.empty((BT, N), np.int32)
    w = 1.0 / np.arange(1, pmax + 1) ** 1.1
    w /= w.sum()
    for p in range(BT):
        s = rng.choice(pmax, size=N, replace=False, p=w)
        rest = s[~np.isin(s, np.arange(hot))]
        s = np.concatenate([np.arange(hot), rest])[:N].astype(np.int32)
        rng.shuffle(s)
        npad = int(round(pad_frac * N * rng.uniform(0.5, 1.5))) if pad_frac > 0 else 0
        if npad:
            s[N - min(npad, N):] = pmax
        slot[p] = s
    masked = rng.random(BT) < masked_frac
    slot[masked] = -1
    return slot, masked


@pytest.mark.parametrize("BT,N,pmax,C,pad_frac,hot,masked_frac", [
    (700, 50, 1000, 256, 0.0, 3, 0.0),          # hot slots in all 700 positions (> 512: chunked partials), no padding
    (1300, 50, 1000, 128, 0.3, 2, 0.1),         # 30 % zero-padded negatives, masked clicks, 3 position chunks
    (90, 9, 180, 128, 0.6, 1, 0.2),             # tiny: mostly padding
    (37, 200, 4000, 64, 0.05, 0, 0.0),          # config-5 negatives count
])
def test_combine_bwd_matches_index_add(gpu, BT, N, pmax, C, pad_frac, hot, masked_frac):
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    rng = np.random.default_rng(BT + N)
    slot, masked = _make_slots(rng, BT, N, pmax, pad_frac, hot, masked_frac)
    NC = N + 1
    dpre = rng.standard_normal((BT + BT * NC, C)).astype(np.float32)
    cand = dpre[BT:].reshape(BT, NC, C)                        # (a view: the edits below land in dpre)
    cand[masked] = 0.0                                         # masked clicks carry exactly zero gradient
    dpre[:BT][masked] = 0.0
    # float64 reference
    dU = dpre[:BT].astype(np.float64) + cand.astype(np.float64).sum(1)
    dV = np.zeros((2 * BT + pmax + 1, C))
    dV[:BT] = dpre[:BT]
    dV[BT:2 * BT] = cand[:, 0]
    s = slot.reshape(-1)
    ok = s >= 0
    np.add.at(dV, 2 * BT + s[ok], cand[:, 1:].reshape(-1, C)[ok].astype(np.float64))
    if pad_frac >= 0.2:
        assert (s == pmax).sum() > 0.125 * ok.sum()            # the case ADVICE r01 asked for
    d_dpre, d_slot = torch.from_numpy(dpre).to(gpu), torch.from_numpy(slot).to(gpu)
    need = lib.cham_combine_bwd_workspace_bytes(C, BT, N, pmax)
    outs = []
    for _ in range(2):
        ws = torch.full(((need + 3) // 4,), float('nan'), dtype=torch.float32, device=gpu)
        o_dU = torch.full((BT, C), float('nan'), device=gpu)
        o_dV = torch.full((2 * BT + pmax + 1, C), float('nan'), device=gpu)
        check(lib.cham_combine_bwd(ptr(d_dpre), C, BT, N, pmax, ptr(d_slot), ptr(o_dU), ptr(o_dV), ptr(ws), ws.numel() * 4,
                                   torch.cuda.current_stream().cuda_stream), "cham_combine_bwd")
        torch.cuda.synchronize()
        outs.append((o_dU.cpu(), o_dV.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "not bit-reproducible"
    g_dU, g_dV = outs[0][0].double().numpy(), outs[0][1].double().numpy()
    assert np.isfinite(g_dU).all() and np.isfinite(g_dV).all()
    assert np.abs(g_dU - dU).max() < 2e-5 * max(1.0, np.abs(dU).max())
    assert np.abs(g_dV - dV).max() < 2e-5 * max(1.0, np.abs(dV).max())
    assert lib.cham_combine_bwd(ptr(d_dpre), C, BT, N, pmax, ptr(d_slot), ptr(o_dU), ptr(o_dV), ptr(ws), 64, None) == -22


@pytest.mark.parametrize("BT,N,pmax,C,pad_frac,hot,masked_frac", [
    (700, 50, 1000, 256, 0.0, 3, 0.0), (1300, 50, 1000, 128, 0.3, 2, 0.1), (90, 9, 180, 128, 0.6, 1, 0.2), (37, 200, 4000, 64, 0.05, 0, 0.0),
])
def test_combine_bwd_b16_matches_index_add(gpu, BT, N, pmax, C, pad_frac, hot, masked_frac):
    """The bf16 instantiation (candidate rows bf16, clicked-input rows fp32) at the cases of the fp32 test: the candidate rows are rounded
    to bf16 first and the float64 reference is taken over the rounded values, so the bound is the fp32 test's."""
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    rng = np.random.default_rng(BT + N)
    slot, masked = _make_slots(rng, BT, N, pmax, pad_frac, hot, masked_frac)
    NC = N + 1
    dpre_in = rng.standard_normal((BT, C)).astype(np.float32)
    cand32 = rng.standard_normal((BT, NC, C)).astype(np.float32)
    cand32[masked] = 0.0
    dpre_in[masked] = 0.0
    bits = F.round_bf16_bits(cand32).reshape(BT, NC, C)
    cand = (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)       # the bf16 values, widened exactly
    dU = dpre_in.astype(np.float64) + cand.sum(1)
    dV = np.zeros((2 * BT + pmax + 1, C))
    dV[:BT] = dpre_in
    dV[BT:2 * BT] = cand[:, 0]
    s = slot.reshape(-1)
    ok = s >= 0
    np.add.at(dV, 2 * BT + s[ok], cand[:, 1:].reshape(-1, C)[ok])
    d_in, d_slot = torch.from_numpy(dpre_in).to(gpu), torch.from_numpy(slot).to(gpu)
    d_cand = torch.from_numpy(bits.view(np.int16)).to(gpu).view(torch.bfloat16)
    need = lib.cham_combine_bwd_workspace_bytes(C, BT, N, pmax)
    outs = []
    for _ in range(2):
        ws = torch.full(((need + 3) // 4,), float('nan'), dtype=torch.float32, device=gpu)
        o_dU, o_dV = Out(gpu, (BT, C)), Out(gpu, (2 * BT + pmax + 1, C))
        check(lib.cham_combine_bwd_b16(ptr(d_in), ptr(d_cand), C, BT, N, pmax, ptr(d_slot), o_dU.ptr(), o_dV.ptr(), ptr(ws), ws.numel() * 4,
                                       torch.cuda.current_stream().cuda_stream), "cham_combine_bwd_b16")
        outs.append((o_dU.numpy(), o_dV.numpy()))
    assert F.same_bits(outs[0][0], outs[1][0]) and F.same_bits(outs[0][1], outs[1][1]), "not bit-reproducible"
    g_dU, g_dV = outs[0][0].astype(np.float64), outs[0][1].astype(np.float64)
    assert np.isfinite(g_dU).all() and np.isfinite(g_dV).all()
    print("\n    dU %.2e  dV %.2e  (bound 2e-5)" % (np.abs(g_dU - dU).max() / max(1.0, np.abs(dU).max()), np.abs(g_dV - dV).max() / max(1.0, np.abs(dV).max())))
    assert np.abs(g_dU - dU).max() < 2e-5 * max(1.0, np.abs(dU).max())
    assert np.abs(g_dV - dV).max() < 2e-5 * max(1.0, np.abs(dV).max())
    assert lib.cham_combine_bwd_b16(ptr(d_in), ptr(d_cand), C, BT, N, pmax, ptr(d_slot), o_dU.ptr(), o_dV.ptr(), ptr(ws), 64, None) == -22


def _row_ranges(BT, N):
    """(name, begin, count): the clicked-input rows, exactly the candidate rows (the per-position kernel), the whole matrix in one call, and
    a range that starts and ends inside a position's candidates (one row into position 0's, one row into position 1's - or 0's last)."""
    NC, rows = N + 1, BT + BT * (N + 1)
    return [('inputs', 0, BT), ('candidates', BT, BT * NC), ('whole', 0, rows), ('inside', BT + 1, min(NC, rows - BT - 2))]


@pytest.mark.parametrize("C", F.COMBINE_C)
@pytest.mark.parametrize("case", range(len(F.SLOT_CASES)))
def test_combine_fwd_is_exact(gpu, case, C):
    """N of {1, 3, 9, 50, 200} (N + 1 a multiple of 4 and not), C of {64, 128, 1024, 1280} (1280 floats = 320 float4: a second trip of the
    256 threads), slot tables with pads and masked clicks (-1 reads the pad row 2 BT + pmax).  Rows outside the range stay NaN."""
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check
    lib = _lib.load()
    inp = F.combine_inputs(case, C)
    BT, N, pmax = inp['BT'], inp['N'], inp['pmax']
    rows = BT + BT * (N + 1)
    want = F.combine_fwd(inp['U'], inp['V'], inp['slot'], BT, N, pmax, dtype=np.float32)
    assert want.dtype == np.float32 and want.shape == (rows, C)
    U, V, slot = _dev(gpu, inp['U']), _dev(gpu, inp['V']), _dev(gpu, inp['slot'])
    for name, begin, count in _row_ranges(BT, N):
        def run():
            Z1 = Out(gpu, (rows, C))
            check(lib.cham_combine_fwd(U.data_ptr(), V.data_ptr(), C, BT, N, pmax, slot.data_ptr(), Z1.ptr(), begin, count, _st()), "cham_combine_fwd")
            return (Z1.numpy(),)
        got = _twice(run)[0]
        assert F.same_bits(got[begin:begin + count], want[begin:begin + count]), "rows of the range '%s' differ" % name
        assert np.isnan(got[:begin]).all() and np.isnan(got[begin + count:]).all(), "rows outside the range '%s' were written" % name

    def run16():
        Z1c = Out(gpu, (BT * (N + 1), C), torch.bfloat16)
        check(lib.cham_combine_fwd_b16(U.data_ptr(), V.data_ptr(), C, BT, N, pmax, slot.data_ptr(), Z1c.ptr(), _st()), "cham_combine_fwd_b16")
        return (Z1c.numpy(),)
    assert F.same_bits(_twice(run16)[0], F.round_bf16_bits(want[BT:]).reshape(BT * (N + 1), C)), "bf16 candidate rows are not round_bf16 of the fp32 rows"


def test_combine_fwd_argument_errors(gpu):
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    inp = F.combine_inputs(1, 64)
    BT, N, pmax, C = inp['BT'], inp['N'], inp['pmax'], 64
    rows = BT + BT * (N + 1)
    U, V, slot = _dev(gpu, inp['U']), _dev(gpu, inp['V']), _dev(gpu, inp['slot'])
    Z1 = Out(gpu, (rows, C))
    call = lambda C_, begin, count, z=Z1.ptr(), u=U.data_ptr(): lib.cham_combine_fwd(u, V.data_ptr(), C_, BT, N, pmax, slot.data_ptr(), z, begin, count, _st())
    assert call(C, 0, rows + 1) == -22 and call(C, rows - 1, 2) == -22 and call(C, rows, 1) == -22 and call(C, -1, 2) == -22 and call(C, 0, 0) == -22
    assert call(C - 2, 0, BT) == -22 and call(C, 0, BT, z=None) == -22 and call(C, 0, BT, u=None) == -22
    assert lib.cham_combine_fwd_b16(U.data_ptr(), V.data_ptr(), C - 2, BT, N, pmax, slot.data_ptr(), Z1.ptr(), _st()) == -22
    assert lib.cham_combine_fwd_b16(U.data_ptr(), V.data_ptr(), C, BT, 0, pmax, slot.data_ptr(), Z1.ptr(), _st()) == -22
    torch.cuda.synchronize()
    assert Z1.untouched()
