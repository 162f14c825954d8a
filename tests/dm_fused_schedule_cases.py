"""What tests/test_dm_fused_schedule_gpu.py and scripts/make_dm_fused_parent_bits.py share: the cases that walk the column-tile pipeline of
csrc/dm_fused.hip through its states, host-made deterministic inputs, and one launch of each form into NaN-filled outputs.

The fixture tests/golden/dm_fused_parent_bits.npz was written by the generator from the build BEFORE the tile loop's loads moved in front of
the products: the kernel's results must stay those bits (no operand, product, MFMA order, epilogue arithmetic or sum order changed)."""
import functools
import hashlib
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dm_fused_parent_bits.npz")
FORMS = ('h2h', 'h2', 'p3', 'b16')
# (BT, N, C): the pipeline's states, not the workload's size
CASES = [
    (6, 50, 64),        # one tile: the prologue's tile is the last
    (6, 50, 128),       # two tiles
    (6, 50, 320),       # odd tile count in steady state; the second workgroup holds 1 of 5 positions
    (11, 50, 1024),     # sixteen tiles; last workgroup partial
    (3, 31, 256),       # 1 + N = 32: a position per wave
    (2, 255, 192),      # 1 + N = 256: one position per workgroup, a wave never crosses a position
    (1, 50, 1024),      # a single position
]
STORED = CASES[0]       # the case whose outputs the fixture holds in full
BEHIND = 64             # rows allocated behind the valid rows of dS1, Z2 and pred


def case_id(case):
    return "%dx%dx%d" % case


@functools.lru_cache(maxsize=None)
def inputs(BT, N, C):
    """Gaussian dS1, 0.1 x Gaussian Ws1, tanh of Gaussians for Z2 and pred (the tanh in float64, rounded once to fp32)."""
    rng = np.random.default_rng(1000003 * BT + 1009 * N + C)
    Rc = BT * (N + 1)
    inp = dict(dS1=rng.standard_normal((Rc, 128)).astype(np.float32),
               Ws1=(0.1 * rng.standard_normal((C, 128))).astype(np.float32),
               Z2=np.tanh(rng.standard_normal((Rc, C))).astype(np.float32),
               pred=np.tanh(rng.standard_normal((BT, C))).astype(np.float32))
    for v in inp.values():
        v.setflags(write=False)
    return inp


def inputs_digest(inp):
    h = hashlib.sha256()
    for k in ('dS1', 'Ws1', 'Z2', 'pred'):
        h.update(inp[k].tobytes())
    return h.hexdigest()


def _framed(gpu, a, fill, dtype=torch.float32):
    buf = torch.full((a.shape[0] + BEHIND, a.shape[1]), fill, dtype=dtype, device=gpu)
    buf[:a.shape[0]] = torch.from_numpy(np.array(a)).to(gpu).to(dtype)
    return buf


def _bits(t):
    """A device tensor -> its bytes as a numpy array (16-bit formats as uint16, fp32 as uint32)."""
    if t.element_size() == 2:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def run_form(gpu, lib, form, case, fill=float('nan')):
    """One form at one case: two launches into NaN-filled outputs, which must agree bit for bit (a load that had not landed when it was used
    shows as a difference or a NaN).  `fill`: what stands in the BEHIND rows behind the valid rows of dS1, Z2 and pred.
    -> {name: bits} for every plane of dZ2, dpred and b2part."""
    from chameleon_recsys_amd._lib import check, ptr
    BT, N, C = case
    NC = N + 1
    Rc = BT * NC
    inp = inputs(BT, N, C)
    st = torch.cuda.current_stream().cuda_stream
    b16 = form == 'b16'
    dt = torch.bfloat16 if b16 else torch.float32
    dS1, Z2, pred = _framed(gpu, inp['dS1'], fill, dt), _framed(gpu, inp['Z2'], fill, dt), _framed(gpu, inp['pred'], fill)
    Ws1 = torch.from_numpy(np.array(inp['Ws1'])).to(gpu)
    if b16:
        W16 = Ws1.bfloat16()
    else:
        W3 = torch.zeros(3, C, 128, dtype=torch.bfloat16, device=gpu)
        check(lib.cham_split3(ptr(Ws1), C, 128, 128, ptr(W3), C * 128, 128, None, 0, 0, st), "cham_split3")
        rw, rout, rds = (torch.zeros(8, device=gpu) for _ in range(3))
        check(lib.cham_h2_scale_rownorm(ptr(Ws1), C, 128, 128, None, ptr(rw), st), "cham_h2_scale_rownorm")
        check(lib.cham_h2_scale_rownorm2(ptr(dS1), Rc, 128, 128, rw.data_ptr() + 8, ptr(rout), ptr(rds), st), "cham_h2_scale_rownorm2")
        Wh = torch.zeros(2, C, 128, dtype=torch.float16, device=gpu)
        check(lib.cham_split2h(ptr(Ws1), C, 128, 128, ptr(Wh), C * 128, 128, None, 0, 0, ptr(rw), 0, st), "cham_split2h")
    nplanes, odt = {'p3': (3, torch.bfloat16), 'b16': (1, torch.bfloat16)}.get(form, (2, torch.float16))
    runs = []
    for _ in range(2):
        D = torch.full((nplanes, Rc, C), float('nan'), dtype=odt, device=gpu)
        dp, b2 = torch.full((BT, C), float('nan'), device=gpu), torch.full((BT, C), float('nan'), device=gpu)
        tail = (ptr(Z2), ptr(pred), C, BT, N, ptr(D), Rc * C)
        if form == 'p3':
            rc = lib.cham_dm_mulpred_p3(ptr(dS1), 128, 128, ptr(W3), C * 128, *tail, ptr(dp), ptr(b2), st)
        elif form == 'h2':
            rc = lib.cham_dm_mulpred_h2(ptr(dS1), 128, 128, ptr(W3), C * 128, *tail, ptr(rout), ptr(dp), ptr(b2), st)
        elif form == 'h2h':
            rc = lib.cham_dm_mulpred_h2h(ptr(dS1), 128, 128, ptr(Wh), C * 128, ptr(rds), ptr(rw), *tail, ptr(rout), ptr(dp), ptr(b2), st)
        else:
            rc = lib.cham_dm_mulpred_b16(ptr(dS1), 128, 128, ptr(W16), ptr(Z2), ptr(pred), C, BT, N, ptr(D), ptr(dp), ptr(b2), st)
        check(rc, "cham_dm_mulpred_" + form)
        torch.cuda.synchronize()
        out = {"dZ2_%d" % q: _bits(D[q]) for q in range(nplanes)}
        out["dpred"], out["b2part"] = _bits(dp), _bits(b2)
        runs.append(out)
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), "two launches differ in %s (%s, %s)" % (k, form, case_id(case))
    nan16 = {torch.bfloat16: 0x7F80, torch.float16: 0x7C00}[odt]
    for k, v in runs[0].items():
        if v.dtype == np.uint16:
            isnan = ((v & nan16) == nan16) & ((v & (0x7F if odt == torch.bfloat16 else 0x3FF)) != 0)
        else:
            isnan = np.isnan(v.view(np.float32))
        assert not isnan.any(), "%s holds a NaN (%s, %s): not fully written, or a value that had not landed was used" % (k, form, case_id(case))
    return runs[0]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
