"""Manual tool (not a test): the two forms of the fused scorer dgrad (csrc/dm_fused.hip) that the step drivers run - cham_dm_mulpred_h2h (fp32
configuration: two fp16 planes in and out) and cham_dm_mulpred_b16 (bf16 configuration) - at the G1 shape, on random operands (tanh of
Gaussians for Z2 / pred) and the scale records cham_h2_scale_rownorm / _rownorm2 / cham_split2h write, as tests/test_dm_fused_gpu.py drives them.

    python scripts/bench_dm_fused_forms.py [--other-lib PATH] [--rounds 12] [--launches 10]

--other-lib: a second build of libchameleon_nar.so (another checkout's, copied somewhere).  The two libraries alternate in ONE process, round
by round, on the same buffers; per library and form: median and minimum of the per-round mean launch time, and the TB/s of the algorithmic
bytes (dS1 and Z2 in, the planes of dZ2 out; Ws1, pred and the per-position outputs are < 1 % of them)."""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import check, ptr


def _bind(path):
    lib = ctypes.CDLL(path)
    for name in ("cham_dm_mulpred_h2h", "cham_dm_mulpred_b16"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def _round(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other-lib", default=None)
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--launches", type=int, default=10)
    args = ap.parse_args()
    assert args.rounds >= 10 or not args.other_lib, "alternate over at least 10 rounds"
    base = _lib.load()
    libs = [("this build", _bind(_lib.LIB_PATH))]
    if args.other_lib:
        libs.append(("other (%s)" % args.other_lib, _bind(os.path.abspath(args.other_lib))))
    dev = torch.device("cuda:0")
    BT, N, C = 256 * 19, 50, 1024
    NC = N + 1
    Rc = BT * NC
    g = torch.Generator(device=dev).manual_seed(0)
    dS1 = torch.randn(Rc, 128, device=dev, generator=g) * 1e-3
    Ws1 = torch.randn(C, 128, device=dev, generator=g) * 0.05
    Z2 = torch.tanh(torch.randn(Rc, C, device=dev, generator=g))
    pred = torch.tanh(torch.randn(BT, C, device=dev, generator=g))
    st = torch.cuda.current_stream().cuda_stream
    rw, rout, rds = (torch.zeros(8, device=dev) for _ in range(3))
    check(base.cham_h2_scale_rownorm(ptr(Ws1), C, 128, 128, None, ptr(rw), st), "cham_h2_scale_rownorm")
    check(base.cham_h2_scale_rownorm2(ptr(dS1), Rc, 128, 128, rw.data_ptr() + 8, ptr(rout), ptr(rds), st), "cham_h2_scale_rownorm2")
    Wh = torch.zeros(2, C, 128, dtype=torch.float16, device=dev)
    check(base.cham_split2h(ptr(Ws1), C, 128, 128, ptr(Wh), C * 128, 128, None, 0, 0, ptr(rw), 0, st), "cham_split2h")
    D = torch.empty(2, Rc, C, dtype=torch.float16, device=dev)
    dp, b2 = torch.empty(BT, C, device=dev), torch.empty(BT, C, device=dev)
    dS1b, Ws1b, Z2b = dS1.bfloat16(), Ws1.bfloat16(), Z2.bfloat16()
    Db = torch.empty(Rc, C, dtype=torch.bfloat16, device=dev)
    torch.cuda.synchronize()

    def calls(lib):
        return {
            "h2h": (lambda: check(lib.cham_dm_mulpred_h2h(ptr(dS1), 128, 128, ptr(Wh), C * 128, ptr(rds), ptr(rw), ptr(Z2), ptr(pred), C, BT, N, ptr(D),
                                                          Rc * C, ptr(rout), ptr(dp), ptr(b2), st), "cham_dm_mulpred_h2h"),
                    4.0 * Rc * 128 + 4.0 * Rc * C + 4.0 * Rc * C),
            "b16": (lambda: check(lib.cham_dm_mulpred_b16(ptr(dS1b), 128, 128, ptr(Ws1b), ptr(Z2b), ptr(pred), C, BT, N, ptr(Db), ptr(dp), ptr(b2), st),
                                  "cham_dm_mulpred_b16"),
                    2.0 * Rc * 128 + 2.0 * Rc * C + 2.0 * Rc * C),
        }

    for form in ("h2h", "b16"):
        fns = [(name, *calls(lib)[form]) for name, lib in libs]
        for _, fn, _ in fns:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _, _ in fns}
        for _ in range(args.rounds):
            for name, fn, _ in fns:
                times[name].append(_round(fn, args.launches))
        for name, _, by in fns:
            t = times[name]
            med, mn = statistics.median(t), min(t)
            print("cham_dm_mulpred_%s  %-40s median %.4f ms  min %.4f ms  (%d rounds x %d launches; %.2f TB/s of its %.2f GB at the median)"
                  % (form, name, med, mn, len(t), args.launches, by / med / 1e9, by / 1e9))
        assert torch.isfinite(dp).all() and torch.isfinite(b2).all()


if __name__ == "__main__":
    main()
