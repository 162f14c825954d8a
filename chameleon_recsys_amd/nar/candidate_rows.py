"""The arithmetics of the candidate rows: one class per way the B*T*(1+N) candidate rows of a step are stored and multiplied (the "arms")."""
# The step driver (nar_model.NARModuleModel._forward / backward) owns the SCHEDULE - lanes and events - and asks the arm of the step for every
# piece of arithmetic:
#   F32Rows    fp32 matrices through NARRuntime.gemm (gemm_dtype 'f32_native', CHAM_GEMM_P3=0, and any step with dropout or without candidate rows)
#   P3Rows     Z1 and dZ2 as three bf16 planes (csrc/gemm_p3.hip; CHAM_GEMM_H2=0)
#   H2Rows     ... as two fp16 planes + scale records (csrc/gemm_h2.hip; the default)
#   Bf16Rows   bf16-resident matrices (csrc/gemm_b16.hip; gemm_dtype 'bf16')
# An arm holds no state: its persistent buffers (weight planes / shadows, scale records) are attributes of the runtime, its per-shape buffers
# attributes of the StepPlan, under the names tests and tools read.  The R = pl.PC candidate rows of a step are rows [P, P + R) of the fp32 matrices
# (P = pl.P valid positions) or the first R rows of the plane / bf16 matrices.  A new arm subclasses the nearest one and overrides what differs;
# every method enqueues on torch's current stream (`s` is its raw handle where an entry point is called directly).
import torch

from .. import _lib
from .._lib import check, ptr

ACT_NONE, ACT_LEAKY, ACT_TANH = 0, 1, 2


def _h2b_block():
    return int(_lib.load().cham_h2b_block_elements())


def blocked_plane_elements(tiles, C):
    """Elements of ONE tile-blocked plane of `tiles` row tiles and leading dimension C (csrc/common.h h2b_index)."""
    return tiles * (C // 32) * _h2b_block()


def planes_from_blocked(t, tiles, C=None):
    """[planes, >= tiles * (C / 32) * block] memory in the TILE-BLOCKED layout ([row tile][C / 32][256][32] (+ padding), csrc/common.h
    h2b_index) -> the row-major [planes, tiles * 256, C] matrix (a copy; tests and debugging)."""
    npl = t.shape[0]
    C = t.shape[2] if C is None else C
    blk = _h2b_block()
    flat = t.reshape(npl, -1)[:, :tiles * (C // 32) * blk]
    return flat.reshape(npl, tiles, C // 32, blk)[..., :8192].reshape(npl, tiles, C // 32, 256, 32).permute(0, 1, 3, 2, 4).reshape(npl, tiles * 256, C)


def planes_to_blocked(t):
    """Row-major [planes, R, C] (C % 32 == 0) -> (tile-blocked [planes, tiles * (C / 32) * block] with the rows beyond R zero, tiles)."""
    npl, R, C = t.shape
    tiles = -(-R // 256)
    blk = _h2b_block()
    pad = torch.zeros(npl, tiles * 256, C, dtype=t.dtype, device=t.device)
    pad[:, :R] = t
    out = torch.zeros(npl, tiles, C // 32, blk, dtype=t.dtype, device=t.device)
    out[..., :8192] = pad.reshape(npl, tiles, 256, C // 32, 32).permute(0, 1, 3, 2, 4).reshape(npl, tiles, C // 32, 8192)
    return out.reshape(npl, -1), tiles


class F32Rows:
    """fp32 rows: one [P + R, C] matrix each for Z1, Z2, dZ2, dZ1, clicked-input rows first."""
    planes = False          # Z1 / dZ2 candidate rows live as planes (schedule: the W2 weight gradient is a plane GEMM + the clicked rows)
    b16 = False             # bf16-resident (schedule: which batches enqueue the critical chain first; the W2 wgrad runs beside the CAR dgrad)
    softmax_fwd, softmax_bwd = 'cham_score_softmax_fwd', 'cham_score_softmax_bwd'      # entry points that read this arm's S3 (bwd: + '_dev')
    rankloss_fwd, rankloss_bwd = 'cham_score_rankloss_fwd', 'cham_score_rankloss_bwd'   # ... under a pairwise ranking loss (--loss_function; csrc/rank_loss.hip)
    diversity_bwd = 'cham_diversity_bwd'                                               # ... and the one that runs behind softmax_bwd (--diversity_reg_factor)

    def __init__(self, rt):
        self.rt = rt

    def refresh_shadows(self, s):      # the arm's shadows of the weights, once per weight version (NARRuntime.refresh_shadows)
        pass

    def alloc(self, pl, f32):
        pl.Z1, pl.Z2, pl.dZ2, pl.dZ1 = (f32(pl.Rall, pl.C) for _ in range(4))

    def cand_Z1(self, pl, P, n):
        return pl.Z1[P:P + n]

    def fused_dz2(self, pl):      # does ONE kernel take the scorer layer-1 dgrad and the cand (.) pred backward this step?
        return False

    def dm_timed(self, pl, **flags):      # ... a launch of the GEMM family in rt.profile
        return self.rt._timed(1, (), lambda c0, c1: dict(M=pl.PC, N=pl.C, K=128, transA=0, transB=1, splits=1, act=0, dref=False, dact=0, bias=False,
                                                         rowscale=False, dmf=True, tile=0, epi=0, **flags))

    # ---- forward
    def z1(self, pl, s, drop):      # candidate rows of the PreCAR output; drop = the step's dense input form (nar/input_rows.py: dense rows x the stacked W1) or None (U + V)
        rt, C, P, R = self.rt, pl.C, pl.P, pl.PC
        if drop:
            rt.gemm(pl.Xd[P:], drop.W1, pl.Z1[P:], R, C, drop.Fw, drop.Fw, C, C, bias=rt.p('b1'), act=ACT_LEAKY)
        else:
            check(rt.lib.cham_combine_fwd(ptr(pl.U), ptr(pl.V), C, P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.Z1), P, R, s), "cham_combine_fwd")

    def car_fwd(self, pl):
        rt, C = self.rt, pl.C
        rt.gemm(pl.Z1[pl.P:], rt.p('W2'), pl.Z2[pl.P:], pl.PC, C, C, C, C, C, bias=rt.p('b2'), act=ACT_TANH)

    def scorer_fwd(self, pl, s):      # (cand (.) pred) -> 128 -> 64 -> 32
        rt, p, C, R = self.rt, self.rt.p, pl.C, pl.PC
        rt.gemm(pl.Z2[pl.P:pl.P + R], p('Ws1'), pl.S1, R, 128, C, C, 128, 128, bias=p('bs1'), act=ACT_LEAKY, rowscale=pl.pred, ldrs=C, rs_div=pl.NC,
                h2scales=(rt.sc_unit, rt.sc_ws1n) if rt.s1_h2_fwd else None)
        rt.gemm(pl.S1, p('Ws2'), pl.S2, R, 64, 128, 128, 64, 64, bias=p('bs2'), act=ACT_LEAKY)
        rt.gemm(pl.S2, p('Ws3'), pl.S3, R, 32, 64, 64, 32, 32, bias=p('bs3'), act=ACT_LEAKY)

    # ---- backward
    def scorer_dgrad(self, pl, s):      # scorer layers 3 and 2 (-> dS1) and what the arm derives from dS1 before its consumers start
        rt, p, R = self.rt, self.rt.p, pl.PC
        rt.gemm(pl.dS3, p('Ws3'), pl.dS2, R, 64, 32, 32, 32, 64, transB=1, dref=pl.S2, ldr=64, dact=ACT_LEAKY)
        rt.gemm(pl.dS2, p('Ws2'), pl.dS1, R, 128, 64, 64, 64, 128, transB=1, dref=pl.S1, ldr=128, dact=ACT_LEAKY)
        if not self.fused_dz2(pl):
            pl.ensure_rows('dZ2')          # the scorer layer-1 dgrad goes through HBM

    def s1_wgrad(self, pl):      # (two-fp16-plane arm, CHAM_S1_H2: |cand (.) pred| <= 1 - the constant scale record; dS1 by its max row norm)
        rt, C, R = self.rt, pl.C, pl.PC
        rt.gemm(pl.Z2[pl.P:pl.P + R], pl.dS1, rt.g('Ws1'), C, 128, R, C, 128, 128, transA=1, rowscale=pl.pred, ldrs=C, rs_div=pl.NC, splits=0,
                h2scales=(rt.sc_unit, pl.sc_ds1) if (rt.s1_h2 and self.planes) else None)
        rt.colsum(pl.dS1, 128, R, 128, rt.g('bs1'))

    def small_wgrads(self, pl):      # layers 2-4: short split-K GEMMs + column sums, nothing but Adam (and the early DP bucket) waits for them
        rt, g, R, b16 = self.rt, self.rt.g, pl.PC, self.b16
        if b16:
            rt.gemm_b16(pl.S1, 128, 1, pl.dS2, 64, 0, g('Ws2'), 64, 1, 128, 64, R, splits=0)
        else:
            rt.gemm(pl.S1, pl.dS2, g('Ws2'), 128, 64, R, 128, 64, 64, transA=1, splits=0)
        rt.colsum(pl.dS2, 64, R, 64, g('bs2'), b16=b16)
        if b16:
            rt.gemm_b16(pl.S2, 64, 1, pl.dS3, 32, 0, g('Ws3'), 32, 1, 64, 32, R, splits=0)
        else:
            rt.gemm(pl.S2, pl.dS3, g('Ws3'), 64, 32, R, 64, 32, 32, transA=1, splits=0)
        rt.colsum(pl.dS3, 32, R, 32, g('bs3'), b16=b16)
        rt.colsum(pl.S3, 32, R, 32, g('Ws4'), w=pl.ds, b16=b16)
        rt.colsum(pl.ds, 1, R, 1, g('bs4'))

    def s1_dgrad(self, pl):      # scorer layer-1 dgrad through HBM (steps whose dz2() does not fuse it)
        self.rt.gemm(pl.dS1, self.rt.p('Ws1'), pl.dZ2[pl.P:pl.P + pl.PC], pl.PC, pl.C, 128, 128, 128, pl.C, transB=1)

    def dz2(self, pl, s):      # cand (.) pred backward -> the gradient at the CAR tanh + dpred.  k_mulpred_bwd: HBM-bound (3 GB), between two MFMA-bound GEMMs
        P, R = pl.P, pl.PC
        check(self.rt.lib.cham_mulpred_bwd(ptr(pl.dZ2[P:P + R]), ptr(pl.Z2[P:P + R]), ptr(pl.pred), pl.C, P, pl.N, ptr(pl.dpred), s), "cham_mulpred_bwd")

    def car_dgrad(self, pl):
        rt, C, P, R = self.rt, pl.C, pl.P, pl.PC
        if R > 0:
            rt.gemm(pl.dZ2[P:P + R], rt.p('W2'), pl.dZ1[P:P + R], R, C, C, C, C, C, transB=1, dref=pl.Z1[P:P + R], ldr=C, dact=ACT_LEAKY)

    def w2_wgrad(self, pl, splits=0, cand=True):      # over ALL rows in one GEMM, the second-largest of the step
        self.rt.gemm(pl.Z1, pl.dZ2, self.rt.g('W2'), pl.C, pl.C, pl.P + pl.PC, pl.C, pl.C, pl.C, transA=1, splits=0)

    def b2_grad(self, pl):
        self.rt.colsum(pl.dZ2, pl.C, pl.P + pl.PC, pl.C, self.rt.g('b2'))

    def dense_dZ1(self, pl, st):      # dZ1 of all CAR rows as one fp32 matrix (dense PreCAR backward of the dropout path)
        return pl.dZ1

    # ---- the cosine head (--recommendations_ranking cosine; csrc/cosine.hip) over this arm's storage
    def cosine_fwd(self, pl, s):      # cos(pred, candidate row) -> pl.cosq [R, 4] = (cos, 0, 0, 0), the inverse norms pl.rz [R] / pl.rp [P]
        P, C = pl.P, pl.C
        check(self.rt.lib.cham_cosine_fwd(ptr(pl.Z2[P:P + pl.PC]), C, ptr(pl.pred), C, P, pl.N, ptr(pl.cosq), ptr(pl.rz), ptr(pl.rp), s), "cham_cosine_fwd")

    def cosine_bwd(self, pl, s):      # ds -> the gradient at the CAR tanh + dpred: what scorer_dgrad + s1_dgrad + s1_wgrad + small_wgrads + dz2 are to the MLP head
        P, R = pl.P, pl.PC
        pl.ensure_rows('dZ2')
        check(self.rt.lib.cham_cosine_bwd(ptr(pl.Z2[P:P + R]), ptr(pl.pred), ptr(pl.ds), ptr(pl.rz), ptr(pl.rp), ptr(pl.cosq), ptr(pl.mask), pl.C, P, pl.N,
                                          ptr(pl.dZ2[P:P + R]), ptr(pl.dpred), None, s), "cham_cosine_bwd")

    def combine_bwd(self, pl, ws, st):      # dZ1 -> dU (per click) and dV (per item row) by the deterministic slot scatter
        check(self.rt.lib.cham_combine_bwd(ptr(pl.dZ1), pl.C, pl.P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.dU), ptr(pl.dV), ptr(ws), ws.numel() * 4, st),
              "cham_combine_bwd")


class P3Rows(F32Rows):
    """Plane-resident CAR GEMMs: the candidate rows of Z1 and dZ2 live in HBM as three bf16 planes written by their producers (no fp32 copy)."""
    # W2 / W2^T / Ws1 get plane shadows once per weight version; Z2, dZ1 and the scorer stay fp32.  Base of the two-fp16-plane arm.
    planes = True
    plane_count, plane_dtype = 3, torch.bfloat16

    def __init__(self, rt):
        self.rt = rt
        C, dev = rt.layout.C, rt.device
        rt.w2p = torch.zeros(self.plane_count, C, C, dtype=self.plane_dtype, device=dev)       # planes of W2 as stored (CAR dgrad)
        rt.w2tp = torch.zeros(self.plane_count, C, C, dtype=self.plane_dtype, device=dev)      # planes of W2^T (CAR forward)
        rt.ws1p = torch.zeros(3, C, 128, dtype=torch.bfloat16, device=dev)     # planes of Ws1 as stored (the fused dgrad's own products)

    def refresh_shadows(self, s):
        rt, C = self.rt, self.rt.layout.C
        check(rt.lib.cham_split3(ptr(rt.p('W2')), C, C, C, ptr(rt.w2p), C * C, C, ptr(rt.w2tp), C * C, C, s), "cham_split3")
        if rt.dm_fused:
            check(rt.lib.cham_split3(ptr(rt.p('Ws1')), C, 128, 128, ptr(rt.ws1p), C * 128, 128, None, 0, 0, s), "cham_split3")

    @classmethod
    def estimate_bytes(cls, rt, L, B, T, N):      # share of StepPlan.estimate_bytes: Z1 and dZ2 as planes, the b2 partial sums and the segment table
        return 2 * cls.plane_count * 2 * B * T * (N + 1) * L.C + 4 * B * T * L.C + 4 * int(rt.lib.cham_group_rows_segments_len(2 * B * T + 20 * N + 1))

    def alloc(self, pl, f32):
        # The candidate rows of Z1 exist as planes only, and with the fused scorer dgrad those of dZ2 too: the fp32 matrices keep the
        # clicked-input rows (ensure_rows() grows them on the paths that do need all rows - dropout, NC outside the fused kernel's range)
        C, BT, Rall = pl.C, pl.BT, pl.Rall
        # (the cosine head's backward writes the planes directly, like the fused dgrad)
        pl.Z1, pl.Z2, pl.dZ2, pl.dZ1 = f32(BT, C), f32(Rall, C), f32(BT if (self.fused_dz2(pl) or self.rt.cosine) else Rall, C), f32(Rall, C)
        pl.z1_tiles = pl.dz2_tiles = 0
        self.alloc_planes(pl)
        pl.p3_ps = pl.Rc * C                              # plane stride of a row-major operand ...
        pl.z1_ps, pl.dz2_ps = pl.Z1p[0].numel(), pl.dZ2p[0].numel()      # ... and of each operand as allocated
        pl.b2part = f32(BT, C)

    def alloc_planes(self, pl):
        pl.Z1p, pl.dZ2p = (torch.empty(3, pl.Rc, pl.C, dtype=torch.bfloat16, device=self.rt.device) for _ in range(2))

    def cand_Z1(self, pl, P, n):
        z = pl.Z1p[:, :n].float()
        return z[0] + z[1] + z[2]

    def fused_dz2(self, pl):
        return self.rt.dm_fused and 32 <= pl.NC <= 256

    def z1(self, pl, s, drop):
        check(self.rt.lib.cham_combine_fwd_p3(ptr(pl.U), ptr(pl.V), pl.C, pl.P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.Z1p), pl.p3_ps, s), "cham_combine_fwd_p3")

    def car_fwd(self, pl):
        rt, C = self.rt, pl.C
        rt.gemm_p3(pl.Z1p, pl.p3_ps, C, rt.w2tp, C * C, C, 0, pl.Z2[pl.P:], C, pl.PC, C, C, bias=rt.p('b2'), act=ACT_TANH)

    def dz2(self, pl, s):
        # ... straight into the planes + this position's share of the b2 gradient; with the layer-1 dgrad in the same kernel where it takes the
        # shape (csrc/dm_fused.hip): dM never reaches HBM
        rt, C, P, R = self.rt, pl.C, pl.P, pl.PC
        if self.fused_dz2(pl):
            with self.dm_timed(pl, bf16=False, h2out=False, f16p=False):
                check(rt.lib.cham_dm_mulpred_p3(ptr(pl.dS1), 128, 128, ptr(rt.ws1p), C * 128, ptr(pl.Z2[P:P + R]), ptr(pl.pred), C, P, pl.N, ptr(pl.dZ2p),
                                                pl.p3_ps, ptr(pl.dpred), ptr(pl.b2part), s), "cham_dm_mulpred_p3")
        else:
            check(rt.lib.cham_mulpred_bwd_p3(ptr(pl.dZ2[P:P + R]), ptr(pl.Z2[P:P + R]), ptr(pl.pred), C, P, pl.N, ptr(pl.dpred), ptr(pl.dZ2p), pl.p3_ps,
                                             ptr(pl.b2part), s), "cham_mulpred_bwd_p3")

    def car_dgrad(self, pl):      # planes of dZ2 x planes of W2 as stored; leaky' from the sign of Z1's h plane
        rt, C = self.rt, pl.C
        rt.gemm_p3(pl.dZ2p, pl.p3_ps, C, rt.w2p, C * C, C, 0, pl.dZ1[pl.P:], C, pl.PC, C, C, dref_h=pl.Z1p, ldr=C, dact=ACT_LEAKY)

    def w2_wgrad_cand(self, pl, splits):      # candidate rows' share of the W2 weight gradient from the planes (TN, split-K)
        self.rt.gemm_p3(pl.Z1p, pl.p3_ps, pl.C, pl.dZ2p, pl.p3_ps, pl.C, 1, self.rt.g('W2'), pl.C, pl.C, pl.C, pl.PC, splits=splits)

    def w2_wgrad(self, pl, splits=0, cand=True):      # ... (unless another lane wrote it: cand=False) + the clicked-input rows (fp32) by the on-the-fly kernel
        if cand:
            self.w2_wgrad_cand(pl, splits)
        self.rt.gemm(pl.Z1, pl.dZ2, self.rt.g('W2'), pl.C, pl.C, pl.P, pl.C, pl.C, pl.C, transA=1, splits=0, accumulate=1)

    def b2_grad(self, pl):      # b2 from the per-position partial sums the dZ2 producer left + the clicked rows
        self.rt.colsum(pl.b2part, pl.C, pl.P, pl.C, self.rt.g('b2'))
        self.rt.colsum(pl.dZ2, pl.C, pl.P, pl.C, self.rt.g('b2'), accumulate=1)


class H2Rows(P3Rows):
    """Two fp16 planes (h, l) x a power-of-two scale derived on the device from a bound of the matrix: THREE plane products instead of six."""
    # Optionally TILE-BLOCKED planes (CHAM_H2_BLOCKED), per-click sums of dZ1 from the CAR dgrad's epilogue (CHAM_DGRAD_GROUPSUM), the scorer's
    # first layer on two fp16 planes (CHAM_S1_H2)
    plane_count, plane_dtype = 2, torch.float16

    def __init__(self, rt):
        P3Rows.__init__(self, rt)
        # H2Scale records (32 bytes each, zero-initialised): W2's scale; max row norm of Ws1 (factor of the dZ2 bound)
        rt.sc_w2, rt.sc_ws1n = (torch.zeros(8, dtype=torch.float32, device=rt.device) for _ in range(2))
        # constant record of an operand bounded by 1 (cand (.) pred: tanh x tanh): scale 2^14 - a factor of two inside fp16's range
        rt.sc_unit = torch.tensor([16384.0, 1.0 / 16384.0, 1.0, 0, 0, 0, 0, 0], dtype=torch.float32, device=rt.device)
        # ... and Ws1's two fp16 planes under the scale of sc_ws1n (the fused dgrad's own products, CHAM_S1_H2)
        rt.ws1h = torch.zeros(2, rt.layout.C, 128, dtype=torch.float16, device=rt.device)

    def refresh_shadows(self, s):
        rt, C = self.rt, self.rt.layout.C
        check(rt.lib.cham_split2h(ptr(rt.p('W2')), C, C, C, ptr(rt.w2p), C * C, C, ptr(rt.w2tp), C * C, C, ptr(rt.sc_w2), 1, s), "cham_split2h")
        if rt.cosine:      # no Ws1
            return
        k1 = rt.layout.entries['Ws1'].shape[1]
        check(rt.lib.cham_h2_scale_rownorm(ptr(rt.p('Ws1')), C, k1, k1, None, ptr(rt.sc_ws1n), s), "cham_h2_scale_rownorm")
        if rt.dm_fused:
            check(rt.lib.cham_split3(ptr(rt.p('Ws1')), C, 128, 128, ptr(rt.ws1p), C * 128, 128, None, 0, 0, s), "cham_split3")
            if rt.dm_f16:     # (scale: the row-norm record derived just above - no second pass over the weight)
                check(rt.lib.cham_split2h(ptr(rt.p('Ws1')), C, 128, 128, ptr(rt.ws1h), C * 128, 128, None, 0, 0, ptr(rt.sc_ws1n), 0, s), "cham_split2h")

    def alloc_planes(self, pl):
        # TILE-BLOCKED planes (round 6; csrc/common.h h2b_index): [row tiles of 256][C / 32][256][32] - what the NT GEMMs fetch per
        # request is whole 128-byte lines.  Z1's planes always (cham_combine_fwd_h2b writes them); dZ2's when the fused scorer dgrad
        # is their producer (cham_dm_mulpred_h2_blk; the unfused cham_mulpred_bwd_h2 writes row-major).  Row tiles are allocated
        # whole (+ one: a workgroup of the fused dgrad addresses two tiles from its first row's), zero-initialised.
        rt, dev, C, Rc = self.rt, self.rt.device, pl.C, pl.Rc
        tiles = -(-Rc // 256) + 1
        if rt.h2_blocked:
            pl.z1_tiles = tiles if rt.h2_blocked_which in ("1", "z1") else 0
            pl.dz2_tiles = tiles if (self.fused_dz2(pl) and rt.h2_blocked_which in ("1", "dz2")) else 0
        pl.Z1p, pl.dZ2p = (torch.zeros(2, blocked_plane_elements(t, C), dtype=torch.float16, device=dev) if t
                           else torch.zeros(2, Rc, C, dtype=torch.float16, device=dev) for t in (pl.z1_tiles, pl.dz2_tiles))
        # the scale records of the two matrices and of dS1 itself (operand of the Ws1 weight gradient)
        pl.sc_z1, pl.sc_dz2, pl.sc_ds1 = (torch.zeros(8, dtype=torch.float32, device=dev) for _ in range(3))
        # per-click column sums of dZ1 from the CAR dgrad's epilogue (round 6; csrc/gemm_h2.hip H2Params::gsum): dU without a second
        # pass over the 1 GB of candidate rows
        if rt.dgrad_groupsum and pl.NC >= 32 and Rc > 0:
            pl.gsum = torch.empty(int(rt.lib.cham_gemm_h2_groupsum_bytes(Rc, C, pl.NC)) // 4, dtype=torch.float32, device=dev)

    def cand_Z1(self, pl, P, n):
        z = (planes_from_blocked(pl.Z1p, pl.z1_tiles, pl.C) if pl.z1_tiles else pl.Z1p)[:, :n].float()      # tile-blocked planes -> row-major
        return (z[0] + z[1]) * pl.sc_z1[1]

    def z1(self, pl, s, drop):      # ... x 2^k, k from the bound max|U| + max|V|
        lib, C, P = self.rt.lib, pl.C, pl.P
        check(lib.cham_h2_scale_absmax(ptr(pl.U), P * C, ptr(pl.V), (2 * P + pl.pmax + 1) * C, ptr(pl.sc_z1), s), "cham_h2_scale_absmax")
        check(lib.cham_combine_fwd_h2b(ptr(pl.U), ptr(pl.V), C, P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.Z1p), pl.z1_ps, ptr(pl.sc_z1),
                                       1 if pl.z1_tiles else 0, s), "cham_combine_fwd_h2")

    def car_fwd(self, pl):
        rt, C = self.rt, pl.C
        rt.gemm_h2(pl.Z1p, pl.z1_ps, C, pl.sc_z1, rt.w2tp, C * C, C, rt.sc_w2, 0, pl.Z2[pl.P:], C, pl.PC, C, C, bias=rt.p('b2'), act=ACT_TANH, a_tiles=pl.z1_tiles)

    def scorer_dgrad(self, pl, s):
        # ... and the scale of the gradient at the CAR tanh from the Cauchy-Schwarz bound of dS1 Ws1^T: max row norm of dS1 x max row norm of Ws1
        P3Rows.scorer_dgrad(self, pl, s)
        check(self.rt.lib.cham_h2_scale_rownorm2(ptr(pl.dS1), pl.PC, pl.dS1.shape[1], pl.dS1.shape[1], self.rt.sc_ws1n.data_ptr() + 8, ptr(pl.sc_dz2),
                                                 ptr(pl.sc_ds1), s), "cham_h2_scale_rownorm2")

    def dz2(self, pl, s):
        rt, lib, C, P, R, f16 = self.rt, self.rt.lib, pl.C, pl.P, pl.PC, self.rt.dm_f16
        Z2c = pl.Z2[P:P + R]
        if not self.fused_dz2(pl):
            return check(lib.cham_mulpred_bwd_h2(ptr(pl.dZ2[P:P + R]), ptr(Z2c), ptr(pl.pred), C, P, pl.N, ptr(pl.dpred), ptr(pl.dZ2p), pl.dz2_ps, ptr(pl.b2part),
                                                 ptr(pl.sc_dz2), s), "cham_mulpred_bwd_h2")
        with self.dm_timed(pl, bf16=False, h2out=True, f16p=bool(f16)):
            if pl.dz2_tiles:      # ... with the planes of dZ2 written tile-blocked (ds1 / w scale records: the kernel's own products on two fp16 planes too)
                check(lib.cham_dm_mulpred_h2_blk(ptr(pl.dS1), 128, 128, ptr(rt.ws1h if f16 else rt.ws1p), C * 128, ptr(pl.sc_ds1) if f16 else None,
                                                 ptr(rt.sc_ws1n) if f16 else None, ptr(Z2c), ptr(pl.pred), C, P, pl.N, ptr(pl.dZ2p), pl.dz2_ps, ptr(pl.sc_dz2),
                                                 ptr(pl.dpred), ptr(pl.b2part), s), "cham_dm_mulpred_h2_blk")
            elif f16:             # the kernel's own products on two fp16 planes too
                check(lib.cham_dm_mulpred_h2h(ptr(pl.dS1), 128, 128, ptr(rt.ws1h), C * 128, ptr(pl.sc_ds1), ptr(rt.sc_ws1n), ptr(Z2c), ptr(pl.pred),
                                              C, P, pl.N, ptr(pl.dZ2p), pl.dz2_ps, ptr(pl.sc_dz2), ptr(pl.dpred), ptr(pl.b2part), s), "cham_dm_mulpred_h2h")
            else:
                check(lib.cham_dm_mulpred_h2(ptr(pl.dS1), 128, 128, ptr(rt.ws1p), C * 128, ptr(Z2c), ptr(pl.pred), C, P, pl.N, ptr(pl.dZ2p), pl.dz2_ps,
                                             ptr(pl.sc_dz2), ptr(pl.dpred), ptr(pl.b2part), s), "cham_dm_mulpred_h2")

    def cosine_bwd(self, pl, s):
        # ... as two fp16 planes + this click's share of the b2 gradient; the scale record from max_r |ds_r| rz_r, which bounds every element
        # (csrc/cosine.hip k_cosine_bound: |p^_k - cos z^_k| <= 1)
        lib, P, R = self.rt.lib, pl.P, pl.PC
        check(lib.cham_cosine_bound(ptr(pl.ds), ptr(pl.rz), R, ptr(pl.cos_t), s), "cham_cosine_bound")
        check(lib.cham_h2_scale_absmax(ptr(pl.cos_t), (R + 3) & ~3, None, 0, ptr(pl.sc_dz2), s), "cham_h2_scale_absmax")
        check(lib.cham_cosine_bwd_h2(ptr(pl.Z2[P:P + R]), ptr(pl.pred), ptr(pl.ds), ptr(pl.rz), ptr(pl.rp), ptr(pl.cosq), ptr(pl.mask), pl.C, P, pl.N,
                                     ptr(pl.dZ2p), pl.dz2_ps, ptr(pl.sc_dz2), ptr(pl.dpred), ptr(pl.b2part), s), "cham_cosine_bwd_h2")

    def car_dgrad(self, pl):
        rt, C = self.rt, pl.C
        rt.gemm_h2(pl.dZ2p, pl.dz2_ps, C, pl.sc_dz2, rt.w2p, C * C, C, rt.sc_w2, 0, pl.dZ1[pl.P:], C, pl.PC, C, C, dref_h=pl.Z1p, ldr=C, dact=ACT_LEAKY,
                   a_tiles=pl.dz2_tiles, dref_blocked=1 if pl.z1_tiles else 0, group_rows=pl.NC, groupsum=pl.gsum)

    def w2_wgrad_cand(self, pl, splits):
        self.rt.gemm_h2(pl.Z1p, pl.z1_ps, pl.C, pl.sc_z1, pl.dZ2p, pl.dz2_ps, pl.C, pl.sc_dz2, 1, self.rt.g('W2'), pl.C, pl.C, pl.C, pl.PC, splits=splits,
                        a_tiles=pl.z1_tiles, b_tiles=pl.dz2_tiles)

    def combine_bwd(self, pl, ws, st):
        if pl.gsum is None:
            return P3Rows.combine_bwd(self, pl, ws, st)
        # dU from the group sums of the CAR dgrad's epilogue
        check(self.rt.lib.cham_combine_bwd_gs(ptr(pl.dZ1), pl.C, pl.P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.dU), ptr(pl.dV), ptr(ws), ws.numel() * 4,
                                              ptr(pl.gsum), pl.gsum.numel() * 4, st), "cham_combine_bwd_gs")


class Bf16Rows(F32Rows):
    """bf16 configuration: the candidate-row matrices (Z1c, Z2c, Mc, S1-S3 and their gradients) are bf16 in HBM, fp32 accumulation."""
    # Weights go through bf16 shadows (plain + transposed: csrc/gemm_b16.hip wants both operands k-contiguous - W^T forward, W dgrad); the
    # clicked-input rows stay fp32 (they feed / come from the fp32 recurrent branch)
    b16 = True
    softmax_fwd, softmax_bwd = 'cham_score_softmax_fwd_b16', 'cham_score_softmax_bwd_b16'
    rankloss_fwd, rankloss_bwd = 'cham_score_rankloss_fwd_b16', 'cham_score_rankloss_bwd_b16'
    diversity_bwd = 'cham_diversity_bwd_b16'
    SHADOWED = ('W2', 'Ws1', 'Ws2', 'Ws3')

    def __init__(self, rt):
        self.rt = rt
        if rt.layout.C % 128:
            raise ValueError("gemm_dtype='bf16' needs CAR_embedding_size % 128 == 0")
        if rt.cosine:      # no scorer weights
            self.SHADOWED = ('W2',)
        for name in self.SHADOWED:
            r, c = rt.layout.entries[name].shape
            rt.shadow[name] = torch.zeros(r, c, dtype=torch.bfloat16, device=rt.device)
            rt.shadow[name + 'T'] = torch.zeros(c, r, dtype=torch.bfloat16, device=rt.device)

    def refresh_shadows(self, s):
        rt = self.rt
        for name in self.SHADOWED:
            r, c = rt.layout.entries[name].shape
            check(rt.lib.cham_cast_b16(ptr(rt.p(name)), r, c, ptr(rt.shadow[name]), ptr(rt.shadow[name + 'T']), s), "cham_cast_b16")

    def alloc(self, pl, f32):
        pl.Z1, pl.Z2, pl.dZ2, pl.dZ1 = (f32(pl.BT, pl.C) for _ in range(4))
        pl.Z1c, pl.Z2c, pl.dZ2c, pl.dZ1c = (torch.empty(pl.Rc, pl.C, dtype=torch.bfloat16, device=self.rt.device) for _ in range(4))
        if not self.rt.cosine:      # cand (.) pred, the operand of the MLP head's first layer
            pl.Mc = torch.empty(pl.Rc, pl.C, dtype=torch.bfloat16, device=self.rt.device)
        pl.b2part = f32(pl.BT, pl.C)

    def cand_Z1(self, pl, P, n):
        return pl.Z1c[:n].float()

    def fused_dz2(self, pl):
        return self.rt.dm_fused_b16 and 32 <= pl.NC <= 256

    def z1(self, pl, s, drop):
        rt, C, P, R = self.rt, pl.C, pl.P, pl.PC
        if drop:      # dense PreCAR rows (masks differ per occurrence): bf16-rounded operands, fp32 out, stored as the bf16-resident Z1c
            rt.gemm(pl.Xd[P:], drop.W1, pl.Z1f[P:], R, C, drop.Fw, drop.Fw, C, C, bias=rt.p('b1'), act=ACT_LEAKY)
            check(rt.lib.cham_cast_b16(pl.Z1f[P:].data_ptr(), R, C, ptr(pl.Z1c), None, s), "cham_cast_b16")
        else:
            check(rt.lib.cham_combine_fwd_b16(ptr(pl.U), ptr(pl.V), C, P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.Z1c), s), "cham_combine_fwd_b16")

    def car_fwd(self, pl):
        rt, C = self.rt, pl.C
        rt.gemm_b16(pl.Z1c, C, 0, rt.shadow['W2T'], C, 1, pl.Z2c, C, 0, pl.PC, C, C, bias=rt.p('b2'), act=ACT_TANH, dma=rt.b16_dma)

    def scorer_fwd(self, pl, s):
        rt, p, sh, C, R = self.rt, self.rt.p, self.rt.shadow, pl.C, pl.PC
        check(rt.lib.cham_mul_rows_b16(ptr(pl.Z2c), ptr(pl.pred), C, pl.P, pl.NC, ptr(pl.Mc), s), "cham_mul_rows_b16")
        rt.gemm_b16(pl.Mc, C, 0, sh['Ws1T'], C, 1, pl.S1, 128, 0, R, 128, C, bias=p('bs1'), act=ACT_LEAKY)
        rt.gemm_b16(pl.S1, 128, 0, sh['Ws2T'], 128, 1, pl.S2, 64, 0, R, 64, 128, bias=p('bs2'), act=ACT_LEAKY)
        rt.gemm_b16(pl.S2, 64, 0, sh['Ws3T'], 64, 1, pl.S3, 32, 0, R, 32, 64, bias=p('bs3'), act=ACT_LEAKY)

    def scorer_dgrad(self, pl, s):
        rt, sh, R = self.rt, self.rt.shadow, pl.PC
        rt.gemm_b16(pl.dS3, 32, 0, sh['Ws3'], 32, 1, pl.dS2, 64, 0, R, 64, 32, dref=pl.S2, ldr=64, dact=ACT_LEAKY)
        rt.gemm_b16(pl.dS2, 64, 0, sh['Ws2'], 64, 1, pl.dS1, 128, 0, R, 128, 64, dref=pl.S1, ldr=128, dact=ACT_LEAKY)

    def s1_wgrad(self, pl):      # weight gradients: activations^T x gradients, both bf16 [rows, *] (TN through the LDS transpose read)
        self.rt.gemm_b16(pl.Mc, pl.C, 1, pl.dS1, 128, 0, self.rt.g('Ws1'), 128, 1, pl.C, 128, pl.PC, splits=0)
        self.rt.colsum(pl.dS1, 128, pl.PC, 128, self.rt.g('bs1'), b16=True)

    def s1_dgrad(self, pl):
        self.rt.gemm_b16(pl.dS1, 128, 0, self.rt.shadow['Ws1'], 128, 1, pl.dZ2c[:pl.PC], pl.C, 0, pl.PC, pl.C, 128)

    def dz2(self, pl, s):      # fused: the same fusion as the plane arms over single bf16 matrices (dM rounded to bf16 where the pair stores it)
        rt, C, P, R = self.rt, pl.C, pl.P, pl.PC
        Z2c, dZ2c = pl.Z2c[:R], pl.dZ2c[:R]
        if not self.fused_dz2(pl):
            return check(rt.lib.cham_mulpred_bwd_b16(ptr(dZ2c), ptr(Z2c), ptr(pl.pred), C, P, pl.N, ptr(pl.dpred), s), "cham_mulpred_bwd")
        with self.dm_timed(pl, bf16=True):
            check(rt.lib.cham_dm_mulpred_b16(ptr(pl.dS1), 128, 128, ptr(rt.shadow['Ws1']), ptr(Z2c), ptr(pl.pred), C, P, pl.N, ptr(dZ2c), ptr(pl.dpred),
                                             ptr(pl.b2part), s), "cham_dm_mulpred_b16")

    def cosine_fwd(self, pl, s):      # (the cosine itself is fp32: it is never rounded to bf16)
        C = pl.C
        check(self.rt.lib.cham_cosine_fwd_b16(ptr(pl.Z2c), C, ptr(pl.pred), C, pl.P, pl.N, ptr(pl.cosq), ptr(pl.rz), ptr(pl.rp), s), "cham_cosine_fwd_b16")

    def cosine_bwd(self, pl, s):
        check(self.rt.lib.cham_cosine_bwd_b16(ptr(pl.Z2c), ptr(pl.pred), ptr(pl.ds), ptr(pl.rz), ptr(pl.rp), ptr(pl.cosq), ptr(pl.mask), pl.C, pl.P, pl.N,
                                              ptr(pl.dZ2c), ptr(pl.dpred), ptr(pl.b2part), s), "cham_cosine_bwd_b16")

    def car_dgrad(self, pl):
        rt, C = self.rt, pl.C
        rt.gemm_b16(pl.dZ2c[:pl.PC], C, 0, rt.shadow['W2'], C, 1, pl.dZ1c, C, 0, pl.PC, C, C, dref=pl.Z1c, ldr=C, dact=ACT_LEAKY, dma=rt.b16_dma)

    def w2_wgrad(self, pl, splits=0, cand=True):      # the candidate rows (bf16, TN) + the clicked-input rows (fp32)
        rt, C = self.rt, pl.C
        rt.gemm_b16(pl.Z1c, C, 1, pl.dZ2c[:pl.PC], C, 0, rt.g('W2'), C, 1, C, C, pl.PC, splits=0, dma=rt.b16_dma)
        rt.gemm(pl.Z1, pl.dZ2, rt.g('W2'), C, C, pl.P, C, C, C, transA=1, splits=0, accumulate=1)

    def b2_grad(self, pl):
        rt, C = self.rt, pl.C
        if self.fused_dz2(pl) or rt.cosine:      # the per-position sums of the stored gradient rows, written by the fused kernel / the cosine backward
            rt.colsum(pl.b2part, C, pl.P, C, rt.g('b2'))
        else:
            rt.colsum(pl.dZ2c[:pl.PC], C, pl.PC, C, rt.g('b2'), b16=True)
        rt.colsum(pl.dZ2, C, pl.P, C, rt.g('b2'), accumulate=1)

    def dense_dZ1(self, pl, st):      # fp32 image of [clicked rows (fp32) ; candidate rows (bf16-resident)]
        pl.dZ1f[:pl.P].copy_(pl.dZ1[:pl.P])
        check(self.rt.lib.cham_upcast_b16(ptr(pl.dZ1c), pl.PC * pl.C, pl.dZ1f[pl.P:].data_ptr(), st), "cham_upcast_b16")
        return pl.dZ1f

    def combine_bwd(self, pl, ws, st):
        check(self.rt.lib.cham_combine_bwd_b16(ptr(pl.dZ1), ptr(pl.dZ1c), pl.C, pl.P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.dU), ptr(pl.dV), ptr(ws),
                                               ws.numel() * 4, st), "cham_combine_bwd_b16")
