"""Float64 references, exact-sum input builders and slips of the backward path between the scorer's first layer and the feature tables, for
tests/test_backward_reference_cpu.py and tests/test_backward_exact_gpu.py.  numpy only: neither torch nor the library is imported here.

  fused scorer dgrad (csrc/dm_fused.hip, five entry points; the formulas of its header)
      dM[r, c]    = sum_k dS1[r, k] Ws1[c, k]                         K = 128
      dZ2[r, c]   = dM[r, c] * pred[p(r), c] * (1 - Z2[r, c]^2)       p(r) = r // (1 + N)
      dpred[p, c] = (sum_{r in p} dM[r, c] Z2[r, c]) * (1 - pred[p, c]^2)
      b2part[p,c] = sum_{r in p} dZ2[r, c]
  combine backward (csrc/scorer.hip; include/chameleon_nar.h)
      dU[bt] = dpre[bt] + sum_c dpre[cand (bt, c)];  dV[bt] = dpre[bt];  dV[BT + bt] = dpre[cand (bt, 0)];
      dV[2 BT + s] += dpre[cand (bt, 1 + n)] for every slot[bt, n] = s in [0, pmax] (pmax = the pad slot; -1 = masked: nowhere)
      group sums: groupsum[(q * (127 // G + 2) + k) * C + column] = the column sums of the rows of group (128 q) // G + k inside 128-row chunk q
  feature backward (csrc/features.hip):  dgamma[c] = sum_r dxs[r, c] xraw[r, c],  dbeta[c] = sum_r dxs[r, c]

EXACT-SUM inputs.  All operands are small integers times powers of two, so every fp32 product and every fp32 partial sum is exact in any
order and a kernel has to give the float64 value bit for bit (tests/test_backward_reference_cpu.py evaluates every case in fp32 in two
orders).  The widest sums, in units of the smallest term:
  * dM: |dS1| <= 3 (integers, at most DM_NNZ = 8 non-zeros per row), |Ws1| in {0, 0.5, 1, 2}: |dM| <= 8 * 3 * 2 = 48 in units of 0.5 - 7 bits;
  * dZ2 = dM * pred * (1 - Z2^2) with pred, Z2 in {0, +-0.5, +-1} (1 - x^2 in {1, 0.75, 0}): units of 0.5 * 0.5 * 0.25 = 1/16, |dZ2| <= 48
    - 10 bits: the h plane of two fp16 planes (11 bits) and two of the three bf16 planes (8 + 8) hold it whole;
  * b2part: 256 rows of a position, 256 * 48 * 16 < 2^18;  dpred: dM Z2 in units of 0.25, 256 rows, x (1 - pred^2) in units of 1/4:
    256 * 48 * 16 < 2^18;
  * the bf16 twin: ONE non-zero per row of dS1, so dM = dS1 * Ws1 (2 + 2 bits) and dZ2 (x 9 / 16 at most: 6 bits) are bf16 values and both
    roundings of the kernel are the identity;
  * combine: integer dpre in [-8, 8]; the pad slot is held by at most 1025 * 255 entries: 8 * 261 375 < 2^21; a hot slot by 1025 positions;
  * feature backward: dxs integers in [-8, 8], xraw in {0.5, 1, 2, -1}: units of 0.5, R <= 2049 rows: 2049 * 8 * 2 * 2 < 2^17.
All far below 2^24.

Every reference takes keyword SLIPS, the mistakes the kernels' structure invites; the CPU file shows that each changes an output."""
import functools
import os
import re

import numpy as np

from tests import gemm_reference as G
from tests.tail_reference import same_bits                      # noqa: F401  (re-exported: B.same_bits)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@functools.lru_cache(maxsize=None)
def kernel_constants():
    """The chunk sizes, read from the kernels' sources: SLOT_HOT (positions per chunk of a hot slot), SLOT_LIST (entries per chunk of the
    pad slot's scan), SBW_CHUNKS and the smallest row chunk of cham_feature_bwd_ws."""
    src = lambda f: open(os.path.join(ROOT, "chameleon_recsys_amd", "csrc", f)).read()
    sc, ft = src("scorer.hip"), src("features.hip")
    one = lambda pat, s: int(re.search(pat, s).group(1))
    return dict(slot_hot=one(r"#define SLOT_HOT (\d+)", sc), slot_list=one(r"#define SLOT_LIST (\d+)", sc),
                sbw_chunks=one(r"#define SBW_CHUNKS (\d+)", ft), sbw_min_rows=one(r"if \(rows_per_chunk < (\d+)\) rows_per_chunk = \1;", ft))


def exact32(x):
    """A float64 array of fp32-representable values -> float32 with every zero +0.0 (the sign of a zero is not part of the contract)."""
    x = np.asarray(x)
    y = x.astype(f32)
    assert np.array_equal(y.astype(f64), x.astype(f64)), "not an fp32 value"
    return y + f32(0.0)


def pos_zero(x):
    return np.asarray(x) + np.asarray(x).dtype.type(0.0)


# ---- fused scorer dgrad --------------------------------------------------------------------------------------------------------------------
DM_K = 128
DM_NNZ = 8
DM_NC = (32, 33, 51, 64, 85, 86, 128, 129, 256)                  # 1 + N: PW = 8, 7, 5, 4, 3, 2, 2, 1, 1
DM_C = (64, 128, 192)
DM_SLIPS = ('last_row_dropped', 'row_past_valid_added', 'boundary_off_by_one', 'pred_from_neighbour', 'columns_swapped', 'one_minus_z')


def dm_pw(NC):
    return 256 // NC


def dm_bts(NC):
    PW = dm_pw(NC)
    return sorted({1, PW - 1, PW, PW + 1, 2 * PW + 1} - {0})


def dm_cases():
    return [(NC, BT, C) for NC in DM_NC for BT in dm_bts(NC) for C in DM_C]


_W_VALUES = np.array([0, 0.5, -0.5, 1, -1, 2, -2], f32)
_T_VALUES = np.array([0, 0.5, -0.5, 1, -1], f32)


@functools.lru_cache(maxsize=None)
def dm_inputs(NC, BT, C, b16=False):
    """dS1 [BT NC, 128], Ws1 [C, 128], Z2 [BT NC, C], pred [BT, C] (float32, exact-sum values) and `masked` [BT]: positions whose dS1 rows
    are all zero (BT >= 2: at least one, never all; first, last and middle over the cases), whole rows and single elements of Z2 = +-1, whole
    positions and single elements of pred = 0."""
    rng = np.random.default_rng([NC, BT, C, int(b16)])
    Rc = BT * NC
    nnz = 1 if b16 else DM_NNZ
    dS1 = np.zeros((Rc, DM_K), f32)
    cols = rng.integers(0, DM_K, (Rc, nnz))
    vals = rng.integers(1, 4, (Rc, nnz)) * rng.choice([-1, 1], (Rc, nnz))
    dS1[np.arange(Rc)[:, None], cols] = vals                      # (assignment: a repeated column does not add up)
    masked = (np.arange(BT) + NC + BT) % 4 == 0
    if BT >= 2 and not masked.any():
        masked[BT // 2] = True
    if masked.all():
        masked[0] = False
    dS1[np.repeat(masked, NC)] = 0.0
    Ws1 = rng.choice(_W_VALUES, (C, DM_K))
    Z2 = rng.choice(_T_VALUES, (Rc, C), p=[0.1, 0.3, 0.3, 0.15, 0.15])
    sat = rng.random(Rc) < 0.1
    sat[rng.integers(0, Rc)] = True
    Z2[sat] = rng.choice(np.array([-1, 1], f32), (int(sat.sum()), 1))
    pred = rng.choice(_T_VALUES, (BT, C), p=[0.1, 0.25, 0.25, 0.2, 0.2])
    pz = (rng.random(BT) < 0.2) & (BT >= 3)
    if BT >= 3:
        pz[(BT // 2 + 1) % BT] = True
        pz[np.flatnonzero(~masked)[0]] = False                     # (never every live position)
    pred[pz & ~masked] = 0.0
    out = dict(NC=NC, BT=BT, C=C, b16=b16, dS1=dS1, Ws1=Ws1.astype(f32), Z2=Z2.astype(f32), pred=pred.astype(f32), masked=masked, pred_zero=pz & ~masked)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def _bf16(x, dt):
    return G.bf16_rne(x.astype(f32)).astype(dt)


def dm_reference(inp, dtype=f64, perm_seed=None, **slip):
    """-> dict(dM, dZ2 [BT NC, C], dpred, b2 [BT, C]) in `dtype`: the K products added one k after the other, the rows of a position one
    after the other - in ascending order, or (perm_seed) in a seeded permutation of the k and of the rows.  b16: dM and dZ2 rounded to bf16
    where the kernel rounds them, b2 sums the rounded rows."""
    assert not set(slip) - set(DM_SLIPS), slip
    dt = dtype
    NC, BT, C, b16 = inp['NC'], inp['BT'], inp['C'], inp['b16']
    Rc, PW = BT * NC, dm_pw(NC)
    A, W, Z, P = inp['dS1'].astype(dt), inp['Ws1'].astype(dt), inp['Z2'].astype(dt), inp['pred'].astype(dt)
    rng = np.random.default_rng(perm_seed) if perm_seed is not None else None
    korder = rng.permutation(DM_K) if rng is not None else np.arange(DM_K)
    rorder = rng.permutation(Rc) if rng is not None else np.arange(Rc)
    partial_last = BT % PW != 0
    if slip.get('last_row_dropped') and partial_last:
        A = A.copy()
        A[Rc - 1] = 0
    dM = np.zeros((Rc, C), dt)
    for k in korder:
        dM += A[:, k, None] * W[None, :, k]
    if slip.get('columns_swapped'):
        dM = dM.reshape(Rc, C // 2, 2)[:, :, ::-1].reshape(Rc, C)
    if b16:
        dM = _bf16(dM, dt)
    r = np.arange(Rc)
    owner = r // NC
    if slip.get('boundary_off_by_one'):                           # a position's first row goes to its neighbour (inside a workgroup)
        owner = np.where((r % NC == 0) & (owner % PW != 0), owner - 1, owner)
    psrc = (np.arange(BT) + 1) % BT if slip.get('pred_from_neighbour') else np.arange(BT)
    Pr = P[psrc]
    dz = (dt(1) - Z) if slip.get('one_minus_z') else (dt(1) - Z * Z)
    dZ2 = dM * Pr[owner] * dz
    if b16:
        dZ2 = _bf16(dZ2, dt)
    gz = dM * Z
    s, b2 = np.zeros((BT, C), dt), np.zeros((BT, C), dt)
    for i in rorder:
        s[owner[i]] += gz[i]
        b2[owner[i]] += dZ2[i]
    if slip.get('row_past_valid_added') and partial_last:        # the row behind the last valid one: ones where the tests put NaN
        s[BT - 1] += dt(0.5)
        b2[BT - 1] += Pr[BT - 1] * dt(0.75)
    return dict(dM=dM, dZ2=dZ2, dpred=s * (dt(1) - Pr * Pr), b2=b2)


def dm_scale_bound(inp):
    """The bound cham_h2_scale_rownorm2 records for dZ2's planes: (max row norm of dS1) x (max row norm of Ws1) >= max |dM| >= max |dZ2|."""
    n = lambda X: float(np.sqrt((X.astype(f64) ** 2).sum(1)).max())
    return n(inp['dS1']) * n(inp['Ws1'])


# ---- combine backward ----------------------------------------------------------------------------------------------------------------------
COMBINE_BT = (1, 2, 511, 512, 513, 1025)
COMBINE_N = (1, 2, 31, 50, 255)
COMBINE_SLIPS = ('pad_slot_dropped', 'masked_slot_to_row_0', 'chunk_edge_row_doubled')
GS_SLIPS = ('piece_k_plus_1',)
GS_CASES = ((32, 3), (51, 7), (127, 3), (128, 3), (129, 5), (256, 3))      # (1 + N, BT): BT (1 + N) % 128 != 0 where 1 + N allows it


def combine_cases():
    """(BT, N, pmax, C, plain): the whole BT x N matrix at C = 4 (the smallest width: one float4), pmax handed round 1 / a few / more than
    BT N; C = 68 (not a multiple of 64) on a diagonal; `plain` cases (no masked click, no all-pad click: the hot slot in EVERY position) at
    the chunk size, one above it and two chunks + 1."""
    hot = kernel_constants()['slot_hot']
    assert COMBINE_BT == (1, 2, hot - 1, hot, hot + 1, 2 * hot + 1), "COMBINE_BT no longer brackets SLOT_HOT"
    cases = []
    for i, BT in enumerate(COMBINE_BT):
        for j, N in enumerate(COMBINE_N):
            pmax = (1, N + 3, BT * N + 3)[(i + j) % 3]
            cases.append((BT, N, pmax, 4, False))
            if (i - j) % len(COMBINE_N) == 0 or (BT, N) == (1025, 50):
                cases.append((BT, N, max(N + 3, 40), 68, False))
    for BT in (hot, hot + 1, 2 * hot + 1):
        cases.append((BT, 2, 5, 4, True))
    cases.append((hot + 1, 31, 40, 68, True))
    return cases


@functools.lru_cache(maxsize=None)
def combine_inputs(BT, N, pmax, C, plain=False):
    """slot [BT, N] int32 and dpre [BT + BT (N + 1), C] float32 (integers in [-8, 8]).  Slot 0 sits in every click that holds a real slot;
    the other real slots of a click are distinct (a click holds a pool slot at most once: k_click_select); slot pmax - 1 is used once;
    a random tail of every other click is the pad slot pmax, one click holds it N times; masked clicks (slot -1: first, last and middle)
    carry zero gradient - except ONE, whose candidate rows are not zero: they count in dU and must reach no row of dV."""
    rng = np.random.default_rng([BT, N, pmax, C, int(plain)])
    nother = max(pmax - 2, 0)
    j = np.arange(N)[None, :]
    p = np.arange(BT)[:, None]
    slot = np.where(j == 0, 0, 1 + (p * N + j - 1) % max(nother, 1)).astype(np.int64)
    kmax = 1 + min(N - 1, nother)
    k = np.full(BT, kmax)
    if not plain:
        short = rng.random(BT) < 0.5
        k[short] = rng.integers(1, kmax + 1, int(short.sum()))
    slot[j >= k[:, None]] = pmax
    allpad = cold = -1
    masked = np.zeros(BT, bool)
    if not plain:
        if BT >= 3:
            masked[[0, BT - 1, BT // 2]] = True
        elif BT == 2:
            masked[1] = True
        free = np.flatnonzero(~masked)
        if len(free) >= 2:
            allpad = int(free[len(free) // 3])
            slot[allpad] = pmax
    free = np.flatnonzero(~masked & (np.arange(BT) != allpad))
    if pmax >= 2 and N >= 2 and len(free):
        cold = int(free[-1])
        slot[cold, N - 1] = pmax - 1
    slot = rng.permuted(slot, axis=1)
    slot[masked] = -1
    NC = N + 1
    dpre = rng.integers(-8, 9, (BT + BT * NC, C)).astype(f32)
    loud = int(np.flatnonzero(masked)[-1]) if masked.any() else -1
    for m in np.flatnonzero(masked):
        dpre[m] = 0.0
        if m != loud:
            dpre[BT + m * NC:BT + (m + 1) * NC] = 0.0
    slot = slot.astype(np.int32)
    slot.setflags(write=False), dpre.setflags(write=False)
    return dict(BT=BT, N=N, pmax=pmax, C=C, slot=slot, dpre=dpre, masked=masked, allpad=allpad, cold=cold, loud=loud)


def combine_reference(inp, dtype=f64, perm_seed=None, **slip):
    """-> dU [BT, C], dV [2 BT + pmax + 1, C] by np.add.at over the slot entries (ascending, or in a seeded permutation)."""
    assert not set(slip) - set(COMBINE_SLIPS), slip
    BT, N, pmax, C = inp['BT'], inp['N'], inp['pmax'], inp['C']
    NC = N + 1
    dpre = inp['dpre'].astype(dtype)
    cand = dpre[BT:].reshape(BT, NC, C)
    rng = np.random.default_rng(perm_seed) if perm_seed is not None else None
    dU = dpre[:BT].copy()
    for c in (rng.permutation(NC) if rng is not None else range(NC)):
        dU += cand[:, c]
    dV = np.zeros((2 * BT + pmax + 1, C), dtype)
    dV[:BT] = dpre[:BT]
    dV[BT:2 * BT] = cand[:, 0]
    s = inp['slot'].reshape(-1).astype(np.int64)
    rows = cand[:, 1:].reshape(-1, C)
    idx = np.arange(len(s))
    if slip.get('masked_slot_to_row_0'):
        s = np.where(s < 0, 0, s)
    if slip.get('pad_slot_dropped'):
        idx = idx[s[idx] != pmax]
    if slip.get('chunk_edge_row_doubled'):                        # the first position of a later chunk of a hot slot counted by both chunks
        pos = idx // N
        hot = kernel_constants()['slot_hot']
        idx = np.concatenate([idx, idx[(pos % hot == 0) & (pos > 0) & (s[idx] >= 0) & (s[idx] < pmax)]])
    idx = idx[s[idx] >= 0]
    if rng is not None:
        idx = rng.permutation(idx)
    np.add.at(dV, 2 * BT + s[idx], rows[idx])
    return dU, dV


def group_sums(cand_rows, G_):
    """The group-sum array of include/chameleon_nar.h for M = len(cand_rows) rows in groups of G_ consecutive rows: [2 ceil(M / 256) x
    (127 // G_ + 2), C]; the pieces no row falls into are NaN."""
    M, C = cand_rows.shape
    gsk = 127 // G_ + 2
    out = np.full((2 * (-(-M // 256)) * gsk, C), np.nan, cand_rows.dtype)
    for q in range(-(-M // 128)):
        lo, hi = 128 * q, min(128 * q + 128, M)
        g0 = lo // G_
        for g in range(g0, (hi - 1) // G_ + 1):
            out[q * gsk + (g - g0)] = cand_rows[max(lo, g * G_):min(hi, (g + 1) * G_)].sum(0)
    return out


def du_from_group_sums(dpre_in, gsum, BT, N, **slip):
    """dU[bt] = dpre[bt] + the pieces of group bt in chunk order."""
    assert not set(slip) - set(GS_SLIPS), slip
    G_ = N + 1
    gsk = 127 // G_ + 2
    dU = dpre_in.copy()
    for bt in range(BT):
        for q in range((bt * G_) >> 7, ((bt + 1) * G_ - 1 >> 7) + 1):
            k = bt - (128 * q) // G_ + (1 if slip.get('piece_k_plus_1') else 0)
            dU[bt] += gsum[q * gsk + k]
    return dU


# ---- feature backward ----------------------------------------------------------------------------------------------------------------------
FEATURE_F = (4, 60, 64, 68, 1024)
FEATURE_SLIPS = ('chunk_edge_row_dropped',)
_X_VALUES = np.array([0.5, 1, 2, -1], f32)


def feature_rows_per_chunk(R):
    k = kernel_constants()
    return max(-(-R // k['sbw_chunks']), k['sbw_min_rows'])


def feature_rs():
    """1, 63, 64, 65; both sides of a row-chunk edge at the smallest chunk (m: m - 1, m, m + 1 rows, and two chunks + 1) and where the
    chunk grows by a row (CHUNKS x m and one more: chunks of m + 1 rows, the last one short)."""
    k = kernel_constants()
    m, ch = k['sbw_min_rows'], k['sbw_chunks']
    return tuple(sorted({1, 63, 64, 65, m - 1, m, m + 1, 2 * m + 1, ch * m, ch * m + 1}))


def feature_cases():
    rs = feature_rs()
    return [(R, F) for R in rs for F in FEATURE_F if R <= 129 or F in (4, 68)] + [(rs[-1], 1024)]


@functools.lru_cache(maxsize=None)
def feature_inputs(R, F):
    rng = np.random.default_rng([R, F])
    dxs = rng.integers(-8, 9, (R, F)).astype(f32)
    xraw = rng.choice(_X_VALUES, (R, F))
    dxs.setflags(write=False), xraw.setflags(write=False)
    return dxs, xraw


def feature_reference(dxs, xraw, dtype=f64, perm_seed=None, **slip):
    assert not set(slip) - set(FEATURE_SLIPS), slip
    R = len(dxs)
    g, x = dxs.astype(dtype), xraw.astype(dtype)
    rows = np.arange(R)
    if slip.get('chunk_edge_row_dropped'):
        m = feature_rows_per_chunk(R)
        rows = rows[(rows % m != 0) | (rows == 0)]
    if perm_seed is not None:
        rows = np.random.default_rng(perm_seed).permutation(rows)
    dg, db = np.zeros(dxs.shape[1], dtype), np.zeros(dxs.shape[1], dtype)
    for r in rows:
        dg += g[r] * x[r]
        db += g[r]
    return dg, db


SLIPS = DM_SLIPS + COMBINE_SLIPS + GS_SLIPS + FEATURE_SLIPS


# ---- the random-data cases: per-element bounds ------------------------------------------------------------------------------------------------
MARGIN = G.MARGIN
DM_RANDOM = (51, 7, 128)                                           # (1 + N, BT, C)


@functools.lru_cache(maxsize=None)
def dm_random_inputs():
    NC, BT, C = DM_RANDOM
    rng = np.random.default_rng(51)
    n = lambda *s: rng.standard_normal(s).astype(f32)
    return dict(NC=NC, BT=BT, C=C, dS1=n(BT * NC, DM_K), Ws1=n(C, DM_K) * f32(0.1), Z2=np.tanh(n(BT * NC, C)), pred=np.tanh(n(BT, C)))


def dm_random_reference(inp, form, sa=1.0, sw=1.0):
    """-> (ref, S, bound, extra) dicts over 'dZ2', 'dpred', 'b2' for one form of the fused dgrad on Gaussian operands.  As tests/gemm_reference.py:
    ref is the float64 sum of exactly the plane products the form makes (six of three bf16 planes; three of two fp16 planes under the scales
    sa, sw for 'h2h'), S the same expression with |.| for every term (1 + x^2 for 1 - x^2), and bound = 8 e with e the worst |twin - ref| / S
    of an fp32 evaluation that adds one term after the other; extra = what is allowed on top of bound x S (zero here).  'b16': dm_random_b16."""
    NC, BT, C = inp['NC'], inp['BT'], inp['C']
    Rc = BT * NC
    if form == 'b16':
        return dm_random_b16(inp)
    if form == 'h2h':
        A = [X.astype(f32) for X in G.split2h(inp['dS1'], sa, keep_sign=False)]
        W = [X.astype(f32) for X in G.split2h(inp['Ws1'], sw)]
        Z, products, inv = inp['Z2'], G.H2_PRODUCTS, 1.0 / (sa * sw)
    else:
        A, W, Z, products, inv = list(G.split3(inp['dS1'])), list(G.split3(inp['Ws1'])), inp['Z2'], G.P3_PRODUCTS, 1.0
    P = inp['pred']

    def chain(dt):
        dM, SM = np.zeros((Rc, C), dt), np.zeros((Rc, C), dt)
        Ad, Wd = [X.astype(dt) for X in A], [X.astype(dt) for X in W]
        for k in range(DM_K):
            for qa, qb in products:
                t = Ad[qa][:, k, None] * Wd[qb][None, :, k]
                dM += t
                SM += np.abs(t)
        dM, SM = dM * dt(inv), SM * dt(inv)
        z, p = Z.astype(dt), np.repeat(P.astype(dt), NC, 0)
        o = dM * p * (dt(1) - z * z)
        So = SM * np.abs(p) * (dt(1) + z * z)
        gz, Sgz = dM * z, SM * np.abs(z)
        s, b2, Ss, Sb = (np.zeros((BT, C), dt) for _ in range(4))
        for c in range(NC):
            s += gz[c::NC]; b2 += o[c::NC]; Ss += Sgz[c::NC]; Sb += So[c::NC]
        pp = P.astype(dt)
        return dict(dZ2=o, dpred=s * (dt(1) - pp * pp), b2=b2), dict(dZ2=So, dpred=Ss * (dt(1) + pp * pp), b2=Sb)
    ref, S = chain(f64)
    twin = chain(f32)[0]
    bound, extra = {}, {}
    for k in ref:
        with np.errstate(invalid='ignore', divide='ignore'):
            e = np.where(S[k] > 0, np.abs(twin[k].astype(f64) - ref[k]) / S[k], 0.0)
        bound[k] = MARGIN * float(e.max())
        extra[k] = np.zeros_like(ref[k])
    return ref, S, bound, extra


def ratio(got, ref, S, extra=0.0):
    """max over the elements of (|got - ref| - extra) / S; a NaN counts as infinite."""
    got = np.asarray(got, f64)
    err = np.abs(got - ref) - extra
    with np.errstate(invalid='ignore', divide='ignore'):
        r = np.where(np.isnan(got), np.inf, np.where(err > 0, err / S, 0.0))
    return float(r.max())


COMBINE_RANDOM = (37, 50, 200, 64)                                 # (BT, N, pmax, C)
FEATURE_RANDOM = (300, 100)                                        # (R, F)


def _bound(twin, ref, S):
    with np.errstate(invalid='ignore', divide='ignore'):
        e = np.where(S > 0, np.abs(twin.astype(f64) - ref) / S, 0.0)
    return MARGIN * float(e.max())


@functools.lru_cache(maxsize=None)
def combine_random_inputs():
    """The slot table of the exact case of the same shape under Gaussian gradients: `f32` (all rows fp32) and `b16` (the candidate rows as
    the bf16 values the bf16 entry point reads)."""
    BT, N, pmax, C = COMBINE_RANDOM
    base = combine_inputs(BT, N, pmax, C)
    dpre = np.random.default_rng(37).standard_normal(base['dpre'].shape).astype(f32)
    dpre[base['dpre'] == 0] *= f32(base['loud'] < 0)              # (zero rows of the masked clicks stay zero)
    for m in np.flatnonzero(base['masked']):
        dpre[m] = 0.0
        if m != base['loud']:
            dpre[BT + m * (N + 1):BT + (m + 1) * (N + 1)] = 0.0
    d16 = dpre.copy()
    d16[BT:] = G.bf16_rne(dpre[BT:])
    return dict(base, dpre=dpre), dict(base, dpre=d16)


@functools.lru_cache(maxsize=None)
def combine_random_reference():
    """name -> ((dU, dV) float64, (S_dU, S_dV), (bound_dU, bound_dV)) for 'f32', 'b16' and 'gs' (dU = dpre + the group-sum pieces as STORED,
    i.e. the float64 sums rounded to fp32 by the host that builds the array)."""
    BT, N, pmax, C = COMBINE_RANDOM
    out = {}
    for name, inp in zip(('f32', 'b16'), combine_random_inputs()):
        ref = combine_reference(inp)
        S = combine_reference(dict(inp, dpre=np.abs(inp['dpre'])))
        twin = combine_reference(inp, dtype=f32)
        out[name] = (ref, S, tuple(_bound(t, r, s) for t, r, s in zip(twin, ref, S)))
    inp = combine_random_inputs()[0]
    gs = group_sums(inp['dpre'][BT:].astype(f64), N + 1).astype(f32)
    dU = du_from_group_sums(inp['dpre'][:BT].astype(f64), gs.astype(f64), BT, N)
    SU = du_from_group_sums(np.abs(inp['dpre'][:BT]).astype(f64), np.abs(gs).astype(f64), BT, N)
    tU = du_from_group_sums(inp['dpre'][:BT], gs, BT, N)
    (_, dV), (_, SV), (_, bV) = out['f32']
    out['gs'] = ((dU, dV), (SU, SV), (_bound(tU, dU, SU), bV))
    return out


@functools.lru_cache(maxsize=None)
def feature_random_inputs():
    rng = np.random.default_rng(300)
    return rng.standard_normal(FEATURE_RANDOM).astype(f32), rng.standard_normal(FEATURE_RANDOM).astype(f32)


@functools.lru_cache(maxsize=None)
def feature_random_reference():
    dxs, xraw = feature_random_inputs()
    ref = feature_reference(dxs, xraw)
    S = feature_reference(np.abs(dxs), np.abs(xraw))
    twin = feature_reference(dxs, xraw, dtype=f32)
    return ref, S, tuple(_bound(t, r, s) for t, r, s in zip(twin, ref, S))


def _bf16_boundary_distance(x64, r):
    """Distance of x64 to the nearest rounding boundary of bf16 around its rounded value r (the midpoints to r's two neighbours; the lower
    neighbour of a power of two is half as far)."""
    _, e = np.frexp(r.astype(f64))
    ulp = np.ldexp(1.0, e - 8)
    m, _ = np.frexp(np.abs(r.astype(f64)))
    below = (m == 0.5) & (np.abs(x64) < np.abs(r))
    return np.where(below, ulp / 4, ulp / 2) - np.abs(x64 - r)


def dm_random_b16(inp):
    """The bf16 twin (cham_dm_mulpred_b16) on Gaussian operands rounded to bf16: dM = bf16(sum of the bf16 products), dZ2 = bf16(dM pred
    (1 - Z2^2)), dpred from the rounded dM, b2 from the rounded dZ2 - the reference rounds where the kernel rounds.  An fp32 sum on the
    other side of a rounding boundary moves a stored value by one bf16 ulp (2^-7 of it at most), so an element is SAFE when the float64 dM
    is further than the twin's bound (8 e S) from a boundary and the float64 dZ2 further than 2^-22 |dM pred| (1 + Z2^2) - four fp32
    roundings, contracted or not: there the kernel must store the reference's bits, extra['bits'] where extra['safe'].  Elsewhere dZ2 gets
    two ulps (2^-6 |dZ2|); the sums get one ulp of each unsafe row's term on top of 8 e S."""
    NC, BT, C = inp['NC'], inp['BT'], inp['C']
    Rc = BT * NC
    A, W, Z, P = G.bf16_rne(inp['dS1']), G.bf16_rne(inp['Ws1']), G.bf16_rne(inp['Z2']), inp['pred']

    def gemm(dt):
        dM, SM = np.zeros((Rc, C), dt), np.zeros((Rc, C), dt)
        Ad, Wd = A.astype(dt), W.astype(dt)
        for k in range(DM_K):
            t = Ad[:, k, None] * Wd[None, :, k]
            dM += t
            SM += np.abs(t)
        return dM, SM
    dM64, SM = gemm(f64)
    dM32, _ = gemm(f32)
    with np.errstate(invalid='ignore', divide='ignore'):
        bound_m = MARGIN * float(np.where(SM > 0, np.abs(dM32.astype(f64) - dM64) / SM, 0.0).max())
    g = G.bf16_rne(dM64.astype(f32))
    unsafe_m = _bf16_boundary_distance(dM64, g) <= bound_m * SM

    def tail(g_, dt):
        z, p = Z.astype(dt), np.repeat(P.astype(dt), NC, 0)
        o_pre = g_.astype(dt) * p * (dt(1) - z * z)
        o = G.bf16_rne(o_pre.astype(f32)).astype(dt)
        gz = g_.astype(dt) * z
        s, b2 = np.zeros((BT, C), dt), np.zeros((BT, C), dt)
        for c in range(NC):
            s += gz[c::NC]; b2 += o[c::NC]
        pp = P.astype(dt)
        return o_pre, o, gz, s * (dt(1) - pp * pp), b2
    o_pre, o, gz, dpred, b2 = tail(g, f64)
    z64, p64 = Z.astype(f64), np.repeat(P.astype(f64), NC, 0)
    unsafe_o = _bf16_boundary_distance(o_pre, o) <= 2.0 ** -22 * np.abs(g.astype(f64) * p64) * (1 + z64 * z64)
    unsafe = unsafe_m | unsafe_o
    pos = lambda X: X.reshape(BT, NC, C).sum(1)
    pp = P.astype(f64)
    ref = dict(dZ2=o, dpred=dpred, b2=b2)
    S = dict(dZ2=np.abs(o) + (o == 0), dpred=pos(np.abs(gz)) * (1 + pp * pp), b2=pos(np.abs(o)))
    ulp = 2.0 ** -7
    extra = dict(dZ2=np.where(unsafe, 2 * ulp * (1 + ulp) * np.abs(o), 0.0), dpred=pos(np.where(unsafe_m, ulp * np.abs(gz), 0.0)) * (1 + pp * pp),
                 b2=pos(np.where(unsafe, 2 * ulp * (1 + ulp) * np.abs(o), 0.0)))
    _, o32, _, dpred32, b232 = tail(G.bf16_rne(dM32), f32)
    twin = dict(dZ2=o32, dpred=dpred32, b2=b232)
    bound = {}
    for k in ref:
        err = np.abs(twin[k].astype(f64) - ref[k]) - extra[k]
        with np.errstate(invalid='ignore', divide='ignore'):
            bound[k] = MARGIN * float(np.where((err > 0) & (S[k] > 0), err / S[k], 0.0).max())
    # (the twin's b2 is exact: bf16 terms, one order.  Another order may round once - an fp32 sum is not held below one rounding, 2^-24 S)
    bound['b2'] = max(bound['b2'], MARGIN * 2.0 ** -24)
    extra['safe'], extra['bits'] = ~unsafe, G.bf16_bits(o.astype(f32) + f32(0.0))          # (zeros as +0: 1 - Z2^2 = 0 where bf16 Z2 = +-1)
    return ref, S, bound, extra
