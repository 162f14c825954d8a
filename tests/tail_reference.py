"""float64 numpy references of the scorer tail (csrc/scorer.hip from cham_mulpred_bwd down) and of the optimizer kernels (csrc/optim.hip),
written from the reference's nar_model.py (:478-517 scores and softmax, :639-683 loss and novelty term, :708-722 Adam, :777-794 ranking,
:1147-1148 novelty of a popularity) and from TF 1.12's AdamOptimizer - not from the kernels and not from oracle/nar_oracle.py.  Inputs
are the fp32 (or bf16-representable fp32) values a kernel gets, widened exactly; everything is evaluated in float64.

Also here, shared by tests/test_tail_reference_cpu.py and the two GPU files so that all three see the same numbers: the input
generators (`softmax_inputs`, `mulpred_inputs`, `adam_inputs`), the case lists, and the error measures."""
import numpy as np

K3 = 32                       # width of the last hidden scorer layer (matching_dense_layer_3)
LEAKY = 0.2                   # tf.nn.leaky_relu's default alpha, nar_model.py:447-473
TINY = np.float32(1.17549435e-38)      # smallest positive normal fp32 (bf16-representable: 2^-126)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- bf16 -------------------------------------------------------------------------------------------------------------------------
def round_bf16_bits(x):
    """uint16 bf16 bit patterns of the fp32 array x, round-to-nearest-even on the bit pattern (integer arithmetic only)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x):
    """x (fp32) rounded to the nearest bf16 value (ties to even), returned as fp32."""
    return bf16_bits_to_f32(round_bf16_bits(x))


def bf16_matches(got_bits, ref64, tol):
    """A bf16 output against round_bf16(ref): (all elements allowed, share of elements that needed the allowance).  Allowed are
    round_bf16(ref) and, where ref lies within `tol` (absolute, array or scalar) of a rounding boundary, the bf16 values from
    round_bf16(ref - tol) to round_bf16(ref + tol)."""
    ref64 = f64(ref64)
    got = f64(bf16_bits_to_f32(got_bits))
    exact = f64(round_bf16(ref64.astype(np.float32)))
    lo, hi = f64(round_bf16((ref64 - tol).astype(np.float32))), f64(round_bf16((ref64 + tol).astype(np.float32)))
    ok = (got == exact) | ((got >= lo) & (got <= hi))
    return bool(ok.all()), float((got != exact).mean()) if got.size else 0.0


# ---- scorer tail ------------------------------------------------------------------------------------------------------------------
def _softmax(z):
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def novelty(pop, base):
    """nar_model.py:1147-1148 with log_base of :28-31: -log(pop) / log(base).  No epsilon: pop must be positive."""
    return -np.log(f64(pop)) / np.log(float(base))


def score_softmax(S3, w4, b4, tau, mask, nov_factor=0.0, neg_ids=None, pop_norm=None, pop_log_base=2.0):
    """S3 [BT, 1+N, K3] (column 0 the positive): logits = S3 w4 + b4 (matching_dense_layer_4), probs = softmax(logits / tau) (:514-515),
    nll[bt] = mask * (-log probs[bt, 0] - nov_factor * sum_n q_n nov_n) (:660, :675, :683) with q = softmax(negative logits / tau)
    (:517) and nov_n = -log_base(pop_norm[neg_n]) (:544).  sum(nll) / sum(mask) is the data part of total_loss (:664, :680)."""
    S3, w4, m = f64(S3), f64(w4), f64(mask)
    logits = S3 @ w4 + float(np.asarray(b4).reshape(-1)[0])
    z = logits / float(tau)
    probs = _softmax(z)
    nll = -np.log(probs[:, 0]) * m
    out = dict(logits=logits, probs=probs)
    if nov_factor > 0:
        q = _softmax(z[:, 1:])
        nov = novelty(np.asarray(pop_norm)[np.asarray(neg_ids)], pop_log_base)
        out.update(q=q, nov=nov, novterm=(q * nov).sum(-1))
        nll = nll - float(nov_factor) * out['novterm'] * m
    out['nll'] = nll
    return out


def leaky_grad_from_output(y):
    """Derivative of leaky_relu taken from its saved OUTPUT y: 1 where y > 0, alpha elsewhere (so +0.0 and -0.0 give alpha)."""
    return np.where(f64(y) > 0, 1.0, LEAKY)


def score_softmax_grad(S3, w4, b4, tau, mask, sum_mask, nov_factor=0.0, neg_ids=None, pop_norm=None, pop_log_base=2.0):
    """Gradient of L = sum(nll) / sum_mask, differentiated by hand.  With z = s / tau:
        d(-log p_0)/ds_c = (p_c - [c == 0]) / tau
        d(sum_n q_n nov_n)/ds_c = q_c (nov_c - sum_n q_n nov_n) / tau   for a negative c, 0 for the positive
    so ds_c = mask / (tau sum_mask) * ((p_c - [c == 0]) - nov_factor * q_c (nov_c - q.nov) [c > 0]), and
    dS3 = ds * w4 * leaky'(S3) is the gradient at the pre-activation of layer 3."""
    f = score_softmax(S3, w4, b4, tau, mask, nov_factor, neg_ids, pop_norm, pop_log_base)
    g = f['probs'].copy()
    g[:, 0] -= 1.0
    if nov_factor > 0:
        g[:, 1:] -= float(nov_factor) * f['q'] * (f['nov'] - f['novterm'][:, None])
    ds = g * (f64(mask) / (float(tau) * float(sum_mask)))[:, None]
    dS3 = ds[:, :, None] * f64(w4)[None, None, :] * leaky_grad_from_output(S3)
    return dict(ds=ds, dS3=dS3)


def rank_items(probs, label_next, neg_ids, mask):
    """tf.nn.top_k over all 1 + N candidates (:782): descending, the lower index first among equals.  Returns the ranked ids (:792),
    the sorted probabilities (:784) and the 0-based rank of the positive, -1 at a padded click."""
    probs = np.asarray(probs)
    order = np.argsort(-f64(probs), axis=-1, kind='stable')
    ids = np.concatenate([np.asarray(label_next, np.int64)[:, None], np.asarray(neg_ids, np.int64)], 1)
    rank = np.argmax(order == 0, axis=-1).astype(np.int32)
    return dict(pred_ids=np.take_along_axis(ids, order, 1), pred_probs=np.take_along_axis(probs, order, 1),
                label_rank=np.where(np.asarray(mask) != 0, rank, -1).astype(np.int32))


def mulpred_grad(dM, Z2c, pred):
    """Backward of M = Z2c * pred (:478-495) through the two tanh layers that produced Z2c [BT, 1+N, C] and pred [BT, C], given dM:
    at the CAR tanh dZ2 = dM * pred * (1 - Z2c^2); at the FC2 tanh dpred_pre = (sum_c dM * Z2c) * (1 - pred^2); col_part = sum_c dZ2."""
    dM, Z, p = f64(dM), f64(Z2c), f64(pred)
    dZ2 = dM * p[:, None, :] * (1.0 - Z * Z)
    return dict(dZ2=dZ2, dpred_pre=(dM * Z).sum(1) * (1.0 - p * p), col_part=dZ2.sum(1))


def mul_rows(Z2c, pred):
    return f64(Z2c) * f64(pred)[:, None, :]


# ---- optimizer --------------------------------------------------------------------------------------------------------------------
def adam_lr_t(lr, t, b1=0.9, b2=0.999):
    """tf.train.AdamOptimizer: lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t), t = 1 at the first step."""
    return float(lr) * np.sqrt(1.0 - float(b2) ** t) / (1.0 - float(b1) ** t)


def adam_tf(p, g, m, v, n_reg, lam, lr, t, b1=0.9, b2=0.999, eps=1e-8, lr_t=None):
    """One TF-Adam step on the flat buffer.  The L2 regulariser lam * sum(p^2) / 2 of the first n_reg entries adds lam * p to their
    gradient; m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g^2, p <- p - lr_t m / (sqrt(v) + eps): epsilon OUTSIDE the root.
    lr_t: the step size as the kernels get it (one fp32 scalar, see adam_scalars); default adam_lr_t(lr, t, b1, b2)."""
    p, g, m, v = f64(p), f64(g).copy(), f64(m), f64(v)
    g[:n_reg] += float(lam) * p[:n_reg]
    m = float(b1) * m + (1.0 - float(b1)) * g
    v = float(b2) * v + (1.0 - float(b2)) * g * g
    lr_t = adam_lr_t(lr, t, b1, b2) if lr_t is None else float(lr_t)
    return dict(p=p - lr_t * m / (np.sqrt(v) + float(eps)), m=m, v=v)


def adam_scalars(lr, t, lam):
    """The scalar arguments as a kernel receives them: fp32 values (lr_t computed in double from the nominal betas, as
    NARModuleModel.adam_lr_t does, then rounded), widened exactly - 0.999f is not 0.999."""
    r = lambda x: float(np.float32(x))
    return dict(lam=r(lam), lr=lr, t=t, b1=r(0.9), b2=r(0.999), eps=r(1e-8), lr_t=r(adam_lr_t(lr, t)))


def l2_loss(p, n_reg, lam):
    """tf.losses.get_regularization_loss (:655): sum over the regularised tensors of lam * tf.nn.l2_loss = lam * sum(w^2) / 2."""
    return 0.5 * float(lam) * float((f64(p)[:n_reg] ** 2).sum())


def loss_finalize(nll, sum_mask, sumsq, lam):
    """[total, xe, reg] of :664-667: xe = sum(nll) / sum(mask), reg = lam / 2 * sum(w^2)."""
    xe, reg = float(f64(nll).sum()) / float(sum_mask), 0.5 * float(lam) * float(sumsq)
    return np.array([xe + reg, xe, reg])


def colsum(X, w=None):
    """out[c] = sum_r w[r] X[r, c]: a bias gradient (w: the row weights of a masked / weighted sum, or None)."""
    X = f64(X)
    return X.sum(0) if w is None else (X * f64(w)[:, None]).sum(0)


# ---- error measures ---------------------------------------------------------------------------------------------------------------
def rel_err(got, ref):
    """max |got - ref| / max |ref| of one array (inf when got is not finite)."""
    got, ref = f64(got), f64(ref)
    if not np.isfinite(got).all():
        return float('inf')
    if ref.size == 0:
        return 0.0
    return float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300))


def comp_err(got, ref):
    """Worst component of |got - ref| / |ref| (a short vector whose components differ in scale, e.g. [total, xe, reg]); a component whose
    reference is zero has to be zero."""
    got, ref = f64(got).ravel(), f64(ref).ravel()
    if not np.isfinite(got).all() or (got[ref == 0] != 0).any():
        return float('inf')
    nz = ref != 0
    return float((np.abs(got - ref)[nz] / np.abs(ref[nz])).max()) if nz.any() else 0.0


def row_err(got, ref):
    """Worst click of max |got - ref| / max |ref| taken PER CLICK (axis 0): the rows of probs, ds and dS3 span many orders of magnitude
    at tau = 0.1.  Clicks whose reference row is identically zero (masked) are left to the exact-zero assertion."""
    got, ref = f64(got).reshape(len(got), -1), f64(ref).reshape(len(ref), -1)
    if not np.isfinite(got).all():
        return float('inf')
    scale = np.abs(ref).max(1)
    live = scale > 0
    if not live.any():
        return 0.0
    return float((np.abs(got - ref).max(1)[live] / scale[live]).max())


# ---- inputs -----------------------------------------------------------------------------------------------------------------------
# (N, BT, tau, nov_factor, pop_log_base, mask kind, bf16): every N of {1, 9, 50, 62, 63, 64, 127, 128, 200} - 1 + N on both sides of one
# and two 64-lane strides -, every BT of {1, 3, 4, 5, 257}, the corners, the three temperatures, both novelty settings and bases, the
# three masks and both element types
SOFTMAX_CASES = [
    (1, 1, 1.0, 0.0, 2.0, 'ones', False),
    (1, 257, 0.1, 0.3, 2.0, 'ragged', False),
    (9, 3, 0.2, 0.3, 10.0, 'ones', True),
    (9, 257, 0.2, 0.0, 2.0, 'ragged', False),
    (50, 4, 0.1, 0.0, 2.0, 'ragged', False),
    (50, 5, 0.1, 0.3, 2.0, 'zeros', False),
    (62, 5, 0.1, 0.3, 2.0, 'ragged', False),
    (63, 257, 0.1, 0.3, 10.0, 'ragged', False),
    (64, 5, 0.2, 0.0, 2.0, 'ones', True),
    (127, 3, 0.1, 0.3, 2.0, 'ones', False),
    (128, 4, 1.0, 0.3, 10.0, 'ragged', True),
    (200, 1, 0.1, 0.3, 2.0, 'ones', False),
    (200, 257, 0.1, 0.3, 2.0, 'ragged', True),
]
N_ITEMS = 500
LOGIT_TARGETS = (6.0, 0.05, 1.0, 3.0, 0.3)     # max |logit - b4| per click, cycled: z = logit / tau reaches 60 at tau = 0.1, stays < 1 elsewhere


def softmax_inputs(N, BT, tau, nov_factor, pop_log_base, mask_kind, bf16, seed=0):
    """Inputs of the softmax / ranking kernels by the issue's rules.  S3 is a post-leaky-ReLU tensor with exact +0.0 / -0.0 and the smallest
    normals planted; the clicks' logit scales cycle through LOGIT_TARGETS; click 1 has a positive 5 logits below its best negative
    (probability < 1e-20 and nll ~ 50 at tau = 0.1); with the ragged mask click 2 has a positive at least 10 logits above every negative
    (probability ~ 1, and exp overflows fp32 at tau = 0.1 unless the max over ALL candidates is subtracted) and is masked, so that its
    logits and probs are owed and its nll, ds and dS3 are exact zeros; every third click has tied negatives (bit-identical
    rows, as zero-padded negatives are), click 0 tying the positive in."""
    rng = np.random.default_rng(1000 * N + BT + seed)
    NC = N + 1
    pre = rng.standard_normal((BT, NC, K3)).astype(np.float32)
    S3 = np.where(pre > 0, pre, np.float32(LEAKY) * pre).astype(np.float32)
    w4 = (0.35 * rng.standard_normal(K3)).astype(np.float32)
    w4[np.abs(w4) < 0.05] = 0.05
    b4 = np.array([0.37], np.float32)
    u = (w4.astype(np.float64) / float(w4.astype(np.float64) @ w4.astype(np.float64)))       # u . w4 = 1
    for bt in range(BT):
        raw = np.abs(S3[bt].astype(np.float64) @ w4.astype(np.float64)).max()
        S3[bt] *= np.float32(LOGIT_TARGETS[bt % len(LOGIT_TARGETS)] / raw)
    if BT > 1:
        S3[1, 0] = (-2.5 * u).astype(np.float32)
        S3[1, 1] = (2.5 * u).astype(np.float32)
    if BT > 2 and mask_kind == 'ragged':
        S3[2, 0] = (5.5 * u).astype(np.float32)
        S3[2, 1:] = (-(4.5 + 0.5 * rng.random((N, 1))) * u[None, :]).astype(np.float32)
    for bt in range(BT):
        if bt % 4 < 2:                   # whole columns, so that the click's largest |ds| meets a zero of either sign (and ties keep them)
            S3[bt, :, 3 + bt % 4], S3[bt, :, 7 + bt % 4] = np.float32(0.0), np.float32(-0.0)
    flat = S3.reshape(-1)
    idx = rng.choice(flat.size, size=max(24, flat.size // 50), replace=False)
    plant = np.array([0.0, -0.0, TINY, -TINY], np.float32)
    flat[idx] = plant[np.arange(idx.size) % 4]
    if bf16:
        S3 = round_bf16(S3).reshape(BT, NC, K3)
    w64 = w4.astype(np.float64)
    special = mask_kind == 'ragged' and BT > 2           # click 2 keeps its lead (and is masked, see below)
    for bt in range(BT):
        # Elsewhere the positive leads the best negative by at most 0.03 logits: ds of a click is (p - [c == 0]) * scale, and where
        # p_0 -> 1 the whole row cancels to ~0, so that an error relative to the row's max measures nothing (fp32 gives 0 for 1e-40)
        lg = S3[bt].astype(np.float64) @ w64
        top = 1 + int(np.argmax(lg[1:]))
        if lg[0] - lg[top] > 0.03 and not (special and bt == 2):
            S3[bt, [0, top]] = S3[bt, [top, 0]]
    for bt in range(0, BT, 3):                 # ties last, so that the tied rows stay bit-identical
        if N >= 2:
            k = int(rng.integers(2, N + 1))
            rows = 1 + rng.choice(N, size=k, replace=False)
            lg = S3[bt].astype(np.float64) @ w64
            top = 1 + int(np.argmax(lg[1:]))
            if bt == 0 and top not in rows:
                rows[0] = top              # click 0: the positive ties with the BEST negative (it matters to the ranking and to q)
            S3[bt, rows] = S3[bt, rows[np.argmax(lg[rows])]]          # (the best of them: the positive's lead does not grow)
            if bt == 0:
                S3[bt, 0] = S3[bt, rows[0]]
        elif bt == 0:
            S3[bt, 0] = S3[bt, 1]
    if mask_kind == 'ones':
        mask = np.ones(BT, np.uint8)
    elif mask_kind == 'zeros':
        mask = np.zeros(BT, np.uint8)
    else:
        mask = (rng.random(BT) < 0.7).astype(np.uint8)
        mask[:2] = 1
        mask[2:4] = 0
    neg_ids = rng.integers(0, N_ITEMS, size=(BT, N)).astype(np.int64)
    neg_ids[0, 0] = 0
    pop_norm = np.exp(rng.uniform(np.log(1e-7), 0.0, N_ITEMS)).astype(np.float32)
    pop_norm[0], pop_norm[1] = np.float32(1e-7), np.float32(1.0)
    label_next = rng.integers(1, N_ITEMS, size=BT).astype(np.int64)
    return dict(S3=S3, w4=w4, b4=b4, tau=tau, mask=mask, sum_mask=float(mask.sum()), nov_factor=nov_factor, pop_log_base=pop_log_base,
                neg_ids=neg_ids, pop_norm=pop_norm, label_next=label_next, N=N, BT=BT, bf16=bf16, dominant=bool(special))


def softmax_args(inp):
    """The keyword arguments of score_softmax for one input set."""
    return dict(S3=inp['S3'], w4=inp['w4'], b4=inp['b4'], tau=inp['tau'], mask=inp['mask'], nov_factor=inp['nov_factor'],
                neg_ids=inp['neg_ids'], pop_norm=inp['pop_norm'], pop_log_base=inp['pop_log_base'])


# (C, N, BT): C = 1024 is one float4 per thread, 64 leaves most threads idle
MULPRED_CASES = [(64, 1, 1), (64, 50, 37), (128, 200, 1), (128, 1, 37), (256, 50, 1), (256, 200, 37), (1024, 1, 1), (1024, 50, 37), (1024, 200, 1)]


def mulpred_inputs(C, N, BT, bf16=False):
    rng = np.random.default_rng(C + 10 * N + BT)
    Z = np.tanh(1.5 * rng.standard_normal((BT, N + 1, C))).astype(np.float32)
    pred = np.tanh(1.5 * rng.standard_normal((BT, C))).astype(np.float32)
    dM = (rng.standard_normal((BT, N + 1, C)) * np.exp(rng.uniform(-6, 0, (BT, N + 1, 1)))).astype(np.float32)
    if bf16:
        Z, dM = round_bf16(Z).reshape(Z.shape), round_bf16(dM).reshape(dM.shape)
    return dict(dM=dM, Z2c=Z, pred=pred)


# (n, n_reg, lam, t); n_reg in {0, 4, n / 2 rounded to 4, n}
ADAM_LR = 1e-3
ADAM_BIG = 8192 * 256 * 4 + 8              # the grid is capped at 8192 workgroups x 256 threads x 4 floats: a second grid-stride trip
ADAM_CASES = [(4, 0, 0.0, 1), (4, 4, 1e-4, 2), (1020, 0, 1e-4, 1), (1020, 4, 1e-4, 1000), (1020, 508, 1e-4, 2), (1020, 1020, 1e-4, 1),
              (1020, 1020, 0.0, 1000), (ADAM_BIG, ADAM_BIG // 2 // 4 * 4, 1e-4, 2)]


def adam_inputs(n, seed=0):
    """p of mixed magnitude (a quarter of it ~1e-6, where one fp32 ulp of p is far below a step); g log-uniform over 1e-9 .. 1, both signs,
    with a block of exact zeros; m, v from an earlier float64 step rounded to fp32, and a block at m = v = 0 (the first step: there
    |dp| = lr_t |g| / (|g| sqrt(1 - b2) + eps) tells epsilon outside the root from epsilon inside it for |g| below ~1e-6)."""
    rng = np.random.default_rng(n % 100003 + seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    p[rng.random(n) < 0.25] *= np.float32(1e-5)
    g = (np.exp(rng.uniform(np.log(1e-9), 0.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    g0 = (np.exp(rng.uniform(np.log(1e-9), 0.0, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    prev = adam_tf(p, g0, np.zeros(n), np.zeros(n), 0, 0.0, ADAM_LR, 1)
    m, v = prev['m'].astype(np.float32), prev['v'].astype(np.float32)
    q = max(1, n // 4)
    g[q // 2:q] = 0.0                       # exact zeros (half of them on a first step)
    m[:q], v[:q] = 0.0, 0.0                 # first step
    return dict(p=p, g=g, m=m, v=v)


def adam_step_err(p_new, p_old, ref_p, lr_t):
    """max over entries of (|dp_got - dp_ref| - ulp(p)) / lr_t, floored at 0: the update compared in units of lr_t, with one fp32 ulp of
    the weight allowed for the rounding of p - dp itself."""
    p_old = np.asarray(p_old, np.float32)
    if not np.isfinite(f64(p_new)).all():
        return float('inf')
    d = np.abs((f64(p_new) - f64(p_old)) - (f64(ref_p) - f64(p_old))) - f64(np.spacing(np.abs(p_old)))
    return float(max(d.max(), 0.0) / lr_t)


COLSUM_F = [1, 3, 4, 12, 32, 128, 256, 378, 1024, 1028]


def colsum_vec_ok(F, ld):
    """The shapes the float4 stage-1 kernel takes (and the only ones cham_colsum_b16 admits)."""
    return F % 4 == 0 and F // 4 <= 256 and 256 % (F // 4) == 0 and ld % 4 == 0


def colsum_cases():
    """(R, F, ld, weights, accumulate).  R: {1, 63, 64, 65} around one 64-row chunk, 64 * 67 + 5 (67 chunks + a short one: both loops of
    the second stage), 70 000 (more than 64 rows per chunk; the narrow F only, to keep the arrays small) and, where the float4 kernel
    runs, 4 rpi - 1, 4 rpi, 4 rpi + 1 with rpi = 256 / (F / 4) row lanes.  ld, weights and accumulate rotate so that every value of
    each meets every F."""
    cases = []
    for F in COLSUM_F:
        Rs = [1, 63, 64, 65, 64 * 67 + 5] + ([70000] if F <= 32 else [])
        if colsum_vec_ok(F, F):
            rpi = 256 // (F // 4)
            Rs += [4 * rpi - 1, 4 * rpi, 4 * rpi + 1]
        for i, R in enumerate(Rs):
            cases.append((R, F, F + (0, 4, 1)[i % 3], i % 2 == 0, (i // 2) % 2))
    return cases


def colsum_inputs(R, F, ld, bf16=False):
    rng = np.random.default_rng(R * 31 + F)
    X = (rng.standard_normal((R, ld)) + 0.25).astype(np.float32)
    if bf16:
        X = round_bf16(X).reshape(R, ld)
    w = rng.uniform(0.0, 2.0, R).astype(np.float32)
    w[rng.random(R) < 0.2] = 0.0                      # masked rows
    prev = rng.standard_normal(F).astype(np.float32)   # what `out` holds before an accumulating call
    return dict(X=X, w=w, prev=prev)


def colsum_chunk_rows(R):
    return max(64, (R + 1023) // 1024)


# (n_reg, BT) of the loss kernels
LOSS_CASES = [(0, 1), (4, 255), (1000, 256), (1000, 257), (5 * 10 ** 6, 5000)]
LOSS_LAMBDA = 1e-4


def loss_inputs(n_reg, BT):
    rng = np.random.default_rng(n_reg % 1009 + BT)
    p = (0.05 * rng.standard_normal(n_reg + 8)).astype(np.float32)      # 8 entries beyond n_reg that must not count
    mask = (rng.random(BT) < 0.7).astype(np.uint8)
    mask[0] = 1
    nll = np.where(mask != 0, rng.uniform(0.0, 60.0, BT), 0.0).astype(np.float32)      # a masked position carries nll = 0
    return dict(p=p, nll=nll, mask=mask, sum_mask=float(mask.sum()))


# ---- device buffers of the GPU tests ------------------------------------------------------------------------------------------------
GUARD = 64                    # elements on either side of every output (a multiple of 8: float4 / bf16x4 alignment is kept)
SENTINEL = -0x5A5A5A5B        # integer outputs start as this; float outputs as NaN


class Guarded:
    """An output array inside a larger device allocation.  The array and GUARD elements on either side start as NaN (integers: SENTINEL):
    an element the kernel owes and does not write stays NaN and fails the comparison, and numpy() insists that the guards are as they were."""

    def __init__(self, gpu, shape, dtype=None, init=None):
        import torch
        self.torch = torch
        dtype = dtype or torch.float32
        n = int(np.prod(shape))
        self.fp = dtype.is_floating_point
        self.fill = float('nan') if self.fp else (SENTINEL if dtype in (torch.int32, torch.int64) else 0x5A)
        self.buf = torch.full((n + 2 * GUARD,), self.fill, dtype=dtype, device=gpu)
        self.t = self.buf[GUARD:GUARD + n].view(*shape)
        if init is not None:
            self.t.copy_(init)

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.buf.element_size()          # (not self.t.data_ptr(): an empty view may report none)

    def _is_fill(self, x):
        return bool(self.torch.isnan(x.float()).all()) if self.fp else bool((x == self.fill).all())

    def intact(self):
        return self._is_fill(self.buf[:GUARD]) and self._is_fill(self.buf[self.buf.numel() - GUARD:])

    def untouched(self):
        return self._is_fill(self.buf)

    def numpy(self):
        """fp32 / integer arrays as they are, bf16 and fp16 as uint16 bit patterns."""
        assert self.intact(), "a kernel wrote outside its output"
        t = self.t
        if t.dtype in (self.torch.bfloat16, self.torch.float16):
            return t.view(self.torch.int16).cpu().numpy().view(np.uint16)
        return t.cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
