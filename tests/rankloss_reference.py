"""Float64 reference of the pairwise ranking losses (--loss_function; csrc/rank_loss.hip), for
tests/test_rankloss_cpu.py and tests/test_rankloss_gpu.py.

Per click, r [..., 1 + N] = logits / tau with r_0 the positive, d_n = r_0 - r_n, s the logistic function and q = softmax(r_1..r_N) over the
negatives alone (differentiated, not a constant):
    bpr       l = -(1/N) sum_n log s(d_n)
    top1      l = (1/N) sum_n [s(-d_n) + s(r_n^2)]
    bpr_max   l = -log(sum_n q_n s(d_n) + 1e-24) + lam sum_n q_n r_n^2
    top1_max  l = sum_n q_n [s(-d_n) + s(r_n^2)]
`loss` states the table (any float dtype: run on float32 tensors it is the fp32 restatement the GPU tolerances are built on), `hand_grad`
the hand-derived dl/dr the kernels implement, `autograd_grad` what torch differentiates from `loss`."""
import torch

KINDS = ('bpr', 'top1', 'bpr_max', 'top1_max')
GRID_N = (1, 4, 63, 64, 130)
GRID_SCALE = (1.0, 8.0, 40.0)
LOG_EPS = 1e-24
EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -126


def log_sigmoid(x):
    """min(x, 0) - log1p(exp(-|x|)): no log of a sigmoid that may have underflowed."""
    return torch.clamp(x, max=0.0) - torch.log1p(torch.exp(-x.abs()))


def dsigmoid(x):
    """s'(x) = s(x) s(-x) from e = exp(-|x|): no 1 - s(x)."""
    e = torch.exp(-x.abs())
    return e / ((1.0 + e) * (1.0 + e))


def _parts(r):
    r0, rn = r[..., :1], r[..., 1:]
    return r0, rn, r0 - rn


def loss(kind, r, lam=0.5, sigmoid=torch.sigmoid):
    """l [...] of r [..., 1 + N]."""
    _, rn, d = _parts(r)
    if kind == 'bpr':
        return -log_sigmoid(d).mean(-1)
    if kind == 'top1':
        return (sigmoid(-d) + sigmoid(rn * rn)).mean(-1)
    q = torch.softmax(rn, -1)
    if kind == 'bpr_max':
        return -torch.log((q * sigmoid(d)).sum(-1) + LOG_EPS) + lam * (q * rn * rn).sum(-1)
    if kind == 'top1_max':
        return (q * (sigmoid(-d) + sigmoid(rn * rn))).sum(-1)
    raise ValueError(kind)


def hand_grad(kind, r, lam=0.5):
    """dl/dr [..., 1 + N], hand-derived."""
    _, rn, d = _parts(r)
    N = rn.shape[-1]
    if kind == 'bpr':
        gn = torch.sigmoid(-d) / N
        g0 = -gn.sum(-1, keepdim=True)
    elif kind == 'top1':
        gn = (dsigmoid(d) + 2.0 * rn * dsigmoid(rn * rn)) / N
        g0 = -(dsigmoid(d)).sum(-1, keepdim=True) / N
    elif kind == 'bpr_max':
        q = torch.softmax(rn, -1)
        A = (q * torch.sigmoid(d)).sum(-1, keepdim=True)
        R = (q * rn * rn).sum(-1, keepdim=True)
        dA = q * (torch.sigmoid(d) - A) - q * dsigmoid(d)
        dR = q * (rn * rn - R) + 2.0 * q * rn
        gn = -dA / (A + LOG_EPS) + lam * dR
        g0 = -(q * dsigmoid(d)).sum(-1, keepdim=True) / (A + LOG_EPS)
    elif kind == 'top1_max':
        q = torch.softmax(rn, -1)
        Tn = torch.sigmoid(-d) + torch.sigmoid(rn * rn)
        l = (q * Tn).sum(-1, keepdim=True)
        gn = q * (Tn - l) + q * (dsigmoid(d) + 2.0 * rn * dsigmoid(rn * rn))
        g0 = -(q * dsigmoid(d)).sum(-1, keepdim=True)
    else:
        raise ValueError(kind)
    return torch.cat([g0, gn], -1)


def autograd_grad(kind, r, lam=0.5):
    """What torch differentiates from `loss`, with s(x) written exp(log s(x)): torch.sigmoid's own backward is s (1 - s), whose 1 - s
    carries an absolute error of one ulp of 1 - more than the whole derivative where it has half saturated."""
    x = r.detach().clone().requires_grad_(True)
    loss(kind, x, lam, sigmoid=lambda v: torch.exp(log_sigmoid(v))).sum().backward()
    return x.grad


def abs_terms(kind, r, lam=0.5):
    """(loss_abs [...], grad_abs [...]): the sums of the absolute values of the summands l and dl/dr are made of, the magnitudes a rounding
    bound of the form k eps sum|terms| refers to.  loss_abs carries + 1: the softmax weights and the sigmoids are O(1) quantities whose
    rounding is absolute (the error of log(A) is the RELATIVE error of A)."""
    _, rn, d = _parts(r)
    N = rn.shape[-1]
    sd, ds_, dr2 = torch.sigmoid(-d), dsigmoid(d), (2.0 * rn * dsigmoid(rn * rn)).abs()
    if kind == 'bpr':
        return 1.0 + log_sigmoid(d).abs().mean(-1), 2.0 * sd.sum(-1) / N
    if kind == 'top1':
        return 1.0 + (sd + torch.sigmoid(rn * rn)).mean(-1), (2.0 * ds_ + dr2).sum(-1) / N
    q = torch.softmax(rn, -1)
    if kind == 'bpr_max':
        A = (q * torch.sigmoid(d)).sum(-1, keepdim=True)
        R = (q * rn * rn).sum(-1, keepdim=True)
        ga = (q * (torch.sigmoid(d) + A) + 2.0 * q * ds_).sum(-1) / (A.squeeze(-1) + LOG_EPS) + lam * (q * (rn * rn + R + 2.0 * rn.abs())).sum(-1)
        return 1.0 + torch.log(A.squeeze(-1) + LOG_EPS).abs() + lam * R.squeeze(-1), ga
    Tn = sd + torch.sigmoid(rn * rn)
    l = (q * Tn).sum(-1, keepdim=True)
    return 1.0 + l.squeeze(-1), (q * (Tn + l) + 2.0 * q * ds_ + q * dr2).sum(-1)


def make_logits(BT, N, scale, seed=0):
    """fp32 logits [BT, 1 + N] ~ N(0, scale^2)."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * N + int(scale))
    return (scale * torch.randn(BT, N + 1, generator=g, dtype=torch.float64)).float()


def reference(kind, s, tau, lam, mask):
    """Float64 per-click outputs of the kernel pair for fp32 logits s [BT, NC] and a 0/1 mask [BT]: dict(nll [BT], ds [BT, NC], probs,
    loss_abs [BT], ds_abs [BT])."""
    r = s.double() / tau
    mk = torch.as_tensor(mask).double()
    l, g = loss(kind, r, lam), hand_grad(kind, r, lam)
    la, ga = abs_terms(kind, r, lam)
    k = mk / (tau * mk.sum())
    return dict(nll=l * mk, ds=g * k[:, None], probs=torch.softmax(r, -1), loss_abs=la * mk, ds_abs=ga * k)


def f32_deviation(kind, s, tau, lam, mask):
    """The fp32 restatement (the same formulas on float32 tensors, r = s * (1 / tau) as the kernels form it) against `reference`, per
    click: (|l32 - l64| [BT], max_c |ds32 - ds64| [BT], whether every fp32 value is finite)."""
    ref = reference(kind, s, tau, lam, mask)
    r32 = s.float() * torch.tensor(1.0 / tau, dtype=torch.float32)
    l32, g32 = loss(kind, r32, lam), hand_grad(kind, r32, lam)
    assert l32.dtype == torch.float32 and g32.dtype == torch.float32
    mk = torch.as_tensor(mask).double()
    k = mk / (tau * mk.sum())
    finite = bool(torch.isfinite(l32).all()) and bool(torch.isfinite(g32).all())
    return (l32.double() * mk - ref['nll']).abs(), (g32.double() * k[:, None] - ref['ds']).abs().amax(-1), finite


def kernel_bounds(kind, s, tau, lam, mask, factor=4.0):
    """Per-click absolute bounds (nll_tol [BT], ds_tol [BT]) of the GPU kernels against `reference`: the larger of `factor` x the fp32
    restatement's own deviation at that click and (N + 32) eps sum|terms|, + (N + 32) 2^-126 [x 1 / (A + 1e-24) for the gradient of
    bpr_max, which divides by it]: a term below the smallest normal fp32 number is held to no relative precision, or flushed to zero.
    `factor` allows for the butterfly summation order and the device's expf / logf / log1pf; it started at 8, the worst error observed on an
    MI355X was 1.4 x the restatement's deviation (profiles/rankloss_notes.md), and it was tightened to 4."""
    ref = reference(kind, s, tau, lam, mask)
    N = s.shape[-1] - 1
    dev_l, dev_g, _ = f32_deviation(kind, s, tau, lam, mask)
    k = (N + 32) * EPS32
    tiny = (N + 32) * TINY32
    amp = 1.0
    if kind == 'bpr_max':
        _, rn, d = _parts(s.double() / tau)
        amp = 1.0 / ((torch.softmax(rn, -1) * torch.sigmoid(d)).sum(-1) + LOG_EPS)
    mk = torch.as_tensor(mask).double()
    return (torch.maximum(factor * dev_l, k * ref['loss_abs']) + tiny,
            torch.maximum(factor * dev_g, k * ref['ds_abs']) + tiny * amp * mk / (tau * mk.sum()))
