"""float64 restatement of the cosine ranking head (--recommendations_ranking cosine; csrc/cosine.hip) for
tests/test_cosine_cpu.py and tests/test_cosine_gpu.py.

For a click with p = pred (FC2 tanh output, width C) and candidate rows z_c (CAR tanh output, c = 0 the label):
    inv(x)  = rsqrt(max(sum_k x_k^2, 1e-12))                       (tf.nn.l2_normalize)
    rz_c = inv(z_c), rp = inv(p), z^_c = z_c rz_c, p^ = p rp,  cos_c = sum_k z^_ck p^_k
`autograd_grads` takes the two tanh PRE-activations as leaves and lets autograd differentiate sum_c ds_c cos_c; `closed_form` is what the
kernels compute, with the expressions over absolute values the tests' error bounds are stated in."""
import torch

NORM_FLOOR = 1e-12


def inv_norm(x):
    return torch.rsqrt(torch.clamp((x * x).sum(-1), min=NORM_FLOOR))


def cosine(z, p):
    """z [..., NC, C], p [..., C] -> (cos [..., NC], rz [..., NC], rp [...])."""
    rz, rp = inv_norm(z), inv_norm(p)
    zh, ph = z * rz.unsqueeze(-1), p * rp.unsqueeze(-1)
    return (zh * ph.unsqueeze(-2)).sum(-1), rz, rp


def autograd_grads(z, p, ds):
    """Gradients of sum_c ds_c cos_c with respect to the pre-activations atanh(z), atanh(p) (float64 leaves; |z|, |p| < 1)."""
    z, p, ds = (torch.as_tensor(x, dtype=torch.float64) for x in (z, p, ds))
    zpre = torch.atanh(z).detach().requires_grad_(True)
    ppre = torch.atanh(p).detach().requires_grad_(True)
    cos, _, _ = cosine(torch.tanh(zpre), torch.tanh(ppre))
    (ds * cos).sum().backward()
    return cos.detach(), zpre.grad, ppre.grad


def closed_form(z, p, ds):
    """dict(cos, rz, rp, dz, dp, abs_cos, abs_dz, abs_dp): the closed forms
        dZ2pre_ck   = ds_c rz_c (p^_k - cos_c z^_ck) (1 - z_ck^2)
        dpred_pre_k = (sum_c ds_c rp (z^_ck - cos_c p^_k)) (1 - p_k^2)
    with the projection term of a clamped vector (sum of squares < 1e-12: its inverse norm is the constant 1e6) dropped, and the same
    expressions evaluated over absolute values (every product and sum of |terms|: what an fp32 evaluation's rounding error scales with)."""
    z, p, ds = (torch.as_tensor(x, dtype=torch.float64) for x in (z, p, ds))
    cos, rz, rp = cosine(z, p)
    zfree = ((z * z).sum(-1) >= NORM_FLOOR).to(z.dtype)          # 0 where the row's norm is clamped
    pfree = ((p * p).sum(-1) >= NORM_FLOOR).to(z.dtype)
    zh, ph = z * rz.unsqueeze(-1), (p * rp.unsqueeze(-1)).unsqueeze(-2)
    g = (ds * rz).unsqueeze(-1)
    dz = g * (ph - (cos * zfree).unsqueeze(-1) * zh) * (1.0 - z * z)
    inner = ds.unsqueeze(-1) * (zh - (cos * pfree.unsqueeze(-1)).unsqueeze(-1) * ph)
    dp = inner.sum(-2) * rp.unsqueeze(-1) * (1.0 - p * p)
    abs_cos = (zh.abs() * ph.abs()).sum(-1)
    abs_dz = g.abs() * (ph.abs() + abs_cos.unsqueeze(-1) * zh.abs()) * (1.0 + z * z)
    abs_dp = (ds.abs().unsqueeze(-1) * (zh.abs() + abs_cos.unsqueeze(-1) * ph.abs())).sum(-2) * rp.unsqueeze(-1) * (1.0 + p * p)
    return dict(cos=cos, rz=rz, rp=rp, dz=dz, dp=dp, abs_cos=abs_cos, abs_dz=abs_dz, abs_dp=abs_dp)


def make_case(BT, NC, C, seed=0, special=True, dtype=torch.float32):
    """Inputs of the kernel tests: z [BT, NC, C] and p [BT, C] in (-1, 1) like tanh outputs, ds [BT, NC], mask [BT] (uint8).  With `special`:
    an exact-zero candidate row, a row with sum z^2 < 1e-12 (every element 1e-8), a zero pred (the last click, when BT > 1) and - when
    BT >= 3 - a masked click, whose ds is 0 as the softmax backward leaves it."""
    g = torch.Generator().manual_seed(1000 * seed + 17 * BT + 3 * NC + C)
    z = torch.tanh(0.8 * torch.randn(BT, NC, C, generator=g, dtype=torch.float64)).to(dtype)
    p = torch.tanh(0.8 * torch.randn(BT, C, generator=g, dtype=torch.float64)).to(dtype)
    ds = (torch.randn(BT, NC, generator=g, dtype=torch.float64) / (0.1 * BT * NC)).to(dtype)
    mask = torch.ones(BT, dtype=torch.uint8)
    if special:
        z[0, 0] = 0.0
        z[0, NC - 1] = 1e-8
        if BT > 1:
            p[BT - 1] = 0.0
        if BT >= 3:
            mask[1] = 0
            ds[1] = 0.0
    return z, p, ds, mask
