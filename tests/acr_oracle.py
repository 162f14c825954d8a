"""Float64 restatement of the ACR model (reference acr_module/acr/acr_model.py:83-289) in torch autograd, for the ACR tests.

The max over time is ``torch.amax``, which splits the gradient evenly among tied positions as tf.reduce_max does.  The same code runs
in float32 (``dtype=torch.float32``): the tests bound the GPU's deviation from the float64 result by a multiple of the float32
restatement's own deviation.  Nothing here is imported by the product package."""
from collections import OrderedDict

import numpy as np
import torch

U = 2.0 ** -24                      # unit roundoff of fp32


def gamma(n):
    return n * U / (1.0 - n * U)


def conv_relu(x, W, bias):
    """x [B, L, E], W [k, E, F], bias [F] -> relu(conv "valid") [B, L-k+1, F]."""
    k = W.shape[0]
    win = x.unfold(1, k, 1)                                  # [B, L-k+1, E, k]
    return torch.relu(torch.einsum('btej,jef->btf', win, W) + bias)


def conv_abs_bound(x, W, bias):
    """|bias| + sum |x||w| per conv output element [B, L-k+1, F]: the factor of the fp32 rounding bound gamma_(kE+2)."""
    k = W.shape[0]
    return torch.einsum('btej,jef->btf', x.abs().unfold(1, k, 1), W.abs()) + bias.abs()


def weighted_ce(logits, labels, class_weights=None):
    """tf.losses.sparse_softmax_cross_entropy(weights = class_weights[labels]) under SUM_BY_NONZERO_WEIGHTS."""
    ce = torch.logsumexp(logits, dim=1) - logits.gather(1, labels.view(-1, 1)).squeeze(1)
    if class_weights is None:
        return ce.mean()
    w = class_weights[labels]
    nz = (w != 0).sum()
    return (w * ce).sum() / nz if int(nz) > 0 else (w * ce).sum() * 0.0


def first_index_conv_grads(x, argmax, g, k):
    """The closed form the kernel implements, in float64 numpy: x [B, L, E] gathered input, argmax [B, F] (first index of the max),
    g [B, F] = dpool where pool > 0 else 0  ->  dW [k, E, F] = sum_b g[b,f] x[b, argmax[b,f] + j, e],  dbias [F] = sum_b g[b,f]."""
    x, g = np.asarray(x, np.float64), np.asarray(g, np.float64)
    B, F = g.shape
    dW = np.zeros((k, x.shape[2], F))
    for b in range(B):
        for f in range(F):
            if g[b, f] != 0.0:
                t = int(argmax[b, f])
                dW[:, :, f] += g[b, f] * x[b, t:t + k, :]
    return dW, g.sum(axis=0)


def first_index_conv_abs(x, argmax, g, k):
    """sum_b |g||x| per element of dW [k, E, F] and of dbias [F]: the factors of the backward's rounding bound gamma_(B+1)."""
    return first_index_conv_grads(np.abs(np.asarray(x, np.float64)), argmax, np.abs(np.asarray(g, np.float64)), k)


class ACROracle:
    """weights: {'conv_<s>/kernel' [k,E,F], 'conv_<s>/bias', 'fc2/kernel', 'fc2/bias', 'ace/kernel', 'ace/bias',
    'output_<head>/kernel', 'output_<head>/bias'} (the logical, un-padded tensors of ACR_Model.logical_weights())."""

    def __init__(self, table, n_sizes, heads, weights, l2_reg_lambda, learning_rate, class_weights=None, dtype=torch.float64):
        self.dtype = dtype
        self.table = torch.as_tensor(np.asarray(table), dtype=dtype)
        self.n_sizes, self.heads = n_sizes, OrderedDict(heads)
        self.w = OrderedDict((n, torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True)) for n, v in weights.items())
        self.l2, self.lr = l2_reg_lambda, learning_rate
        self.cw = {n: torch.as_tensor(np.asarray(v), dtype=dtype) for n, v in (class_weights or {}).items()}
        self.m = {n: torch.zeros_like(v) for n, v in self.w.items()}
        self.v = {n: torch.zeros_like(v) for n, v in self.w.items()}
        self.step = 0

    def forward(self, text):
        x = self.table[torch.as_tensor(np.asarray(text), dtype=torch.long)]
        pools = [conv_relu(x, self.w['conv_%d/kernel' % s], self.w['conv_%d/bias' % s]).amax(dim=1) for s in range(self.n_sizes)]
        pool = torch.cat(pools, dim=1)
        fc2 = torch.relu(pool @ self.w['fc2/kernel'] + self.w['fc2/bias'])
        ace = torch.tanh(fc2 @ self.w['ace/kernel'] + self.w['ace/bias'])
        logits = OrderedDict((n, ace @ self.w['output_%s/kernel' % n] + self.w['output_%s/bias' % n]) for n in self.heads)
        return pool, fc2, ace, logits

    def loss(self, text, labels):
        _, _, _, logits = self.forward(text)
        ce = sum(weighted_ce(logits[n], torch.as_tensor(np.asarray(labels[n]), dtype=torch.long), self.cw.get(n)) for n in self.heads)
        reg = self.l2 * sum((v * v).sum() / 2 for n, v in self.w.items() if n.endswith('/kernel'))
        return ce + reg, ce, reg

    def train_step(self, text, labels):
        """One tf.train.AdamOptimizer step; returns dict(loss, grads {name: numpy}, params {name: numpy} AFTER the update).
        The optimizer's scalars are what an fp32 variable's update receives (TF casts beta1, beta2 and epsilon to the variable's dtype:
        0.999f is 0.99900001287, so 1 - beta2 is not 0.001) and lr_t is computed in double from the nominal betas, then rounded - the
        convention of tests/tail_reference.py adam_scalars, which the optimizer kernel's own tests use."""
        r = lambda x: float(np.float32(x))
        b1, b2, eps = r(0.9), r(0.999), r(1e-8)
        for v in self.w.values():
            v.grad = None
        total, ce, reg = self.loss(text, labels)
        total.backward()
        self.step += 1
        lr_t = r(self.lr * np.sqrt(1.0 - 0.999 ** self.step) / (1.0 - 0.9 ** self.step))
        grads = OrderedDict()
        with torch.no_grad():
            for n, p in self.w.items():
                g = p.grad if p.grad is not None else torch.zeros_like(p)
                grads[n] = g.detach().numpy().copy()
                self.m[n] = b1 * self.m[n] + (1 - b1) * g
                self.v[n] = b2 * self.v[n] + (1 - b2) * g * g
                p -= lr_t * self.m[n] / (self.v[n].sqrt() + eps)
        return dict(loss=float(total.detach()), ce=float(ce.detach()), reg=float(reg.detach()), grads=grads,
                    params=OrderedDict((n, p.detach().numpy().copy()) for n, p in self.w.items()))


def max_rel_dev(got, ref):
    """Max-norm deviation relative to the reference tensor's largest magnitude."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = np.abs(ref).max()
    return float(np.abs(got - ref).max() / scale) if scale > 0 else float(np.abs(got).max())
