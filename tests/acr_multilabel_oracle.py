"""Float64 restatement of the ACR model's MULTILABEL head (reference acr_module/acr/acr_model.py:202-215, :6-8, :254-268) for the
Adressa ACR tests, on top of tests/acr_oracle.py.

The head is torch's ``binary_cross_entropy_with_logits`` against the COUNT-valued multi-hot target under autograd; the closed forms the
kernel implements are restated beside it in numpy so that the CPU tests can hold one against the other.  Nothing here is imported by the
product package."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests import acr_oracle as AO

U = AO.U


def multi_hot(ids, C):
    """z [B, C] float64: z[b,c] = #{k : ids[b,k] == c} (reduce_sum(one_hot): a duplicated id counts twice, an id outside [0, C) counts
    nowhere), then column 0, the padding id, forced to 0.  ids: [B, K]; K may be 0."""
    ids = np.asarray(ids)
    assert ids.ndim == 2
    z = np.zeros((ids.shape[0], C))
    for b in range(ids.shape[0]):
        for v in ids[b]:
            if 0 <= v < C:
                z[b, int(v)] += 1.0
    z[:, 0] = 0.0
    return z


def sigmoid_ce(logits, z):
    """mean over the classes, then over the rows (= the mean over all B C elements) of sigmoid_cross_entropy_with_logits."""
    return F.binary_cross_entropy_with_logits(logits, z, reduction='mean')


def autograd_loss_and_dlogits(x, z):
    """(loss, dlogits) in float64 through autograd."""
    xt = torch.tensor(np.asarray(x, np.float64), requires_grad=True)
    loss = sigmoid_ce(xt, torch.tensor(np.asarray(z, np.float64)))
    loss.backward()
    return float(loss.detach()), xt.grad.numpy()


def closed_form(x, z):
    """The formulas of the kernel in float64 numpy: (term [B, C], loss, dlogits [B, C])."""
    x, z = np.asarray(x, np.float64), np.asarray(z, np.float64)
    term = np.maximum(x, 0.0) - x * z + np.log1p(np.exp(-np.abs(x)))
    e = np.exp(-np.abs(x))
    sig = np.where(x >= 0, 1.0, e) / (1.0 + e)
    return term, term.sum() / x.size, (sig - z) / x.size


def counts(x, z):
    """(pred uint8 [B, C], (tp, fp, fn)) by a direct count; pred = x > 0."""
    p = np.asarray(x) > 0
    pos = np.asarray(z) > 0
    return p.astype(np.uint8), (int((p & pos).sum()), int((p & ~pos).sum()), int((~p & pos).sum()))


def precision_recall(batch_counts):
    """tf.metrics.precision / recall over a list of per-batch (tp, fp, fn): sums first; an empty denominator gives 0."""
    tp, fp, fn = (sum(c[i] for c in batch_counts) for i in range(3))
    return (tp / (tp + fp) if tp + fp else 0.0), (tp / (tp + fn) if tp + fn else 0.0)


class ACRMultilabelOracle(AO.ACROracle):
    """ACROracle whose heads named in ``multilabel`` take labels[head] = zero-padded id lists [B, Kmax] and the sigmoid cross-entropy
    (no class weights); the other heads keep the weighted softmax cross-entropy."""

    def __init__(self, *args, multilabel=(), **kw):
        super().__init__(*args, **kw)
        self.multilabel = tuple(multilabel)

    def head_loss(self, n, logits, labels):
        if n in self.multilabel:
            z = torch.as_tensor(multi_hot(labels[n], self.heads[n]), dtype=self.dtype)
            return sigmoid_ce(logits[n], z)
        return AO.weighted_ce(logits[n], torch.as_tensor(np.asarray(labels[n]), dtype=torch.long), self.cw.get(n))

    def loss(self, text, labels):
        _, _, _, logits = self.forward(text)
        ce = sum(self.head_loss(n, logits, labels) for n in self.heads)
        reg = self.l2 * sum((v * v).sum() / 2 for n, v in self.w.items() if n.endswith('/kernel'))
        return ce + reg, ce, reg


def make_pair(model, table, class_weights, lr):
    """(float64 oracle, float32 oracle) at the model's current weights."""
    heads = OrderedDict(model.layout.heads)
    w = model.logical_weights()
    mk = lambda dt: ACRMultilabelOracle(table, len(model.layout.sizes), heads, w, model.l2_reg_lambda, lr, class_weights=class_weights,
                                        dtype=dt, multilabel=model.multilabel)
    return mk(torch.float64), mk(torch.float32)
