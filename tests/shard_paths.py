"""What tests/test_shard_paths_cpu.py and tests/test_shard_paths_gpu.py share (host only): the model variants, the batches, the per-entry
gradient bound and the oracle evaluated on row shards.

The per-entry bound.  A step evaluated on row shards (micro-batches, data-parallel ranks) computes the same real-number gradient as the
whole-batch step in another fp32 summation order.  How far two correct fp32 evaluations of one gradient tensor lie apart is measured on the
oracle itself: the float32 oracle against its float64 twin, on the same batch and the same weights, per entry of the flat parameter layout
(not per flat buffer: a small tensor cannot hide behind the item table).  The shard sum may deviate from the whole-batch gradient by
    max(FACTOR x max|g_oracle32 - g_oracle64|, 8 u x max|g_oracle64|),   u = 2^-24, FACTOR = 4
over the entry (the factor for another summation and rounding order is the one tests/test_acr_gpu.py uses).  An entry whose factor a
correct path is measured to exceed is listed in the GPU file's ENTRY_FACTOR with twice the measured worst, and no bound ever goes above the
step-parity bound 3e-4 x max|ref| + 2e-5 of tests/test_step_gpu.py."""
from collections import OrderedDict

import numpy as np

from chameleon_recsys_amd.nar import synthetic
from tests import helpers as H

U = 2.0 ** -24
FACTOR = 4.0
B, SEQ_LEN, NEG, N_ITEMS = 48, 8, 8, 1000          # the smallest batch at which every split below is uneven and the sessions are ragged
WORLDS = (2, 3)
MICRO = (20, 47)                                  # 20 + 20 + 8 sessions; 47 + 1: a one-session shard is the smallest a shard can be

# id -> (pair builder, what differs from tiny_params)
VARIANTS = OrderedDict([
    ('default', ('plain', dict())),
    ('gru2', ('plain', dict(rnn_cell='gru', rnn_num_layers=2, H=256))),                    # fused time loop, stacked
    ('gru_wide', ('plain', dict(rnn_cell='gru', H=500))),                                  # step-wise point kernels, Hp 512
    ('lstm2', ('lstm', dict(rnn_cell='lstm', rnn_num_layers=2, H=300))),
    ('novelty', ('plain', dict(novelty_reg_factor=0.3))),
    ('diversity', ('diversity', dict(diversity_reg_factor=0.5, clustered_ace=True))),
    ('cosine', ('cosine', dict(recommendations_ranking='cosine'))),
    ('cosine_all', ('cosine', dict(recommendations_ranking='cosine', diversity_reg_factor=0.5, novelty_reg_factor=0.3, clustered_ace=True))),
    ('dropout', ('plain', dict(dropout_keep_prob=0.8, rnn_cell='gru', rnn_num_layers=2))),   # DenseInput path
    ('planes', ('plain', dict(C=256))),                # plane-resident CAR GEMMs, W2 plane shadows, fused dgrad
    ('planes_cosine', ('cosine', dict(recommendations_ranking='cosine', C=256))),          # two-plane cosine backward, its own scale record
    ('bf16', ('plain', dict(gemm_dtype='bf16', C=256))),
])
PLANE_VARIANTS = ('planes', 'planes_cosine', 'bf16')          # scale records are maxima over the call's rows: shard and whole batch round differently


def params(variant, **more):
    from tests import diversity_oracle as DO
    over = dict(VARIANTS[variant][1], **more)
    if over.pop('clustered_ace', False):
        over['content_article_embeddings_matrix'] = DO.clustered_ace(N_ITEMS, 64)
    return H.tiny_params(batch_size=B, neg=NEG, **over)


def batches(p, n=4):
    return synthetic.make_batches(n, B, SEQ_LEN, N_ITEMS, p['session_features_config'], length_dist='g1')


def make_pair(variant, seed=3, **more):
    """(params, HIP model, float32 oracle) of a variant - the oracle emulates the bf16 rounding where the parameters ask for it."""
    kind, p = VARIANTS[variant][0], params(variant, **more)
    if kind == 'plain':
        model, orc = H.make_pair(p, seed=seed)
    elif kind == 'lstm':
        from tests import lstm_oracle
        model, orc = lstm_oracle.make_pair(p, seed=seed)
    elif kind == 'diversity':
        from tests import diversity_oracle
        model, orc = diversity_oracle.make_pair(p, seed=seed)
    else:
        from tests import cosine_oracle
        model, orc = cosine_oracle.make_pair(p, seed=seed)
    return p, model, orc


def twin(orc, dtype, weights=None, **over):
    """The oracle's class in another dtype on the same weights (or on `weights`, with the same step counter: the sampler is keyed by it),
    and with parameters overridden (gemm_dtype='f32' of a bf16 pair)."""
    t = type(orc)(dict(orc.p, **over), weights=orc.weights_numpy() if weights is None else weights, dtype=dtype)
    t.global_step = orc.global_step
    return t


def layout_of(p):
    from chameleon_recsys_amd.nar.layout import ParamLayout
    acfg, ace = p['articles_features_config'], p['content_article_embeddings_matrix']
    n_items = acfg['article_id'].get('cardinality', ace.shape[0]) if 'article_id' in acfg else ace.shape[0]
    return ParamLayout(p['session_features_config'], acfg, n_items, ace.shape[1], p['CAR_embedding_size'], p['rnn_units'],
                       p.get('rnn_num_layers', 1), p.get('rnn_cell', 'ugrnn'), p.get('internal_features_config'),
                       p.get('max_cardinality_for_ohe', 10), p.get('recommendations_ranking', 'mlp'))


def valid_mask(f):
    T = np.asarray(f['item_clicked']).shape[1]
    return np.arange(T)[None, :] < (np.asarray(f['session_size']).reshape(-1, 1) - 1)


# ---- the oracle, whole batch and on row shards ----------------------------------------------------------------------------------------
def data_loss(ref):
    """What the HIP backward differentiates: everything but the L2 term (that one is added inside the Adam kernel)."""
    return ref['total_loss'] - ref['reg_loss']


def oracle_grads(orc):
    return OrderedDict((k, v.grad.numpy().astype(np.float64) if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in orc.w.items())


def oracle_pass(orc, f, l, buf, pop, signs=None):
    """One whole-batch forward + backward -> dict(logits, xe, loss (data terms), grads, neg_items, mask, div_e); `signs`: a function that
    returns a fresh NAROracle.leaky_signs record (the HIP run's leaky-ReLU branches), or None."""
    for v in orc.w.values():
        v.grad = None
    orc.leaky_signs = signs() if signs is not None else None
    ref = orc.forward(f, l, buf, pop, 'train')
    orc.leaky_signs = None
    data_loss(ref).backward()
    return dict(logits=ref['logits'].detach().numpy().astype(np.float64), xe=float(ref['xe_loss'].detach()), loss=float(data_loss(ref).detach()),
                total=float(ref['total_loss'].detach()), grads=oracle_grads(orc), neg_items=ref['neg_items'].numpy(), mask=ref['mask'].numpy(),
                div_e=ref['div_e'].detach().numpy().astype(np.float64) if 'div_e' in ref else None)


def oracle_on_row_shards(orc, f, l, buf, pop, neg_items, world):
    """The oracle called on `world` row shards separately, each with the whole batch's negatives for its rows and the global max time
    stamp, its loss rescaled to the global denominator, the gradients summed: a sharded step WITHOUT global first-batch statistics (on
    an empty recent-clicks buffer every call takes them from its own rows).  -> (logits of the rows concatenated, summed gradients)."""
    from chameleon_recsys_amd.nar import parallel
    for v in orc.w.values():
        v.grad = None
    n = np.asarray(f['item_clicked']).shape[0]
    g_mask, max_ts = float(valid_mask(f).sum()), int(np.asarray(f['event_timestamp']).max())
    logits = []
    for r in range(world):
        b, e = parallel.shard_rows(n, r, world)
        fl, ll = parallel.slice_batch(f, l, b, e)
        ref = orc.forward(fl, ll, buf, pop, 'train', neg_items=neg_items[b:e], global_max_ts=max_ts)
        (data_loss(ref) * (float(valid_mask(fl).sum()) / g_mask)).backward()          # gradients accumulate over the shards
        logits.append(ref['logits'].detach().numpy().astype(np.float64))
    return np.concatenate(logits), oracle_grads(orc)


# ---- the bound -------------------------------------------------------------------------------------------------------------------------
def _pack64(L, logical):
    """Logical float64 tensors -> the flat layout (float32 storage: the caller packs DIFFERENCES, whose rounding to float32 is 2^-24 of
    themselves, and magnitudes)."""
    return L.pack({k: np.asarray(v, np.float64) for k, v in logical.items()}).astype(np.float64)


def oracle_deviation(L, g32, g64):
    """name -> (max |g_oracle32 - g_oracle64|, max |g_oracle64|) per layout entry from the two oracle gradients (logical dicts)."""
    dev = _pack64(L, {k: np.asarray(g32[k], np.float64) - np.asarray(g64[k], np.float64) for k in g64})
    ref = _pack64(L, g64)
    return OrderedDict((name, (float(np.abs(dev[e.offset:e.offset + e.size]).max()), float(np.abs(ref[e.offset:e.offset + e.size]).max())))
                       for name, e in L.entries.items())


ZERO_GRADIENT_ENTRIES = ('bs4',)          # the only entries that may be treated as below


def zero_gradient_entries(L, g64):
    """Entries whose TRUE gradient is identically zero - bs4: the softmax is shift invariant, sum_c (p_c - y_c) = 0 at every click -
    recognised as tests/test_g1shape_parity_gpu.py does: largest float64 magnitude below 1e-5 of the model's largest gradient.  Asserted
    to be bs4 and nothing else: any other entry that small is a finding, not a case for another bound."""
    ref = _pack64(L, g64)
    gmax = float(np.abs(ref).max())
    zero = [n for n, e in L.entries.items() if e.size and float(np.abs(ref[e.offset:e.offset + e.size]).max()) < 1e-5 * gmax]
    assert set(zero) <= set(ZERO_GRADIENT_ENTRIES), zero
    return zero


def entry_bounds(L, g32, g64, factors=None):
    """name -> bound per layout entry; `factors`: the entries whose factor was raised (capped by the step-parity bound).  bs4, whose true
    gradient is identically zero, holds on every side the roundoff of a sum over all candidate rows whose terms cancel: both oracle
    figures are ~0 (the float32 oracle's can be exactly 0), so no finite factor on them describes that roundoff - measured on the GPU
    3e-9 ... 5e-8, ratios of 1e6 and more.  It is held to the ceiling no raised factor may pass, the step-parity bound
    3e-4 x max|ref| + 2e-5 = 2e-5."""
    out = OrderedDict()
    zero = zero_gradient_entries(L, g64)
    for name, (dev, scale) in oracle_deviation(L, g32, g64).items():
        f = (factors or {}).get(name, FACTOR)
        bound = max(f * dev, 8.0 * U * scale)
        out[name] = min(bound, 3e-4 * scale + 2e-5) if f > FACTOR else bound
        if name in zero:
            out[name] = 3e-4 * scale + 2e-5
    return out


def entry_deviations(L, flat_a, flat_b):
    """name -> max |a - b| over the entry, for two flat gradient images."""
    a, b = (np.asarray(x.detach().cpu().numpy() if hasattr(x, 'detach') else x, np.float64) for x in (flat_a, flat_b))
    return OrderedDict((name, float(np.abs(a[e.offset:e.offset + e.size] - b[e.offset:e.offset + e.size]).max())) for name, e in L.entries.items())


def check_entries(L, flat_sum, flat_full, g32, g64, factors=None, label=''):
    """Asserts the per-entry bound and returns name -> ratio of the deviation to the un-factored oracle deviation (the floor included)."""
    bounds = entry_bounds(L, g32, g64, factors)
    unit = oracle_deviation(L, g32, g64)
    devs = entry_deviations(L, flat_sum, flat_full)
    # the ratio is quoted against the oracle deviation with the floor at factor 4 folded in: an entry at the floor reads 4.0
    zero = zero_gradient_entries(L, g64)
    ratios = OrderedDict((n, devs[n] / max(unit[n][0], 8.0 * U * unit[n][1] / FACTOR, 1e-300)) for n in devs if n not in zero)
    for n in zero:
        print("%s zero-gradient entry %s: |g_sum - g_full| %.2e (bound %.2e)" % (label, n, devs[n], bounds[n]))
    worst = max(ratios, key=lambda n: ratios[n])
    print("%s per-entry |g_sum - g_full| / oracle deviation: worst %.2f (%s); above 1: %s" % (
        label, ratios[worst], worst, ", ".join("%s %.2f" % (n, r) for n, r in ratios.items() if r > 1.0) or "none"))
    bad = [(n, devs[n], bounds[n], ratios[n]) for n in devs if devs[n] > bounds[n]]
    assert not bad, "%s entries outside the bound (name, deviation, bound, ratio): %r" % (label, bad)
    return ratios
