"""The CPU oracle with the cosine ranking head (--recommendations_ranking cosine), for tests/test_cosine_cpu.py and
tests/test_cosine_gpu.py: a test-side subclass of NAROracle, as tests/lstm_oracle.py and tests/diversity_oracle.py are.

NAROracle.forward hands `_scorer` only the product cand (.) pred, so the subclass lets that call return zeros and restates the scoring
stage from the tensors the base forward returns (car_pos, car_neg, pred - all part of the autograd graph):
    logit_c = cos(pred, CAR row of candidate c), both l2-normalised as tf.nn.l2_normalize does    (nar_model.py:435-437)
    probs = softmax(logits / tau); xe, L2, novelty and diversity terms exactly as NAROracle / DiversityOracle state them.
The match1..4 variables do not exist in this mode: they are removed from the specs, the weights and the Adam slots."""
from collections import OrderedDict

import numpy as np
import torch

from oracle.nar_oracle import NAROracle, init_params
from tests.cosine_reference import cosine
from tests.diversity_oracle import diversity_e


def _is_match(name):
    return name.startswith('match')


class CosineOracle(NAROracle):
    def __init__(self, params, weights=None, seed=42, **kw):
        if weights is not None and not any(_is_match(k) for k in weights):      # the base constructor wants every variable of the MLP model
            full = init_params(params, seed)
            weights = OrderedDict((k, weights[k] if k in weights else full[k]) for k in full)
        NAROracle.__init__(self, params, weights=weights, seed=seed, **kw)
        for d in (self.specs, self.w, self.m, self.v):
            for k in [k for k in d if _is_match(k)]:
                del d[k]

    def _scorer(self, m):
        return m.sum(-1, keepdim=True) * 0.0

    def forward(self, features, labels, buffer_ids, pop_norm, mode='train', *args, **kw):
        out = NAROracle.forward(self, features, labels, buffer_ids, pop_norm, mode, *args, **kw)
        p = self.p
        cand = torch.cat([out['car_pos'].unsqueeze(2), out['car_neg']], 2)            # [B, T, 1 + N, C]
        logits, _, _ = cosine(cand, out['pred'])
        tau = self._c(float(p['softmax_temperature']))
        probs = torch.softmax(logits / tau, dim=-1)
        mask = out['mask'].to(self.dt)
        xe = -(torch.log(probs[:, :, 0]) * mask).sum() / mask.sum()
        reg = self.reg_loss()
        total = xe + reg
        neg = out['neg_items']
        if p.get('novelty_reg_factor', 0.0) > 0.0:
            pop_t = torch.as_tensor(np.asarray(pop_norm, dtype=np.float32)).to(self.dt)
            neg_prob = torch.softmax(logits[:, :, 1:] / tau, dim=-1)
            neg_nov = -(torch.log(pop_t[neg]) / torch.log(self._c(float(p.get('popularity_smooth_log_base', 2.0)))))
            total = total - (p['novelty_reg_factor'] * (neg_prob * neg_nov * mask.unsqueeze(-1)).sum(-1)).sum() / mask.sum()
        label_next = torch.as_tensor(labels['label_next_item']).long()
        ids = torch.cat([label_next.unsqueeze(-1), neg], 2)
        f = float(p.get('diversity_reg_factor', 0.0))
        if f > 0.0:
            e = diversity_e(probs, ids, self.ace)
            out['div_e'] = e
            out['diversity_loss'] = self._c(f) * (e * mask).sum() / mask.sum()
            total = total + out['diversity_loss']
        out.update(total_loss=total, xe_loss=xe, reg_loss=reg, logits=logits, probs=probs)
        if mode != 'train':
            order = torch.sort(probs, dim=-1, descending=True, stable=True).indices
            out['predicted_item_ids'] = torch.gather(ids, 2, order)
            out['predicted_item_probs'] = torch.gather(probs, 2, order)
        return out


def label_rank(probs):
    """Rank of candidate 0 under the descending stable sort (lowest index wins ties): what cham_rank_items reports."""
    probs = np.asarray(probs)
    return (probs[..., 1:] > probs[..., :1]).sum(-1)


def pair_weights(p, seed=3):
    """helpers.pair_weights for the parameter layout of p['recommendations_ranking'] (host only)."""
    from chameleon_recsys_amd.nar.layout import ParamLayout
    acfg, ace = p['articles_features_config'], p['content_article_embeddings_matrix']
    n_items = acfg['article_id'].get('cardinality', ace.shape[0]) if 'article_id' in acfg else ace.shape[0]
    L = ParamLayout(p['session_features_config'], acfg, n_items, ace.shape[1], p['CAR_embedding_size'], p['rnn_units'],
                    p.get('rnn_num_layers', 1), p.get('rnn_cell', 'ugrnn'), p.get('internal_features_config'),
                    p.get('max_cardinality_for_ohe', 10), p.get('recommendations_ranking', 'mlp'))
    w = L.unpack(L.pack(L.init_logical(seed)))
    rng = np.random.default_rng(seed)
    for k in w:
        if k.endswith('bias') or k == 'beta':
            w[k] = (0.05 * rng.standard_normal(w[k].shape)).astype(np.float32)
        if k == 'gamma':
            w[k] = (1.0 + 0.1 * rng.standard_normal(w[k].shape)).astype(np.float32)
    return w


def make_model(p, rt, mode=None):
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel
    mode = ModeKeys.TRAIN if mode is None else mode
    train = mode == ModeKeys.TRAIN
    return NARModuleModel(mode, None, None, p['session_features_config'], p['articles_features_config'],
                          p['batch_size'], p['lr'], p.get('dropout_keep_prob', 1.0) if train else 1.0,
                          p['train_total_negative_samples' if train else 'eval_total_negative_samples'],
                          p['train_negative_samples_from_buffer' if train else 'eval_negative_samples_from_buffer'],
                          p['content_article_embeddings_matrix'],
                          softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                          recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                          recent_clicks_for_normalization=p['recent_clicks_for_normalization'],
                          articles_metadata=p['articles_metadata'], CAR_embedding_size=p['CAR_embedding_size'],
                          rnn_units=p['rnn_units'], novelty_reg_factor=p.get('novelty_reg_factor', 0.0),
                          diversity_reg_factor=p.get('diversity_reg_factor', 0.0), runtime=rt,
                          rnn_num_layers=p.get('rnn_num_layers', 1), rnn_cell=p.get('rnn_cell', 'ugrnn'), gemm_dtype=p.get('gemm_dtype', 'f32'),
                          recommendations_ranking=p.get('recommendations_ranking', 'mlp'))


def make_pair(p, seed=3, oracle_dtype=torch.float32):
    """(HIP NARModuleModel(train), CosineOracle) sharing pair_weights(p, seed); p['recommendations_ranking'] must be 'cosine'."""
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    w = pair_weights(p, seed)
    rt = NARRuntime(p, seed=seed, weights=w)
    return make_model(p, rt), CosineOracle(p, weights=w, dtype=oracle_dtype)


# ---- evaluation: the HIP label_rank equals the oracle's wherever the oracle's probabilities separate the label from every other candidate
# by more than twice the forward tolerance.  Chosen on the CPU so that the condition leaves out at most 10 % of the valid clicks for the
# ORACLE alone: with untrained weights the cosines of a click's candidates spread by ~0.06, so each competitor falls inside the +-2e-3
# window of the label's probability with a few per cent probability - ten negatives leave out 10-20 % of the clicks whatever tau and seed,
# five negatives at tau 0.07 and weight seed 6 leave out 1.5 % (tests/test_cosine_cpu.py recomputes the share).
EVAL = dict(tau=0.07, weight_seed=6, neg=5, n_warm=3, max_excluded=0.10)


def eval_setup():
    """(params, warmed ClickedItemsState, the evaluation batch)."""
    from chameleon_recsys_amd.nar import synthetic
    from tests import helpers as H
    p = H.tiny_params(recommendations_ranking='cosine', softmax_temperature=EVAL['tau'], neg=EVAL['neg'])
    batches = synthetic.make_batches(EVAL['n_warm'] + 1, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    return p, H.warm_state(p, batches[:EVAL['n_warm']]), batches[EVAL['n_warm']]


def separated_clicks(probs, mask, gap):
    """Valid clicks whose label probability differs from every other candidate's by more than `gap`."""
    probs = np.asarray(probs, np.float64)
    return np.asarray(mask, bool) & (np.abs(probs[..., 1:] - probs[..., :1]).min(-1) > gap)
