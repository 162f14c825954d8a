"""The CPU oracle with the content-diversity regulariser (--diversity_reg_factor), for tests/test_diversity.py and
tests/test_diversity_gpu.py: a test-side subclass of NAROracle that adds the term to `total_loss` and nothing else.

The loss is the one the reference states in its commented-out block (nar_model.py:551-636, 685-702), per valid click with candidates
c = 0..N (0 the label, 1..N the sampled negatives), ids id_c and p = softmax(logits / tau):
    e^_c  = ACE[id_c] * rsqrt(max(sum_d ACE[id_c,d]^2, 1e-12))          (tf.nn.l2_normalize, :563)
    S_cc' = e^_c . e^_c' where id_c != id_c', 0 where the ids are equal   (:572-574: the diagonal of the UNIQUE-id similarity matrix)
    e     = p^T S p                                                       (:620-630, 689)
    diversity_reg_loss = factor * sum(mask e) / sum(mask)                 (:696-698; the reference's denominator sum(mask sum_j p_j) = sum(mask))
`diversity_e` forms S explicitly; `diversity_closed_form` is the O(NC D) restatement the HIP kernels use, with the logit gradient."""
import torch

from oracle.nar_oracle import NAROracle


def similarity(ids, ace):
    """S [..., NC, NC] of the candidates `ids` [..., NC] (int64) over the ACE matrix `ace` [n_items, D], in ace's dtype."""
    a = ace[ids]
    eh = a * torch.rsqrt(torch.clamp((a * a).sum(-1, keepdim=True), min=1e-12))
    S = eh @ eh.transpose(-1, -2)
    return torch.where(ids.unsqueeze(-1) == ids.unsqueeze(-2), torch.zeros_like(S), S)


def diversity_e(probs, ids, ace):
    """e [...] = p^T S p through the explicit S."""
    S = similarity(ids, ace)
    return (probs * (S @ probs.unsqueeze(-1)).squeeze(-1)).sum(-1)


def diversity_closed_form(probs, ids, ace, mask, factor, tau):
    """(sp [..., NC], e [...], gx [..., NC]) without S: (S p)_c = e^_c . m - |e^_c|^2 sum_{c': id_c' = id_c} p_c', m = sum_c p_c e^_c, and
    gx = d(factor * sum(mask e) / sum(mask)) / d logit_c = factor * mask / (tau sum(mask)) * 2 p_c ((S p)_c - e)."""
    a = ace[ids]
    eh = a * torch.rsqrt(torch.clamp((a * a).sum(-1, keepdim=True), min=1e-12))
    m = (probs.unsqueeze(-1) * eh).sum(-2)
    same = ((ids.unsqueeze(-1) == ids.unsqueeze(-2)).to(probs.dtype) * probs.unsqueeze(-2)).sum(-1)
    sp = (eh * m.unsqueeze(-2)).sum(-1) - (eh * eh).sum(-1) * same
    e = (probs * sp).sum(-1)
    mk = mask.to(probs.dtype)
    gx = factor * mk.unsqueeze(-1) / (tau * mk.sum()) * 2.0 * probs * (sp - e.unsqueeze(-1))
    return sp, e, gx


class DiversityOracle(NAROracle):
    def forward(self, features, labels, *args, **kw):
        out = NAROracle.forward(self, features, labels, *args, **kw)
        f = float(self.p.get('diversity_reg_factor', 0.0))
        if f > 0.0:
            ids = torch.cat([torch.as_tensor(labels['label_next_item']).long().unsqueeze(-1), out['neg_items']], 2)
            e = diversity_e(out['probs'], ids, self.ace)
            mask = out['mask'].to(self.dt)
            out['div_e'] = e
            out['diversity_loss'] = self._c(f) * (e * mask).sum() / mask.sum()
            out['total_loss'] = out['total_loss'] + out['diversity_loss']
        return out


def clustered_ace(n_items, ace_dim, n_clusters=4, noise=0.35, seed=5, scale=6.0):
    """An ACE matrix with content clusters: a few random unit centres + noise, row-normalised x scale as synthetic.make_catalog does.  (With
    independent random rows the off-diagonal similarity is O(1 / sqrt(D)) and the diversity term vanishes.)"""
    import numpy as np
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_clusters, ace_dim))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    ace = centres[rng.integers(0, n_clusters, size=n_items)] + noise * rng.standard_normal((n_items, ace_dim)) / np.sqrt(ace_dim)
    ace /= np.linalg.norm(ace, axis=1, keepdims=True)
    return (ace * scale).astype(np.float32)


def make_pair(p, seed=3, oracle_dtype=torch.float32):
    """helpers.make_pair with diversity_reg_factor passed on: (HIP NARModuleModel(train), DiversityOracle) sharing helpers.pair_weights."""
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    from tests.helpers import pair_weights
    w = pair_weights(p, seed)
    rt = NARRuntime(p, seed=seed, weights=w)
    model = NARModuleModel(ModeKeys.TRAIN, None, None, p['session_features_config'], p['articles_features_config'],
                           p['batch_size'], p['lr'], p.get('dropout_keep_prob', 1.0), p['train_total_negative_samples'],
                           p['train_negative_samples_from_buffer'], p['content_article_embeddings_matrix'],
                           softmax_temperature=p['softmax_temperature'], reg_weight_decay=p['reg_weight_decay'],
                           recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                           recent_clicks_for_normalization=p['recent_clicks_for_normalization'],
                           articles_metadata=p['articles_metadata'], CAR_embedding_size=p['CAR_embedding_size'],
                           rnn_units=p['rnn_units'], novelty_reg_factor=p.get('novelty_reg_factor', 0.0),
                           diversity_reg_factor=p.get('diversity_reg_factor', 0.0), runtime=rt,
                           rnn_num_layers=p.get('rnn_num_layers', 1), rnn_cell=p.get('rnn_cell', 'ugrnn'), gemm_dtype=p.get('gemm_dtype', 'f32'),
                           elapsed_days_smooth_log_base=p.get('elapsed_days_smooth_log_base', 1.3),
                           popularity_smooth_log_base=p.get('popularity_smooth_log_base', 2.0))
    return model, DiversityOracle(p, weights=w, dtype=oracle_dtype)


# ---- "training with the factor lowers the term": twenty tiny steps, then p^T S p on one held-out batch ---------------------------------
# Chosen on the CPU with DiversityOracle (fp32): lr 1e-3 and factor 1.0 lower the held-out mask-weighted mean of div_e from E_PLAIN
# (factor 0) to E_REG, a relative decrease of 20 %; tests/test_diversity.py recomputes both, profiles/diversity_notes.md records them.
TRAINED = dict(factor=1.0, lr=1e-3, steps=20, e_plain=0.18549, e_reg=0.14807)


def trained_setup(factor):
    """(params, warmed ClickedItemsState, the training batches, the held-out batch) of the run above with `factor`."""
    from chameleon_recsys_amd.nar import synthetic
    from tests import helpers as H
    p = H.tiny_params(diversity_reg_factor=factor, content_article_embeddings_matrix=clustered_ace(1000, 64), lr=TRAINED['lr'])
    n = TRAINED['steps']
    batches = synthetic.make_batches(n + 3, 64, 8, 1000, p['session_features_config'], length_dist='g1')
    return p, H.warm_state(p, batches[:2]), batches[2:2 + n], batches[2 + n]


def masked_mean(e, mask):
    import numpy as np
    e, mask = np.asarray(e, np.float64), np.asarray(mask, np.float64)
    return float((e * mask).sum() / mask.sum())


def oracle_heldout_div_e(factor):
    """Mask-weighted mean of div_e on the held-out batch after DiversityOracle trained with `factor`."""
    from tests import helpers as H
    p, st, train, held = trained_setup(factor)
    orc = DiversityOracle(p, weights=H.pair_weights(p))
    for f, l in train:
        orc.train_step(f, l, st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy())
        H.update_state(st, f, l)
    orc.p = dict(p, diversity_reg_factor=TRAINED['factor'])          # (the term is measured whatever the run trained with)
    with torch.no_grad():
        out = orc.forward(*held, st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy(), 'train')
    return masked_mean(out['div_e'].numpy(), out['mask'].numpy())
