"""numpy model of full-candidate evaluation, from a score matrix, the label's score per chunk, the candidate set, the
sessions' ids and the labels; and the shared tiny batch of the model-level tests (host only: no GPU, no HIP library).

    competitors(p) = { c in cand : c != l and c not in aci[b, :] }
    full_rank(p)   = #{ c in competitors(p) : not (z_c < z_l or (z_c == z_l and c > l)) }      z_l: the label's score in c's chunk

Scores are compared as given (the caller passes the float32 values); a NaN on either side makes the comparison false, i.e. counts against
the label.  Padded positions (label 0) have rank -1 and 0 competitors."""
import functools

import numpy as np

from tests.predict_reference import candidate_set      # noqa: F401  (the same set: distinct ids in [1, n_items) of the buffer, ascending)


def competitors(cand, aci_row, label):
    """bool [K]: the candidates the click's label is ranked against."""
    cand = np.asarray(cand, dtype=np.int64)
    return (cand != label) & ~np.isin(cand, np.asarray(aci_row, dtype=np.int64))


def full_rank(scores, label_scores, Nc, cand, aci_row, label):
    """(rank, number of competitors) of one click: scores [K], label_scores [ceil(K / Nc)] = the label's score beside chunk j."""
    cand = np.asarray(cand, dtype=np.int64)
    comp = competitors(cand, aci_row, label)
    rank = 0
    for i in np.flatnonzero(comp):
        z, zl, c = scores[i], label_scores[i // Nc], int(cand[i])
        below = bool(z < zl) or (bool(z == zl) and c > int(label))
        rank += 0 if below else 1
    return rank, int(comp.sum())


def full_ranks(scores, label_scores, Nc, cand, aci, labels):
    """scores [B, T, K], label_scores [B, T, chunks], aci [B, T + 1], labels [B, T] -> (rank int32 [B, T], competitors int32 [B, T])."""
    labels = np.asarray(labels, dtype=np.int64)
    B, T = labels.shape
    rank, comp = np.full((B, T), -1, np.int32), np.zeros((B, T), np.int32)
    for b in range(B):
        for t in range(T):
            if labels[b, t] != 0:
                rank[b, t], comp[b, t] = full_rank(scores[b, t], label_scores[b, t], Nc, cand, aci[b], labels[b, t])      # (K = 0: rank 0)
    return rank, comp


def bracket(z, zl, cand, aci_row, label, beta):
    """[lo, hi] = [#(z_c - z_l > 2 beta), #(z_c - z_l >= -2 beta)] over the click's competitors: every rank a path whose logits are within
    beta of z, zl (float64 reference values) can report, whatever the tie rule."""
    comp = competitors(cand, aci_row, label)
    diff = np.asarray(z, np.float64)[comp] - float(zl)
    return int((diff > 2 * beta).sum()), int((diff >= -2 * beta).sum())


# ---------------------------------------------------------------------------------------------------- the shared batch
ARMS = [('f32', 256), ('f32_native', 128), ('bf16', 128)]          # (gemm_dtype, CAR width), as tests/test_predict_gpu.py
BOUND = {'f32': 1e-3, 'f32_native': 1e-3, 'bf16': 4e-3}           # the arms' logit bounds of tests/test_predict_gpu.py
SEED, N_ITEMS = 29, 1000


def params(arm, C):
    from tests import helpers as H
    return H.tiny_params(C=C, gemm_dtype=arm, batch_size=8)


@functools.lru_cache(maxsize=None)
def case(seed=SEED):
    """(features, labels of the evaluated batch, recent-clicks buffer, pop_norm, cand, aci): three batches of 8 sessions, the state fed from
    the first two, the third evaluated.  Seed 29: B 8, T 7, K 16, 29 valid clicks."""
    from chameleon_recsys_amd.nar import synthetic
    from tests import helpers as H
    p = params('f32', 128)
    batches = synthetic.make_batches(3, 8, 8, N_ITEMS, p['session_features_config'], length_dist='g1', seed=seed)
    st = H.warm_state(p, batches[:2])
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    f, l = batches[2]
    aci = np.concatenate([np.asarray(f['item_clicked'], np.int64), np.asarray(l['label_last_item'], np.int64).reshape(-1, 1)], 1)
    return f, l, buf, pop, candidate_set(buf, N_ITEMS), aci


@functools.lru_cache(maxsize=None)
def oracle_logits(arm, C, seed=SEED):
    """Oracle EVAL logits float64 [B, T, 1 + K]: column 0 the label, column 1 + i candidate i as a negative of every click."""
    import torch
    from oracle.nar_oracle import NAROracle
    from tests import helpers as H
    f, l, buf, pop, cand, _ = case(seed)
    p = params(arm, C)
    B, T = f['item_clicked'].shape
    neg = np.broadcast_to(cand, (B, T, cand.shape[0])).copy()
    with torch.no_grad():
        ref = NAROracle(p, weights=H.pair_weights(p)).forward(f, l, buf, pop, mode='eval', neg_items=neg)
    return ref['logits'].numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def oracle_brackets(arm, C, seed=SEED):
    """(lo int [B, T], hi int [B, T]; -1 at padded positions) of every click's rank under the arm's logit bound."""
    f, l, _, _, cand, aci = case(seed)
    lg = oracle_logits(arm, C, seed)
    labels = np.asarray(l['label_next_item'], np.int64)
    lo, hi = np.full(labels.shape, -1), np.full(labels.shape, -1)
    for b, t in zip(*np.nonzero(labels)):
        lo[b, t], hi[b, t] = bracket(lg[b, t, 1:], lg[b, t, 0], cand, aci[b], labels[b, t], BOUND[arm])
    return lo, hi
