"""Content-diversity regulariser (--diversity_reg_factor), host side: the three entry points exist in the header, the built library and the
ctypes table, and the test oracle's term (explicit similarity matrix, tests/diversity_oracle.py) and its autograd logit gradient equal the
closed form the HIP kernels evaluate (csrc/diversity.hip) in float64."""
import ctypes
import os
import re

import numpy as np
import torch

from chameleon_recsys_amd import _lib
from tests import diversity_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cham_diversity_fwd", "cham_diversity_bwd", "cham_diversity_bwd_b16")


def test_entry_points_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chameleon_nar.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cham_\w+)\s*\(", src))
    assert os.path.exists(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'` first"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in SYMBOLS:
        assert n in declared, "%s is not declared in include/chameleon_nar.h" % n
        assert hasattr(lib, n), "%s is not exported by the built library" % n
        assert n in _lib._SIGNATURES, "%s is missing from the ctypes table" % n
    # (probs, label_ids, neg_ids, mask, BT, N, ace, ld_ace, D, n_items, factor, sp, e, nll, stream)
    assert len(_lib._SIGNATURES["cham_diversity_fwd"][1]) == 15
    assert _lib._SIGNATURES["cham_diversity_bwd"] == _lib._SIGNATURES["cham_diversity_bwd_b16"]


def edge_case(dtype=torch.float64, seed=0):
    """[B=2, T=3] clicks of NC = 7 candidates over a 12-article table of D = 5: duplicate ids inside a click, a label equal to a negative,
    zero-padded negatives (id 0, whose row is NOT zero here: equal ids have similarity 0 whatever the row), an all-zero row (id 3), a
    near-zero row (id 4: norm^2 below 1e-12) and a masked position."""
    g = torch.Generator().manual_seed(seed)
    ace = torch.randn(12, 5, generator=g, dtype=torch.float64)
    ace[3] = 0.0
    ace[4] = 1e-8 * torch.randn(5, generator=g, dtype=torch.float64)
    ids = torch.tensor([[[5, 1, 2, 5, 7, 0, 0], [6, 6, 3, 4, 8, 9, 9], [1, 3, 3, 4, 4, 0, 0]],
                        [[2, 10, 11, 2, 2, 1, 0], [0, 0, 0, 0, 0, 0, 0], [9, 8, 7, 6, 5, 4, 3]]])
    mask = torch.tensor([[True, True, False], [True, True, True]])
    logits = torch.randn(2, 3, 7, generator=g, dtype=torch.float64)
    return ace.to(dtype), ids, mask, logits.to(dtype)


def test_oracle_term_and_logit_gradient_equal_the_closed_form():
    ace, ids, mask, logits = edge_case()
    factor, tau = 0.7, 0.1
    logits.requires_grad_(True)
    probs = torch.softmax(logits / tau, -1)
    e = DO.diversity_e(probs, ids, ace)
    mk = mask.to(torch.float64)
    loss = factor * (e * mk).sum() / mk.sum()
    loss.backward()
    sp, e2, gx = DO.diversity_closed_form(probs.detach(), ids, ace, mask, factor, tau)
    S = DO.similarity(ids, ace)
    assert float((S.diagonal(dim1=-2, dim2=-1)).abs().max()) == 0.0
    assert float(S[0, 0, 0, 3]) == 0.0 and float(S[0, 0, 5, 6]) == 0.0            # equal ids: the label and a negative, two paddings
    assert float(S[0, 1, 2].abs().max()) == 0.0                                      # the all-zero row is similar to nothing
    assert float((sp - (S @ probs.detach().unsqueeze(-1)).squeeze(-1)).abs().max()) < 1e-12
    assert float((e2 - e.detach()).abs().max()) < 1e-12
    assert float(e.detach()[1, 1]) == 0.0                                            # a click of one id only
    assert float((gx - logits.grad).abs().max()) < 1e-12
    assert float(gx[0, 2].abs().max()) == 0.0 and float(logits.grad[0, 2].abs().max()) == 0.0      # the masked position
    assert float(gx.abs().max()) > 1e-3                                              # ... and the comparison is not one of zeros


def test_oracle_forward_adds_the_term_to_the_total_loss():
    """DiversityOracle.forward: total = xe + reg + factor * sum(mask e) / sum(mask), div_e from its own probs; factor 0 is NAROracle."""
    from chameleon_recsys_amd.nar import synthetic
    from oracle.nar_oracle import NAROracle
    from tests import helpers as H
    p = H.tiny_params(diversity_reg_factor=0.5, content_article_embeddings_matrix=DO.clustered_ace(1000, 64))
    f, l = synthetic.make_batches(1, 16, 8, 1000, p['session_features_config'], length_dist='g1')[0]
    st = H.warm_state(p, [])
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    w = H.pair_weights(p)
    out = DO.DiversityOracle(p, weights=w).forward(f, l, buf, pop, 'train')
    ref = NAROracle(dict(p, diversity_reg_factor=0.0), weights=w).forward(f, l, buf, pop, 'train')
    mask = out['mask'].float()
    want = 0.5 * float((out['div_e'].detach() * mask).sum() / mask.sum())
    assert want > 1e-3
    assert abs(float(out['total_loss'].detach()) - float(ref['total_loss'].detach()) - want) < 1e-5
    assert float(out['xe_loss'].detach()) == float(ref['xe_loss'].detach())
    plain = DO.DiversityOracle(dict(p, diversity_reg_factor=0.0), weights=w).forward(f, l, buf, pop, 'train')
    assert 'div_e' not in plain and float(plain['total_loss'].detach()) == float(ref['total_loss'].detach())


def test_recorded_oracle_decrease_of_the_trained_term():
    """The two values tests/test_diversity_gpu.py holds the HIP model against: DiversityOracle trained with the factor ends at least 10 %
    lower on the held-out batch than trained without it."""
    t = DO.TRAINED
    e_plain, e_reg = DO.oracle_heldout_div_e(0.0), DO.oracle_heldout_div_e(t['factor'])
    print("held-out mean div_e: factor 0 -> %.5f, factor %g -> %.5f" % (e_plain, t['factor'], e_reg))
    assert abs(e_plain - t['e_plain']) < 2e-3 and abs(e_reg - t['e_reg']) < 2e-3
    assert (e_plain - e_reg) / e_plain >= 0.10 and (t['e_plain'] - t['e_reg']) / t['e_plain'] >= 0.10
