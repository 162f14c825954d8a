"""Cosine ranking head (--recommendations_ranking cosine), host side: the closed-form gradients the HIP kernels evaluate (csrc/cosine.hip)
equal float64 autograd - clamp regime included -, the bound the two-plane arm builds its scale record from holds, the parameter layout
of the mode has no scorer variables, the trainers thread the flag into `params`, and the unsupported arm is refused."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd.nar import synthetic
from chameleon_recsys_amd.nar.layout import ParamLayout
from tests import cosine_oracle as CO
from tests import cosine_reference as CR
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("cham_cosine_fwd", "cham_cosine_fwd_b16", "cham_cosine_bound", "cham_cosine_bwd", "cham_cosine_bwd_h2", "cham_cosine_bwd_b16")


def test_entry_points_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "chameleon_nar.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cham_\w+)\s*\(", src))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in SYMBOLS:
        assert n in declared and hasattr(lib, n) and n in _lib._SIGNATURES, n
    assert _lib._SIGNATURES["cham_cosine_fwd"] == _lib._SIGNATURES["cham_cosine_fwd_b16"]
    assert _lib._SIGNATURES["cham_cosine_bwd"] == _lib._SIGNATURES["cham_cosine_bwd_b16"]


@pytest.mark.parametrize("BT,NC,C", [(1, 2, 128), (5, 5, 132), (3, 65, 128)])
def test_closed_form_gradients_equal_autograd(BT, NC, C):
    """Random rows + an exact-zero candidate row, a row with sum z^2 < 1e-12, a zero pred and a masked click (ds = 0)."""
    z, p, ds, _ = CR.make_case(BT, NC, C, seed=1, dtype=torch.float64)
    cos, gz, gp = CR.autograd_grads(z, p, ds)
    cf = CR.closed_form(z, p, ds)
    assert float((cf['cos'] - cos).abs().max()) < 1e-14
    sz, sp = max(1.0, float(gz.abs().max())), max(1.0, float(gp.abs().max()))
    assert float((cf['dz'] - gz).abs().max()) < 1e-12 * sz
    assert float((cf['dp'] - gp).abs().max()) < 1e-12 * sp
    assert float(gz.abs().max()) > 1e-3 and float(gp.abs().max()) > 1e-3           # ... and the comparison is not one of zeros
    # the clamp regime: inverse norm exactly 1e6, no projection term
    assert float(cf['rz'][0, 0]) == 1e6 and float(cf['rz'][0, NC - 1]) == 1e6
    assert float(cf['cos'][0, 0]) == 0.0 and float(cf['dz'][0, 0].abs().max()) > 0.0       # a zero row still receives ds rz p^ (1 - 0)
    want = ds[0, NC - 1].double() * 1e6 * (p[0] * cf['rp'][0]) * (1.0 - 1e-16)
    assert float((cf['dz'][0, NC - 1] - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if BT > 1:
        assert float(cf['rp'][BT - 1]) == 1e6 and float(cf['cos'][BT - 1].abs().max()) == 0.0
        assert float(cf['dz'][BT - 1].abs().max()) == 0.0                              # p^ = 0 and cos = 0
        assert float(cf['dp'][BT - 1].abs().max()) > 0.0                               # sum_c ds_c 1e6 z^_c
    if BT >= 3:
        assert float(cf['dz'][1].abs().max()) == 0.0 and float(cf['dp'][1].abs().max()) == 0.0


def test_bound_of_the_two_plane_scale_record_holds():
    """|dZ2pre_ck| <= max_r |ds_r| rz_r: |p^_k - cos z^_k| <= sin of the angle between the unit vectors, |p^_k| <= 1 in the clamp regime."""
    for seed in range(6):
        BT, NC, C = 4, 7, 36
        z, p, ds, _ = CR.make_case(BT, NC, C, seed=seed, special=seed % 2 == 0, dtype=torch.float64)
        if seed == 3:
            z[2, 1] = -p[2]             # anti-parallel and (next) parallel rows: the projection removes everything
            z[2, 2] = 0.5 * p[2]
        cf = CR.closed_form(z, p, ds)
        bound = float((ds.abs() * cf['rz']).max())
        assert float(cf['dz'].abs().max()) <= bound * (1.0 + 1e-12)
        assert float((cf['dz'].abs().amax(-1) - ds.abs() * cf['rz']).max()) <= 1e-12 * bound      # ... row by row
    # and in float32, as the kernels evaluate it: no element leaves the record's bound by more than rounding
    z, p, ds, _ = CR.make_case(5, 9, 64, seed=11)
    cf32 = CR.closed_form(z, p, ds)
    assert float(cf32['dz'].abs().max()) <= float((ds.double().abs() * cf32['rz']).max()) * (1.0 + 1e-6)


def _layout(p, ranking):
    return ParamLayout(p['session_features_config'], p['articles_features_config'], 1000, 64, p['CAR_embedding_size'], p['rnn_units'],
                       recommendations_ranking=ranking)


def test_param_layout_of_the_cosine_mode():
    p = H.tiny_params()
    mlp, cos = _layout(p, 'mlp'), _layout(p, 'cosine')
    assert not [n for n in cos.entries if n.startswith(('Ws', 'bs'))]
    assert [n for n in mlp.entries if n not in cos.entries] == ['Ws1', 'Ws2', 'Ws3', 'Ws4', 'bs1', 'bs2', 'bs3', 'bs4']
    C = p['CAR_embedding_size']
    assert mlp.n_reg - cos.n_reg == C * 128 + 128 * 64 + 64 * 32 + 32
    assert not [k for k in cos.logical_specs() if k.startswith('match')]
    assert not [k for k in cos.tf_variable_names() if 'matching_dense_layer' in k] and not cos.tf_variable_aliases().keys() & set(
        k for k in mlp.tf_variable_aliases() if 'matching' in k)
    assert len(mlp.tf_variable_names()) - len(cos.tf_variable_names()) == 8
    # every offset is consistent and the regularised tensors are still a prefix
    off = 0
    for e in cos.entries.values():
        assert e.offset == off
        off += e.size
    assert cos.total >= off and cos.total % 256 == 0
    # pack / unpack round trip, through the TF names too
    w = cos.init_logical(7)
    rng = np.random.default_rng(0)
    w = {k: (v + rng.standard_normal(v.shape).astype(np.float32)) for k, v in w.items()}
    back = cos.unpack(cos.pack(w))
    assert list(back) == list(cos.logical_specs())
    assert all(np.array_equal(back[k], w[k]) for k in w)
    again = cos.from_tf_variables(cos.to_tf_variables(back))
    assert all(np.array_equal(again[k], w[k]) for k in w)
    assert mlp.fingerprint() != cos.fingerprint()
    with pytest.raises(ValueError, match="recommendations_ranking"):
        _layout(p, 'dot')
    # the default is the MLP head, unchanged
    assert ParamLayout(p['session_features_config'], p['articles_features_config'], 1000, 64, C, p['rnn_units']).fingerprint() == mlp.fingerprint()


def test_state_dicts_of_the_two_modes_do_not_cross_load():
    """NARRuntime.load_state_dict compares the layout fingerprints (no device needed for the check itself)."""
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    p = H.tiny_params()
    for a, b in (('mlp', 'cosine'), ('cosine', 'mlp')):
        src, dst = _layout(p, a), _layout(p, b)
        sd = dict(flat=torch.zeros(src.total), m=torch.zeros(src.total), v=torch.zeros(src.total), global_step=3, layout=src.fingerprint())
        rt = NARRuntime.__new__(NARRuntime)
        rt.layout, rt.flat = dst, torch.zeros(dst.total)
        with pytest.raises(ValueError, match="different parameter layout"):
            rt.load_state_dict(sd)


def test_cosine_oracle_has_no_scorer_variables_and_scores_by_cosine():
    p = H.tiny_params(recommendations_ranking='cosine')
    f, l = synthetic.make_batches(1, 16, 8, 1000, p['session_features_config'], length_dist='g1')[0]
    st = H.warm_state(p, [])
    buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
    w = CO.pair_weights(p)
    assert not [k for k in w if k.startswith('match')]
    orc = CO.CosineOracle(p, weights=w)
    assert list(orc.w) == list(w) and list(orc.specs) == list(w)
    out = orc.forward(f, l, buf, pop, 'train')
    lg = out['logits'].detach()
    assert float(lg.abs().max()) <= 1.0 + 1e-6 and float(lg.std()) > 1e-3
    cand = torch.cat([out['car_pos'].unsqueeze(2), out['car_neg']], 2).detach().double()
    want = torch.nn.functional.cosine_similarity(cand, out['pred'].detach().double().unsqueeze(2), dim=-1)
    assert float((lg.double() - want).abs().max()) < 1e-5
    out['total_loss'].backward()
    assert all(v.grad is not None for k, v in orc.w.items() if k in ('CAR/kernel', 'FC2/kernel', 'PreCAR/kernel'))
    ev = orc.forward(f, l, buf, pop, 'eval')
    rank = CO.label_rank(ev['probs'].detach().numpy())
    lab = torch.as_tensor(l['label_next_item']).long()
    pos = (ev['predicted_item_ids'] == lab.unsqueeze(-1)).float().argmax(-1).numpy()
    m = ev['mask'].numpy()
    assert (pos[m] <= rank[m]).all()          # (a negative may carry the label's id: the first occurrence is at or before the label's rank)


def test_eval_rank_condition_leaves_out_few_clicks_for_the_oracle_alone():
    """tests/test_cosine_gpu.py compares label_rank on the clicks whose ORACLE probabilities separate the label from every other candidate by
    more than 2 x 1e-3; the set-up (cosine_oracle.EVAL) must make that at least 90 % of the valid clicks."""
    from chameleon_recsys_amd.nar.nar_model import NARModuleModel
    p, st, (f, l) = CO.eval_setup()
    orc = CO.CosineOracle(p, weights=CO.pair_weights(p, CO.EVAL['weight_seed']))
    with torch.no_grad():
        out = orc.forward(f, l, st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy(), mode='eval',
                          step=NARModuleModel.eval_step_key(0, 0))
    mask = out['mask'].numpy()
    sep = CO.separated_clicks(out['probs'].numpy(), mask, 2e-3)
    left_out = 1.0 - sep.sum() / mask.sum()
    print("valid clicks %d, left out %.3f" % (mask.sum(), left_out))
    assert mask.sum() >= 150 and left_out <= CO.EVAL['max_excluded']
    ranks = CO.label_rank(out['probs'].numpy())[sep]
    assert len(set(ranks.tolist())) >= 4          # ... and the ranks compared are not all the same


@pytest.mark.parametrize("module", ["nar_trainer_gcom", "nar_trainer_adressa"])
def test_trainers_parse_the_flag_and_pass_it_into_params(module, monkeypatch):
    import importlib
    from chameleon_recsys_amd.nar import nar_trainer_gcom as base
    mod = importlib.import_module("chameleon_recsys_amd.nar." + module)
    ap = mod.define_flags()
    assert ap.parse_args([]).recommendations_ranking == 'mlp'
    flags = ap.parse_args(['--recommendations_ranking', 'cosine'])
    assert flags.recommendations_ranking == 'cosine'
    with pytest.raises(SystemExit):
        ap.parse_args(['--recommendations_ranking', 'dot'])
    help_text = ap.format_help()
    assert 'nar_model.py:435-437' in " ".join(help_text.split())
    monkeypatch.setattr(base, 'FLAGS', flags)
    p = H.tiny_params()
    est = base.build_estimator(None, p['content_article_embeddings_matrix'], p['articles_metadata'], p['articles_features_config'],
                               p['session_features_config'])
    assert est.params['recommendations_ranking'] == 'cosine'
    # ... and the model function hands it to the model
    seen = {}

    class Spy:
        def __init__(self, *a, **kw):
            seen.update(kw)
            raise RuntimeError("stop here")
    monkeypatch.setattr(base, 'NARModuleModel', Spy)
    with pytest.raises(RuntimeError, match="stop here"):
        base.nar_module_model_fn({}, {}, base.ModeKeys.TRAIN, dict(est.params, clicked_items_state=None))
    assert seen['recommendations_ranking'] == 'cosine'


def test_three_plane_arm_refuses_the_cosine_head(monkeypatch):
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    monkeypatch.setenv("CHAM_GEMM_H2", "0")
    p = H.tiny_params(C=256, recommendations_ranking='cosine')
    with pytest.raises(ValueError, match="three-bf16-plane"):
        NARRuntime(p)
