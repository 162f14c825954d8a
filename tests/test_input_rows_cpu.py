"""The input rows of the step (nar/input_rows.py) without a GPU: through a recording library, a recording gemm / colsum and a plan of small CPU
tensors, every launch of the feature front end, of the two forms of the PreCAR input layer and of their backward at B = 2, T = 3, N = 2 - its
order, its scalar arguments, and which buffer (and element offset) each pointer argument names.  The expected sequences are written out
here, not derived from the classes: they are what NARModuleModel._forward / backward launched before this code had a module of its own."""
import copy
import inspect
import re
import types

import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from chameleon_recsys_amd.nar.candidate_rows import F32Rows
from chameleon_recsys_amd.nar.input_rows import (SITE_FC1, SITE_INPUT_CLICKED, SITE_INPUT_NEGATIVE, SITE_INPUT_POSITIVE, SITE_RNN_OUT, DenseInput,
                                                 Dropout, FactorisedInput, FeatureRows, step_scalar)
from chameleon_recsys_amd.nar.layout import COL_ITEMEMB, ParamLayout
from chameleon_recsys_amd.nar.nar_model import NARModuleModel
from tests.recording import Recorder, S

B, T, N, NC, PMAX = 2, 3, 2, 3, 40
N_ITEMS, D, C, FC, FI, FW = 200, 16, 128, 72, 88, 160
MAX_TS, SUM_MASK, SEED, STEP, ROW_BEGIN = 1506830400123, 5.0, 42, 5, 4
# the synthetic G1 layout at 200 items: (kind, feature row, first column, width, cardinality, element offset of the table in flat / grads)
CTX_GROUPS = [(2, 2, 11, 17, 23, 0), (2, 3, 28, 14, 12, 392), (2, 4, 42, 18, 29, 560)]
ITEM_GROUPS = [(2, 0, 0, 37, 461, 1084), (COL_ITEMEMB, 0, 53, 30, 200, 18144)]
OFF = dict(gamma_ctx=24144, beta_ctx=24216, gamma_item=24288, beta_item=24376, W1c=24464, W1i=33680, b1=284592)
PARAMS = synthetic.default_params(N_ITEMS, D, C=C, H=255)
LAYOUT = ParamLayout(PARAMS['session_features_config'], PARAMS['articles_features_config'], N_ITEMS, D, C, 255, 1, 'ugrnn')
POSITIONS = [None, [0, 1, 3, 4]]          # all six positions valid; compacted to P = 4


def fl(name):
    return 'flat+%d' % OFF[name]


def gr(name):
    return 'grads+%d' % OFF[name]


def off(name, n):          # how the recorder names element n of a buffer
    return name if n == 0 else '%s+%d' % (name, n)


def test_the_layout_is_the_one_the_sequences_are_written_for():
    L = LAYOUT
    assert (L.Fc, L.Fi, L.f_ctx, L.D, L.C) == (FC, FI, 71, D, C)
    assert L.ctx_emb_groups() == CTX_GROUPS and L.item_emb_groups() == ITEM_GROUPS
    assert {n: L.entries[n].offset for n in OFF} == OFF
    segs, singles = L.item_segments()
    assert (segs.shape[0], singles.shape[0]) == (3, 5)


class Runtime(Recorder):
    """Stand-in for NARRuntime: the recording host + what the input rows read of a runtime.  Weights and gradients are views of ONE flat buffer
    each, as in the real one, so a pointer into them is logged as flat+offset / grads+offset."""

    def __init__(self, dev_scalars=True, feature_bwd_ws=True, L=LAYOUT):
        Recorder.__init__(self, L)
        self.layout, self.device, self.params, self.n_items, self.item_id_bits = L, torch.device('cpu'), PARAMS, N_ITEMS, 8
        self.dev_scalars, self.feature_bwd_ws, self.tf_random_seed, self.b16, self.lane = dev_scalars, feature_bwd_ws, SEED, False, ''
        self.flat, self.grads = self.name(torch.zeros(L.total), 'flat'), self.name(torch.zeros(L.total), 'grads')
        self.scalars = self.name(torch.zeros(8, dtype=torch.int32), 'scalars')
        for lane in ('', '_side', '_aux'):
            setattr(self, 'gemm_ws' + lane, self.name(torch.zeros(64), 'gemm_ws' + lane))
        self.p, self.g, self.stream = (lambda n: self.view(self.flat, n)), (lambda n: self.view(self.grads, n)), (lambda: S)
        self.lib.cham_combine_bwd_workspace_bytes = lambda *a: self.log.append(('cham_combine_bwd_workspace_bytes',) + a) or 4 * 96
        self.features = FeatureRows(self, np.ascontiguousarray(PARAMS['content_article_embeddings_matrix'], dtype=np.float32))
        self.precar = FactorisedInput(self)
        for n in ('ace', 'created', 'meta_cat', 'ctx_desc', 'item_desc', 'item_segs', 'item_singles'):
            self.name(getattr(self, n), n)

    def view(self, flat, name):
        e = self.layout.entries[name]
        return flat[e.offset:e.offset + int(np.prod(e.shape))].view(*e.shape)

    def _lane_ws(self, name):          # NARRuntime._lane_ws picks by the current stream; here the test says which lane is current
        return getattr(self, name + self.lane)


class Plan(types.SimpleNamespace):
    def ensure_rows(self, name):
        assert getattr(self, name).shape[0] >= self.Rall
        return getattr(self, name)


def make(positions=None, **kw):
    """(runtime, plan, batch) of a step with the valid positions `positions` (None: all B * T): the plan holds what StepPlan allocates for the
    input rows, at the plan's full size, + what FactorisedInput.alloc adds."""
    rt = Runtime(**kw)
    BT, P = B * T, B * T if positions is None else len(positions)
    f32, i64, i32 = (lambda *s: torch.zeros(*s)), (lambda *s: torch.zeros(*s, dtype=torch.int64)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    RV, Rall = 2 * BT + PMAX + 1, BT * (1 + NC)
    pl = Plan(B=B, T=T, N=N, NC=NC, BT=BT, Rc=BT * NC, Rall=Rall, pmax=PMAX, RV=RV, C=C, P=P, PC=P * NC, pos=None if positions is None else i32(P),
              pool=i64(PMAX), ids_all=i64(RV), ref_ts=i64(RV), rec_raw=f32(RV), nov_raw=f32(RV), stats=f32(3, 8), stat_scratch=f32(30), w_rows=f32(RV),
              perm=i32(RV), seg=i32(64), group_ws=i32(128), Xc_raw=f32(BT, FC), Xc_s=f32(BT, FC), dXc=f32(BT, FC), Xi_raw=f32(RV, FI),
              Xi_s=f32(RV, FI), dXi=f32(RV, FI), seq_len=i32(B), mask=torch.zeros(BT, dtype=torch.uint8), cur_neg_slot=i32(BT, N),
              Z1=f32(Rall, C), dZ1=f32(Rall, C), dZ2=f32(Rall, C), grouped_ev=None, Xd=None, cat=None, precar=None, arm=F32Rows(rt))
    rt.precar.alloc(pl, f32)
    assert {n: tuple(getattr(pl, n).shape) for n in ('U', 'dU', 'V', 'dV')} == {'U': (BT, C), 'dU': (BT, C), 'V': (RV, C), 'dV': (RV, C)}
    d = dict(B=B, T=T, max_ts=MAX_TS, sum_mask=SUM_MASK, row_begin=ROW_BEGIN, ic_rows=i64(P), ln_rows=i64(P), ets_rows=i64(P), d_seq_len=i32(B),
             d_mask=torch.zeros(P, dtype=torch.uint8), cat=i64(6, P), num=f32(3, P))
    for n, v in list(vars(pl).items()) + list(d.items()):
        if torch.is_tensor(v):
            rt.name(v, n)
    d['seq_len'], d['mask'] = d.pop('d_seq_len'), d.pop('d_mask')
    del rt.log[:]
    return rt, pl, d


def state(rt, n_last, device):
    st = dict(last=rt.name(torch.zeros(30, dtype=torch.int64), 'last'), n_last=n_last, pop_norm=rt.name(torch.zeros(N_ITEMS), 'pop_norm'))
    if device:
        st['device'] = True
    return st


# ---------------------------------------------------------------------------------------------------------------- resident tables
def test_tables_and_descriptors_are_set_on_the_runtime():
    rt = Runtime()
    L, meta = LAYOUT, PARAMS['articles_metadata']
    assert torch.equal(rt.ace, torch.from_numpy(PARAMS['content_article_embeddings_matrix'])) and rt.ace.dtype == torch.float32
    assert torch.equal(rt.created, torch.from_numpy(np.asarray(meta['created_at_ts'], dtype=np.int64)))
    assert rt.meta_cat.dtype == torch.int64 and torch.equal(rt.meta_cat, torch.from_numpy(np.asarray(meta['category_id'], np.int64))[None])
    assert np.array_equal(rt.ctx_desc.numpy(), L.ctx_descriptors()) and np.array_equal(rt.item_desc.numpy(), L.item_descriptors())
    segs, singles = L.item_segments()
    assert np.array_equal(rt.item_segs.numpy(), segs) and np.array_equal(rt.item_singles.numpy(), singles)
    assert (rt.n_item_segs, rt.n_item_singles, rt.item_lds) == (3, 5, True)
    assert rt.ctx_emb_groups == CTX_GROUPS and rt.item_emb_groups == ITEM_GROUPS


def test_a_fractional_integer_column_is_refused_with_the_same_words():
    p = dict(PARAMS, articles_features_config=copy.deepcopy(PARAMS['articles_features_config']), articles_metadata=dict(PARAMS['articles_metadata']))
    p['articles_features_config']['category_id'] = {'type': 'numerical', 'dtype': 'int'}
    p['articles_metadata']['category_id'] = np.full(N_ITEMS, 0.5)
    L = ParamLayout(p['session_features_config'], p['articles_features_config'], N_ITEMS, D, C, 255, 1, 'ugrnn')
    rt = types.SimpleNamespace(layout=L, device=torch.device('cpu'), params=p, n_items=N_ITEMS)
    with pytest.raises(ValueError, match=re.escape("article feature 'category_id' holds non-integer values but its config says dtype 'int': declare it "
                                                   "{'type': 'numerical', 'dtype': 'float'}")):
        FeatureRows(rt, np.zeros((N_ITEMS, D), np.float32))


# ---------------------------------------------------------------------------------------------------------------- front end, forward
@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("dev_scalars", [True, False])
def test_step_ints_group_rows_dynamic_raw(positions, dev_scalars):
    rt, pl, d = make(positions, dev_scalars=dev_scalars)
    P, RV = pl.P, 2 * pl.P + PMAX + 1
    st = state(rt, 30, True)
    if dev_scalars:          # the batch slot of a captured step holds no host scalar: everything comes from the record
        d['max_ts'] = d['sum_mask'] = None
    rt.features.step_ints(pl, d, S)
    rt.features.group_rows(pl, S)
    rt.features.dynamic_raw(pl, st, S)
    assert rt.log == [
        ('cham_step_ints_dev' if dev_scalars else 'cham_step_ints', 'ic_rows', 'ln_rows', 'pool', 'ets_rows', 'scalars' if dev_scalars else MAX_TS,
         P, PMAX, 'd_seq_len', B, 'd_mask', 'ids_all', 'ref_ts', 'seq_len', 'mask', 'stream'),
        ('cham_group_rows', 'ids_all', RV, 8, 'perm', 'seg', 'group_ws', 4 * 128, 'stream'),
        ('cham_item_dynamic_raw', 'ids_all', 'ref_ts', RV, 'created', 'pop_norm', 'rec_raw', 'nov_raw', 'stream')]
    assert step_scalar(rt, 'cham_x', 3) == (('cham_x_dev', rt.scalars.data_ptr()) if dev_scalars else ('cham_x', 3))
    assert step_scalar(rt, 'cham_x', None if dev_scalars else 3.7, int) == (('cham_x_dev', rt.scalars.data_ptr()) if dev_scalars else ('cham_x', 3))


@pytest.mark.parametrize("dev_scalars", [True, False])
@pytest.mark.parametrize("device", [True, False])
def test_norm_stats_from_the_recent_clicks(device, dev_scalars):
    rt, pl, d = make(dev_scalars=dev_scalars)
    if device and dev_scalars:
        d['max_ts'] = None
    rt.features.norm_stats(pl, d, state(rt, 30, device), S)
    fn = ('cham_norm_stats_from_buffer_dev' if dev_scalars else 'cham_norm_stats_from_buffer') if device else 'cham_norm_stats_from_recent'
    assert rt.log == [(fn, 'last', 30, 'scalars' if (device and dev_scalars) else MAX_TS, 'created', 'pop_norm', 'stat_scratch', 'stats', 'stream')]


@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("device", [True, False])
def test_norm_stats_of_the_first_batch_from_its_own_rows(positions, device):
    rt, pl, d = make(positions)
    P, RV = pl.P, 2 * pl.P + PMAX + 1
    rt.features.norm_stats(pl, d, state(rt, 0, device), S)
    assert rt.log == [('cham_row_weights', 'ids_all', 2 * P, 'cur_neg_slot', P * N, PMAX, 'pool', 'w_rows', 'w_rows+%d' % (2 * P), 'stream')] + [
        ('cham_norm_stats_from_rows', off('rec_raw', a), off('nov_raw', a), off('w_rows', a), b - a, off('stats', 8 * g), 'stream')
        for g, (a, b) in enumerate([(0, P), (P, 2 * P), (2 * P, RV)])]


@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("lds,singles", [(True, 5), (True, 0), (False, 5)])
def test_assemble(positions, lds, singles):
    rt, pl, d = make(positions)
    P, RV = pl.P, 2 * pl.P + PMAX + 1
    rt.item_lds, rt.n_item_singles = lds, singles
    rt.features.assemble(pl, d, S)
    rows = ('ids_all', RV, P, 2 * P, 'meta_cat', N_ITEMS, 'ace', D, 'rec_raw', 'nov_raw', 'stats', 'item_desc', FI)
    out = ('flat', fl('gamma_item'), fl('beta_item'), 'Xi_raw', 'Xi_s', 'stream')
    assert rt.log == [
        ('cham_ctx_assemble', 'cat', 'num', P, 'ctx_desc', FC, 'flat', fl('gamma_ctx'), fl('beta_ctx'), 'Xc_raw', 'Xc_s', 'stream'),
        ('cham_item_assemble_lds',) + rows + ('item_segs', 3, 'item_singles' if singles else None, singles) + out if lds else
        ('cham_item_assemble',) + rows + out]
    assert pl.cat is d['cat']


# ---------------------------------------------------------------------------------------------------------------- front end, backward
def ctx_bwd_launches(P, ws):
    return [('cham_feature_bwd_ws', 'dXc', 'Xc_raw', P, FC, gr('gamma_ctx'), gr('beta_ctx'), ws, 4 * 64, 'stream') if ws else
            ('cham_feature_bwd', 'dXc', 'Xc_raw', P, FC, gr('gamma_ctx'), gr('beta_ctx'), 'stream')] + [
        ('cham_emb_grad_scan', 'dXc', P, FC, c0, dim, fl('gamma_ctx'), 'cat+%d' % (feat * P), None, card, off('grads', o), 'stream')
        for feat, c0, dim, card, o in [(2, 11, 17, 23, 0), (3, 28, 14, 12, 392), (4, 42, 18, 29, 560)]]


def item_bwd_launches(RV, ws):
    return [('cham_feature_bwd_ws', 'dXi', 'Xi_raw', RV, FI, gr('gamma_item'), gr('beta_item'), ws, 4 * 64, 'stream') if ws else
            ('cham_feature_bwd', 'dXi', 'Xi_raw', RV, FI, gr('gamma_item'), gr('beta_item'), 'stream'),
            ('cham_emb_grad_scan', 'dXi', RV, FI, 0, 37, fl('gamma_item'), 'meta_cat', 'ids_all', 461, 'grads+1084', 'stream'),
            ('cham_emb_grad_grouped', 'dXi', RV, FI, 53, 30, fl('gamma_item'), 'ids_all', 'perm', 'seg', 'grads+18144', 'stream')]


@pytest.mark.parametrize("positions", POSITIONS)
@pytest.mark.parametrize("ws", [True, False])
def test_feature_backward_and_embedding_gradients(positions, ws):
    rt, pl, d = make(positions, feature_bwd_ws=ws)
    pl.cat = d['cat']
    rt.lane = '_aux'          # the user-context half on the third lane: that lane's workspace
    rt.features.ctx_bwd(pl)
    assert rt.log == ctx_bwd_launches(pl.P, ws and 'gemm_ws_aux')
    del rt.log[:]
    rt.lane = ''
    rt.features.item_bwd(pl)
    assert rt.log == item_bwd_launches(2 * pl.P + PMAX + 1, ws and 'gemm_ws')
    rt.lane = '_side'
    del rt.log[:]
    rt.features.feature_bwd(pl.dXi, pl.Xi_raw, 7, 5, 'gamma_item', 'beta_item')
    assert rt.log == [('cham_feature_bwd_ws', 'dXi', 'Xi_raw', 7, 5, gr('gamma_item'), gr('beta_item'), 'gemm_ws_side', 4 * 64, 'stream') if ws else
                      ('cham_feature_bwd', 'dXi', 'Xi_raw', 7, 5, gr('gamma_item'), gr('beta_item'), 'stream')]


def test_a_second_metadata_table_is_read_at_its_row_of_meta_cat():
    rt, pl, d = make()
    rt.item_emb_groups = [(2, 3, 5, 6, 7, 100)]
    rt.name(torch.zeros(4, N_ITEMS, dtype=torch.int64), 'meta_cat4')
    rt.meta_cat = rt.names['meta_cat4']
    rt.features.item_bwd(pl)
    assert rt.log[1:] == [('cham_emb_grad_scan', 'dXi', 2 * B * T + PMAX + 1, FI, 5, 6, fl('gamma_item'), 'meta_cat4+%d' % (3 * N_ITEMS), 'ids_all', 7,
                           'grads+100', 'stream')]


# ---------------------------------------------------------------------------------------------------------------- factorised form
TN, NT = dict(transA=1, splits=0), dict(transB=1)


@pytest.mark.parametrize("positions", POSITIONS)
def test_factorised_forward_and_backward(positions):
    rt, pl, d = make(positions)
    pre, P, RV = rt.precar, pl.P, 2 * pl.P + PMAX + 1
    assert pre.dropout is None
    pl.cat = d['cat']
    pre.forward(pl, S)
    pre.clicked_z1(pl, S)
    pl.arm.z1(pl, S, None)
    assert rt.log == [('gemm', 'Xc_s', fl('W1c'), 'U', P, C, FC, FC, C, C, dict(bias=fl('b1'))),
                      ('gemm', 'Xi_s', fl('W1i'), 'V', RV, C, FI, FI, C, C, {}),
                      ('cham_combine_fwd', 'U', 'V', C, P, N, PMAX, 'cur_neg_slot', 'Z1', 0, P, 'stream'),
                      ('cham_combine_fwd', 'U', 'V', C, P, N, PMAX, 'cur_neg_slot', 'Z1', P, 3 * P, 'stream')]
    del rt.log[:]
    pre.backward(pl, rt.gemm_ws, S)
    assert rt.log == [('cham_combine_bwd', 'dZ1', C, P, N, PMAX, 'cur_neg_slot', 'dU', 'dV', 'gemm_ws', 4 * 64, 'stream')]
    del rt.log[:]
    rt.lane = '_aux'
    pre.ctx_chain(pl)
    assert rt.log == [('gemm', 'Xc_s', 'dU', gr('W1c'), FC, C, P, FC, C, C, TN),
                      ('colsum', 'dU', C, P, C, gr('b1'), {}),
                      ('gemm', 'dU', fl('W1c'), 'dXc', P, FC, C, C, C, FC, NT)] + ctx_bwd_launches(P, 'gemm_ws_aux')
    del rt.log[:]
    rt.lane = ''
    pre.item_chain(pl)
    assert rt.log == [('gemm', 'Xi_s', 'dV', gr('W1i'), FI, C, RV, FI, C, C, TN),
                      ('gemm', 'dV', fl('W1i'), 'dXi', RV, FI, C, C, C, FI, NT)] + item_bwd_launches(RV, 'gemm_ws')


# ---------------------------------------------------------------------------------------------------------------- dense form, dropout
def dense(rt, pl):
    pre = DenseInput(rt, Dropout(rt, 0.8, STEP + (1 << 32), T, ROW_BEGIN))          # (the step key is the low 32 bits)
    pre.alloc(pl)
    for n in ('Xd', 'dXd', 'dUx', 'dVx', 'FC1d', 'drop_ws'):
        rt.name(getattr(pl, n), n)
    rt.name(pl.rnn_drop[0], 'rnn_drop')
    return pre


def mask_launches(X, P, pos):          # the three input sites: the clicked rows, then per position the positive and the negatives
    keep = 0.8
    return [('cham_dropout', X, X, P, FW, FW, keep, SEED, STEP, 16, 16, 1, pos, T, ROW_BEGIN, FC, 1, 'stream'),
            ('cham_dropout', '%s+%d' % (X, P * FW), '%s+%d' % (X, P * FW), 3 * P, FW, FW, keep, SEED, STEP, 17, 18, NC, pos, T, ROW_BEGIN, FC, 1, 'stream')]


def test_site_numbers():
    assert (SITE_INPUT_CLICKED, SITE_INPUT_POSITIVE, SITE_INPUT_NEGATIVE, SITE_FC1, SITE_RNN_OUT) == (16, 17, 18, 19, 20)


def test_dense_buffers_are_made_once_on_first_use():
    rt, pl, d = make()
    pre = dense(rt, pl)
    BT, RV, Rall = B * T, 2 * B * T + PMAX + 1, B * T * (1 + NC)
    assert rt.log == [('cham_combine_bwd_workspace_bytes', FW, B * T, N, PMAX)]
    assert {n: tuple(getattr(pl, n).shape) for n in ('Xd', 'dXd', 'dUx', 'dVx', 'FC1d', 'drop_ws')} == {
        'Xd': (Rall, FW), 'dXd': (Rall, FW), 'dUx': (BT, FW), 'dVx': (RV, FW), 'FC1d': (BT, 512), 'drop_ws': (96,)}
    assert [tuple(t.shape) for t in pl.rnn_drop] == [(BT, 256)] and not hasattr(pl, 'Z1f')
    Xd = pl.Xd
    pre.alloc(pl)
    assert pl.Xd is Xd and len(rt.log) == 1
    assert (pre.Fw, pre.W1.data_ptr(), pre.gW1.data_ptr(), tuple(pre.W1.shape), tuple(pre.gW1.shape)) == (
        FW, rt.p('W1c').data_ptr(), rt.g('W1c').data_ptr(), (FW, C), (FW, C))
    rt.b16 = True          # bf16 configuration: + the fp32 images of the bf16-resident candidate rows
    pl.Xd = None
    pre.alloc(pl)
    assert tuple(pl.Z1f.shape) == tuple(pl.dZ1f.shape) == (Rall, C)


@pytest.mark.parametrize("positions", POSITIONS)
def test_dense_forward_and_backward(positions):
    rt, pl, d = make(positions)
    pre, P, RV, pos = dense(rt, pl), pl.P, 2 * pl.P + PMAX + 1, None if positions is None else 'pos'
    Rall = P + 3 * P
    pl.cat = d['cat']
    del rt.log[:]
    z1 = dict(bias=fl('b1'), act=1)
    pre.forward(pl, S)
    pre.clicked_z1(pl, S)
    pl.arm.z1(pl, S, pre)
    assert rt.log == [('cham_dense_rows', 'Xc_s', FC, 'Xi_s', FI, P, N, PMAX, 'cur_neg_slot', 'Xd', 'stream')] + mask_launches('Xd', P, pos) + [
        ('gemm', 'Xd', fl('W1c'), 'Z1', P, C, FW, FW, C, C, z1),
        ('gemm', 'Xd+%d' % (P * FW), fl('W1c'), 'Z1+%d' % (P * C), 3 * P, C, FW, FW, C, C, z1)]          # the candidate rows: Xd[P:] -> Z1[P:]
    # the schedule's own sites go through the same object
    del rt.log[:]
    pre.dropout.apply(pl.FC1d, pl.FC1d, P, 512, 512, SITE_FC1, SITE_FC1, 1, pl.pos)
    pre.dropout.apply(pl.rnn_drop[0], pl.rnn_drop[0], B * T, 256, 256, SITE_RNN_OUT + 1, SITE_RNN_OUT + 1, 1, None)
    assert rt.log == [('cham_dropout', 'FC1d', 'FC1d', P, 512, 512, 0.8, SEED, STEP, 19, 19, 1, pos, T, ROW_BEGIN, 512, 0, 'stream'),
                      ('cham_dropout', 'rnn_drop', 'rnn_drop', B * T, 256, 256, 0.8, SEED, STEP, 21, 21, 1, None, T, ROW_BEGIN, 256, 0, 'stream')]
    del rt.log[:]
    pl.dUx.copy_(torch.arange(pl.dUx.numel()).view_as(pl.dUx)); pl.dVx.copy_(-torch.arange(pl.dVx.numel()).view_as(pl.dVx))
    pl.dXc.fill_(7.0); pl.dXi.fill_(7.0)
    assert pl.arm.dense_dZ1(pl, S) is pl.dZ1
    pre.backward(pl, rt.gemm_ws, S)
    assert rt.log == [('gemm', 'Xd', 'dZ1', gr('W1c'), FW, C, Rall, FW, C, C, TN),
                      ('colsum', 'dZ1', C, Rall, C, gr('b1'), {}),
                      ('gemm', 'dZ1', fl('W1c'), 'dXd', Rall, FW, C, C, C, FW, NT)] + mask_launches('dXd', P, pos) + [
        ('cham_combine_bwd', 'dXd', FW, P, N, PMAX, 'cur_neg_slot', 'dUx', 'dVx', 'drop_ws', 4 * 96, 'stream')]
    # the two halves of the summed input gradient: context columns of the per-position sums, item columns of the per-item-row sums
    assert torch.equal(pl.dXc[:P], pl.dUx[:P, :FC]) and torch.equal(pl.dXi[:RV], pl.dVx[:RV, FC:])
    assert (pl.dXc[P:] == 7.0).all() and (pl.dXi[RV:] == 7.0).all()
    del rt.log[:]
    rt.lane = ''
    pre.ctx_chain(pl)
    pre.item_chain(pl)
    assert rt.log == ctx_bwd_launches(P, 'gemm_ws') + item_bwd_launches(RV, 'gemm_ws')


def test_the_stacked_w1_needs_w1i_right_behind_w1c():
    L = copy.copy(LAYOUT)
    L.entries = dict(LAYOUT.entries)
    e = copy.copy(L.entries['W1i'])
    e.offset += 4
    L.entries['W1i'] = e
    rt = Runtime(L=LAYOUT)
    rt.layout = L
    with pytest.raises(AssertionError):
        DenseInput(rt, None)
    rt.layout = LAYOUT
    DenseInput(rt, None)


# ---------------------------------------------------------------------------------------------------------------- the driver names none of it
MOVED = ('cham_step_ints', 'cham_item_dynamic_raw', 'cham_norm_stats_', 'cham_row_weights', 'cham_ctx_assemble', 'cham_item_assemble', 'cham_dense_rows',
         'cham_dropout', 'cham_feature_bwd', 'cham_emb_grad_')


def test_the_driver_names_no_entry_point_that_moved():
    src = inspect.getsource(NARModuleModel._forward) + inspect.getsource(NARModuleModel.backward)
    assert 'cham_rows_gather' in src          # (what the scan reads is the driver)
    assert [n for n in MOVED if n in src] == []
    module = inspect.getsource(inspect.getmodule(FeatureRows))
    assert [n for n in MOVED if n not in module] == []
