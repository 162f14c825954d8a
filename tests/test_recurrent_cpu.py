"""The launch paths of the recurrent stack (nar/recurrent.py) without a GPU: which path a step gets, the buffers each path adds to a plan,
and - through a recording library, a recording gemm and a plan of small CPU tensors - every launch of a layer's time loop at T = 3, B = 2:
its order, its scalar arguments, and which buffer each pointer argument names.  The expected sequences are written out here, not derived
from the classes: they are what NARModuleModel._forward / backward launched before the paths had a module of their own."""
import types

import pytest
import torch

from chameleon_recsys_amd.nar import recurrent, synthetic
from chameleon_recsys_amd.nar.layout import ParamLayout
from chameleon_recsys_amd.nar.nar_model import NARRuntime
from chameleon_recsys_amd.nar.recurrent import CoopUgrnn, FusedRnn, StepwiseGru, StepwiseUgrnn
from tests.recording import Recorder, S

B, T = 2, 3
F32 = dict(force_f32=True)


def _layout(cell, rnn_units, layers=1):
    p = synthetic.default_params(200, 16, C=128, H=rnn_units, rnn_cell=cell)
    return ParamLayout(p['session_features_config'], p['articles_features_config'], 200, 16, 128, rnn_units, layers, cell)


LAYOUTS = {}


def layout(cell, rnn_units):
    key = (cell, rnn_units)
    if key not in LAYOUTS:
        LAYOUTS[key] = _layout(cell, rnn_units)
    return LAYOUTS[key]


# ---------------------------------------------------------------------------------------------------------------- selection
DEFAULT = 'default'
SELECTION = [
    ('ugrnn', 255, 1000, 32, DEFAULT, CoopUgrnn),
    ('ugrnn', 255, 1000, 32, -1, FusedRnn),
    ('ugrnn', 255, 1000, 2048, DEFAULT, FusedRnn),
    ('ugrnn', 255, 0, 32, DEFAULT, FusedRnn),
    ('ugrnn', 255, 131072, 1024, DEFAULT, CoopUgrnn),          # both bounds are inclusive ...
    ('ugrnn', 255, 131073, 1024, DEFAULT, FusedRnn),
    ('ugrnn', 255, 131072, 1025, DEFAULT, FusedRnn),
] + [(cell, units, PC, Bs, rows, cls)
     for cell, units, cls in [('ugrnn', 512, FusedRnn), ('ugrnn', 600, StepwiseUgrnn), ('gru', 384, FusedRnn), ('gru', 385, StepwiseGru),
                              ('gru', 255, FusedRnn)]
     for PC, Bs in [(0, 32), (1000, 32), (1000, 2048), (1 << 22, 256)] for rows in (DEFAULT, -1)]


@pytest.mark.parametrize("cell,units,PC,Bs,rows,cls", SELECTION)
def test_path_selection(cell, units, PC, Bs, rows, cls):
    L = layout(cell, units)
    default = recurrent.default_coop_rows(L)
    assert default == (131072 if (cell, L.Hp) == ('ugrnn', 256) else -1)
    assert recurrent.path_class(L, PC, Bs, default if rows == DEFAULT else rows) is cls


def test_runtime_selects_per_step_and_keeps_one_instance_per_path():
    """NARRuntime.rnn_path on a stand-in runtime: rnn_coop_rows is read at every call (tools set it on a live runtime), a path is built once."""
    L = layout('ugrnn', 255)
    rt = types.SimpleNamespace(layout=L, rnn_coop_rows=recurrent.default_coop_rows(L), _rnn_paths={})
    pl = types.SimpleNamespace(PC=1000, B=32)
    coop = NARRuntime.rnn_path(rt, pl)
    assert type(coop) is CoopUgrnn and coop.host is rt and NARRuntime.rnn_path(rt, pl) is coop
    rt.rnn_coop_rows = -1
    fused = NARRuntime.rnn_path(rt, pl)
    assert type(fused) is FusedRnn and NARRuntime.rnn_path(rt, pl) is fused
    rt.rnn_coop_rows = 131072
    assert NARRuntime.rnn_path(rt, pl) is coop
    pl.PC = 0
    assert NARRuntime.rnn_path(rt, pl) is fused
    # no cooperative step so far: nothing to ask the device
    assert NARRuntime.rnn_coop_timed_out(types.SimpleNamespace(_rnn_paths={})) is False


# ---------------------------------------------------------------------------------------------------------------- recording host + plan
def make(cell, units, cls, layers=1):
    """(path, plan, host, {buffer alloc() added: shape}) of class `cls`: the plan holds what StepPlan keeps for every path + what alloc() adds."""
    L = layout(cell, units)
    host = Recorder(L, layers)
    Hp, NG, gru = L.Hp, L.NG, cell == 'gru'
    f32 = lambda *s: torch.zeros(*s)
    pl = types.SimpleNamespace(B=B, T=T, BT=B * T, PC=B * T * 11, seq_len=torch.zeros(B, dtype=torch.int32), dxproj=f32(B * T, NG * Hp), drnn=f32(B * T, Hp))
    for name in ('xproj', 'rnn_out', 'hprev', 'G', 'Cc', 'R', 'RH'):
        width = NG * Hp if name == 'xproj' else Hp
        setattr(pl, name, [f32(B * T, width) if (gru or name not in ('R', 'RH')) else None for _ in range(layers)])
    path = recurrent.path_class(L, pl.PC, B, recurrent.default_coop_rows(L))(host, L)
    assert type(path) is cls
    shared = set(vars(pl))
    path.alloc(pl, f32)
    for name, v in vars(pl).items():
        if torch.is_tensor(v):
            host.name(v, name)
        elif isinstance(v, list):
            for l, t in enumerate(v):
                if t is not None:
                    host.name(t, name if l == 0 else '%s[%d]' % (name, l))
    return path, pl, host, {n: tuple(getattr(pl, n).shape) for n in set(vars(pl)) - shared}


# ---------------------------------------------------------------------------------------------------------------- allocation
def test_alloc_adds_only_what_the_path_needs():
    per_step = {'h_state': (B, 640), 'zh': (B, 1280), 'carry': (B, 640), 'dzs': (B, 1280), 'direct': (B, 640)}
    assert make('ugrnn', 600, StepwiseUgrnn)[3] == per_step                     # no zc / dzc / drh, no WhT
    assert make('gru', 385, StepwiseGru)[3] == {'h_state': (B, 512), 'zh': (B, 1024), 'carry': (B, 512), 'dzs': (B, 1024), 'direct': (B, 512),
                                                'zc': (B, 512), 'dzc': (B, 512), 'drh': (B, 512)}
    # a plan's steps alternate between the cooperative and the fused path: both hold the transposed weights, neither a per-step buffer
    assert make('ugrnn', 255, CoopUgrnn)[3] == {'WhT': (512, 256)}
    L = layout('ugrnn', 255)
    pl = types.SimpleNamespace(B=B)
    FusedRnn(None, L).alloc(pl, lambda *s: torch.zeros(*s))
    assert {n: tuple(v.shape) for n, v in vars(pl).items() if n != 'B'} == {'WhT': (512, 256)}
    assert make('gru', 255, FusedRnn)[3] == {'WhT': (768, 256)}


# ---------------------------------------------------------------------------------------------------------------- sequences
def test_stepwise_gru_sequences():
    path, pl, host, _ = make('gru', 385, StepwiseGru)
    Hp = 512
    pl.h_state.fill_(1.0)
    path.forward(pl, 0, S)
    assert host.log == [e for t in (0, 1, 2) for e in (
        ('gemm', 'h_state', 'Wh0', 'zh', B, 1024, 512, 512, 1024, 1024, F32),
        ('cham_gru_point_gates_fwd', 'xproj', 'zh', 'seq_len', B, T, t, Hp, 'h_state', 'hprev', 'G', 'R', 'RH', 'stream'),
        ('gemm', 'RH+%d' % (t * Hp) if t else 'RH', 'Wch0', 'zc', B, 512, 512, T * Hp, 512, 512, F32),          # RH[:, t]: lda = T * Hp
        ('cham_gru_point_out_fwd', 'xproj', 'zc', 'seq_len', B, T, t, Hp, 'G', 'hprev', 'h_state', 'rnn_out', 'Cc', 'stream'))]
    assert not pl.h_state.any()                          # the state starts from zero
    del host.log[:]
    pl.carry.fill_(1.0); pl.direct.fill_(5.0)
    path.backward(pl, 0, S)
    assert host.log == [e for t in (2, 1, 0) for e in (
        ('cham_gru_point_c_bwd', 'drnn', 'carry', 'seq_len', B, T, t, Hp, 'hprev', 'G', 'Cc', 'dxproj', 'dzc', 'dzs', 'direct', 'stream'),
        ('gemm', 'dzc', 'Wch0', 'drh', B, 512, 512, 512, 512, 512, dict(transB=1, force_f32=True)),
        ('cham_gru_point_r_bwd', 'drh', 'seq_len', B, T, t, Hp, 'hprev', 'R', 'dxproj', 'dzs', 'direct', 'stream'),
        ('gemm', 'dzs', 'Wh0', 'carry', B, 512, 1024, 1024, 1024, 512, dict(transB=1, accumulate=1, force_f32=True)))]
    assert (pl.carry == 5.0).all()                       # carry = direct before the GEMM accumulates into it


def test_stepwise_ugrnn_sequences():
    path, pl, host, _ = make('ugrnn', 600, StepwiseUgrnn)
    Hp = 640
    pl.h_state.fill_(1.0)
    path.forward(pl, 0, S)
    assert host.log == [e for t in (0, 1, 2) for e in (
        ('gemm', 'h_state', 'Wh0', 'zh', B, 1280, 640, 640, 1280, 1280, F32),
        ('cham_ugrnn_point_fwd', 'xproj', 'zh', 'seq_len', B, T, t, Hp, 'h_state', 'rnn_out', 'hprev', 'G', 'Cc', 'stream'))]
    assert not pl.h_state.any()
    del host.log[:]
    pl.carry.fill_(1.0); pl.direct.fill_(5.0)
    path.backward(pl, 0, S)
    assert host.log == [e for t in (2, 1, 0) for e in (
        ('cham_ugrnn_point_bwd', 'drnn', 'carry', 'seq_len', B, T, t, Hp, 'hprev', 'G', 'Cc', 'dxproj', 'dzs', 'direct', 'stream'),
        ('gemm', 'dzs', 'Wh0', 'carry', B, 640, 1280, 1280, 1280, 640, dict(transB=1, accumulate=1, force_f32=True)))]
    assert (pl.carry == 5.0).all()


def test_fused_sequences_both_cells_second_layer():
    path, pl, host, _ = make('gru', 255, FusedRnn, layers=2)
    path.forward(pl, 1, S)
    assert host.log == [('cham_rnn_fwd', 1, 'xproj[1]', 'Wh1', 'seq_len', B, T, 256, 'rnn_out[1]', 'hprev[1]', 'G[1]', 'Cc[1]', 'R[1]', 'RH[1]', 'stream')]
    del host.log[:]
    path.backward(pl, 1, S)
    assert host.log == [('cham_transpose_f32', 'Wh1', 256, 512, 'WhT', 'stream'),
                        ('cham_transpose_f32', 'Wch1', 256, 256, 'WhT+%d' % (512 * 256), 'stream'),          # W_ch^T behind W_gh^T
                        ('cham_rnn_bwd', 1, 'drnn', 'WhT', 'seq_len', B, T, 256, 'hprev[1]', 'G[1]', 'Cc[1]', 'R[1]', 'dxproj', 'stream')]
    # UGRNN beyond the cooperative threshold: one transpose, no reset planes
    L = layout('ugrnn', 255)
    path, pl, host, _ = make('ugrnn', 255, CoopUgrnn)
    path = FusedRnn(host, L)
    path.forward(pl, 0, S)
    path.backward(pl, 0, S)
    assert host.log == [('cham_rnn_fwd', 0, 'xproj', 'Wh0', 'seq_len', B, T, 256, 'rnn_out', 'hprev', 'G', 'Cc', None, None, 'stream'),
                        ('cham_transpose_f32', 'Wh0', 256, 512, 'WhT', 'stream'),
                        ('cham_rnn_bwd', 0, 'drnn', 'WhT', 'seq_len', B, T, 256, 'hprev', 'G', 'Cc', None, 'dxproj', 'stream')]


def test_cooperative_sequences():
    path, pl, host, _ = make('ugrnn', 255, CoopUgrnn)
    nbytes = 4096
    host.lib.cham_rnn_coop_workspace_bytes = lambda b, hp: host.log.append(('cham_rnn_coop_workspace_bytes', b, hp)) or nbytes
    ws = host.name(path.ws(pl), 'ws')
    assert ws.dtype == torch.uint8 and ws.numel() == nbytes and not ws.any()
    path.forward(pl, 0, S)
    path.backward(pl, 0, S)
    assert host.log == [('cham_rnn_coop_workspace_bytes', B, 256),          # once per batch size: forward and backward share the workspace
                        ('cham_ugrnn_fwd_coop', 'xproj', 'Wh0', 'seq_len', B, T, 256, 'rnn_out', 'hprev', 'G', 'Cc', 'ws', nbytes, 'stream'),
                        ('cham_ugrnn_bwd_coop', 'drnn', 'Wh0', 'seq_len', B, T, 256, 'hprev', 'G', 'Cc', 'dxproj', 'ws', nbytes, 'stream')]
    del host.log[:]
    assert path.timed_out(S) is False
    assert host.log == [('cham_rnn_coop_timeouts', 'ws', B, 256, 'stream')]
    host.lib.cham_rnn_coop_timeouts = lambda *a: 1
    assert path.timed_out(S) is True


# ---------------------------------------------------------------------------------------------------------------- weight gradients
WG = dict(transA=1, splits=0, force_f32=True)


@pytest.mark.parametrize("cell,units,cls,Hp", [('ugrnn', 255, CoopUgrnn, 256), ('ugrnn', 600, StepwiseUgrnn, 640)])
def test_wgrads_ugrnn(cell, units, cls, Hp):
    path, pl, host, _ = make(cell, units, cls)
    path.wgrads(pl, 0)
    assert host.log == [('gemm', 'hprev', 'dxproj', 'dWh0', Hp, 2 * Hp, B * T, Hp, 2 * Hp, 2 * Hp, WG),
                        ('colsum', 'dxproj', 2 * Hp, B * T, 2 * Hp, 'db0', {})]


@pytest.mark.parametrize("cell,units,cls,Hp", [('gru', 255, FusedRnn, 256), ('gru', 385, StepwiseGru, 512)])
def test_wgrads_gru_adds_the_candidate_product(cell, units, cls, Hp):
    path, pl, host, _ = make(cell, units, cls, layers=2)
    path.wgrads(pl, 1)
    assert host.log == [('gemm', 'hprev[1]', 'dxproj', 'dWh1', Hp, 2 * Hp, B * T, Hp, 3 * Hp, 2 * Hp, WG),
                        ('gemm', 'RH[1]', 'dxproj+%d' % (2 * Hp), 'dWch1', Hp, Hp, B * T, Hp, 3 * Hp, Hp, WG),          # dz_c: columns [2 Hp, 3 Hp)
                        ('colsum', 'dxproj', 3 * Hp, B * T, 3 * Hp, 'db1', {})]
