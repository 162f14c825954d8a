"""The LSTM's launch path (nar/recurrent.py: StepwiseLstm) without a GPU, in the manner of tests/test_recurrent_cpu.py and on its recording
host: the path every LSTM step gets, the buffers it adds to a plan, and every launch of one layer's forward and backward at T = 3, B = 2 -
order, scalar arguments, and the buffer each pointer names.  The expected sequences are written out, not derived from the class."""
import types

import pytest
import torch

from chameleon_recsys_amd.nar import recurrent
from chameleon_recsys_amd.nar.recurrent import StepwiseLstm, StepwiseUgrnn
from tests.recording import Recorder, S
from tests.test_recurrent_cpu import B, F32, T, WG, layout


def make(units, layers=1):
    """(path, plan, host, {buffer alloc() added: shape}): the plan holds what StepPlan keeps for an LSTM layout + what alloc() adds."""
    L = layout('lstm', units)
    host = Recorder(L, layers)
    Hp = L.Hp
    for l in range(layers):                    # the recording host sizes W_h for the two-block cells: the LSTM's has four
        host.weights['rnn%d/Wh' % l] = host.name(torch.zeros(Hp, 4 * Hp), 'Wh%d' % l)
        host.grads['rnn%d/Wh' % l] = host.name(torch.zeros(Hp, 4 * Hp), 'dWh%d' % l)
    f32 = lambda *s: torch.zeros(*s)
    pl = types.SimpleNamespace(B=B, T=T, BT=B * T, PC=B * T * 11, seq_len=torch.zeros(B, dtype=torch.int32), dxproj=f32(B * T, 4 * Hp), drnn=f32(B * T, Hp))
    for name in ('xproj', 'rnn_out', 'hprev', 'G', 'Cc', 'R', 'RH'):
        setattr(pl, name, [f32(B * T, 4 * Hp if name == 'xproj' else Hp) for _ in range(layers)])
    path = recurrent.path_class(L, pl.PC, B, recurrent.default_coop_rows(L))(host, L)
    assert type(path) is StepwiseLstm
    shared = set(vars(pl))
    path.alloc(pl, f32)
    added = {}
    for name, v in vars(pl).items():
        if torch.is_tensor(v):
            host.name(v, name)
            shape = tuple(v.shape)
        elif isinstance(v, list):
            for l, t in enumerate(v):
                host.name(t, name if l == 0 else '%s[%d]' % (name, l))
            shape = [tuple(t.shape) for t in v]
        else:
            continue
        if name not in shared:
            added[name] = shape
    return path, pl, host, added


@pytest.mark.parametrize("units", [100, 255, 384, 500, 1000])
@pytest.mark.parametrize("PC,Bs", [(0, 32), (1000, 32), (1000, 2048), (131072, 1024), (1 << 22, 256)])
def test_every_lstm_step_takes_the_stepwise_path(units, PC, Bs):
    L = layout('lstm', units)
    assert L.rnn_stepwise and recurrent.default_coop_rows(L) == -1
    for rows in (-1, 131072):
        assert recurrent.path_class(L, PC, Bs, rows) is StepwiseLstm


def test_lstm_path_is_the_ugrnn_time_loop_over_four_blocks():
    assert issubclass(StepwiseLstm, StepwiseUgrnn) and StepwiseLstm.launches_per_step == (2, 3)
    assert StepwiseLstm.forward is StepwiseUgrnn.forward and StepwiseLstm.backward is StepwiseUgrnn.backward
    path = make(100)[0]
    assert (path.Hp, path.NGH, path.WhN) == (128, 512, 512)


@pytest.mark.parametrize("units,Hp,layers", [(100, 128, 1), (600, 640, 2)])
def test_alloc_adds_both_states_their_gradients_and_two_planes_per_layer(units, Hp, layers):
    assert make(units, layers)[3] == {
        'h_state': (B, Hp), 'zh': (B, 4 * Hp), 'carry': (B, Hp), 'dzs': (B, 4 * Hp), 'direct': (B, Hp),
        'c_state': (B, Hp), 'carry_c': (B, Hp), 'cprev': [(B * T, Hp)] * layers, 'TC': [(B * T, Hp)] * layers}


def test_stepwise_lstm_sequences():
    path, pl, host, _ = make(300)
    Hp = 384
    pl.h_state.fill_(1.0); pl.c_state.fill_(1.0)
    path.forward(pl, 0, S)
    assert host.log == [e for t in (0, 1, 2) for e in (
        ('gemm', 'h_state', 'Wh0', 'zh', B, 1536, 384, 384, 1536, 1536, F32),
        ('cham_lstm_point_fwd', 'xproj', 'zh', 'seq_len', B, T, t, Hp, 'h_state', 'c_state', 'rnn_out', 'hprev', 'cprev', 'G', 'Cc', 'R', 'RH',
         'TC', 'stream'))]
    assert not pl.h_state.any() and not pl.c_state.any()          # both states start from zero
    del host.log[:]
    pl.carry.fill_(1.0); pl.carry_c.fill_(1.0); pl.direct.fill_(5.0)
    path.backward(pl, 0, S)
    assert host.log == [e for t in (2, 1, 0) for e in (
        ('cham_lstm_point_bwd', 'drnn', 'carry', 'carry_c', 'seq_len', B, T, t, Hp, 'cprev', 'G', 'Cc', 'R', 'RH', 'TC', 'dxproj', 'dzs', 'direct',
         'stream'),
        ('gemm', 'dzs', 'Wh0', 'carry', B, 384, 1536, 1536, 1536, 384, dict(transB=1, accumulate=1, force_f32=True)))]
    assert (pl.carry == 5.0).all()                                # carry = direct before the GEMM accumulates into it
    assert not pl.carry_c.any()                                   # zeroed with the carry; only the kernel writes it afterwards


def test_second_layer_uses_its_own_planes_and_weights():
    path, pl, host, _ = make(100, layers=2)
    path.forward(pl, 1, S)
    assert host.log[:2] == [
        ('gemm', 'h_state', 'Wh1', 'zh', B, 512, 128, 128, 512, 512, F32),
        ('cham_lstm_point_fwd', 'xproj[1]', 'zh', 'seq_len', B, T, 0, 128, 'h_state', 'c_state', 'rnn_out[1]', 'hprev[1]', 'cprev[1]', 'G[1]',
         'Cc[1]', 'R[1]', 'RH[1]', 'TC[1]', 'stream')]
    del host.log[:]
    path.backward(pl, 1, S)
    assert host.log[0] == ('cham_lstm_point_bwd', 'drnn', 'carry', 'carry_c', 'seq_len', B, T, 2, 128, 'cprev[1]', 'G[1]', 'Cc[1]', 'R[1]', 'RH[1]',
                           'TC[1]', 'dxproj', 'dzs', 'direct', 'stream')


def test_wgrads_lstm_span_four_blocks():
    path, pl, host, _ = make(100, layers=2)
    path.wgrads(pl, 1)
    assert host.log == [('gemm', 'hprev[1]', 'dxproj', 'dWh1', 128, 512, B * T, 128, 512, 512, WG),
                        ('colsum', 'dxproj', 512, B * T, 512, 'db1', {})]
