"""The LSTM session encoder without a GPU: the float64 BPTT reference (tests/lstm_reference.py) against torch float64 autograd of the same
TF 1.12 cell; the float32 restatement of the step-wise path's two point stages and two GEMMs against that reference, within the bound the
GPU test holds the kernels to - and a mutant that forgets the cell state's gradient, which the bound must catch; the parameter layout.

Worst relative error on one CPU: lstm_bptt vs autograd 6.6e-16 over all arrays; the restatement over all widths, shapes and arrays 2.0e-7;
the mutant's dxproj 0.56 - 0.87."""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from chameleon_recsys_amd.nar.layout import ParamLayout
from tests.lstm_reference import REL_BOUND, SAVED, kernel_reference, lstm_bptt, padded_inputs, point_stages, rel_err

# float64 arithmetic over sums of at most a few hundred terms: 1e-10 relative leaves five orders of magnitude of headroom
F64_BOUND = 1e-10
# the GPU test's shapes (a partial last block; a non-power-of-two width; the widest) + one row without recurrence
SHAPES = [(128, 5, 3), (384, 37, 6), (1024, 8, 4), (128, 1, 1)]


def _autograd(x, lengths, K, b, R):
    """The cell written forward-only in torch float64; gradients by autograd."""
    x, K, b = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, K, b))
    lens, Rt = torch.as_tensor(lengths), torch.as_tensor(R, dtype=torch.float64)
    B, T, _ = x.shape
    H = K.shape[1] // 4
    h = c = torch.zeros(B, H, dtype=torch.float64)
    outs = []
    for t in range(T):
        i, j, f, o = (torch.cat([x[:, t], h], 1) @ K + b).split(H, 1)
        cn = torch.sigmoid(f + 1.0) * c + torch.sigmoid(i) * torch.tanh(j)
        hn = torch.sigmoid(o) * torch.tanh(cn)
        v = (t < lens).unsqueeze(1)
        outs.append(torch.where(v, hn, torch.zeros_like(hn)))
        h, c = torch.where(v, hn, h), torch.where(v, cn, c)
    out = torch.stack(outs, 1)
    (out * Rt).sum().backward()
    return [a.detach().numpy() for a in (out, x.grad, K.grad, b.grad)]


@pytest.mark.parametrize("B,T,I,H", [(7, 5, 6, 9), (3, 1, 4, 5), (12, 9, 16, 24)])
def test_lstm_bptt_matches_float64_autograd(B, T, I, H):
    rng = np.random.default_rng(100 * B + T)
    x, R = rng.standard_normal((B, T, I)), rng.standard_normal((B, T, H))
    K, b = rng.standard_normal((I + H, 4 * H)) * (I + H) ** -0.5, 0.3 * rng.standard_normal(4 * H)
    lengths = rng.integers(0, T + 1, size=B)
    lengths[:3] = [T, 0, 1][:B]
    got, ref = lstm_bptt(x, lengths, K, b, R), _autograd(x, lengths, K, b, R)
    errs = [rel_err(g, r) for g, r in zip(got, ref)]
    print("lstm_bptt vs autograd B %d T %d: out, dx, dK, db %r" % (B, T, errs))
    assert max(errs) <= F64_BOUND, errs
    assert lstm_bptt(x, lengths, K, b, R, weight_grads=False)[2:] == (None, None)


def test_saved_planes_are_the_forward_activations():
    """saved=True: hprev / cprev are the states BEFORE the step (carried beyond the length), the gates recombine to the output."""
    rng = np.random.default_rng(3)
    B, T, I, H = 4, 5, 3, 6
    x, R = rng.standard_normal((B, T, I)), rng.standard_normal((B, T, H))
    K, b = rng.standard_normal((I + H, 4 * H)) * 0.4, np.zeros(4 * H)
    lengths = np.array([T, 0, 2, 1])
    out, _, _, _, s = lstm_bptt(x, lengths, K, b, R, saved=True)
    assert set(s) == set(SAVED)
    valid = (np.arange(T)[None, :] < lengths[:, None])[..., None]
    assert np.allclose(out, np.where(valid, s['Go'] * s['TC'], 0.0), atol=0, rtol=1e-15)
    assert np.allclose(s['TC'], np.tanh(s['Gf'] * s['cprev'] + s['Gi'] * s['Gj']), atol=0, rtol=1e-15)
    assert not s['hprev'][:, 0].any() and not s['cprev'][:, 0].any()
    assert np.array_equal(s['hprev'][2, 2:], np.repeat(out[2, 1][None], T - 2, 0))          # carried once the session has ended
    assert np.array_equal(s['cprev'][2, 3], s['cprev'][2, 2]) and s['cprev'][2, 2].any()


_cases = {}


def _case(Hp, B, T):
    """Inputs and float64 reference of one (width, shape), computed once for the restatement and the mutant."""
    if (Hp, B, T) not in _cases:
        inp = padded_inputs(Hp, B, T, seed=5 * Hp + B + T)
        _cases[(Hp, B, T)] = (inp, kernel_reference(inp['xproj'], inp['lengths'], inp['Wh'], inp['dout']))
    return _cases[(Hp, B, T)]


def test_padded_inputs_have_pad_lanes_and_the_edge_lengths():
    inp = padded_inputs(128, 5, 3, seed=1)
    assert inp['H'] == 111 and list(inp['lengths']) == [3, 0, 1, 3, 2]
    assert not inp['Wh'][111:].any() and not inp['Wh'].reshape(128, 4, 128)[..., 111:].any()
    assert not inp['xproj'].reshape(5, 3, 4, 128)[..., 111:].any() and not inp['dout'][..., 111:].any()
    assert inp['dout'][1].any()                                        # non-zero beyond the length


@pytest.mark.parametrize("Hp,B,T", SHAPES)
def test_point_stage_restatement_matches_float64_bptt(Hp, B, T):
    inp, ref = _case(Hp, B, T)
    got = point_stages(inp)
    assert set(got) == set(ref) == set(SAVED) | {'out', 'dxproj'} and all(np.isfinite(a).all() for a in got.values())
    errs = {k: rel_err(got[k], ref[k]) for k in ref}
    print("point stages Hp %d B %d T %d: worst %.2e" % (Hp, B, T, max(errs.values())))
    assert max(errs.values()) <= REL_BOUND, errs
    beyond = np.arange(T)[None, :] >= inp['lengths'][:, None]
    assert not got['out'][beyond].any() and not got['dxproj'][beyond].any()
    H = inp['H']                                                       # pad lanes: z = 0, so j = 0, c stays 0 and every dz is 0
    for k in ('out', 'hprev', 'cprev', 'Gj', 'TC'):
        assert not got[k][..., H:].any(), k
    assert not got['dxproj'].reshape(B, T, 4, Hp)[..., H:].any()


@pytest.mark.parametrize("Hp,B,T", SHAPES[:3])                        # (1, 1) has no recurrence: carry_c is never read
def test_bound_catches_a_dropped_cell_state_gradient(Hp, B, T):
    inp, ref = _case(Hp, B, T)
    err = rel_err(point_stages(inp, drop_carry_c=True)['dxproj'], ref['dxproj'])
    print("mutant (carry_c stays 0) Hp %d B %d T %d: %.2e" % (Hp, B, T, err))
    assert err > REL_BOUND, err


# ---------------------------------------------------------------------------------------------------------------- layout
def _layout(rnn_units, cell, layers=1):
    p = synthetic.default_params(200, 16, C=128, H=rnn_units, rnn_cell=cell)
    return ParamLayout(p['session_features_config'], p['articles_features_config'], 200, 16, 128, rnn_units, layers, cell)


@pytest.mark.parametrize("layers", [1, 2])
def test_lstm_layout_pack_unpack_round_trip(layers):
    L = _layout(111, 'lstm', layers)
    H, Hp, C = 111, 128, 128
    assert (L.H, L.Hp, L.NG, L.cell) == (H, Hp, 4, 'lstm')
    specs = L.logical_specs()
    rng = np.random.default_rng(7)
    w = {k: rng.standard_normal(shape).astype(np.float32) for k, (shape, _, _) in specs.items()}
    flat = L.pack(w)
    back = L.unpack(flat)
    assert list(back) == list(specs)
    for k in w:
        assert np.array_equal(back[k], w[k]), k
    for l in range(layers):
        I, Ip = (C, C) if l == 0 else (H, Hp)
        assert specs['rnn/%d/kernel' % l] == ((I + H, 4 * H), 'xavier', False) and specs['rnn/%d/bias' % l] == ((4 * H,), 'zeros', False)
        assert L.entries['rnn%d/Wx' % l].shape == (Ip, 4 * Hp) and L.entries['rnn%d/Wh' % l].shape == (Hp, 4 * Hp)
        assert L.entries['rnn%d/b' % l].shape == (4 * Hp,) and 'rnn%d/Wch' % l not in L.entries
        K = w['rnn/%d/kernel' % l]
        Wx, Wh, b = (L._view(flat, 'rnn%d/%s' % (l, n)) for n in ('Wx', 'Wh', 'b'))
        for k in range(4):                                             # block k of the TF kernel lands in padded block k; pads are zero
            assert np.array_equal(Wx[:I, k * Hp:k * Hp + H], K[:I, k * H:(k + 1) * H])
            assert np.array_equal(Wh[:H, k * Hp:k * Hp + H], K[I:, k * H:(k + 1) * H])
            assert np.array_equal(b[k * Hp:k * Hp + H], w['rnn/%d/bias' % l][k * H:(k + 1) * H])
            assert not Wx[:, k * Hp + H:(k + 1) * Hp].any() and not Wh[:, k * Hp + H:(k + 1) * Hp].any() and not b[k * Hp + H:(k + 1) * Hp].any()
        assert not Wh[H:].any() and not Wx[I:].any()
    init = L.init_logical(seed=1)
    assert not init['rnn/0/bias'].any() and init['rnn/0/kernel'].any()          # the forget bias is the kernel's + 1, not a variable's value


def test_lstm_tf_variable_names_and_shapes():
    L = _layout(111, 'lstm', 2)
    names, specs = L.tf_variable_names(), L.logical_specs()
    for l, I in ((0, 128), (1, 111)):
        cell = 'main/RNN/rnn/multi_rnn_cell/cell_%d/lstm_cell/' % l
        assert names[cell + 'kernel'] == 'rnn/%d/kernel' % l and names[cell + 'bias'] == 'rnn/%d/bias' % l
        assert specs[names[cell + 'kernel']][0] == (I + 111, 444) and specs[names[cell + 'bias']][0] == (444,)
    assert not [n for n in names if 'ugrnn_cell' in n or 'gru_cell' in n]
    w = L.init_logical(seed=2)
    back = L.from_tf_variables({k + ':0': v for k, v in L.to_tf_variables(w).items()})
    assert list(back) == list(w) and all(np.array_equal(back[k], w[k]) for k in w)


def test_lstm_is_stepwise_at_every_width_and_the_other_thresholds_stand():
    assert _layout(100, 'lstm').rnn_stepwise and _layout(100, 'lstm').Hp == 128
    assert _layout(384, 'lstm').rnn_stepwise and _layout(1000, 'lstm').rnn_stepwise
    assert not _layout(384, 'gru').rnn_stepwise and _layout(385, 'gru').rnn_stepwise
    assert not _layout(512, 'ugrnn').rnn_stepwise and _layout(513, 'ugrnn').rnn_stepwise
    for cell, ng in (('ugrnn', 2), ('gru', 3)):                        # what the other cells lay out is what it was
        L = _layout(255, cell)
        assert L.NG == ng and L.entries['rnn0/Wh'].shape == (256, 512) and L.entries['rnn0/Wx'].shape == (128, ng * 256)
    assert _layout(255, 'lstm').fingerprint() != _layout(255, 'gru').fingerprint()
    with pytest.raises(ValueError, match="rnn_cell"):
        _layout(255, 'rnn')


# ---------------------------------------------------------------------------------------------------------------- the test-side oracle
@pytest.mark.parametrize("layers", [1, 2])
def test_lstm_oracle_cell_matches_the_reference(layers):
    """tests/lstm_oracle.py (what the GPU step-parity tests compare the HIP path with) against lstm_bptt, as
    tests/test_oracle_second_opinion.py does for the oracle's own cells: forward, d x and the variables' gradients; layer by layer."""
    from tests import helpers as H
    from tests.lstm_oracle import LstmOracle
    B, T, C, Hn = 6, 7, 16, 24
    p = H.tiny_params(C=C, H=Hn, neg=5, batch_size=B, rnn_cell='lstm', rnn_num_layers=layers, n_items=200, ace_dim=8)
    orc = LstmOracle(p, seed=4)
    assert [tuple(orc.w['rnn/%d/kernel' % l].shape) for l in range(layers)] == [(C + Hn, 4 * Hn), (2 * Hn, 4 * Hn)][:layers]
    assert list(orc.w) == list(orc.specs)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((B, T, C)).astype(np.float32)
    lengths = np.array([7, 3, 1, 5, 0, 2])
    R = rng.standard_normal((B, T, Hn)).astype(np.float32)
    xt = torch.from_numpy(x).requires_grad_(True)
    out = orc._rnn(xt, torch.from_numpy(lengths))
    (out * torch.from_numpy(R)).sum().backward()
    w = {k: v.detach().numpy().astype(np.float64) for k, v in orc.w.items()}
    # the stack in the reference: forward layer by layer, backward in reverse with d x of the upper layer as the lower one's R
    xs, Rl = [x.astype(np.float64)], R.astype(np.float64)
    for l in range(layers):
        xs.append(lstm_bptt(xs[l], lengths, w['rnn/%d/kernel' % l], w['rnn/%d/bias' % l], Rl, weight_grads=False)[0])
    assert np.abs(out.detach().numpy() - xs[-1]).max() < 2e-6
    assert not out.detach().numpy()[1, 3:].any() and not out.detach().numpy()[4].any()          # zero output past the length
    for l in range(layers - 1, -1, -1):
        _, dx, dK, db = lstm_bptt(xs[l], lengths, w['rnn/%d/kernel' % l], w['rnn/%d/bias' % l], Rl)
        for k, g in (('rnn/%d/kernel' % l, dK), ('rnn/%d/bias' % l, db)):
            assert np.abs(orc.w[k].grad.numpy() - g).max() < 2e-5 * max(1.0, np.abs(g).max()), k
        Rl = dx
    assert np.abs(xt.grad.numpy() - Rl).max() < 2e-5 * max(1.0, np.abs(Rl).max())
