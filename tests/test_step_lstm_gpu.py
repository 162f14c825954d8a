"""The training step with an LSTM session encoder (`rnn_cell='lstm'`: the step-wise path at every width, one recurrent GEMM and one gate
kernel per time step and direction) against the CPU oracle with the same cell (tests/lstm_oracle.py, pinned to the float64 BPTT reference
by tests/test_lstm_cpu.py): the checks of tests/test_step_gpu.py at Hp 128, 384 (stacked) and 1024, through the bf16 arithmetic,
valid-position compaction, per-layer output dropout, the optimizer step and the trainer's command line.  The input projection, the
weight-gradient code, compaction, dropout and stacking of the step read only xproj / the saved planes / dxproj; the parity here is what
shows that they need nothing LSTM-specific beyond the four column blocks."""
import os

import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from tests import helpers as H
from tests.lstm_oracle import LstmOracle, make_pair
from tests.test_step_gpu import _compare_step

pytestmark = pytest.mark.gpu


def _params(Hn, layers=1, **over):
    return H.tiny_params(C=128, H=Hn, neg=9, batch_size=40, rnn_cell='lstm', rnn_num_layers=layers, **over)


def _batches(p, n):
    return synthetic.make_batches(n, 40, 8, 1000, p['session_features_config'], length_dist='g1')


@pytest.mark.parametrize("layers,Hn", [(1, 100), (2, 300), (1, 1000)])        # Hp 128; Hp 384 stacked; Hp 1024
def test_step_parity_lstm(gpu, layers, Hn):
    """Bit-exact negatives, logits / probs / losses, and every gradient on a batch without leaky-ReLU kink flips (the flips come from the
    scorer and CAR pre-activations, not from the recurrent stack)."""
    p = _params(Hn, layers)
    batches = _batches(p, 4)
    st = H.warm_state(p, batches[:2])
    model, orc = make_pair(p, seed=5)
    L = model.rt.layout
    assert L.rnn_stepwise and L.cell == 'lstm' and L.NG == 4 and L.Hp == (Hn + 127) // 128 * 128
    flips = [_compare_step(model, orc, *batches[i], st) for i in (2, 3)]
    assert type(model._plan.rnn).__name__ == 'StepwiseLstm'
    print("LSTM layers %d H %d: kink flips %r" % (layers, Hn, flips))
    assert min(flips) == 0, flips


def test_step_parity_lstm_dropout(gpu):
    """keep 0.9 at Hp 128: the layer's output h is dropped behind the recurrence, neither state is."""
    keep = 0.9
    p = _params(100, dropout_keep_prob=keep)
    batches = _batches(p, 5)
    st = H.warm_state(p, batches[:2])
    model, orc = make_pair(p, seed=5)
    assert model.keep_prob == keep and model.rt.layout.cell == 'lstm'
    flips = []
    for i in (2, 3, 4):
        flips.append(_compare_step(model, orc, *batches[i], st))
        x_neg = orc.forward(*batches[i], st.get_recent_clicks_buffer(), st.get_articles_recent_pop_norm(), 'train')['x_neg']
        mask = np.asarray(batches[i][1]['label_next_item']) != 0
        dropped = float((x_neg.detach().numpy()[mask] == 0).mean())
        assert dropped > (1.0 - keep) * 0.8, dropped
        model.rt.global_step += 1; orc.global_step += 1
    print("LSTM dropout: kink flips %r" % flips)
    assert min(flips) == 0, flips


def test_step_parity_lstm_bf16_compute_mode(gpu):
    """gemm_dtype='bf16' at Hp 128: the input projection x W_x and its gradients on bf16-rounded operands, the recurrent product and the
    W_h gradient in fp32.  The criterion and the bounds are those of tests/test_step_gpu.py::test_step_parity_bf16_compute_mode, the
    project's check of this arithmetic (two correct bf16 evaluations differ by more than each differs from fp32): forward against the
    oracle emulating the rounding - logits 2e-3, loss 1e-3 - and within 3e-2 of the fp32 oracle's loss; every HIP gradient as close to the
    fp32 oracle's as the emulated bf16 gradient is (x 3 + 2 % of the tensor's max)."""
    p = _params(100, gemm_dtype='bf16')
    batches = _batches(p, 4)
    st = H.warm_state(p, batches[:2])
    model, orc = make_pair(p, seed=5)
    assert model.rt.gemm_dtype == 'bf16' and orc.gemm_dtype == 'bf16'
    orc32 = LstmOracle(dict(p, gemm_dtype='f32'), weights=orc.weights_numpy())
    for f, l in batches[2:4]:
        buf, pop = st.get_recent_clicks_buffer().copy(), st.get_articles_recent_pop_norm().copy()
        model.feed_state(pop, buf)
        model.forward(model.upload_batch(f, l))
        out = model.outputs_numpy()
        grads = {}
        for name, o in (("bf16", orc), ("f32", orc32)):
            for v in o.w.values():
                v.grad = None
            ref = o.forward(f, l, buf, pop, 'train')
            if name == "bf16":
                mask = ref['mask'].numpy()
                assert np.array_equal(out['neg_items'], ref['neg_items'].numpy())
                assert np.abs(out['logits'] - ref['logits'].detach().numpy())[mask].max() < 2e-3
                assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < 1e-3
            else:
                assert abs(out['loss'][0] - float(ref['total_loss'].detach())) < 3e-2
            ref['xe_loss'].backward()
            grads[name] = {k: (v.grad.numpy().copy() if v.grad is not None else np.zeros_like(v.detach().numpy())) for k, v in o.w.items()}
        model.backward()
        torch.cuda.synchronize()
        g = model.rt.logical_grads()
        assert set(g) == set(grads["f32"])
        for k in g:
            scale = max(1e-6, float(np.abs(grads["f32"][k]).max()))
            e_hip = float(np.abs(g[k] - grads["f32"][k]).max())
            e_emu = float(np.abs(grads["bf16"][k] - grads["f32"][k]).max())
            assert e_hip < 3.0 * e_emu + 2e-2 * scale + 2e-5, (k, e_hip, e_emu, scale)
        H.update_state(st, f, l)


def test_lstm_compaction_equals_padded_masked_path(gpu):
    """test_wide_gru_compaction_equals_padded_masked_path for the LSTM, with its bounds: the step-wise recurrence keeps the [B, T] layout
    between the scatter and the gather either side of it."""
    p = _params(100)
    batches = _batches(p, 4)
    st = H.warm_state(p, batches[:2])
    mc, _ = make_pair(p, seed=5)
    mp, _ = make_pair(p, seed=5)
    mp.rt.compact = False
    for f, l in batches[2:4]:
        outs = []
        for m in (mc, mp):
            m.feed_state(st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer())
            d = m.upload_batch(f, l)
            m.forward(d); m.backward()
            torch.cuda.synchronize()
            outs.append((m.outputs_numpy(), m.rt.grads.clone(), d))
        (oc, gc, dc), (op, gp, dp_) = outs
        assert dc['pos'] is not None and dp_['pos'] is None and dc['P'] < dp_['P']
        mask = np.arange(f['item_clicked'].shape[1])[None, :] < (np.asarray(f['session_size']).reshape(-1, 1) - 1)
        assert np.array_equal(oc['neg_items'], op['neg_items'])
        assert np.abs(oc['logits'] - op['logits'])[mask].max() < 1e-5
        assert np.abs(oc['loss'] - op['loss']).max() < 1e-5
        assert float((gc - gp).abs().max()) < 2e-5 * float(gp.abs().max()) + 1e-7
        for m in (mc, mp):
            m.apply_gradients()
        H.update_state(st, f, l)
        H.assert_runtimes_close(mc.rt, mp.rt, p['lr'])
        for name in ('flat', 'm', 'v'):          # (see the test this one follows: restart both from the same weights / slots)
            getattr(mp.rt, name).copy_(getattr(mc.rt, name))


@pytest.mark.parametrize("layers,Hn", [(1, 100), (2, 300)])
def test_lstm_trains_and_keeps_its_pads_zero(gpu, layers, Hn):
    """Three consecutive optimizer steps leave finite losses, and every pad row and column of W_x, W_h and b exactly zero: at a pad lane
    z = 0, so j = 0 and c never leaves 0, and every dz there is 0."""
    p = _params(Hn, layers)
    batches = _batches(p, 5)
    st = H.warm_state(p, batches[:2])
    model, _ = make_pair(p, seed=5)
    L = model.rt.layout
    before = model.rt.flat.clone()
    losses = []
    for f, l in batches[2:5]:
        model.feed_state(st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer())
        losses.append(model.train_step(model.upload_batch(f, l)).cpu().numpy().copy())
        H.update_state(st, f, l)
    print("LSTM losses: %r" % [float(x[0]) for x in losses])
    assert np.isfinite(np.stack(losses)).all(), losses
    assert model.rt.global_step == 3
    flat = model.rt.flat.cpu().numpy()
    Hh, Hp = L.H, L.Hp
    assert Hh < Hp
    for l in range(layers):
        I = L.C if l == 0 else Hh
        Wx, Wh, b = (L._view(flat, 'rnn%d/%s' % (l, n)) for n in ('Wx', 'Wh', 'b'))
        assert Wx.shape[1] == Wh.shape[1] == b.shape[0] == 4 * Hp
        moved = L._view(before.cpu().numpy(), 'rnn%d/Wh' % l) != Wh
        assert moved[:Hh].reshape(Hh, 4, Hp)[..., :Hh].mean() > 0.9, "W_h of layer %d did not train" % l
        assert not Wx[I:].any() and not Wh[Hh:].any(), "pad rows of layer %d" % l
        for k in range(4):
            pad = slice(k * Hp + Hh, (k + 1) * Hp)
            assert not Wx[:, pad].any() and not Wh[:, pad].any() and not b[pad].any(), "pad columns of block %d, layer %d" % (k, l)
            assert b[k * Hp:k * Hp + Hh].any()


def test_trainer_cli_trains_and_evaluates_an_lstm(gpu, tmp_path):
    """`nar_trainer_gcom --rnn_cell lstm --rnn_units 200` end to end: hourly train -> evaluate over TFRecord files (the EVAL forward goes
    through the same step-wise branch), finite metrics, a checkpoint - which a GRU layout refuses to load."""
    from chameleon_recsys_amd.nar import nar_trainer_gcom as T
    from chameleon_recsys_amd.nar.nar_model import NARRuntime
    files, csv, pkl = synthetic.write_dataset(str(tmp_path / "data"), 3, 40, 300, 16, seq_len=10, seed=5)
    argv = ['--batch_size', '24', '--truncate_session_length', '10', '--learning_rate', '1e-3', '--reg_l2', '1e-5',
            '--softmax_temperature', '0.2', '--recent_clicks_buffer_max_size', '600', '--recent_clicks_for_normalization', '100',
            '--eval_metrics_top_n', '3', '--CAR_embedding_size', '64', '--rnn_cell', 'lstm', '--rnn_units', '200',
            '--train_total_negative_samples', '7', '--train_negative_samples_from_buffer', '50', '--eval_total_negative_samples', '12',
            '--eval_negative_samples_from_buffer', '60', '--content_embedding_scale_factor', '6.0', '--training_hours_for_each_eval', '2',
            '--disable_eval_benchmarks', '--train_set_path_regex', str(tmp_path / "data" / "sessions_hour_*.tfrecord.gz"),
            '--acr_module_articles_metadata_csv_path', csv, '--acr_module_articles_content_embeddings_pickle_path', pkl,
            '--model_dir', str(tmp_path / "model")]
    est = T.main(argv)
    rt = est._store['runtime']
    L = rt.layout
    assert L.cell == 'lstm' and L.Hp == 256 and L.NG == 4 and L.rnn_stepwise
    ckpt = os.path.join(str(tmp_path / "model"), "model.ckpt.pt")
    assert os.path.exists(ckpt)
    assert est.global_step == 4                                  # 2 training files x 40 sessions / batch 24 -> 2 steps each
    log = T.eval_sessions_metrics_log
    assert len(log) == 1 and 0.0 <= log[-1]['hitrate_at_n'] <= 1.0 and np.isfinite(log[-1]['mrr_at_n'])
    assert torch.isfinite(rt.flat).all()
    assert 'main/RNN/rnn/multi_rnn_cell/cell_0/lstm_cell/kernel' in est.get_variable_names()
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    assert sd['layout'] == L.fingerprint()
    rt.load_state_dict(sd)                                       # its own layout takes it back ...
    gru = NARRuntime(dict(rt.params, rnn_cell='gru'), seed=1)
    with pytest.raises(ValueError, match="different parameter layout"):
        gru.load_state_dict(sd)                                  # ... another cell's refuses it
