"""The training step with a GRU encoder wider than the fused kernels reach (rnn_units above 384: the step-wise path, two recurrent GEMMs
and two gate kernels per time step and direction) against the CPU oracle: the checks of tests/test_step_gpu.py at Hp 512, 640 (stacked)
and 1024, through valid-position compaction, per-layer output dropout and the optimizer step.  The weight-gradient code of the step reads
only the saved planes and dxproj; the gradient parity here is what shows that it needs no GRU-specific change."""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd.nar import synthetic
from tests import helpers as H
from tests.test_step_gpu import _compare_step

pytestmark = pytest.mark.gpu


def _params(Hn, layers=1, **over):
    return H.tiny_params(C=128, H=Hn, neg=9, batch_size=40, rnn_cell='gru', rnn_num_layers=layers, **over)


@pytest.mark.parametrize("layers,Hn", [(1, 500), (2, 600), (1, 1000)])        # Hp 512; Hp 640 stacked; Hp 1024
def test_step_parity_wide_gru(gpu, layers, Hn):
    """test_step_parity_rnn_variants for the step-wise GRU: bit-exact negatives, logits / probs / losses, and every gradient on a batch
    without leaky-ReLU kink flips (the flips come from the scorer and CAR pre-activations, not from the recurrent stack)."""
    p = _params(Hn, layers)
    batches = synthetic.make_batches(4, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    model, orc = H.make_pair(p, seed=5)
    L = model.rt.layout
    assert L.rnn_stepwise and L.cell == 'gru' and L.Hp == (Hn + 127) // 128 * 128
    flips = [_compare_step(model, orc, *batches[i], st) for i in (2, 3)]
    print("wide GRU layers %d H %d: kink flips %r" % (layers, Hn, flips))
    assert min(flips) == 0, flips


def test_wide_gru_compaction_equals_padded_masked_path(gpu):
    """test_valid_position_compaction_equals_padded_masked_path at Hp 512: the step-wise recurrence keeps the [B, T] layout between the
    scatter and the gather either side of it."""
    p = _params(500)
    batches = synthetic.make_batches(4, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    mc, _ = H.make_pair(p, seed=5)
    mp, _ = H.make_pair(p, seed=5)
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


def test_step_parity_wide_gru_dropout(gpu):
    """test_step_parity_dropout at Hp 512, keep 0.9: the layer's output is dropped behind the step-wise recurrence, its state is not."""
    keep = 0.9
    p = _params(500, dropout_keep_prob=keep)
    batches = synthetic.make_batches(5, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    model, orc = H.make_pair(p, seed=5)
    assert model.keep_prob == keep and model.rt.layout.rnn_stepwise
    flips = []
    for i in (2, 3, 4):
        flips.append(_compare_step(model, orc, *batches[i], st))
        x_neg = orc.forward(*batches[i], st.get_recent_clicks_buffer(), st.get_articles_recent_pop_norm(), 'train')['x_neg']
        mask = np.asarray(batches[i][1]['label_next_item']) != 0
        dropped = float((x_neg.detach().numpy()[mask] == 0).mean())
        assert dropped > (1.0 - keep) * 0.8, dropped
        model.rt.global_step += 1; orc.global_step += 1
    print("wide GRU dropout: kink flips %r" % flips)
    assert min(flips) == 0, flips


def test_wide_gru_trains(gpu):
    """Three consecutive optimizer steps at Hp 512 leave finite losses."""
    p = _params(500)
    batches = synthetic.make_batches(5, 40, 8, 1000, p['session_features_config'], length_dist='g1')
    st = H.warm_state(p, batches[:2])
    model, _ = H.make_pair(p, seed=5)
    losses = []
    for f, l in batches[2:5]:
        model.feed_state(st.get_articles_recent_pop_norm(), st.get_recent_clicks_buffer())
        losses.append(model.train_step(model.upload_batch(f, l)).cpu().numpy().copy())
        H.update_state(st, f, l)
    print("wide GRU losses: %r" % [float(x[0]) for x in losses])
    assert np.isfinite(np.stack(losses)).all(), losses
    assert model.rt.global_step == 3


def test_trainer_cli_trains_and_evaluates_a_wide_gru(gpu, tmp_path):
    """`nar_trainer_gcom --rnn_cell gru --rnn_units 1000` end to end: hourly train -> evaluate over TFRecord files (the EVAL forward goes
    through the same step-wise branch), finite metrics, a checkpoint."""
    import os
    from chameleon_recsys_amd.nar import nar_trainer_gcom as T
    files, csv, pkl = synthetic.write_dataset(str(tmp_path / "data"), 3, 40, 300, 16, seq_len=10, seed=5)
    argv = ['--batch_size', '24', '--truncate_session_length', '10', '--learning_rate', '1e-3', '--reg_l2', '1e-5',
            '--softmax_temperature', '0.2', '--recent_clicks_buffer_max_size', '600', '--recent_clicks_for_normalization', '100',
            '--eval_metrics_top_n', '3', '--CAR_embedding_size', '64', '--rnn_cell', 'gru', '--rnn_units', '1000',
            '--train_total_negative_samples', '7', '--train_negative_samples_from_buffer', '50', '--eval_total_negative_samples', '12',
            '--eval_negative_samples_from_buffer', '60', '--content_embedding_scale_factor', '6.0', '--training_hours_for_each_eval', '2',
            '--disable_eval_benchmarks', '--train_set_path_regex', str(tmp_path / "data" / "sessions_hour_*.tfrecord.gz"),
            '--acr_module_articles_metadata_csv_path', csv, '--acr_module_articles_content_embeddings_pickle_path', pkl,
            '--model_dir', str(tmp_path / "model")]
    est = T.main(argv)
    L = est._store['runtime'].layout
    assert L.cell == 'gru' and L.Hp == 1024 and L.rnn_stepwise
    assert os.path.exists(os.path.join(str(tmp_path / "model"), "model.ckpt.pt"))
    assert est.global_step == 4                                  # 2 training files x 40 sessions / batch 24 -> 2 steps each
    log = T.eval_sessions_metrics_log
    assert len(log) == 1 and 0.0 <= log[-1]['hitrate_at_n'] <= 1.0 and np.isfinite(log[-1]['mrr_at_n'])
    assert torch.isfinite(est._store['runtime'].flat).all()
