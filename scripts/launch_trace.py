"""Launch trace of the training step (manual tool, not a test): proves that a change of the step DRIVER - the schedule in
NARModuleModel._forward / backward, an arm of nar/candidate_rows.py, a launch path of nar/recurrent.py, the feature rows or an input form
of nar/input_rows.py - left every launch, its order, its arguments and its lane as they were.

One configuration per process (the switches are read when the library / the runtime is created), traced under both schedules:
  short   as is: at these shapes Rc <= rt.w2_main_rows - W2 weight gradient on the main lane, cooperative recurrent kernels, no head split
  full    rt.w2_main_rows = 0, rt.rnn_coop_rows = -1: third lane, deferred W2 weight gradient, head split, single-workgroup recurrent kernels
Each run = four optimizer steps + one evaluate_step on five synthetic batches (device-resident state, presampled negatives; the configurations
in HOST_STATE feed the host's ClickedItemsState instead - the only way to cham_norm_stats_from_recent).  rt.lib and the state's lib are replaced
by a proxy that writes one line per library call of every step - the first one included: it builds the plan and, with an empty state, takes the
normalisation statistics from the batch's own rows - with the entry point, every non-pointer argument by value, every pointer argument
(_lib._SIGNATURES says which) renamed by order of first appearance - p0, p1, ..., 0 for NULL.  The stream is a pointer argument, so its tag names
the lane.  The run ends with the SHA-1 of the stacked losses and of rt.flat / m / v / grads.

The script touches rt.lib and _SIGNATURES only, so the same file runs on any two commits:
  python scripts/launch_trace.py --list
  python scripts/launch_trace.py --config NAME --out DIR      ->  DIR/NAME.short.trace, DIR/NAME.full.trace, DIR/NAME.sha1
and `diff -r` of the two DIRs must be empty."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name -> (environment, tiny_params overrides, runtime attributes, make_batches length_dist, micro-batch sessions)
CONFIGS = {
    'default': ({}, {}, {}, 'g1', 0),
    'h2_0': ({'CHAM_GEMM_H2': '0'}, {}, {}, 'g1', 0),
    'p3_0': ({'CHAM_GEMM_P3': '0'}, {}, {}, 'g1', 0),
    'f32_native': ({}, {'gemm_dtype': 'f32_native'}, {}, 'g1', 0),
    'bf16': ({}, {'gemm_dtype': 'bf16'}, {}, 'g1', 0),
    'bf16_nodma': ({}, {'gemm_dtype': 'bf16'}, {'b16_dma': False}, 'g1', 0),
    'h2_blocked_1': ({'CHAM_H2_BLOCKED': '1'}, {}, {}, 'g1', 0),
    'h2_blocked_dz2': ({'CHAM_H2_BLOCKED': 'dz2'}, {}, {}, 'g1', 0),
    's1_h2_0': ({'CHAM_S1_H2': '0'}, {}, {}, 'g1', 0),
    's1_h2_a': ({'CHAM_S1_H2': 'a'}, {}, {}, 'g1', 0),
    'groupsum_0': ({'CHAM_DGRAD_GROUPSUM': '0'}, {}, {}, 'g1', 0),
    'overlap_0': ({'CHAM_OVERLAP': '0'}, {}, {}, 'g1', 0),
    'dev_scalars_0': ({'CHAM_DEV_SCALARS': '0'}, {}, {}, 'g1', 0),
    'compact_0': ({'CHAM_COMPACT': '0'}, {}, {}, 'g1', 0),
    'tail_aux_0': ({'CHAM_TAIL_SPLIT': '0', 'CHAM_WGRAD_AUX': '0'}, {}, {}, 'g1', 0),
    'dropout_f32': ({}, {'dropout_keep_prob': 0.8}, {}, 'g1', 0),
    'dropout_bf16': ({}, {'dropout_keep_prob': 0.8, 'gemm_dtype': 'bf16'}, {}, 'g1', 0),
    'neg10': ({}, {'neg': 10}, {}, 'g1', 0),
    'neg10_bf16': ({}, {'neg': 10, 'gemm_dtype': 'bf16'}, {}, 'g1', 0),
    'gru2': ({}, {'rnn_cell': 'gru', 'rnn_num_layers': 2}, {}, 'g1', 0),
    'ugrnn2': ({}, {'rnn_num_layers': 2}, {}, 'g1', 0),                                    # two layers: no third lane for the small weight gradients
    'ugrnn_wide': ({}, {'H': 600}, {}, 'g1', 0),                                           # Hp 640: step-wise UGRNN
    'gru_wide': ({}, {'rnn_cell': 'gru', 'H': 500}, {}, 'g1', 0),                          # Hp 512: step-wise GRU
    'gru_wide2': ({}, {'rnn_cell': 'gru', 'H': 400, 'rnn_num_layers': 2}, {}, 'g1', 0),
    'gru_dropout': ({}, {'rnn_cell': 'gru', 'H': 500, 'dropout_keep_prob': 0.8}, {}, 'g1', 0),
    'lstm': ({}, {'rnn_cell': 'lstm'}, {}, 'g1', 0),                                       # step-wise at every width
    'lstm2': ({}, {'rnn_cell': 'lstm', 'H': 400, 'rnn_num_layers': 2}, {}, 'g1', 0),
    'full_length': ({}, {}, {}, 'full', 0),
    'microbatched': ({}, {}, {}, 'g1', 8),
    'host_state': ({}, {}, {}, 'g1', 0),                                                   # recent clicks uploaded from the host every step
    'item_elem': ({}, {}, {'item_lds': False}, 'g1', 0),                                   # item rows by the one-thread-per-element assemble
}
HOST_STATE = {'host_state'}
SCHEDULES = {'short': {}, 'full': {'w2_main_rows': 0, 'rnn_coop_rows': -1}}
B, SEQ, N_ITEMS = 16, 6, 1000


class Trace:
    def __init__(self):
        self.lines, self.tags, self.on = [], {}, False

    def tag(self, a):
        if a is None or a == 0:
            return '0'
        if not isinstance(a, int):          # a host array (launch counters)
            return 'host'
        return self.tags.setdefault(a, 'p%d' % len(self.tags))


class LibProxy:
    """Forwards every entry point of the library; records the calls of those _SIGNATURES describes while the trace is on."""

    def __init__(self, lib, trace, signatures):
        self.__dict__.update(_lib=lib, _trace=trace, _sig=signatures)

    def __getattr__(self, name):
        fn, sig, tr = getattr(self._lib, name), self._sig.get(name), self._trace
        if sig is None:
            return fn
        is_ptr = [a.__name__ == 'c_void_p' for a in sig[1]]

        def call(*args):
            if tr.on:
                tr.lines.append(name + ' ' + ' '.join(tr.tag(a) if p else repr(a) for a, p in zip(args, is_ptr)))
            return fn(*args)
        self.__dict__[name] = call
        return call


def sha1(t):
    return hashlib.sha1(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run(cfg, schedule):
    import torch
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd.nar import synthetic
    from chameleon_recsys_amd.nar.clicked_items_state import ClickedItemsState, DeviceClickedItemsState
    from chameleon_recsys_amd.nar.nar_model import ModeKeys, NARModuleModel, NARRuntime
    from tests import helpers as H
    _env, over, attrs, length_dist, micro = CONFIGS[cfg]
    kw = dict(C=256, batch_size=B, seq_len=SEQ, neg=31)
    kw.update(over)
    p = H.tiny_params(**kw)
    rt = NARRuntime(p, seed=3, weights=H.pair_weights(p))

    def model_of(mode, keep, neg, neg_buf):          # tests/helpers.make_pair's recipe without the oracle half
        return NARModuleModel(mode, None, None, p['session_features_config'], p['articles_features_config'], p['batch_size'], p['lr'], keep,
                              neg, neg_buf, p['content_article_embeddings_matrix'], softmax_temperature=p['softmax_temperature'],
                              reg_weight_decay=p['reg_weight_decay'], recent_clicks_buffer_max_size=p['recent_clicks_buffer_max_size'],
                              recent_clicks_for_normalization=p['recent_clicks_for_normalization'], articles_metadata=p['articles_metadata'],
                              CAR_embedding_size=p['CAR_embedding_size'], rnn_units=p['rnn_units'],
                              novelty_reg_factor=p.get('novelty_reg_factor', 0.0), runtime=rt, rnn_num_layers=p.get('rnn_num_layers', 1),
                              rnn_cell=p.get('rnn_cell', 'ugrnn'), gemm_dtype=p.get('gemm_dtype', 'f32'))
    model = model_of(ModeKeys.TRAIN, p.get('dropout_keep_prob', 1.0), p['train_total_negative_samples'], p['train_negative_samples_from_buffer'])
    ev = model_of(ModeKeys.EVAL, 1.0, p['eval_total_negative_samples'], p['eval_negative_samples_from_buffer'])
    for k, v in list(attrs.items()) + list(SCHEDULES[schedule].items()):
        assert hasattr(rt, k), k
        setattr(rt, k, v)
    host = cfg in HOST_STATE
    st = (ClickedItemsState if host else DeviceClickedItemsState)(p['recent_clicks_buffer_hours'], p['recent_clicks_buffer_max_size'],
                                                                  p['recent_clicks_for_normalization'], N_ITEMS)
    tr = Trace()
    rt.lib = LibProxy(rt.lib, tr, _lib._SIGNATURES)
    if not host:
        st.lib = LibProxy(st.lib, tr, _lib._SIGNATURES)
    batches = synthetic.make_batches(5, B, SEQ, N_ITEMS, p['session_features_config'], length_dist=length_dist)
    dev = [model.upload_batch(f, l) for f, l in batches]
    losses = []
    for i, d in enumerate(dev):
        tr.on = True
        tr.lines.append('# step %d' % (i + 1))
        m = model if i < 4 else ev
        if host:
            m.feed_state(st.get_articles_recent_pop_norm().copy(), st.get_recent_clicks_buffer().copy())
        else:
            m.feed_state(st, st)
        if i == 4:
            losses.append(m.evaluate_step(d).clone())
        elif micro:
            losses.append(m.train_step_microbatched(batches[i][0], batches[i][1], micro).clone())
        else:
            losses.append(m.train_step(d).clone())
        if host:
            H.update_state(st, *batches[i])
        else:
            st.update_from_device_batch(d['aci'], d['g_event_ts'])
        if i + 1 < 4 and not micro and not host:
            model.presample(dev[i + 1])
    torch.cuda.synchronize()
    tr.on = False
    if rt.rnn_coop_timed_out():
        raise RuntimeError("a cooperative recurrent workgroup timed out")
    hashes = [sha1(torch.stack(losses)), sha1(rt.flat), sha1(rt.m), sha1(rt.v), sha1(rt.grads)]
    return tr.lines, hashes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--list', action='store_true')
    ap.add_argument('--config', choices=sorted(CONFIGS))
    ap.add_argument('--out', help='directory of the trace files (needed with --config)')
    a = ap.parse_args()
    if a.list or not a.config:
        print('\n'.join(CONFIGS))
        return
    if not a.out:
        ap.error('--out DIR is needed with --config')
    os.environ.update(CONFIGS[a.config][0])          # before the library is loaded and the runtime is built
    os.makedirs(a.out, exist_ok=True)
    out = []
    for schedule in SCHEDULES:
        lines, hashes = run(a.config, schedule)
        with open(os.path.join(a.out, '%s.%s.trace' % (a.config, schedule)), 'w') as f:
            f.write('\n'.join(lines) + '\n')
        out.append('%s %s lines=%d losses=%s flat=%s m=%s v=%s grads=%s' % ((a.config, schedule, len(lines)) + tuple(hashes)))
    with open(os.path.join(a.out, a.config + '.sha1'), 'w') as f:
        f.write('\n'.join(out) + '\n')
    print('\n'.join(out))


if __name__ == '__main__':
    main()
