"""Top-n next-article prediction for open sessions: the driver behind NARModuleModel.predict_step."""
# The input-click stages (features, PreCAR / CAR of the clicked rows, the recurrent stack, the session FCs) run ONCE per batch over all valid
# positions on the model's own plan, as in EVAL.  The candidate-row stages run per CHUNK of Nc candidates on a second plan of shape
# (B = P_last, T = 1, N = Nc) - one "position" per session with at least one click, its last one: cham_predict_fill_chunk writes the chunk into
# that plan's sampler outputs, so the feature front end, U + V, CAR layer 2 and the ranking head see it exactly as they see sampled negatives
# (the label column holds the pad item and is ignored).  cham_predict_topn_merge carries the top-n and the log-sum-exp across the chunks,
# always in the order 0 .. ceil(K / Nc) - 1.  Nothing here writes the weights, the recent-clicks state, global_step or an evaluation record.
import numpy as np
import torch

from .._lib import check, ptr
from .candidate_rows import ACT_LEAKY, ACT_TANH

MAX_TOP_N = 64         # cham_predict_topn_merge: the running list is one entry per lane
MAX_T = 128            # ... and its exclusion scan holds a session's clicks in LDS


def check_top_n(n):
    if not (isinstance(n, (int, np.integer)) and 1 <= int(n) <= MAX_TOP_N):
        raise ValueError("predict_top_n must be an integer in [1, %d] (got %r)" % (MAX_TOP_N, n))
    return int(n)


def normalise_candidates(candidates, n_items):
    """Explicit candidate ids -> sorted distinct int64 array; an id outside [1, n_items) is a ValueError."""
    c = np.asarray(candidates)
    if c.size and not np.issubdtype(c.dtype, np.integer):
        raise ValueError("candidates must be integer item ids")
    c = c.astype(np.int64).reshape(-1)
    if c.size and (int(c.min()) < 1 or int(c.max()) >= n_items):
        raise ValueError("candidates: item ids must be in [1, %d) (got %d .. %d)" % (n_items, int(c.min()), int(c.max())))
    return np.unique(c)


def last_positions(item_clicked):
    """(lengths [B] = index of the last non-zero click + 1, 0 for a row without a click)."""
    nz = np.asarray(item_clicked) != 0
    T = nz.shape[1]
    return np.where(nz.any(1), T - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.int64)


def default_chunk_width(B, T, train_negatives, P_last, K):
    """The largest Nc with P_last (1 + Nc) <= B T (1 + train_negatives) - the candidate rows of the model's own training plan - and no wider
    than the candidate set rounded up to the merge kernel's tile of 64."""
    budget = B * T * (1 + int(train_negatives))
    return int(max(1, min(budget // max(1, P_last) - 1, -(-max(1, K) // 64) * 64)))


def empty_result(B, n, K=0, Nc=0, chunks=0):
    return dict(item_ids=np.zeros((B, n), np.int64), scores=np.full((B, n), -np.inf, np.float32), probs=np.zeros((B, n), np.float32),
                K=int(K), Nc=int(Nc), chunks=int(chunks), P_last=0, candidates=np.zeros(0, np.int64))


def upload_predict_batch(model, features):
    """Features batch (no labels) -> the device batch of predict_step: upload_batch's tensors for the input-click stages (pad labels,
    session lengths from item_clicked itself) + the last-click rows of the candidate-row stages."""
    L = model.rt.layout
    ic = np.ascontiguousarray(features['item_clicked'], dtype=np.int64)
    B, T = ic.shape
    if T > MAX_T:
        raise ValueError("predict: sessions of %d clicks - the exclusion scan of cham_predict_topn_merge holds at most %d" % (T, MAX_T))
    lens = last_positions(ic)
    f = dict(features)
    f['session_size'] = lens + 1
    labels = dict(label_next_item=np.zeros((B, T), np.int64), label_last_item=np.zeros((B, 1), np.int64))
    sess = np.flatnonzero(lens > 0)
    P_last = int(sess.shape[0])
    if P_last == 0:
        return dict(B=B, T=T, P_last=0, empty_predict=True)
    d = model.upload_batch(f, labels)
    flat = sess * T + (lens[sess] - 1)
    if d['pos'] is not None:      # row of (b, t_b) among the compacted valid positions
        rank = np.cumsum((np.arange(T)[None, :] < lens[:, None]).reshape(-1)) - 1
        rows = rank[flat]
    else:
        rows = flat
    ets = np.ascontiguousarray(features['event_timestamp'], dtype=np.int64).reshape(-1)
    cat = np.stack([np.asarray(features[n], np.int64).reshape(-1)[flat] for n in L.ctx_cat_names]) if L.ctx_cat_names \
        else np.zeros((1, P_last), np.int64)
    num = np.stack([np.asarray(features[n], np.float32).reshape(-1)[flat] for n in L.ctx_num_names]) if L.ctx_num_names \
        else np.zeros((1, P_last), np.float32)
    last = model._h2d(dict(rows=rows.astype(np.int32), ic_rows=ic.reshape(-1)[flat], ln_rows=np.zeros(P_last, np.int64), ets_rows=ets[flat],
                           seq_len=np.ones(P_last, np.int32), mask=np.ones(P_last, np.uint8), cat=cat, num=num, excl=ic[sess]))
    last.update(B=P_last, T=1, Bg=P_last, row_begin=0, sum_mask=float(P_last), max_ts=d['max_ts'], P=P_last, pos=None)
    d.update(P_last=P_last, sess=sess, last=last)
    return d


def _candidates(model, candidates):
    """(cand int64 device tensor, K_dev int32 [1], K, host ids): the explicit list, or the distinct non-zero ids of the fed recent-clicks
    buffer - on the device for a device-resident state, from the host array otherwise."""
    rt, st = model.rt, model._dev_state
    dev = rt.device
    if candidates is None and st.get('device'):
        buf = st['buffer']
        ws = getattr(rt, '_predict_cand_ws', None)
        need = int(rt.lib.cham_predict_candidates_workspace_bytes(rt.n_items))
        if ws is None or ws.numel() < need:
            ws = rt._predict_cand_ws = torch.empty(need, dtype=torch.uint8, device=dev)
        cand = torch.zeros(max(1, buf.numel()), dtype=torch.int64, device=dev)
        K_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        check(rt.lib.cham_predict_candidates(ptr(buf), buf.numel(), rt.n_items, ptr(cand), cand.numel(), ptr(K_dev), ptr(ws), ws.numel(),
                                             rt.stream()), "cham_predict_candidates")
        K = int(K_dev.item())          # the chunk count is a host decision: one read-back per batch
        return cand, K_dev, K, None
    if candidates is None:
        buf = np.asarray(model.pop_recent_items_buffer, dtype=np.int64).reshape(-1)
        ids = np.unique(buf[(buf >= 1) & (buf < rt.n_items)])
    else:
        ids = normalise_candidates(candidates, rt.n_items)
    K = int(ids.shape[0])
    if K == 0:
        return None, None, 0, ids
    return torch.from_numpy(ids).to(dev), torch.tensor([K], dtype=torch.int32, device=dev), K, ids


def _input_clicks(model, d):
    """The input-click stages of the EVAL forward on the model's own plan, without sampler and candidate rows: pl.pred [P, C]."""
    rt, lib, L = model.rt, model.rt.lib, model.rt.layout
    st = model._dev_state
    B, T = d['B'], d['T']
    pl = rt.plan(B, T, model.negative_samples, model.negative_sample_from_buffer, d['Bg'])
    check(lib.cham_set_log_bases(model.elapsed_days_smooth_log_base, model.popularity_smooth_log_base), "cham_set_log_bases")
    torch.cuda.current_stream().wait_event(d['uploaded'])
    s = rt.stream()
    rt.refresh_shadows()
    pos, BT = d['pos'], d['P']
    pl.pos, pl.P, pl.PC = pos, BT, BT * pl.NC
    if rt.dev_scalars:      # (max_ts of this batch; the sampler keys of the record stay as they are)
        rt.set_step_scalars(0, d['max_ts'], d['sum_mask'], fields=2, stream=s)
    pl.cur_neg_ids, pl.cur_neg_slot = pl.neg_ids, pl.neg_slot
    if pl.grouped_ev is not None:
        torch.cuda.current_stream().wait_event(pl.grouped_ev)
        pl.grouped_ev = None
    fr, p, C, Hp, NGH = rt.features, rt.p, L.C, L.Hp, L.NG * L.Hp
    fr.step_ints(pl, d, s)
    fr.dynamic_raw(pl, st, s)
    fr.norm_stats(pl, d, st, s)
    fr.assemble(pl, d, s)
    pre = pl.precar = rt.precar
    pre.forward(pl, s)
    pre.clicked_z1(pl, s)
    rt.gemm(pl.Z1, p('W2'), pl.Z2, BT, C, C, C, C, C, bias=p('b2'), act=ACT_TANH)
    x, ldx, K = pl.Z2, C, C
    if pos is not None:
        pl.Z2f.zero_()
        check(lib.cham_rows_scatter(ptr(pl.Z2), ptr(pos), BT, C, ptr(pl.Z2f), s), "cham_rows_scatter")
        x = pl.Z2f
    rnn = pl.rnn = rt.rnn_path(pl)
    for l in range(L.L):
        rt.gemm(x, p('rnn%d/Wx' % l), pl.xproj[l], pl.BT, NGH, K, ldx, NGH, NGH, bias=p('rnn%d/b' % l))
        rnn.forward(pl, l, s)
        x, ldx, K = pl.rnn_out[l], Hp, Hp
    if pos is not None:
        check(lib.cham_rows_gather(ptr(x), ptr(pos), BT, Hp, ptr(pl.rnn_c), s), "cham_rows_gather")
        x = pl.rnn_c
    rt.gemm(x, p('Wf1'), pl.FC1, BT, 512, Hp, Hp, 512, 512, bias=p('bf1'), act=ACT_LEAKY)
    rt.gemm(pl.FC1, p('Wf2'), pl.pred, BT, C, 512, 512, C, C, bias=p('bf2'), act=ACT_TANH)
    return pl


def _score_chunk(model, plc, d2, s):
    """The candidate-row stages over the last-click rows for the chunk in plc's sampler outputs: plc.logits [P_last, 1 + Nc]."""
    rt, lib, st = model.rt, model.rt.lib, model._dev_state
    fr, p = rt.features, rt.p
    fr.step_ints(plc, d2, s)
    fr.dynamic_raw(plc, st, s)
    fr.norm_stats(plc, d2, st, s)
    fr.assemble(plc, d2, s)
    pre = plc.precar = rt.precar
    pre.forward(plc, s)
    arm = plc.arm = rt.step_arm(planes=True)
    arm.z1(plc, s, None)
    arm.car_fwd(plc)
    if rt.cosine:
        arm.cosine_fwd(plc, s)
        softmax_fwd, S3, K3, w4, b4 = 'cham_score_softmax_fwd', plc.cosq, 4, rt.cos_w4, rt.cos_b4
    else:
        arm.scorer_fwd(plc, s)
        softmax_fwd, S3, K3, w4, b4 = arm.softmax_fwd, plc.S3, 32, p('Ws4'), p('bs4')
    check(getattr(lib, softmax_fwd)(ptr(S3), K3, ptr(w4), ptr(b4), plc.P, plc.N, float(model.softmax_temperature), ptr(plc.mask), ptr(plc.logits),
                                    ptr(plc.probs), ptr(plc.nll), 0.0, ptr(plc.cur_neg_ids), ptr(st['pop_norm']), ptr(plc.nov_aux), s),
          "cham_score_softmax_fwd")


def predict_step(model, d, topn, candidates=None, chunk_candidates=None):
    """See NARModuleModel.predict_step."""
    rt, lib = model.rt, model.rt.lib
    n = check_top_n(topn)
    if chunk_candidates is not None and int(chunk_candidates) < 1:
        raise ValueError("chunk_candidates must be >= 1")
    st = model._dev_state
    if st is None:
        raise RuntimeError("feed_state() must be called before predict_step (ItemsStateUpdaterHook.before_run)")
    B, T = d['B'], d['T']
    explicit = None if candidates is None else normalise_candidates(candidates, rt.n_items)      # (range errors before anything is launched)
    if st['n_last'] == 0:
        if explicit is not None and explicit.size:
            raise ValueError("predict: explicit candidates need a fed recent-clicks state with at least one click (recency and novelty are "
                             "normalised with the state's statistics)")
        return empty_result(B, n)      # empty state, no explicit candidates: no candidates, nothing launched
    if d.get('empty_predict'):
        return empty_result(B, n)
    cand, K_dev, K, host_ids = _candidates(model, explicit)
    if K == 0:
        return empty_result(B, n)
    P_last, d2, dev = d['P_last'], d['last'], rt.device
    train_negs = getattr(model, 'predict_train_negative_samples', None) or model.negative_samples
    Nc = int(chunk_candidates) if chunk_candidates is not None else default_chunk_width(B, T, train_negs, P_last, K)
    chunks = -(-K // Nc)
    pl = _input_clicks(model, d)
    s = rt.stream()
    plc = rt.plan(P_last, 1, Nc, model.negative_sample_from_buffer, P_last)
    plc.pos, plc.P, plc.PC = None, P_last, P_last * plc.NC
    torch.cuda.current_stream().wait_event(d2['uploaded'])
    if plc.grouped_ev is not None:
        torch.cuda.current_stream().wait_event(plc.grouped_ev)
        plc.grouped_ev = None
    check(lib.cham_rows_gather(ptr(pl.pred), ptr(d2['rows']), P_last, rt.layout.C, ptr(plc.pred), s), "cham_rows_gather")
    plc.cur_neg_ids, plc.cur_neg_slot = plc.neg_ids, plc.neg_slot
    top_id = torch.zeros(P_last, n, dtype=torch.int64, device=dev)
    top_score = torch.full((P_last, n), float('-inf'), dtype=torch.float32, device=dev)
    ms = torch.zeros(P_last, 2, dtype=torch.float32, device=dev)
    ms[:, 0] = float('-inf')
    probs = torch.zeros(P_last, n, dtype=torch.float32, device=dev)
    tau = float(model.softmax_temperature)
    for j in range(chunks):      # the contract's chunk order: (m, s) accumulate in it
        check(lib.cham_predict_fill_chunk(ptr(cand), ptr(K_dev), j, Nc, P_last, plc.pmax, ptr(plc.neg_ids), ptr(plc.neg_slot), ptr(plc.pool), s),
              "cham_predict_fill_chunk")
        _score_chunk(model, plc, d2, s)
        check(lib.cham_predict_topn_merge(ptr(plc.logits), ptr(cand), ptr(K_dev), j, Nc, ptr(d2['excl']), T, P_last, n, tau, ptr(top_id),
                                          ptr(top_score), ptr(ms), s), "cham_predict_topn_merge")
    check(lib.cham_predict_topn_finish(ptr(top_score), ptr(ms), P_last, n, tau, ptr(probs), s), "cham_predict_topn_finish")
    if st.get('device'):
        model.articles_recent_pop_norm.note_consumed(d['aci'])      # last read of the state
    model._predict_plan = plc
    out = empty_result(B, n, K, Nc, chunks)
    sess = d['sess']
    out['item_ids'][sess] = top_id.cpu().numpy()
    out['scores'][sess] = top_score.cpu().numpy()
    out['probs'][sess] = probs.cpu().numpy()
    out['P_last'] = P_last
    out['candidates'] = host_ids if host_ids is not None else cand[:K].cpu().numpy()
    return out
