"""Full-candidate evaluation: the rank of every valid click's label among ALL recent candidates (--eval_full_candidates)."""
# Runs inside NARModuleModel.evaluate_step, behind the sampled ranking: the step's plan still holds pl.pred [P, C] of the valid positions, so
# the input-click stages are not run again.  The valid positions are walked in ROW BLOCKS of exactly Rb = B rows (the last one padded by
# repeating its first row) on ONE second plan of shape (B = Rb, T = 1, N = Nc) - the plan shape of nar/predict.py, with the real label in the
# label column - and the candidates in chunks of Nc: cham_predict_fill_chunk, predict._score_chunk, cham_eval_full_rank_merge per chunk, in
# the order 0 .. ceil(K / Nc) - 1; cham_eval_full_rank_scatter per block; one cham_eval_rank_hist per batch into the full record.
# The label's logit a chunk's candidates are compared with is column 0 of THAT chunk's logits.
# Nothing here writes the weights, the recent-clicks state, global_step, the sampler keys or a record of the sampled evaluation.
import torch

from .._lib import check, ptr
from .predict import _candidates, _score_chunk, default_chunk_width

MAX_T1 = 128           # cham_eval_full_rank_merge holds a session's clicks + its last label in LDS
RECOMMENDER = 'chameleon_full'


def check_session_length(T):
    if T + 1 > MAX_T1:
        raise ValueError("eval_full_candidates: sessions of %d click positions - cham_eval_full_rank_merge holds at most %d ids per session "
                         "(clicks + the last label)" % (T, MAX_T1))


def new_record(model, topn, t_cap, chunk_candidates=None, block_rows=None, return_scores=False):
    """The state behind NARModuleModel.enable_full_candidate_ranking (bounds: those of enable_rank_histogram)."""
    if not 1 <= topn <= 256:
        raise ValueError("the rank histogram needs 1 <= eval_metrics_top_n <= 256 (got %d)" % topn)
    if t_cap < 1:
        raise ValueError("t_cap must be >= 1")
    for name, v in (('chunk_candidates', chunk_candidates), ('block_rows', block_rows)):
        if v is not None and int(v) < 1:
            raise ValueError("%s must be >= 1" % name)
    dev = model.rt.device
    return dict(topn=int(topn), t_cap=int(t_cap), hist=torch.zeros(int(t_cap), int(topn) + 1, dtype=torch.int64, device=dev),
                pop_sum=torch.zeros(int(t_cap), dtype=torch.float64, device=dev),
                chunk_candidates=None if chunk_candidates is None else int(chunk_candidates),
                block_rows=None if block_rows is None else int(block_rows), return_scores=bool(return_scores),
                batches=0, K_sum=0, last=None)


def results(model, by_session_position=False):
    """{'hitrate_at_n_chameleon_full': ..., 'mrr_at_n_chameleon_full': ..., 'ndcg_at_n_chameleon_full': ... (+ the per-position hit rates),
    'full_candidates_mean': mean K over the evaluation's batches} of the evaluate_steps since enable_full_candidate_ranking."""
    from .evaluation import compute_metrics_results
    from .metrics import HitRate, HitRateBySessionPosition, MRR, NDCG, accuracy_from_rank_hist
    fr = model._fr
    acc = accuracy_from_rank_hist(fr['hist'].cpu().numpy(), fr['pop_sum'].cpu().numpy(), fr['topn'])

    class _Value:
        def __init__(self, metric):
            self.name = metric

        def result(self):
            return acc[self.name]
    names = [HitRate.name, MRR.name, NDCG.name] + ([HitRateBySessionPosition.name] if by_session_position else [])
    out = compute_metrics_results([_Value(n) for n in names], recommender=RECOMMENDER)
    out['full_candidates_mean'] = fr['K_sum'] / float(fr['batches']) if fr['batches'] else float('nan')
    return out


def rank_step(model, pl, d):
    """One EVAL batch: see the head of this file.  pl = the step's plan after forward(), d = its device batch."""
    rt, lib, st, fr = model.rt, model.rt.lib, model._dev_state, model._fr
    B, T, dev = d['B'], d['T'], rt.device
    check_session_length(T)
    if T > fr['t_cap']:
        raise ValueError("evaluation batch of %d click positions: the full-candidate record was enabled for %d" % (T, fr['t_cap']))
    s = rt.stream()
    label_rank = torch.full((B, T), -1, dtype=torch.int32, device=dev)
    n_comp = torch.zeros(B, T, dtype=torch.int32, device=dev)
    # the valid positions: flat = b T + t of each, rows = its row of pl.pred and of the batch's per-row tensors
    if d['pos'] is not None:
        flat, P = d['pos'], int(d['P'])
        rows = torch.arange(P, dtype=torch.int32, device=dev)
    else:
        flat = rows = torch.nonzero(d['mask'].view(-1)).view(-1).to(torch.int32)
        P = int(flat.numel())
    K = 0
    if st['n_last'] > 0 and P > 0:
        cand, K_dev, K, _ = _candidates(model, None)      # once per batch, one read-back of K
    out = dict(label_rank=label_rank, competitors=n_comp, K=K, Nc=0, blocks=0, chunks=0)
    if P > 0 and K == 0:       # no candidates, no competitors: every valid click ranks first
        label_rank.view(-1)[flat.long()] = 0
    elif P > 0:
        Rb = fr['block_rows'] or B
        Nc = fr['chunk_candidates'] or default_chunk_width(B, T, model.negative_samples, Rb, K)
        chunks, blocks = -(-K // Nc), -(-P // Rb)
        out.update(Nc=Nc, blocks=blocks, chunks=chunks)
        # every block's rows (a padding row repeats its block's first row): flat position, row of pl.pred, session row of aci
        i = torch.arange(blocks * Rb, device=dev)
        i = torch.where(i < P, i, (i // Rb) * Rb)
        flat_all, rows_all = flat[i].contiguous(), rows[i].contiguous()
        sess_all = (torch.div(flat_all, T, rounding_mode='floor') + int(d['row_begin'])).to(torch.int32)
        ones_i, ones_m = torch.ones(Rb, dtype=torch.int32, device=dev), torch.ones(Rb, dtype=torch.uint8, device=dev)
        beat, comp = torch.zeros(Rb, dtype=torch.int32, device=dev), torch.zeros(Rb, dtype=torch.int32, device=dev)
        plc = rt.plan(Rb, 1, Nc, model.negative_sample_from_buffer, Rb)
        plc.pos, plc.P, plc.PC = None, Rb, Rb * plc.NC
        if plc.grouped_ev is not None:
            torch.cuda.current_stream().wait_event(plc.grouped_ev)
            plc.grouped_ev = None
        plc.cur_neg_ids, plc.cur_neg_slot = plc.neg_ids, plc.neg_slot
        kept = [] if fr['return_scores'] else None
        for k in range(blocks):
            sl = slice(k * Rb, (k + 1) * Rb)
            rows_k, flat_k, sess_k = rows_all[sl].clone(), flat_all[sl].clone(), sess_all[sl].clone()
            r64 = rows_k.long()
            # the block's ids, time stamps, context columns and labels, gathered on the device from the batch's own tensors (the label goes
            # where prediction puts the pad item)
            d2 = dict(B=Rb, T=1, Bg=Rb, row_begin=0, sum_mask=float(Rb), max_ts=d['max_ts'], P=Rb, pos=None, ic_rows=d['ic_rows'][r64],
                      ln_rows=d['ln_rows'][r64], ets_rows=d['ets_rows'][r64], seq_len=ones_i, mask=ones_m, cat=d['cat'][:, r64].contiguous(),
                      num=d['num'][:, r64].contiguous())
            check(lib.cham_rows_gather(ptr(pl.pred), ptr(rows_k), Rb, rt.layout.C, ptr(plc.pred), s), "cham_rows_gather")
            beat.zero_()
            comp.zero_()
            for j in range(chunks):
                check(lib.cham_predict_fill_chunk(ptr(cand), ptr(K_dev), j, Nc, Rb, plc.pmax, ptr(plc.neg_ids), ptr(plc.neg_slot), ptr(plc.pool), s),
                      "cham_predict_fill_chunk")
                _score_chunk(model, plc, d2, s)
                check(lib.cham_eval_full_rank_merge(ptr(plc.logits), ptr(cand), ptr(K_dev), j, Nc, ptr(d2['ln_rows']), ptr(sess_k),
                                                    ptr(d['aci']), T + 1, Rb, ptr(beat), ptr(comp), s), "cham_eval_full_rank_merge")
                if kept is not None:
                    kept.append(plc.logits[:Rb].clone())
            check(lib.cham_eval_full_rank_scatter(ptr(beat), ptr(comp), ptr(flat_k), min(Rb, P - k * Rb), ptr(label_rank), ptr(n_comp), s),
                  "cham_eval_full_rank_scatter")
        if kept is not None:      # tests: per click the [K] scores and the label's logit of every chunk (NaN at padded positions)
            lg = torch.stack(kept).view(blocks, chunks, Rb, 1 + Nc)
            sc = lg[..., 1:].permute(0, 2, 1, 3).reshape(blocks * Rb, chunks * Nc)[:P, :K]
            lab = lg[..., 0].permute(0, 2, 1).reshape(blocks * Rb, chunks)[:P]
            scores = torch.full((B * T, K), float('nan'), dtype=torch.float32, device=dev)
            label_logit = torch.full((B * T, chunks), float('nan'), dtype=torch.float32, device=dev)
            scores[flat.long()], label_logit[flat.long()] = sc, lab
            out.update(scores=scores.view(B, T, K).cpu().numpy(), label_logit=label_logit.view(B, T, chunks).cpu().numpy(),
                       candidates=cand[:K].cpu().numpy())
    check(lib.cham_eval_rank_hist(ptr(label_rank), ptr(d['label_next']), B, T, fr['topn'], ptr(st['pop_norm']), rt.n_items, ptr(fr['hist']),
                                  ptr(fr['pop_sum']), fr['t_cap'], s), "cham_eval_rank_hist")
    if st.get('device'):
        model.articles_recent_pop_norm.note_consumed(d['aci'])      # the state is read up to here: its update waits for this
    fr['batches'] += 1
    fr['K_sum'] += K
    fr['last'] = out


def outputs(model):
    """label_rank / competitors int32 [B, T] as numpy + K, Nc, blocks, chunks (+ scores, label_logit, candidates with return_scores) of the
    last evaluate_step."""
    last = model._fr['last']
    out = dict(last)
    out['label_rank'], out['competitors'] = last['label_rank'].cpu().numpy(), last['competitors'].cpu().numpy()
    return out
