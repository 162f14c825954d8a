"""The input rows of the step: the feature front end (K1) and the PreCAR input layer in its two forms, forward and backward."""
# The step driver (nar_model.NARModuleModel._forward / backward) owns the SCHEDULE - which lane the row grouping, the clicked rows' Z1 and the
# two halves of the backward tail run on, and every event - and asks this module for the arithmetic at the head and the tail of the step:
#   FeatureRows        the resident article tables and feature descriptors, the K1 launches (integer head, row grouping, dynamic raw features,
#                      normalisation statistics, the two assembles) and their backward (dgamma / dbeta, the embedding-table gradients)
#   FactorisedInput    PreCAR input layer as U = Xc W1c + b1 (per click) + V = Xi W1i (per unique item row): every step without dropout
#   DenseInput         ... on the dense [clicked | candidates] x [ctx | item] rows x the stacked W1, a mask per element (dropout_keep_prob < 1)
#   Dropout            the mask generator of one step: its key and one method that launches cham_dropout; the SITE_* numbers name the masks
# FeatureRows is built once per runtime and sets the tables on it, under the names tests and tools read: rt.ace, created, meta_cat, ctx_desc,
# item_desc, item_segs, n_item_segs, item_singles, n_item_singles, ctx_emb_groups, item_emb_groups, item_lds.  On a plan it owns ids_all,
# ref_ts, rec_raw, nov_raw, stats, stat_scratch, w_rows, perm, seg, group_ws, Xc_raw, Xc_s, Xi_raw, Xi_s (StepPlan allocates them) and cat, the
# context columns of the step (the embedding gradients scan them again).
# _forward chooses the input form once and stores it on the plan (pl.precar, beside pl.arm and pl.rnn); backward() reads it there.  A form
# implements alloc (its plan buffers: U, dU, V, dV / Xd, dXd, dUx, dVx, drop_ws, Z1f, dZ1f and the dropped FC1d, rnn_drop), forward (the
# projections), clicked_z1 (the clicked rows' Z1, where the schedule wants it), backward (dZ1 -> the gradients the two chains start from),
# ctx_chain and item_chain (weight gradient, d(features), feature backward of one half: independent of each other, so on any two lanes); a
# dense form also carries W1, gW1, Fw and dropout, which the arm's z1(pl, s, form) and the schedule's own dropout sites read.  A new form
# subclasses the nearest one and overrides what differs; a new feature stage is a method of FeatureRows and one line of the driver.
# Every method enqueues on torch's current stream (`s`: its raw handle where the driver has it, rt.stream() otherwise).
import numpy as np
import torch

from .._lib import check, ptr
from .candidate_rows import ACT_LEAKY
from .layout import COL_ITEMEMB

# Dropout sites (cham_dropout's site_first / site_rest: one mask stream per tf.layers.dropout / DropoutWrapper of the reference)
SITE_INPUT_CLICKED = 16       # nar_model.py:338   input_user_items_features
SITE_INPUT_POSITIVE = 17      # nar_model.py:352   positive_user_items_features (first row of a position's candidate group)
SITE_INPUT_NEGATIVE = 18      # nar_model.py:368   negative_user_items_features (the group's other rows)
SITE_FC1 = 19                 # nar_model.py:418   rnn_outputs_fc1
SITE_RNN_OUT = 20             # nar_model.py:1331  DropoutWrapper(output_keep_prob) of recurrent layer l: SITE_RNN_OUT + l


def step_scalar(rt, name, value, cast=None):
    """(entry point, argument) of a launch that reads a per-step scalar: `name`_dev and the runtime's step-scalar record, or `name` and the value
    (through `cast`, on this arm only: the batch of a captured step carries None for its host scalars)."""
    return (name + '_dev', ptr(rt.scalars)) if rt.dev_scalars else (name, value if cast is None else cast(value))


class Dropout:
    """Masks of one step: keyed by (seed, step, site, global row, column), so the backward pass regenerates the mask of its forward site."""

    def __init__(self, rt, keep, step, T, row_begin):
        self.rt, self.keep, self.seed, self.step, self.T, self.row_begin = rt, float(keep), rt.tf_random_seed, step & 0xFFFFFFFF, T, row_begin

    def apply(self, x, y, rows, cols, ld, site_first, site_rest, group, posmap, col_split=None, col_shift=0):
        rt = self.rt
        check(rt.lib.cham_dropout(ptr(x), ptr(y), rows, cols, ld, self.keep, self.seed, self.step, site_first, site_rest, group, ptr(posmap), self.T,
                                  self.row_begin, cols if col_split is None else col_split, col_shift, rt.stream()), "cham_dropout")


class FeatureRows:
    """Resident article tables (ACE matrix, metadata - re-fed from numpy every step by the reference, nar_model.py:1458-1467), descriptors, K1."""

    def __init__(self, rt, ace):
        self.rt = rt
        L, dev, acfg, meta = rt.layout, rt.device, rt.params['articles_features_config'], rt.params['articles_metadata']
        rt.ace = torch.from_numpy(ace).to(dev)
        rt.created = torch.from_numpy(np.ascontiguousarray(meta['created_at_ts'], dtype=np.int64)).to(dev)

        def meta_column(n):
            # metadata columns live in ONE int64 table.  A float-valued numerical article feature (config dtype 'float',
            # nar_model.py:755-757) is stored as its float32 bit pattern and read back bit-exactly by the assemble kernels
            # (layout.meta_is_float -> descriptor sub-field 1); everything else as the integer it is.
            a = np.asarray(meta[n])
            if n in L.meta_is_float:
                return np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
            if acfg[n]['type'] == 'numerical' and not np.issubdtype(a.dtype, np.integer) and not np.array_equal(a, np.round(a)):
                raise ValueError("article feature %r holds non-integer values but its config says dtype %r: declare it "
                                 "{'type': 'numerical', 'dtype': 'float'}" % (n, acfg[n].get('dtype')))
            return a.astype(np.int64)
        mc = np.stack([meta_column(n) for n in L.meta_names]) if L.meta_names else np.zeros((1, rt.n_items), np.int64)
        rt.meta_cat = torch.from_numpy(np.ascontiguousarray(mc)).to(dev)
        rt.ctx_desc = torch.from_numpy(L.ctx_descriptors()).to(dev)
        rt.ctx_emb_groups, rt.item_emb_groups = L.ctx_emb_groups(), L.item_emb_groups()
        segs, singles = L.item_segments()
        rt.item_segs, rt.n_item_segs = torch.from_numpy(np.ascontiguousarray(segs)).to(dev), int(segs.shape[0])
        rt.item_singles, rt.n_item_singles = torch.from_numpy(np.ascontiguousarray(singles)).to(dev), int(singles.shape[0])
        # item rows through LDS tiles (csrc/features.hip k_item_assemble_lds); rows too wide for the tile: one thread per element
        rt.item_lds = L.Fi * 4 * 8 <= 64 * 1024
        rt.item_desc = torch.from_numpy(L.item_descriptors()).to(dev)

    # ---- forward.  Item row set = [clicked ; positives ; pool slots ; pad item 0]: RV = 2 P + pmax + 1 rows
    def step_ints(self, pl, d, s):      # one launch: the ids and reference time stamps of the item rows, seq_len and the position mask of the stages below
        rt = self.rt
        fn, max_ts = step_scalar(rt, 'cham_step_ints', d['max_ts'], int)
        check(getattr(rt.lib, fn)(ptr(d['ic_rows']), ptr(d['ln_rows']), ptr(pl.pool), ptr(d['ets_rows']), max_ts, pl.P, pl.pmax, ptr(d['seq_len']),
                                  pl.B, ptr(d['mask']), ptr(pl.ids_all), ptr(pl.ref_ts), ptr(pl.seq_len), ptr(pl.mask), s), fn)

    def group_rows(self, pl, stream):      # rows of equal id made contiguous: the embedding-gradient sums of the backward pass (depends on ids only)
        check(self.rt.lib.cham_group_rows(ptr(pl.ids_all), 2 * pl.P + pl.pmax + 1, self.rt.item_id_bits, ptr(pl.perm), ptr(pl.seg), ptr(pl.group_ws),
                                          pl.group_ws.numel() * 4, stream), "cham_group_rows")

    def dynamic_raw(self, pl, st, s):      # recency and novelty of every item row, before normalisation
        rt = self.rt
        check(rt.lib.cham_item_dynamic_raw(ptr(pl.ids_all), ptr(pl.ref_ts), 2 * pl.P + pl.pmax + 1, ptr(rt.created), ptr(st['pop_norm']),
                                           ptr(pl.rec_raw), ptr(pl.nov_raw), s), "cham_item_dynamic_raw")

    def norm_stats(self, pl, d, st, s):
        """Mean / std of recency and novelty over the recent clicks `st` holds: the device buffer (max_ts from the step-scalar record or by
        value) or the host's upload; nothing clicked yet: over the batch's own rows, per group (clicked, positives, pool)."""
        rt, lib, BT = self.rt, self.rt.lib, pl.P
        if st['n_last'] > 0:
            fn, max_ts = (step_scalar(rt, 'cham_norm_stats_from_buffer', d['max_ts']) if st.get('device') else
                          ('cham_norm_stats_from_recent', d['max_ts']))
            check(getattr(lib, fn)(ptr(st['last']), st['n_last'], max_ts, ptr(rt.created), ptr(st['pop_norm']), ptr(pl.stat_scratch),
                                   ptr(pl.stats), s), fn)
            return
        # very first batch: population = the call's own non-pad ids (nar_model.py:1078-1084)
        check(lib.cham_row_weights(ptr(pl.ids_all), 2 * BT, ptr(pl.cur_neg_slot), BT * pl.N, pl.pmax, ptr(pl.pool), ptr(pl.w_rows),
                                   pl.w_rows[2 * BT:].data_ptr(), s), "cham_row_weights")
        for g, (a, b) in enumerate([(0, BT), (BT, 2 * BT), (2 * BT, 2 * BT + pl.pmax + 1)]):
            check(lib.cham_norm_stats_from_rows(pl.rec_raw[a:].data_ptr(), pl.nov_raw[a:].data_ptr(), pl.w_rows[a:].data_ptr(), b - a,
                                                pl.stats[g].data_ptr(), s), "cham_norm_stats_from_rows")

    def norm_stats_first_batch_of_shard(self, pl, d, st, neg_slot, s):
        """The very first batch when the call is a ROW SHARD of it (micro-batch, data-parallel rank): the population is the GLOBAL batch's
        non-pad ids, not the shard's - the whole-batch step normalises every row with the statistics of all clicked ids, all positives and
        all sampled negatives (nar_model.py:1078-1084, 1168-1181), and every shard must use the same ones.  Every shard holds what that
        takes: the global ids d['aci'] [Bg, T + 1], time stamps and session lengths d['g_seq_len'] - the valid positions are t < length, as
        upload_batch masks them; the clicked id of position t is aci[:, t], its positive aci[:, t + 1], the session's last one the label in
        column T - and `neg_slot`, the pool slots of the GLOBAL batch's negatives (NARModuleModel._whole_batch_neg_slots).  Same rows in
        the same order and the same launches as norm_stats() on the whole batch's valid positions, into pl.stats.  Once per training run:
        scratch tensors, one host synchronisation (the boolean compaction)."""
        rt, lib, T, pmax = self.rt, self.rt.lib, d['T'], pl.pmax
        aci, ets, lens = d['aci'], d['g_event_ts'], d['g_seq_len'].long().clamp(0, T)
        valid = torch.arange(T, device=aci.device)[None, :] < lens[:, None]
        nxt = aci[:, 1:].clone()
        has = lens > 0
        nxt[has, lens[has] - 1] = aci[has, T]
        ids_c, ts_c, ids_p = aci[:, :T][valid], ets[valid], nxt[valid]
        P = ids_c.numel()
        ids = torch.cat([ids_c, ids_p, pl.pool[:pmax], torch.zeros(1, dtype=torch.int64, device=aci.device)])
        ref_ts = torch.cat([ts_c, ets.max().reshape(1).expand(P + pmax + 1)])
        R = 2 * P + pmax + 1
        rec, nov, w = (torch.empty(R, dtype=torch.float32, device=aci.device) for _ in range(3))
        check(lib.cham_item_dynamic_raw(ptr(ids), ptr(ref_ts), R, ptr(rt.created), ptr(st['pop_norm']), ptr(rec), ptr(nov), s),
              "cham_item_dynamic_raw")
        check(lib.cham_row_weights(ptr(ids), 2 * P, ptr(neg_slot), neg_slot.numel(), pmax, ptr(pl.pool), ptr(w), w[2 * P:].data_ptr(), s),
              "cham_row_weights")
        for g, (a, b) in enumerate([(0, P), (P, 2 * P), (2 * P, R)]):
            check(lib.cham_norm_stats_from_rows(rec[a:].data_ptr(), nov[a:].data_ptr(), w[a:].data_ptr(), b - a, pl.stats[g].data_ptr(), s),
                  "cham_norm_stats_from_rows")

    def assemble(self, pl, d, s):      # raw + scaled / centred rows: user context (one per position), items (one per row of the item row set)
        rt, lib, L, p, BT = self.rt, self.rt.lib, self.rt.layout, self.rt.p, pl.P
        pl.cat = d['cat']
        check(lib.cham_ctx_assemble(ptr(d['cat']), ptr(d['num']), BT, ptr(rt.ctx_desc), L.Fc, ptr(rt.flat), ptr(p('gamma_ctx')),
                                    ptr(p('beta_ctx')), ptr(pl.Xc_raw), ptr(pl.Xc_s), s), "cham_ctx_assemble")
        rows = (ptr(pl.ids_all), 2 * BT + pl.pmax + 1, BT, 2 * BT, ptr(rt.meta_cat), rt.n_items, ptr(rt.ace), L.D, ptr(pl.rec_raw), ptr(pl.nov_raw),
                ptr(pl.stats), ptr(rt.item_desc), L.Fi)
        out = (ptr(rt.flat), ptr(p('gamma_item')), ptr(p('beta_item')), ptr(pl.Xi_raw), ptr(pl.Xi_s), s)
        if rt.item_lds:
            check(lib.cham_item_assemble_lds(*rows, ptr(rt.item_segs), rt.n_item_segs, ptr(rt.item_singles) if rt.n_item_singles else None,
                                             rt.n_item_singles, *out), "cham_item_assemble_lds")
        else:
            check(lib.cham_item_assemble(*rows, *out), "cham_item_assemble")

    # ---- backward
    def feature_bwd(self, dX, Xraw, R, F, gname, bname):
        # dgamma / dbeta column sums: the coalesced two-launch form through this lane's workspace (CHAM_FEATURE_BWD_WS=0: one workgroup per column)
        rt, g = self.rt, self.rt.g
        if rt.feature_bwd_ws:
            ws = rt._lane_ws('gemm_ws')
            check(rt.lib.cham_feature_bwd_ws(ptr(dX), ptr(Xraw), R, F, ptr(g(gname)), ptr(g(bname)), ptr(ws), ws.numel() * 4, rt.stream()),
                  "cham_feature_bwd_ws")
        else:
            check(rt.lib.cham_feature_bwd(ptr(dX), ptr(Xraw), R, F, ptr(g(gname)), ptr(g(bname)), rt.stream()), "cham_feature_bwd")

    def ctx_bwd(self, pl):      # scale / center and the embedding tables of the user-context rows
        rt, BT, Fc = self.rt, pl.P, self.rt.layout.Fc
        self.feature_bwd(pl.dXc, pl.Xc_raw, BT, Fc, 'gamma_ctx', 'beta_ctx')
        n_rows_cat = pl.cat.shape[1]
        for kind, feat, c0, dim, card, off in rt.ctx_emb_groups:
            check(rt.lib.cham_emb_grad_scan(ptr(pl.dXc), BT, Fc, c0, dim, ptr(rt.p('gamma_ctx')), pl.cat.data_ptr() + 8 * feat * n_rows_cat,
                                            None, card, rt.grads.data_ptr() + 4 * off, rt.stream()), "cham_emb_grad_scan")

    def item_bwd(self, pl):      # ... of the item rows: the item embedding by the forward's row grouping, metadata embeddings by a scan
        rt, lib, RV, Fi = self.rt, self.rt.lib, 2 * pl.P + pl.pmax + 1, self.rt.layout.Fi
        self.feature_bwd(pl.dXi, pl.Xi_raw, RV, Fi, 'gamma_item', 'beta_item')
        for kind, feat, c0, dim, card, off in rt.item_emb_groups:
            if kind == COL_ITEMEMB:
                if pl.grouped_ev is not None:
                    torch.cuda.current_stream().wait_event(pl.grouped_ev)
                check(lib.cham_emb_grad_grouped(ptr(pl.dXi), RV, Fi, c0, dim, ptr(rt.p('gamma_item')), ptr(pl.ids_all), ptr(pl.perm),
                                                ptr(pl.seg), rt.grads.data_ptr() + 4 * off, rt.stream()), "cham_emb_grad_grouped")
            else:
                check(lib.cham_emb_grad_scan(ptr(pl.dXi), RV, Fi, c0, dim, ptr(rt.p('gamma_item')), rt.meta_cat.data_ptr() + 8 * feat * rt.n_items,
                                             ptr(pl.ids_all), card, rt.grads.data_ptr() + 4 * off, rt.stream()), "cham_emb_grad_scan")


class FactorisedInput:
    """U (per click) + V (per unique item row): the layer's products run once per row of the two feature matrices, the arm combines them."""
    dropout = None          # the step's mask generator (schedule: the FC1 and recurrent-output sites; the arm's z1 takes the dense rows)

    def __init__(self, rt):
        self.rt = rt

    def alloc(self, pl, f32):
        C = pl.C
        pl.U, pl.dU = f32(pl.BT, C), f32(pl.BT, C)
        pl.V, pl.dV = f32(pl.RV, C), f32(pl.RV, C)

    # ---- forward
    def forward(self, pl, s):
        rt, p, L, C = self.rt, self.rt.p, self.rt.layout, pl.C
        rt.gemm(pl.Xc_s, p('W1c'), pl.U, pl.P, C, L.Fc, L.Fc, C, C, bias=p('b1'))
        rt.gemm(pl.Xi_s, p('W1i'), pl.V, 2 * pl.P + pl.pmax + 1, C, L.Fi, L.Fi, C, C)

    def clicked_z1(self, pl, s):      # PreCAR combine of the clicked-input rows: they feed the recurrent branch
        check(self.rt.lib.cham_combine_fwd(ptr(pl.U), ptr(pl.V), pl.C, pl.P, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.Z1), 0, pl.P, s),
              "cham_combine_fwd")

    # ---- backward
    def backward(self, pl, ws, s):      # dZ1 -> dU, dV by the arm's deterministic scatter
        pl.arm.combine_bwd(pl, ws, s)

    def ctx_chain(self, pl):      # user-context half: weight gradient, bias, d(features), then scale / center and the embedding tables
        rt, p, g, C, BT, Fc = self.rt, self.rt.p, self.rt.g, pl.C, pl.P, self.rt.layout.Fc
        rt.gemm(pl.Xc_s, pl.dU, g('W1c'), Fc, C, BT, Fc, C, C, transA=1, splits=0)
        rt.colsum(pl.dU, C, BT, C, g('b1'))
        rt.gemm(pl.dU, p('W1c'), pl.dXc, BT, Fc, C, C, C, Fc, transB=1)
        rt.features.ctx_bwd(pl)

    def item_chain(self, pl):      # item half
        rt, C, RV, Fi = self.rt, pl.C, 2 * pl.P + pl.pmax + 1, self.rt.layout.Fi
        rt.gemm(pl.Xi_s, pl.dV, rt.g('W1i'), Fi, C, RV, Fi, C, C, transA=1, splits=0)
        rt.gemm(pl.dV, rt.p('W1i'), pl.dXi, RV, Fi, C, C, C, Fi, transB=1)
        rt.features.item_bwd(pl)


class DenseInput(FactorisedInput):
    """dropout_keep_prob < 1 (nar_model.py:338, 352, 368): the per-element masks make every CAR row occurrence-specific, so the layer runs on the
    dense [clicked | candidates] x [ctx | item] rows against the stacked W1 = [W1c ; W1i].  Built per step: it carries the step's masks."""

    def __init__(self, rt, dropout):
        self.rt, self.dropout = rt, dropout
        L = rt.layout
        e1, e2 = L.entries['W1c'], L.entries['W1i']
        assert e2.offset == e1.offset + e1.size
        self.Fw = L.Fc + L.Fi
        self.W1 = rt.flat[e1.offset:e2.offset + e2.size].view(self.Fw, L.C)
        self.gW1 = rt.grads[e1.offset:e2.offset + e2.size].view(self.Fw, L.C)

    def alloc(self, pl, f32=None):
        """Buffers of the dropout path (dense input rows, dropped FC1 / recurrent outputs) - on a plan's first step with dropout."""
        rt = self.rt
        if not rt.b16:
            pl.ensure_rows('Z1'); pl.ensure_rows('dZ2')
        if pl.Xd is None:
            L, Fw = rt.layout, self.Fw
            f32 = f32 or (lambda *s: torch.empty(*s, dtype=torch.float32, device=rt.device))
            pl.Xd, pl.dXd = f32(pl.Rall, Fw), f32(pl.Rall, Fw)
            pl.dUx, pl.dVx = f32(pl.BT, Fw), f32(pl.RV, Fw)
            pl.FC1d = f32(pl.BT, 512)
            pl.rnn_drop = [f32(pl.BT, L.Hp) for _ in range(L.L)]
            need = rt.lib.cham_combine_bwd_workspace_bytes(Fw, pl.B * pl.T, pl.N, pl.pmax)
            pl.drop_ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=rt.device)
            if rt.b16:      # bf16 configuration: the dense PreCAR layer computes / consumes fp32 images of the bf16-resident candidate rows
                pl.Z1f, pl.dZ1f = f32(pl.Rall, L.C), f32(pl.Rall, L.C)

    def mask_rows(self, pl, X):      # the three input sites on the dense rows: context columns by position, item columns by occurrence
        L, BT, Fw, Fc = self.rt.layout, pl.P, self.Fw, self.rt.layout.Fc
        self.dropout.apply(X, X, BT, Fw, Fw, SITE_INPUT_CLICKED, SITE_INPUT_CLICKED, 1, pl.pos, Fc, Fc - L.f_ctx)
        self.dropout.apply(X[BT:], X[BT:], pl.PC, Fw, Fw, SITE_INPUT_POSITIVE, SITE_INPUT_NEGATIVE, pl.NC, pl.pos, Fc, Fc - L.f_ctx)

    def forward(self, pl, s):      # dense rows, masks, and the clicked-input rows' Z1 right away (the arm's z1 takes the candidate rows)
        rt, L, C, BT, Fw = self.rt, self.rt.layout, pl.C, pl.P, self.Fw
        self.alloc(pl)
        check(rt.lib.cham_dense_rows(ptr(pl.Xc_s), L.Fc, ptr(pl.Xi_s), L.Fi, BT, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.Xd), s), "cham_dense_rows")
        self.mask_rows(pl, pl.Xd)
        rt.gemm(pl.Xd, self.W1, pl.Z1, BT, C, Fw, Fw, C, C, bias=rt.p('b1'), act=ACT_LEAKY)

    def clicked_z1(self, pl, s):      # written by forward()
        pass

    def backward(self, pl, ws, s):
        # one weight gradient over all CAR rows, d(input rows) masked, then summed per position / per item row by the same deterministic
        # scatter as the factorised form (width Fc + Fi)
        rt, C, BT, Fw, Fc = self.rt, pl.C, pl.P, self.Fw, self.rt.layout.Fc
        Rall, RV = BT + pl.PC, 2 * BT + pl.pmax + 1
        dZ1 = pl.arm.dense_dZ1(pl, s)
        rt.gemm(pl.Xd, dZ1, self.gW1, Fw, C, Rall, Fw, C, C, transA=1, splits=0)
        rt.colsum(dZ1, C, Rall, C, rt.g('b1'))
        rt.gemm(dZ1, self.W1, pl.dXd, Rall, Fw, C, C, C, Fw, transB=1)
        self.mask_rows(pl, pl.dXd)
        check(rt.lib.cham_combine_bwd(ptr(pl.dXd), Fw, BT, pl.N, pl.pmax, ptr(pl.cur_neg_slot), ptr(pl.dUx), ptr(pl.dVx), ptr(pl.drop_ws),
                                      pl.drop_ws.numel() * 4, s), "cham_combine_bwd")
        pl.dXc[:BT].copy_(pl.dUx[:BT, :Fc]); pl.dXi[:RV].copy_(pl.dVx[:RV, Fc:])

    def ctx_chain(self, pl):      # (the weight gradient and d(features) of both halves came out of backward())
        self.rt.features.ctx_bwd(pl)

    def item_chain(self, pl):
        self.rt.features.item_bwd(pl)
