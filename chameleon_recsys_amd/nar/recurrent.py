"""The launch paths of the recurrent stack: one class per way the time loop of a recurrent layer is launched."""
# The step driver (nar_model.NARModuleModel._forward / backward) owns the SCHEDULE - lanes, events, the input projections x W_x, compaction and
# dropout around the layers, the hand-over to the CAR dgrad at layer 0 - and asks the path of the step for the time loop of each layer:
#   FusedRnn        both cells, one workgroup per 32 sessions runs all T steps (csrc/rnn.hip k_ugrnn_* / k_gru_*; Hp <= 512, GRU <= 384)
#   CoopUgrnn       UGRNN at Hp 256 on eight cooperating workgroups per 32 sessions (csrc/rnn_coop.hip), steps of few candidate rows
#   StepwiseUgrnn   widths beyond LDS: per time step 1 GEMM + 1 point-wise kernel forward, 1 kernel + copy + accumulating GEMM backward
#   StepwiseGru     ... 2 GEMMs + 2 kernels forward, 2 kernels + 2 GEMMs + 1 copy backward (the candidate needs r * h of ALL hidden units)
#   StepwiseLstm    the LSTM at every width: the UGRNN's launches over four gate blocks; the cell state c lives in the point kernels
# path_class() is the one place that chooses; the driver stores the path on the plan (pl.rnn), as it does pl.arm, and backward() reads it: a
# backward that chose differently would read planes its forward never wrote.
# A path is handed a HOST and uses nothing else of it: host.lib, host.gemm(A, B, C, M, N, K, lda, ldb, ldc, transB=, accumulate=, force_f32=),
# the weight lookup host.p(name) - and, in wgrads() only, host.g(name) and host.colsum() - so scripts/bench_rnn_stepwise.py drives these classes
# without a model.  (host.lib is read per call: tools replace it on a live runtime.)  Buffers: the plan keeps what every path reads and
# writes (seq_len, xproj, dxproj, rnn_out, hprev, G, Cc, R, RH, drnn - the driver and the weight gradients read them too; the LSTM keeps its
# gates i, j, f, o in G, Cc, R, RH); alloc() adds what
# only this path needs, under the names below.  A new path subclasses the nearest one, implements alloc / forward / backward for one layer
# `l` on the current stream (`s`: its raw handle), leaves rnn_out / hprev / G / Cc (GRU: + R, RH) and dxproj as the others do - wgrads() and
# the driver read them - and gets its line in path_class().
import torch

from .._lib import check, ptr


def default_coop_rows(L):
    """NARRuntime.rnn_coop_rows as built: steps with at most this many candidate rows take the cooperative kernels (-1: never)."""
    # The threshold of the W2 weight gradient's lane (NARRuntime.w2_main_rows) selects the recurrent kernels too: steps with at most this many
    # candidate rows (ragged batches, the shard of a strong-scaling rank) run the UGRNN time steps on eight cooperating workgroups per 32
    # sessions with W_h resident in LDS (csrc/rnn_coop.hip: ~8 us per time step instead of ~33, but 120-155 KB of LDS per workgroup - no CU
    # shared with a plane-GEMM workgroup); a full batch hides the single-workgroup kernels (csrc/rnn.hip, 33 KB of LDS) behind its big GEMMs
    return 131072 if (L.cell == 'ugrnn' and L.Hp == 256 and not L.rnn_stepwise) else -1


def path_class(L, PC, B, coop_rows):
    """The path of a step with PC candidate rows over B sessions (L: the ParamLayout, coop_rows: NARRuntime.rnn_coop_rows at this moment)."""
    if L.rnn_stepwise:
        return {'gru': StepwiseGru, 'lstm': StepwiseLstm}.get(L.cell, StepwiseUgrnn)
    return CoopUgrnn if (0 < PC <= coop_rows and B <= 1024) else FusedRnn


class RnnPath:
    """What the paths share: the shape of a layer and the weight gradients of its recurrent products."""
    launches_per_step = None      # (forward, backward) per time step: GEMMs + kernels (+ the carry copy); None: the whole time loop is one kernel

    def __init__(self, host, L):
        self.host, self.Hp, self.NGH, self.cell = host, L.Hp, L.NG * L.Hp, (1 if L.cell == 'gru' else 0)
        self.WhN = (4 if L.cell == 'lstm' else 2) * L.Hp      # columns of W_h, the recurrent gate product (GRU: r | u; its candidate has W_ch)

    def wgrads(self, pl, l):      # recurrent weights: their forward product runs in the fp32 time-step kernel -> fp32 wgrad in every mode
        h, Hp, NGH, WhN, BTf = self.host, self.Hp, self.NGH, self.WhN, pl.BT
        h.gemm(pl.hprev[l], pl.dxproj, h.g('rnn%d/Wh' % l), Hp, WhN, BTf, Hp, NGH, WhN, transA=1, splits=0, force_f32=True)
        if self.cell == 1:   # candidate kernel: (r * h_prev)^T dz_c
            h.gemm(pl.RH[l], pl.dxproj[:, 2 * Hp:], h.g('rnn%d/Wch' % l), Hp, Hp, BTf, Hp, NGH, Hp, transA=1, splits=0, force_f32=True)
        h.colsum(pl.dxproj, NGH, BTf, NGH, h.g('rnn%d/b' % l))


class FusedRnn(RnnPath):
    """Both cells in the single-workgroup kernels; the backward reads the recurrent weights transposed (WhT: W_gh^T, GRU: + W_ch^T behind it)."""

    def alloc(self, pl, f32):
        pl.WhT = f32(self.NGH, self.Hp)

    def forward(self, pl, l, s):
        check(self.host.lib.cham_rnn_fwd(self.cell, ptr(pl.xproj[l]), ptr(self.host.p('rnn%d/Wh' % l)), ptr(pl.seq_len), pl.B, pl.T, self.Hp,
                                         ptr(pl.rnn_out[l]), ptr(pl.hprev[l]), ptr(pl.G[l]), ptr(pl.Cc[l]), ptr(pl.R[l]), ptr(pl.RH[l]), s), "cham_rnn_fwd")

    def backward(self, pl, l, s):
        lib, p, Hp = self.host.lib, self.host.p, self.Hp
        check(lib.cham_transpose_f32(ptr(p('rnn%d/Wh' % l)), Hp, 2 * Hp, ptr(pl.WhT), s), "cham_transpose_f32")
        if self.cell == 1:
            check(lib.cham_transpose_f32(ptr(p('rnn%d/Wch' % l)), Hp, Hp, pl.WhT[2 * Hp:].data_ptr(), s), "cham_transpose_f32")
        check(lib.cham_rnn_bwd(self.cell, ptr(pl.drnn), ptr(pl.WhT), ptr(pl.seq_len), pl.B, pl.T, Hp, ptr(pl.hprev[l]), ptr(pl.G[l]),
                               ptr(pl.Cc[l]), ptr(pl.R[l]), ptr(pl.dxproj), s), "cham_rnn_bwd")


class CoopUgrnn(FusedRnn):
    """Cooperative UGRNN time steps.  A plan's steps alternate between this path and the fused one (by their candidate rows): allocates alike."""

    def __init__(self, host, L):
        FusedRnn.__init__(self, host, L)
        self._ws = {}

    def ws(self, pl):
        """Exchange buffers + flags of the cooperative kernels for batches of pl.B sessions (zero-initialised once; the forward and the
        backward of a step run on the same lane and share it)."""
        ws = self._ws.get(pl.B)
        if ws is None:
            nb = int(self.host.lib.cham_rnn_coop_workspace_bytes(pl.B, self.Hp))
            ws = self._ws[pl.B] = torch.zeros(nb, dtype=torch.uint8, device=pl.seq_len.device)
        return ws

    def timed_out(self, s):
        """True if a cooperating workgroup ever gave up a bounded spin (synchronises)."""
        return any(int(self.host.lib.cham_rnn_coop_timeouts(ptr(ws), B, self.Hp, s)) != 0 for B, ws in self._ws.items())

    def forward(self, pl, l, s):
        ws = self.ws(pl)
        check(self.host.lib.cham_ugrnn_fwd_coop(ptr(pl.xproj[l]), ptr(self.host.p('rnn%d/Wh' % l)), ptr(pl.seq_len), pl.B, pl.T, self.Hp,
                                                ptr(pl.rnn_out[l]), ptr(pl.hprev[l]), ptr(pl.G[l]), ptr(pl.Cc[l]), ptr(ws), ws.numel(), s), "cham_ugrnn_fwd_coop")

    def backward(self, pl, l, s):
        ws = self.ws(pl)
        check(self.host.lib.cham_ugrnn_bwd_coop(ptr(pl.drnn), ptr(self.host.p('rnn%d/Wh' % l)), ptr(pl.seq_len), pl.B, pl.T, self.Hp, ptr(pl.hprev[l]),
                                                ptr(pl.G[l]), ptr(pl.Cc[l]), ptr(pl.dxproj), ptr(ws), ws.numel(), s), "cham_ugrnn_bwd_coop")


class StepwiseUgrnn(RnnPath):
    """Large hidden size: one GEMM (h W_h) + one gate kernel per time step; backward one kernel + a copy + the accumulating GEMM."""
    # The time loops, the state's zero fill, the gate product and the backward's carry tail are the GRU's too: it overrides the point_* stages.
    launches_per_step = (2, 3)

    def alloc(self, pl, f32):      # the running state, its gate product, and the backward's state gradient with its two summands
        B, Hp = pl.B, self.Hp
        pl.h_state, pl.zh, pl.carry = f32(B, Hp), f32(B, self.WhN), f32(B, Hp)
        pl.dzs, pl.direct = f32(B, self.WhN), f32(B, Hp)

    def forward(self, pl, l, s):
        Hp, WhN, Wh = self.Hp, self.WhN, self.host.p('rnn%d/Wh' % l)
        self.zero_state(pl)
        for t in range(pl.T):
            self.host.gemm(pl.h_state, Wh, pl.zh, pl.B, WhN, Hp, Hp, WhN, WhN, force_f32=True)      # zh = h W_h (GRU: the r | u columns, W_gh)
            self.point_fwd(pl, l, t, s)

    def backward(self, pl, l, s):
        Hp, WhN, Wh = self.Hp, self.WhN, self.host.p('rnn%d/Wh' % l)
        self.zero_carry(pl)
        for t in range(pl.T - 1, -1, -1):
            self.point_bwd(pl, l, t, s)
            # carry = direct + dzs W_h^T, GRU: [dz_r | dz_u] W_gh^T  (rows beyond their length: dzs = 0, direct = carry -> unchanged)
            pl.carry.copy_(pl.direct)
            self.host.gemm(pl.dzs, Wh, pl.carry, pl.B, Hp, WhN, WhN, WhN, Hp, transB=1, accumulate=1, force_f32=True)

    def zero_state(self, pl):      # a layer's forward starts from the zero state, its backward from a zero state gradient
        pl.h_state.zero_()

    def zero_carry(self, pl):
        pl.carry.zero_()

    def point_fwd(self, pl, l, t, s):
        check(self.host.lib.cham_ugrnn_point_fwd(ptr(pl.xproj[l]), ptr(pl.zh), ptr(pl.seq_len), pl.B, pl.T, t, self.Hp, ptr(pl.h_state), ptr(pl.rnn_out[l]),
                                                 ptr(pl.hprev[l]), ptr(pl.G[l]), ptr(pl.Cc[l]), s), "cham_ugrnn_point_fwd")

    def point_bwd(self, pl, l, t, s):
        check(self.host.lib.cham_ugrnn_point_bwd(ptr(pl.drnn), ptr(pl.carry), ptr(pl.seq_len), pl.B, pl.T, t, self.Hp, ptr(pl.hprev[l]), ptr(pl.G[l]),
                                                 ptr(pl.Cc[l]), ptr(pl.dxproj), ptr(pl.dzs), ptr(pl.direct), s), "cham_ugrnn_point_bwd")


class StepwiseGru(StepwiseUgrnn):
    """GRU beyond Hp 384: gates, then the candidate over r * h - two GEMMs + two kernels per time step, and their mirror image backward."""
    launches_per_step = (4, 5)

    def alloc(self, pl, f32):      # + the candidate's recurrent product and its two gradients (zh / dzs hold the r | u columns of the gate GEMM)
        StepwiseUgrnn.alloc(self, pl, f32)
        pl.zc, pl.dzc, pl.drh = (f32(pl.B, self.Hp) for _ in range(3))

    def point_fwd(self, pl, l, t, s):
        lib, B, T, Hp = self.host.lib, pl.B, pl.T, self.Hp
        check(lib.cham_gru_point_gates_fwd(ptr(pl.xproj[l]), ptr(pl.zh), ptr(pl.seq_len), B, T, t, Hp, ptr(pl.h_state), ptr(pl.hprev[l]),
                                           ptr(pl.G[l]), ptr(pl.R[l]), ptr(pl.RH[l]), s), "cham_gru_point_gates_fwd")
        self.host.gemm(pl.RH[l].view(B, T * Hp)[:, t * Hp:], self.host.p('rnn%d/Wch' % l), pl.zc, B, Hp, Hp, T * Hp, Hp, Hp, force_f32=True)      # RH[:, t], strided
        check(lib.cham_gru_point_out_fwd(ptr(pl.xproj[l]), ptr(pl.zc), ptr(pl.seq_len), B, T, t, Hp, ptr(pl.G[l]), ptr(pl.hprev[l]),
                                         ptr(pl.h_state), ptr(pl.rnn_out[l]), ptr(pl.Cc[l]), s), "cham_gru_point_out_fwd")

    def point_bwd(self, pl, l, t, s):
        lib, B, T, Hp = self.host.lib, pl.B, pl.T, self.Hp
        check(lib.cham_gru_point_c_bwd(ptr(pl.drnn), ptr(pl.carry), ptr(pl.seq_len), B, T, t, Hp, ptr(pl.hprev[l]), ptr(pl.G[l]), ptr(pl.Cc[l]),
                                       ptr(pl.dxproj), ptr(pl.dzc), ptr(pl.dzs), ptr(pl.direct), s), "cham_gru_point_c_bwd")
        self.host.gemm(pl.dzc, self.host.p('rnn%d/Wch' % l), pl.drh, B, Hp, Hp, Hp, Hp, Hp, transB=1, force_f32=True)     # d(r h) = dzc W_ch^T
        check(lib.cham_gru_point_r_bwd(ptr(pl.drh), ptr(pl.seq_len), B, T, t, Hp, ptr(pl.hprev[l]), ptr(pl.R[l]), ptr(pl.dxproj), ptr(pl.dzs),
                                       ptr(pl.direct), s), "cham_gru_point_r_bwd")


class StepwiseLstm(StepwiseUgrnn):
    """LSTM, step-wise at every width: the UGRNN's time loops over four gate blocks i | j | f | o; c and its gradient never leave the kernels."""
    # the gates share the plan's planes with the other cells' (G = i, Cc = j, R = f, RH = o); hprev is, as everywhere, the Wh gradient's operand
    launches_per_step = (2, 3)

    def alloc(self, pl, f32):      # + the second state and its gradient, and per layer the two planes the plan has no name for: c_{t-1}, tanh(c_t)
        StepwiseUgrnn.alloc(self, pl, f32)
        pl.c_state, pl.carry_c = f32(pl.B, self.Hp), f32(pl.B, self.Hp)
        pl.cprev = [f32(pl.B * pl.T, self.Hp) for _ in pl.hprev]
        pl.TC = [f32(pl.B * pl.T, self.Hp) for _ in pl.hprev]

    def zero_state(self, pl):
        pl.h_state.zero_()
        pl.c_state.zero_()

    def zero_carry(self, pl):
        pl.carry.zero_()
        pl.carry_c.zero_()

    def point_fwd(self, pl, l, t, s):
        check(self.host.lib.cham_lstm_point_fwd(ptr(pl.xproj[l]), ptr(pl.zh), ptr(pl.seq_len), pl.B, pl.T, t, self.Hp, ptr(pl.h_state), ptr(pl.c_state),
                                                ptr(pl.rnn_out[l]), ptr(pl.hprev[l]), ptr(pl.cprev[l]), ptr(pl.G[l]), ptr(pl.Cc[l]), ptr(pl.R[l]),
                                                ptr(pl.RH[l]), ptr(pl.TC[l]), s), "cham_lstm_point_fwd")

    def point_bwd(self, pl, l, t, s):
        check(self.host.lib.cham_lstm_point_bwd(ptr(pl.drnn), ptr(pl.carry), ptr(pl.carry_c), ptr(pl.seq_len), pl.B, pl.T, t, self.Hp, ptr(pl.cprev[l]),
                                                ptr(pl.G[l]), ptr(pl.Cc[l]), ptr(pl.R[l]), ptr(pl.RH[l]), ptr(pl.TC[l]), ptr(pl.dxproj), ptr(pl.dzs),
                                                ptr(pl.direct), s), "cham_lstm_point_bwd")
