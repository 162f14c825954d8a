"""Float64 numpy reference of the LSTM session encoder with hand-derived back-propagation through time, written from the TF 1.12 cell
definition (tf.nn.rnn_cell.LSTMCell with its defaults - no peepholes, projection or clipping, forget_bias 1.0, state_is_tuple - under
dynamic_rnn's length masking), in the style of tests/rnn_reference.py and, like it, not from the oracle's or the kernels' code.

    z = [x, h] K + b,  column blocks i | j | f | o;   i = s(z_i)  j = tanh(z_j)  f = s(z_f + 1)  o = s(z_o)
    c' = f c + i j;   h' = o tanh(c');   beyond a row's length the output is zero and BOTH states are carried.

The kernels take the input projection x W_x + b as their input (`xproj`), so they are fed through `lstm_bptt` with the identity-padded
kernel of `lstm_kernel`: d loss / d x is then exactly the kernels' `dxproj`.  `padded_inputs` draws inputs in the padded layout of the model
as rnn_reference.padded_inputs does; `point_stages` restates in numpy float32 what cham_lstm_point_fwd / _bwd and the two recurrent GEMMs
of the step-wise path compute (tests/test_lstm_cpu.py pins it to the reference, tests/test_lstm_point_gpu.py the kernels)."""
import numpy as np

from tests.rnn_reference import PAD, REL_BOUND, rel_err          # noqa: F401  (the bound and its measure are the other cells')

SAVED = ('hprev', 'cprev', 'Gi', 'Gj', 'Gf', 'Go', 'TC')         # the planes the forward kernel saves, [B, T, Hp] each


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def lstm_bptt(x, lengths, K, b, R, saved=False, weight_grads=True):
    """loss = sum(out * R).  Returns out and d loss / d (x, K, b); dK and db are None with weight_grads=False.  saved=True appends a dict
    of what the kernels save per step: hprev (h_{t-1}), cprev (c_{t-1}), Gi, Gj, Gf, Go (the activated gates) and TC (tanh(c'))."""
    B, T, I = x.shape
    H_ = K.shape[1] // 4
    h, c = np.zeros((B, H_)), np.zeros((B, H_))
    st, outs = [], []
    for t in range(T):
        z = np.concatenate([x[:, t], h], 1) @ K + b
        gi, gj = _sig(z[:, :H_]), np.tanh(z[:, H_:2 * H_])
        gf, go = _sig(z[:, 2 * H_:3 * H_] + 1.0), _sig(z[:, 3 * H_:])
        cn = gf * c + gi * gj
        tc = np.tanh(cn)
        hn = go * tc
        v = (t < lengths)[:, None]
        st.append((h, c, gi, gj, gf, go, tc))
        outs.append(np.where(v, hn, 0.0))
        h, c = np.where(v, hn, h), np.where(v, cn, c)
    out = np.stack(outs, 1)
    dx = np.zeros_like(x)
    dK, db = (np.zeros_like(K), np.zeros_like(b)) if weight_grads else (None, None)
    dh, dc = np.zeros((B, H_)), np.zeros((B, H_))          # d loss / d (h_t, c_t) through the state path
    for t in range(T - 1, -1, -1):
        v = (t < lengths)[:, None]
        hp, cp, gi, gj, gf, go, tc = st[t]
        dhn = np.where(v, R[:, t] + dh, 0.0)               # output path + state path, both only where the step is valid
        dcn = np.where(v, dc + dhn * go * (1 - tc * tc), 0.0)
        dz = np.concatenate([dcn * gj * gi * (1 - gi), dcn * gi * (1 - gj * gj), dcn * cp * gf * (1 - gf), dhn * tc * go * (1 - go)], 1)
        if weight_grads:
            dK += np.concatenate([x[:, t], hp], 1).T @ dz
            db += dz.sum(0)
        dxin = dz @ K.T
        dx[:, t] = dxin[:, :I]
        dh = np.where(v, 0.0, dh) + dxin[:, I:]            # invalid step: both state gradients carried through unchanged (dz = 0 there)
        dc = np.where(v, dcn * gf, dc)
    if saved:
        return out, dx, dK, db, dict(zip(SAVED, (np.stack(a, 1) for a in zip(*st))))
    return out, dx, dK, db


# ---- the kernels' view: xproj in, dxproj out ------------------------------------------------------------------------------------

def lstm_kernel(Wh):
    """K = [I_4Hp ; W_h]: with x = xproj and b = 0, [x, h] K = xproj + h W_h and d loss / d x = dxproj."""
    Hp = Wh.shape[0]
    return np.concatenate([np.eye(4 * Hp), Wh], 0)


def kernel_reference(xproj, lengths, Wh, dout):
    """What the step-wise LSTM path computes, in float64: a dict of out, the SAVED planes and dxproj (float32 inputs of the kernels' layout)."""
    f = lambda a: np.asarray(a, np.float64)
    x = f(xproj)
    out, dx, _, _, s = lstm_bptt(x, lengths, lstm_kernel(f(Wh)), np.zeros(x.shape[2]), f(dout), saved=True, weight_grads=False)
    return dict(s, out=out, dxproj=dx)


def padded_inputs(Hp, B, T, seed, x_scale=0.7):
    """rnn_reference.padded_inputs for the LSTM: H = Hp - 17 real hidden units, zero pad rows and columns in every column block of W_h
    [Hp,4Hp] and xproj [B,T,4Hp], zero pad lanes in dout [B,T,Hp] (which is non-zero beyond a session's length: the kernels must ignore it);
    lengths [B] int32 in [0, T] that hold T, 0, 1, T, T - 1 in this order as far as B allows.  Float32 arrays."""
    rng = np.random.default_rng(seed)
    H = Hp - PAD
    Wh = rng.standard_normal((Hp, 4, Hp)) * Hp ** -0.5
    Wh[H:] = 0
    Wh[..., H:] = 0
    xproj = (x_scale * rng.standard_normal((B, T, 4, Hp))).astype(np.float32)
    xproj[..., H:] = 0
    dout = rng.standard_normal((B, T, Hp)).astype(np.float32)
    dout[..., H:] = 0
    lengths = rng.integers(0, T + 1, size=B).astype(np.int32)
    lengths[:5] = [T, 0, 1, T, T - 1][:B]
    return dict(xproj=xproj.reshape(B, T, 4 * Hp), Wh=Wh.reshape(Hp, 4 * Hp).astype(np.float32), dout=dout, lengths=lengths, H=H)


# ---- the step-wise path restated in float32 ---------------------------------------------------------------------------------------
f32 = np.float32


def _sig32(x):
    return (f32(1) / (f32(1) + np.exp(-x, dtype=f32))).astype(f32)


def _mm32(a, w):
    """A recurrent product with fp32 operands and an fp32 result (accumulated wider, as a GEMM's error is far below the bound's)."""
    return (a.astype(np.float64) @ w.astype(np.float64)).astype(f32)


def point_stages(inp, drop_carry_c=False):
    """out, the SAVED planes and dxproj of the step-wise path, float32: per step zh = h W_h + the forward point stage; the backward point
    stage + carry_h = direct + dzs W_h^T.  drop_carry_c: the mutant whose backward forgets the cell state's gradient (carry_c stays 0)."""
    xproj, Wh, dout, lens = inp['xproj'], inp['Wh'], inp['dout'], inp['lengths']
    B, T, Hp = dout.shape
    x = xproj.reshape(B, T, 4, Hp)
    o = {k: np.full((B, T, Hp), np.nan, f32) for k in ('out',) + SAVED}
    dx = np.full((B, T, 4, Hp), np.nan, f32)
    h, c = np.zeros((B, Hp), f32), np.zeros((B, Hp), f32)
    one = f32(1)
    for t in range(T):
        valid = (t < lens)[:, None]
        z = _mm32(h, Wh).reshape(B, 4, Hp) + x[:, t]                                  # the gate GEMM, then point_fwd
        gi, gj, gf, go = _sig32(z[:, 0]), np.tanh(z[:, 1], dtype=f32), _sig32(z[:, 2] + one), _sig32(z[:, 3])
        cn = gf * c + gi * gj
        tc = np.tanh(cn, dtype=f32)
        hn = go * tc
        for k, a in zip(('out',) + SAVED, (np.where(valid, hn, f32(0)), h, c, gi, gj, gf, go, tc)):
            o[k][:, t] = a
        h, c = np.where(valid, hn, h), np.where(valid, cn, c)
    carry_h, carry_c = np.zeros((B, Hp), f32), np.zeros((B, Hp), f32)
    for t in range(T - 1, -1, -1):
        valid = (t < lens)[:, None]
        cp, gi, gj, gf, go, tc = (o[k][:, t] for k in SAVED[1:])
        dh = dout[:, t] + carry_h                                                     # point_bwd
        dc = carry_c + dh * go * (one - tc * tc)
        dz = np.stack([dc * gj * gi * (one - gi), dc * gi * (one - gj * gj), dc * cp * gf * (one - gf), dh * tc * go * (one - go)], 1)
        dz = np.where(valid[:, :, None], dz, f32(0)).astype(f32)
        if not drop_carry_c:
            carry_c = np.where(valid, dc * gf, carry_c)
        direct = np.where(valid, f32(0), carry_h)
        dx[:, t] = dz
        carry_h = (direct.astype(np.float64) + dz.reshape(B, 4 * Hp).astype(np.float64) @ Wh.T.astype(np.float64)).astype(f32)   # copy + GEMM
    o['dxproj'] = dx.reshape(B, T, 4 * Hp)
    assert all(a.dtype == f32 for a in o.values())
    return o
