"""Float64 numpy references of the recurrent cells with hand-derived back-propagation through time, written from the TF 1.12 cell
definitions (nar_model.py:1308-1361 of the reference: the cell under dynamic_rnn's length masking), not from the oracle's or the kernels'
code.  tests/test_oracle_second_opinion.py pins the oracle to them; tests/test_rnn_kernels_gpu.py pins csrc/rnn.hip to them.

The kernels take the input projection x W_x + b as their input (`xproj`), so they are fed through these functions with an identity-padded
kernel (`ugrnn_kernel` / `gru_kernels`): d loss / d x is then exactly the kernels' `dxproj`.  `padded_inputs` draws inputs in the padded
layout of the model ("rnn_units to a multiple of 128"), shared by the GPU tests and the CPU test that calibrates their bound."""
import numpy as np

# max |got - ref| <= REL_BOUND * max |ref|, per array (the bound tests/test_rnn_coop_gpu.py holds between two fp32 paths)
REL_BOUND = 2e-5
PAD = 17                 # H = Hp - PAD: every width has pad lanes


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def ugrnn_bptt(x, lengths, K, b, R, saved=False, weight_grads=True):
    """tf.contrib.rnn.UGRNNCell (TF 1.12 rnn_cell.py): [g_act, c_act] = [x, h] K + b; c = tanh(c_act); g = sigmoid(g_act + 1);
    h' = g h + (1 - g) c.  dynamic_rnn: beyond a row's length the output is zero and the state is carried.  loss = sum(out * R).
    Returns out and d loss / d (x, K, b); dK and db are None with weight_grads=False.  saved=True appends a dict of the activations
    the kernels save per step: hprev (h_{t-1}), g, c, each [B, T, H]."""
    B, T, I = x.shape
    H_ = K.shape[1] // 2
    h = np.zeros((B, H_)); hs, gs, cs, outs = [], [], [], []
    for t in range(T):
        z = np.concatenate([x[:, t], h], 1) @ K + b
        c, g = np.tanh(z[:, H_:]), _sig(z[:, :H_] + 1.0)
        hn = g * h + (1 - g) * c
        v = (t < lengths)[:, None]
        hs.append(h); gs.append(g); cs.append(c)
        outs.append(np.where(v, hn, 0.0)); h = np.where(v, hn, h)
    out = np.stack(outs, 1)
    dx, dh = np.zeros_like(x), np.zeros((B, H_))
    dK, db = (np.zeros_like(K), np.zeros_like(b)) if weight_grads else (None, None)
    for t in range(T - 1, -1, -1):
        v = (t < lengths)[:, None]
        dhn = np.where(v, R[:, t] + dh, 0.0)             # output path + state path (both only where the step is valid)
        carry = np.where(v, 0.0, dh)                      # invalid step: state carried through unchanged
        g, c, hp = gs[t], cs[t], hs[t]
        dg, dc = dhn * (hp - c), dhn * (1 - g)
        dz = np.concatenate([dg * g * (1 - g), dc * (1 - c * c)], 1)
        if weight_grads:
            xin = np.concatenate([x[:, t], hp], 1)
            dK += xin.T @ dz; db += dz.sum(0)
        dxin = dz @ K.T
        dx[:, t] = dxin[:, :I]
        dh = carry + dhn * g + dxin[:, I:]
    if saved:
        return out, dx, dK, db, dict(hprev=np.stack(hs, 1), g=np.stack(gs, 1), c=np.stack(cs, 1))
    return out, dx, dK, db


def gru_bptt(x, lengths, Kg, bg, Kc, bc, R, saved=False, weight_grads=True):
    """tf.nn.rnn_cell.GRUCell (TF 1.12): [r, u] = sigmoid([x, h] Kg + bg); c = tanh([x, r h] Kc + bc); h' = u h + (1 - u) c.
    The weight gradients are None with weight_grads=False.  saved=True appends a dict of hprev (h_{t-1}), u, c, r and rh (r h_{t-1})."""
    B, T, I = x.shape
    H_ = Kc.shape[1]
    h = np.zeros((B, H_)); st, outs = [], []
    for t in range(T):
        ru = _sig(np.concatenate([x[:, t], h], 1) @ Kg + bg)
        r, u = ru[:, :H_], ru[:, H_:]
        c = np.tanh(np.concatenate([x[:, t], r * h], 1) @ Kc + bc)
        hn = u * h + (1 - u) * c
        v = (t < lengths)[:, None]
        st.append((h, r, u, c))
        outs.append(np.where(v, hn, 0.0)); h = np.where(v, hn, h)
    out = np.stack(outs, 1)
    dx = np.zeros_like(x)
    wg = (np.zeros_like(Kg), np.zeros_like(bg), np.zeros_like(Kc), np.zeros_like(bc)) if weight_grads else None
    dh = np.zeros((B, H_))
    for t in range(T - 1, -1, -1):
        v = (t < lengths)[:, None]
        hp, r, u, c = st[t]
        dhn = np.where(v, R[:, t] + dh, 0.0)
        carry = np.where(v, 0.0, dh)
        du, dc = dhn * (hp - c), dhn * (1 - u)
        dzc = dc * (1 - c * c)
        dxc = dzc @ Kc.T
        drh = dxc[:, I:]
        dr = drh * hp
        dzg = np.concatenate([dr * r * (1 - r), du * u * (1 - u)], 1)
        if weight_grads:
            xc = np.concatenate([x[:, t], r * hp], 1)
            xg = np.concatenate([x[:, t], hp], 1)
            wg[2][...] += xc.T @ dzc; wg[3][...] += dzc.sum(0)
            wg[0][...] += xg.T @ dzg; wg[1][...] += dzg.sum(0)
        dxg = dzg @ Kg.T
        dx[:, t] = dxc[:, :I] + dxg[:, :I]
        dh = carry + dhn * u + drh * r + dxg[:, I:]
    if saved:
        hp, r, u, c = (np.stack(a, 1) for a in zip(*st))
        return out, dx, wg, dict(hprev=hp, u=u, c=c, r=r, rh=r * hp)
    return out, dx, wg


# ---- the kernels' view: xproj in, dxproj out ------------------------------------------------------------------------------------

def ugrnn_kernel(Wh):
    """K = [I_2Hp ; W_h]: with x = xproj and b = 0, [x, h] K = xproj + h W_h and d loss / d x = dxproj."""
    Hp = Wh.shape[0]
    return np.concatenate([np.eye(2 * Hp), Wh], 0)


def gru_kernels(Wgh, Wch):
    """Kg = [[I_2Hp ; 0] ; W_gh], Kc = [[0 ; I_Hp] ; W_ch] over x = xproj = [r | u | c] blocks (b = 0): d loss / d x = dxproj."""
    Hp = Wch.shape[0]
    Kg = np.concatenate([np.eye(2 * Hp), np.zeros((Hp, 2 * Hp)), Wgh], 0)
    Kc = np.concatenate([np.zeros((2 * Hp, Hp)), np.eye(Hp), Wch], 0)
    return Kg, Kc


def kernel_reference(cell, xproj, lengths, Wh, Wch, dout):
    """What cham_rnn_fwd / cham_rnn_bwd compute, in float64: a dict of out, hprev, G (g or u), Cc and dxproj, and for GRU R and RH.
    Inputs are float32 arrays of the kernels' layout (Wh = W_gh for GRU, Wch = W_ch or None)."""
    f = lambda a: np.asarray(a, np.float64)
    x, R = f(xproj), f(dout)
    if cell == 'ugrnn':
        out, dx, _, _, s = ugrnn_bptt(x, lengths, ugrnn_kernel(f(Wh)), np.zeros(x.shape[2]), R, saved=True, weight_grads=False)
        return dict(out=out, hprev=s['hprev'], G=s['g'], Cc=s['c'], dxproj=dx)
    Hp = Wch.shape[0]
    Kg, Kc = gru_kernels(f(Wh), f(Wch))
    out, dx, _, s = gru_bptt(x, lengths, Kg, np.zeros(2 * Hp), Kc, np.zeros(Hp), R, saved=True, weight_grads=False)
    return dict(out=out, hprev=s['hprev'], G=s['u'], Cc=s['c'], R=s['r'], RH=s['rh'], dxproj=dx)


def rel_err(got, ref):
    """max |got - ref| / max |ref| (the quantity REL_BOUND bounds)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(got - ref).max()) / max(1e-30, float(np.abs(ref).max()))


def padded_inputs(cell, Hp, B, T, seed, x_scale=0.7):
    """Inputs in the model's padded layout: H = Hp - 17 real hidden units, zero pad rows and columns in W_h / W_ch, zero pad columns
    in every column block of xproj, zero pad lanes in dout; weights ~ N(0, 1/Hp), xproj ~ x_scale N(0, 1), dout ~ N(0, 1) (also at the
    steps beyond a session's length, which the kernels must ignore); ragged lengths in [0, T] that hold 0, 1 and T where B allows,
    session 0 with length T.  Float32 arrays xproj [B,T,NG Hp], Wh [Hp,2Hp], Wch [Hp,Hp] or None, dout [B,T,Hp]; lengths [B] int32."""
    rng = np.random.default_rng(seed)
    H = Hp - PAD
    NG = 2 if cell == 'ugrnn' else 3

    def w(cols):
        m = rng.standard_normal((Hp, cols * Hp)) * Hp ** -0.5
        m[H:] = 0
        for k in range(cols):
            m[:, k * Hp + H:(k + 1) * Hp] = 0
        return m.astype(np.float32)

    Wh = w(2)
    Wch = w(1) if cell == 'gru' else None
    xproj = (x_scale * rng.standard_normal((B, T, NG, Hp))).astype(np.float32)
    xproj[..., H:] = 0
    dout = rng.standard_normal((B, T, Hp)).astype(np.float32)
    dout[..., H:] = 0
    lengths = rng.integers(0, T + 1, size=B).astype(np.int32)
    lengths[:5] = [T, 0, 1, T, T - 1][:B]
    return dict(xproj=xproj.reshape(B, T, NG * Hp), Wh=Wh, Wch=Wch, dout=dout, lengths=lengths, H=H)
