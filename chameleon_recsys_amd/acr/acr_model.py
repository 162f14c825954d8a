"""The ACR model (acr_module/acr/acr_model.py:83-289) on the HIP kernels of csrc/acr.hip and the project's GEMM / optimizer kernels.

    x[b,t,:]     = table[text[b,t], :]                      constant table (not trained); id 0 = <PAD> is an ordinary, unmasked row
    conv_k[b,t,f] = relu(bias_k[f] + sum_{j<k} sum_e x[b,t+j,e] W_k[j,e,f]),  t = 0..L-k      one per size in cnn_filter_sizes
    pool         = concat_k max_t conv_k                    [B, n_sizes F]
    fc2          = relu(pool W_a + b_a);  ace = tanh(fc2 W_h + b_h)   -> the exported Article Content Embedding
    logits_l     = ace W_l + b_l                            one head per label feature, multiclass or multilabel
    loss         = sum_l CE_l + l2_reg_lambda sum_kernels sum(w^2) / 2

A multiclass head's CE is the sparse softmax cross-entropy with optional per-class weights.  A multilabel head's (ACR_ModelMultilabel
only, see below) is the sigmoid cross-entropy against a multi-hot target built from the batch's zero-padded id lists [B, Kmax]:
    z[b,c] = #{k : ids[b,k] == c} for c >= 1 (a duplicated id counts twice), z[b,0] = 0 (the padding id)
    CE     = mean_b mean_c (max(x,0) - x z + log1p(exp(-|x|)));   prediction = x > 0 (uint8 multi-hot);   no class weights
(acr_model.py:202-215, :6-8).  The multi-hot matrix is built inside the kernel and never reaches memory (csrc/acr.hip).

Built: text_feature_extractor = CNN, training_task = metadata_classification, multiclass heads with optional per-class weights,
multilabel heads.  Refused (NotImplementedError / ValueError naming the flag): the cuDNN LSTM / GRU extractors, the autoencoder task,
dropout_keep_prob < 1.

Multilabel heads are OPT-IN: ACR_Model and check_supported refuse them as they did before the head was built, ACR_ModelMultilabel (what
acr_trainer_adressa constructs) and check_supported(..., multilabel=True) accept them.  The G1 trainer's contract - a multilabel head in
its label features is an error that names the head - is part of its tested interface, and a model without such a head launches exactly
the kernels it launched before.

All parameters live in ONE flat fp32 buffer, the L2-regularised kernels first (``n_reg``), then the biases.  Widths that cham_gemm_f32
needs as multiples of 4 (n_sizes F, acr_embeddings_size, every cardinality) are padded with zero rows / columns; zero-initialised
padding has a zero gradient and stays exactly zero under Adam with L2 (tests/test_acr_gpu.py).

Initialisation: Xavier-uniform (+-sqrt(6 / (fan_in + fan_out)); conv kernel fan_in = k E, fan_out = k F), zero biases, drawn from a
numpy RandomState(42) (the reference's RANDOM_SEED) in layout order.  TensorFlow's own random stream is not reproduced.

The gradient of the max goes to the FIRST position that attains it (TF splits it evenly among ties; the rules agree whenever the tied
windows are identical, which is the case that occurs: DESIGN.md)."""
import ctypes
import math
from collections import OrderedDict

import numpy as np

RANDOM_SEED = 42
ADAM_BETA1, ADAM_BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def roundup4(n):
    return (int(n) + 3) // 4 * 4


def check_flags(training_task, text_feature_extractor, dropout_keep_prob=1.0):
    """Raises for the flag values whose arm of the reference is not built."""
    ext, task = str(text_feature_extractor).upper(), str(training_task).lower()
    if ext in ('LSTM', 'GRU'):
        raise NotImplementedError("--text_feature_extractor %s: the cuDNN recurrent extractors are not built; only CNN" % ext)
    if ext != 'CNN':
        raise ValueError("--text_feature_extractor %r invalid: (CNN | LSTM | GRU)" % text_feature_extractor)
    if task == 'autoencoder':
        raise NotImplementedError("--training_task autoencoder is not built; only metadata_classification")
    if task != 'metadata_classification':
        raise ValueError("--training_task %r invalid: (metadata_classification | autoencoder)" % training_task)
    if float(dropout_keep_prob) < 1.0:
        raise NotImplementedError("--dropout_keep_prob < 1 is not built (the shipped launch scripts use 1.0)")


def check_supported(training_task, text_feature_extractor, labels_features_config, params, multilabel=False):
    """check_flags plus the label heads: multiclass heads with a cardinality, and multilabel heads when ``multilabel`` is set.
    The opt-in keeps the G1 path's refusal (see the module docstring); ACR_ModelMultilabel passes True."""
    check_flags(training_task, text_feature_extractor, params.get('dropout_keep_prob', 1.0))
    if not labels_features_config:
        raise ValueError("label_features is empty: metadata_classification needs at least one label head")
    for name, cfg in labels_features_config.items():
        ct = cfg.get('classification_type')
        if ct == 'multilabel' and not multilabel:
            raise NotImplementedError("label feature %r: classification_type multilabel is not accepted here, only multiclass "
                                      "(multilabel heads are opt-in: ACR_ModelMultilabel, acr_trainer_adressa)" % name)
        if ct not in ('multiclass', 'multilabel'):
            raise ValueError("label feature %r: classification_type %r invalid" % (name, ct))
        if int(cfg.get('cardinality', 0)) < 1:
            raise ValueError("label feature %r needs a cardinality" % name)


class ACRLayout:
    """Flat parameter layout: entries name -> (offset, logical shape, padded shape), regularised kernels first."""

    def __init__(self, E, filter_sizes, F, acr_embeddings_size, heads):
        self.E, self.sizes, self.F, self.A = int(E), [int(k) for k in filter_sizes], int(F), int(acr_embeddings_size)
        self.heads = OrderedDict((n, int(c)) for n, c in heads.items())
        self.PW = len(self.sizes) * self.F
        self.ldP, self.ldA = roundup4(self.PW), roundup4(self.A)
        self.ldC = OrderedDict((n, roundup4(c)) for n, c in self.heads.items())
        self.entries = OrderedDict()
        off = 0

        def add(name, shape, padded):
            nonlocal off
            self.entries[name] = (off, tuple(shape), tuple(padded))
            off += roundup4(int(np.prod(padded)))

        for s, k in enumerate(self.sizes):
            add('conv_%d/kernel' % s, (k, self.E, self.F), (k, self.E, self.F))
        add('fc2/kernel', (self.PW, self.A), (self.ldP, self.ldA))
        add('ace/kernel', (self.A, self.A), (self.ldA, self.ldA))
        for n, c in self.heads.items():
            add('output_%s/kernel' % n, (self.A, c), (self.ldA, self.ldC[n]))
        self.n_reg = off                                   # exactly the kernels: biases are not regularised (acr_model.py:141-168, :282)
        for s in range(len(self.sizes)):
            add('conv_%d/bias' % s, (self.F,), (self.F,))
        add('fc2/bias', (self.A,), (self.ldA,))
        add('ace/bias', (self.A,), (self.ldA,))
        for n, c in self.heads.items():
            add('output_%s/bias' % n, (c,), (self.ldC[n],))
        self.n_params = off

    def offset(self, name):
        return self.entries[name][0]

    def fan(self, name):
        shape = self.entries[name][1]
        if name.startswith('conv_'):
            k, e, f = shape
            return k * e, k * f
        return shape

    def xavier_limit(self, name):
        fi, fo = self.fan(name)
        return math.sqrt(6.0 / (fi + fo))

    def init(self, seed=RANDOM_SEED):
        """Flat fp32 numpy buffer: Xavier-uniform kernels in layout order, zero biases, zero padding."""
        rng = np.random.RandomState(seed)
        flat = np.zeros(self.n_params, np.float32)
        for name in self.entries:
            if name.endswith('/kernel'):
                lim = self.xavier_limit(name)
                self.scatter(flat, name, rng.uniform(-lim, lim, size=self.entries[name][1]).astype(np.float32))
        return flat

    def view(self, flat, name):
        off, _, padded = self.entries[name]
        return flat[off:off + int(np.prod(padded))].reshape(padded)

    def gather(self, flat, name):
        _, shape, _ = self.entries[name]
        return self.view(flat, name)[tuple(slice(0, d) for d in shape)].copy()

    def scatter(self, flat, name, value):
        _, shape, _ = self.entries[name]
        self.view(flat, name)[tuple(slice(0, d) for d in shape)] = np.asarray(value, np.float32).reshape(shape)

    def padding_mask(self):
        """True where the flat buffer holds padding (rows / columns beyond the logical shape, allocation tails)."""
        m = np.ones(self.n_params, bool)
        for name, (_, shape, _) in self.entries.items():
            self.view(m, name)[tuple(slice(0, d) for d in shape)] = False
        return m


def validate_batch(text, labels, vocab_size, heads, multilabel_heads=()):
    """Host-side range checks BEFORE any upload: an out-of-range id becomes a ValueError, never a GPU fault.  The labels of a head named
    in ``multilabel_heads`` are a zero-padded id list [B, Kmax] (Kmax = 0 is legal), those of any other head one id per row."""
    text = np.asarray(text)
    if text.ndim != 2 or text.shape[0] < 1:
        raise ValueError("text must be [B, L], got shape %r" % (text.shape,))
    if text.size and (text.min() < 0 or text.max() >= vocab_size):
        raise ValueError("text holds a token id outside [0, %d): min %d, max %d" % (vocab_size, text.min(), text.max()))
    if labels is not None:
        for n, c in heads.items():
            y = np.asarray(labels[n])
            if n in multilabel_heads:
                if y.ndim != 2:
                    raise ValueError("label %r (multilabel) must be [B, Kmax], got shape %r" % (n, y.shape))
            else:
                y = y.reshape(-1)
            if y.shape[0] != text.shape[0]:
                raise ValueError("label %r has %d rows, text has %d" % (n, y.shape[0], text.shape[0]))
            if y.size and (y.min() < 0 or y.max() >= c):
                raise ValueError("label %r holds an id outside [0, %d): min %d, max %d" % (n, c, y.min(), y.max()))


class ACR_Model:
    """train_step / eval_step / predict over numpy batches (features['text'] [B, L], labels {head: [B]}; a multilabel head's labels
    are the zero-padded id lists [B, Kmax], accepted by ACR_ModelMultilabel only)."""

    MULTILABEL_HEADS = False          # the opt-in (module docstring): ACR_ModelMultilabel sets it

    def __init__(self, training_task, text_feature_extractor, labels_features_config, params, device=None, seed=RANDOM_SEED):
        check_supported(training_task, text_feature_extractor, labels_features_config, params, multilabel=self.MULTILABEL_HEADS)
        import torch
        from .. import _lib
        self.torch, self._lib_mod = torch, _lib
        self.lib = _lib.load()                                            # raises when the HIP library is missing: no fallback
        self.device = torch.device(device or 'cuda:0')
        self.params_dict = params
        self.l2_reg_lambda = float(params['l2_reg_lambda'])
        self.learning_rate = float(params['learning_rate'])
        table = np.ascontiguousarray(params['word_embeddings_matrix'], dtype=np.float32)
        self.V, E = table.shape
        self.ldE = roundup4(E)
        sizes = [int(k) for k in str(params['cnn_filter_sizes']).split(',')]
        # feature_weight_on_loss: the reference reads it from the dict of ALL label features instead of the feature's own entry
        # (acr_model.py:219), so it is always 1.0; kept - every head's loss enters with weight 1.
        heads = OrderedDict((n, cfg['cardinality']) for n, cfg in labels_features_config.items())
        self.multilabel = tuple(n for n, cfg in labels_features_config.items() if cfg['classification_type'] == 'multilabel')
        self.layout = L = ACRLayout(E, sizes, params['cnn_num_filters'], params['acr_embeddings_size'], heads)
        t = torch.zeros((self.V, self.ldE), dtype=torch.float32)
        t[:, :E] = torch.from_numpy(table)
        self.table = t.to(self.device)
        self.params = torch.from_numpy(L.init(seed)).to(self.device)
        self.grads = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        self.global_step = 0
        self.class_weights = {}
        for n, w in (params.get('labels_class_weights') or {}).items():
            if n in heads and n not in self.multilabel:                   # (the multilabel loss takes no class weights, :214)
                w = np.asarray(w, np.float32).reshape(-1)
                if w.shape[0] != heads[n]:
                    raise ValueError("labels_class_weights[%r] has %d entries, cardinality is %d" % (n, w.shape[0], heads[n]))
                self.class_weights[n] = torch.from_numpy(w).to(self.device)
        self.c_sizes = (ctypes.c_int * len(sizes))(*sizes)
        self.sumsq = torch.zeros(1024, dtype=torch.float32, device=self.device)
        self.loss_terms = torch.zeros(len(heads), dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(3, dtype=torch.float32, device=self.device)         # [total, sum of the heads' CE, L2 term]
        self._bufs, self._ws = {}, None
        self._ptr_arrays()

    # ---- plumbing
    def _ptr_arrays(self):
        L, n = self.layout, len(self.layout.sizes)
        arr = ctypes.c_void_p * n

        def ptrs(t, suffix):
            return arr(*[t.data_ptr() + 4 * L.offset('conv_%d/%s' % (s, suffix)) for s in range(n)])
        self.pW, self.pb = ptrs(self.params, 'kernel'), ptrs(self.params, 'bias')
        self.pdW, self.pdb = ptrs(self.grads, 'kernel'), ptrs(self.grads, 'bias')

    def _p(self, t, name):
        return t.data_ptr() + 4 * self.layout.offset(name)

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def _check(self, rc, what):
        self._lib_mod.check(rc, what)

    def _buffers(self, B):
        if B not in self._bufs:
            L, z = self.layout, lambda *s, dt=self.torch.float32: self.torch.zeros(s, dtype=dt, device=self.device)
            d = dict(pool=z(B, L.ldP), dpool=z(B, L.ldP), argmax=z(B, L.PW, dt=self.torch.int32), fc2=z(B, L.ldA), dfc2=z(B, L.ldA),
                     ace=z(B, L.ldA), dace=z(B, L.ldA), row_ws=z(B),
                     colsum_ws=z(max(1, self.lib.cham_colsum_workspace_bytes(B, max([L.ldA] + list(L.ldC.values()))) // 4)))
            for n in L.heads:
                d['logits_' + n] = z(B, L.ldC[n]); d['dlogits_' + n] = z(B, L.ldC[n])
                if n not in self.multilabel:
                    d['pred_' + n] = z(B, dt=self.torch.int32)
            for n in self.multilabel:                                   # uint8 multi-hot predictions, (tp, fp, fn), the partials
                d['pred_' + n] = z(B, L.ldC[n], dt=self.torch.uint8); d['counts_' + n] = z(3, dt=self.torch.int32)
                d['ml_ws_' + n] = z(max(1, self.lib.cham_acr_sigmoid_xent_workspace_bytes(B, L.heads[n]) // 4))
            self._bufs[B] = d
        return self._bufs[B]

    def _gemm(self, A, lda, tA, Bm, ldb, tB, C, ldc, M, N, K, bias=None, act=0, accumulate=0):
        self._check(self.lib.cham_gemm_f32(A, lda, tA, Bm, ldb, tB, C, ldc, M, N, K, bias, act, None, 0, 0, None, 0, 1, accumulate, None, 0, 1,
                                           self._stream()), "cham_gemm_f32")

    def _upload(self, features, labels):
        text = np.asarray(features['text'])
        validate_batch(text, labels, self.V, self.layout.heads, self.multilabel)
        kmax = max(self.layout.sizes)
        if text.shape[1] < kmax:
            raise ValueError("the batch's padded length %d is below the largest cnn_filter_sizes entry %d (the reference yields an "
                             "empty max there)" % (text.shape[1], kmax))
        tok = self.torch.from_numpy(np.ascontiguousarray(text, dtype=np.int32)).to(self.device)
        lab = None
        if labels is not None:
            lab = {n: self.torch.from_numpy(np.ascontiguousarray(np.asarray(labels[n]).reshape(-1), dtype=np.int32)).to(self.device)
                   for n in self.layout.heads if n not in self.multilabel}
            for n in self.multilabel:                                     # [B, Kmax] int32; Kmax = 0 -> no list at all (a NULL pointer)
                ids = np.ascontiguousarray(labels[n], dtype=np.int32)
                lab[n] = self.torch.from_numpy(ids).to(self.device) if ids.shape[1] else None
        return tok, lab

    # ---- forward / backward
    def _forward(self, tok):
        L, lib, st, ptr = self.layout, self.lib, self._stream(), self._lib_mod.ptr
        B, T = tok.shape
        buf = self._buffers(B)
        need = lib.cham_acr_conv_pool_workspace_bytes(B, T, self.c_sizes, len(L.sizes), L.F)
        if self._ws is None or self._ws.numel() * 4 < need:
            self._ws = self.torch.empty((need + 3) // 4, dtype=self.torch.float32, device=self.device)
        self._check(lib.cham_acr_conv_pool_fwd(ptr(tok), B, T, ptr(self.table), self.V, L.E, self.ldE, self.c_sizes, len(L.sizes), L.F,
                                               self.pW, self.pb, ptr(buf['pool']), L.ldP, ptr(buf['argmax']), ptr(self._ws),
                                               self._ws.numel() * 4, st), "cham_acr_conv_pool_fwd")
        P = self.params
        self._gemm(ptr(buf['pool']), L.ldP, 0, self._p(P, 'fc2/kernel'), L.ldA, 0, ptr(buf['fc2']), L.ldA, B, L.ldA, L.ldP,
                   bias=self._p(P, 'fc2/bias'))
        self._check(lib.cham_acr_relu(ptr(buf['fc2']), B * L.ldA, st), "cham_acr_relu")
        self._gemm(ptr(buf['fc2']), L.ldA, 0, self._p(P, 'ace/kernel'), L.ldA, 0, ptr(buf['ace']), L.ldA, B, L.ldA, L.ldA,
                   bias=self._p(P, 'ace/bias'), act=2)
        for n in L.heads:
            self._gemm(ptr(buf['ace']), L.ldA, 0, self._p(P, 'output_%s/kernel' % n), L.ldC[n], 0, ptr(buf['logits_' + n]), L.ldC[n], B,
                       L.ldC[n], L.ldA, bias=self._p(P, 'output_%s/bias' % n))
        return buf

    def _losses(self, buf, lab, B, with_grad):
        L, lib, st, ptr = self.layout, self.lib, self._stream(), self._lib_mod.ptr
        for i, n in enumerate(L.heads):
            if n in self.multilabel:
                self._sigmoid_xent(buf, n, B, lab[n], self.loss_terms.data_ptr() + 4 * i, with_grad)
                continue
            self._check(lib.cham_acr_softmax_xent(ptr(buf['logits_' + n]), L.ldC[n], B, L.heads[n], None if lab is None else ptr(lab[n]),
                                                  ptr(self.class_weights.get(n)), self.loss_terms.data_ptr() + 4 * i,
                                                  ptr(buf['dlogits_' + n]) if with_grad else None, ptr(buf['pred_' + n]), ptr(buf['row_ws']),
                                                  st), "cham_acr_softmax_xent")
        self._check(lib.cham_sumsq_partial(ptr(self.params), L.n_reg, ptr(self.sumsq), st), "cham_sumsq_partial")
        self._check(lib.cham_loss_finalize(ptr(self.loss_terms), len(L.heads), 1.0, ptr(self.sumsq), self.l2_reg_lambda, ptr(self.loss), st),
                    "cham_loss_finalize")

    def _sigmoid_xent(self, buf, n, B, ids, loss_slot, with_grad):
        """The multilabel head ``n``: ids = the device id lists [B, Kmax] or None (no list: every target is 0)."""
        L, ptr = self.layout, self._lib_mod.ptr
        K = 0 if ids is None else ids.shape[1]
        ws = buf['ml_ws_' + n]
        self._check(self.lib.cham_acr_sigmoid_xent(ptr(buf['logits_' + n]), L.ldC[n], B, L.heads[n], ptr(ids), K, K, loss_slot,
                                                   ptr(buf['dlogits_' + n]) if with_grad else None, ptr(buf['pred_' + n]), L.ldC[n],
                                                   ptr(buf['counts_' + n]), ptr(ws), ws.numel() * 4, self._stream()),
                    "cham_acr_sigmoid_xent")

    def _backward(self, tok, buf):
        L, lib, st, ptr = self.layout, self.lib, self._stream(), self._lib_mod.ptr
        B, T = tok.shape
        P, G = self.params, self.grads
        ws, wsb = ptr(buf['colsum_ws']), buf['colsum_ws'].numel() * 4

        def colsum(X, ld, F, name):
            self._check(lib.cham_colsum(X, ld, B, F, None, self._p(G, name), 0, ws, wsb, st), "cham_colsum")

        for i, n in enumerate(L.heads):
            dl, ldc = ptr(buf['dlogits_' + n]), L.ldC[n]
            self._gemm(ptr(buf['ace']), L.ldA, 1, dl, ldc, 0, self._p(G, 'output_%s/kernel' % n), ldc, L.ldA, ldc, B)       # TN wgrad
            colsum(dl, ldc, ldc, 'output_%s/bias' % n)
            self._gemm(dl, ldc, 0, self._p(P, 'output_%s/kernel' % n), ldc, 1, ptr(buf['dace']), L.ldA, B, L.ldA, ldc,     # NT dgrad
                       accumulate=1 if i else 0)
        self._check(lib.cham_acr_act_bwd(ptr(buf['dace']), ptr(buf['ace']), B * L.ldA, 1, st), "cham_acr_act_bwd")
        self._gemm(ptr(buf['fc2']), L.ldA, 1, ptr(buf['dace']), L.ldA, 0, self._p(G, 'ace/kernel'), L.ldA, L.ldA, L.ldA, B)
        colsum(ptr(buf['dace']), L.ldA, L.ldA, 'ace/bias')
        self._gemm(ptr(buf['dace']), L.ldA, 0, self._p(P, 'ace/kernel'), L.ldA, 1, ptr(buf['dfc2']), L.ldA, B, L.ldA, L.ldA)
        self._check(lib.cham_acr_act_bwd(ptr(buf['dfc2']), ptr(buf['fc2']), B * L.ldA, 0, st), "cham_acr_act_bwd")
        self._gemm(ptr(buf['pool']), L.ldP, 1, ptr(buf['dfc2']), L.ldA, 0, self._p(G, 'fc2/kernel'), L.ldA, L.ldP, L.ldA, B)
        colsum(ptr(buf['dfc2']), L.ldA, L.ldA, 'fc2/bias')
        self._gemm(ptr(buf['dfc2']), L.ldA, 0, self._p(P, 'fc2/kernel'), L.ldA, 1, ptr(buf['dpool']), L.ldP, B, L.ldP, L.ldA)
        self._check(lib.cham_acr_conv_pool_bwd(ptr(tok), B, T, ptr(self.table), self.V, L.E, self.ldE, self.c_sizes, len(L.sizes), L.F,
                                               ptr(buf['dpool']), ptr(buf['pool']), L.ldP, ptr(buf['argmax']), self.pdW, self.pdb, st),
                    "cham_acr_conv_pool_bwd")

    # ---- the three modes
    def train_step(self, features, labels):
        """One optimizer step (tf.train.AdamOptimizer defaults, no clipping).  Returns the device tensor [total, CE, L2] of the loss
        BEFORE the update."""
        tok, lab = self._upload(features, labels)
        buf = self._forward(tok)
        self._losses(buf, lab, tok.shape[0], True)
        self._backward(tok, buf)
        self.global_step += 1
        t = self.global_step
        lr_t = self.learning_rate * math.sqrt(1.0 - ADAM_BETA2 ** t) / (1.0 - ADAM_BETA1 ** t)
        ptr = self._lib_mod.ptr
        self._check(self.lib.cham_adam_tf(ptr(self.params), ptr(self.grads), ptr(self.m), ptr(self.v), self.layout.n_params, self.layout.n_reg,
                                          self.l2_reg_lambda, lr_t, ADAM_BETA1, ADAM_BETA2, ADAM_EPS, self._stream()), "cham_adam_tf")
        self._last = buf
        return self.loss

    def eval_step(self, features, labels):
        """Loss and predictions of a batch without an update: (loss [3] numpy, predictions()); the (tp, fp, fn) of the multilabel
        heads are then in multilabel_counts()."""
        tok, lab = self._upload(features, labels)
        buf = self._forward(tok)
        self._losses(buf, lab, tok.shape[0], False)
        self._last = buf
        return self.loss.cpu().numpy(), self.predictions()

    def predict(self, features):
        """(acr_embedding [B, acr_embeddings_size] float32, predictions()) of a batch at ITS padded length."""
        tok, _ = self._upload(features, None)
        buf = self._forward(tok)
        lib, ptr, L = self.lib, self._lib_mod.ptr, self.layout
        dummy = self.torch.zeros(tok.shape[0], dtype=self.torch.int32, device=self.device)
        for n in L.heads:          # only the argmax output is used: PREDICT has no labels (all-zero labels, the loss slot is scratch)
            if n in self.multilabel:
                self._sigmoid_xent(buf, n, tok.shape[0], None, self.loss_terms.data_ptr(), False)
                continue
            self._check(lib.cham_acr_softmax_xent(ptr(buf['logits_' + n]), L.ldC[n], tok.shape[0], L.heads[n], ptr(dummy), None,
                                                  self.loss_terms.data_ptr(), None, ptr(buf['pred_' + n]), ptr(buf['row_ws']), self._stream()),
                        "cham_acr_softmax_xent")
        self._last = buf
        return buf['ace'][:, :L.A].cpu().numpy(), self.predictions()

    def predictions(self):
        """{head: argmax [B] int64 (multiclass) or the multi-hot x > 0 [B, C] uint8 (multilabel)} of the last batch."""
        L = self.layout
        return {n: self._last['pred_' + n][:, :L.heads[n]].cpu().numpy() if n in self.multilabel
                else self._last['pred_' + n].cpu().numpy().astype(np.int64) for n in L.heads}

    def multilabel_counts(self):
        """{multilabel head: (tp, fp, fn)} of the last batch, counted on the device against the batch's multi-hot targets (after predict,
        which has no labels: tp = fn = 0)."""
        return {n: tuple(int(v) for v in self._last['counts_' + n].cpu().numpy()) for n in self.multilabel}

    # ---- host views (tests, checkpoints)
    def logical_weights(self):
        flat = self.params.cpu().numpy()
        return OrderedDict((n, self.layout.gather(flat, n)) for n in self.layout.entries)

    def logical_grads(self):
        flat = self.grads.cpu().numpy()
        return OrderedDict((n, self.layout.gather(flat, n)) for n in self.layout.entries)

    def state_dict(self):
        return dict(params=self.params.cpu(), m=self.m.cpu(), v=self.v.cpu(), global_step=int(self.global_step))

    def load_state_dict(self, sd):
        if tuple(sd['params'].shape) != tuple(self.params.shape):
            raise ValueError("checkpoint holds %d parameters, the model has %d" % (sd['params'].numel(), self.params.numel()))
        self.params.copy_(sd['params']); self.m.copy_(sd['m']); self.v.copy_(sd['v'])
        self.global_step = int(sd['global_step'])


class ACR_ModelMultilabel(ACR_Model):
    """ACR_Model that also accepts multilabel heads (the Adressa label set: category0 multiclass + keywords multilabel).  A class of
    its own because the base class's refusal of such a head is part of the G1 trainer's tested interface (module docstring)."""

    MULTILABEL_HEADS = True
