"""NAR module model on MI355X: host orchestration of the HIP kernels in libchameleon_nar.so.

Mirrors nar_module/nar/nar_model.py of the reference:
  * ``NARModuleModel(mode, inputs, labels, ...)`` keeps the reference constructor (nar_model.py:102-129) and the
    attributes its SessionRunHook reads (:1435-1467);
  * the TF graph (:210-722) becomes an eager sequence of stream-ordered kernel launches over device-resident
    buffers: negative sampling -> de-duplicated feature assembly -> factorised PreCAR -> CAR -> UGRNN -> FCs ->
    scorer -> sampled softmax loss -> full backward -> L2 + TF-Adam.
PyTorch is only used for device memory, streams and (data-parallel) torch.distributed; all arithmetic of the step
runs in the hand-written HIP kernels.  There is no CPU fallback.
"""
import contextlib
import ctypes
import math
import os

import numpy as np
import torch

from .. import _lib
from .. import _roctx
from .._lib import check, ptr
from .candidate_rows import (ACT_LEAKY, ACT_NONE, ACT_TANH, Bf16Rows, F32Rows, H2Rows, P3Rows, blocked_plane_elements,  # noqa: F401
                             planes_from_blocked, planes_to_blocked)
from . import recurrent
from .clicked_items_state import lane_stream
from .input_rows import SITE_FC1, SITE_RNN_OUT, DenseInput, Dropout, FactorisedInput, FeatureRows, step_scalar
from .layout import ParamLayout
from .metrics import BEYOND_ACCURACY_PER_CLICK, ItemCoverage


class ModeKeys:                       # tf.estimator.ModeKeys
    TRAIN = 'train'
    EVAL = 'eval'
    PREDICT = 'infer'


# --loss_function: the value -> the `loss_kind` of cham_score_rankloss_* (csrc/rank_loss.hip); 'softmax' runs cham_score_softmax_* instead
LOSS_FUNCTIONS = ('softmax', 'bpr', 'top1', 'bpr_max', 'top1_max')


# Raw handle (hipStream_t as an int) of torch's current stream.  torch.cuda.current_stream() builds a Python Stream object (~8 us);
# a step makes ~100 launches, and with short sessions the host's enqueue time is what bounds the boundary throughput - the private
# C getters cost ~0.3 us.  (Fallback if a torch build lacks them.)
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_raw_device = getattr(torch._C, '_cuda_getDevice', None)


_raw_checked = False


def _stream():
    global _raw_stream, _raw_checked
    if _raw_stream is not None and _raw_device is not None:
        if not _raw_checked:       # private torch API: validate it once against the public one (a changed signature / meaning -> fall back)
            _raw_checked = True
            try:
                if int(_raw_stream(_raw_device())) != int(torch.cuda.current_stream().cuda_stream):
                    _raw_stream = None
            except Exception:
                _raw_stream = None
            if _raw_stream is None:
                return torch.cuda.current_stream().cuda_stream
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


class Tensor:
    """Lazy fetch handle: what a symbolic tf.Tensor attribute of the reference model is to its SessionRunHook
    (nar_model.py:1435-1456).  ``eval()`` returns the numpy value of the LAST executed step."""

    def __init__(self, name, fn):
        self.name, self._fn = name, fn

    def eval(self):
        v = self._fn()
        if torch.is_tensor(v):
            v = v.cpu().numpy()
        return v


class Placeholder:
    """tf.placeholder stand-in (nar_model.py:170-202): fed through ``NARModuleModel.feed(feed_dict)``."""

    def __init__(self, name):
        self.name = name

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, o):
        return isinstance(o, Placeholder) and o.name == self.name


# The Estimator's "variable store": TF re-creates the graph at every train()/evaluate() call and restores the
# variables from the checkpoint in model_dir; here the device-resident NARRuntime simply survives between calls.
_VARIABLE_STORE = None


class variable_store:
    def __init__(self, store):
        self.store = store

    def __enter__(self):
        global _VARIABLE_STORE
        self._prev, _VARIABLE_STORE = _VARIABLE_STORE, self.store
        return self.store

    def __exit__(self, *a):
        global _VARIABLE_STORE
        _VARIABLE_STORE = self._prev


_TORCH_DTYPE = {np.dtype(n).str: t for n, t in (('int64', torch.int64), ('int32', torch.int32), ('float32', torch.float32),
                                                   ('uint8', torch.uint8))}


def pack_offsets(arrays, align=256):
    """Byte offsets of a dict of numpy arrays packed back to back into one staging block (each start aligned: the device views of
    upload_batch reinterpret the block per dtype) and the block's size."""
    offs, total = {}, 0
    for k, a in arrays.items():
        offs[k] = total
        total += (a.nbytes + align - 1) & ~(align - 1)
    return offs, total


class _PinnedRing:
    """Page-locked staging buffers for the per-step host -> device copies: a batch's arrays are packed into one
    pinned arena and copied with truly asynchronous DMA (a copy from pageable memory goes through the driver's bounce buffer and
    blocks the host).  A ring of arenas; an arena is re-used only after the copies issued from it have completed (event)."""

    def __init__(self, n=4, nbytes=4 << 20):
        self.n, self.nbytes = n, nbytes
        self.bufs, self.events, self.k, self.off = [None] * n, [None] * n, -1, 0

    def begin(self, need):
        self.k = (self.k + 1) % self.n
        if self.events[self.k] is not None:
            self.events[self.k].synchronize()
        if self.bufs[self.k] is None or self.bufs[self.k].numel() < need:
            self.bufs[self.k] = torch.empty(max(need, self.nbytes), dtype=torch.uint8, pin_memory=True)
        self.off = 0

    def stage(self, a):
        n = a.nbytes
        if n == 0 or self.off + n > self.bufs[self.k].numel():      # (arena sized too small: this array goes through pageable memory)
            return torch.from_numpy(a)
        view = self.bufs[self.k][self.off:self.off + n]
        self.off += (n + 255) & ~255
        t = view.view(torch.from_numpy(a).dtype).view(a.shape)
        t.copy_(torch.from_numpy(a))
        return t

    def end(self, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self.events[self.k] = ev


def plane_arms(gemm_dtype, C):
    """(x3, p3, h2): which plane arithmetic the switches select for gemm_dtype and CAR width C (NARRuntime.__init__ explains each)."""
    x3 = gemm_dtype == 'f32' and os.environ.get("CHAM_GEMM_X3", "1") == "1"
    p3 = x3 and os.environ.get("CHAM_GEMM_P3", "1") == "1" and C % 256 == 0
    h2 = p3 and os.environ.get("CHAM_GEMM_H2", "1") == "1"
    return x3, p3, h2


class NARRuntime:
    """Everything that outlives a single train()/evaluate() call: weights + Adam slots in ONE flat HBM buffer,
    resident article tables (ACE matrix, metadata - re-fed from numpy every step by the reference,
    nar_model.py:1458-1467), global step, workspaces."""
    plans_created = 0         # plans built by plan() (bookkeeping: a first-seen padded length costs GBs of allocation)
    stream = staticmethod(_stream)      # raw handle of torch's current stream: what the arithmetic modules launch on

    def __init__(self, params, device='cuda:0', seed=42, weights=None):
        self.lib = _lib.load()
        self._views = {}
        _, p3, h2 = plane_arms(params.get('gemm_dtype', 'f32'), params['CAR_embedding_size'])
        if params.get('recommendations_ranking', 'mlp') == 'cosine' and p3 and not h2:
            raise ValueError("recommendations_ranking='cosine' is not supported on the three-bf16-plane arm (CHAM_GEMM_H2=0): its backward has "
                             "no plane-resident form there - use the default two-fp16-plane arm, CHAM_GEMM_P3=0, gemm_dtype 'f32_native' or 'bf16'")
        if not torch.cuda.is_available():
            raise _lib.ChameleonLibError("no ROCm device visible: the NAR step has no CPU path")
        self.device = torch.device(device)
        self.params = params
        acfg = params['articles_features_config']
        ace = np.ascontiguousarray(params['content_article_embeddings_matrix'], dtype=np.float32)
        self.n_items = acfg['article_id'].get('cardinality', ace.shape[0]) if 'article_id' in acfg else ace.shape[0]
        if self.n_items != ace.shape[0]:
            raise ValueError("article_id cardinality (%d) != ACE rows (%d)" % (self.n_items, ace.shape[0]))
        self.item_id_bits = max(1, int(self.n_items - 1).bit_length())      # radix passes of the row grouping (cham_group_rows)
        self.layout = ParamLayout(params['session_features_config'], acfg, self.n_items, ace.shape[1],
                                  params['CAR_embedding_size'], params['rnn_units'],
                                  params.get('rnn_num_layers', 1), params.get('rnn_cell', 'ugrnn'),
                                  params.get('internal_features_config'), params.get('max_cardinality_for_ohe', 10),
                                  params.get('recommendations_ranking', 'mlp'))
        L = self.layout
        # ranking head (--recommendations_ranking): 'mlp' = cand (.) pred -> 128 -> 64 -> 32 -> 1, 'cosine' = cos(pred, candidate row), no weights
        # (csrc/cosine.hip).  The softmax kernels then read cosq [R, 4] with these constants as their last layer
        self.cosine = L.ranking == 'cosine'
        logical = weights if weights is not None else L.init_logical(seed)
        dev = self.device
        self.flat = torch.from_numpy(L.pack(logical)).to(dev)
        self.m = torch.zeros_like(self.flat)
        self.v = torch.zeros_like(self.flat)
        self.grads = torch.zeros_like(self.flat)
        self.global_step = 0
        # The launch parameters that change from step to step (sampler key, the batch's max time stamp, sum(mask), Adam's lr_t) live in a
        # 32-byte DEVICE record (csrc/common.h ChamStepScalars, include/chameleon_nar.h "STEP SCALARS"), written by set_step_scalars() in
        # front of the step: the step's launches then carry no per-step host value and can be captured in a hipGraph (GraphedTrainStep).
        # CHAM_DEV_SCALARS=0: the by-value entry points (A/B arm; bit-identical results).  capturing: a graph capture is in progress - the
        # record is NOT written by the step's code (the replay writes it in front of every launch of the graph).
        self.dev_scalars = os.environ.get("CHAM_DEV_SCALARS", "1") == "1"
        # round 6: the loss record's kernels (L2 term, finalize) and the zero fill of the embedding gradients off the main lane (CHAM_LOSS_SIDE=0: on it)
        self.loss_side = os.environ.get("CHAM_LOSS_SIDE", "1") == "1"
        # round 6: per-click sums of dZ1 in the CAR dgrad's epilogue instead of a second pass over its 1 GB (CHAM_DGRAD_GROUPSUM=0: k_combine_bwd_u)
        self.dgrad_groupsum = os.environ.get("CHAM_DGRAD_GROUPSUM", "1") == "1"
        # round 6, the serial tail of the backward pass (profiles/r06_notes.md section 5b): dgamma / dbeta column sums with coalesced reads
        # through a workspace (CHAM_FEATURE_BWD_WS), the user-context half of the PreCAR input's backward on the third lane (CHAM_TAIL_SPLIT)
        self.feature_bwd_ws = os.environ.get("CHAM_FEATURE_BWD_WS", "1") == "1"
        self.tail_split = os.environ.get("CHAM_TAIL_SPLIT", "1") == "1"
        self.capturing = False
        self.scalars = None
        # 'f32': exact fp32 MFMA (BASELINE config 2, the default); 'bf16': operands of every Dense / matmul rounded to bf16 on
        # the fly, fp32 accumulation, fp32 storage / softmax / loss / Adam (BASELINE config 3)
        self.gemm_dtype = params.get('gemm_dtype', 'f32')
        # 'f32': fp32 operands; the wide GEMMs (N > 64) run as six bf16-plane products per fp32 product on the bf16 matrix cores
        # (csrc/gemm_x3.hip, fp32-grade error, 6/16 of the native fp32 matrix time), the narrow ones on v_mfma_f32_32x32x2_f32.
        # 'f32_native': every GEMM on the native fp32 MFMA (csrc/gemm.hip) - the reference arm of the parity tests.
        # 'bf16': BASELINE config 3 (bf16-resident candidate-row matrices, fp32 accumulate).
        if self.gemm_dtype not in ('f32', 'f32_native', 'bf16'):
            raise ValueError("gemm_dtype must be 'f32', 'f32_native' or 'bf16'")
        self.x3, self.p3, self.h2 = plane_arms(self.gemm_dtype, self.layout.C)
        # plane-resident CAR GEMMs (csrc/gemm_p3.hip): the candidate rows of Z1 and dZ2 live in HBM as three bf16 planes written by
        # their producers, W2 / W2^T get plane shadows once per step; same six plane products as gemm_x3.hip.  CHAM_GEMM_P3=0: the
        # on-the-fly split for those three GEMMs too (A/B arm).  The only shape gate is C % 256 == 0 below (decided once, here): any other
        # argument the plane kernels reject is an error of this module and raises from check() mid-step - loudly, there is no silent
        # fall-back to another arithmetic
        # two-fp16-plane form of those three GEMMs (csrc/gemm_h2.hip, round 4): planes (h, l) x a power-of-two scale derived on the device
        # from a bound of the matrix, THREE plane products instead of six - the kernels were power-limited, so halving the MFMA count is
        # what moves them; same float64-error bar as the six-product form (tests/test_gemm_h2_gpu.py).  CHAM_GEMM_H2=0: the three-bf16-plane arm
        # ... optionally with the candidate-row planes TILE-BLOCKED (round 6; [row tiles of 256][C / 32][256][32], csrc/common.h h2b_index): an
        # LDS-DMA request of the NT forms (16 rows x 32 k) is then 1 KB of whole 128-byte lines instead of sixteen half lines.  Bit-identical
        # results (same pieces, same products).  MEASURED (profiles/r06_notes.md section 2): the NT forms gain 4-5 % (stand-alone 1.41 -> 1.36 and
        # 1.44 -> 1.375 ms), the TN weight gradient loses 2.5 % stand-alone and 6-19 % in the step, the plane-writing combine 0.09 ms: the step is
        # 0.05 ms SLOWER (7.89 vs 7.84 ms) - the NT forms were power-limited, not line-fill-limited.  Hence OFF by default; CHAM_H2_BLOCKED=1 is
        # the arm (needs the 64-byte-piece NT kernel, CHAM_H2_NT_WIDE=1).
        blk = os.environ.get("CHAM_H2_BLOCKED", "0")          # 1 = both matrices, dz2 / z1 = only that one (A/B arms)
        self.h2_blocked = (self.h2 and blk in ("1", "dz2", "z1") and os.environ.get("CHAM_H2_NT_WIDE", "1") == "1" and self.layout.C % 32 == 0)
        self.h2_blocked_which = blk if self.h2_blocked else "0"
        # NT forms of those GEMMs (CAR forward, CAR dgrad) on the 64-byte-source-piece kernel (csrc/gemm_h2.hip gemm_h2w_kernel, round 5);
        # CHAM_H2_NT_WIDE=0: the 32-byte-piece kernel of round 4 (bit-identical results, A/B arm).  A LIBRARY-wide setting, made once per
        # process when the library is loaded (chameleon_recsys_amd/_lib.py): constructing a second runtime never flips the kernels of the first
        # the scorer's first layer on two fp16 planes split while staged (round 5) - THREE plane products instead of six for the 3 x 65 GFLOP that were
        # left on six-product kernels: its weight gradient (csrc/gemm_x3.hip NP = 2, cham_gemm_f32x2h; |cand (.) pred| <= 1: a constant scale record,
        # dS1 by its max row norm) and the products inside its fused dgrad (csrc/dm_fused.hip MODE 3, cham_dm_mulpred_h2h; Ws1's planes by its max
        # row norm).  CHAM_S1_H2=1 (default): those two BACKWARD kernels; =a: the forward GEMM as well (another 0.1 ms, but the 200-step loss
        # curve then left the float64 curve earlier than every other fp32 arm - one trajectory; the CPU oracle with the same rounding: 1.1-1.4 x -
        # profiles/r05_notes.md section 9 - so the forward keeps its exact 24-bit operands); =0: six bf16 products in all three
        mode = os.environ.get("CHAM_S1_H2", "1") if self.h2 else "0"
        self.s1_h2 = mode in ("1", "a")          # the weight gradient
        self.dm_f16 = self.s1_h2                  # the fused dgrad's own products
        self.s1_h2_fwd = mode == "a"              # the forward GEMM
        self.tf_random_seed = int(params.get('tf_random_seed', 42))
        # The input rows (nar/input_rows.py): the feature front end - it puts the resident article tables and the feature descriptors here, as
        # attributes of this runtime - and the factorised PreCAR input layer (the dense form of a step with dropout is built by that step)
        self.features = FeatureRows(self, ace)
        self.precar = FactorisedInput(self)
        self.gemm_ws = torch.empty(64 << 20, dtype=torch.float32, device=dev)        # 256 MB split-K partials (main stream)
        self.colsum_ws = torch.empty(4 << 20, dtype=torch.float32, device=dev)
        # the recurrent branch (8 CUs busy) runs on a side stream, overlapped with the candidate-row CAR GEMMs (normal priority: a
        # high-priority side lane was needed by the early builds only, profiles/r01_notes.md items 2 and 25)
        self.side_stream = lane_stream(dev, "side", 0)
        self._side_raw = self.side_stream.cuda_stream
        self.gemm_ws_side = torch.empty(32 << 20, dtype=torch.float32, device=dev)       # split-K partials of the side lane
        self.colsum_ws_side = torch.empty(2 << 20, dtype=torch.float32, device=dev)
        # third lane (round 5, CHAM_WGRAD_AUX): the small weight / bias gradients of the backward pass leave the side lane, whose W2 weight
        # gradient then starts the moment the main lane's CAR dgrad has finished instead of behind ~1 ms of small launches
        self.wgrad_aux = os.environ.get("CHAM_WGRAD_AUX", "1") == "1"
        self.aux_stream = lane_stream(dev, "aux", 0)
        self._aux_raw = self.aux_stream.cuda_stream
        self.gemm_ws_aux = torch.empty(16 << 20, dtype=torch.float32, device=dev)
        self.colsum_ws_aux = torch.empty(2 << 20, dtype=torch.float32, device=dev)
        # head of the step (round 5, CHAM_HEAD_SPLIT): the clicked rows' PreCAR combine + CAR layer 2 feed the recurrent branch only - they
        # run at the head of the side lane instead of in front of the main lane's plane producer and CAR forward GEMM
        self.head_split = os.environ.get("CHAM_HEAD_SPLIT", "1") == "1"
        self.overlap = os.environ.get("CHAM_OVERLAP", "1") == "1"           # CHAM_OVERLAP=0: the same program order on one stream
        # row-wise stages on the non-padded (session, time) positions only (upload_batch); CHAM_COMPACT=0 computes the padded
        # positions too and masks them, like the reference graph does
        self.compact = os.environ.get("CHAM_COMPACT", "1") == "1"
        # Measured schedule constants (the A/B arms they won against are in profiles/r01-r04_notes.md, not in the code):
        #   * K-splits of the plane-resident W2 weight gradient: 32 = two rounds of shorter workgroups, the main lane's PreCAR backward
        #     slips in between (16 = one workgroup per CU for the whole kernel, nothing else gets a CU meanwhile);
        #   * short (ragged) batches, at most this many candidate rows: the W2 weight gradient runs on the MAIN lane while that lane waits
        #     for the clicked-row gradient out of the side lane's recurrent chain (the chain does not shrink with the valid positions);
        #   * otherwise it waits for the main lane's CAR dgrad (two one-workgroup-per-CU matrix kernels only time-slice the chip) and is
        #     the side lane's LAST work: the small weight / bias gradients go first and run under that dgrad.
        self.p3_w2_splits = 32
        self.w2_main_rows = 131072
        #   * the same threshold selects the recurrent kernels (nar/recurrent.py: why, and the launch paths it selects between - made on first use)
        self.rnn_coop_rows = recurrent.default_coop_rows(L)
        self._rnn_paths = {}
        self.presample = os.environ.get("CHAM_PRESAMPLE", "1") == "1"       # NARModuleModel.presample (A/B switch)
        self.upload_stream = lane_stream(dev, "upload")       # H2D copies of a batch on their own stream, from a page-locked staging ring
        self.pinned = _PinnedRing()
        self.sumsq = torch.zeros(1024, dtype=torch.float32, device=dev)
        # bf16 configuration: bf16 shadows (plain + transposed) of the weights whose GEMMs run over the candidate rows, refreshed
        # whenever the fp32 master copy changed (csrc/gemm_b16.hip wants both operands k-contiguous: W^T forward, W dgrad)
        self.b16 = self.gemm_dtype == 'bf16'
        self.shadow, self._shadow_key, self.weights_version = {}, None, 0
        # bf16 configuration: the three candidate-row CAR GEMMs on the LDS-DMA core (csrc/gemm_p3.hip, gemm_b1_kernel) where it takes the
        # shape; the register-staged kernels of csrc/gemm_b16.hip otherwise (tests switch rt.b16_dma off to cover those at the G1 shape)
        self.b16_dma = self.gemm_dtype == 'bf16' and L.C % 256 == 0
        # ... and the scorer layer-1 dgrad fused with the cand (.) pred / CAR-tanh backward (csrc/dm_fused.hip, MODE 2) where the kernel takes
        # the shape (1 + N in [32, 256] is checked per step)
        self.dm_fused_b16 = self.gemm_dtype == 'bf16' and not self.cosine and L.entries['Ws1'].shape == (L.C, 128) and L.C % 64 == 0
        # plane arms: scorer layer-1 dgrad fused with the cand (.) pred backward (csrc/dm_fused.hip) where the kernel takes the shape; otherwise
        # (and for 1 + N outside [32, 256]) the two separate kernels
        self.dm_fused = self.p3 and not self.cosine and L.entries['Ws1'].shape == (L.C, 128) and L.C % 64 == 0
        if self.cosine:
            self.cos_w4 = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float32, device=dev)
            self.cos_b4 = torch.zeros(4, dtype=torch.float32, device=dev)
        # The arithmetic of the candidate rows (nar/candidate_rows.py): the arm the switches above select - it allocates its weight planes / shadows
        # and scale records here, as attributes of this runtime - and the fp32 rows every step falls back to that the planes do not take
        self.f32_rows = F32Rows(self)
        self.arm = Bf16Rows(self) if self.b16 else (H2Rows if self.h2 else P3Rows)(self) if self.p3 else self.f32_rows
        self._plans = {}
        self.max_plans = 24                       # padded lengths T seen in a run (seq_len - 1 = 19 at most for G1)
        self.plan_bytes_budget = 128 << 30        # of the 288 GB: activations of the cached shapes
        self.profile = None           # list -> per-GEMM-launch HIP-event timing (bench.py roofline leg)
        # data-parallel context (set by parallel.DataParallelNAR)
        self.dp_rank, self.dp_world, self.dp_allreduce, self.dp_sharded = 0, 1, None, None
        self.dp_early_bucket, self.dp_gather_slots, self.dp_mode, self.dp_active = None, None, 'allreduce', False

    # ---- views into the flat buffers
    def view(self, flat, name):
        """Tensor view of one logical tensor inside a flat buffer (cached per buffer: a step asks ~70 times)."""
        cache = self._views.get(id(flat))
        if cache is None or cache[0] is not flat:
            cache = self._views[id(flat)] = (flat, {})
        v = cache[1].get(name)
        if v is None:
            e = self.layout.entries[name]
            v = cache[1][name] = flat[e.offset:e.offset + int(np.prod(e.shape))].view(*e.shape)
        return v

    def p(self, name):
        return self.view(self.flat, name)

    def g(self, name):
        return self.view(self.grads, name)

    def logical_weights(self):
        return self.layout.unpack(self.flat.cpu().numpy())

    def logical_grads(self):
        return self.layout.unpack(self.grads.cpu().numpy())

    def load_logical_weights(self, logical):
        self.flat.copy_(torch.from_numpy(self.layout.pack(logical)))
        self.weights_version += 1

    def shadows_stale(self):
        return (self.b16 or self.p3) and (self.global_step, self.weights_version) != self._shadow_key

    def step_arm(self, planes=True):
        # the arm of a step or a plan: the configured one, or the fp32 rows where planes cannot be used - planes=False: dropout, no candidate
        # row; rt.p3 switched off on the live runtime (bench.py's native-MFMA leg)
        return self.arm if (self.b16 or (self.p3 and planes)) else self.f32_rows

    def refresh_shadows(self):
        """bf16 shadows (bf16 configuration) / bf16 plane shadows of W2 (plane-resident CAR GEMMs) of the candidate-row GEMM weights,
        once per weight version (one small launch per weight)."""
        if not self.shadows_stale():
            return
        key = (self.global_step, self.weights_version)
        self.arm.refresh_shadows(_stream())
        self._shadow_key = key

    def state_dict(self):
        """Weights + Adam slots + step.  Under the sharded data-parallel mode a rank only maintains the slots of the
        parameter slice it owns: they are all-gathered first (a COLLECTIVE - every rank must call state_dict()), so that any
        rank's checkpoint resumes the same optimizer trajectory in any mode (the mode is recorded)."""
        m, v = self.m, self.v
        if getattr(self, 'dp_gather_slots', None) is not None:
            m, v = self.dp_gather_slots(m, v)
        return {'flat': self.flat.cpu(), 'm': m.cpu(), 'v': v.cpu(), 'global_step': self.global_step,
                'dp_mode': getattr(self, 'dp_mode', 'allreduce'), 'dp_world': self.dp_world, 'layout': self.layout.fingerprint()}

    def load_state_dict(self, sd):
        """Restores weights + Adam slots; refuses a checkpoint written for another parameter layout (a changed feature config, cell
        type or CAR / RNN width with the same element count would otherwise be restored into the wrong offsets)."""
        if sd.get('layout') is not None and sd['layout'] != self.layout.fingerprint():
            raise ValueError("checkpoint was written for a different parameter layout (feature config / rnn_cell / sizes changed)")
        if tuple(sd['flat'].shape) != tuple(self.flat.shape):
            raise ValueError("checkpoint holds %d parameters, the model %d" % (sd['flat'].numel(), self.flat.numel()))
        self.flat.copy_(sd['flat']); self.m.copy_(sd['m']); self.v.copy_(sd['v'])
        self.global_step = int(sd['global_step'])
        self.weights_version += 1

    def rnn_path(self, pl):
        """The launch path of the recurrent stack (nar/recurrent.py) for the current step of `pl` - or, for a plan under construction, the
        path whose buffers it needs."""
        cls = recurrent.path_class(self.layout, pl.PC, pl.B, self.rnn_coop_rows)
        path = self._rnn_paths.get(cls)
        if path is None:
            path = self._rnn_paths[cls] = cls(self, self.layout)
        return path

    def rnn_coop_timed_out(self):
        """True if a cooperating recurrent workgroup ever gave up a bounded spin (synchronises; tests / bench / end of Estimator.train)."""
        coop = self._rnn_paths.get(recurrent.CoopUgrnn)
        return coop is not None and coop.timed_out(_stream())

    def plan(self, B, T, N, n_buf, Bg=None):
        """Buffers for one batch shape, cached: ragged hourly files produce a handful of padded lengths T.  Least-recently-used
        plans are dropped one at a time (count / byte budget), never all at once."""
        key = (B, T, N, n_buf, Bg or B, self.p3, self.h2)      # (the plane buffers of a plan follow the arithmetic it was built for)
        pl = self._plans.pop(key, None)
        if pl is None:
            need = StepPlan.estimate_bytes(self.layout, B, T, N, self)
            while self._plans and (len(self._plans) >= self.max_plans or
                                   need + sum(p.nbytes for p in self._plans.values()) > self.plan_bytes_budget):
                self._plans.pop(next(iter(self._plans)))          # oldest entry (dicts keep insertion order)
            pl = StepPlan(self, B, T, N, n_buf, Bg or B)
            pl.nbytes = pl.allocated_bytes()                       # what the eviction above counts for the plans already cached
            self.plans_created += 1
        self._plans[key] = pl                                      # (re)insert as most recently used
        return pl

    def _lane_ws(self, name):
        """The split-K / column-sum workspace of the lane (stream) the caller is enqueuing on: lanes run concurrently."""
        st = _stream()
        if st == self._side_raw:
            return getattr(self, name + '_side')
        if st == self._aux_raw:
            return getattr(self, name + '_aux')
        return getattr(self, name)

    def warm_plans(self, B, Ts, N, n_buf, Bg=None):
        """Builds the buffer set of every padded length in ``Ts`` now (a trainer's warm-up): hourly session files produce a handful of
        padded lengths T <= truncate_session_length - 1, and the first batch of each would otherwise allocate and zero-fill several GB
        in the middle of training (tens of ms).  Bounded by ``max_plans`` / ``plan_bytes_budget`` like any other plan."""
        for T in Ts:
            self.plan(B, int(T), N, n_buf, Bg)

    # ---- thin kernel wrappers -------------------------------------------------------------------------
    def _timed(self, splits, counters, record):
        return _TimedLaunch(self, splits, counters, record)

    def gemm(self, A, B, C, M, N, K, lda, ldb, ldc, transA=0, transB=0, bias=None, act=ACT_NONE, dref=None, ldr=0,
             dact=ACT_NONE, rowscale=None, ldrs=0, rs_div=1, accumulate=0, splits=1, force_f32=False, h2scales=None):
        """h2scales = (record of A [x rowscale], record of B): the two-fp16-plane form of the bf16x3 kernel (cham_gemm_f32x2h; default
        arithmetic only - the other arithmetics ignore it)."""
        bf16 = self.gemm_dtype == 'bf16' and not force_f32
        x3 = self.x3 and not force_f32

        def record(c0, c1):
            rec = _launch_record(M, N, K, transA, transB, act, dref is not None, dact, bias is not None, rowscale=rowscale is not None, bf16=bf16,
                                 splits=int(c1[0][15]), tile=next((i for i in range(13) if c1[0][i] != c0[0][i]), -1), epi=int(c1[0][14]))
            xt = next((i for i in (0, 1, 2, 4, 5) if c1[1][i] != c0[1][i]), -1) if x3 else -1
            if xt >= 0:          # ran on a bf16x3 instance (otherwise: delegated to the native kernels, recorded above)
                rec.update(x3=True, tile=xt & 3, x2h=xt >= 4, epi=int(c1[1][6]), splits=int(c1[1][7]))
            return rec
        with self._timed(splits, ('cham_gemm_launch_counts', 'cham_gemm_f32x3_launch_counts') if x3 else ('cham_gemm_launch_counts',), record) as (ws, ws_bytes):
            if h2scales is not None and x3 and not bf16 and self.s1_h2:
                if dref is not None or transB:
                    raise ValueError("the two-plane form takes the NN and TN shapes only")
                check(self.lib.cham_gemm_f32x2h(ptr(A), lda, transA, ptr(B), ldb, transB, ptr(C), ldc, M, N, K, ptr(bias), act, ptr(rowscale), ldrs,
                                                rs_div, accumulate, ws, ws_bytes, splits, ptr(h2scales[0]), ptr(h2scales[1]), _stream()), "cham_gemm_f32x2h")
            else:
                fn = self.lib.cham_gemm_bf16 if bf16 else (self.lib.cham_gemm_f32x3 if x3 else self.lib.cham_gemm_f32)
                check(fn(ptr(A), lda, transA, ptr(B), ldb, transB, ptr(C), ldc, M, N, K, ptr(bias), act,
                         ptr(dref), ldr, dact, ptr(rowscale), ldrs, rs_div, accumulate, ws, ws_bytes, splits, _stream()), "cham_gemm_f32")

    def gemm_b16(self, A, lda, transA, B, ldb, transB, C, ldc, out_f32, M, N, K, bias=None, act=ACT_NONE, dref=None, ldr=0,
                 dact=ACT_NONE, accumulate=0, splits=1, dma=False):
        """bf16-resident GEMM (csrc/gemm_b16.hip): NT (transA=0, transB=1) or TN (transA=1, transB=0).  dma: the LDS-DMA core
        (cham_gemm_b16_dma; NT with bf16 output / TN with fp32 output, M and N multiples of 256 for TN)."""
        def record(c0, c1):
            (c0,), (c,) = c0, c1
            how = (dict(b1=True, b1w=bool(c[4] > c0[4]), out_f32=int(transA)) if dma else
                   dict(tile=next((i for i in range(5) if c[i] != c0[i]), -1), b16=True, out_f32=int(c[5])))
            return _launch_record(M, N, K, transA, transB, act, dref is not None, dact, bias is not None, bf16=True, splits=int(c[7]), epi=int(c[6]), **how)
        with self._timed(splits, ('cham_gemm_p3_launch_counts' if dma else 'cham_gemm_b16_launch_counts',), record) as (ws, ws_bytes):
            if dma:
                check(self.lib.cham_gemm_b16_dma(ptr(A), lda, ptr(B), ldb, transA, ptr(C), ldc, M, N, K, ptr(bias), act, ptr(dref), ldr, dact,
                                                 accumulate, ws, ws_bytes, splits, _stream()), "cham_gemm_b16_dma")
            else:
                check(self.lib.cham_gemm_b16(ptr(A), lda, transA, ptr(B), ldb, transB, ptr(C), ldc, out_f32, M, N, K, ptr(bias), act, ptr(dref),
                                             ldr, dact, accumulate, ws, ws_bytes, splits, _stream()), "cham_gemm_b16")

    def gemm_p3(self, A, a_ps, lda, B, b_ps, ldb, tn, C, ldc, M, N, K, bias=None, act=ACT_NONE, dref_h=None, ldr=0, dact=ACT_NONE,
                accumulate=0, splits=1):
        """Plane-product GEMM over pre-split bf16 planes (csrc/gemm_p3.hip): NT (tn=0) or TN (tn=1, split-K)."""
        record = lambda c0, c1: _launch_record(M, N, K, tn, 0 if tn else 1, act, dref_h is not None, dact, bias is not None, splits=int(c1[0][7]),
                                               epi=int(c1[0][6]), p3=True)
        with self._timed(splits, ('cham_gemm_p3_launch_counts',), record) as (ws, ws_bytes):
            check(self.lib.cham_gemm_p3(ptr(A), a_ps, lda, ptr(B), b_ps, ldb, tn, ptr(C), ldc, M, N, K, ptr(bias), act, ptr(dref_h), ldr, dact,
                                        accumulate, ws, ws_bytes, splits, _stream()), "cham_gemm_p3")

    def gemm_h2(self, A, a_ps, lda, a_sc, B, b_ps, ldb, b_sc, tn, C, ldc, M, N, K, bias=None, act=ACT_NONE, dref_h=None, ldr=0, dact=ACT_NONE,
                accumulate=0, splits=1, a_tiles=0, b_tiles=0, dref_blocked=0, group_rows=0, groupsum=None):
        """Plane-product GEMM over two fp16 planes + scale records (csrc/gemm_h2.hip): NT (tn=0) or TN (tn=1, split-K).  a_tiles / b_tiles > 0:
        that operand is TILE-BLOCKED with this many row tiles per plane (include/chameleon_nar.h cham_gemm_h2b), dref_blocked: dref_h likewise.
        groupsum (dgrad only): the epilogue also leaves the column sums of every group of `group_rows` rows (cham_gemm_h2_dgrad_gs)."""
        def record(c0, c1):
            (c0,), (c,) = c0, c1
            return _launch_record(M, N, K, tn, 0 if tn else 1, act, dref_h is not None, dact, bias is not None, splits=int(c[7]), epi=int(c[6]),
                                  h2=True, h2w=bool(c[2] > c0[2]), h2blk=bool(c[3] > c0[3]))
        with self._timed(splits, ('cham_gemm_h2_launch_counts',), record) as (ws, ws_bytes):
            if groupsum is not None:
                check(self.lib.cham_gemm_h2_dgrad_gs(ptr(A), a_ps, lda, ptr(a_sc), ptr(B), b_ps, ldb, ptr(b_sc), ptr(C), ldc, M, N, K, ptr(dref_h), ldr,
                                                     a_tiles, dref_blocked, group_rows, ptr(groupsum), groupsum.numel() * 4, _stream()), "cham_gemm_h2_dgrad_gs")
            else:
                check(self.lib.cham_gemm_h2b(ptr(A), a_ps, lda, ptr(a_sc), ptr(B), b_ps, ldb, ptr(b_sc), tn, ptr(C), ldc, M, N, K, ptr(bias), act, ptr(dref_h),
                                             ldr, dact, accumulate, ws, ws_bytes, splits, a_tiles, b_tiles, dref_blocked, _stream()), "cham_gemm_h2b")

    def colsum(self, X, ld, R, F, out, w=None, accumulate=0, b16=False):
        ws = self._lane_ws('colsum_ws')
        check((self.lib.cham_colsum_b16 if b16 else self.lib.cham_colsum)(ptr(X), ld, R, F, ptr(w), ptr(out), accumulate, ptr(ws),
                                                                           ws.numel() * 4, _stream()), "cham_colsum")

    def set_step_scalars(self, step=0, max_ts=0, sum_mask=1.0, lr_t=0.0, fields=7, stream=None):
        """Writes the selected fields of the step-scalar record (fields: 1 = sampler keys (step, step + 1), 2 = max_ts + sum_mask, 4 = lr_t) on
        `stream` (default: the current one), in stream order in front of the launches that read it.  No-op during a graph capture."""
        if self.capturing:
            return
        if self.scalars is None:
            self.scalars = torch.zeros(max(8, self.lib.cham_step_scalars_bytes() // 4), dtype=torch.int32, device=self.device)
        check(self.lib.cham_step_scalars_set(ptr(self.scalars), int(step) & 0xFFFFFFFF, (int(step) + 1) & 0xFFFFFFFF, int(max_ts), float(sum_mask),
                                             float(lr_t), fields, _stream() if stream is None else stream), "cham_step_scalars_set")

    def side(self):
        """Context manager: run the enclosed launches on the side stream (or inline when overlap is disabled)."""
        return torch.cuda.stream(self.side_stream) if self.overlap else contextlib.nullcontext()

    def fork(self):
        if self.overlap:
            self.side_stream.wait_stream(torch.cuda.current_stream())

    def join(self):
        if self.overlap:
            torch.cuda.current_stream().wait_stream(self.side_stream)


def _launch_record(M, N, K, transA, transB, act, dref, dact, bias, rowscale=False, bf16=False, splits=1, tile=0, epi=0, **flags):
    # one entry of rt.profile (bench.py kernel_symbol / roofline leg, scripts/gemm_breakdown.py, scripts/insitu_gemm.py)
    return dict(M=M, N=N, K=K, transA=transA, transB=transB, splits=splits, act=act, dref=dref, dact=dact, bias=bias, rowscale=rowscale,
                bf16=bf16, tile=tile, epi=epi, **flags)


def _launch_counts(fn, n=16):      # what a launch-counter entry point of the library has counted (8 or 16 counters)
    out = (ctypes.c_longlong * n)()
    fn(out, 0)
    return list(out)


class _TimedLaunch:
    """NARRuntime._timed(splits, counters, record): context manager around ONE launch of the GEMM family."""
    # Yields (pointer, bytes) of the lane's split-K workspace ((None, 0) for splits == 1); while rt.profile is a list, two HIP events on the current
    # stream immediately around the launch and record(c0, c1) + ev=(start, end) appended for bench.py's roofline (c0 / c1: the launch counters named
    # in `counters` before / after).  (A class, not a generator: with rt.profile None a launch pays two near-empty calls.)
    __slots__ = ('rt', 'ws', 'counters', 'record', 'e0', 'c0')

    def __init__(self, rt, splits, counters, record):
        self.rt, self.counters, self.record = rt, counters, record
        ws = rt._lane_ws('gemm_ws') if splits != 1 else None
        self.ws = (ptr(ws), ws.numel() * 4) if ws is not None else (None, 0)

    def __enter__(self):
        if self.rt.profile is not None:
            self.e0, self.c0 = torch.cuda.Event(enable_timing=True), [_launch_counts(getattr(self.rt.lib, name)) for name in self.counters]
            self.e0.record()       # torch's current stream == the stream the kernel is launched on (_stream())
        return self.ws

    def __exit__(self, exc_type, exc, tb):
        if self.rt.profile is not None and exc_type is None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            c1 = [_launch_counts(getattr(self.rt.lib, name)) for name in self.counters]
            self.rt.profile.append(dict(self.record(self.c0, c1), ev=(self.e0, e1)))


class StepPlan:
    """Device buffers for one (B, T, N) shape.  Row layouts: see csrc/scorer.hip."""

    @staticmethod
    def estimate_bytes(L, B, T, N, rt=None):
        """Dominant buffers only (decides what to evict BEFORE the plan exists; the plan then records what it really allocated):
        Z1, Z2, dZ1, dZ2 over all CAR rows + the scorer activations over the candidate rows + the plane-resident operands of the
        candidate-row CAR GEMMs (Z1 and dZ2 as two fp16 / three bf16 planes), the b2 partial sums and the segment table."""
        rows = B * T * (N + 2)
        head = 4 + 4 + 2 if getattr(L, 'ranking', 'mlp') == 'cosine' else 2 * (128 + 64 + 32)      # cosine head: cosq + its scratch gradient, rz, the bound buffer
        need = 4 * (4 * rows * L.C + rows * head)        # (the bf16 configuration needs ~5/8 of this)
        if rt is not None and rt.p3:
            need += (H2Rows if rt.h2 else P3Rows).estimate_bytes(rt, L, B, T, N)
        return need

    def allocated_bytes(self):
        """Bytes of device memory this plan holds (every tensor attribute, lists and dicts of tensors included)."""
        seen, total = set(), 0

        def walk(x):
            nonlocal total
            if torch.is_tensor(x):
                st = x.untyped_storage()
                if st.data_ptr() not in seen:
                    seen.add(st.data_ptr())
                    total += st.nbytes()
            elif isinstance(x, (list, tuple)):
                for y in x:
                    walk(y)
            elif isinstance(x, dict):
                for y in x.values():
                    walk(y)
        for v in vars(self).values():
            walk(v)
        return total

    def __init__(self, rt, B, T, N, n_buf, Bg):
        L, dev = rt.layout, rt.device
        self.B, self.T, self.N, self.n_buf, self.Bg = B, T, N, n_buf, Bg
        self.BT = BT = B * T
        self.NC = NC = N + 1
        self.Rc = Rc = BT * NC
        self.Rall = Rall = BT + Rc
        self.pmax = pmax = 20 * N
        self.RV = RV = 2 * BT + pmax + 1
        C, Hp, Fc, Fi = L.C, L.Hp, L.Fc, L.Fi
        self.C = C
        f32 = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        i64 = lambda *s: torch.zeros(*s, dtype=torch.int64, device=dev)
        # sampler
        # two sets of sampler outputs: the next step's negatives can be drawn (NARModuleModel.presample) while this step's
        # backward still reads its own
        self._samp = [dict(neg_ids=i64(B, T, N), neg_slot=torch.zeros(B, T, N, dtype=torch.int32, device=dev), pool=i64(pmax),
                           canon=torch.zeros(pmax, dtype=torch.int32, device=dev), meta=torch.zeros(4, dtype=torch.int32, device=dev))
                      for _ in range(2)]
        self.use_sampler_set(0)
        need = rt.lib.cham_combine_bwd_workspace_bytes(L.C, B * T, N, 20 * N)
        if need > rt.gemm_ws.numel() * 4:
            rt.gemm_ws = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        if need > rt.gemm_ws_side.numel() * 4:
            rt.gemm_ws_side = torch.empty((need + 3) // 4, dtype=torch.float32, device=dev)
        self.ws_bytes = rt.lib.cham_neg_sample_workspace_bytes(Bg * (T + 1), int(rt.params['recent_clicks_buffer_max_size']), n_buf)
        self.sampler_ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=dev)
        # features
        self.ids_all = i64(RV)
        self.ref_ts = i64(RV)
        self.rec_raw, self.nov_raw = f32(RV), f32(RV)
        self.stats = f32(3, 8)
        self.stat_scratch = f32(3 * max(1, int(rt.params['recent_clicks_for_normalization'])))
        self.w_rows = f32(RV)
        self.perm = torch.zeros(RV, dtype=torch.int32, device=dev)          # item rows grouped by id (cham_group_rows)
        self.seg = torch.zeros(int(rt.lib.cham_group_rows_segments_len(RV)), dtype=torch.int32, device=dev)      # its segment table
        self.group_ws = torch.zeros(int(rt.lib.cham_group_rows_workspace_bytes(RV)) // 4, dtype=torch.int32, device=dev)
        self.Xc_raw, self.Xc_s, self.dXc = f32(BT, Fc), f32(BT, Fc), f32(BT, Fc)
        self.Xi_raw, self.Xi_s, self.dXi = f32(RV, Fi), f32(RV, Fi), f32(RV, Fi)
        # PreCAR input layer (nar/input_rows.py: the factorised form; the dense form of the dropout path allocates on its first step), CAR
        rt.precar.alloc(self, f32)
        # Z1, Z2, dZ2, dZ1 (+ planes, scale records, b2 partial sums) in the arithmetic the plan is built for; self.arm: the arm of the LAST
        # step on this plan (forward() sets it, backward() and cand_Z1() read it)
        self.gsum = self.arm = None
        arm = rt.step_arm()
        arm.alloc(self, f32)
        cand = lambda *s: torch.empty(*s, dtype=torch.bfloat16 if arm.b16 else torch.float32, device=dev)      # storage of the matrices with one row per candidate
        # RNN
        self.seq_len = torch.zeros(B, dtype=torch.int32, device=dev)
        NG = L.NG
        self.xproj = [f32(BT, NG * Hp) for _ in range(L.L)]
        self.dxproj = f32(BT, NG * Hp)
        self.rnn_out = [f32(BT, Hp) for _ in range(L.L)]
        self.hprev = [f32(BT, Hp) for _ in range(L.L)]
        self.G = [f32(BT, Hp) for _ in range(L.L)]
        self.Cc = [f32(BT, Hp) for _ in range(L.L)]
        four = L.cell in ('gru', 'lstm')          # GRU: r and r * h_prev; LSTM: its third and fourth gate
        self.R = [f32(BT, Hp) if four else None for _ in range(L.L)]
        self.RH = [f32(BT, Hp) if four else None for _ in range(L.L)]
        self.drnn = f32(BT, Hp)
        # FCs / scorer
        self.FC1, self.dFC1 = f32(BT, 512), f32(BT, 512)
        self.pred, self.dpred = f32(BT, C), f32(BT, C)
        if rt.cosine:      # cos(pred, candidate row) in column 0 of cosq (the softmax kernels' "S3", K3 = 4; dcosq: their scratch "dS3"), the inverse
            # norms of the rows and of pred, and the bound buffer |ds| rz of the two-plane backward (csrc/cosine.hip); fp32 in every arm
            self.cosq, self.dcosq = f32(Rc, 4), f32(Rc, 4)
            self.rz, self.rp, self.cos_t = f32(Rc), f32(BT), f32((Rc + 3) & ~3)
        else:
            self.S1, self.dS1 = cand(Rc, 128), cand(Rc, 128)
            self.S2, self.dS2 = cand(Rc, 64), cand(Rc, 64)
            self.S3, self.dS3 = cand(Rc, 32), cand(Rc, 32)
        self.ds = f32(Rc)
        self.logits, self.probs = f32(BT, NC), f32(BT, NC)
        self.nll = f32(BT)
        self.nov_aux = f32(BT, 3)
        self.div_sp = self.div_e = None       # --diversity_reg_factor > 0: S p [BT, NC] and p^T S p [BT] of the step (ensure_diversity)
        self.rank_aux = None                  # --loss_function other than softmax: the loss's per-click record (ensure_rank_aux)
        self.mask = torch.zeros(BT, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros(3, dtype=torch.float32, device=dev)
        # valid-position compaction (see NARModuleModel.upload_batch): compact copies of the sampler output, and the
        # [B, T]-layout staging buffers either side of the recurrent stack
        self.neg_ids_c = i64(BT, N)
        self.neg_slot_c = torch.zeros(BT, N, dtype=torch.int32, device=dev)
        self.Z2f, self.rnn_c, self.drnn_c, self.dxproj_c = f32(BT, C), f32(BT, Hp), f32(BT, Hp), f32(BT, NG * Hp)
        self.pos, self.P, self.PC = None, BT, Rc         # of the current step: compaction map, valid positions, candidate rows (P * NC)
        # ... and the launch path of its recurrent stack (nar/recurrent.py; forward() sets it, backward() reads it), which adds the buffers only
        # that path needs to the shared ones under "RNN" above
        self.rnn = rt.rnn_path(self)
        self.rnn.alloc(self, f32)
        # made on first need: the event of the side lane's row grouping (training-mode forward), the item rows a data-parallel step can touch
        # (sparse modes), the dense input form's buffers; precar: the input form of the LAST step on this plan, cat: its context columns
        # (nar/input_rows.py); nbytes: set by NARRuntime.plan once the plan is built
        self.grouped_ev = self.touched = self.Xd = self.precar = self.cat = None
        self.nbytes = 0
        # The zero fills above run on the stream that built the plan.  A stream that touches these buffers without being ordered behind
        # that point must wait for this event first: presample() may be the FIRST user of a plan (a padded length T seen for the first
        # time), it writes the sampler outputs on the state's stream - and the fills, still queued behind the running step, would wipe them.
        self.created = torch.cuda.Event()
        self.created.record()

    def ensure_rows(self, name):
        """The fp32 matrix `name` with one row per CAR row ([BT + Rc, C]): allocated in full on first need (see __init__).  Called before
        the step's first write to it."""
        t = getattr(self, name)
        if t.shape[0] < self.Rall:
            t = torch.empty(self.Rall, t.shape[1], dtype=t.dtype, device=t.device)
            setattr(self, name, t)
            self.nbytes = self.allocated_bytes()         # what the plan cache's byte budget counts (NARRuntime.plan)
        return t

    def ensure_diversity(self):
        """The two buffers of the content-diversity term (csrc/diversity.hip), allocated on the first step of a model that has it."""
        if self.div_sp is None:
            dev = self.probs.device
            self.div_sp = torch.empty(self.BT, self.NC, dtype=torch.float32, device=dev)
            self.div_e = torch.empty(self.BT, dtype=torch.float32, device=dev)
            self.nbytes = self.allocated_bytes()
        return self.div_sp, self.div_e

    def ensure_rank_aux(self):
        """The per-click record a pairwise ranking loss carries from forward to backward ([BT, 8]; csrc/rank_loss.hip), allocated on the
        first step of a model with a non-default --loss_function."""
        if self.rank_aux is None:
            self.rank_aux = torch.empty(self.BT, 8, dtype=torch.float32, device=self.probs.device)
            self.nbytes = self.allocated_bytes()
        return self.rank_aux

    def cand_Z1(self, P=None):
        """Candidate rows of the PreCAR output of the last step as fp32 [P * NC, C] (tests): the fp32 matrix, or the sum of its planes."""
        P = self.P if P is None else P
        n = P * self.NC
        return self.arm.cand_Z1(self, P, n)

    def use_sampler_set(self, k):
        self._samp_cur = k
        for name, t in self._samp[k].items():
            setattr(self, name, t)

    def full_rows(self, x, group=1):
        """Debug / test helper: rows of the current step (one group of ``group`` rows per valid position) -> the [B*T*group, ...]
        layout with zeros at padded positions."""
        x = x[:self.P * group]
        if self.pos is None:
            return x
        out = torch.zeros((self.BT * group,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
        out.view(self.BT, -1)[self.pos.long()] = x.reshape(self.P, -1)
        return out


class NARModuleModel:
    """Reference constructor signature: nar_module/nar/nar_model.py:102-129 (+ ``runtime``, the device-resident
    state that TF keeps in its checkpoint / session)."""

    def __init__(self, mode, inputs, labels, session_features_config, articles_features_config, batch_size, lr, keep_prob,
                 negative_samples, negative_sample_from_buffer, content_article_embeddings_matrix, rnn_num_layers=1,
                 softmax_temperature=1.0, reg_weight_decay=0.0, recent_clicks_buffer_hours=1.0,
                 recent_clicks_buffer_max_size=1000, recent_clicks_for_normalization=1000, articles_metadata=None,
                 plot_histograms=False, metrics_top_n=5, elapsed_days_smooth_log_base=1.3, popularity_smooth_log_base=2.0,
                 CAR_embedding_size=256, rnn_units=256, max_cardinality_for_ohe=10, novelty_reg_factor=0.0,
                 diversity_reg_factor=0.0,
                 internal_features_config={'recency': True, 'novelty': True, 'article_content_embeddings': True,
                                           'item_clicked_embeddings': True},
                 eval_cold_start=False, runtime=None, rnn_cell='ugrnn', gemm_dtype='f32', recommendations_ranking='mlp',
                 loss_function='softmax', bpr_max_reg=0.5):
        # log_base / log_1p bases of the recency and novelty features (nar_model.py:28-34, 1071-1075, 1148): launch scalars of the kernels
        for b in (elapsed_days_smooth_log_base, popularity_smooth_log_base):
            if not (b > 0.0) or b == 1.0:
                raise ValueError("log bases must be > 0 and != 1")
        self.elapsed_days_smooth_log_base = float(elapsed_days_smooth_log_base)
        self.popularity_smooth_log_base = float(popularity_smooth_log_base)
        self.novelty_reg_factor = float(novelty_reg_factor)
        # content-diversity regulariser (the reference's commented-out loss, nar_model.py:551-636, 685-702)
        self.diversity_reg_factor = float(diversity_reg_factor)
        if not (self.diversity_reg_factor >= 0.0):
            raise ValueError("diversity_reg_factor must be >= 0")
        # training objective over the [positive, N negatives] scores (--loss_function): 'softmax' = the reference's
        # sampled softmax + NLL (csrc/scorer.hip), the others GRU4Rec's pairwise ranking losses (csrc/rank_loss.hip).  Not part of the
        # parameter layout: a checkpoint written under one loss loads under another
        if loss_function not in LOSS_FUNCTIONS:
            raise ValueError("loss_function=%r: one of %s" % (loss_function, ', '.join(LOSS_FUNCTIONS)))
        self.loss_function = loss_function
        self.bpr_max_reg = float(bpr_max_reg)
        if not (self.bpr_max_reg >= 0.0):
            raise ValueError("bpr_max_reg must be >= 0")
        self.is_training = (mode == ModeKeys.TRAIN)
        if self.is_training and not (0.0 < keep_prob <= 1.0):
            raise ValueError("dropout_keep_prob must be in (0, 1]")
        self.mode = mode
        self.inputs, self.labels = inputs, labels
        self.lr, self.keep_prob = lr, keep_prob
        self.negative_samples = negative_samples
        self.negative_sample_from_buffer = negative_sample_from_buffer
        self.softmax_temperature = softmax_temperature
        self.reg_weight_decay = reg_weight_decay
        self.metrics_top_n = metrics_top_n
        self.recent_clicks_for_normalization = recent_clicks_for_normalization
        self.recent_clicks_buffer_max_size = recent_clicks_buffer_max_size
        self.eval_cold_start = eval_cold_start
        if runtime is None and _VARIABLE_STORE is not None and _VARIABLE_STORE.get('runtime') is not None:
            runtime = _VARIABLE_STORE['runtime']
        if runtime is None:
            seed = _VARIABLE_STORE.get('tf_random_seed', 42) if _VARIABLE_STORE is not None else 42
            runtime = NARRuntime(dict(tf_random_seed=seed,session_features_config=session_features_config,
                                      articles_features_config=articles_features_config,
                                      content_article_embeddings_matrix=content_article_embeddings_matrix,
                                      articles_metadata=articles_metadata, CAR_embedding_size=CAR_embedding_size,
                                      rnn_units=rnn_units, rnn_num_layers=rnn_num_layers, rnn_cell=rnn_cell, gemm_dtype=gemm_dtype,
                                      recommendations_ranking=recommendations_ranking,
                                      internal_features_config=internal_features_config,
                                      max_cardinality_for_ohe=max_cardinality_for_ohe,
                                      recent_clicks_buffer_max_size=recent_clicks_buffer_max_size,
                                      recent_clicks_for_normalization=recent_clicks_for_normalization), seed=seed)
            if _VARIABLE_STORE is not None:
                _VARIABLE_STORE['runtime'] = runtime
        self.rt = runtime
        if recommendations_ranking not in ('mlp', 'cosine'):
            raise ValueError("recommendations_ranking must be 'mlp' or 'cosine'")
        self.recommendations_ranking = runtime.layout.ranking      # (the runtime's parameter layout decides: it may outlive this model)
        # state "placeholders" (nar_model.py:195-202): fed by ItemsStateUpdaterHook.before_run
        self.articles_recent_pop_norm = None
        self.pop_recent_items_buffer = None
        self._dev_state = None
        self.total_loss = None
        self._accumulating = False             # train_step_microbatched: gradients of a micro-batch are not final
        self.train = self.train_step           # the reference's ``model.train`` op
        self._eval_iter = 0
        self._eval = None
        self._ba = None                        # enable_beyond_accuracy_metrics: launch scalars; _ba_buffers: maps, counts, per-click values
        self._ba_buffers = None
        self._rh = None                        # enable_rank_histogram: the device record of cham_eval_rank_hist
        self._fr = None                        # enable_full_candidate_ranking: the record and the last batch's ranks (nar/full_eval.py)
        self.dp = None                        # parallel.DataParallelNAR.attach: the data-parallel wrapper this model's batches go through
        # attributes ItemsStateUpdaterHook fetches / feeds (nar_model.py:1435-1467)
        inp = lambda k: Tensor(k, lambda: np.asarray(self.inputs[k]))
        self.item_clicked = inp('item_clicked')
        self.event_timestamp = Tensor('event_timestamp', lambda: np.asarray(self.inputs['event_timestamp'])[..., None])   # :233
        self.session_id, self.user_id = inp('session_id'), inp('user_id')
        self.next_item_label = Tensor('next_item_label', lambda: np.asarray(self.labels['label_next_item']))
        self.label_last_item = Tensor('label_last_item', lambda: np.asarray(self.labels['label_last_item']))
        self.batch_negative_items = Tensor('batch_negative_items', lambda: self._plan.neg_ids)
        self.predicted_item_ids = Tensor('predicted_item_ids', lambda: self._eval['pred_ids'])
        self.predicted_item_probs = Tensor('predicted_item_probs', lambda: self._eval['pred_probs'])
        self.label_rank = Tensor('label_rank', lambda: self._eval['label_rank'])
        self.batch_items_count = Tensor('batch_items_count', lambda: self._batch_counts()[0])          # :258
        self.batch_unique_items_count = Tensor('batch_unique_items_count', lambda: self._batch_counts()[1])   # :261
        self.loss_t = Tensor('total_loss', lambda: self.total_loss)
        self.ph_articles_recent_pop_norm = Placeholder('articles_recent_pop_norm')      # :195
        self.ph_pop_recent_items_buffer = Placeholder('pop_recent_items_buffer')        # :200
        self.ph_content_article_embeddings_matrix = Placeholder('content_article_embeddings_matrix')   # :170
        self.ph_articles_metadata = {n: Placeholder('articles_metadata/' + n) for n in (articles_metadata or {})}

    def _batch_counts(self):
        ic = np.asarray(self.inputs['item_clicked'])
        nz = ic[ic != 0]
        return int(nz.shape[0]), int(np.unique(nz).shape[0])

    def feed(self, feed_dict):
        """session.run(feed_dict=...) of the hook (nar_model.py:1458-1467).  The ACE matrix / metadata placeholders are
        accepted and ignored when they are the arrays already resident in HBM (the reference re-feeds them every step
        only to keep them out of the checkpoint)."""
        by_name = {(k.name if isinstance(k, Placeholder) else k): v for k, v in feed_dict.items()}
        self.feed_state(by_name['articles_recent_pop_norm'], by_name['pop_recent_items_buffer'])

    # ------------------------------------------------------------------ host -> device
    def feed_device_state(self, state):
        """Device-resident state (clicked_items_state.DeviceClickedItemsState): nothing is uploaded."""
        state.sync_to_current()           # the previous batch's update runs on the state's own stream
        self.articles_recent_pop_norm = state
        self.pop_recent_items_buffer = state
        self._dev_state = dict(buffer=state.buf_ids, pop_norm=state.pop_norm, last=state.buf_ids,
                               n_last=min(self.recent_clicks_for_normalization, state.buf_ids.numel()) if state.n_updates > 0 else 0,
                               device=True)

    def feed_state(self, pop_norm, buffer_ids):
        """The hook's feed_dict (nar_model.py:1458-1463)."""
        if getattr(pop_norm, 'is_device', False):
            return self.feed_device_state(pop_norm)
        self.articles_recent_pop_norm = pop_norm
        self.pop_recent_items_buffer = buffer_ids
        dev = self.rt.device
        buf = np.ascontiguousarray(buffer_ids, dtype=np.int64)
        nz = buf[buf != 0][: self.recent_clicks_for_normalization]           # nar_model.py:1041-1044
        self._dev_state = dict(
            buffer=torch.from_numpy(buf).to(dev, non_blocking=True),
            pop_norm=torch.from_numpy(np.ascontiguousarray(pop_norm, dtype=np.float32)).to(dev, non_blocking=True),
            last=torch.from_numpy(np.ascontiguousarray(nz)).to(dev, non_blocking=True), n_last=int(nz.shape[0]))

    def upload_current(self, features, labels):
        """How a batch of the input stream reaches the device: this rank's row shard of it (with the global integers and ``row_begin``)
        under an attached data-parallel wrapper, the whole batch otherwise."""
        if self.dp is not None:
            return self.dp.upload(features, labels)
        return self.upload_batch(features, labels)

    def upload_batch(self, features, labels, global_features=None, global_labels=None, row_begin=0):
        """numpy batch (input_fn output) -> device tensors + the few host scalars the launch parameters need."""
        L, dev = self.rt.layout, self.rt.device
        item_clicked = np.ascontiguousarray(features['item_clicked'], dtype=np.int64)
        B, T = item_clicked.shape
        gf = features if global_features is None else global_features
        gl = labels if global_labels is None else global_labels
        aci = np.concatenate([np.asarray(gf['item_clicked'], np.int64), np.asarray(gl['label_last_item'], np.int64).reshape(-1, 1)], 1)
        ssz = np.asarray(features['session_size'], dtype=np.int64).reshape(-1)
        seq_len = (ssz - 1).astype(np.int32)                                   # nar_model.py:227
        mask = (np.arange(T)[None, :] < seq_len[:, None])                      # :231
        g_ssz = np.asarray(gf['session_size'], dtype=np.int64).reshape(-1)
        g_T = np.asarray(gf['item_clicked']).shape[1]
        sum_mask = float(np.minimum(np.maximum(g_ssz - 1, 0), g_T).sum())      # global denominator (:664)
        ets = np.ascontiguousarray(features['event_timestamp'], dtype=np.int64)
        max_ts = int(np.asarray(gf['event_timestamp']).max())                  # :235
        cat = np.stack([np.asarray(features[n], np.int64).reshape(-1) for n in L.ctx_cat_names]) if L.ctx_cat_names \
            else np.zeros((1, B * T), np.int64)
        num = np.stack([np.asarray(features[n], np.float32).reshape(-1) for n in L.ctx_num_names]) if L.ctx_num_names \
            else np.zeros((1, B * T), np.float32)
        g_ets = ets if global_features is None else np.ascontiguousarray(gf['event_timestamp'], dtype=np.int64)
        label_next = np.ascontiguousarray(labels['label_next_item'], dtype=np.int64)
        # Valid-position compaction.  The reference computes every padded (session, time) position and multiplies it
        # away with sequence_mask (nar_model.py:231, 664); here the row-wise stages (features, CAR, scorer, softmax and
        # their gradients) run on the P non-padded positions only - same loss and gradients, P/(B*T) of the work
        # (G1-like session lengths: ~1/3).  Only the sampler (keyed by (row, position)) and the recurrent stack keep
        # the [B, T] layout.
        mrows = mask.reshape(-1)
        pos = np.flatnonzero(mrows).astype(np.int32)
        P = int(pos.shape[0])
        host = dict(g_event_ts=g_ets, aci=aci, item_clicked=item_clicked, label_next=label_next, event_ts=ets, seq_len=seq_len)
        if global_features is not None:      # lengths of the GLOBAL batch's sessions (a row shard's first-batch statistics: FeatureRows)
            host['g_seq_len'] = np.minimum(np.maximum(g_ssz - 1, 0), g_T).astype(np.int32)
        compacted = self.rt.compact and 0 < P < B * T
        if compacted:
            host.update(pos=pos, ic_rows=item_clicked.reshape(-1)[pos], ln_rows=label_next.reshape(-1)[pos], ets_rows=ets.reshape(-1)[pos],
                        mask=np.ones(P, np.uint8), cat=cat[:, pos], num=num[:, pos])
        else:
            host.update(mask=mrows.astype(np.uint8), cat=cat, num=num)
        d = dict(B=B, T=T, Bg=aci.shape[0], row_begin=row_begin, sum_mask=sum_mask, max_ts=max_ts, P=P if compacted else B * T, pos=None)
        d.update(self._h2d(host))
        if not compacted:
            d.update(ic_rows=d['item_clicked'].view(-1), ln_rows=d['label_next'].view(-1), ets_rows=d['event_ts'].view(-1))
        if global_features is None:
            d['g_seq_len'] = d['seq_len']
        return d

    def _h2d(self, host):
        """The batch's arrays -> device tensors + the 'uploaded' event its consumers (forward, presample) wait for.  The copies
        run on their own stream: queued behind the running step's kernels on the compute stream, a copy from pageable host
        memory would block the host until that step has finished (one implicit synchronisation per step).  With the pinned
        ring (default) the arrays are packed into ONE page-locked arena and cross in ONE copy into one device block the
        returned tensors are views of (13 copies, allocations and stream records fewer per step on the host)."""
        dev = self.rt.device
        main, up, ring = torch.cuda.current_stream(), self.rt.upload_stream, self.rt.pinned
        arrs = {k: np.ascontiguousarray(a) for k, a in host.items()}
        out = {}
        if ring is not None:
            offs, total = pack_offsets(arrs)
            ring.begin(total)
            arena = ring.bufs[ring.k]
            bytes_view = arena.numpy()
            for k, a in arrs.items():
                if a.nbytes:
                    bytes_view[offs[k]:offs[k] + a.nbytes] = a.reshape(-1).view(np.uint8)
            with torch.cuda.stream(up if up is not None else main):
                block = torch.empty(max(total, 256), dtype=torch.uint8, device=dev)
                block[:total].copy_(arena[:total], non_blocking=True)
            if up is not None:
                block.record_stream(main)         # allocated on the upload stream, consumed on the compute stream
            for k, a in arrs.items():
                out[k] = block[offs[k]:offs[k] + a.nbytes].view(_TORCH_DTYPE[a.dtype.str]).view(a.shape)
            # the packed device block and its layout: a batch of the same shape can be copied into a persistent input slot with ONE
            # device-to-device copy (GraphedTrainStep)
            out['_block'], out['_total'] = block, total
            out['_layout'] = tuple((k, offs[k], a.dtype.str, a.shape) for k, a in arrs.items())
        else:
            for k, a in arrs.items():
                x = torch.from_numpy(a)
                if up is None:
                    out[k] = x.to(dev, non_blocking=True)
                    continue
                with torch.cuda.stream(up):
                    x = x.to(dev, non_blocking=True)
                x.record_stream(main)
                out[k] = x
        out['uploaded'] = torch.cuda.Event()
        out['uploaded'].record(up if up is not None else main)
        if ring is not None:
            ring.end(up if up is not None else main)
        return out

    def _neg_sample(self, pl, d, step, k, stream, which=None, out=None, rows=None):
        """K0 negative sampling (nar_model.py:265-276) of batch d with key `step` into the plan's sampler-output set k.  which = 0 / 1: the key
        is the .step / .step_next field of the runtime's step-scalar record (device) instead of the argument.  out, rows: other outputs than
        set k's, for the global rows [rows[0], rows[0] + rows[1]) instead of this call's (_whole_batch_neg_slots)."""
        rt, st, o = self.rt, self._dev_state, pl._samp[k] if out is None else out
        row_begin, row_count = (d['row_begin'], d['B']) if rows is None else rows
        if which is not None:
            check(rt.lib.cham_neg_sample_dev(ptr(d['aci']), d['Bg'], d['T'] + 1, ptr(st['buffer']), st['buffer'].numel(),
                                             rt.tf_random_seed, ptr(rt.scalars), which, row_begin, row_count, self.negative_samples,
                                             self.negative_sample_from_buffer, ptr(o['neg_ids']), ptr(o['neg_slot']), ptr(o['pool']),
                                             ptr(o['canon']), ptr(o['meta']), ptr(pl.sampler_ws), pl.ws_bytes, stream), "cham_neg_sample_dev")
            return
        check(rt.lib.cham_neg_sample(ptr(d['aci']), d['Bg'], d['T'] + 1, ptr(st['buffer']), st['buffer'].numel(),
                                     rt.tf_random_seed, step, row_begin, row_count, self.negative_samples,
                                     self.negative_sample_from_buffer, ptr(o['neg_ids']), ptr(o['neg_slot']), ptr(o['pool']),
                                     ptr(o['canon']), ptr(o['meta']), ptr(pl.sampler_ws), pl.ws_bytes, stream), "cham_neg_sample")

    def _whole_batch_neg_slots(self, pl, d, step, stream, which=None):
        """Pool slots [Bg, T, N] of the negatives of EVERY row of the global batch, for a call that is a row shard of it (the first batch's
        statistics, _forward): the sampler once more with rows [0, Bg) into scratch outputs (it is keyed by the global row, so these are the
        negatives each shard draws for its own rows).  Once per training run: 12 bytes per global negative of scratch (ids + slots; about
        200 MB at 4096 sessions x 20 x 200), freed on return of the step.  The draw rebuilds the pool in the plan's sampler workspace: that
        workspace is sized by the global batch and nothing reads it after a sampler call has returned its outputs, so this call's own
        negatives (drawn before, on the same stream) are not affected."""
        Bg, T, N, dev = d['Bg'], d['T'], self.negative_samples, self.rt.device
        out = dict(neg_ids=torch.empty(Bg, T, N, dtype=torch.int64, device=dev), neg_slot=torch.empty(Bg, T, N, dtype=torch.int32, device=dev),
                   pool=torch.empty(pl.pmax, dtype=torch.int64, device=dev), canon=torch.empty(pl.pmax, dtype=torch.int32, device=dev),
                   meta=torch.empty(4, dtype=torch.int32, device=dev))
        self._neg_sample(pl, d, step, pl._samp_cur, stream, which=which, out=out, rows=(0, Bg))
        return out['neg_slot']

    def presample(self, d):
        """Draw the negatives of the NEXT training step now.  Sampling depends on the recent-clicks state and the batch's ids,
        not on the weights, so it can run on the device state's stream right behind the state update of the current batch,
        while the current step's backward is still executing (0.3 ms of latency-bound kernels off the head of every step).
        ``d`` = the uploaded next batch; forward() picks the result up when the batch and the sampler key match."""
        rt, state = self.rt, self.articles_recent_pop_norm
        if not (rt.presample and self.is_training and getattr(state, 'is_device', False) and state.stream is not None
                and self._dev_state is not None and self._dev_state.get('device')):
            return False
        pl = rt.plan(d['B'], d['T'], self.negative_samples, self.negative_sample_from_buffer, d['Bg'])
        k, step = 1 - pl._samp_cur, rt.global_step
        if not rt.capturing:      # (events recorded outside a capture are not waited for inside one: the replay is stream-ordered behind them)
            state.stream.wait_event(pl.created)
            if d.get('uploaded') is not None:
                state.stream.wait_event(d['uploaded'])
            d['aci'].record_stream(state.stream)
        with torch.cuda.stream(state.stream):      # in order behind the state update it must see
            # (captured step: the key is the record's .step_next - this call runs behind the step whose key is .step)
            self._neg_sample(pl, d, step, k, state.stream.cuda_stream, which=1 if rt.capturing else None)
            ev = torch.cuda.Event()
            ev.record()
        d['_presampled'] = (pl, k, step, ev)
        return True

    # ------------------------------------------------------------------ forward
    def forward(self, d, step=None):
        depth = _roctx.depth()
        try:
            return self._forward(d, step)
        finally:
            _roctx.unwind(depth)          # (an error raised mid-step leaves no stage range open - ADVICE r05)

    def _forward(self, d, step):
        rt, lib, L = self.rt, self.rt.lib, self.rt.layout
        st = self._dev_state
        if st is None:
            raise RuntimeError("feed_state() must be called before every step (ItemsStateUpdaterHook.before_run)")
        B, T, N = d['B'], d['T'], self.negative_samples
        pl = rt.plan(B, T, N, self.negative_sample_from_buffer, d['Bg'])
        self._plan, self._d = pl, d
        check(lib.cham_set_log_bases(self.elapsed_days_smooth_log_base, self.popularity_smooth_log_base), "cham_set_log_bases")
        if d.get('uploaded') is not None:
            torch.cuda.current_stream().wait_event(d['uploaded'])
        s = _stream()
        # weight shadows (planes of W2 / W2^T, the row-norm bound of Ws1, bf16 shadows): four small launches that depend on the weights only -
        # on the side lane (idle at the head of a step) behind the previous step's Adam, beside this lane's feature kernels (round 4: the
        # head of a step is ~35 latency-bound launches in a row on one lane)
        shadows_ev = None
        if rt.overlap and rt.shadows_stale():
            rt.side_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(rt.side_stream):
                rt.refresh_shadows()
                shadows_ev = torch.cuda.Event()
                shadows_ev.record()
        # BT = rows of the row-wise stages = the P valid positions (all B*T when nothing is padded); BTf = the [B, T] layout
        pos, BT, BTf, NC, pmax = d['pos'], d['P'], pl.BT, pl.NC, pl.pmax
        Rc = BT * NC
        pl.pos, pl.P, pl.PC = pos, BT, Rc
        C, Hp = L.C, L.Hp
        NGH = L.NG * L.Hp
        if step is None:
            step = rt.global_step if self.is_training else self.eval_step_key(rt.global_step, self._eval_iter)
        p = rt.p
        # K0 negative sampling (nar_model.py:265-276) - unless presample() already drew this batch's negatives for this key
        _roctx.push("K0 negative sampling")
        ps = d.pop('_presampled', None)
        dsc = rt.dev_scalars          # per-step launch scalars from the device record (NARRuntime.__init__)
        if dsc:
            rt.set_step_scalars(step, d['max_ts'], d['sum_mask'], fields=3, stream=s)
        if ps is not None and ps[0] is pl and ps[2] == step and st.get('device'):
            pl.use_sampler_set(ps[1])
            if ps[3] is not None:
                torch.cuda.current_stream().wait_event(ps[3])
        else:
            self._neg_sample(pl, d, step, pl._samp_cur, s, which=0 if dsc else None)
        if rt.dp_mode in ('sparse', 'sparse_rs') and getattr(rt, 'dp_active', rt.dp_world > 1):
            # item rows this step can touch on ANY rank (parallel.py, mode "sparse"): GLOBAL clicked ids + candidate pool + pad item,
            # as int32 row indices in a buffer of the plan (nothing is allocated or freed around the collective)
            n1 = d['aci'].numel()
            if pl.touched is None or pl.touched.numel() < n1 + pmax + 1:
                pl.touched = torch.zeros(n1 + pmax + 1, dtype=torch.int32, device=rt.device)
            pl.touched[:n1].copy_(d['aci'].reshape(-1))
            pl.touched[n1:n1 + pmax].copy_(pl.pool)
            pl.touched[n1 + pmax:n1 + pmax + 1].zero_()
            rt.dp_touched = pl.touched[:n1 + pmax + 1]
        neg_ids, neg_slot = pl.neg_ids, pl.neg_slot
        if pos is not None:
            neg_ids, neg_slot = pl.neg_ids_c, pl.neg_slot_c
            check(lib.cham_rows_gather(ptr(pl.neg_ids), ptr(pos), BT, 2 * N, ptr(neg_ids), s), "cham_rows_gather")
            check(lib.cham_rows_gather(ptr(pl.neg_slot), ptr(pos), BT, N, ptr(neg_slot), s), "cham_rows_gather")
        pl.cur_neg_ids, pl.cur_neg_slot = neg_ids, neg_slot
        # a training-mode forward on this plan that was NOT followed by backward() (a loss-only call, an exception in between) leaves the
        # side lane's row grouping un-awaited: it reads ids_all and writes perm / seg - wait for it before rewriting ids_all
        if pl.grouped_ev is not None:
            torch.cuda.current_stream().wait_event(pl.grouped_ev)
        # K1 item row set = [clicked ; positives ; pool slots ; pad item 0]
        _roctx.pop(); _roctx.push("K1 features (gather, normalise, scale / center)")
        # (one launch - round 5: eight copy / fill launches before - also seq_len and the position mask of the stages below)
        fr = rt.features
        fr.step_ints(pl, d, s)
        pl.grouped_ev = None
        if self.is_training:      # rows of equal id made contiguous: the embedding-gradient sums of the backward pass (depends on ids only)
            if rt.overlap:        # ~10 launches nobody needs before the end of the backward: on the side lane, behind the id copies above
                e_ids = torch.cuda.Event()
                e_ids.record()
                rt.side_stream.wait_event(e_ids)
                with torch.cuda.stream(rt.side_stream):
                    fr.group_rows(pl, _stream())
                    pl.grouped_ev = torch.cuda.Event()
                    pl.grouped_ev.record()
            else:
                fr.group_rows(pl, s)
        fr.dynamic_raw(pl, st, s)
        if st['n_last'] == 0 and (d['Bg'] > B or d['row_begin'] > 0):
            # the very first batch, and this call is a row shard of it: the statistics of the GLOBAL batch's rows, as the whole-batch step
            # takes them - the negatives of every global row drawn once more (the sampler is keyed by the global row) for their multiplicities
            fr.norm_stats_first_batch_of_shard(pl, d, st, self._whole_batch_neg_slots(pl, d, step, s, which=0 if dsc else None), s)
        else:
            fr.norm_stats(pl, d, st, s)
        fr.assemble(pl, d, s)
        if shadows_ev is not None:
            torch.cuda.current_stream().wait_event(shadows_ev)
        else:
            rt.refresh_shadows()
        _roctx.pop(); _roctx.push("K2 PreCAR + CAR, K3 recurrent branch (side lane)")
        drop = self.is_training and self.keep_prob < 1.0
        # (full batches only: with ragged sessions the side lane's recurrent chain IS the critical path and the two launches are better
        # off on the main lane - G1-like lengths 114-115 k vs 111-112 k sessions/s, profiles/r05_notes.md)
        head_split = rt.head_split and rt.overlap and BT * NC > rt.w2_main_rows
        # the form of the PreCAR input layer (nar/input_rows.py), decided here, once: factorised U (per click) + V (per unique item row), or, with
        # dropout, the dense rows under this step's masks - its forward() leaves the clicked-input rows' Z1 too
        pre = pl.precar = DenseInput(rt, Dropout(rt, self.keep_prob, step, T, d['row_begin'])) if drop else rt.precar
        dropout = pre.dropout
        pre.forward(pl, s)
        # PreCAR combine + CAR layer 2 on the clicked-input rows first: they feed the recurrent branch ...
        if not head_split:
            pre.clicked_z1(pl, s)
            rt.gemm(pl.Z1, p('W2'), pl.Z2, BT, C, C, C, C, C, bias=p('b2'), act=ACT_TANH)
        rt.fork()
        with rt.side():   # ... which is latency-bound (one workgroup per 32 sessions) and overlaps with ...
            if head_split:      # (round 5) ... at the head of THIS lane: only the recurrent branch reads the clicked rows' CAR output
                pre.clicked_z1(pl, _stream())
                rt.gemm(pl.Z1, p('W2'), pl.Z2, BT, C, C, C, C, C, bias=p('b2'), act=ACT_TANH)
            x, ldx, K = pl.Z2, C, C
            if pos is not None:          # clicked rows back into the [B, T] layout of the recurrent stack (zeros at padded steps)
                pl.Z2f.zero_()
                check(lib.cham_rows_scatter(ptr(pl.Z2), ptr(pos), BT, C, ptr(pl.Z2f), _stream()), "cham_rows_scatter")
                x = pl.Z2f
            rnn = pl.rnn = rt.rnn_path(pl)      # the launch path of the time loops (nar/recurrent.py), decided here, once
            for l in range(L.L):
                rt.gemm(x, p('rnn%d/Wx' % l), pl.xproj[l], BTf, NGH, K, ldx, NGH, NGH, bias=p('rnn%d/b' % l))
                rnn.forward(pl, l, _stream())
                x, ldx, K = pl.rnn_out[l], Hp, Hp
                if drop:     # DropoutWrapper(output_keep_prob), nar_model.py:1331: the layer's OUTPUT is dropped, its state is not
                    dropout.apply(pl.rnn_out[l], pl.rnn_drop[l], BTf, Hp, Hp, SITE_RNN_OUT + l, SITE_RNN_OUT + l, 1, None)
                    x = pl.rnn_drop[l]
            if pos is not None:
                check(lib.cham_rows_gather(ptr(x), ptr(pos), BT, Hp, ptr(pl.rnn_c), _stream()), "cham_rows_gather")
                x = pl.rnn_c
            rt.gemm(x, p('Wf1'), pl.FC1, BT, 512, Hp, Hp, 512, 512, bias=p('bf1'), act=ACT_LEAKY)
            fc1 = pl.FC1
            if drop:         # nar_model.py:418
                dropout.apply(pl.FC1, pl.FC1d, BT, 512, 512, SITE_FC1, SITE_FC1, 1, pos)
                fc1 = pl.FC1d
            rt.gemm(fc1, p('Wf2'), pl.pred, BT, C, 512, 512, C, C, bias=p('bf2'), act=ACT_TANH)
        # ... the candidate rows: PreCAR combine (HBM-bound) + the dominant GEMM, CAR layer 2 on the B*T*(1+N) rows
        # in the arithmetic of this step (nar/candidate_rows.py), decided here, once: the configured arm, the fp32 rows where planes cannot be used
        arm = pl.arm = rt.step_arm(planes=not drop and Rc > 0)
        arm.z1(pl, s, pre if drop else None)
        arm.car_fwd(pl)
        rt.join()
        # scorer: (cand (.) pred) -> 128 -> 64 -> 32 -> 1, softmax(/tau), masked NLL
        _roctx.pop(); _roctx.push("K5 scorer, softmax, loss")
        if rt.cosine:      # cos(pred, candidate row), then the same kernel: its last-layer dot over (cos, 0, 0, 0) x (1, 0, 0, 0) returns cos (fp32 in every arm)
            arm.cosine_fwd(pl, s)
            softmax_fwd, rankloss_fwd, S3, K3, w4, b4 = 'cham_score_softmax_fwd', 'cham_score_rankloss_fwd', pl.cosq, 4, rt.cos_w4, rt.cos_b4
        else:
            arm.scorer_fwd(pl, s)
            softmax_fwd, rankloss_fwd, S3, K3, w4, b4 = arm.softmax_fwd, arm.rankloss_fwd, pl.S3, 32, p('Ws4'), p('bs4')
        loss_args = (ptr(S3), K3, ptr(w4), ptr(b4), BT, N, float(self.softmax_temperature), ptr(pl.mask), ptr(pl.logits), ptr(pl.probs),
                     ptr(pl.nll), self.novelty_reg_factor, ptr(neg_ids), ptr(st['pop_norm']), ptr(pl.nov_aux))
        if self.loss_function == 'softmax':
            check(getattr(lib, softmax_fwd)(*loss_args, s), "cham_score_softmax_fwd")
        else:        # a pairwise ranking loss: the same outputs + the per-click record of its backward
            check(getattr(lib, rankloss_fwd)(*loss_args, LOSS_FUNCTIONS.index(self.loss_function), self.bpr_max_reg, ptr(pl.ensure_rank_aux()), s),
                  "cham_score_rankloss_fwd")
        if self.diversity_reg_factor > 0.0:      # + factor * p^T S p into nll, ahead of the loss record below (TRAIN and EVAL)
            sp, e = pl.ensure_diversity()
            check(lib.cham_diversity_fwd(ptr(pl.probs), ptr(d['ln_rows']), ptr(neg_ids), ptr(pl.mask), BT, N, ptr(rt.ace), rt.ace.stride(0),
                                         rt.ace.shape[1], rt.ace.shape[0], self.diversity_reg_factor, ptr(sp), ptr(e), ptr(pl.nll), s),
                  "cham_diversity_fwd")
        def loss_kernels(s):
            check(lib.cham_sumsq_partial(ptr(rt.flat), L.n_reg, ptr(rt.sumsq), s), "cham_sumsq_partial")
            fn, sum_mask = step_scalar(rt, 'cham_loss_finalize', d['sum_mask'])      # (from the step-scalar record, or by value)
            check(getattr(lib, fn)(ptr(pl.nll), BT, sum_mask, ptr(rt.sumsq), float(self.reg_weight_decay), ptr(pl.loss), s), fn)
        if getattr(self, '_defer_loss', False) and rt.overlap and rt.loss_side:
            # inside a training step (train_step: forward -> backward -> Adam) the L2 term and the loss record leave the main lane - nothing in
            # the backward pass reads them, they sat between the softmax and its backward (round 6); the backward's final join covers them
            e_nll = torch.cuda.Event(); e_nll.record()
            rt.side_stream.wait_event(e_nll)
            with torch.cuda.stream(rt.side_stream):
                loss_kernels(_stream())
        else:
            loss_kernels(s)
        _roctx.pop()
        self.total_loss = pl.loss            # device [total, xe, reg]; xe is this rank's share under data parallel
        if not self.is_training and st.get('device'):
            self.articles_recent_pop_norm.note_consumed(d['aci'])      # last read of the state in an EVAL step
        return pl

    # ------------------------------------------------------------------ backward (hand-derived; nar_model.py:718)
    def backward(self):
        """Hand-derived backward in two stream lanes.  MAIN carries the critical dgrad chain (softmax -> scorer -> CAR layer 2 ->
        PreCAR combine -> features); SIDE carries everything that only produces weight gradients - wgrad GEMMs,
        bias column sums - plus the session-FC / recurrent chain and the clicked-row CAR dgrad, so the HBM-bound elementwise
        kernels of one lane run beside the MFMA-bound GEMMs of the other (DESIGN.md "Step schedule").  Every cross-lane
        dependency is an explicit event; with overlap off the same program order runs on one stream."""
        rt, lib, L = self.rt, self.rt.lib, self.rt.layout
        pl, d = self._plan, self._d
        # the log bases are host-side values of the library read when a kernel is launched: set again here, another model of this process
        # (different bases) may have run its forward pass since ours
        check(lib.cham_set_log_bases(self.elapsed_days_smooth_log_base, self.popularity_smooth_log_base), "cham_set_log_bases")
        s = _stream()
        N = pl.N
        pos, BT, BTf, NC = pl.pos, pl.P, pl.BT, pl.NC          # see forward(): BT = valid positions
        Rc = BT * NC
        neg_ids = pl.cur_neg_ids
        C, Hp = L.C, L.Hp
        cell, NGH = (1 if L.cell == 'gru' else 0), L.NG * L.Hp
        p, g = rt.p, rt.g
        main_stream, on = torch.cuda.current_stream(), rt.overlap
        pre = pl.precar                  # the form of the PreCAR input layer, as forward() chose it (nar/input_rows.py) ...
        dropout = pre.dropout            # ... and the step's masks, if it had any
        drop = dropout is not None
        arm = pl.arm                     # the arithmetic of the candidate rows, as forward() chose it (nar/candidate_rows.py)
        b16 = arm.b16

        def mark():                      # event on the current stream
            if not on:
                return None
            ev = torch.cuda.Event(); ev.record()
            return ev

        @contextlib.contextmanager
        def side(*events):               # run the block on the side lane after `events`
            if not on:
                yield
                return
            for ev in events:
                rt.side_stream.wait_event(ev)
            with torch.cuda.stream(rt.side_stream):
                yield

        def main_wait(ev):
            if on:
                main_stream.wait_event(ev)

        @contextlib.contextmanager
        def aux(*events):                # run the block on the third lane after `events`
            for ev in events:
                rt.aux_stream.wait_event(ev)
            with torch.cuda.stream(rt.aux_stream):
                yield
        e_auxdone = None

        e_start = mark()                 # side lane must not run ahead of the previous step's tail
        if on and rt.loss_side:          # (round 6) the zero fill of the embedding gradients on the side lane: their writers - the last kernels
            with side(e_start):          # of the main / third lane - come behind e_dZ1in, an event of this lane
                rt.grads[:L.emb_end].zero_()
        else:
            rt.grads[:L.emb_end].zero_()
            e_start = mark()
        # (sum(mask): from the step-scalar record written by this step's forward, or by value)
        cosine = rt.cosine               # the cosine head: ds is all its backward needs of these two kernels (dcosq is their scratch output)
        if cosine:
            softmax_bwd, rankloss_bwd, diversity_bwd, S3, K3, w4, dS3 = ('cham_score_softmax_bwd', 'cham_score_rankloss_bwd', 'cham_diversity_bwd',
                                                                         pl.cosq, 4, rt.cos_w4, pl.dcosq)
        else:
            softmax_bwd, rankloss_bwd, diversity_bwd, S3, K3, w4, dS3 = arm.softmax_bwd, arm.rankloss_bwd, arm.diversity_bwd, pl.S3, 32, p('Ws4'), pl.dS3
        loss_args = (ptr(S3), K3, ptr(w4), ptr(pl.probs), ptr(pl.mask), BT, N, float(self.softmax_temperature),
                     ptr(rt.scalars) if rt.dev_scalars else d['sum_mask'], ptr(pl.ds), ptr(dS3), self.novelty_reg_factor, ptr(neg_ids),
                     ptr(self._dev_state['pop_norm']), ptr(pl.logits), ptr(pl.nov_aux))
        if self.loss_function == 'softmax':
            check(getattr(lib, softmax_bwd + ('_dev' if rt.dev_scalars else ''))(*loss_args, s), "cham_score_softmax_bwd")
        else:
            check(getattr(lib, rankloss_bwd + ('_dev' if rt.dev_scalars else ''))(
                *loss_args, LOSS_FUNCTIONS.index(self.loss_function), self.bpr_max_reg, ptr(pl.rank_aux), s), "cham_score_rankloss_bwd")
        if self.diversity_reg_factor > 0.0:      # ds += the diversity term's logit gradient, dS3 again from it
            check(getattr(lib, diversity_bwd)(
                ptr(S3), K3, ptr(w4), ptr(pl.probs), ptr(pl.mask), BT, N, float(self.softmax_temperature),
                ptr(rt.scalars) if rt.dev_scalars else None, 0.0 if rt.dev_scalars else d['sum_mask'], ptr(pl.div_sp), ptr(pl.div_e),
                self.diversity_reg_factor, ptr(pl.ds), ptr(dS3), s), diversity_bwd)
        if self._dev_state.get('device'):
            self.articles_recent_pop_norm.note_consumed(d['aci'])      # last read of the state in a TRAIN step
        # scorer dgrad chain on this lane (three short GEMMs); the side lane takes the layer-1 weight gradient FIRST - 65 GFLOP of
        # matrix work that then runs beside the HBM-bound k_mulpred_bwd instead of beside the MFMA-bound CAR dgrad - and the small
        # (HBM-bound, split-K) weight / bias gradients of layers 2-4 after it
        if not cosine:
            arm.scorer_dgrad(pl, s)
        e_dS1 = mark()     # (starting the side lane only after the next GEMM, to pair its MFMA work with k_mulpred_bwd's HBM work,
        #                      measured 0.26 ms slower: 17.28-17.33 vs 17.01-17.07 ms, A/B in one gpurun call)
        # scorer layer-1 dgrad: through HBM here, unless this step's arm takes it in one kernel with the cand (.) pred backward below
        # (csrc/dm_fused.hip: dM never reaches HBM)
        if not cosine and not arm.fused_dz2(pl):
            arm.s1_dgrad(pl)
        # Side lane, "critical chain first": with short sessions the CAR GEMMs shrink and the
        # main lane ends up waiting for the clicked-row gradient that comes out of the side lane's FC -> recurrent -> CAR chain (0.4 ms
        # of a 3.4 ms step in the kernel trace of the G1-like bench leg).  So that chain is enqueued ahead of every weight / bias
        # gradient it does not need; those follow behind it.
        # (bf16 configuration with full-length sessions: 6.26 vs 6.17 ms - the deferred gradients then land beside the W2 wgrad - so there it
        # is used for compacted, i.e. ragged, batches only: 2.23 vs 2.35 ms; fp32: 13.0 = 13.0 ms full-length, 2.95 vs 3.11 ms G1-like lengths)
        crit_first = on and (not b16 or pos is not None)
        w2_main = bool(on and arm.planes and 0 < Rc <= rt.w2_main_rows)
        # third lane for the small weight gradients (full batches of the default / six-plane fp32 arithmetic, one recurrent layer of the
        # UGRNN kind: with more layers the per-layer gradients read a buffer the next layer's backward overwrites)
        use_aux = bool(on and rt.wgrad_aux and arm.planes and not w2_main and L.L == 1 and cell == 0 and not L.rnn_stepwise and not drop)
        if cosine:      # no scorer weights: one HBM-bound kernel (+ the bound record of the two-plane arm) takes ds to the gradient at the CAR tanh and dpred
            arm.cosine_bwd(pl, s)
        else:
            with side(e_start, e_dS1):
                arm.s1_wgrad(pl)
                if not crit_first:
                    arm.small_wgrads(pl)
            arm.dz2(pl, s)
        e_dZ2c = mark()              # dZ2c final + dpred
        # The candidate-row dgrad of CAR layer 2 on the main lane (needs dZ2c only): the largest GEMM of the backward, ENQUEUED BEFORE the
        # side lane's long launch sequence below - in the bf16 configuration the GPU keeps up with the host, and the ~25 launches of the
        # side block (0.5-0.8 ms of host time) left this lane idle for that long (kernel-trace timeline, profiles/r02_notes.md);
        # NT layout on the 256x256 tile.
        arm.car_dgrad(pl)
        e_cdgrad = mark()
        e_w2main = None
        if w2_main:      # candidate rows' share of the W2 weight gradient here, in the main lane's wait for the side lane's recurrent chain
            arm.w2_wgrad_cand(pl, 0)
            e_w2main = mark()
        # session FCs + recurrent layers (latency-bound: one workgroup per 32 sessions) ...
        last = L.L - 1
        deferred_w2 = None
        with side(e_dZ2c):
            ss = _stream()
            rnn = pl.rnn                 # the launch path of the time loops, as forward() chose it (nar/recurrent.py)
            rnn_y = (lambda l: pl.rnn_drop[l]) if drop else (lambda l: pl.rnn_out[l])     # what the next layer / FC1 consumed

            def fc_wgrads():
                rt.gemm(pl.FC1d if drop else pl.FC1, pl.dpred, g('Wf2'), 512, C, BT, 512, C, C, transA=1, splits=0)
                rt.colsum(pl.dpred, C, BT, C, g('bf2'))
                rt.gemm(pl.rnn_c if pos is not None else rnn_y(last), pl.dFC1, g('Wf1'), Hp, 512, BT, Hp, 512, 512, transA=1, splits=0)
                rt.colsum(pl.dFC1, 512, BT, 512, g('bf1'))
                if crit_first and not cosine:
                    arm.small_wgrads(pl)
                if rt.dp_early_bucket is not None and not self._accumulating:
                    rt.dp_early_bucket(rt.grads)     # data parallel: [Wf1 .. Ws4] gradients are final - their all-reduce starts now
            rt.gemm(pl.dpred, p('Wf2'), pl.dFC1, BT, 512, C, C, C, 512, transB=1, dref=pl.FC1, ldr=512, dact=ACT_LEAKY)
            if drop:                     # (mask and leaky' are both element-wise factors: the order does not matter)
                dropout.apply(pl.dFC1, pl.dFC1, BT, 512, 512, SITE_FC1, SITE_FC1, 1, pos)
            if not crit_first:
                fc_wgrads()
            if pos is not None:          # d rnn_out back into the [B, T] layout (zero at padded steps)
                rt.gemm(pl.dFC1, p('Wf1'), pl.drnn_c, BT, Hp, 512, 512, 512, Hp, transB=1)
                pl.drnn.zero_()
                check(lib.cham_rows_scatter(ptr(pl.drnn_c), ptr(pos), BT, Hp, ptr(pl.drnn), ss), "cham_rows_scatter")
            else:
                rt.gemm(pl.dFC1, p('Wf1'), pl.drnn, BT, Hp, 512, 512, 512, Hp, transB=1)
            if drop:
                dropout.apply(pl.drnn, pl.drnn, BTf, Hp, Hp, SITE_RNN_OUT + last, SITE_RNN_OUT + last, 1, None)
            for l in range(last, -1, -1):
                rnn.backward(pl, l, ss)
                if l == 0:   # -> gradient w.r.t. the CAR tanh pre-activation of the clicked-input rows (main lane waits for it)
                    dxp = pl.dxproj
                    if pos is not None:
                        dxp = pl.dxproj_c
                        check(lib.cham_rows_gather(ptr(pl.dxproj), ptr(pos), BT, NGH, ptr(dxp), ss), "cham_rows_gather")
                    rt.gemm(dxp, p('rnn0/Wx'), pl.dZ2, BT, C, NGH, NGH, NGH, C, transB=1, dref=pl.Z2, ldr=C, dact=ACT_TANH)
                    # CAR layer-2 dgrad of the clicked rows right here (0.1 ms; behind the W2 wgrad it would starve: that kernel's
                    # 256 workgroups fill every CU's register file for 4 ms) - the main lane's PreCAR backward waits for it ...
                    rt.gemm(pl.dZ2, p('W2'), pl.dZ1, BT, C, C, C, C, C, transB=1, dref=pl.Z1, ldr=C, dact=ACT_LEAKY)
                    e_dZ1in = mark()
                    if crit_first and not use_aux:
                        fc_wgrads()
                    if use_aux:
                        # (round 5) the small weight / bias gradients leave this lane for the third one - every producer they read is
                        # final at e_dZ1in - and the W2 weight gradient (candidate rows from the planes, TN split-K, + the clicked rows)
                        # starts the moment the main lane's CAR dgrad has finished, not behind ~1 ms of small launches
                        with aux(e_dZ1in):
                            if crit_first:
                                fc_wgrads()
                            arm.b2_grad(pl)
                            rt.gemm(pl.Z2, dxp, g('rnn0/Wx'), C, NGH, BT, C, NGH, NGH, transA=1, splits=0)
                            rnn.wgrads(pl, 0)
                            e_auxdone = mark()
                        rt.side_stream.wait_event(e_cdgrad)
                        arm.w2_wgrad(pl, rt.p3_w2_splits)
                        continue
                    elif arm.planes:
                        # ... and the CAR layer-2 weight gradient: the candidate rows from their planes (TN, split-K), the clicked-input
                        # rows (fp32) added by the on-the-fly kernel; b2 from the per-position partial sums of k_mulpred_bwd_p3
                        def w2_grads():
                            if w2_main:       # (the candidate rows' share was written by the main lane: behind e_cdgrad it is complete)
                                rt.side_stream.wait_event(e_w2main)
                            elif on:
                                rt.side_stream.wait_event(e_cdgrad)
                            arm.w2_wgrad(pl, rt.p3_w2_splits, cand=not w2_main)
                        arm.b2_grad(pl)
                        if on and not w2_main:
                            # the plane weight gradient waits for the main lane's CAR dgrad (two one-workgroup-per-CU matrix kernels only
                            # time-slice the chip): everything this lane still has to do that does NOT wait - bias sums, the recurrent and
                            # input-projection weight gradients - goes first and runs under that dgrad; the big GEMM is the lane's last work
                            deferred_w2 = w2_grads
                        else:
                            w2_grads()
                    else:
                        # ... and the CAR layer-2 weight gradient (fp32: over ALL rows, the second-largest GEMM of the step - behind the CAR
                        # dgrad; bf16-resident: the candidate rows (TN) + the clicked-input rows, beside it)
                        if on and not b16:
                            rt.side_stream.wait_event(e_cdgrad)
                        arm.w2_wgrad(pl)
                        arm.b2_grad(pl)
                    rt.gemm(pl.Z2, dxp, g('rnn0/Wx'), C, NGH, BT, C, NGH, NGH, transA=1, splits=0)
                else:
                    rt.gemm(pl.dxproj, p('rnn%d/Wx' % l), pl.drnn, BTf, Hp, NGH, NGH, NGH, Hp, transB=1)
                    rt.gemm(rnn_y(l - 1), pl.dxproj, g('rnn%d/Wx' % l), Hp, NGH, BTf, Hp, NGH, NGH, transA=1, splits=0)
                    if drop:
                        dropout.apply(pl.drnn, pl.drnn, BTf, Hp, Hp, SITE_RNN_OUT + l - 1, SITE_RNN_OUT + l - 1, 1, None)
                rnn.wgrads(pl, l)
            if deferred_w2 is not None:
                deferred_w2()
        if on:
            main_wait(e_dZ1in)
        # PreCAR backward beside the W2 wgrad of the side lane: dZ1 -> the gradients at the layer's two inputs (combine scatter; dense form:
        # + its weight gradient), then per half the W1 weight gradient, d(features), scale / center and the embedding tables (nar/input_rows.py)
        st = _stream()
        pre.backward(pl, rt.gemm_ws, st)
        # Round 6: the two halves are independent once dU / dV exist, and they are the SERIAL tail of the step - ~25 latency-bound launches
        # behind the W2 weight gradient with the chip otherwise idle.  The user-context half goes to the third lane, the item half
        # stays here (CHAM_TAIL_SPLIT=0: both on this lane, the order of rounds 1-5).  Same kernels, same arguments: same results.
        if on and rt.tail_split and not drop and st == main_stream.cuda_stream:
            e_duv = mark()
            with aux(e_duv):
                pre.ctx_chain(pl)
                e_ctx = mark()
            pre.item_chain(pl)
            main_stream.wait_event(e_ctx)
        else:
            pre.ctx_chain(pl)
            pre.item_chain(pl)
        rt.join()
        if e_auxdone is not None:
            main_stream.wait_event(e_auxdone)

    def adam_lr_t(self, t):
        """tf.train.AdamOptimizer's bias-corrected learning rate of optimizer step t (>= 1)."""
        return self.lr * math.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t)

    def apply_gradients(self):
        """tf.train.AdamOptimizer(lr, 0.9, 0.999, 1e-8).apply_gradients (nar_model.py:708-722) + the dense L2 term."""
        rt, L = self.rt, self.rt.layout
        rt.global_step += 1           # (also invalidates the bf16 weight shadows: NARRuntime.refresh_shadows keys on it)
        if not rt.capturing and getattr(self, '_plan', None) is not None:
            self._plan.eager_steps = getattr(self._plan, 'eager_steps', 0) + 1      # (GraphedTrainStep captures warm shapes only)
        t = rt.global_step
        lr_t = self.adam_lr_t(t)
        if rt.dev_scalars:
            rt.set_step_scalars(lr_t=lr_t, fields=4)

        def adam(a, b, grads, g_off):       # Adam on the parameter range [a, b); grads[g_off + i] pairs with flat[a + i]
            n_reg = min(max(L.n_reg - a, 0), b - a)
            if rt.dev_scalars:      # lr_t from the step-scalar record
                check(rt.lib.cham_adam_tf_dev(rt.flat.data_ptr() + 4 * a, grads.data_ptr() + 4 * g_off, rt.m.data_ptr() + 4 * a,
                                              rt.v.data_ptr() + 4 * a, b - a, n_reg, float(self.reg_weight_decay), ptr(rt.scalars),
                                              0.9, 0.999, 1e-8, _stream()), "cham_adam_tf_dev")
                return
            check(rt.lib.cham_adam_tf(rt.flat.data_ptr() + 4 * a, grads.data_ptr() + 4 * g_off, rt.m.data_ptr() + 4 * a,
                                      rt.v.data_ptr() + 4 * a, b - a, n_reg, float(self.reg_weight_decay), float(lr_t),
                                      0.9, 0.999, 1e-8, _stream()), "cham_adam_tf")

        if rt.dp_sharded is not None:       # reduce-scatter -> Adam on this rank's slice -> all-gather (parallel.py)
            rt.dp_sharded(rt.grads, rt.flat, adam)
            return
        if rt.dp_allreduce is not None:
            rt.dp_allreduce(rt.grads)
        adam(0, L.total, rt.grads, 0)

    def train_step_microbatched(self, features, labels, micro_sessions, global_features=None, global_labels=None, row_begin=0):
        """One optimizer step over the batch processed as row shards of ``micro_sessions`` sessions (activations of the
        B*T*(1+N) candidate rows bounded by the shard; BASELINE config 5 = 4096 sessions x 200 negatives).  Every shard sees
        the GLOBAL ids (pool, max timestamp, sum(mask), sampler keyed by the global row; on the very first batch also the normalisation
        statistics of the global batch's rows), gradients accumulate, ONE Adam.
        Same result as train_step on the whole batch up to fp32 summation order (tests/test_shard_paths_gpu.py: every model variant,
        warm and empty recent-clicks state; bf16: up to the bf16 rounding of the per-shard dU / dV sums)."""
        from .parallel import slice_batch
        rt = self.rt
        gf = features if global_features is None else global_features
        gl = labels if global_labels is None else global_labels
        n = np.asarray(features['item_clicked']).shape[0]
        if getattr(rt, 'grads_acc', None) is None:
            rt.grads_acc = torch.empty_like(rt.grads)
            rt.loss_acc = torch.zeros(3, dtype=torch.float32, device=rt.device)
        self._accumulating = True
        for k, b in enumerate(range(0, n, micro_sessions)):
            e = min(n, b + micro_sessions)
            f, l = slice_batch(features, labels, b, e)
            self.forward(self.upload_batch(f, l, gf, gl, row_begin=row_begin + b))
            self.backward()
            check(rt.lib.cham_accumulate(ptr(rt.grads_acc), ptr(rt.grads), rt.layout.total, int(k == 0), _stream()), "cham_accumulate")
            check(rt.lib.cham_loss_accumulate(ptr(rt.loss_acc), ptr(self._plan.loss), int(k == 0), _stream()), "cham_loss_accumulate")
        self._accumulating = False
        rt.grads, rt.grads_acc = rt.grads_acc, rt.grads          # Adam (and the data-parallel all-reduce) read rt.grads
        self.apply_gradients()
        self.total_loss = rt.loss_acc
        return self.total_loss

    def stage_next(self, dataset):
        """Training-loop hook (estimator.Estimator.train): upload the batch AFTER the current one and draw its negatives now
        (presample), so that neither the H2D copies nor the sampler sit at the head of the next step."""
        self._staged = None
        state = self.articles_recent_pop_norm
        if not (self.rt.presample and self.is_training and getattr(state, 'is_device', False)):
            return
        nxt = dataset.peek()
        if nxt is None:
            return
        d = self.upload_current(nxt[0], nxt[1])
        if not d.get('empty'):
            self.presample(d)
        self._staged = (nxt[0]['item_clicked'], d)

    def train_step(self, device_batch=None):
        """One optimizer step on the current batch (the reference's ``session.run(model.train)``)."""
        d = device_batch
        if d is None:
            staged, self._staged = getattr(self, '_staged', None), None
            if staged is not None and staged[0] is self.inputs['item_clicked']:        # the very arrays stage_next() uploaded
                d = staged[1]
            else:
                d = self.upload_current(self.inputs, self.labels)
        if d.get('empty'):
            return self._empty_shard_train_step(d)
        with _roctx.range_("NAR step: forward (K0 sampler .. loss)"):        # (CHAM_ROCTX=1: roctx ranges for rocprofv3 --marker-trace)
            self._defer_loss = True          # the loss record may finish on the side lane: backward() joins it
            try:
                pl = self.forward(d)
            finally:
                self._defer_loss = False
        if self.eval_cold_start:       # nar_model.py:520: the ranked candidates are also needed while TRAINING for the cold-start analysis
            self._rank_items(pl, d)
        with _roctx.range_("NAR step: backward"):
            self.backward()
        with _roctx.range_("NAR step: exchange + L2 + TF-Adam"):
            self.apply_gradients()
        return self.total_loss

    def _empty_shard_train_step(self, d):
        """The optimizer step of a data-parallel rank whose row shard of the global batch is EMPTY (fewer sessions than ranks: the last batch
        of a file chunk): no forward, no backward and no kernel over zero rows - a zero gradient buffer and a zero loss share, then the same
        exchange (the early bucket included: every rank issues the same collectives in the same order) and the same Adam as every other
        rank.  ``d`` carries the global integers the replicated state update reads (parallel.DataParallelNAR.upload)."""
        rt = self.rt
        self._empty_shard_loss(d)
        rt.grads.zero_()
        if rt.dp_early_bucket is not None:
            rt.dp_early_bucket(rt.grads)
        with _roctx.range_("NAR step: exchange + L2 + TF-Adam"):
            self.apply_gradients()
        return self.total_loss

    def _empty_shard_loss(self, d):
        """Loss record [total, xe, reg] of a rank without rows of this batch: xe share 0, the L2 term of the (replicated) weights - the loss
        kernels of forward() over ONE zero row in place of the batch's, so that nothing is launched over zero rows."""
        rt, lib, s = self.rt, self.rt.lib, _stream()
        self._d = d
        if d.get('uploaded') is not None:      # (the replicated state update reads the global integers behind this stream)
            torch.cuda.current_stream().wait_event(d['uploaded'])
        if getattr(self, '_empty_loss', None) is None:
            self._empty_loss = (torch.zeros(1, dtype=torch.float32, device=rt.device), torch.zeros(3, dtype=torch.float32, device=rt.device))
        nll, loss = self._empty_loss
        check(lib.cham_sumsq_partial(ptr(rt.flat), rt.layout.n_reg, ptr(rt.sumsq), s), "cham_sumsq_partial")
        check(lib.cham_loss_finalize(ptr(nll), 1, float(d['sum_mask']), ptr(rt.sumsq), float(self.reg_weight_decay), ptr(loss), s),
              "cham_loss_finalize")
        self.total_loss = loss

    @staticmethod
    def eval_step_key(global_step, eval_iter):
        """Sampler key of the eval_iter-th batch of an evaluate() call (distinct from every training step's key)."""
        return (global_step + 1000003 * (eval_iter + 1)) & 0xFFFFFFFF

    def _rank_items(self, pl, d):
        """rank_items_by_predicted_prob (nar_model.py:777-794) of the last forward pass -> self._eval (what the hook fetches)."""
        rt, dev = self.rt, self.rt.device
        ev = self._eval
        if ev is None or ev['pred_ids'].shape != (pl.B, pl.T, pl.NC):
            ev = self._eval = dict(pred_ids=torch.zeros(pl.B, pl.T, pl.NC, dtype=torch.int64, device=dev),
                                   pred_probs=torch.zeros(pl.B, pl.T, pl.NC, dtype=torch.float32, device=dev),
                                   label_rank=torch.zeros(pl.B, pl.T, dtype=torch.int32, device=dev))
        if pl.pos is None:
            check(rt.lib.cham_rank_items(ptr(pl.probs), ptr(d['label_next']), ptr(pl.neg_ids), ptr(pl.mask), pl.BT, pl.N,
                                         ptr(ev['pred_ids']), ptr(ev['pred_probs']), ptr(ev['label_rank']), _stream()),
                  "cham_rank_items")
        else:       # rank the valid positions, then back into the [B, T, 1+N] layout (padded positions: ids 0, probs 0, rank -1)
            P, NC = pl.P, pl.NC
            c = ev.get('compact')
            if c is None or c[0].shape[0] < P:
                c = ev['compact'] = (torch.zeros(pl.BT, NC, dtype=torch.int64, device=dev), torch.zeros(pl.BT, NC, dtype=torch.float32, device=dev),
                                     torch.zeros(pl.BT, dtype=torch.int32, device=dev))
            check(rt.lib.cham_rank_items(ptr(pl.probs), ptr(d['ln_rows']), ptr(pl.cur_neg_ids), ptr(pl.mask), P, pl.N,
                                         ptr(c[0]), ptr(c[1]), ptr(c[2]), _stream()), "cham_rank_items")
            ev['pred_ids'].zero_(); ev['pred_probs'].zero_(); ev['label_rank'].fill_(-1)
            for src, dst, words in ((c[0], ev['pred_ids'], 2 * NC), (c[1], ev['pred_probs'], NC), (c[2], ev['label_rank'], 1)):
                check(rt.lib.cham_rows_scatter(ptr(src), ptr(pl.pos), P, words, ptr(dst), _stream()), "cham_rows_scatter")

    def evaluate_step(self, device_batch=None):
        """EVAL-mode ``session.run``: forward with the eval negative-sample counts (nar_trainer_gcom.py:240-242) +
        rank_items_by_predicted_prob (nar_model.py:777-794) [+ the beyond-accuracy metrics of the ranked lists]."""
        d = device_batch if device_batch is not None else self.upload_current(self.inputs, self.labels)
        if d.get('empty'):       # a data-parallel rank without rows of this batch: nothing to rank, nothing added to the records
            self._empty_shard_loss(d)
            self._eval_iter += 1
            return self.total_loss
        pl = self.forward(d)
        self._rank_items(pl, d)
        if self._rh is not None:
            self._rank_histogram(d)
        if self._ba is not None:
            self._beyond_accuracy(d)
        if self._fr is not None:      # after the step's own records: nothing above reads what this leaves
            from . import full_eval
            depth = _roctx.depth()
            try:
                full_eval.rank_step(self, pl, d)
            finally:
                _roctx.unwind(depth)
        self._eval_iter += 1
        return self.total_loss

    # ------------------------------------------------------------------ top-n prediction for open sessions (nar/predict.py, csrc/predict.hip)
    def upload_predict_batch(self, features):
        """Features batch as input_fn yields it (labels are not needed) -> the device batch predict_step takes."""
        from . import predict
        return predict.upload_predict_batch(self, features)

    def predict_step(self, device_batch=None, topn=10, candidates=None, chunk_candidates=None):
        """PREDICT-mode ``session.run``: for every session of the batch the `topn` (1..64) candidates most likely to be clicked next after its
        last click.  Candidates: `candidates` (item ids in [1, n_items); de-duplicated and sorted) or, by default, the
        distinct ids of the fed recent-clicks buffer; a session's own clicks are excluded.  The score of a candidate is the logit the EVAL
        forward gives it as a negative sample of the session's last click; probs = softmax(score / softmax_temperature) over the session's
        non-excluded candidates; order: score descending, smaller id first among equal scores; lists shorter than topn are padded with id 0,
        score -inf, prob 0 (a session without a click: all padding).  The candidates are scored in chunks of `chunk_candidates` (default: as
        many as keep the chunk's P_last (1 + Nc) candidate rows within those of the model's training plan).  Returns numpy arrays
        item_ids int64 / scores / probs float32 [B, topn] and K (candidates), Nc, chunks, P_last, candidates (the ids, ascending).
        Leaves the weights, the clicked-items state, global_step, the sampler keys and every evaluation record as they are."""
        from . import predict
        predict.check_top_n(topn)
        d = device_batch if device_batch is not None else self.upload_predict_batch(self.inputs)
        depth = _roctx.depth()
        try:
            return predict.predict_step(self, d, topn, candidates, chunk_candidates)
        finally:
            _roctx.unwind(depth)

    # ------------------------------------------------------------------ rank histogram of the evaluation (csrc/eval_metrics.hip)
    def enable_rank_histogram(self, topn, t_cap):
        """From now on every evaluate_step adds its clicks to a device record (cham_eval_rank_hist): hist int64 [t_cap, topn + 1] = valid
        clicks by (session position, rank of the positive; ranks >= topn in the last bin) and pop_sum fp64 [t_cap] = sum of the labels'
        recent normalised popularity by position.  HitRate@n, MRR@n, NDCG@n and HitRate-by-position follow from it
        (metrics.accuracy_from_rank_hist); integer, so the records of data-parallel ranks add up exactly.  Allocates and zeroes the record."""
        if not 1 <= topn <= 256:
            raise ValueError("the rank histogram needs 1 <= eval_metrics_top_n <= 256 (got %d)" % topn)
        if t_cap < 1:
            raise ValueError("t_cap must be >= 1")
        dev = self.rt.device
        self._rh = dict(topn=int(topn), t_cap=int(t_cap), hist=torch.zeros(int(t_cap), int(topn) + 1, dtype=torch.int64, device=dev),
                        pop_sum=torch.zeros(int(t_cap), dtype=torch.float64, device=dev))

    def reserve_rank_histogram(self, T):
        """Make room for batches of T click positions (a longer record, the counts so far kept).  Data-parallel ranks call this with the
        GLOBAL batch's T for every batch, the ranks without rows included: their records have one shape when they are summed."""
        rh = self._rh
        if T > rh['t_cap']:
            t_cap = max(int(T), 2 * rh['t_cap'])
            hist = torch.zeros(t_cap, rh['topn'] + 1, dtype=torch.int64, device=self.rt.device)
            pop_sum = torch.zeros(t_cap, dtype=torch.float64, device=self.rt.device)
            hist[:rh['t_cap']].copy_(rh['hist'])
            pop_sum[:rh['t_cap']].copy_(rh['pop_sum'])
            rh.update(t_cap=t_cap, hist=hist, pop_sum=pop_sum)

    def _rank_histogram(self, d):
        """This eval step's label ranks (after _rank_items: in a compacted batch after the scatter back into [B, T], padded positions -1)
        into the record, on the current stream; pop_norm = the array this batch was fed."""
        rh, ev, st = self._rh, self._eval, self._dev_state
        B, T = ev['label_rank'].shape
        if T > rh['t_cap']:
            raise ValueError("evaluation batch of %d click positions: the rank histogram was enabled for %d" % (T, rh['t_cap']))
        check(self.rt.lib.cham_eval_rank_hist(ptr(ev['label_rank']), ptr(d['label_next']), B, T, rh['topn'], ptr(st['pop_norm']),
                                              self.rt.n_items, ptr(rh['hist']), ptr(rh['pop_sum']), rh['t_cap'], _stream()),
              "cham_eval_rank_hist")
        if st.get('device'):
            self.articles_recent_pop_norm.note_consumed(d['aci'])      # pop_norm is read up to here: the state update waits for this

    def rank_histogram(self):
        """(hist [t_cap, topn + 1] int64, pop_sum [t_cap] float64) as numpy: what the evaluate_steps since enable_rank_histogram added."""
        return self._rh['hist'].cpu().numpy(), self._rh['pop_sum'].cpu().numpy()

    # ------------------------------------------------------------------ full-candidate evaluation (nar/full_eval.py, csrc/eval_full.hip)
    def enable_full_candidate_ranking(self, topn, t_cap, chunk_candidates=None, block_rows=None, return_scores=False):
        """From now on every evaluate_step also ranks each valid click's label against EVERY distinct id of the fed recent-clicks buffer
        (the session's own ids excluded) and adds the ranks to a second cham_eval_rank_hist record (bounds and
        shapes: enable_rank_histogram).  Allocates and zeroes the record.  Tests only: chunk_candidates / block_rows override the chunk
        width and the row-block size, return_scores keeps per click the [K] scores and the label's logit of every chunk."""
        from . import full_eval
        self._fr = full_eval.new_record(self, topn, t_cap, chunk_candidates, block_rows, return_scores)

    def reserve_full_candidate_ranking(self, T):
        """Make room for batches of T click positions (reserve_rank_histogram's rule: a longer record, the counts so far kept)."""
        from . import full_eval
        full_eval.check_session_length(T)
        fr = self._fr
        if T > fr['t_cap']:
            t_cap = max(int(T), 2 * fr['t_cap'])
            hist = torch.zeros(t_cap, fr['topn'] + 1, dtype=torch.int64, device=self.rt.device)
            pop_sum = torch.zeros(t_cap, dtype=torch.float64, device=self.rt.device)
            hist[:fr['t_cap']].copy_(fr['hist'])
            pop_sum[:fr['t_cap']].copy_(fr['pop_sum'])
            fr.update(t_cap=t_cap, hist=hist, pop_sum=pop_sum)

    def full_rank_histogram(self):
        """(hist [t_cap, topn + 1] int64, pop_sum [t_cap] float64) as numpy: the full-candidate ranks since enable_full_candidate_ranking."""
        return self._fr['hist'].cpu().numpy(), self._fr['pop_sum'].cpu().numpy()

    def full_rank_outputs(self):
        """The last evaluate_step's label_rank and competitors (int32 [B, T] numpy; rank -1 at padded positions) + K, Nc, blocks, chunks."""
        from . import full_eval
        return full_eval.outputs(self)

    # ------------------------------------------------------------------ beyond-accuracy evaluation metrics (csrc/eval_metrics.hip)
    def enable_beyond_accuracy_metrics(self, topn, relevance_positive_sample, relevance_negative_samples, recent_clicks_buffer):
        """From now on every evaluate_step also computes ESI-R, ESI-RR, EILD-R and EILD-RR of its ranked top-n lists and marks the
        coverage maps (cham_eval_beyond_accuracy).  The maps live on the device until the next call, which re-seeds them: the
        clicked map from ``recent_clicks_buffer`` - the device state's ring buffer (read in place) or a host array."""
        if not 2 <= topn <= 64:
            raise ValueError("the beyond-accuracy metrics need 2 <= eval_metrics_top_n <= 64 (got %d)" % topn)
        rt, lib, n_items = self.rt, self.rt.lib, self.rt.n_items
        ba = self._ba_buffers
        if ba is None:
            ba = self._ba_buffers = dict(
                rec=torch.zeros(n_items, dtype=torch.uint8, device=rt.device), clk=torch.zeros(n_items, dtype=torch.uint8, device=rt.device),
                ws=torch.empty(lib.cham_eval_coverage_workspace_bytes(n_items), dtype=torch.uint8, device=rt.device),
                counts=torch.zeros(2, dtype=torch.int64, device=rt.device), per_click=None)
        if isinstance(recent_clicks_buffer, torch.Tensor):
            buf = recent_clicks_buffer
        else:
            buf = torch.from_numpy(np.ascontiguousarray(recent_clicks_buffer, dtype=np.int64).reshape(-1)).to(rt.device)
        ba['seed'] = buf                          # (kept alive until the seed launch has run)
        check(lib.cham_eval_coverage_seed(ptr(buf), buf.numel(), n_items, ptr(ba['rec']), ptr(ba['clk']), _stream()),
              "cham_eval_coverage_seed")
        # data parallel: fp64 column sums of the per-click values and the number of valid clicks, over this rank's rows of every batch
        ba['sums'] = torch.zeros(4, dtype=torch.float64, device=rt.device)
        ba['clicks'] = torch.zeros(1, dtype=torch.int64, device=rt.device)
        self._ba = dict(topn=int(topn), rel_pos=float(relevance_positive_sample), rel_neg=float(relevance_negative_samples))

    def _beyond_accuracy(self, d):
        """Per-click beyond-accuracy values of the ranked lists of this eval step + the coverage counts, on the current stream."""
        rt, lib, ba, ev = self.rt, self.rt.lib, self._ba_buffers, self._eval
        B, T, NC = ev['pred_ids'].shape
        if ba['per_click'] is None or ba['per_click'].shape[0] != B * T:
            ba['per_click'] = torch.empty(B * T, 4, dtype=torch.float32, device=rt.device)
        st = self._dev_state
        check(lib.cham_eval_beyond_accuracy(ptr(ev['pred_ids']), NC, ptr(d['label_next']), ptr(d['item_clicked']), B * T, ptr(rt.ace),
                                            rt.ace.shape[1], rt.n_items, ptr(st['pop_norm']), self._ba['topn'], self._ba['rel_pos'],
                                            self._ba['rel_neg'], ptr(ba['per_click']), ptr(ba['rec']), ptr(ba['clk']), _stream()),
              "cham_eval_beyond_accuracy")
        check(lib.cham_eval_coverage_count(ptr(ba['rec']), ptr(ba['clk']), rt.n_items, ptr(ba['ws']), ba['ws'].numel(), ptr(ba['counts']),
                                           _stream()), "cham_eval_coverage_count")
        if st.get('device'):
            self.articles_recent_pop_norm.note_consumed(d['aci'])      # pop_norm is read up to here: the state update waits for this
        self._ba_shape = (B, T)
        if self.dp is not None:      # the rank's share of the evaluation's totals (per_click is 0 at padded positions); reduced once, in the hook's end()
            ba['sums'] += ba['per_click'].double().sum(dim=0)
            ba['clicks'] += (d['label_next'] != 0).sum()

    def coverage_counts(self, rec_map=None, clk_map=None):
        """(recommended, clicked) item counts of the coverage maps (default: this model's), one cham_eval_coverage_count + one read-back."""
        rt, ba = self.rt, self._ba_buffers
        rec, clk = (ba['rec'], ba['clk']) if rec_map is None else (rec_map, clk_map)
        check(rt.lib.cham_eval_coverage_count(ptr(rec), ptr(clk), rt.n_items, ptr(ba['ws']), ba['ws'].numel(), ptr(ba['counts']), _stream()),
              "cham_eval_coverage_count")
        return tuple(ba['counts'].cpu().tolist())

    def beyond_accuracy_outputs(self):
        """(per_click [B, T, 4] float32 = ESI-R, ESI-RR, EILD-R, EILD-RR (0 at padded positions), (recommended, clicked) item counts
        of the coverage maps) after the last evaluate_step: the two device-to-host reads of the feature per batch."""
        ba = self._ba_buffers
        per_click = ba['per_click'].view(*self._ba_shape, 4).cpu().numpy()
        rec, clk = ba['counts'].cpu().tolist()
        return per_click, (rec, clk)

    def run_step(self):
        """What ``session.run(train_op | eval fetches)`` does for the current value of the input handles."""
        return self.train_step() if self.is_training else self.evaluate_step()

    # convenience for tests / hooks -------------------------------------------------------------------
    def outputs_numpy(self):
        pl = self._plan
        torch.cuda.synchronize()
        out = dict(loss=pl.loss.cpu().numpy(), logits=pl.full_rows(pl.logits).view(pl.B, pl.T, pl.NC).cpu().numpy(),
                   probs=pl.full_rows(pl.probs).view(pl.B, pl.T, pl.NC).cpu().numpy(), neg_items=pl.neg_ids.cpu().numpy(),
                   neg_slot=pl.neg_slot.cpu().numpy(), pool=pl.pool.cpu().numpy(), meta=pl.meta.cpu().numpy())
        if self.diversity_reg_factor > 0.0:      # p^T S p per click (zeros at padded positions)
            out['div_e'] = pl.full_rows(pl.div_e).view(pl.B, pl.T).cpu().numpy()
        return out


class GraphedTrainStep:
    """One training step of a NARModuleModel - forward, backward, TF-Adam, the recent-clicks state update and the NEXT batch's negative
    sampling - captured ONCE in a hipGraph (torch.cuda.CUDAGraph: stream capture of the step's lanes) and replayed per step.  The reference
    runs a step as ONE session.run (nar_model.py:1434-1470); eagerly this runtime submits ~135 launches through ctypes (0.9-1.0 ms of host
    time per step: what bounds a 32-session data-parallel shard or short sessions); a replay submits three: [the batch -> the step's input
    slot (one device-to-device copy of the packed block), cham_step_scalars_set, graph launch].

    What makes the step capturable: its launches carry no per-step host value - sampler key, max time stamp, sum(mask) and Adam's lr_t are
    read from the device record (csrc/common.h ChamStepScalars) - and its inputs sit at fixed addresses (the slot).  Limits (checked by
    supports()): one batch shape per object (B, T, global batch, row offset; NOT compacted - i.e. every position valid, or CHAM_COMPACT=0),
    device-resident ClickedItemsState, keep_prob 1, no data-parallel exchange inside the step, pinned upload ring (the packed block).
    Results are BIT-IDENTICAL to the eager step (tests/test_graph_step_gpu.py): same kernels, same arguments, same order per lane.

    Sampler hand-over: the graph's forward reads sampler-output set A; behind the state update the graph draws the NEXT batch's negatives
    (key .step_next) into set B from the `next` input slot and, as its last node, copies B -> A.  The first replay is preceded by an eager
    draw of the first batch's negatives into A."""

    def __init__(self, model, state):
        self.model, self.state, self.rt = model, state, model.rt
        self.graph, self.key, self.slots, self._expect = None, None, None, None
        self.replays = 0

    @staticmethod
    def shape_key(d):
        return (d['B'], d['T'], d['Bg'], d['row_begin'], d['P'], d.get('_total'), d.get('_layout'))

    def supports(self, d):
        """None when batch d can go through the captured step, else the reason (str)."""
        m, rt = self.model, self.rt
        if not rt.dev_scalars:
            return "CHAM_DEV_SCALARS=0"
        if d.get('pos') is not None or d['P'] != d['B'] * d['T']:
            return "compacted batch (the valid-position count varies from batch to batch)"
        if d.get('_block') is None:
            return "no packed device block (pinned upload ring off)"
        if not getattr(self.state, 'is_device', False) or self.state.stream is None:
            return "host-side ClickedItemsState"
        if self.state.n_updates < 1:
            return "empty recent-clicks state (the very first batch takes its normalisation statistics from its own rows: another launch sequence)"
        if getattr(rt, 'dp_active', False):
            return "data-parallel exchange inside the step"
        if m.keep_prob < 1.0 or m.eval_cold_start or not m.is_training or not rt.presample:
            return "dropout / cold-start analysis / presampling off"
        if m.diversity_reg_factor > 0.0:
            return "diversity regulariser (its two launches are not part of the captured step)"
        if rt.cosine:
            return "cosine ranking head (its launches are not part of the captured step)"
        if m.loss_function != 'softmax':
            return "loss_function %s (the captured step is the softmax loss's launch sequence)" % m.loss_function
        if self.key is not None and self.shape_key(d) != self.key:
            return "another batch shape than the captured one"
        if self.graph is None:      # capture needs a warm shape: buffers, workspaces, the step-scalar record and the kernels' dynamic-LDS
            # attributes are set up by the first eager step - none of that belongs inside a stream capture
            pl = rt._plans.get((d['B'], d['T'], m.negative_samples, m.negative_sample_from_buffer, d['Bg'], rt.p3, rt.h2))
            if pl is None or getattr(pl, 'eager_steps', 0) < 1 or rt.scalars is None:
                return "no eager training step has run on this batch shape yet (run one train_step first)"
        return None

    def _make_slot(self, d):
        blk = torch.zeros(max(d['_total'], 256), dtype=torch.uint8, device=self.rt.device)
        slot = dict(B=d['B'], T=d['T'], Bg=d['Bg'], row_begin=d['row_begin'], sum_mask=None, max_ts=None, P=d['P'], pos=None, uploaded=None,
                    _block=blk, _total=d['_total'], _layout=d['_layout'])
        for k, off, dt, shape in d['_layout']:
            n = int(np.prod(shape)) * np.dtype(dt).itemsize
            slot[k] = blk[off:off + n].view(_TORCH_DTYPE[dt]).view(shape)
        slot.update(ic_rows=slot['item_clicked'].view(-1), ln_rows=slot['label_next'].view(-1), ets_rows=slot['event_ts'].view(-1))
        return slot

    def _load(self, slot, d):
        torch.cuda.current_stream().wait_event(d['uploaded'])
        slot['_block'][:d['_total']].copy_(d['_block'][:d['_total']], non_blocking=True)

    def _capture(self, d, d_next):
        m, rt, state = self.model, self.rt, self.state
        self.key = self.shape_key(d)
        cur, nxt = self._make_slot(d), self._make_slot(d_next)
        self.slots = (cur, nxt)
        pl = rt.plan(d['B'], d['T'], m.negative_samples, m.negative_sample_from_buffer, d['Bg'])
        self._load(cur, d); self._load(nxt, d_next)
        m.feed_state(state, state)
        # the first batch's negatives, eagerly, into the set the captured forward reads (key by value: this is step rt.global_step)
        a = pl._samp_cur
        cur_scalars = dict(cur, max_ts=d['max_ts'], sum_mask=d['sum_mask'])
        m._neg_sample(pl, cur_scalars, rt.global_step, a, _stream())
        torch.cuda.synchronize()
        state.updated_event = state.consumed_event = None          # (everything has finished: no event of the eager past is waited for inside the capture)
        pl.grouped_ev = None
        g = torch.cuda.CUDAGraph()
        rt.capturing = True
        step0, upd0 = rt.global_step, state.n_updates
        try:
            with torch.cuda.graph(g):
                cur['_presampled'] = (pl, a, rt.global_step, None)
                m.forward(cur)
                m.backward()
                m.apply_gradients()                     # (increments rt.global_step: undone below - nothing has executed)
                state.update_from_device_batch(cur['aci'], cur['g_event_ts'])
                ok = m.presample(nxt)                   # -> set 1 - a, key .step_next
                assert ok, "presample() declined inside the capture"
                ev = nxt.pop('_presampled')[3]
                main = torch.cuda.current_stream()
                main.wait_event(ev)
                if state.updated_event is not None:
                    main.wait_event(state.updated_event)
                for name in ('neg_ids', 'neg_slot', 'pool', 'canon', 'meta'):
                    pl._samp[a][name].copy_(pl._samp[1 - a][name], non_blocking=True)
                # ... and the next batch becomes the current one: the host loads ONE slot per step
                cur['_block'].copy_(nxt['_block'], non_blocking=True)
        finally:      # (also when the capture fails: nothing of it has executed, the eager step remains usable)
            rt.capturing = False
            rt.global_step, state.n_updates = step0, upd0
            state.updated_event = state.consumed_event = None
            pl.grouped_ev = None
            pl.use_sampler_set(a)
            cur.pop('_presampled', None); nxt.pop('_presampled', None)
        self.graph, self.plan = g, pl
        return g

    def step(self, d, d_next):
        """One optimizer step on batch d; d_next = the batch of the following step (its negatives are drawn behind this step).  Returns the
        device loss tensor [total, xe, reg] (as train_step)."""
        why = self.supports(d) or self.supports(d_next)
        if why is not None:
            raise RuntimeError("GraphedTrainStep: %s" % why)
        m, rt, state = self.model, self.rt, self.state
        if self.graph is None:
            self._capture(d, d_next)
        else:
            if d is not self._expect:
                # not the batch the previous replay moved into the current slot and drew negatives for: load it and draw them now,
                # eagerly, with this step's key by value (what the eager forward does for a batch that was not presampled)
                self._load(self.slots[0], d)
                m._neg_sample(self.plan, d, rt.global_step, self.plan._samp_cur, _stream())
            self._load(self.slots[1], d_next)
        self._expect = d_next
        t = rt.global_step + 1
        check(rt.lib.cham_step_scalars_set(ptr(rt.scalars), rt.global_step & 0xFFFFFFFF, (rt.global_step + 1) & 0xFFFFFFFF, int(d['max_ts']),
                                           float(d['sum_mask']), float(m.adam_lr_t(t)), 7, _stream()), "cham_step_scalars_set")
        self.graph.replay()
        rt.global_step = t
        state.n_updates += 1
        state.updated_event = state.consumed_event = None
        self.replays += 1
        m._plan, m._d, m.total_loss = self.plan, self.slots[0], self.plan.loss
        return m.total_loss


_DEVICE_FED_METRICS = (ItemCoverage,) + BEYOND_ACCURACY_PER_CLICK     # fed by cham_eval_beyond_accuracy, not update_metrics


class ItemsStateUpdaterHook:
    """SessionRunHook around every step (nar_model.py:1369-1700), NAR-path subset:
      * before_run (:1434-1470): feeds ``articles_recent_pop_norm`` / ``pop_recent_items_buffer`` (+ the ACE matrix and
        metadata placeholders, which are already resident in HBM here) and names the fetches;
      * after_run (:1504-1650): in EVAL, HitRate@n / MRR@n of the ranked candidates (the reference's numpy streaming
        metrics, metrics.py, plus the TF streaming twins nar_model.py:826-835, 859-885); always: the recent-clicks state
        update from the batch (:1635-1649);
      * begin / end (:1410-1431, :1669-1695): state snapshot around evaluation, metrics appended to
        ``eval_sessions_metrics_log``;
      * ``eval_metrics_by_session_position`` (HitRate@n per click position, :1718) and ``eval_cold_start`` (steps between an
        item's first click and its first top-n recommendation, :1480-1494, 1621-1625, 1662-1666; runs in TRAIN and EVAL);
      * ``eval_beyond_accuracy_metrics`` (off by default; the reference always builds them, :1709-1719): NDCG@n on the host, and
        item coverage, ESI-R / ESI-RR (novelty) and content EILD-R / EILD-RR (diversity, relevance of the negatives =
        ``eval_negative_sample_relevance``) from cham_eval_beyond_accuracy, which reads the ranked ids, the ACE matrix, the
        ``articles_recent_pop_norm`` this batch was fed and the coverage maps seeded from the recent-clicks buffer at begin().
      * under an active data-parallel wrapper (``model.dp``, nar/parallel.py) an EVAL pass covers this rank's session rows of every batch:
        the ranked lists stay on the device, the accuracy metrics come from the rank histogram (cham_eval_rank_hist), and end() reduces
        every record over the ranks ONCE (DataParallelNAR.reduce_eval_records) - every rank logs the same, global numbers.
      * ``eval_benchmark_classifiers`` = names out of nar/baselines.BASELINE_NAMES ('pop_recent', 'cb', 'coocurrent', 'sr', 'v-sknn'): the reference's
        order per batch - evaluate the baselines on the model's candidate rows (EVAL, :1607-1613), let them learn the batch (both modes,
        :1627-1631), then the state update; their state (``eval_benchmarks_state``, a baselines.DeviceBaselines that outlives the hook) is
        snapshotted and restored with the clicked-items state; end() merges 'hitrate_at_n_<name>' / 'mrr_at_n_<name>' into the results.
      * ``eval_full_candidates`` (off by default): begin() enables the model's full-candidate ranking in EVAL, before_run
        reserves its record for the batch's T, evaluate_step ranks every valid click against every distinct id of the fed recent-clicks
        buffer, end() merges 'hitrate_at_n_chameleon_full', 'mrr_at_n_chameleon_full', 'ndcg_at_n_chameleon_full' (+ the per-position hit
        rates) and 'full_candidates_mean' into the results; refused by begin() under an active data-parallel wrapper.
      * in ``ModeKeys.PREDICT`` (Estimator.predict) before_run feeds the state; nothing is fetched, logged, snapshotted or updated.
    Out of scope: the ItemKNN ('item_knn') and undecayed SessionKNN ('sknn') baselines and the reference's dict form of ``eval_benchmark_classifiers``,
    the baselines' beyond-accuracy and cold-start records, the metrics the reference defines but does not instantiate."""

    def __init__(self, mode, model, eval_metrics_top_n, clicked_items_state, eval_sessions_metrics_log,
                 sessions_negative_items_log=None, sessions_chameleon_recommendations_log=None,
                 content_article_embeddings_matrix=None, articles_metadata=None, eval_negative_sample_relevance=None,
                 eval_benchmark_classifiers=[], eval_metrics_by_session_position=False, eval_cold_start=False,
                 eval_metric_ops=None, eval_beyond_accuracy_metrics=False, eval_benchmarks_state=None, eval_full_candidates=False):
        from .baselines import BASELINE_NAMES
        self.eval_full_candidates = bool(eval_full_candidates)
        if eval_benchmark_classifiers and not (isinstance(eval_benchmark_classifiers, (list, tuple)) and
                                               all(isinstance(x, str) and x in BASELINE_NAMES for x in eval_benchmark_classifiers)):
            raise NotImplementedError("baseline recommenders (nar/benchmarks) are out of scope: pass --disable_eval_benchmarks")
        self.eval_benchmark_classifiers = tuple(eval_benchmark_classifiers or ())
        self.baselines = eval_benchmarks_state if self.eval_benchmark_classifiers else None
        self.eval_cold_start = eval_cold_start
        self.eval_metrics_by_session_position = eval_metrics_by_session_position
        self.mode, self.model = mode, model
        self.eval_metrics_top_n = eval_metrics_top_n
        self.clicked_items_state = clicked_items_state
        self.eval_sessions_metrics_log = eval_sessions_metrics_log
        self.sessions_negative_items_log = sessions_negative_items_log
        self.sessions_chameleon_recommendations_log = sessions_chameleon_recommendations_log
        self.content_article_embeddings_matrix = content_article_embeddings_matrix
        self.articles_metadata = articles_metadata or {}
        self.eval_metric_ops = eval_metric_ops or {}
        self.eval_negative_sample_relevance = eval_negative_sample_relevance
        self.eval_beyond_accuracy_metrics = eval_beyond_accuracy_metrics

    def begin(self):
        if self.mode == ModeKeys.PREDICT:      # feeds the state (before_run) and does nothing else
            return
        if self.eval_full_candidates and self._data_parallel():
            raise ValueError("--eval_full_candidates: the full-candidate evaluation runs on one process, not under data parallelism")
        if self.eval_benchmark_classifiers:
            if self._data_parallel():
                raise ValueError("eval_benchmarks: the baseline recommenders are not available in a data-parallel run")
            if self.baselines is None:
                from .baselines import DeviceBaselines
                rt = self.model.rt
                self.baselines = DeviceBaselines(self.eval_benchmark_classifiers, rt.n_items, rt.ace, device=rt.device)
            if self.baselines.ace is None:
                self.baselines.attach_ace(self.model.rt.ace)       # the matrix already resident in HBM
            if self.mode == ModeKeys.EVAL:
                self.baselines.save_state_checkpoint()
                self.baselines.begin_evaluation(self.eval_metrics_top_n)
        if self.mode == ModeKeys.EVAL:
            from .metrics import HitRate, HitRateBySessionPosition, MRR, create_beyond_accuracy_metrics
            self.clicked_items_state.save_state_checkpoint()                    # nar_model.py:1415
            self.eval_streaming_metrics_last = {}
            self.streaming_metrics = [HitRate(self.eval_metrics_top_n), MRR(self.eval_metrics_top_n)]       # create_eval_metrics, :1696-1721
            if self.eval_beyond_accuracy_metrics:
                st = self.clicked_items_state
                host_buffer = st.get_recent_clicks_buffer()
                self.streaming_metrics += create_beyond_accuracy_metrics(self.eval_metrics_top_n, self.eval_negative_sample_relevance,
                                                                         self.content_article_embeddings_matrix, host_buffer)
                # the coverage maps are seeded from the same ring buffer: in place when it is in HBM
                self.model.enable_beyond_accuracy_metrics(self.eval_metrics_top_n, 1.0, self.eval_negative_sample_relevance,
                                                          st.buf_ids if getattr(st, 'is_device', False) else host_buffer)
            if self.eval_metrics_by_session_position:
                self.streaming_metrics.append(HitRateBySessionPosition(self.eval_metrics_top_n))
            if self.eval_full_candidates:
                self.model.enable_full_candidate_ranking(self.eval_metrics_top_n, 32)
            self.stats_logs = []
            if self._data_parallel():
                # every rank evaluates its own rows of every batch: the accuracy metrics come from the device-side rank histogram, summed
                # over the ranks once, in end() - the host classes above only fix the names and the order of the result keys
                if self.eval_cold_start or self.sessions_negative_items_log is not None or self.sessions_chameleon_recommendations_log is not None:
                    raise ValueError("eval_cold_start / save_eval_sessions_negative_samples / save_eval_sessions_recommendations need every "
                                     "rank's ranked lists on one host: not available in a data-parallel evaluation")
                self.model.enable_rank_histogram(self.eval_metrics_top_n, 32)
                self._dp_loss = torch.zeros(3, dtype=torch.float64, device=self.model.rt.device)
                self.eval_global_loss_sum = None

    def _data_parallel(self):
        dp = getattr(self.model, 'dp', None)
        return dp is not None and dp.active

    def after_create_session(self, session=None, coord=None):
        pass

    def before_run(self, run_context):
        from .estimator import SessionRunArgs
        m = self.model
        fetches = {'clicked_items': m.item_clicked, 'clicked_timestamps': m.event_timestamp,
                   'next_item_labels': m.next_item_label, 'last_item_label': m.label_last_item,
                   'session_id': m.session_id, 'user_id': m.user_id}
        dp_eval = self.mode == ModeKeys.EVAL and self._data_parallel()
        if self.eval_full_candidates and self.mode == ModeKeys.EVAL:
            m.reserve_full_candidate_ranking(np.asarray(m.inputs['item_clicked']).shape[1])
        if dp_eval:      # the ranked lists stay on the device (a rank without rows of this batch has none)
            fetches.update(batch_items_count=m.batch_items_count, batch_unique_items_count=m.batch_unique_items_count)
            m.reserve_rank_histogram(np.asarray(m.inputs['item_clicked']).shape[1])
        elif self.eval_cold_start or self.mode == ModeKeys.EVAL:               # nar_model.py:1444
            fetches.update(predicted_item_ids=m.predicted_item_ids, eval_batch_negative_items=m.batch_negative_items,
                           batch_items_count=m.batch_items_count, batch_unique_items_count=m.batch_unique_items_count,
                           predicted_item_probs=m.predicted_item_probs, label_rank=m.label_rank)
        dev = getattr(self.clicked_items_state, 'is_device', False)
        feed_dict = {m.ph_articles_recent_pop_norm: self.clicked_items_state if dev else self.clicked_items_state.get_articles_recent_pop_norm(),
                     m.ph_pop_recent_items_buffer: self.clicked_items_state if dev else self.clicked_items_state.get_recent_clicks_buffer(),
                     m.ph_content_article_embeddings_matrix: self.content_article_embeddings_matrix}
        for name in self.articles_metadata:
            if name in m.ph_articles_metadata:
                feed_dict[m.ph_articles_metadata[name]] = self.articles_metadata[name]
        if self.mode == ModeKeys.PREDICT:      # the state is fed, nothing is fetched (there are no labels), nothing is updated
            return SessionRunArgs(fetches={}, feed_dict=feed_dict)
        return SessionRunArgs(fetches=fetches, feed_dict=feed_dict)

    def after_run(self, run_context, run_values):
        if self.mode == ModeKeys.PREDICT:
            return
        r = run_values.results
        clicked_items = r['clicked_items']
        clicked_timestamps = np.squeeze(r['clicked_timestamps'], axis=-1)
        next_item_labels, last_item_label = r['next_item_labels'], r['last_item_label']
        sessions_ids = r['session_id']
        if self.mode == ModeKeys.EVAL and self._data_parallel():
            # the inputs are the GLOBAL batch on every rank: these counts are global as they stand
            self.stats_logs.append({'batch_items_count': r['batch_items_count'],
                                    'batch_unique_items_count': r['batch_unique_items_count'],
                                    'batch_sessions_count': len(sessions_ids)})
            self._dp_loss += self.model.total_loss.double()      # [total, xe share, L2] of this rank's rows (device add, no read-back)
        elif self.mode == ModeKeys.EVAL:
            predicted_item_ids = r['predicted_item_ids']
            # TF streaming twins (sparse_recall_at_top_k, define_mrr_metric) from the device-side rank of the positive
            rank = r['label_rank']
            valid = rank >= 0
            hit = valid & (rank < self.eval_metrics_top_n)
            if 'hitrate_at_n' in self.eval_metric_ops:
                self.eval_metric_ops['hitrate_at_n'].update(hit.sum(), valid.sum())
            if 'mrr_at_n' in self.eval_metric_ops:
                self.eval_metric_ops['mrr_at_n'].update((1.0 / (1.0 + rank[hit])).sum(), valid.sum())
            self.eval_streaming_metrics_last = {k: v.result() for k, v in self.eval_metric_ops.items()}
            if self.sessions_negative_items_log is not None:                   # :1530-1541
                for session_id, labels, neg_items in zip(sessions_ids, next_item_labels, r['eval_batch_negative_items']):
                    self.sessions_negative_items_log.append(
                        {'session_id': str(session_id),
                         'negative_items': [n for l, n in zip(labels.tolist(), neg_items.tolist()) if l != 0]})
            if self.sessions_chameleon_recommendations_log is not None:        # :1544-1580
                probs = r['predicted_item_probs'].round(decimals=7)
                pop = self.clicked_items_state.get_articles_recent_pop_norm()
                for session_id, labels, ids, pp in zip(sessions_ids, next_item_labels, predicted_item_ids, probs):
                    keep = labels != 0
                    self.sessions_chameleon_recommendations_log.append(
                        {'session_id': str(session_id), 'next_click_labels': labels[keep].tolist(),
                         'predicted_item_ids': ids[keep].tolist(), 'predicted_item_probs': pp[keep].tolist(),
                         'predicted_item_norm_pop': pop[ids[keep]].round(decimals=7).tolist()})
            self.stats_logs.append({'batch_items_count': r['batch_items_count'],
                                    'batch_unique_items_count': r['batch_unique_items_count'],
                                    'batch_sessions_count': len(sessions_ids)})
            from .evaluation import compute_metrics_results, update_metrics
            labels_norm_pop = preds_norm_pop = None
            if self.eval_metrics_by_session_position:                          # nar_model.py:1590-1593
                labels_norm_pop = self.clicked_items_state.get_articles_recent_pop_norm()[next_item_labels]
            on_device = [m for m in self.streaming_metrics if isinstance(m, _DEVICE_FED_METRICS)]
            update_metrics(predicted_item_ids, next_item_labels, labels_norm_pop, preds_norm_pop, clicked_items,
                           [m for m in self.streaming_metrics if not isinstance(m, _DEVICE_FED_METRICS)], recommender='chameleon')
            if on_device:                        # computed by evaluate_step (cham_eval_beyond_accuracy) from this batch's fed state
                per_click, counts = self.model.beyond_accuracy_outputs()
                valid = np.asarray(next_item_labels) != 0
                for m in on_device:
                    if isinstance(m, ItemCoverage):
                        m.add_counts(*counts)
                    else:
                        m.add_values(per_click[..., BEYOND_ACCURACY_PER_CLICK.index(type(m))][valid])
            self.eval_streaming_metrics_last.update(compute_metrics_results(self.streaming_metrics, recommender='chameleon'))
        if self.eval_cold_start:                                               # nar_model.py:1621-1625, both modes
            self.update_items_cold_start_state(r['user_id'], clicked_items, next_item_labels, r['eval_batch_negative_items'],
                                               r['predicted_item_ids'])
        if self.baselines is not None:
            self._run_baselines()
        # state update, nar_model.py:1635-1649
        if getattr(self.clicked_items_state, 'is_device', False):     # straight from the batch tensors already in HBM
            d = self.model._d
            self.clicked_items_state.update_from_device_batch(d['aci'], d['g_event_ts'])
            return
        from .clicked_items_state import batch_clicks_for_state
        ids, ts = batch_clicks_for_state(clicked_items, last_item_label, clicked_timestamps)
        self.clicked_items_state.update_items_state(ids, ts)

    def _run_baselines(self):
        """The baselines' share of a step, on the step's stream, from the batch tensors already in HBM: evaluate BEFORE the batch is
        learned (EVAL; nar_model.py:1607-1613), then learn it (both modes; :1627-1631).  No read-back."""
        m, st = self.model, self.clicked_items_state
        d = m._d
        if self.mode == ModeKeys.EVAL:
            recent_pop = None
            if 'pop_recent' in self.eval_benchmark_classifiers:
                if getattr(st, 'is_device', False):
                    recent_pop = st.recent_pop
                else:      # the counts behind the articles_recent_pop_norm this batch was fed
                    recent_pop = torch.from_numpy(np.ascontiguousarray(st.get_articles_recent_pop(), dtype=np.int32)).to(m.rt.device)
            self.baselines.evaluate(d['item_clicked'], d['label_next'], m._plan.neg_ids, recent_pop)
            if recent_pop is not None and getattr(st, 'is_device', False):
                st.note_consumed(d['aci'])         # recent_pop is read up to here: the state update waits for this
        session_ids = None
        if 'v-sknn' in self.eval_benchmark_classifiers:      # the ring keeps the session ids: 8 bytes per row, host -> device
            session_ids = torch.from_numpy(np.ascontiguousarray(np.asarray(m.session_id.eval()).reshape(-1), dtype=np.int64)).to(m.rt.device)
        self.baselines.learn(d['aci'], session_ids)

    def update_items_cold_start_state(self, users_ids, clicked_items, next_item_labels, eval_batch_negative_items, predicted_item_ids):
        """nar_model.py:1480-1494 (the benchmark recommenders' part, :1496-1501, is out of scope)."""
        st = self.clicked_items_state
        clicked_items_nonzero = set(np.asarray(clicked_items).reshape(-1).tolist()) | set(np.asarray(next_item_labels).reshape(-1).tolist())
        clicked_items_nonzero.discard(0)
        st.increment_current_step()
        st.update_items_first_click_step(clicked_items_nonzero)
        predicted_top_item_ids = np.asarray(predicted_item_ids)[:, :, :self.eval_metrics_top_n]
        st.get_cold_start_state().update_items_num_steps_before_first_rec(predicted_top_item_ids, st.items_first_click_step,
                                                                          st.get_current_step())

    def _reduce_data_parallel_eval(self):
        """The evaluation's records of this rank's rows -> global results, identical on every rank: ONE reduce_eval_records (int64 rank
        histogram and click count, fp64 popularity / beyond-accuracy / loss sums; MAX-union of the coverage maps)."""
        from .evaluation import compute_metrics_results
        from .metrics import HitRate, HitRateBySessionPosition, MRR, NDCG, accuracy_from_rank_hist
        m, dp, n = self.model, self.model.dp, self.eval_metrics_top_n
        ba = m._ba_buffers if self.eval_beyond_accuracy_metrics else None
        sums = self._dp_loss if ba is None else torch.cat([self._dp_loss, ba['sums']])
        red = dp.reduce_eval_records(m._rh['hist'], m._rh['pop_sum'], counts=None if ba is None else ba['clicks'], sums=sums,
                                     rec_map=None if ba is None else ba['rec'], clk_map=None if ba is None else ba['clk'])
        hist = red['hist'].cpu().numpy()
        acc = accuracy_from_rank_hist(hist, red['pop_sum'].cpu().numpy(), n)
        sums = red['sums'].cpu().numpy()
        # loss: xe shares summed over ranks + the L2 term every rank reports (summed world times)
        self.eval_global_loss_sum = float(sums[1] + sums[2] / dp.world)
        total, hits = int(hist.sum()), int(hist[:, :n].sum())
        if 'hitrate_at_n' in self.eval_metric_ops:
            self.eval_metric_ops['hitrate_at_n'].update(hits, total)
        if 'mrr_at_n' in self.eval_metric_ops:
            self.eval_metric_ops['mrr_at_n'].update(acc[MRR.name] * total if total else 0.0, total)
        self.eval_streaming_metrics_last = {k: v.result() for k, v in self.eval_metric_ops.items()}
        values = {HitRate.name: acc[HitRate.name], MRR.name: acc[MRR.name], NDCG.name: acc[NDCG.name],
                  HitRateBySessionPosition.name: acc[HitRateBySessionPosition.name]}
        if ba is not None:
            rec, clk = red['coverage_counts']
            values[ItemCoverage.name] = rec / float(clk)
            clicks = int(red['counts'].cpu()[0])
            for k, cls in enumerate(BEYOND_ACCURACY_PER_CLICK):
                values[cls.name] = float(sums[3 + k]) / clicks if clicks else float('nan')

        class _Reduced:
            def __init__(self, name):
                self.name = name

            def result(self):
                return values[self.name]
        self.eval_streaming_metrics_last.update(compute_metrics_results([_Reduced(x.name) for x in self.streaming_metrics],
                                                                        recommender='chameleon'))

    def end(self, session=None):
        if self.mode == ModeKeys.PREDICT:
            return
        if self.mode == ModeKeys.EVAL and self._data_parallel():
            self._reduce_data_parallel_eval()
        if self.mode == ModeKeys.EVAL:                                         # :1669-1695
            self.eval_streaming_metrics_last['clicks_count'] = int(np.sum([x['batch_items_count'] for x in self.stats_logs]))
            self.eval_streaming_metrics_last['sessions_count'] = int(np.sum([x['batch_sessions_count'] for x in self.stats_logs]))
            if self.eval_cold_start:                                           # add_cold_start_stats, :1662-1666
                self.eval_streaming_metrics_last['coldstart_chameleon'] = self.clicked_items_state.get_cold_start_state().get_statistics()
            if self.baselines is not None:
                self.eval_streaming_metrics_last.update(self.baselines.results(self.eval_metrics_top_n, self.eval_metrics_by_session_position))
            if self.eval_full_candidates:
                from . import full_eval
                self.eval_streaming_metrics_last.update(full_eval.results(self.model, self.eval_metrics_by_session_position))
            self.eval_sessions_metrics_log.append(self.eval_streaming_metrics_last)
            self.clicked_items_state.restore_state_checkpoint()
        if self.baselines is not None:
            self.baselines.check_tables()          # a dropped insert is an error (the growth rule makes it unreachable)
            if self.mode == ModeKeys.EVAL:
                self.baselines.restore_state_checkpoint()
