"""The kernels of csrc/eval_full.hip alone against the numpy model (tests/full_rank_reference.py), exactly: integer counts of comparisons.

Shape: R = 5 rows, Nc = 70, K = 100, T1 = 4 - two column tiles of 64 per chunk with the second ragged (6 columns), two chunks with the
last ragged (30 of 70 columns; what lies beyond K is +inf and ids that would compete, so a column that is not skipped shows)."""
import numpy as np
import pytest
import torch

from chameleon_recsys_amd import _lib
from chameleon_recsys_amd._lib import check, ptr
from tests import full_rank_reference as R

pytestmark = pytest.mark.gpu

ROWS, NC, K, T1, B, T = 5, 70, 100, 4, 3, 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


def inputs():
    """cand [K] (+ 40 ids of junk behind it), aci [B, T1], per-row session / label / flat position, scores [ROWS, K] on a grid of 7 values
    (many ties), the label's score per row and chunk."""
    rng = np.random.default_rng(7)
    ids = np.sort(rng.choice(np.arange(1, 400), K + 40, replace=False))
    cand, junk = ids[:K], ids[K:]
    outside = int(np.setdiff1d(np.arange(1, 400), ids)[17])
    aci = np.array([[cand[3], cand[64], cand[99], 0],                # excluded ids in both tiles and both chunks; a pad slot
                    [cand[10], cand[10], outside, cand[70]],         # a repeated click; an id that is no candidate
                    [0, 0, 0, cand[50]]], np.int64)
    row_session = np.array([0, 1, 1, 2, 0], np.int32)
    labels = np.array([cand[64], outside, cand[70], cand[50], 399 + 5], np.int64)       # inside cand (rows 0, 2, 3), outside (1, 4: beyond every id)
    flat = np.array([0, 3, 4, 8, 2], np.int32)                       # b T + t of the rows; row 4 is padding of the block
    scores = rng.integers(-3, 4, (ROWS, K)).astype(np.float32)
    lab = rng.integers(-3, 4, (ROWS, 2)).astype(np.float32)
    scores[3, [0, 5, 69, 70, 99]] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    lab[3] = [np.inf, -np.inf]                                       # +inf label beside chunk 0, -inf beside chunk 1: ties with the infinities above
    scores[2, [1, 80]] = np.nan
    lab[4, 0] = np.nan                                               # a NaN label (chunk 0 only)
    return cand, junk, aci, row_session, labels, flat, scores, lab


def chunk_logits(scores, lab, Nc):
    """[chunks, ROWS, 1 + Nc]: column 0 the label's score, +inf beyond K."""
    chunks = -(-K // Nc)
    lg = np.full((chunks, ROWS, 1 + Nc), np.inf, np.float32)
    for j in range(chunks):
        w = min(Nc, K - j * Nc)
        lg[j, :, 0] = lab[:, j]
        lg[j, :, 1:1 + w] = scores[:, j * Nc:j * Nc + w]
    return lg


def run(dev, scores, lab, Nc):
    lib = _lib.load()
    cand, junk, aci, row_session, labels, _, _, _ = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cand_t, K_t = t(np.concatenate([cand, junk])), torch.tensor([K], dtype=torch.int32, device=dev)
    aci_t, sess_t, lab_t = t(aci), t(row_session), t(labels)
    beat = torch.zeros(ROWS, dtype=torch.int32, device=dev)
    comp = torch.zeros(ROWS, dtype=torch.int32, device=dev)
    for j, lg in enumerate(chunk_logits(scores, lab, Nc)):
        lg_t = t(lg)
        check(lib.cham_eval_full_rank_merge(ptr(lg_t), ptr(cand_t), ptr(K_t), j, Nc, ptr(lab_t), ptr(sess_t), ptr(aci_t), T1, ROWS, ptr(beat),
                                            ptr(comp), _stream()), "cham_eval_full_rank_merge")
    torch.cuda.synchronize()
    return beat, comp


def model(scores, lab, Nc):
    cand, _, aci, row_session, labels, _, _, _ = inputs()
    out = [R.full_rank(scores[r], lab[r], Nc, cand, aci[row_session[r]], labels[r]) for r in range(ROWS)]
    return np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out], np.int32)


def test_merge_matches_the_numpy_model_exactly_and_repeats(gpu):
    cand, _, aci, row_session, labels, _, scores, lab = inputs()
    want_rank, want_comp = model(scores, lab, NC)
    # the cases are really in there: excluded ids, ties on both sides of the id rule, non-finite values, a NaN label
    assert want_comp.tolist() == [K - 3, K - 2, K - 2, K - 1, K - 3]
    assert want_rank[4] >= 70 - 2                                    # the NaN label loses to every competitor of chunk 0
    beat, comp = run(gpu, scores, lab, NC)
    assert np.array_equal(beat.cpu().numpy(), want_rank) and np.array_equal(comp.cpu().numpy(), want_comp)
    again = run(gpu, scores, lab, NC)
    assert torch.equal(again[0], beat) and torch.equal(again[1], comp)


def test_two_chunks_accumulate_to_one_chunk_of_K(gpu):
    _, _, _, _, _, _, scores, lab = inputs()
    same = np.repeat(lab[:, :1], 2, axis=1)                          # the label's score is the same beside both chunks
    a = run(gpu, scores, same, NC)
    b = run(gpu, scores, same[:, :1], K)
    want = model(scores, same, NC)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert np.array_equal(a[0].cpu().numpy(), want[0]) and np.array_equal(a[1].cpu().numpy(), want[1])


def test_scatter_writes_the_valid_rows_only(gpu):
    lib, dev = _lib.load(), gpu
    flat = inputs()[5]
    beat = torch.tensor([4, 0, 7, 99, 55], dtype=torch.int32, device=dev)
    comp = torch.tensor([9, 8, 7, 100, 66], dtype=torch.int32, device=dev)
    rank = torch.full((B * T,), -1, dtype=torch.int32, device=dev)
    n_comp = torch.zeros(B * T, dtype=torch.int32, device=dev)
    check(lib.cham_eval_full_rank_scatter(ptr(beat), ptr(comp), ptr(torch.from_numpy(flat).to(dev)), 4, ptr(rank), ptr(n_comp), _stream()),
          "cham_eval_full_rank_scatter")
    torch.cuda.synchronize()
    assert rank.cpu().tolist() == [4, -1, -1, 0, 7, -1, -1, -1, 99] and n_comp.cpu().tolist() == [9, 0, 0, 8, 7, 0, 0, 0, 100]


def test_arguments_are_checked(gpu):
    lib, dev = _lib.load(), gpu
    z = torch.zeros(8, dtype=torch.int64, device=dev)
    p = ptr(z)
    assert lib.cham_eval_full_rank_merge(p, p, p, 0, 4, p, p, p, 129, 1, p, p, _stream()) != 0      # T1 beyond the LDS row
    assert lib.cham_eval_full_rank_merge(p, p, p, 0, 0, p, p, p, 4, 1, p, p, _stream()) != 0
    assert lib.cham_eval_full_rank_merge(p, p, p, 0, 4, p, p, None, 4, 1, p, p, _stream()) != 0
    assert lib.cham_eval_full_rank_scatter(p, p, p, 0, p, p, _stream()) != 0
