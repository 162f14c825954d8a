"""Negative sampler: the oracle against the reference's own property tests
(nar_module/nar/benchmarks/candidate_sampling_tests.py:10-99), and the HIP sampler bit-exact against the oracle."""
import numpy as np
import pytest

from oracle import philox, sampler as S

BUF = np.array([1, 2, 3, 1, 2, 3, 4, 4, 4, 5, 5, 5, 6, 6, 7, 7, 8, 9, 10] + [0] * 13, dtype=np.int64)


def test_philox_known_answers():
    """Random123 kat_vectors for philox4x32-10."""
    f = lambda *a: [int(w) for w in philox.philox4x32_10(*a)]
    assert f(0, 0, 0, 0, 0, 0) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert f(*[0xffffffff] * 6) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert f(0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344, 0xa4093822, 0x299f31d0) == \
        [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]


# ---- reference property tests, candidate_sampling_tests.py ------------------------------------------------
def test_get_sample_from_recently_clicked_items_buffer():          # :16-20
    sample = S.sample_from_recent_buffer(BUF, 5, 42, 0)
    assert sample.shape == (5,) and 0 not in sample
    assert np.isin(sample, BUF).all()


def _click(valid_list, n, j=0):
    pool = np.array(valid_list, dtype=np.int64)
    return S.neg_items_click(pool, S.canonical_slots(pool), np.ones(len(pool), bool), n, 3, j, 42, 7)[0]


def test_get_neg_items_click():                                     # :22-26
    sample = _click([1, 2, 2, 4, 4, 5, 4, 3, 2, 16, 4, 8, 6], 5)
    assert sample.shape == (5,) and np.unique(sample).shape == (5,)


def test_get_neg_items_click_padding():                             # :28-33
    sample = _click([1, 2, 2], 10)
    assert sample.shape == (10,) and np.count_nonzero(sample) == 2 and not sample[2:].any()


def _session(session_items, cands, n):
    pool = np.array(cands, dtype=np.int64)
    canon = S.canonical_slots(pool)
    valid = ~np.isin(pool, session_items)
    return np.vstack([S.neg_items_click(pool, canon, valid, n, 0, j, 42, 0)[0] if c != 0 else np.zeros(n, np.int64)
                      for j, c in enumerate(session_items)])


def test_get_neg_items_session():                                   # :36-45
    samples = _session([1, 2, 3], [1, 3, 5, 7, 9, 11, 13, 15, 18, 20, 9, 11], 10)
    assert samples.shape == (3, 10) and np.count_nonzero(samples == 0) == 6 and not samples[:, -2:].any()
    for i in [1, 2, 3]:
        assert i not in samples


def test_get_negative_samples_padded_sessions():                    # :61-71
    aci = np.array([[1, 2, 3], [4, 0, 0]], dtype=np.int64)
    out = np.stack([_session(list(r), [1, 3, 5, 7, 9, 11, 13, 15, 18, 20, 9, 11], 10) for r in aci])
    assert out.shape == (2, 3, 10) and np.count_nonzero(out == 0) == 2 * 10 + 2 * 3 and not out[1, -2:].any()
    for sess, neg in zip(aci, out):
        assert not (set(sess.ravel()) & set(neg.ravel())) - {0}


def test_get_batch_negative_samples():                              # :74-99
    aci = np.array([[1, 2, 3, 4, 5], [4, 5, 6, 7, 0]], dtype=np.int64)
    out = S.batch_negative_samples(aci, BUF, 4, 10, 42, 0)           # drops the last position (nar_model.py:275)
    assert out.shape == (2, 4, 4)
    for sess, neg in zip(aci, out):
        assert not (set(sess.ravel()) & set(neg.ravel())) - {0}
    for b in range(2):
        for j in range(4):
            nz = out[b, j][out[b, j] != 0]
            assert len(np.unique(nz)) == len(nz)                     # no repetition per click


def test_dp_rows_are_sharding_independent():
    rng = np.random.default_rng(0)
    aci = rng.integers(1, 200, size=(16, 6)).astype(np.int64)
    aci[3, 4:] = 0
    buf = np.concatenate([rng.integers(1, 200, size=300), np.zeros(100, np.int64)])
    full = S.batch_negative_samples(aci, buf, 5, 50, 42, 3)
    lo = S.batch_negative_samples(aci, buf, 5, 50, 42, 3, rows=range(0, 8))
    hi = S.batch_negative_samples(aci, buf, 5, 50, 42, 3, rows=range(8, 16))
    assert np.array_equal(full, np.concatenate([lo, hi]))


def test_popularity_weighting_matches_reference_clone_in_distribution():
    """The reference's numpy clone draws np.random.permutation; ours a keyed sort: same first-pick distribution."""
    pool = np.array([7] * 6 + [8] * 3 + [9], dtype=np.int64)
    canon = S.canonical_slots(pool)
    first = [S.neg_items_click(pool, canon, np.ones(10, bool), 1, b, 0, 42, s)[0][0] for s in range(40) for b in range(50)]
    frac = np.bincount(first, minlength=10)[7:] / len(first)
    assert np.allclose(frac, [0.6, 0.3, 0.1], atol=0.04)


# ---- HIP sampler == oracle, bit exact -----------------------------------------------------------------------
def _gpu_sample(gpu, aci, buf, N, n_buf, seed, step, row_begin=0, row_count=None):
    import torch
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    Bg, T1 = aci.shape
    row_count = Bg if row_count is None else row_count
    d_aci = torch.from_numpy(aci).to(gpu); d_buf = torch.from_numpy(buf).to(gpu)
    neg = torch.zeros(row_count, T1 - 1, N, dtype=torch.int64, device=gpu)
    slot = torch.zeros(row_count, T1 - 1, N, dtype=torch.int32, device=gpu)
    pool = torch.zeros(20 * N, dtype=torch.int64, device=gpu)
    canon = torch.zeros(20 * N, dtype=torch.int32, device=gpu)
    meta = torch.zeros(4, dtype=torch.int32, device=gpu)
    nb = lib.cham_neg_sample_workspace_bytes(Bg * T1, len(buf), n_buf)
    ws = torch.empty(nb, dtype=torch.uint8, device=gpu)
    check(lib.cham_neg_sample(ptr(d_aci), Bg, T1, ptr(d_buf), len(buf), seed, step, row_begin, row_count, N, n_buf, ptr(neg),
                              ptr(slot), ptr(pool), ptr(canon), ptr(meta), ptr(ws), nb, torch.cuda.current_stream().cuda_stream),
          "neg_sample")
    torch.cuda.synchronize()
    return neg.cpu().numpy(), slot.cpu().numpy(), pool.cpu().numpy(), canon.cpu().numpy(), meta.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T1,N,n_buf,buf_size,n_items,fill", [
    (64, 8, 10, 100, 2000, 1000, 1500),       # config 1 (tiny)
    (16, 5, 4, 10, 64, 50, 0),                # empty buffer, few candidates -> zero padding
    (256, 20, 50, 3000, 20000, 46000, 20000),  # config 2 (G1 shape), full buffer
    (32, 30, 100, 5000, 6000, 13000, 4000),    # Adressa shape
])
def test_hip_sampler_bit_exact(gpu, B, T1, N, n_buf, buf_size, n_items, fill):
    rng = np.random.default_rng(B * 1000 + N)
    aci = rng.integers(1, n_items, size=(B, T1)).astype(np.int64)
    lens = rng.integers(2, T1 + 1, size=B)
    for b in range(B):
        aci[b, lens[b]:] = 0
    buf = np.zeros(buf_size, np.int64)
    buf[:fill] = rng.integers(1, n_items, size=fill)
    for step in (0, 5):
        neg, slot, pool, canon, meta = _gpu_sample(gpu, aci, buf, N, n_buf, 42, step)
        ref, aux = S.batch_negative_samples(aci, buf, N, n_buf, 42, step, return_aux=True)
        P = len(aux['pool'])
        assert meta[3] == P and meta[1] == len(aux['buf_sample'])
        assert np.array_equal(pool[:P], aux['pool']) and not pool[P:].any()
        assert np.array_equal(canon[:P], aux['canon'])
        assert np.array_equal(neg, ref)
        # slots point at the sampled id (or the pad slot)
        ok = (slot >= 0) & (slot < 20 * N)
        assert np.array_equal(pool[np.where(ok, slot, 0)][ok], neg[ok])
        assert (neg[slot == 20 * N] == 0).all() and (neg[slot < 0] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T1,N,n_buf,buf_size,n_items,fill", [
    (64, 8, 10, 100, 2000, 1000, 1500),
    (16, 5, 4, 10, 64, 50, 0),
])
def test_hip_sampler_dev_equals_by_value(gpu, B, T1, N, n_buf, buf_size, n_items, fill):
    """cham_neg_sample_dev takes the step from the step-scalars record (`which` 0: .step, 1: .step_next): all five outputs bit-equal to
    cham_neg_sample with the same step by value, at two of the bit-exact cases above."""
    import torch
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    rng = np.random.default_rng(B * 1000 + N)
    aci = rng.integers(1, n_items, size=(B, T1)).astype(np.int64)
    lens = rng.integers(2, T1 + 1, size=B)
    for b in range(B):
        aci[b, lens[b]:] = 0
    buf = np.zeros(buf_size, np.int64)
    buf[:fill] = rng.integers(1, n_items, size=fill)
    st = torch.cuda.current_stream().cuda_stream
    rec = torch.zeros(lib.cham_step_scalars_bytes(), dtype=torch.uint8, device=gpu)
    steps = (5, 77)
    check(lib.cham_step_scalars_set(rec.data_ptr(), steps[0], steps[1], 0, 0.0, 0.0, 1, st), "cham_step_scalars_set")
    d_aci, d_buf = torch.from_numpy(aci).to(gpu), torch.from_numpy(buf).to(gpu)
    nb = lib.cham_neg_sample_workspace_bytes(B * T1, len(buf), n_buf)
    for which in (0, 1):
        # (outputs start as zeros, as in _gpu_sample: both forms leave pool / canon beyond the P pool entries as they were)
        neg = torch.zeros(B, T1 - 1, N, dtype=torch.int64, device=gpu)
        slot = torch.zeros(B, T1 - 1, N, dtype=torch.int32, device=gpu)
        pool = torch.zeros(20 * N, dtype=torch.int64, device=gpu)
        canon = torch.zeros(20 * N, dtype=torch.int32, device=gpu)
        meta = torch.zeros(4, dtype=torch.int32, device=gpu)
        ws = torch.empty(nb, dtype=torch.uint8, device=gpu)
        check(lib.cham_neg_sample_dev(ptr(d_aci), B, T1, ptr(d_buf), len(buf), 42, rec.data_ptr(), which, 0, B, N, n_buf, ptr(neg), ptr(slot), ptr(pool),
                                      ptr(canon), ptr(meta), ptr(ws), nb, st), "cham_neg_sample_dev")
        torch.cuda.synchronize()
        got = (neg.cpu().numpy(), slot.cpu().numpy(), pool.cpu().numpy(), canon.cpu().numpy(), meta.cpu().numpy())
        want = _gpu_sample(gpu, aci, buf, N, n_buf, 42, steps[which])
        other = _gpu_sample(gpu, aci, buf, N, n_buf, 42, steps[1 - which])
        for name, g, w in zip(("neg_ids", "neg_slot", "pool", "canon", "meta"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (name, which)
        assert not np.array_equal(got[0], other[0]), "the two steps draw the same negatives: `which` would not show"
    assert lib.cham_neg_sample_dev(ptr(d_aci), B, T1, ptr(d_buf), len(buf), 42, None, 0, 0, B, N, n_buf, ptr(neg), ptr(slot), ptr(pool), ptr(canon),
                                   ptr(meta), ptr(ws), nb, st) == -22


@pytest.mark.gpu
def test_hip_sampler_row_shards(gpu):
    rng = np.random.default_rng(5)
    aci = rng.integers(1, 500, size=(32, 9)).astype(np.int64)
    buf = rng.integers(1, 500, size=800).astype(np.int64)
    full = _gpu_sample(gpu, aci, buf, 8, 200, 42, 11)[0]
    a = _gpu_sample(gpu, aci, buf, 8, 200, 42, 11, 0, 16)[0]
    b = _gpu_sample(gpu, aci, buf, 8, 200, 42, 11, 16, 16)[0]
    assert np.array_equal(full, np.concatenate([a, b]))


@pytest.mark.gpu
def test_hip_sampler_global_batch_of_8_gpus(gpu):
    """Bg = 2048 sessions (8 ranks x 256): 44k pool keys -> the threshold-prefiltered rank-select must stay bit exact;
    the oracle is evaluated for two row shards only (as rank 0 / rank 5 would)."""
    rng = np.random.default_rng(77)
    B, T1, N, n_buf = 2048, 20, 50, 3000
    aci = rng.integers(1, 46000, size=(B, T1)).astype(np.int64)
    lens = rng.integers(2, T1 + 1, size=B)
    for b in range(B):
        aci[b, lens[b]:] = 0
    buf = rng.integers(1, 46000, size=20000).astype(np.int64)
    for rb in (0, 5 * 256):
        neg, slot, pool, canon, meta = _gpu_sample(gpu, aci, buf, N, n_buf, 42, 9, rb, 32)
        ref, aux = S.batch_negative_samples(aci, buf, N, n_buf, 42, 9, rows=range(rb, rb + 32), return_aux=True)
        assert np.array_equal(pool, aux['pool']) and np.array_equal(canon, aux['canon'])
        assert meta[1] == len(aux['buf_sample']) == n_buf
        assert np.array_equal(neg, ref)


@pytest.mark.gpu
def test_hip_sampler_nearly_empty_buffer_falls_back_to_full_select(gpu):
    """Fewer valid keys than the selection size: the prefilter must not drop anything."""
    rng = np.random.default_rng(3)
    aci = rng.integers(1, 300, size=(8, 6)).astype(np.int64)
    buf = np.zeros(5000, np.int64); buf[:40] = rng.integers(1, 300, size=40)
    neg, slot, pool, canon, meta = _gpu_sample(gpu, aci, buf, 25, 500, 42, 2)
    ref, aux = S.batch_negative_samples(aci, buf, 25, 500, 42, 2, return_aux=True)
    P = len(aux['pool'])
    assert meta[3] == P and meta[1] == len(aux['buf_sample']) == 40
    assert np.array_equal(pool[:P], aux['pool']) and np.array_equal(neg, ref)


# ---- the sampler at its structural edges: every output bit-exact against the oracle ---------------------------------------------------
def _gpu_sample_raw(gpu, aci, buf, N, n_buf, seed, step, row_begin=0, row_count=None, ws_short=0, fill=-5):
    """cham_neg_sample over outputs prefilled with `fill`; returns (rc, neg, slot, pool, canon, meta) - flat arrays, never NULL pointers."""
    import torch
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import ptr
    lib = _lib.load()
    Bg, T1 = aci.shape
    row_count = Bg if row_count is None else row_count
    n_out = max(1, row_count * max(T1 - 1, 0) * max(N, 0))
    d_aci = torch.from_numpy(aci).to(gpu); d_buf = torch.from_numpy(buf).to(gpu)
    neg = torch.full((n_out,), fill, dtype=torch.int64, device=gpu)
    slot = torch.full((n_out,), fill, dtype=torch.int32, device=gpu)
    pool = torch.full((max(1, 20 * N),), fill, dtype=torch.int64, device=gpu)
    canon = torch.full((max(1, 20 * N),), fill, dtype=torch.int32, device=gpu)
    meta = torch.full((4,), fill, dtype=torch.int32, device=gpu)
    nb = lib.cham_neg_sample_workspace_bytes(Bg * T1, len(buf), n_buf)
    ws = torch.empty(nb, dtype=torch.uint8, device=gpu)
    rc = lib.cham_neg_sample(ptr(d_aci), Bg, T1, ptr(d_buf), len(buf), seed, step, row_begin, row_count, N, n_buf, ptr(neg), ptr(slot), ptr(pool),
                             ptr(canon), ptr(meta), ptr(ws), nb - ws_short, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (rc,) + tuple(t.cpu().numpy() for t in (neg, slot, pool, canon, meta))


def _assert_equals_oracle(gpu, aci, buf, N, n_buf, seed=42, step=3, row_begin=0, row_count=None):
    """neg_ids, pool, canon and meta equal the oracle's, bit for bit, over prefilled outputs; the slots name the sampled ids.
    Returns (neg [rows, T, N], slot, aux)."""
    Bg, T1 = aci.shape
    row_count = Bg if row_count is None else row_count
    rc, neg, slot, pool, canon, meta = _gpu_sample_raw(gpu, aci, buf, N, n_buf, seed, step, row_begin, row_count)
    assert rc == 0
    ref, aux = S.batch_negative_samples(aci, buf, N, n_buf, seed, step, rows=range(row_begin, row_begin + row_count), return_aux=True)
    P, pmax = len(aux['pool']), 20 * N
    assert meta.tolist() == [0, len(aux['buf_sample']), 0, P]
    assert np.array_equal(pool[:P], aux['pool']) and not pool[P:].any()
    assert np.array_equal(canon[:P], aux['canon']) and np.array_equal(canon[P:], np.arange(P, pmax))
    if row_count == 0:
        return None, None, aux
    neg, slot = neg.reshape(ref.shape), slot.reshape(ref.shape)
    assert np.array_equal(neg, ref)
    ok = (slot >= 0) & (slot < pmax)
    assert np.array_equal(pool[np.where(ok, slot, 0)][ok], neg[ok])
    assert (neg[slot == pmax] == 0).all() and (neg[slot < 0] == 0).all() and ((slot >= -1) & (slot <= pmax)).all()
    assert np.array_equal(slot[ok], aux['slots'][ok]) and np.array_equal(ok, aux['slots'] >= 0)
    pad = np.repeat((aci[row_begin:row_begin + row_count, :-1] == 0)[:, :, None], N, 2)
    assert (slot[pad] == -1).all() and (slot[~pad & ~ok] == pmax).all()          # padded click: -1; too few candidates: the pad slot
    return neg, slot, aux


def _ragged(rng, B, T1, n_items):
    aci = rng.integers(1, n_items, size=(B, T1)).astype(np.int64)
    for b, L in enumerate(rng.integers(1, T1 + 1, size=B)):
        aci[b, L:] = 0
    return aci


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [300, 0])
def test_hip_sampler_without_buffer_sample(gpu, fill):
    """n_from_buffer = 0 (a zero-length sample slot array in the workspace): the pool is the batch alone, whatever the buffer holds."""
    rng = np.random.default_rng(20 + fill)
    aci = _ragged(rng, 12, 7, 400)
    buf = np.zeros(400, np.int64); buf[:fill] = rng.integers(1, 400, size=fill)
    _, _, aux = _assert_equals_oracle(gpu, aci, buf, 6, 0)
    assert len(aux['buf_sample']) == 0 and np.isin(aux['pool'], aci).all()


@pytest.mark.gpu
@pytest.mark.parametrize("buf_size", [255, 256, 257, 2048, 2049])
def test_hip_sampler_buffer_sizes_at_the_block_and_tile_edges(gpu, buf_size):
    """One element less / more than a block of 256 keys and than the 2048-key LDS tile of the rank count; the last buffer slot is live."""
    rng = np.random.default_rng(buf_size)
    aci = _ragged(rng, 10, 6, 900)
    buf = rng.integers(1, 900, size=buf_size).astype(np.int64)
    buf[rng.random(buf_size) < 0.1] = 0
    buf[-1], buf[0] = 77, 78
    _assert_equals_oracle(gpu, aci, buf, 7, 120)


@pytest.mark.gpu
def test_hip_sampler_session_that_covers_the_pool(gpu):
    """A session that holds every distinct id of the pool has no candidate: its valid clicks get N zeros with the pad slot 20 N; its
    padded click gets slot -1."""
    aci = np.array([[1, 2, 3, 4, 5, 0, 0], [2, 3, 0, 0, 0, 0, 0], [5, 5, 4, 0, 0, 0, 0]], dtype=np.int64)
    buf = np.array([3, 4, 0, 5, 1, 0, 0, 2], dtype=np.int64)
    N = 4
    neg, slot, aux = _assert_equals_oracle(gpu, aci, buf, N, 6)
    assert set(aux['pool'].tolist()) == {1, 2, 3, 4, 5}
    assert not neg[0].any() and (slot[0, :5] == 20 * N).all() and (slot[0, 5] == -1).all()      # (the output drops position 6)
    assert (np.count_nonzero(neg[1, :2], axis=1) == 3).all() and (np.count_nonzero(neg[2, :3], axis=1) == 3).all()


@pytest.mark.gpu
def test_hip_sampler_pool_of_one_repeated_id(gpu):
    """Every pool entry is the same id: canon is all zeros; sessions that hold the id get nothing, and with a second id in the batch the
    sessions of that id get the first one once, then zeros."""
    aci = np.full((4, 5), 7, np.int64); aci[2, 3:] = 0
    buf = np.full(40, 7, np.int64)
    neg, slot, aux = _assert_equals_oracle(gpu, aci, buf, 3, 25)
    assert not aux['canon'].any() and len(aux['pool']) == 18 + 25 and not neg.any()
    buf[:] = 0
    aci[1] = [9, 9, 9, 0, 0]; aci[3] = [9, 0, 0, 0, 0]
    neg, slot, aux = _assert_equals_oracle(gpu, aci, buf, 3, 25)
    assert neg[1, :3].tolist() == [[7, 0, 0]] * 3 and neg[3, 0].tolist() == [7, 0, 0] and neg[0].tolist() == [[9, 0, 0]] * 4


@pytest.mark.gpu
@pytest.mark.parametrize("n_distinct", [6, 5])
def test_hip_sampler_exactly_enough_and_one_too_few_candidates(gpu, n_distinct):
    """N = 6 negatives from exactly 6 distinct candidates (no zero) and from 5 (one trailing zero, pad slot)."""
    N = 6
    aci = np.array([[1, 2, 1], [2, 1, 0], [1, 2, 2], [2, 2, 1]], dtype=np.int64)
    buf = np.zeros(20, np.int64)
    buf[:2 * n_distinct] = np.tile(np.arange(101, 101 + n_distinct), 2)
    neg, slot, aux = _assert_equals_oracle(gpu, aci, buf, N, 16)
    valid = aci[:, :-1] != 0
    assert (np.count_nonzero(neg[valid], axis=1) == n_distinct).all()
    assert all(sorted(r[:n_distinct].tolist()) == list(range(101, 101 + n_distinct)) for r in neg[valid])
    assert (slot[valid][:, n_distinct:] == 20 * N).all()


@pytest.mark.gpu
@pytest.mark.parametrize("which,limit", [("buffer", 101), ("buffer", 100), ("pool", 100)])
@pytest.mark.parametrize("nv_case", ["at", "above", "three_times"])
def test_hip_sampler_prefilter_switch(gpu, which, limit, nv_case):
    """k_sel_threshold prefilters iff #valid keys > 1.5 limit + 64: #valid = floor of that (full rank-select), one more (prefilter with a
    threshold of almost 2^32) and three times as many, for the buffer selection (limit = n_from_buffer, odd and even) and the pool
    selection (limit = 20 N)."""
    want = int(1.5 * limit + 64)
    nv = {"at": want, "above": want + 1, "three_times": 3 * want}[nv_case]
    rng = np.random.default_rng(nv + limit)
    if which == "buffer":
        N, n_buf = 5, limit
        aci = _ragged(rng, 6, 5, 3000)
        buf = np.zeros(800, np.int64)
        buf[rng.permutation(800)[:nv]] = rng.integers(1, 3000, size=nv)
        assert np.count_nonzero(buf) == nv
    else:
        N, n_buf = limit // 20, 10
        buf = np.zeros(64, np.int64); buf[5:15] = rng.integers(1, 3000, size=10)
        B, T1 = 40, 20
        aci = np.zeros((B, T1), np.int64)
        left = nv - 10                                     # valid keys of the pool selection = batch clicks + the 10 sampled buffer ids
        for b in range(B):
            L = min(T1, left, int(rng.integers(T1 - 3, T1 + 1)))
            aci[b, :L] = rng.integers(1, 3000, size=L)
            left -= L
        assert left == 0 and np.count_nonzero(aci) == nv - 10
    _, _, aux = _assert_equals_oracle(gpu, aci, buf, N, n_buf, row_count=6)
    assert len(aux['buf_sample']) == min(n_buf, np.count_nonzero(buf)) and len(aux['pool']) == 20 * N


@pytest.mark.gpu
def test_hip_sampler_shortest_session_and_single_negative(gpu):
    """T1 = 2 (one click and its label) and N = 1."""
    rng = np.random.default_rng(8)
    buf = rng.integers(1, 200, size=300).astype(np.int64)
    aci = rng.integers(1, 200, size=(9, 2)).astype(np.int64); aci[4, 1] = 0; aci[7] = 0
    _assert_equals_oracle(gpu, aci, buf, 5, 40)
    _assert_equals_oracle(gpu, _ragged(rng, 9, 6, 200), buf, 1, 40)
    _assert_equals_oracle(gpu, aci, buf, 1, 0)


@pytest.mark.gpu
def test_hip_sampler_largest_pool_that_fits_lds(gpu):
    """N = 819: 20 N = 16380 pool slots, sorted as 16384 keys in 128 KB of LDS - the largest N the click kernel takes.  N = 820 doubles the
    sort to 32768 keys, past the LDS budget: -22 and nothing written."""
    rng = np.random.default_rng(819)
    aci = np.array([[11, 12, 13], [14, 15, 0]], dtype=np.int64)
    buf = rng.integers(1, 46000, size=20000).astype(np.int64)
    neg, slot, aux = _assert_equals_oracle(gpu, aci, buf, 819, 17000)
    assert len(aux['pool']) == 16380 and len(aux['buf_sample']) == 17000 and np.count_nonzero(neg[0, 0]) == 819
    rc, neg, slot, pool, canon, meta = _gpu_sample_raw(gpu, aci, buf, 820, 17000, 42, 3)
    assert rc == -22 and (neg == -5).all() and (slot == -5).all() and (pool == -5).all() and (meta == -5).all()


@pytest.mark.gpu
def test_hip_sampler_argument_errors_and_empty_row_range(gpu):
    """row_count = 0 is not an error: pool, canon and meta are written (another rank's rows are sampled from the same pool), neg_ids is not.
    A row range past the batch, T1 = 1, N = 0 and a workspace one byte short are -22 with every output as it was."""
    rng = np.random.default_rng(9)
    aci = _ragged(rng, 8, 5, 300)
    buf = rng.integers(1, 300, size=500).astype(np.int64)
    _assert_equals_oracle(gpu, aci, buf, 4, 50, row_begin=3, row_count=0)
    _assert_equals_oracle(gpu, aci, buf, 4, 50, row_begin=8, row_count=0)
    rc, neg = _gpu_sample_raw(gpu, aci, buf, 4, 50, 42, 3, 3, 0)[:2]
    assert rc == 0 and (neg == -5).all()
    _assert_equals_oracle(gpu, aci, buf, 4, 50, row_begin=5, row_count=3)
    untouched = lambda out: out[0] == -22 and all((a == -5).all() for a in out[1:])
    assert untouched(_gpu_sample_raw(gpu, aci, buf, 4, 50, 42, 3, 5, 4))              # rows 5 .. 8 of 8
    assert untouched(_gpu_sample_raw(gpu, aci, buf, 4, 50, 42, 3, 9, 0))
    assert untouched(_gpu_sample_raw(gpu, aci[:, :1].copy(), buf, 4, 50, 42, 3))       # T1 = 1
    assert untouched(_gpu_sample_raw(gpu, aci, buf, 0, 50, 42, 3))                     # N = 0
    assert untouched(_gpu_sample_raw(gpu, aci, buf, 4, 50, 42, 3, ws_short=1))
