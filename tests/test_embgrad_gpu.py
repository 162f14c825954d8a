"""Deterministic embedding-table gradients (csrc/features.hip: cham_emb_grad_scan, cham_group_rows, cham_emb_grad_grouped) against a
float64 index_add reference - the IndexedSlices TF builds for tf.nn.embedding_lookup (nar_model.py:741, 918) - with heavy
duplicate keys (Zipf ids: the most popular article sits in ~20 % of the rows), and bit-reproducibility (two runs identical)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _s():
    return torch.cuda.current_stream().cuda_stream


def _assert_grouping(ids, perm, seg):
    """perm = the rows sorted by (id, row); seg = the segment table k_seg_table builds from it (heads, long segments, 64-row chunks)."""
    torch.cuda.synchronize()
    R = len(ids)
    pm = perm.cpu().numpy()
    assert np.array_equal(np.sort(pm), np.arange(R)), "perm is not a permutation"
    key = ids[pm] * (1 << 24) + pm
    assert (np.diff(key) > 0).all(), "rows are not sorted by (id, row)"
    assert np.array_equal(pm, np.lexsort((np.arange(R), ids)))
    # segment table: heads of the runs of equal ids in sorted order, the long ones listed
    sg = seg.cpu().numpy()
    sid = ids[pm]
    heads = np.flatnonzero(np.r_[True, sid[1:] != sid[:-1]])
    assert sg[0] == len(heads) and np.array_equal(sg[4:4 + len(heads)], heads) and sg[4 + len(heads)] == R
    lens = np.diff(np.r_[heads, R])
    longs = np.flatnonzero(lens > 32)
    assert sg[1] == len(longs) and np.array_equal(sg[R + 6:R + 6 + len(longs)], longs)
    chunks = (lens[longs] + 63) // 64                                # work items: 64-row chunks of the long segments
    wf = R + 6 + R // 33 + 2
    assert sg[2] == chunks.sum() and np.array_equal(sg[wf:wf + len(longs) + 1], np.r_[0, np.cumsum(chunks)])
    return lens


@pytest.mark.parametrize("R,n_items,dim,F,c0", [(10729, 46000, 117, 408, 288), (3000, 500, 44, 112, 8), (70, 1000, 256, 260, 4),
                                                (23457, 5000000, 16, 96, 0), (4000, 3000, 378, 520, 140),
                                                (1300021, 5000000, 16, 24, 4),         # more rows than rounds 1-3 could group (2^20)
                                                (2048, 70000, 32, 40, 8), (1, 300, 8, 8, 0), (4097, 2, 12, 16, 4)])   # one full sort tile; one row; two ids
def test_grouped_item_embedding_gradient(gpu, R, n_items, dim, F, c0):
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    rng = np.random.default_rng(R)
    key_bits = 0 if R == 70 else int(n_items - 1).bit_length()        # 0: all 32 bits of the ids are sorted
    ids = np.minimum(rng.zipf(1.2, size=R) * 7919 % n_items, n_items - 1).astype(np.int64)
    ids[rng.random(R) < 0.05] = 0                                   # the padding item is a real table row too
    dxs = rng.standard_normal((R, F)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(F)).astype(np.float32)
    uniq, inv = np.unique(ids, return_inverse=True)
    ref = np.zeros((len(uniq), dim))
    np.add.at(ref, inv, dxs[:, c0:c0 + dim].astype(np.float64))
    ref *= gamma[c0:c0 + dim].astype(np.float64)
    d_ids, d_dxs, d_gamma = torch.from_numpy(ids).to(gpu), torch.from_numpy(dxs).to(gpu), torch.from_numpy(gamma).to(gpu)
    perm = torch.full((R,), -1, dtype=torch.int32, device=gpu)
    ws = torch.zeros(lib.cham_group_rows_workspace_bytes(R) // 4, dtype=torch.int32, device=gpu)
    seg = torch.full((int(lib.cham_group_rows_segments_len(R)),), -7, dtype=torch.int32, device=gpu)
    check(lib.cham_group_rows(ptr(d_ids), R, key_bits, ptr(perm), ptr(seg), ptr(ws), ws.numel() * 4, _s()), "cham_group_rows")
    _assert_grouping(ids, perm, seg)
    outs = []
    for _ in range(2):
        table = torch.zeros(n_items * dim if n_items <= 50000 else int(uniq.max() + 1) * dim, device=gpu)
        check(lib.cham_emb_grad_grouped(ptr(d_dxs), R, F, c0, dim, ptr(d_gamma), ptr(d_ids), ptr(perm), ptr(seg), ptr(table), _s()), "grouped")
        torch.cuda.synchronize()
        outs.append(table.cpu())
    assert torch.equal(outs[0], outs[1]), "not bit-reproducible"
    got = outs[0].view(-1, dim).double().numpy()
    assert np.abs(got[uniq] - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())
    untouched = np.ones(got.shape[0], bool); untouched[uniq] = False
    assert not got[untouched].any()


@pytest.mark.parametrize("R,card,dim,F,c0,via_ids", [(4864, 12, 14, 72, 10, False), (7424, 1022, 45, 124, 0, False),
                                                      (10729, 461, 37, 408, 0, True), (300, 29, 18, 72, 54, False), (5000, 300, 130, 200, 3, True)])
def test_scan_small_table_gradient(gpu, R, card, dim, F, c0, via_ids):
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    rng = np.random.default_rng(R + card)
    dxs = rng.standard_normal((R, F)).astype(np.float32)
    gamma = (1.0 + 0.1 * rng.standard_normal(F)).astype(np.float32)
    if via_ids:                       # article metadata: key(r) = meta[ids[r]]
        n_items = 20000
        meta = rng.integers(0, card, size=n_items, dtype=np.int64)
        ids = rng.integers(0, n_items, size=R, dtype=np.int64)
        keys, keysrc, d_ids = meta[ids], torch.from_numpy(meta).to(gpu), torch.from_numpy(ids).to(gpu)
    else:
        keys = np.minimum(rng.zipf(1.5, size=R) - 1, card - 1).astype(np.int64)
        keysrc, d_ids = torch.from_numpy(keys).to(gpu), None
    ref = np.zeros((card, dim))
    np.add.at(ref, keys, dxs[:, c0:c0 + dim].astype(np.float64))
    ref *= gamma[c0:c0 + dim].astype(np.float64)
    d_dxs, d_gamma = torch.from_numpy(dxs).to(gpu), torch.from_numpy(gamma).to(gpu)
    outs = []
    for _ in range(2):
        table = torch.full((card, dim), float('nan'), device=gpu)
        check(lib.cham_emb_grad_scan(ptr(d_dxs), R, F, c0, dim, ptr(d_gamma), ptr(keysrc), ptr(d_ids), card, ptr(table), _s()), "scan")
        torch.cuda.synchronize()
        outs.append(table.cpu())
    assert torch.equal(outs[0], outs[1]), "not bit-reproducible"
    assert np.abs(outs[0].double().numpy() - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())


# ---- exact-arithmetic inputs at constructed segment lengths ----------------------------------------------------------------------
# dxs = integers in [-8, 8], gamma in {0.5, 1, 2, -1}: every partial sum of up to 2^21 such rows is an integer below 2^24 and the one
# multiplication is by a power of two or -1, so fp32 makes no rounding error in ANY summation order.  The kernels must therefore EQUAL
# the float64 np.add.at reference: one dropped, doubled or misplaced row fails whatever the size of the segment it sits in.
SENTINEL = -3.0                                   # table prefill: a row no id names must keep it
# row counts at the short / long split (32 | 33), at the 64-row chunk edges and, with 1025 rows = 17 chunks, a chunk-sum combine whose
# quarters are 5, 5, 5 and 2 chunks; the tail of short runs brings R to 3000 (two sort tiles)
RUN_LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 256, 257, 1025, 34, 96, 193, 264] + [1] * 200


def _exact_inputs(rng, R, F):
    dxs = rng.integers(-8, 9, size=(R, F)).astype(np.float32)
    gamma = rng.choice(np.array([0.5, 1.0, 2.0, -1.0], np.float32), size=F)
    return dxs, gamma


def _ids_from_runs(rng, lengths, n_items):
    """Distinct ids with exactly these row counts, rows shuffled."""
    vals = rng.choice(n_items, size=len(lengths), replace=False).astype(np.int64)
    ids = np.repeat(vals, lengths)
    rng.shuffle(ids)
    return ids


def _group(lib, gpu, ids, key_bits, perm=None, seg=None):
    from chameleon_recsys_amd._lib import check, ptr
    R = len(ids)
    d_ids = torch.from_numpy(ids).to(gpu)
    if perm is None:
        perm = torch.full((R,), -1, dtype=torch.int32, device=gpu)
        seg = torch.full((int(lib.cham_group_rows_segments_len(R)),), -7, dtype=torch.int32, device=gpu)
    ws = torch.zeros(lib.cham_group_rows_workspace_bytes(R) // 4, dtype=torch.int32, device=gpu)
    check(lib.cham_group_rows(ptr(d_ids), R, key_bits, ptr(perm), ptr(seg), ptr(ws), ws.numel() * 4, _s()), "cham_group_rows")
    return d_ids, perm, seg


def _exact_ref(ids, dxs, gamma, c0, dim):
    uniq, inv = np.unique(ids, return_inverse=True)
    ref = np.zeros((len(uniq), dim))
    np.add.at(ref, inv, dxs[:, c0:c0 + dim].astype(np.float64))
    return uniq, ref * gamma[c0:c0 + dim].astype(np.float64)


def _assert_grouped_exact(lib, gpu, ids, d_ids, perm, seg, dxs, gamma, c0, dim, n_rows):
    """cham_emb_grad_grouped over a sentinel-filled table of n_rows rows == the float64 reference, bit for bit, rows nobody names untouched."""
    from chameleon_recsys_amd._lib import check, ptr
    R, F = dxs.shape
    d_dxs, d_gamma = torch.from_numpy(dxs).to(gpu), torch.from_numpy(gamma).to(gpu)
    table = torch.full((n_rows, dim), SENTINEL, device=gpu)
    check(lib.cham_emb_grad_grouped(ptr(d_dxs), R, F, c0, dim, ptr(d_gamma), ptr(d_ids), ptr(perm), ptr(seg), ptr(table), _s()), "grouped")
    torch.cuda.synchronize()
    uniq, ref = _exact_ref(ids, dxs, gamma, c0, dim)
    d_uniq = torch.from_numpy(uniq).to(gpu)
    got = table[d_uniq].cpu().double().numpy()
    bad = np.flatnonzero((got != ref).any(1))
    assert np.array_equal(got, ref), "ids %s (row counts %s) differ from the exact sums" % (uniq[bad][:8], np.bincount(np.unique(ids, return_inverse=True)[1])[bad][:8])
    table[d_uniq] = SENTINEL
    assert bool((table == SENTINEL).all()), "a table row that no id names was written"


@pytest.mark.parametrize("case", ["constructed", "one_id", "all_distinct"])
def test_grouped_gradient_exact_at_constructed_run_lengths(gpu, case):
    """Run lengths 1 ... 1025 chosen at every edge of k_seg_table / k_emb_grad_all; one id for all 6000 rows (one long segment of 94 chunks);
    every row its own id (R segments, none long).  perm, seg and the grouped sums, exact."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(11)
    n_items = 5000
    if case == "constructed":
        ids = _ids_from_runs(rng, RUN_LENGTHS, n_items)
        assert len(ids) == 3000
    elif case == "one_id":
        ids = np.full(6000, 4321, np.int64)
    else:
        ids = rng.permutation(n_items)[:3000].astype(np.int64)
    d_ids, perm, seg = _group(lib, gpu, ids, 13)
    lens = _assert_grouping(ids, perm, seg)
    assert sorted(lens) == sorted(RUN_LENGTHS if case == "constructed" else [6000] if case == "one_id" else [1] * 3000)
    dxs, gamma = _exact_inputs(rng, len(ids), 72)
    _assert_grouped_exact(lib, gpu, ids, d_ids, perm, seg, dxs, gamma, 6, 44, n_items)


_CONSTRUCTED = {}


def _constructed(lib, gpu):
    """The constructed-lengths input grouped once, shared (read-only) by the cases below."""
    if not _CONSTRUCTED:
        rng = np.random.default_rng(12)
        ids = _ids_from_runs(rng, RUN_LENGTHS, 4000)
        d_ids, perm, seg = _group(lib, gpu, ids, 12)
        _assert_grouping(ids, perm, seg)
        dxs, gamma = _exact_inputs(rng, len(ids), 515)
        _CONSTRUCTED.update(ids=ids, d_ids=d_ids, perm=perm, seg=seg, dxs=dxs, gamma=gamma)
    return _CONSTRUCTED


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 256, 257, 511, 512])
def test_grouped_gradient_exact_at_every_column_group_edge(gpu, dim):
    """dim on both sides of the 64-column groups and of the NG = 4 | 8 switch (256 | 257), up to the 512-column limit; c0 % 4 != 0 and
    c0 + dim == F; short and long segments in both instances."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    c = _constructed(lib, gpu)
    c0, F = 3, dim + 3
    dxs, gamma = np.ascontiguousarray(c['dxs'][:, :F]), c['gamma'][:F]
    _assert_grouped_exact(lib, gpu, c['ids'], c['d_ids'], c['perm'], c['seg'], dxs, gamma, c0, dim, 4000)


def test_grouped_gradient_refuses_columns_it_cannot_hold(gpu):
    """dim = 513 (more than the 8 x 64 columns of the widest instance) and c0 + dim > F: -22, table as it was."""
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import ptr
    lib = _lib.load()
    c = _constructed(lib, gpu)
    R = len(c['ids'])
    d_dxs, d_gamma = torch.from_numpy(c['dxs']).to(gpu), torch.from_numpy(c['gamma']).to(gpu)
    for F, c0, dim in ((515, 0, 513), (515, 2, 513), (515, 4, 512), (64, 1, 64)):
        table = torch.full((4000, dim), SENTINEL, device=gpu)
        rc = lib.cham_emb_grad_grouped(ptr(d_dxs), R, F, c0, dim, ptr(d_gamma), ptr(c['d_ids']), ptr(c['perm']), ptr(c['seg']), ptr(table), _s())
        torch.cuda.synchronize()
        assert rc == -22 and bool((table == SENTINEL).all()), (F, c0, dim, rc)


def _wide_ids(rng, R, bits):
    """R ids over the full width of `bits` bits, with repeats: a third as many distinct values as rows, the extremes among them."""
    hi = 1 << bits
    vals = rng.integers(0, hi, size=max(1, R // 3), dtype=np.int64)
    vals[:3] = [hi - 1, 0, hi >> 1]                 # all-ones, zero, the top bit alone (2^31 for 32 bits)
    ids = vals[rng.integers(0, len(vals), size=R)]
    ids[:3] = vals[:3]
    rng.shuffle(ids)
    return ids


@pytest.mark.parametrize("R", [2047, 2048, 2049, 6145])
@pytest.mark.parametrize("key_bits", [8, 9, 16, 17, 24, 25, 32, 0])
def test_group_rows_radix_passes(gpu, key_bits, R):
    """1 ... 4 radix passes with non-zero digits in the top pass (ids over the full key width, at and above 2^31 for 32 / 0 bits), one
    sort tile exactly, one row less / more, and four tiles: perm == np.lexsort over (row, id), and the segment table."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    bits = key_bits or 32
    rng = np.random.default_rng(1000 * bits + R)
    ids = _wide_ids(rng, R, bits)
    assert ids.max() == (1 << bits) - 1 and ids.min() == 0 and (ids >> (8 * ((bits - 1) // 8))).max() > 0
    d_ids, perm, seg = _group(lib, gpu, ids, key_bits)
    _assert_grouping(ids, perm, seg)


def test_grouped_gradient_with_25_bit_ids(gpu):
    """Four passes feeding the gradient: ids clustered on both sides of 2^24 (the fourth pass's digit is 0 or 1), table of max(id) + 1 rows."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(25)
    R, dim = 2500, 4
    ids = ((1 << 24) - 40 + rng.integers(0, 80, size=R)).astype(np.int64)
    ids[:70] = (1 << 24) + 7                        # one long segment above the boundary
    rng.shuffle(ids)
    assert ids.min() < (1 << 24) <= ids.max() < (1 << 25)
    d_ids, perm, seg = _group(lib, gpu, ids, 25)
    _assert_grouping(ids, perm, seg)
    dxs, gamma = _exact_inputs(rng, R, 9)
    _assert_grouped_exact(lib, gpu, ids, d_ids, perm, seg, dxs, gamma, 5, dim, int(ids.max()) + 1)


def test_grouped_gradient_reuses_a_segment_table(gpu):
    """The last workgroup of a long segment re-arms the segment's ticket: a second gradient over the same seg is exact too; and
    cham_group_rows into the same perm / seg for other ids of the same R (other long segments, other chunk counts) leaves nothing behind."""
    from chameleon_recsys_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(13)
    ids = _ids_from_runs(rng, RUN_LENGTHS, 4000)
    d_ids, perm, seg = _group(lib, gpu, ids, 12)
    _assert_grouping(ids, perm, seg)
    for _ in range(2):
        dxs, gamma = _exact_inputs(rng, len(ids), 40)
        _assert_grouped_exact(lib, gpu, ids, d_ids, perm, seg, dxs, gamma, 1, 37, 4000)
    ids2 = _ids_from_runs(rng, [700, 513, 400, 130, 66, 33] + [2] * 579, 4000)
    assert len(ids2) == len(ids)
    d_ids2, perm, seg = _group(lib, gpu, ids2, 12, perm, seg)
    _assert_grouping(ids2, perm, seg)
    for _ in range(2):
        dxs, gamma = _exact_inputs(rng, len(ids2), 40)
        _assert_grouped_exact(lib, gpu, ids2, d_ids2, perm, seg, dxs, gamma, 1, 37, 4000)


@pytest.mark.parametrize("via_ids", [False, True])
@pytest.mark.parametrize("R", [1, 63, 64, 65, 1023, 1024, 1025])
def test_scan_gradient_exact(gpu, R, via_ids):
    """cham_emb_grad_scan on the exact inputs: R on both sides of a wave's 64 rows and of the 16-wave stride, dim on both sides of the
    64-column sub-loop; table rows that no source row looks up are written as exactly 0 over the NaN prefill; keys direct and through ids."""
    from chameleon_recsys_amd import _lib
    from chameleon_recsys_amd._lib import check, ptr
    lib = _lib.load()
    rng = np.random.default_rng(7 * R + via_ids)
    card, F, c0 = 37, 136, 3
    used = np.setdiff1d(np.arange(card), [0, 5, 20, card - 1])        # first, last and two inner table rows stay unused
    dxs, gamma = _exact_inputs(rng, R, F)
    if via_ids:
        n_items = 900
        meta = rng.choice(used, size=n_items).astype(np.int64)
        ids = rng.integers(0, n_items, size=R, dtype=np.int64)
        keys, keysrc, d_ids = meta[ids], torch.from_numpy(meta).to(gpu), torch.from_numpy(ids).to(gpu)
    else:
        keys = rng.choice(used, size=R).astype(np.int64)
        keys[: R // 2] = used[3]                                      # one hot key: half the rows
        keysrc, d_ids = torch.from_numpy(keys).to(gpu), None
    d_dxs, d_gamma = torch.from_numpy(dxs).to(gpu), torch.from_numpy(gamma).to(gpu)
    for dim in (1, 64, 65, 130):
        ref = np.zeros((card, dim))
        np.add.at(ref, keys, dxs[:, c0:c0 + dim].astype(np.float64))
        ref *= gamma[c0:c0 + dim].astype(np.float64)
        table = torch.full((card, dim), float('nan'), device=gpu)
        check(lib.cham_emb_grad_scan(ptr(d_dxs), R, F, c0, dim, ptr(d_gamma), ptr(keysrc), ptr(d_ids), card, ptr(table), _s()), "scan")
        torch.cuda.synchronize()
        got = table.cpu().double().numpy()
        assert np.array_equal(got, ref), (dim, np.flatnonzero((got != ref).any(1)))
        assert not got[[0, 5, 20, card - 1]].any()
