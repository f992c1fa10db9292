"""pfann_search_topk_excl on the GPU: the exact top-k with one range of rows left out per query row, on every path of the
launch plan and every storage, against the delete-the-rows oracle of tests/search_excl_cases.py.

Every case asserts the path it means to hit from the plan of its shape (pfann_search_plan, and pfann_search_plan_excl for
the masked kernels), so a change of the dispatch cannot quietly move a case to another kernel."""
import ctypes
import functools

import numpy as np
import pytest

import search_excl_cases as sx
import search_kernel_cases as skc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def world(n, d):
    db, pos = sx.song_db(1000 + n + d, sx.song_lengths(n + d, n), d)
    db.setflags(write=False)
    return db, pos


# storage: "copy" = fp32 rows + fp16 copy (pre-filter on: canonical scores), "f32" = fp32 rows only (pre-filter off),
# "f16" = fp16-only storage
def make_index(db, storage, label_base=0):
    from pfann_amd.database import DeviceIndex
    idx = DeviceIndex(db.shape[1], 0, storage="f16" if storage == "f16" else "f32")
    idx.load(db, np.array([label_base, label_base + db.shape[0]], np.int64), label_base)
    if storage != "f16":
        assert idx.set_prefilter(storage == "copy") == (storage == "copy")
    return idx


def plan_of(idx, nq, k, path, masked_kernels=()):
    """asserts the path of the shape and that the masked plan is the same path on masked kernels -> oracle kind"""
    stages, flags = idx.search_plan(nq, k)
    mst, mfl = idx.search_plan(nq, k, excl=True)
    assert flags["path"] == path and mfl["path"] == path, (flags, mfl)
    assert flags["canonical_scores"] == mfl["canonical_scores"] and mfl["error"] == "none"
    names = [s[0] for s in mst]
    if idx.ntotal:
        assert names[0] == "excl_prep_kernel"
        # every scan and every fallback of the masked plan is a masked kernel, and nothing else changed
        plain = [s[0] for s in stages]
        assert [nm for nm in names[1:] if not nm.endswith(", true>")] == [nm for nm in plain if not (
            nm.startswith("scan_") or nm.startswith("topk_fallback") or nm.startswith("select_tail"))], (names, plain)
        assert [nm.replace(", true>", ">") for nm in names[1:]] == plain
    assert not [kn for kn in masked_kernels if kn not in names], names
    return "canonical" if flags["canonical_scores"] == "1" else ("f16" if idx.storage == "f16" else "f32")


def run(torch, idx, q, k, lo, hi):
    D, I = idx.search(torch.as_tensor(q).cuda(), k, exclude=(np.asarray(lo, np.int64), np.asarray(hi, np.int64)))
    return D.cpu().numpy(), I.cpu().numpy()


def queries(db, pos, nq, mode):
    """database rows as queries, each with its own song as the range: "run" = consecutive rows (one to three songs: the
    union of a query tile's ranges is narrow, most db tiles skip the mask), "spread" = rows of songs all over the database (the
    union spans it: every db tile tests single rows, neighbouring query rows have different ranges)"""
    n = db.shape[0]
    if mode == "run":
        rows = (n // 3 + np.arange(nq)) % n
    else:                        # 13 songs from one end of the database to the other, taken in turn (13 ranges for the oracle)
        songs = np.linspace(0, len(pos) - 2, 13).astype(np.int64)[np.arange(nq) % 13]
        rows = np.minimum(pos[songs] + np.arange(nq) // 13, pos[songs + 1] - 1)
    lo, hi = sx.own_song_ranges(pos, rows)
    return np.ascontiguousarray(db[rows]), lo, hi


CASES = skc.EXCL_CASES           # name, n, d, nq, k, storage, path, a masked kernel the plan must hold


@pytest.mark.parametrize("mode", ["run", "spread"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_own_song_excluded(torch_cuda, case, mode):
    """Self-match: the queries are database rows and the range is their own song -- more than k rows that beat every row
    outside it (songs of up to 300 rows).  Also: empty ranges and NULL pointers are pfann_search_topk bit for bit."""
    name, n, d, nq, k, storage, path, kern = case
    db, pos = world(n, d)
    idx = make_index(db, storage)
    kind = plan_of(idx, nq, k, path, [kern])
    q, lo, hi = queries(db, pos, nq, mode)
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    sx.assert_masked(D, I, q, db, k, lo, hi, kind, what="%s/%s" % (name, mode))
    # nothing excluded: the unmasked answer, bit for bit
    qd = torch_cuda.as_tensor(q).cuda()
    D0, I0 = (x.cpu().numpy() for x in idx.search(qd, k))
    for elo, ehi in ((np.zeros(nq), np.zeros(nq)), (hi, lo), (np.full(nq, -7), np.full(nq, -3)), (np.full(nq, n), np.full(nq, n + 9))):
        De, Ie = run(torch_cuda, idx, q, k, elo, ehi)
        assert np.array_equal(Ie, I0) and np.array_equal(De.view(np.int32), D0.view(np.int32)), name
    Dn, In = torch_cuda.empty((nq, k), device="cuda"), torch_cuda.empty((nq, k), dtype=torch_cuda.int64, device="cuda")
    assert idx.lib.pfann_search_topk_excl(idx.handle, qd.data_ptr(), nq, k, None, None, Dn.data_ptr(), In.data_ptr(), idx._stream()) == 0
    assert np.array_equal(In.cpu().numpy(), I0) and np.array_equal(Dn.cpu().numpy().view(np.int32), D0.view(np.int32))


STRIDED = skc.EXCL_STRIDED       # name, n, d, nq, modes, the masked sampled pass (the shapes' rule: the registry)


@pytest.mark.parametrize("case", STRIDED, ids=[c[0] for c in STRIDED])
def test_sampled_pass_with_a_row_stride(torch_cuda, case):
    """The masked group-maximum pass where it skips rows: the row of an accumulator is (tile row) x stride, and a range
    that the sampled rows straddle must still lower the threshold by exactly its own rows.  The five-tile case is also the
    only one on the two-buffer form of the d = 128 sampled pass."""
    name, n, d, nq, modes, kern = case
    k = skc.EXCL_STRIDED_K
    db, pos = world(n, d)
    idx = make_index(db, "copy")
    kind = plan_of(idx, nq, k, "gmax", [kern])
    for mode in modes:
        q, lo, hi = queries(db, pos, nq, mode)
        D, I = run(torch_cuda, idx, q, k, lo, hi)
        sx.assert_masked(D, I, q, db, k, lo, hi, kind, what="%s/%s" % (name, mode))
    # six ranges, taken in turn: they begin and end on a sampled row and between two (b is a sampled row and the first of a
    # sampled tile at either stride), are one row wide, and sit at the ends of the shard
    b = 4 * 128 * 50
    pats = np.array([(b - 1, b + 1), (b + 1, b + 3), (b, b + 1), (b - 3, b + 200), (0, 5), (n - 3, n)], np.int64)
    lo, hi = (np.ascontiguousarray(pats[np.arange(nq) % len(pats), c]) for c in (0, 1))
    q = np.ascontiguousarray(db[lo])
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    sx.assert_masked(D, I, q, db, k, lo, hi, kind, what=name + "/geometry")


@pytest.mark.parametrize("storage", ["copy", "f32", "f16"])
def test_small_dense_padding(torch_cuda, storage):
    """n = 40 with 35 rows excluded and k = 10: five answers and five paddings, not excluded rows at the bottom of the list;
    a range over the whole shard (and beyond) leaves nothing."""
    db, pos = sx.song_db(7, [40], 128)
    idx = make_index(db, storage)
    kind = plan_of(idx, 4, 10, "small_dense")
    q = np.ascontiguousarray(db[[0, 17, 39, 5]])
    lo, hi = np.array([3, 0, 5, -100]), np.array([38, 35, 40, 1000])
    D, I = run(torch_cuda, idx, q, 10, lo, hi)
    sx.assert_masked(D, I, q, db, 10, lo, hi, kind, what="pad/" + storage)
    assert (I[:3, 5:] == -1).all() and (I[:3, :5] >= 0).all() and (I[3] == -1).all() and (D[3] == -sx.FLT_MAX).all()


@pytest.mark.parametrize("storage", ["copy", "f32", "f16"])
def test_dense_pass_above_and_below_the_small_select(torch_cuda, storage):
    """n = 6000 (dense, above the 4096 keys of the 256-thread select): rows that leave out 3000, 1000 and no rows sit on
    either side of that limit in one call"""
    n, d, k = 6000, 128, 50
    db, pos = world(n, d)
    idx = make_index(db, storage)
    stages, flags = idx.search_plan(6, k, excl=True)
    assert flags["path"] == "small_dense" and idx.search_plan(6, k)[1]["path"] == "small_dense"
    (scan,) = [st[0] for st in stages if st[0].startswith("scan_")]
    assert scan.startswith("scan_small_kernel<128, ") and scan.endswith(", 2, true>")
    kind = "canonical" if flags["canonical_scores"] == "1" else storage
    rows = np.array([10, 2500, 4000, 5999, 3000, 77])
    q = np.ascontiguousarray(db[rows])
    lo, hi = np.array([0, 2000, 3500, 2999, 0, 0]), np.array([3000, 3000, 6000, 5999, 0, 5990])
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    sx.assert_masked(D, I, q, db, k, lo, hi, kind, what="dense6000/" + storage)
    assert (I[5, 10:] == -1).all() and (I[5, :10] >= 5990).all()


@pytest.mark.parametrize("n,nq,path", [(12288, 19, "small_sampled_folded"), (40000, 130, "gmax"), (20000, 130, "ladder_f16")])
def test_everything_or_almost_everything_excluded(torch_cuda, n, nq, path):
    """Fewer than k rows (or groups) survive the mask: the sampled threshold degenerates and the padding rule still holds.
    Row 0 leaves everything out, row 1 all but 30 rows, row 2 all but k + 5, the others their own song."""
    d, k = 128, 100
    db, pos = world(n, d)
    idx = make_index(db, "copy")
    kind = plan_of(idx, nq, k, path)
    q, lo, hi = queries(db, pos, nq, "run")
    lo[:3], hi[:3] = [0, 30, 50], [n, n, n - k - 5 + 50]
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    sx.assert_masked(D, I, q, db, k, lo, hi, kind, what="all/%d" % n)
    assert (I[0] == -1).all() and (I[1, :30] >= 0).all() and (I[1, 30:] == -1).all() and (I[2] >= 0).all()


def geometry_ranges(n, nq):
    """ranges that start and end on, one before and one after a 64-row and a 128-row db tile boundary, at the ends of the
    shard, of one row, empty, and partly or wholly outside the shard; neighbouring query rows always differ"""
    b64, b128 = 64 * 101, 128 * 77                   # (64 * 101 is no multiple of 128)
    pats = [(0, 700), (n - 700, n), (0, 1), (n - 1, n)]
    for b in (b64, b128):
        pats += [(b - 1, b + 1), (b, b + 1), (b - 1, b), (b + 1, b + 64), (b - 64, b - 1), (b, b + 64), (b - 300, b), (b + 1, b + 300)]
    pats += [(-50, 10), (n - 10, n + 50), (-5, -1), (n, n + 9), (500, 400), (1234, 1235), (-(1 << 40), 77), (n - 77, 1 << 40)]
    lo = np.array([pats[i % len(pats)][0] for i in range(nq)], np.int64)
    hi = np.array([pats[i % len(pats)][1] for i in range(nq)], np.int64)
    return lo, hi


@pytest.mark.parametrize("label_base", [0, 1000])
def test_range_geometry(torch_cuda, label_base):
    """On the gmax shape: the query is the first row of its range (its best match is excluded), the rows next to the range
    are of the same song and come back.  label_base = 1000: ranges and labels live in the label space."""
    n, d, nq, k = 40000, 128, 130, 100
    db, pos = world(n, d)
    idx = make_index(db, "copy", label_base)
    kind = plan_of(idx, nq, k, "gmax")
    lo, hi = geometry_ranges(n, nq)
    q = np.ascontiguousarray(db[np.clip(lo, 0, n - 1)])
    D, I = run(torch_cuda, idx, q, k, lo + label_base, hi + label_base)
    sx.assert_masked(D, I, q, db, k, lo + label_base, hi + label_base, kind, label_base, what="geometry")
    for r in np.flatnonzero((hi - lo == 1) & (lo > 0) & (lo < n - 1))[:4]:          # one row out: the rest of its song leads
        a, b = sx.own_song_ranges(pos, lo[r:r + 1])
        assert a[0] <= I[r, 0] - label_base < b[0] and I[r, 0] - label_base != lo[r]


@pytest.mark.parametrize("nq,storage,path,kern", [
    (3, "copy", "small_sampled_folded", "select_tail_kernel<4, true>"),
    (40, "copy", "ladder_f16", "topk_fallback_kernel<4, true>"),
    (40, "f32", "ladder_f32", "topk_fallback_kernel<4, true>"),
    (3, "f16", "small_sampled_folded", "select_tail_kernel<2, true>"),
])
def test_overflow_falls_back_masked(torch_cuda, nq, storage, path, kern):
    """Rows [0, 9000) are identical and tie at the top, [100, 5000) is excluded: the survivor lists of query row 0 overflow,
    and the exact fallback must leave the same rows out -- ties go to the lower REMAINING row: 0..99, then 5000.."""
    n, d, k = 20000, 128, 150
    db = np.array(world(n, d)[0])
    db[:9000] = db[0]
    idx = make_index(db, storage)
    kind = plan_of(idx, nq, k, path, [kern])
    rng = np.random.default_rng(5)
    q = np.ascontiguousarray(db[np.concatenate([[0], rng.integers(9000, n, nq - 1)])])
    lo, hi = np.full(nq, 100), np.full(nq, 5000)
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    assert np.array_equal(I[0], np.concatenate([np.arange(100), np.arange(5000, 5050)]))
    assert (D[0] == D[0, 0]).all()
    if kind == "canonical":
        sx.assert_masked(D, I, q, db, k, lo, hi, kind, what="overflow")
    else:
        sx.assert_masked(D[1:], I[1:], q[1:], db, k, lo[1:], hi[1:], kind, what="overflow")


@pytest.mark.parametrize("n,nq,path", [(12288, 19, "small_sampled_folded"), (40000, 130, "gmax"), (20000, 130, "ladder_f16")])
def test_a_rows_result_does_not_depend_on_the_other_rows_ranges(torch_cuda, n, nq, path):
    d, k = 128, 100
    db, pos = world(n, d)
    idx = make_index(db, "copy")
    plan_of(idx, nq, k, path)
    q, lo, hi = queries(db, pos, nq, "spread")
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    for r in (0, 7 % nq, nq - 1):
        D1, I1 = run(torch_cuda, idx, q, k, np.full(nq, lo[r]), np.full(nq, hi[r]))
        assert np.array_equal(I1[r], I[r]) and np.array_equal(D1[r].view(np.int32), D[r].view(np.int32)), r


def test_more_than_one_chunk_of_query_rows(torch_cuda):
    """nq > 16384 is walked in chunks: the ranges move with the rows"""
    n, d, k, nq = 5000, 64, 5, 16384 + 300
    db, pos = world(n, d)
    idx = make_index(db, "copy")
    rows = (np.arange(nq) * 31) % n
    lo, hi = sx.own_song_ranges(pos, rows)
    q = np.ascontiguousarray(db[rows])
    D, I = run(torch_cuda, idx, q, k, lo, hi)
    tail = slice(16384 - 40, nq)
    sx.assert_masked(D[tail], I[tail], q[tail], db, k, lo[tail], hi[tail], "canonical", what="chunks")
    assert not ((I >= lo[:, None]) & (I < hi[:, None])).any()


def test_export_and_refusals(torch_cuda):
    from pfann_amd import lib as L
    from pfann_amd.database import search_plan
    lib = L.load()
    assert hasattr(lib, "pfann_search_topk_excl") and hasattr(lib, "pfann_search_plan_excl")
    buf = ctypes.create_string_buffer(64)
    assert lib.pfann_search_plan_excl(1000, 128, 5, 10, 7, buf, len(buf)) == -1 and "storage=7" in L.last_error()
    db, pos = world(300, 128)
    idx = make_index(db, "copy")
    q = torch_cuda.as_tensor(np.array(db[:5])).cuda()
    D = torch_cuda.empty((5, 10), device="cuda")
    I = torch_cuda.empty((5, 10), dtype=torch_cuda.int64, device="cuda")
    lo = torch_cuda.zeros(5, dtype=torch_cuda.int64, device="cuda")
    assert lib.pfann_search_topk_excl(idx.handle, q.data_ptr(), 5, 10, lo.data_ptr(), None, D.data_ptr(), I.data_ptr(), idx._stream()) == -1
    assert "excl" in L.last_error()
    with pytest.raises(ValueError):
        idx.search(q, 10, exclude=(np.zeros(4, np.int64), np.zeros(5, np.int64)))
    with pytest.raises(ValueError):
        search_plan(1000, 128, 5, 10, 1, phase=1, excl=True)
