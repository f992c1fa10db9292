"""The exact search's scores, bit for bit.  Wherever the fp32 shard keeps an fp16 copy, the fp16 scan is only a pre-filter
and every returned score is re-computed in ONE fp32 summation order, the canonical one (csrc/search_common.h canon_part /
canon_sum; oracle/exactdot_c.c states it in C).  Every case below forces one re-scoring path and asserts, without any
tolerance, that the labels are the canonical top-k (ties to the lower row) and the scores the canonical bits of the labels."""
import numpy as np
import pytest

import search_kernel_cases as skc
from pfann_amd import synth
from score_bits import assert_canonical_topk, canonical_topk, rescoring_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _unit(x):
    x = np.asarray(x, np.float64)
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def _index(db, label_base=0, lo=0):
    from pfann_amd.database import DeviceIndex
    idx = DeviceIndex(db.shape[1], 0)
    idx.load(db, np.array([lo, lo + db.shape[0]], np.int64), label_base)
    assert idx.set_prefilter(True), "the shard has no fp16 copy: not a re-scoring path"
    return idx


def _search(torch, idx, q, k):
    D, I = idx.search(torch.as_tensor(q).cuda(), k)
    return D.cpu().numpy(), I.cpu().numpy()


def _assert_plan(idx, nq, k, path, kernels, **phase):
    """The call takes the path its test was written for: the plan's path and every kernel named (csrc/search_plan.h; the
    plan itself is held against a kernel trace by tests/test_search_plan.py).  -> the stages' kernel names."""
    stages, flags = idx.search_plan(nq, k, **phase)
    names = [s[0] for s in stages]
    assert flags["path"] == path and flags["error"] == "none", (flags, names)
    missing = [kn for kn in kernels if kn not in names]
    assert not missing, "the plan does not launch %s: %s" % (missing, names)
    return names, flags


def _check(torch, db, q, k, what, path, kernels, **want_flags):
    idx = _index(db)
    _, flags = _assert_plan(idx, q.shape[0], k, path, kernels)
    assert rescoring_path(db, q) and flags["canonical_scores"] == "1"
    assert {f: flags[f] for f in want_flags} == want_flags
    D, I = _search(torch, idx, q, k)
    return D, I, assert_canonical_topk(D, I, q, db, k, what=what)


def _songs(seed, n, d, run=40, spread=0.6):
    """Rows in runs of `run` similar rows ('songs'), unit norm."""
    db = synth.unit_rows(seed, "sb/db%d_%d" % (n, d), n, d).astype(np.float64)
    db += np.repeat(db[::run], run, axis=0)[:n] / spread
    return _unit(db)


def _queries(seed, db, nq, mix=0.5):
    q = synth.unit_rows(seed, "sb/q%d" % nq, nq, db.shape[1]).astype(np.float64)
    q[::2] = db[(np.arange(len(q[::2])) * 7919) % db.shape[0]] + mix * q[::2]
    return _unit(q)


@pytest.mark.parametrize("d", skc.QS_D)
@pytest.mark.parametrize("nq", skc.QS_NQ)
def test_query_stationary_batches_select_small(torch_cuda, nq, d):
    """nq > 32 at d = 64 / 128 and k <= 128: the group-maximum pass, then the full pass on scan_f16_qres_kernel (nq >= 33 and
    >= 16 db tiles, csrc/search_plan.h gmax), which leaves ~R k survivors per row (far below SMALL_N = 4096), so
    every row is selected and re-scored by select_rescore_small_kernel.  One to seventeen query tiles, ragged last tiles."""
    db = _songs(300 + d, skc.QS_N, d)
    q = _queries(310 + d, db, nq)
    # d = 128: three tile buffers while the grid is at most one workgroup per CU (sampled pass: query tiles x slices <= 256)
    # / less than one round of the 768 resident ones (full pass, 64-row db tiles)
    full = "scan_f16_qres_kernel<8, false, 64, %d>" % (3 if nq <= 1000 else 2) if d == 128 else "scan_f16_qres_kernel<4, false, 128, 2>"
    sampled = "scan_f16_qres_kernel<8, true, 128, %d>" % (3 if nq <= 304 else 2) if d == 128 else "scan_f16_qres_kernel<4, true, 128, 2>"
    _check(torch_cuda, db, q, skc.QS_K, "query-stationary nq=%d d=%d" % (nq, d), "gmax", [sampled, full, "select_rescore_small_kernel"])


def _big_cluster_db(n=skc.BITS_BIG_CLUSTER[0].n, d=skc.BITS_BIG_CLUSTER[0].d):
    """5000 near-identical rows (20000 .. 24999) around a centre c: a query near c keeps all 5000 within the fp16 margin."""
    db = synth.unit_rows(51, "t/big", n, d)
    c = synth.unit_rows(52, "t/bigc", 1, d)
    db[20000:25000] = c + 0.003 * db[20000:25000]
    return _unit(db), c


@pytest.mark.parametrize("nq", skc.BITS_BIG_CLUSTER_NQ)
def test_more_than_4096_survivors_select_body(torch_cuda, nq):
    """The data of test_gpu_parity.py::test_search_topk_more_than_4096_survivors: query rows 0 .. 4 sit near the centre of
    5000 near-identical rows, whose fp16 scores all lie within 2 eps of the k-th best, so those rows keep 4096 < n <= 8192
    survivors: select_rescore_small_kernel leaves them (n > SMALL_N) to select_rescore_kernel (select_rescore_body), which
    re-scores them; the other rows go through select_rescore_small_kernel in the same call."""
    db, c = _big_cluster_db()
    q = synth.unit_rows(53, "t/bigq", nq, 128)
    q[:5] = c + 0.05 * q[:5]
    q = _unit(q)
    _check(torch_cuda, db, q, skc.BITS_BIG_CLUSTER[0].k, "> 4096 survivors nq=%d" % nq, "gmax", ["select_rescore_small_kernel", "select_rescore_kernel"])


def test_sublist_overflow_fallback_fp32_rows(torch_cuda):
    """The data of test_gpu_parity.py::test_search_topk_sublist_overflow_falls_back: 3 x 128 near-identical rows in db tiles
    5, 37, 69 (one interleaved db slice of 32) overflow one survivor sub-list of query rows 0 .. 2, which are flagged and
    recomputed by topk_fallback_kernel from the fp32 rows."""
    d, n, nq = skc.BITS_SUBLIST_OVERFLOW.d, skc.BITS_SUBLIST_OVERFLOW.n, skc.BITS_SUBLIST_OVERFLOW.nq
    db = synth.unit_rows(43, "t/of", n, d)
    c = synth.unit_rows(44, "t/ofc", 1, d)
    for u in range(3):
        lo = (5 + 32 * u) * 128
        db[lo:lo + 128] = c + 0.01 * db[lo:lo + 128]
    db = _unit(db)
    q = synth.unit_rows(45, "t/ofq", nq, d)
    q[:3] = c + 0.05 * q[:3]
    _check(torch_cuda, db, _unit(q), skc.BITS_SUBLIST_OVERFLOW.k, "sub-list overflow", "ladder_f16", ["scan_f16_qres_kernel<8, false, 64, 3>", "topk_fallback_kernel<4>"])


def _small_path_db(seed, n, d):
    """For the small path (nq <= 32): row 0's query has 5000 near-identical rows (> 4096 survivors), row 1's 9000 rows tying
    exactly at the top (every sub-list overflows), row 2's 900 near-identical rows 32 tiles apart (one sub-list of 256
    overflows); the rest are ordinary rows."""
    rng = np.random.default_rng(seed)
    db = rng.standard_normal((n, d)).astype(np.float32)
    c = rng.standard_normal((3, d)).astype(np.float32)
    db[20000:25000] = c[0] + 0.003 * db[20000:25000]
    db[50000:59000] = c[1]
    for u in range(900):
        lo = 70001 + u * 32 * 32
        if lo < n:
            db[lo] = c[2] + 0.01 * db[lo]
    q = np.concatenate([c, rng.standard_normal((16, d)).astype(np.float32)])
    q[0] = c[0] + 0.05 * q[3]
    return _unit(db), _unit(q)


def test_folded_small_path_d128(torch_cuda):
    """nq <= 32, d = 128, n > 8192: the folded small path (csrc/search_plan.h small_sampled_folded: query preparation in the group-maximum pass,
    select_rescore_small_kernel, then select_tail_kernel).  Row 0 takes the select half of the tail launch (> 4096
    survivors), row 1 (exact ties overflowing every sub-list) and row 2 (one overflowing sub-list) its fallback half, and a
    query of norm 1e5 -- beyond fp16's range, flagged by the query preparation -- goes to the fallback too; the ordinary rows
    are selected by select_rescore_small_kernel.  Non-unit query rows, so that the scores are not all below 1."""
    db, q = _small_path_db(71, skc.BITS_FOLDED.n, skc.BITS_FOLDED.d)
    q = np.concatenate([q, 1e5 * q[5:6]]).astype(np.float32)
    q[6:10] *= np.float32(7.5)
    assert (q.shape[0], skc.BITS_FOLDED.k) == (skc.BITS_FOLDED.nq, 300)
    D, I, _ = _check(torch_cuda, db, q, skc.BITS_FOLDED.k, "folded small path", "small_sampled_folded",
                     ["scan_small_kernel<128, 2, 1>", "scan_small_kernel<128, 2, 0>", "select_rescore_small_kernel", "select_tail_kernel<4>"],
                     q_prep="folded", fallback="tail")
    assert np.array_equal(I[1], np.arange(50000, 50300))


def test_unfolded_small_path_d64(torch_cuda):
    """nq <= 32, d = 64, n > 8192: the small path one launch per stage -- query preparation, then select_rescore_small_kernel
    + select_rescore_kernel for row 0's > 4096 survivors, and then topk_fallback_kernel for the rows whose sub-lists
    overflowed (rows 1 and 2)."""
    db, q = _small_path_db(61, skc.BITS_UNFOLDED.n, skc.BITS_UNFOLDED.d)
    assert (q.shape[0], skc.BITS_UNFOLDED.k) == (skc.BITS_UNFOLDED.nq, 300)
    D, I, _ = _check(torch_cuda, db, q, skc.BITS_UNFOLDED.k, "unfolded small path", "small_sampled",
                     ["q_prep_kernel", "scan_small_kernel<64, 2, 1>", "scan_small_kernel<64, 2, 0>", "select_rescore_small_kernel",
                      "select_rescore_kernel", "topk_fallback_kernel<4>"])
    assert np.array_equal(I[1], np.arange(50000, 50300))


@pytest.mark.parametrize("d,nq,k", skc.GENERIC_LADDER)
def test_generic_ladder(torch_cuda, d, nq, k):
    """nq > 32 with k > 128 (no group-maximum pass: the survivor ladder of sampled levels, the re-scoring selects in mode 0
    for the thresholds, mode 1 at the full pass), and d = 96 (d % 8 == 0 but neither 64 nor 128: the ladder on the
    generic scan_f16_kernel at any k).  At nq <= 32 a d = 96 search takes the fp32 MFMA ladder instead (csrc/search_plan.h:
    `small` needs d in {64, 128}), which is not a re-scoring path."""
    db = _songs(400 + d + k, skc.GENERIC_LADDER_N, d)
    q = _queries(410 + d + k, db, nq)
    _check(torch_cuda, db, q, k, "generic ladder d=%d nq=%d k=%d" % (d, nq, k), "ladder_f16",
           ["fill_int2_kernel", "scan_f16_kernel<1>", "select_rescore_small_kernel"])
    scans = [s for s in _index(db).search_plan(nq, k)[0] if s[0].startswith("scan_")]
    assert len(scans) >= 2 and (d == 128 or all(s[0] == "scan_f16_kernel<1>" for s in scans))


def test_dense_small_shard(torch_cuda):
    """nq <= 32, d in {64, 128}, n <= 8192 with an fp16 copy: the dense single pass scores every row with fp32 MFMA, and the
    select re-scores every row within the MFMA-vs-canonical bound of the k-th score, computed in the kernel
    (csrc/search_f16.hip dense_canon_eps): canonical bits, as at every other shard size.  n <= 4096 takes
    select_dense_small_kernel, 4096 < n <= 8192 select_dense_kernel."""
    for d, n, nq, k in skc.DENSE_SMALL:
        db = _songs(500 + n + d, n, d, run=20)
        q = _queries(510 + n + d, db, nq)
        _check(torch_cuda, db, q, k, "dense small shard n=%d d=%d nq=%d k=%d" % (n, d, nq, k), "small_dense",
               ["scan_small_kernel<%d, 4, 2>" % d, "select_dense_small_kernel" if n <= 4096 else "select_dense_kernel"])


def test_margin_non_unit_norms(torch_cuda):
    """The data of test_gpu_parity.py::test_search_prefilter_margin_scales_with_norms: rows of norm 20 .. 60, queries of norm
    25 with thousands of scores 1e-3 relative apart around the k-th best, and one query row of norm 3e5 (the fallback)."""
    d, n, nq = skc.BITS_MARGIN.d, skc.BITS_MARGIN.n, skc.BITS_MARGIN.nq
    base = synth.unit_rows(71, "t/ms", n, d).astype(np.float64)
    c = synth.unit_rows(72, "t/msc", 1, d).astype(np.float64)[0]
    base[1000:4000] = c + 0.02 * base[1000:4000]
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    base *= (20.0 + 40.0 * synth.uniform01(73, "t/msn", n).astype(np.float64))[:, None]
    q = synth.unit_rows(74, "t/msq", nq, d).astype(np.float64)
    q[:40] = c + 0.05 * q[:40]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q *= 25.0
    q[50] *= 12000.0
    _check(torch_cuda, base.astype(np.float32), q.astype(np.float32), skc.BITS_MARGIN.k, "margin", "gmax", ["topk_fallback_kernel<4>"])


def _shards(db, cuts):
    import torch
    db_t = torch.from_numpy(db).cuda()
    return [_index(db_t[lo:hi].contiguous(), lo, lo) for lo, hi in zip(cuts[:-1], cuts[1:])]


def _two_phase(torch, whole, shards, q, k, m=None):
    q_t = torch.as_tensor(q).cuda()
    m = m or skc.bound_m(k, len(shards))
    L = whole.reduce_bound(torch.stack([ix.search_bound(q_t, k, m) for ix in shards]), k)
    parts = [ix.search_bounded(q_t, k, L) for ix in shards]
    Dm, Im = whole.merge_topk(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
    return Dm.cpu().numpy(), Im.cpu().numpy(), L


def test_bounded_second_phase(torch_cuda):
    """The second phase of the two-phase sharded search (search_topk_bounded): with the reduced global bound most rows keep a
    few dozen survivors per shard -- select_rescore_wave_kernel; a pending bound of -inf leaves every row its own threshold
    (hundreds of survivors) -- select_rescore_small_list_kernel; and query rows 0 .. 4 sit near 5000 near-identical rows of
    the first shard, all within the margin of the global bound: > 4096 survivors inside the bounded phase --
    select_rescore_list_kernel (select_rescore_body).  Every per-shard list and the merged list are canonical."""
    torch = torch_cuda
    cuts = skc.BOUNDED["cuts"]
    db, c = _big_cluster_db(cuts[-1])
    for s0 in range(40000, cuts[-1], 40):
        db[s0:s0 + 40] = db[s0] + 0.6 * db[s0:s0 + 40]
    db = _unit(db)
    nq, k = skc.BOUNDED["nq"], skc.BOUNDED["k"]
    q = _queries(81, db, nq)
    q[:5] = _unit(c + 0.05 * synth.unit_rows(82, "sb/bq", 5, 128))
    whole = _index(db)
    shards = _shards(db, cuts)
    Dm, Im, L = _two_phase(torch, whole, shards, q, k)
    want = assert_canonical_topk(Dm, Im, q, db, k, what="two-phase merged")
    D0, I0 = _search(torch, whole, q, k)
    assert_canonical_topk(D0, I0, q, db, k, want=want, what="whole db")
    q_t = torch.as_tensor(q).cuda()
    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        ix, part = shards[j], db[lo:hi]
        _assert_plan(ix, nq, k, "gmax", ["group_max_select_kernel"], phase=1, mtop=skc.bound_m(k, 3))
        _assert_plan(ix, nq, k, "gmax", ["bound_in_kernel", "select_rescore_wave_kernel", "select_rescore_small_list_kernel",
                                         "select_rescore_list_kernel"], phase=2, resume_with_lb=True)
        Dl, Il = _search(torch, ix, q, k)
        wl = canonical_topk(q, part, k)
        wl = (wl[0], np.where(wl[1] >= 0, wl[1] + lo, -1))
        # (labels carry the shard's base: compare against the shard's own canonical list)
        assert np.array_equal(Il, wl[1]) and np.array_equal(Dl.view(np.int32), wl[0].view(np.int32)), "shard %d plain" % j
        ix.search_bound(q_t, k, skc.bound_m(k, 3))
        Dt, It = ix.search_bounded(q_t, k, torch.as_tensor(Dl[:, k - 1]).cuda().contiguous())       # tight: the wave tier
        assert np.array_equal(It.cpu().numpy(), Il) and np.array_equal(Dt.cpu().numpy().view(np.int32), Dl.view(np.int32))
        ix.search_bound(q_t, k, skc.bound_m(k, 3))
        Dn, In = ix.search_bounded(q_t, k, torch.full((nq,), float("-inf"), device="cuda"))      # -inf: the list kernels
        assert np.array_equal(In.cpu().numpy(), Il) and np.array_equal(Dn.cpu().numpy().view(np.int32), Dl.view(np.int32))


def _cross_db():
    """Row c0's neighbours: 5000 near-identical rows in the first third (> 4096 survivors there), and 9000 rows tying exactly a
    little below them in the second third (all within the fp16 margin: that shard's lists overflow, and so do the lists of
    any search over the whole db).  Row c1's: 5000 near-identical rows in the last third alone."""
    d, n = skc.ONE_ROW["d"], skc.ONE_ROW["n"]
    rng = np.random.default_rng(91)
    db = rng.standard_normal((n, d))
    c = _unit(rng.standard_normal((2, d))).astype(np.float64)
    v = _unit(rng.standard_normal((1, d)))[0]
    db[5000:10000] = c[0] + 0.003 * db[5000:10000]
    db[25000:34000] = c[0] + 0.0036 * v
    db[45000:50000] = c[1] + 0.003 * db[45000:50000]
    return _unit(db), c.astype(np.float32)


def test_one_row_same_bits_on_every_path(torch_cuda):
    """The promise in plain terms: one query row gets the same scores and labels, bit for bit, searched alone (nq = 1: the
    folded small path), inside a batch of 100 and of 2100 (the query-stationary kernels), and as a two-phase search over
    three shards in which it has > 4096 survivors on one shard (select_rescore_body) and overflows its survivor lists on
    another (topk_fallback_kernel).  All of them equal the canonical top-k.  Second run: the first shard holds <= 8192 rows
    (the dense small pass) and nq <= 32."""
    torch = torch_cuda
    db, c = _cross_db()
    k = skc.ONE_ROW["k"]
    rows = c                                                       # the rows under test: c0 and c1 themselves
    others = _queries(92, db, max(skc.ONE_ROW["batches"]))
    want = canonical_topk(rows, db, k)
    whole = _index(db)
    _assert_plan(whole, 1, k, "small_sampled_folded", ["select_tail_kernel<4>"])
    for nq in skc.ONE_ROW["batches"]:
        _assert_plan(whole, nq, k, "gmax", ["scan_f16_qres_kernel<8, false, 64, %d>" % (3 if nq == 100 else 2)])
    runs = []
    for j in range(2):
        D, I = _search(torch, whole, rows[j:j + 1], k)
        runs.append(("alone", j, D[0], I[0]))
    for nq in skc.ONE_ROW["batches"]:
        q = np.concatenate([rows, others[:nq - 2]]).astype(np.float32)
        D, I = _search(torch, whole, q, k)
        runs += [("batch %d" % nq, j, D[j], I[j]) for j in range(2)]
        Dm, Im, _ = _two_phase(torch, whole, _shards(db, skc.ONE_ROW["cuts"]), q, k)
        runs += [("two-phase 3 shards, batch %d" % nq, j, Dm[j], Im[j]) for j in range(2)]
    for nq in skc.ONE_ROW["small_batches"]:
        q = np.concatenate([rows, others[:nq]])[:max(nq, 2)].astype(np.float32)
        Dm, Im, _ = _two_phase(torch, whole, _shards(db, skc.ONE_ROW["cuts_dense"]), q, k)
        runs += [("two-phase, shard of 8000 rows, batch %d" % len(q), j, Dm[j], Im[j]) for j in range(2)]
        Dm, Im, _ = _two_phase(torch, whole, _shards(db, skc.ONE_ROW["cuts"]), q, k)
        runs += [("two-phase 3 shards, batch %d" % len(q), j, Dm[j], Im[j]) for j in range(2)]
    for what, j, D, I in runs:
        assert np.array_equal(I, want[1][j]), "%s, row c%d: labels differ from the canonical top-k" % (what, j)
        assert np.array_equal(D.view(np.int32), want[0][j].view(np.int32)), "%s, row c%d: score bits differ" % (what, j)
