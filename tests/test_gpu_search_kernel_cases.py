"""The search kernels no older test held against an exact answer, each on the smallest shape that reaches it under default
tuning (tests/search_kernel_cases.py; tests/test_search_kernel_coverage.py proves on the CPU that the registry reaches every
kernel of csrc/search_plan.h).  Every case asserts from the plan of its own handle that it launches the kernel it was added
for, so a retuning of the plan cannot move it away quietly.

References and rules are the neighbouring tests': "copy" storage (fp32 rows, pre-filter on) -> the canonical top-k, bit for
bit (score_bits.assert_canonical_topk); "f32" -> test_gpu_parity._check_topk (2e-6 on unit rows, ties only at the k-th
score); "f16" -> oracle flat_ip_topk_f16 by test_search_fp16_storage's rule; masked -> search_excl_cases.assert_masked with
the kind of the storage.

Data: "songs" -- runs of 20 to 40 similar unit rows; every second query is planted near a database row, one query row is all
zeros (every score ties: the fallback's answer is rows 0 .. k - 1), and the last query row is planted on the LAST database
row (a ragged last db tile and, at 513 rows, the only row of the last query tile)."""
import functools

import numpy as np
import pytest

import search_excl_cases as sx
import search_kernel_cases as skc
import test_gpu_parity as par
import test_gpu_score_bits as sb
import test_gpu_search_excl as xt
from score_bits import assert_canonical_topk

pytestmark = pytest.mark.gpu
T = "test_gpu_search_kernel_cases::"
FLT_MAX = np.finfo(np.float32).max
ZERO_ROW = 1                    # the all-zero query row (odd: not a planted one)

PATHS = {"small64_f32": "small_sampled", "emit32_f32": "ladder_f32", "small64_f16_dense": "small_dense",
         "small64_f16_dense_n8192": "small_dense", "emit_qt4": "ladder_f32", "emit_qt4_d36": "ladder_f32", "f16_qt4": "ladder_f16",
         "f16_qt4_half": "ladder_f16", "dbr64_nbuf2": "gmax", "wave16_full": "gmax"}


def path_of(c):
    name = c.name[:-5] if c.name.endswith("_excl") else c.name
    return "gmax" if name.startswith("wave") else PATHS[name]


def shape_plan(c):
    """the plan of the case's shape (the checks below assert the kernels again from the plan of the handle they run)"""
    from pfann_amd.database import search_plan
    assert c.phase == 0
    return search_plan(c.n, c.d, c.nq, c.k, skc.plan_storage(c), excl=c.excl)


def ids(c):
    return c.name


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@functools.lru_cache(maxsize=2)
def songs(n, d):
    """[n, d] unit rows in runs of 20 .. 40 similar rows (one length per database), read-only: shared between cases"""
    db = sb._songs(7000 + n + d, n, d, run=20 + (n + d) % 21)
    db.setflags(write=False)
    return db


def queries(db, nq, seed=7100):
    q = sb._queries(seed + nq + db.shape[1], db, nq)
    q[-1] = sb._unit(db[-1:].astype(np.float64) + 0.3 * q[-1:])[0]
    if nq > ZERO_ROW + 1:
        q[ZERO_ROW] = 0.0
    return q


def geometry_ranges(n, nq):
    """six ranges taken in turn (tests/test_gpu_search_excl.py, test_sampled_pass_with_a_row_stride): they begin and end on a
    db tile border (b is the first row of a 128-row tile, hence of a 64-row one) and beside it, one is a single row, and one
    sits at each end of the shard.  The last query row -- planted on the last database row -- loses that row."""
    b = 128 * max(1, (n // 128) // 3)
    pats = np.array([(b - 1, b + 1), (b + 1, b + 3), (b, b + 1), (b - 3, b + 200), (0, 5), (n - 3, n)], np.int64)
    lo, hi = (np.ascontiguousarray(pats[np.arange(nq) % len(pats), col]) for col in (0, 1))
    lo[-1], hi[-1] = pats[5]
    return lo, hi


def masked_queries(db, nq, lo):
    """every third query is the first row of its own range (its best matches are the excluded ones)"""
    q = queries(db, nq)
    third = np.arange(0, nq - 1, 3)
    third = third[third != ZERO_ROW]
    q[third] = db[lo[third]]
    return q


def check(torch, c, db, q):
    """the unmasked case against the reference of its storage -> (D, I)"""
    assert q.shape == (c.nq, c.d) and db.shape == (c.n, c.d) and not c.excl
    if c.storage == "copy":
        D, I, _ = sb._check(torch, db, q, c.k, c.name, path_of(c), c.kernels)
    elif c.storage == "f32":
        D, I = par._check_topk(torch, db, q, c.k, False, path_of(c), c.kernels)
    else:
        D, I, _ = par._check_topk_f16(torch, db, q, c.k, path_of(c), c.kernels)
    return D, I


def check_masked(torch, c, db, q, lo, hi):
    assert q.shape == (c.nq, c.d) and db.shape == (c.n, c.d) and c.excl
    idx = xt.make_index(db, c.storage)
    kind = xt.plan_of(idx, c.nq, c.k, path_of(c), c.kernels)
    assert kind == {"copy": "canonical", "f32": "f32", "f16": "f16"}[c.storage]
    D, I = xt.run(torch, idx, q, c.k, lo, hi)
    sx.assert_masked(D, I, q, db, c.k, lo, hi, kind, what=c.name)
    return D, I


def run_case(torch, c, db):
    if not c.excl:
        return check(torch, c, db, queries(db, c.nq))
    lo, hi = geometry_ranges(c.n, c.nq)
    return check_masked(torch, c, db, masked_queries(db, c.nq, lo), lo, hi)


# --------------------------------------------------------------------------------------------------- the streaming kernels
@pytest.mark.parametrize("c", skc.cases_of(T + "test_small_d64_fp32_streaming"), ids=ids)
def test_small_d64_fp32_streaming(torch_cuda, c):
    """scan_small_kernel<64, 4, 1> and <64, 4, 0>: d = 64, <= 32 query rows, fp32 rows without the pre-filter.  At 12288
    rows every wave of the 512 workgroups streams 6 rows, a workgroup 24, and workgroup b appends to sub-list b & 31: the 384
    rows r with (r / 24) % 32 == 5 are near-identical and all clear query row 0's threshold, 384 > the 256 slots of
    sub-list 5 -- the row is flagged and recomputed by topk_fallback_kernel<4> (the masked twins: row 0 leaves out the
    first 24 of the 384, and 360 still overflow)."""
    db = np.array(songs(c.n, c.d))
    centre = sb._unit(np.random.default_rng(5).standard_normal((1, c.d)))
    rows = np.flatnonzero((np.arange(c.n) // 24) % 32 == 5)
    assert rows.size == 384 > 8192 // 32
    db[rows] = sb._unit(centre + 0.01 * db[rows])
    lo, hi = geometry_ranges(c.n, c.nq)
    lo[0], hi[0] = rows[0], rows[0] + 24
    q = masked_queries(db, c.nq, lo) if c.excl else queries(db, c.nq)
    q[0] = sb._unit(centre + 0.05 * q[0:1])[0]
    D, I = check_masked(torch_cuda, c, db, q, lo, hi) if c.excl else check(torch_cuda, c, db, q)
    assert np.isin(I[0], rows[24:] if c.excl else rows).all(), "row 0's top-k are rows of the planted 384"
    assert lo[ZERO_ROW] > c.k and np.array_equal(I[ZERO_ROW], np.arange(c.k)), "every score ties: the lowest rows"


@pytest.mark.parametrize("c", skc.cases_of(T + "test_fp32_ladder_small_batch"), ids=ids)
def test_fp32_ladder_small_batch(torch_cuda, c):
    """scan_emit_kernel<32, 128, 32, 32, 1>: <= 32 query rows at a d the small path does not take (96)."""
    run_case(torch_cuda, c, songs(c.n, c.d))


@pytest.mark.parametrize("c", skc.cases_of(T + "test_small_d64_fp16_dense"), ids=ids)
def test_small_d64_fp16_dense(torch_cuda, c):
    """scan_small_kernel<64, 2, 2>: d = 64, fp16-only storage, one dense pass -- below the 256-thread select's 4096 rows
    (5000 is above, with a ragged last tile) and at n = CAP = 8192 with k = 1."""
    run_case(torch_cuda, c, songs(c.n, c.d))


# ------------------------------------------------------------------------------- long runs of query tiles per workgroup
@pytest.mark.parametrize("c", skc.cases_of(T + "test_long_query_tile_runs"), ids=ids)
def test_long_query_tile_runs(torch_cuda, c):
    """scan_emit_kernel<128, 128, 64, 64, 4> and scan_f16_kernel<4>: the full pass of the ladders once db tiles x
    ceil(query tiles / 4) reaches 4096 workgroups -- 2049 db tiles (the last one of 56 rows) x 2 here.  513 query rows are
    five query tiles: a full run of four, and a run of ONE tile whose only row, query 512, is planted on the last database
    row (masked: and loses it).  d = 36 is the fp32 ladder a default handle takes (no fp16 copy at d % 8 != 0); fp16-only
    storage runs the selects without re-scoring.
    d = 36 (fp32: K tiles of 32) and d = 96 (fp16: K tiles of 64) end in a K tile that is not full.  There the threads whose
    own k lies past d used to move their load cursor to the next query tile one K tile early, so the first three tiles of
    a full run were scored with operands of their neighbour: 511 of 513 rows came back wrong at d = 96, padded lists at
    d = 36.  Query 512 alone -- a run of one tile -- was right, which is why the shorter runs of the older tests (QT = 1)
    never showed it."""
    (full,) = [s for s in shape_plan(c)[0] if s[0] in c.kernels]
    assert full[1] == 2049 * 2, full
    D, I = run_case(torch_cuda, c, songs(c.n, c.d))
    if not c.excl:
        assert I[-1, 0] == c.n - 1, "query 512 finds the last database row"
    else:
        assert not (I[-1] >= c.n - 3).any() and I[-1, 0] >= c.n - 60, "query 512 finds the rest of the last song"


def test_masked_full_pass_on_two_tile_buffers(torch_cuda):
    """scan_f16_qres_kernel<8, false, 64, 2, true>: 12 query tiles x 64 slices = 768 workgroups, one full round of the
    resident ones -- the masked full pass on two tile buffers (the older masked cases all have fewer: three buffers)."""
    c = skc.case("dbr64_nbuf2_excl")
    run_case(torch_cuda, c, songs(c.n, c.d))


# ------------------------------------------------------------------------------------- the wave-per-row group select
@pytest.mark.parametrize("c", skc.cases_of(T + "test_wave_group_select_16"), ids=ids)
def test_wave_group_select_16(torch_cuda, c):
    """group_max_select_wave_kernel<16>: 513 .. 1024 group maxima per row, 16 per lane.  G = 1024 (8065 query rows: every
    lane holds 16) and G = 832 (9728 rows, the benchmark's launch group: 13 per lane).  A threshold a little too high loses
    true top-k rows silently: only the exact comparison notices.  Masked: query row 2 leaves out everything but k + 5 rows,
    so most of its group maxima are -inf (the select's shared-leading-bits shortcut on -inf keys)."""
    db = songs(c.n, c.d)
    flags = shape_plan(c)[1]
    assert int(flags["groups"]) == (1024 if c.nq == 8065 else 832), flags
    if not c.excl:
        run_case(torch_cuda, c, db)
        return
    lo, hi = geometry_ranges(c.n, c.nq)
    lo[2], hi[2] = 50, c.n - c.k - 5 + 50
    D, I = check_masked(torch_cuda, c, db, masked_queries(db, c.nq, lo), lo, hi)
    assert (I[2] >= 0).all() and ((I[2] < 50) | (I[2] >= hi[2])).all()


def exact_scores_desc(q, part, m, storage, rows=2048):
    """[nq, m] float64: the m largest exact scores of every query row against the shard, descending -- of the rows as the
    storage keeps them (fp16-only storage: fl16(q) . fl16(x), the score that storage defines)"""
    if storage == "f16":
        q, part = q.astype(np.float16), part.astype(np.float16)
    q64, x64 = q.astype(np.float64), part.astype(np.float64)
    out = np.empty((q.shape[0], m))
    for m0 in range(0, q.shape[0], rows):
        s = q64[m0:m0 + rows] @ x64.T
        out[m0:m0 + rows] = -np.sort(np.partition(-s, m - 1, axis=1)[:, :m], axis=1)
    return out


TOPM = {"wave_topm_copy": (skc.WAVE_TOPM, "copy", "group_max_select_wave_kernel<16>"),
        "wave_topm_f16": (skc.WAVE_TOPM, "f16", "group_max_select_wave_kernel<16>"),
        "wave8_topm": (skc.WAVE8_TOPM, "copy", "group_max_select_wave_kernel<8>")}


@pytest.mark.parametrize("prefix", sorted(TOPM))
def test_wave_group_select_topm(torch_cuda, prefix):
    """Phase 1 of the sharded search on the wave selects: with topm the group select also writes the m best group maxima
    of every row, each lowered to a bound of its exact score (pfann_search_bound).  9728 rows x three shards of ~8000 rows
    is what one rank of the multi-GPU benchmark runs (G = 832: <16>); 16384 rows on one shard give G = 512 (<8>).
      - the i-th largest returned value never exceeds the i-th largest EXACT score of the shard by more than the 1e-6
        test_two_phase_sharded_search_is_the_exact_global_topk allows, and exactly min(m, G) values are finite;
      - the reduced bound does not exceed the true global k-th best;
      - search_bounded + merge_topk is the unsplit search, labels and score bits; the unsplit search is the oracle's."""
    torch = torch_cuda
    spec, storage, kernel = TOPM[prefix]
    d, nq, k, cuts = spec["d"], spec["nq"], spec["k"], spec["cuts"]
    m = skc.bound_m(k, 3)
    db = songs(cuts[-1], d)
    q = queries(db, nq)
    whole_case = skc.case(prefix + "_whole")
    assert (whole_case.n, whole_case.nq, whole_case.k, whole_case.storage) == (cuts[-1], nq, k, storage)
    # the unsplit search against the oracle of the storage
    if storage == "copy":
        whole = sb._index(db)
        D0, I0 = sb._search(torch, whole, q, k)
        assert_canonical_topk(D0, I0, q, db, k, what=prefix + " unsplit")
    else:
        D0, I0, whole = par._check_topk_f16(torch, db, q, k)
    q_t = torch.as_tensor(q).cuda()
    db_t = torch.as_tensor(np.array(db)).cuda()
    shards, bounds = [], []
    for j, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        c1, c2 = skc.case("%s_shard%d_bound" % (prefix, j)), skc.case("%s_shard%d_bounded" % (prefix, j))
        assert (c1.n, c1.nq, c1.k, c1.mtop, c1.storage, c1.kernels) == (hi - lo, nq, k, m, storage, (kernel,)) and c2.n == hi - lo
        ix = xt.make_index(db_t[lo:hi].contiguous(), storage, lo) if storage == "f16" else sb._index(db_t[lo:hi].contiguous(), lo, lo)
        names, flags = sb._assert_plan(ix, nq, k, "gmax", [kernel], phase=1, mtop=m)
        assert flags["leaves_bound"] == "1" and names[-1] == kernel
        sb._assert_plan(ix, nq, k, "gmax", ["bound_in_kernel"], phase=2, resume_with_lb=True)
        G = int(flags["groups"])
        c = ix.search_bound(q_t, k, m)
        got = -np.sort(-c.cpu().numpy().astype(np.float64), axis=1)
        assert got.shape == (nq, m) and (np.isfinite(got).sum(1) == min(m, G)).all(), "shard %d: finite values per row" % j
        want = exact_scores_desc(q, db[lo:hi], m, storage)
        over = got - want
        assert over.max() <= 1e-6, "shard %d: a returned value exceeds the exact score of its rank by %g (row %d)" % (
            j, over.max(), int(np.argmax(over.max(1))))
        shards.append(ix)
        bounds.append(c)
    L = whole.reduce_bound(torch.stack(bounds), k)
    kth = torch.as_tensor(D0[:, k - 1]).cuda()
    assert bool((L <= kth + 1e-6).all()), "the reduced bound exceeds the true global k-th best"
    parts = [ix.search_bounded(q_t, k, L) for ix in shards]
    Dm, Im = whole.merge_topk(torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1), k)
    Dm, Im = Dm.cpu().numpy(), Im.cpu().numpy()
    assert np.array_equal(Dm.view(np.int32), D0.view(np.int32)), "two-phase score bits differ from the unsplit search"
    assert np.array_equal(Im, I0), "two-phase labels differ from the unsplit search"


# ----------------------------------------------------------------------------------------- a bound that bounds nothing
@pytest.mark.parametrize("n,d,nq,k,storage", skc.BOUND_NONE_SHAPES)
def test_bound_without_a_sampled_threshold(torch_cuda, n, d, nq, k, storage):
    """bound_none_kernel: pfann_search_bound on a shape without a sampled threshold (the small path, k > 128, fp32 rows
    only, an empty shard) returns -inf everywhere, its reduction is -FLT_MAX, the bounded search behind it is the plain
    search bit for bit, and it leaves no pending state: a following plain search is unchanged (and the oracle's)."""
    torch = torch_cuda
    m = skc.bound_m(k, 3)
    c = skc.case("bound_none_%d_%d_%d_%s" % (n, nq, k, storage))
    assert (c.n, c.d, c.nq, c.k, c.storage, c.mtop, c.phase) == (n, d, nq, k, storage, m, 1)
    db = songs(n, d) if n else np.zeros((0, d), np.float32)
    q = queries(db if n else songs(20000, d), nq)
    if n:
        idx = xt.make_index(db, storage)
    else:                                   # (an empty shard has no fp16 copy to switch on)
        from pfann_amd.database import DeviceIndex
        idx = DeviceIndex(d, 0)
        idx.load(db, np.array([0, 0], np.int64), 0)
    names, flags = sb._assert_plan(idx, nq, k, flags_path(idx, nq, k), c.kernels, phase=1, mtop=m)
    assert names[-1] == "bound_none_kernel" and flags["leaves_bound"] == "0"
    q_t = torch.as_tensor(q).cuda()
    D0, I0 = idx.search(q_t, k)
    lb = idx.search_bound(q_t, k, m)
    assert lb.shape == (nq, m) and bool((lb == float("-inf")).all())
    L = idx.reduce_bound(lb[None], k)
    assert L.shape == (nq,) and bool((L == -FLT_MAX).all())
    D1, I1 = idx.search_bounded(q_t, k, L)
    assert torch.equal(I1, I0) and torch.equal(D1.view(torch.int32), D0.view(torch.int32))
    D2, I2 = idx.search(q_t, k)
    assert torch.equal(I2, I0) and torch.equal(D2.view(torch.int32), D0.view(torch.int32))
    # ... and the plain search is the exact one
    D0, I0 = D0.cpu().numpy(), I0.cpu().numpy()
    if n == 0:
        assert (I0 == -1).all() and (D0 == -FLT_MAX).all()
    elif storage == "copy":
        assert_canonical_topk(D0, I0, q, db, k, what=c.name)
    else:
        par._check_topk(torch, db, q, k, False)


def flags_path(idx, nq, k):
    """the path of the plain search of the shape: phase 1 prints the same (small prints "small")"""
    path = idx.search_plan(nq, k)[1]["path"]
    return "small" if path.startswith("small") else path
