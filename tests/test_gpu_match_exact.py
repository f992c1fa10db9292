"""The sequence matcher (csrc/rerank.hip) against an exact oracle, on every launch plan.  Inputs lie on the grid of
tests/match_exact.py, where fp32 sums are exact in any order: every field of every result -- (song, offset, shift), the float64
score, n_cand and both columns of the per-song block -- is asserted with `==` against match_exact.exact_match, and fp16-only
storage must return the very bytes of fp32 storage.  Labels are constructed (not searched), each generator stressing one
thing: ties, edges of songs, -1 labels, collapsed and full candidate lists, the coarse song table.  Every case asserts the plan
it was written for (match_exact.match_plan).  The one tolerance in this module is the project's 2e-6 under score_alpha > 0
(expf), tests/test_gpu_parity.py::test_seq_score_c_abi_vs_oracle."""
import functools

import numpy as np
import pytest

import match_exact as mx

pytestmark = pytest.mark.gpu

GENS = ("aligned", "tie_storm", "edges", "collapse", "full")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _ragged(n, lo=1, hi=19):
    return [lo + (7 * j + 3) % (hi - lo + 1) for j in range(n)]


# shape -> (plan, qlens, k, qlens and k of the `full` generator: qlen * k a power of two)
SHAPES = {
    "lds_small": ("phased_lds", [1, 5, 9, 13, 17, 21, 25, 7, 25, 3, 11, 19], 20, [16, 8, 1, 4], 32),
    "lds_k1": ("phased_lds", [1, 2, 19, 7, 12, 16, 4, 9], 1, [16, 1, 8, 2], 1),
    # a short query (P < pmax / 32: whole slices return early, lanes of the first are not live) among long ones, P == pmax
    "rank1024": ("phased_rank", [64, 1, 50, 33, 64, 17], 16, [64, 1, 32, 64], 16),
    "rank2048": ("phased_rank", [64, 1, 40, 64, 23], 32, [64, 1, 16], 32),
    "rank4096": ("phased_rank", [64, 1, 64, 37], 64, [64, 2, 32], 64),
    "lds8192": ("phased_lds", [128, 3, 90, 128], 64, [128, 16], 64),          # 8 keys per thread in the compaction
    "hbm": ("phased_hbm", [119, 9, 160], 100, [128, 8], 128),                 # second-sort dedup, with a 9-row query
    "single65": ("single_lds", _ragged(65), 100, [16, 8, 4, 2, 1] * 13, 128),
    "single200": ("single_lds", _ragged(200), 100, [16, 8, 4, 2, 1] * 40, 128),
    "single1000": ("single_lds", _ragged(1000), 20, [16, 8, 4, 2, 1] * 200, 16),
    "single_hbm": ("single_hbm", [100] + _ragged(64), 100, [128] + [8, 4, 2, 1] * 16, 128),
}


def plan_shapes():
    """(plan, nQ, max_qlen, k) of every call this module makes on the shapes above"""
    out = []
    for plan, qlens, k, fq, fk in SHAPES.values():
        out += [(plan, len(qlens), max(qlens), k), (plan, len(fq), max(fq), fk)]
    return out


@functools.lru_cache(maxsize=None)
def _world(d, long_rows=0):
    return mx.std_world(41, d, long_rows)


@functools.lru_cache(maxsize=None)
def _rows(d, long_rows=0):
    return mx.IntRows(_world(d, long_rows)[0])


_INDEX = {}


def _index(key, db, pos, storage="f32", label_base=0, song_range=None):
    from pfann_amd.database import DeviceIndex
    key = (key, storage, label_base)
    if key not in _INDEX:
        idx = DeviceIndex(db.shape[1], 0, storage)
        idx.load(db, pos, label_base, song_range=song_range)
        _INDEX[key] = idx
    return _INDEX[key]


def _batch(gen, shape, d, fsm, seed=0):
    """-> (world key, db, pos, exact rows, batch, k, plan)"""
    plan, qlens, k, fq, fk = SHAPES[shape]
    long_rows = 6000 if gen == "full" else 0
    db, pos = _world(d, long_rows)
    seed += 100 + 7 * sorted(SHAPES).index(shape)
    if gen == "aligned":
        b = mx.aligned(seed, db, pos, qlens, k, fsm)
    elif gen == "tie_storm":
        b = mx.tie_storm(seed, db, pos, qlens, k, mx.STD_COPIES, mx.STD_PERIODIC, fsm)
    elif gen == "edges":
        b = mx.edges(seed, db, pos, qlens, k, fsm)
    elif gen == "collapse":
        b = mx.collapse(seed, db, pos, qlens, k, fsm)
    else:
        b, k = mx.full(seed, db, pos, fq, fk, fsm), fk
    return (d, long_rows), db, pos, _rows(d, long_rows), b, k, plan


def _match(torch, idx, b, fsm, mode, alpha=0.0, only_owned=False, owned_block=False):
    res, ss = idx.match(torch.as_tensor(b.q).cuda(), torch.as_tensor(b.labels).cuda(), b.qstart, b.qlen, fsm, alpha, mode,
                        only_owned, True, owned_block=owned_block)
    return res, ss.cpu().numpy()


def _assert_exact(res, ss, want, what, lo=0, hi=None, n_cand=True):
    """every field of every query, no tolerance; the message names the query, the plan, both candidates and the oracle's
    three best"""
    bad = []
    for j, w in enumerate(want):
        r = res[j]
        got = (int(r["song"]), int(r["offset"]), int(r["shift"]), float(r["score"]), int(r["n_cand"]) if n_cand else None)
        exp = (w["song"], w["offset"], w["shift"], w["score"], w["n_cand"] if n_cand else None)
        if got != exp:
            bad.append("query %d: kernel (song, offset, shift, score, n_cand) %r, oracle %r, oracle's best three %r"
                       % (j, got, exp, w["top"]))
        if ss is not None and not np.array_equal(ss[j], w["ss"][lo:hi]):
            s = np.flatnonzero((ss[j] != w["ss"][lo:hi]).any(1))
            bad.append("query %d: per-song block differs for %d songs, first %d: kernel %r, oracle %r, oracle's best three %r"
                       % (j, s.size, s[0] + lo, ss[j][s[0]].tolist(), w["ss"][lo:hi][s[0]].tolist(), w["top"]))
    assert not bad, "%s: %d of %d queries differ\n%s" % (what, len({b.split(":")[0] for b in bad}), len(want), "\n".join(bad[:8]))


def _case(torch, gen, shape, d, fsm=1, mode=0, storages=("f32",)):
    wkey, db, pos, rows, b, k, plan = _batch(gen, shape, d, fsm)
    got_plan = mx.match_plan(len(b.qlen), max(b.qlen), k)[0]
    assert got_plan == plan, "%s/%s was written for %s and would now take %s" % (shape, gen, plan, got_plan)
    mx.assert_exact_domain(max(b.qlen), d)
    want = mx.exact_batch(b, rows, pos, fsm, mode)
    first = None
    for storage in storages:
        res, ss = _match(torch, _index(wkey, db, pos, storage), b, fsm, mode)
        _assert_exact(res, ss, want, "%s %s d=%d fsm=%d mode=%d %s (%s)" % (shape, gen, d, fsm, mode, storage, plan))
        if first is None:
            first = (res.tobytes(), ss.tobytes())
        else:
            assert (res.tobytes(), ss.tobytes()) == first, "fp16-only storage and fp32 storage return different bytes"
    return want


# ------------------------------------------------------------------------------------------------ plan x generator
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_plan_is_exact_python_path(torch_cuda, shape, gen, d):
    """mode 0, fsm 1, fp32 storage, per-song block: the contiguous fast path of the scoring loop and the run-head replay"""
    want = _case(torch_cuda, gen, shape, d)
    if gen == "full":
        assert all(w["n_cand"] == n * SHAPES[shape][4] for w, n in zip(want, SHAPES[shape][3]))
    if gen == "collapse":
        assert all(w["n_cand"] == 1 for w in want)


MODE_FSM = [(0, 2), (0, 3), (1, 1), (1, 2), (1, 3)]


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("mode,fsm", MODE_FSM)
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", ["lds_small", "rank2048", "single65", "hbm"])
def test_modes_and_frame_shifts_are_exact(torch_cuda, shape, gen, mode, fsm, d):
    """both candidate orders and division rules, the row-by-row scoring loop (fsm > 1), the three per-song replays"""
    _case(torch_cuda, gen, shape, d, fsm, mode)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", ["lds_small", "rank2048", "single65", "hbm"])
def test_fp16_storage_returns_the_bytes_of_fp32_storage(torch_cuda, shape, gen, mode, fsm, d):
    """grid rows are exact in fp16: the fp16-only shard must give the oracle's answer and fp32 storage's bytes"""
    _case(torch_cuda, gen, shape, d, fsm, mode, storages=("f32", "f16"))


@pytest.mark.parametrize("d", [96, 16])
@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("shape", ["lds_small", "rank2048", "single65"])
def test_other_row_widths_are_exact(torch_cuda, shape, mode, fsm, d):
    """d = 96 (one and a half waves per row in the row loop, 24 chunks per row in the fast path) and d = 16"""
    for gen in GENS:
        _case(torch_cuda, gen, shape, d, fsm, mode, storages=("f32", "f16"))


# ------------------------------------------------------------------------------------------------ the song table
@pytest.mark.parametrize("n_songs", mx.LADDER)
def test_song_lookup_across_coarse_table_shapes(torch_cuda, n_songs):
    """labels on the first and last rows of the songs around coarse-table entries, 1 .. 5000 songs of 0..3 rows"""
    d = 64
    db, pos = mx.ladder_world(51, n_songs, d)
    rows = mx.IntRows(db)
    for plan, qlens, k in (("phased_lds", [1, 4, 7, 9, 3, 5, 12], 24), ("single_lds", _ragged(65, 1, 12), 24)):
        for mode, fsm in ((0, 1), (1, 2)):
            b = mx.ladder(52 + fsm, db, pos, qlens, k, fsm)
            assert mx.match_plan(len(qlens), max(qlens), k)[0] == plan
            res, ss = _match(torch_cuda, _index(("ladder", n_songs), db, pos), b, fsm, mode)
            _assert_exact(res, ss, mx.exact_batch(b, rows, pos, fsm, mode), "ladder %d songs %s mode=%d fsm=%d" % (n_songs, plan, mode, fsm))


# ------------------------------------------------------------------------------------------------ plans agree
@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_phased_and_single_launch_return_the_same_bytes(torch_cuda, mode, fsm):
    """48 queries alone (phased, rank sort) and as the head of a batch of 200 (single launch): same bytes, both the oracle's"""
    d, k = 128, 100
    db, pos = _world(d)
    ql = _ragged(200)
    head = [mx.tie_storm(61, db, pos, ql[:16], k, mx.STD_COPIES, mx.STD_PERIODIC, fsm), mx.edges(62, db, pos, ql[16:32], k, fsm),
            mx.aligned(63, db, pos, ql[32:48], k, fsm)]
    tail = mx.aligned(64, db, pos, ql[48:], k, fsm)

    def cat(parts):
        qlen = [n for p in parts for n in p.qlen]
        return mx.Batch(np.concatenate([p.q for p in parts]), np.concatenate([p.labels for p in parts]),
                        [int(x) for x in np.pad(np.cumsum(qlen), (1, 0))[:-1]], qlen)
    small, big = cat(head), cat(head + [tail])
    assert mx.match_plan(48, max(small.qlen), k)[0] == "phased_rank" and mx.match_plan(200, max(big.qlen), k)[0] == "single_lds"
    idx = _index((d, 0), db, pos)
    r1, s1 = _match(torch_cuda, idx, small, fsm, mode)
    r2, s2 = _match(torch_cuda, idx, big, fsm, mode)
    want = mx.exact_batch(big, _rows(d), pos, fsm, mode)
    _assert_exact(r1, s1, want[:48], "48 alone mode=%d fsm=%d" % (mode, fsm))
    _assert_exact(r2, s2, want, "head of 200 mode=%d fsm=%d" % (mode, fsm))
    assert r1.tobytes() == r2[:48].tobytes() and s1.tobytes() == s2[:48].tobytes()


# ------------------------------------------------------------------------------------------------ owner side
def owner_world(d):
    """the standard world with song 16 grown until dist.shard_songs(., 3) cuts at song 17, which has no rows"""
    from pfann_amd.dist import shard_songs
    key = [int(x) for x in np.diff(_world(d)[1])]
    for _ in range(400):
        db, pos = mx.make_world(43, "own%d" % d, key, d, mx.STD_COPIES, mx.STD_PERIODIC)
        cuts = shard_songs(pos, 3)
        if cuts[1][0] == 17:
            return db, pos, cuts
        key[16] += 1
    raise AssertionError("no cut at the rowless song")


@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1)])
@pytest.mark.parametrize("gen", ["tie_storm", "edges"])
def test_owner_side_shards_and_winner_keys(torch_cuda, gen, mode, fsm):
    """three shards, each loaded with label_base and its song range: only_owned candidates and the owned score block equal the
    oracle restricted to the shard's songs; the 128-bit winner keys pick the unsharded oracle's answer, ties across shards
    included"""
    torch = torch_cuda
    d, k = 64, 20
    db, pos, cuts = owner_world(d)
    assert pos[17] == pos[18] and cuts[1][0] == 17
    qlens = _ragged(40)
    if gen == "tie_storm":
        b = mx.tie_storm(71, db, pos, qlens, k, mx.STD_COPIES, mx.STD_PERIODIC, fsm)
    else:
        b = mx.edges(72, db, pos, qlens, k, fsm)
    rows = mx.IntRows(db)
    whole = mx.exact_batch(b, rows, pos, fsm, mode)
    keys, bests = [], []
    for lo, hi in cuts:
        r_lo, r_hi = int(pos[lo]), int(pos[hi])
        idx = _index(("owner", lo), db[r_lo:r_hi], pos, "f32", r_lo, (lo, hi))
        assert idx.owned_songs() == (lo, hi)
        res_dev, ss = idx.match(torch.as_tensor(b.q).cuda(), torch.as_tensor(b.labels).cuda(), b.qstart, b.qlen, fsm, 0.0, mode,
                                True, True, to_host=False, owned_block=True)
        want = mx.exact_batch(b, rows, pos, fsm, mode, (lo, hi))
        _assert_exact(idx.results_to_host(res_dev), ss.cpu().numpy(), want, "shard songs [%d, %d) %s mode=%d fsm=%d" % (lo, hi, gen, mode, fsm),
                      lo, hi)
        keys.append(idx.pack_winner_keys(res_dev))
        bests.append([w["score"] if w["song"] >= 0 else None for w in want])
    win = idx.pick_winner(torch.stack(keys))
    _assert_exact(win, None, whole, "winner over 3 shards %s mode=%d fsm=%d" % (gen, mode, fsm), n_cand=False)
    across = sum(1 for j, w in enumerate(whole) if sum(1 for s in bests if s[j] == w["score"]) >= 2)
    if gen == "tie_storm":
        assert across >= 3, "only %d queries tie across two shards" % across


# ------------------------------------------------------------------------------------------------ score_alpha > 0
ALPHA = 3.0
ALPHA_TOL = 2e-6         # tests/test_gpu_parity.py::test_seq_score_c_abi_vs_oracle


def alpha_case(d, fsm):
    """unit-norm grid rows (score_alpha's exp(-alpha (1 - ip)^2) needs them), copied songs, 150 aligned + 50 tie queries.
    -> (db, pos, batch, number of leading `aligned` queries)"""
    key = [int(x) for x in np.diff(_world(d)[1])]
    db, pos = mx.make_world(81, "alpha%d" % d, key, d, mx.STD_COPIES, (), rows=mx.unit_grid_rows)
    k = 20
    a = mx.aligned(82, db, pos, _ragged(150, 2, 19), k, fsm)
    t = mx.tie_storm(83, db, pos, _ragged(50, 2, 19), k, mx.STD_COPIES, (), fsm, kinds=(4,))
    qlen = a.qlen + t.qlen
    b = mx.Batch(np.concatenate([a.q, t.q]), np.concatenate([a.labels, t.labels]),
                 [int(x) for x in np.pad(np.cumsum(qlen), (1, 0))[:-1]], qlen)
    return db, pos, b, len(a.qlen)


def alpha_oracle(db, pos, b, fsm):
    """the C oracle alone: [(best song, block, gap between the best song's score and the best other song's, its copy aside)]"""
    from oracle import native
    out = []
    for s, n in zip(b.qstart, b.qlen):
        best, ss = native.seq_score(db, pos, b.q[s:s + n], b.labels[s:s + n], fsm, ALPHA)
        twin = [x for src, dst in mx.STD_COPIES for x, y in ((src, dst), (dst, src)) if y == best]
        others = np.delete(ss[:, 0], [best] + twin)         # (a song and its copy tie exactly)
        out.append((best, ss, float(ss[best, 0]) - float(others.max()) if others.size else np.inf))
    return out


def _alpha_score64(db, pos, q, song, off, shift, fsm):
    sub = q[shift::fsm].astype(np.float64)
    tot = 0.0
    for j in range(sub.shape[0]):
        if 0 <= off + j < pos[song + 1] - pos[song]:
            tot += np.exp(-ALPHA * (1.0 - float(sub[j] @ db[pos[song] + off + j].astype(np.float64))) ** 2)
    return tot / max(sub.shape[0], 1)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("fsm", [1, 2])
def test_score_alpha_against_the_c_oracle(torch_cuda, fsm, d):
    """mode 1, score_alpha 3: the one non-exact case (expf).  Score column within 2e-6 of oracle/seqscore_c.c, alignment column
    equal; the decision is the oracle's, or (second branch) a candidate whose score restated in float64 is within 2e-6 of the
    oracle's best -- at most 1 % of the queries may take it, and the inputs keep the oracle's own best-to-runner-up gap above
    2e-6 for at least 99 % (tests/test_match_exact.py checks that on the CPU).  The count of second-branch queries is
    printed; measured on an MI355X: 0 of 200 for each of d 64 / 128 x fsm 1 / 2.Queries cut from copied songs tie bit for bit (same rows, same operations) and must go to the smaller song."""
    db, pos, b, n_al = alpha_case(d, fsm)
    assert mx.match_plan(len(b.qlen), max(b.qlen), 20)[0] == "single_lds"
    res, ss = _match(torch_cuda, _index(("alpha", d), db, pos), b, fsm, 1, ALPHA)
    want = alpha_oracle(db, pos, b, fsm)
    copies = {dst: src for src, dst in mx.STD_COPIES}
    second = other_alignments = 0
    for j, (best, wss, gap) in enumerate(want):
        q = b.q[b.qstart[j]:b.qstart[j] + b.qlen[j]]
        assert np.allclose(ss[j][:, 0], wss[:, 0], atol=ALPHA_TOL, rtol=0), j
        for s in np.flatnonzero(ss[j][:, 1] != wss[:, 1]):       # another alignment of the song: only if it scores the same
            fine = int(ss[j][s, 1])
            s64 = _alpha_score64(db, pos, q, int(s), (fine + (-fine) % fsm) // fsm, (-fine) % fsm, fsm)
            assert abs(s64 - float(wss[s, 0])) <= ALPHA_TOL, (j, int(s), fine, s64, float(wss[s, 0]))
            other_alignments += 1
        r = res[j]
        if j >= n_al:                                   # cut from a copied song: an exact tie, the smaller song wins
            dst = [x for x, src in copies.items() if src == best]
            assert int(r["song"]) == best and dst, (j, int(r["song"]), best)
            assert ss[j][best, 0] == ss[j][dst[0], 0] > 0, j
            continue
        if int(r["song"]) != best:
            second += 1
            s64 = _alpha_score64(db, pos, q, int(r["song"]), int(r["offset"]), int(r["shift"]), fsm)
            assert abs(s64 - float(wss[best, 0])) <= ALPHA_TOL, (j, int(r["song"]), best, s64, float(wss[best, 0]))
    print("score_alpha d=%d fsm=%d: %d of %d queries took the second branch, %d per-song alignments differ at equal score"
          % (d, fsm, second, len(want), other_alignments))
    assert second * 100 <= len(want)


# ------------------------------------------------------------------------------------------------ the d % 4 guard
def test_match_refuses_rows_that_are_not_float4_multiples(torch_cuda):
    """the contiguous scoring path reads rows as float4: d % 4 != 0 is an error of pfann_match (no launch), as it is of the
    search"""
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    d = 6
    db = mx.grid_rows(91, "d6", 40, d)
    idx = DeviceIndex(d, 0)
    idx.load(db, np.array([0, 25, 40], np.int64), 0)
    q = torch_cuda.as_tensor(db[3:8]).cuda()
    labels = torch_cuda.as_tensor(np.arange(3, 8, dtype=np.int64)[:, None]).cuda()
    with pytest.raises(L.PfannError, match="d % 4"):
        idx.match(q, labels, [0], [5])
