"""Ranked top-N answers (pfann_match_topn, csrc/rerank.hip) against the exact oracle of tests/match_topn_exact.py, on every
launch plan of the matcher.  Inputs lie on the grid of tests/match_exact.py, where fp32 sums are exact in any order: every
field of every entry and n_found are asserted with `==`.  The one tolerance is the project's 2e-6 under score_alpha > 0 (expf),
as in tests/test_gpu_match_exact.py."""
import ctypes
import functools

import numpy as np
import pytest

import match_exact as mx
import match_topn_exact as tx

pytestmark = pytest.mark.gpu

GENS = ("aligned", "tie_storm", "edges", "collapse")
NS = (1, 5, 64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _ragged(n, lo=1, hi=19):
    return [lo + (7 * j + 3) % (hi - lo + 1) for j in range(n)]


# shape -> (plan, qlens, k): rows of tests/test_gpu_match_exact.py's table
SHAPES = {
    "lds_small": ("phased_lds", [1, 5, 9, 13, 17, 21, 25, 7, 25, 3, 11, 19], 20),
    "rank2048": ("phased_rank", [64, 1, 40, 64, 23], 32),
    "lds8192": ("phased_lds", [128, 3, 90, 128], 64),
    "hbm": ("phased_hbm", [119, 9, 160], 100),
    "single65": ("single_lds", _ragged(65), 100),
    "single_hbm": ("single_hbm", [100] + _ragged(64), 100),
}


@functools.lru_cache(maxsize=None)
def _world(d):
    return mx.std_world(41, d)


@functools.lru_cache(maxsize=None)
def _rows(d):
    return mx.IntRows(_world(d)[0])


_INDEX = {}


def _index(key, db, pos, storage="f32", label_base=0, song_range=None):
    from pfann_amd.database import DeviceIndex
    key = (key, storage, label_base)
    if key not in _INDEX:
        idx = DeviceIndex(db.shape[1], 0, storage)
        idx.load(db, pos, label_base, song_range=song_range)
        _INDEX[key] = idx
    return _INDEX[key]


def _gen(gen, seed, db, pos, qlens, k, fsm):
    if gen == "aligned":
        return mx.aligned(seed, db, pos, qlens, k, fsm)
    if gen == "tie_storm":
        return mx.tie_storm(seed, db, pos, qlens, k, mx.STD_COPIES, mx.STD_PERIODIC, fsm)
    if gen == "edges":
        return mx.edges(seed, db, pos, qlens, k, fsm)
    return mx.collapse(seed, db, pos, qlens, k, fsm)


@functools.lru_cache(maxsize=None)
def _batch(gen, shape, d, fsm, mode):
    """-> (batch, k, plan, the oracle's top 64 of every query): computed once, shared by every n and storage"""
    plan, qlens, k = SHAPES[shape]
    db, pos = _world(d)
    b = _gen(gen, 100 + 7 * sorted(SHAPES).index(shape), db, pos, qlens, k, fsm)
    mx.assert_exact_domain(max(b.qlen), d)
    return b, k, plan, tx.exact_topn_batch(b, _rows(d), pos, fsm, mode, 64)


def _cut(want, n):
    """the oracle's top 64 -> its top n (a prefix, by definition of the ranking)"""
    return [dict(top=w["top"][:n], n_found=w["n_found"], f32_alone=w["f32_alone"][:n]) for w in want]


def _topn(torch, idx, b, n, fsm, mode, alpha=0.0, only_owned=False):
    return idx.match_topn(torch.as_tensor(b.q).cuda(), torch.as_tensor(b.labels).cuda(), b.qstart, b.qlen, n, fsm, alpha, mode,
                          only_owned)


def _assert_exact(top, n_found, want, what):
    bad = []
    for j, w in enumerate(want):
        got = [tuple(x.item() for x in (e["song"], e["offset"], e["shift"], e["n_cand"], e["score"])) for e in top[j]]
        if got != w["top"]:
            i = next(i for i, (g, e) in enumerate(zip(got, w["top"])) if g != e)
            bad.append("query %d entry %d: kernel (song, offset, shift, n_cand, score) %r, oracle %r" % (j, i, got[i], w["top"][i]))
        if int(n_found[j]) != w["n_found"]:
            bad.append("query %d: n_found %d, oracle %d" % (j, int(n_found[j]), w["n_found"]))
    assert not bad, "%s: %d of %d queries differ\n%s" % (what, len({b.split(":")[0].split(" entry")[0] for b in bad}), len(want),
                                                         "\n".join(bad[:8]))


def _case(torch, gen, shape, d, fsm=1, mode=0, storages=("f32",), ns=NS):
    b, k, plan, want = _batch(gen, shape, d, fsm, mode)
    got_plan = mx.match_plan(len(b.qlen), max(b.qlen), k)[0]
    assert got_plan == plan, "%s/%s was written for %s and would now take %s" % (shape, gen, plan, got_plan)
    db, pos = _world(d)
    for n in ns:
        first = None
        for storage in storages:
            top, nf = _topn(torch, _index(d, db, pos, storage), b, n, fsm, mode)
            assert top.shape == (len(b.qlen), n)
            _assert_exact(top, nf, _cut(want, n), "%s %s d=%d fsm=%d mode=%d n=%d %s (%s)" % (shape, gen, d, fsm, mode, n, storage, plan))
            if first is None:
                first = (top.tobytes(), nf.tobytes())
            else:
                assert (top.tobytes(), nf.tobytes()) == first, "fp16-only storage and fp32 storage return different bytes"


# ------------------------------------------------------------------------------------------------ plan x generator
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_every_plan_is_exact(torch_cuda, shape, gen, d):
    """mode 0, fsm 1, n = 1, 5 and 64 on the LDS list, the HBM slab and the three-launch form with both phase-1 variants"""
    _case(torch_cuda, gen, shape, d)


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("mode,fsm", [(0, 2), (0, 3), (1, 1), (1, 2)])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", ["lds_small", "rank2048", "single65", "hbm"])
def test_modes_and_frame_shifts_are_exact(torch_cuda, shape, gen, mode, fsm, d):
    """both candidate orders; mode 0 with fsm > 1: a song recurs once per shift and must still be ONE entry"""
    _case(torch_cuda, gen, shape, d, fsm, mode)


@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 2)])
@pytest.mark.parametrize("gen", GENS)
@pytest.mark.parametrize("shape", ["lds_small", "rank2048", "single65", "hbm"])
def test_fp16_storage_returns_the_bytes_of_fp32_storage(torch_cuda, shape, gen, mode, fsm):
    _case(torch_cuda, gen, shape, 64, fsm, mode, storages=("f32", "f16"), ns=(5,))


# ------------------------------------------------------------------------------------------------ plans agree
@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_phased_and_single_launch_return_the_same_bytes(torch_cuda, mode, fsm):
    """64 queries alone (phased, rank sort) and followed by a copy of the first as the 65th (single launch): same bytes, both
    the oracle's"""
    d, k, n = 128, 100, 10
    db, pos = _world(d)
    ql = _ragged(64)
    parts = [mx.tie_storm(61, db, pos, ql[:24], k, mx.STD_COPIES, mx.STD_PERIODIC, fsm), mx.edges(62, db, pos, ql[24:44], k, fsm),
             mx.aligned(63, db, pos, ql[44:], k, fsm)]
    qlen = [m for p in parts for m in p.qlen]
    q, labels = np.concatenate([p.q for p in parts]), np.concatenate([p.labels for p in parts])
    small = mx.Batch(q, labels, [int(x) for x in np.pad(np.cumsum(qlen), (1, 0))[:-1]], qlen)
    big = mx.Batch(np.concatenate([q, q[:qlen[0]]]), np.concatenate([labels, labels[:qlen[0]]]),
                   small.qstart + [int(sum(qlen))], qlen + [qlen[0]])
    assert mx.match_plan(64, max(qlen), k)[0] == "phased_rank" and mx.match_plan(65, max(qlen), k)[0] == "single_lds"
    idx = _index(d, db, pos)
    t1, f1 = _topn(torch_cuda, idx, small, n, fsm, mode)
    t2, f2 = _topn(torch_cuda, idx, big, n, fsm, mode)
    want = tx.exact_topn_batch(big, _rows(d), pos, fsm, mode, n)
    _assert_exact(t1, f1, want[:64], "64 alone mode=%d fsm=%d" % (mode, fsm))
    _assert_exact(t2, f2, want, "65 mode=%d fsm=%d" % (mode, fsm))
    assert t1.tobytes() == t2[:64].tobytes() and f1.tobytes() == f2[:64].tobytes()
    assert t2[64].tobytes() == t2[0].tobytes()


# ------------------------------------------------------------------------------------------------ the same call of pfann_match
@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1), (1, 2)])
@pytest.mark.parametrize("shape", ["lds_small", "single65"])
def test_entry_0_is_pfann_match_and_scores_are_its_block(torch_cuda, shape, mode, fsm):
    """entry 0 == pfann_match's result; float32(score) of every entry that is > 0 == the per-song block's slot, the songs with
    such a score are the block's non-zero songs (n >= n_found), and the alignment is the block's wherever no other candidate of
    the song rounds to the same float32"""
    torch, d, n = torch_cuda, 64, 64
    db, pos = _world(d)
    idx = _index(d, db, pos)
    for gen in GENS:
        b, k, plan, want = _batch(gen, shape, d, fsm, mode)
        top, nf = _topn(torch, idx, b, n, fsm, mode)
        res, ss = idx.match(torch.as_tensor(b.q).cuda(), torch.as_tensor(b.labels).cuda(), b.qstart, b.qlen, fsm, 0.0, mode, False, True)
        ss = ss.cpu().numpy()
        for j in range(len(b.qlen)):
            for f in ("song", "offset", "shift", "score"):
                assert top[j, 0][f] == res[j][f], (gen, j, f, top[j, 0], res[j])
            assert nf[j] <= n
            s32 = top[j]["score"].astype(np.float32)
            pos32 = (top[j]["song"] >= 0) & (s32 > 0)
            songs = top[j]["song"][pos32]
            assert np.array_equal(s32[pos32], ss[j][songs, 0]), (gen, j)
            assert set(songs.tolist()) == set(np.flatnonzero(ss[j][:, 0] > 0).tolist()), (gen, j)
            alone = np.asarray(want[j]["f32_alone"]) & pos32
            fine = (top[j]["offset"] * fsm - top[j]["shift"]).astype(np.float32)
            assert np.array_equal(fine[alone], ss[j][top[j]["song"][alone], 1]), (gen, j)


# ------------------------------------------------------------------------------------------------ owner side
def _order_key(e, mode):
    return (e[2], e[0], e[1]) if mode == 0 else (e[0], e[1], e[2])


@pytest.mark.parametrize("mode,fsm", [(0, 1), (0, 2), (1, 1)])
@pytest.mark.parametrize("gen", ["tie_storm", "edges"])
def test_only_owned_lists_merge_to_the_unsharded_list(torch_cuda, gen, mode, fsm):
    """two shards, each loaded with label_base and its song range: a shard's list holds only its songs and equals the oracle
    restricted to them; the exact merge of the two lists in ranking order is the unsharded list"""
    from pfann_amd.dist import shard_songs
    d, k, n = 64, 20, 5
    db, pos = _world(d)
    cuts = shard_songs(pos, 2)
    b = _gen(gen, 71, db, pos, _ragged(40), k, fsm)
    rows = _rows(d)
    whole, whole_nf = _topn(torch_cuda, _index(d, db, pos), b, n, fsm, mode)
    _assert_exact(whole, whole_nf, tx.exact_topn_batch(b, rows, pos, fsm, mode, n), "unsharded %s" % gen)
    lists, founds = [], []
    for lo, hi in cuts:
        r_lo, r_hi = int(pos[lo]), int(pos[hi])
        idx = _index(("own", lo), db[r_lo:r_hi], pos, "f32", r_lo, (lo, hi))
        top, nf = _topn(torch_cuda, idx, b, n, fsm, mode, only_owned=True)
        _assert_exact(top, nf, tx.exact_topn_batch(b, rows, pos, fsm, mode, n, (lo, hi)), "shard songs [%d, %d) %s" % (lo, hi, gen))
        assert ((top["song"] == -1) | ((top["song"] >= lo) & (top["song"] < hi))).all()
        lists.append(top)
        founds.append(nf)
    assert np.array_equal(founds[0] + founds[1], whole_nf)
    for j in range(len(b.qlen)):
        ent = [tuple(x.item() for x in (e["song"], e["offset"], e["shift"], e["n_cand"], e["score"])) for t in lists for e in t[j]
               if e["song"] >= 0]
        ent.sort(key=lambda e: (-e[4], _order_key(e, mode)))
        merged = (ent + [tx.PAD] * n)[:n]
        got = [tuple(x.item() for x in (e["song"], e["offset"], e["shift"], e["n_cand"], e["score"])) for e in whole[j]]
        assert merged == got, (j, merged, got)


# ------------------------------------------------------------------------------------------------ score_alpha > 0
@pytest.mark.parametrize("fsm", [1, 2])
def test_score_alpha_against_the_c_oracle(torch_cuda, fsm):
    """mode 1, score_alpha 3 (expf: the one non-exact case): scores within 2e-6 of oracle/seqscore_c.c's per-song block; songs
    and their order equal the oracle's at every rank whose score is more than 2e-6 away from both neighbours in the oracle's
    ranking (copied songs tie exactly and are skipped by that rule)"""
    import test_gpu_match_exact as tg
    d, n = 64, 5
    db, pos, b, _ = tg.alpha_case(d, fsm)
    top, nf = _topn(torch_cuda, _index(("alpha", d), db, pos), b, n, fsm, 1, tg.ALPHA)
    checked = 0
    for j, (best, wss, gap) in enumerate(tg.alpha_oracle(db, pos, b, fsm)):
        order = [s for s in np.argsort(-wss[:, 0].astype(np.float64), kind="stable") if wss[s, 0] > 0]
        sc = [float(wss[s, 0]) for s in order]
        for i in range(n):
            e = top[j, i]
            if e["song"] < 0:
                assert i >= len(order), (j, i)
                continue
            assert abs(float(np.float32(e["score"])) - float(wss[e["song"], 0])) <= tg.ALPHA_TOL, (j, i, e, float(wss[e["song"], 0]))
            if i < len(order) and (i == 0 or sc[i - 1] - sc[i] > tg.ALPHA_TOL) and (i + 1 >= len(sc) or sc[i] - sc[i + 1] > tg.ALPHA_TOL):
                assert int(e["song"]) == int(order[i]), (j, i, e, order[:n], sc[:n])
                checked += 1
    assert checked >= len(b.qlen), "only %d ranks had a decisive gap" % checked


# ------------------------------------------------------------------------------------------------ refusals
def _raw_call(torch, idx, b, n, max_qlen, only_owned=0):
    q, labels = torch.as_tensor(b.q).cuda(), torch.as_tensor(b.labels).cuda()
    qs, ql = torch.as_tensor(np.asarray(b.qstart, np.int64)).cuda(), torch.as_tensor(np.asarray(b.qlen, np.int32)).cuda()
    nQ = len(b.qlen)
    top = torch.full((nQ, max(n, 1), 24), 0x5A, dtype=torch.uint8, device="cuda")
    nf = torch.full((nQ,), 77, dtype=torch.int32, device="cuda")
    rc = idx.lib.pfann_match_topn(idx.handle, q.data_ptr(), labels.data_ptr(), labels.shape[1], qs.data_ptr(), ql.data_ptr(), nQ,
                                  max_qlen, 1, 0.0, 0, only_owned, n, top.data_ptr(), nf.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, top.cpu().numpy(), nf.cpu().numpy()


@pytest.mark.parametrize("shape", ["lds_small", "rank2048", "single65"])
def test_a_query_longer_than_max_qlen_is_refused(torch_cuda, shape):
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    d, n = 64, 5
    b, k, plan, want = _batch("aligned", shape, d, 1, 0)
    db, pos = _world(d)
    P = 1
    while P < max(b.qlen) * k:
        P <<= 1
    short = (P // 2) // k                      # rows whose list fits half the slots: longer queries are refused
    assert mx.match_plan(len(b.qlen), short, k)[0] == plan and 1 <= short < max(b.qlen)
    pmax = 1
    while pmax < short * k:
        pmax <<= 1
    rc, raw, nf = _raw_call(torch_cuda, _index(d, db, pos), b, n, short)
    assert rc == 0
    top = np.frombuffer(raw.tobytes(), dtype=DeviceIndex.RESULT_DTYPE).reshape(len(b.qlen), n)
    pad = np.array([tx.PAD], dtype=DeviceIndex.RESULT_DTYPE)[0]
    refused = 0
    for j, m in enumerate(b.qlen):
        Pj = 1
        while Pj < m * k:
            Pj <<= 1
        if Pj > pmax:
            refused += 1
            assert top[j, 0]["song"] == -2 and nf[j] == -1 and (top[j, 1:] == pad).all(), (j, top[j], nf[j])
        else:
            _assert_exact(top[j:j + 1], nf[j:j + 1], _cut(want[j:j + 1], n), "query %d beside refused ones" % j)
    assert refused
    with pytest.raises(L.PfannError, match="refused"):
        _index(d, db, pos).topn_to_host(torch_cuda.as_tensor(raw).cuda(), torch_cuda.as_tensor(nf).cuda())


@pytest.mark.parametrize("n", [0, 65])
def test_n_outside_1_to_64_is_an_error_and_launches_nothing(torch_cuda, n):
    from pfann_amd import lib as L
    d = 64
    b, k, plan, want = _batch("aligned", "lds_small", d, 1, 0)
    db, pos = _world(d)
    idx = _index(d, db, pos)
    rc, raw, nf = _raw_call(torch_cuda, idx, b, n, max(b.qlen))
    assert rc == -1 and "1..64" in L.last_error()
    assert (raw == 0x5A).all() and (nf == 77).all()
    rc, raw, nf = _raw_call(torch_cuda, idx, b, 5, max(b.qlen), only_owned=3)        # PFANN_MATCH_OWNED_BLOCK means nothing here
    assert rc == -1 and (raw == 0x5A).all() and (nf == 77).all()
    with pytest.raises(L.PfannError):
        _topn(torch_cuda, idx, b, n, 1, 0)
