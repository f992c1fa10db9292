"""The rescoring stage on the GPU (pfann_match_songs_dense, csrc/dense_songs.hip): every entry against the float64 oracle of
tests/songs_dense_cases.py with `==` on the exact grid; no leak across song edges; byte equality with the ranked dense matcher
on real-valued rows; the byte contract across m, slot, batch and runs; the chain behind pfann_match_topn; pass-through, empties
and refusals; Database.query_rescore_batch."""
import ctypes
import os

import numpy as np
import pytest

import dense_cases as dc
import dense_topn_cases as dt
import match_exact as mx
import songs_dense_cases as sc

pytestmark = pytest.mark.gpu
D = 128


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


_INDEX = {}


def _index(key, db, pos, storage="f32"):
    from pfann_amd.database import DeviceIndex
    if (key, storage) not in _INDEX:
        idx = DeviceIndex(db.shape[1], 0, storage)
        idx.load(db, pos)
        _INDEX[(key, storage)] = idx
    return _INDEX[(key, storage)]


def _world(name, d):
    return dc.small_world(d) if name == "small" else dt.packed_world(d)


def _entry_of(top_row, song):
    """the entry of `song` in one query's list, as bytes"""
    hit = np.flatnonzero(top_row["song"] == song)
    assert hit.size == 1, (song, top_row["song"].tolist())
    return top_row[hit[0]:hit[0] + 1].tobytes()


# ------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("d", [128, 64])
@pytest.mark.parametrize("world", ["small", "packed"])
def test_every_entry_equals_the_oracle(torch_cuda, world, d):
    """queries of 1 / 2 / 19 / 63 / 64 rows cut from the worlds' recordings x m 1 / 3 / 64; lists with padding in the middle,
    duplicates, rowless songs, ids out of range, the first and the last song: every field of every entry and n_found, =="""
    db, pos, q, _, _ = _world(world, d)
    lens = np.diff(pos)
    if world == "small":
        assert (lens == 1).any() and lens.min() > 0
    else:
        assert (lens == 0).sum() > 5 and (lens == 300).sum() == 2 and (lens == 1).sum() == 200
    mx.assert_exact_domain(64, d)
    idx = _index((world, d), db, pos)
    qstart, qlen = sc.cut_queries(q.shape[0])
    assert sorted(set(qlen)) == list(sc.LENGTHS)
    qd = torch_cuda.as_tensor(q).cuda()
    for m in sc.MS:
        lists = sc.make_lists(pos, len(qlen), m, seed=500 + m)
        want = sc.songs_dense_oracle(q, db, pos, qstart, qlen, lists, key=(world, d))
        top, n_found = idx.match_songs_dense(qd, qstart, qlen, lists)
        assert top.shape == (len(qlen), m)
        bad = dt.differing(top, n_found, None, want)
        assert not bad, "%s d %d m %d: %d of %d queries differ\n%s" % (world, d, m, len(bad), len(want), "\n".join(bad[:6]))
        if m == 64:
            found = np.asarray([w["n_found"] for w in want])
            assert found.min() < found.max() < 65 and (top["song"][:, -1] == -1).any(), "the lists do not vary"
    if world == "small":                                                 # the copied pair ties: the lower song ranks first
        pair = (5 - 3, 9 - 3)
        s = int(pos[pair[0]])
        top, _ = idx.match_songs_dense(torch_cuda.as_tensor(db[s:s + 19]).cuda(), [0], [19], [[pair[1], pair[0]]])
        assert top["song"][0].tolist() == [pair[0], pair[1]] and top["score"][0, 0] == top["score"][0, 1]


@pytest.mark.parametrize("n", [19, 64, 2])
def test_no_leak_across_song_edges(torch_cuda, n):
    """both neighbours of every song A hold the query's own rows at A's edges; A is shorter than the query, and one below, at and
    one above the widths at which the candidates or the rows fill a column tile (128 - (n-1) owned columns)"""
    db, pos, q, a_ids = sc.leak_world(n)
    lens = np.diff(pos)
    own = 128 - (n - 1)
    assert {own - 1, own, own + 1} <= {int(lens[a]) for a in a_ids} and min(int(lens[a]) for a in a_ids) <= max(1, n - 5)
    mx.assert_exact_domain(n, D)
    idx = _index(("leak", n), db, pos)
    lists = [a_ids + [-1] * (64 - len(a_ids))]
    want = sc.songs_dense_oracle(q, db, pos, [0], [n], lists)
    top, n_found = idx.match_songs_dense(torch_cuda.as_tensor(q).cuda(), [0], [n], lists)
    bad = dt.differing(top, n_found, None, want)
    assert not bad, "\n".join(bad)
    # what reading past an edge would have given A: n-1 self-products beside one honest product, above its honest score
    honest = {h[0]: h[4] for h in want[0]["top"] if h[0] >= 0}
    q64 = q.astype(np.float64)
    for a in a_ids:
        first, last = db[pos[a]].astype(np.float64), db[pos[a + 1] - 1].astype(np.float64)
        head = ((q64[:n - 1] ** 2).sum() + q64[n - 1] @ first) / n          # offset -(n-1), rows of the song before A read too
        tail = (q64[0] @ last + (q64[1:] ** 2).sum()) / n                   # offset len-1, rows of the song behind A read too
        assert min(head, tail) > honest[a], "song %d: its neighbours' rows would not have shown" % a


# ------------------------------------------------------------------------------------------------ real-valued rows
@pytest.fixture(scope="module")
def self_world(tmp_path_factory):
    """dense_cases.selfmatch_world as a database directory, noisy queries of several lengths cut from it -> (dir, emb, pos, q,
    qstart, qlen)"""
    d = str(tmp_path_factory.mktemp("songs_dense_self"))
    emb, pos = dc.selfmatch_world(d)
    rng = np.random.default_rng(4)
    qlen = [19, 64, 1, 33, 63, 2, 19, 40]
    rows = []
    for j, n in enumerate(qlen):
        s = (0, 2, 4, 7, 9, 11, 3, 8)[j]
        a = int(pos[s]) + (j * 3) % max(1, int(pos[s + 1] - pos[s]) - n // 2)
        x = emb[a:a + n].astype(np.float64) + 0.05 * rng.standard_normal((n, emb.shape[1]))
        rows.append((x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32))
    qstart = [int(x) for x in np.pad(np.cumsum(qlen), (1, 0))[:-1]]
    return d, emb, pos, np.concatenate(rows), qstart, qlen


def test_entries_are_the_ranked_dense_matchers_bytes(torch_cuda, self_world):
    """real-valued rows: every (query, listed song) entry is, as bytes, the entry pfann_match_windows_dense_topn gives that song
    for a one-window recording of the query's rows (n = 64 lists every song); with every song listed the lists are equal"""
    _, emb, pos, q, qstart, qlen = self_world
    n_songs = len(pos) - 1
    have = np.flatnonzero(np.diff(pos) > 0)
    assert have.size == 11 < 64
    idx = _index("self", emb, pos)
    qd = torch_cuda.as_tensor(q).cuda()
    (ref, ref_found, _), wfirst = idx.match_windows_dense_topn(qd, qstart, qlen, 64, 1, 64)
    assert wfirst.tolist() == list(range(len(qlen) + 1)) and (ref_found == 11).all()
    assert len({float(x) for x in ref["score"][:, :11].ravel()}) > 60, "the scores are not real-valued"
    every = np.full((len(qlen), 64), -1, np.int32)
    every[:, 5:5 + n_songs] = np.arange(n_songs)[::-1]                   # all twelve ids, the rowless song 5 among them
    top, n_found = idx.match_songs_dense(qd, qstart, qlen, every)
    assert top.tobytes() == ref.tobytes() and np.array_equal(n_found, ref_found)
    some = np.asarray([[7, 2, -1, 9], [4, 4, 12, 0], [11, 5, 3, 2], [9, 8, 7, 6]] * 2, np.int32)
    top, n_found = idx.match_songs_dense(qd, qstart, qlen, some)
    for j in range(len(qlen)):
        listed = sorted({int(s) for s in some[j] if 0 <= s < n_songs and s in have})
        assert int(n_found[j]) == len(listed) and sorted(top["song"][j][:len(listed)].tolist()) == listed
        assert (top["song"][j][len(listed):] == -1).all() and (np.diff(top["score"][j][:len(listed)]) <= 0).all()
        for s in listed:
            assert _entry_of(top[j], s) == _entry_of(ref[j], s), (j, s)


def test_byte_contract(torch_cuda, self_world):
    """one (query, song): alone with m = 1; in the last slot of m = 64; among 600 other queries with m = 8 (4808 pairs: more than
    the grid has workgroups); and on a second run"""
    _, emb, pos, q, qstart, qlen = self_world
    idx = _index("self", emb, pos)
    torch = torch_cuda
    j0, song = 3, 9
    mine = q[qstart[j0]:qstart[j0] + qlen[j0]]
    alone, _ = idx.match_songs_dense(torch.as_tensor(mine).cuda(), [0], [qlen[j0]], [[song]])
    want = _entry_of(alone[0], song)
    assert alone["song"][0, 0] == song and np.isfinite(alone["score"][0, 0])
    last = np.asarray([[(i * 5) % 9 for i in range(63)] + [song]], np.int32)
    assert song not in last[0, :63]
    got, _ = idx.match_songs_dense(torch.as_tensor(mine).cuda(), [0], [qlen[j0]], last)
    assert _entry_of(got[0], song) == want, "the entry depends on m or on the slot"
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 65, 601)
    lens[300] = qlen[j0]
    starts = np.pad(np.cumsum(lens), (1, 0))[:-1]
    rows = emb[rng.integers(0, emb.shape[0], int(lens.sum()))].copy()
    rows[starts[300]:starts[300] + lens[300]] = mine
    lists = rng.integers(-1, len(pos), (601, 8)).astype(np.int32)
    lists[300] = [0, 1, 2, 3, 4, song, 6, 7]
    assert 601 * 8 > 2048
    many, found = idx.match_songs_dense(torch.as_tensor(rows).cuda(), starts, lens, lists)
    assert _entry_of(many[300], song) == want, "the entry depends on the other queries of the call"
    assert (found >= 0).all() and (found <= 8).all() and found.max() > 4
    again, found2 = idx.match_songs_dense(torch.as_tensor(rows).cuda(), starts, lens, lists)
    assert again.tobytes() == many.tobytes() and np.array_equal(found, found2), "two runs differ"
    assert _entry_of(idx.match_songs_dense(torch.as_tensor(mine).cuda(), [0], [qlen[j0]], [[song]])[0][0], song) == want


# ------------------------------------------------------------------------------------------------ behind pfann_match_topn
def test_chain_repairs_a_wrong_offset(torch_cuda):
    """hand-made labels nominate song A only at an alignment three rows off, and song B: match_topn names B, or A at the wrong
    offset; match_songs_dense on its raw output names A at the dense oracle's offset and score"""
    torch = torch_cuda
    db, pos, _, _, _ = dc.small_world()
    lens = np.diff(pos)
    plain = [s for s in range(len(lens)) if lens[s] >= 27 and s not in (5 - 3, 9 - 3)]      # not the periodic song or its copy
    A, B = plain[0], plain[1]
    n, off = 19, 5
    q = db[pos[A] + off:pos[A] + off + n].copy()
    labels = np.stack([pos[A] + off + 3 + np.arange(n), pos[B] + np.arange(n)], axis=1).astype(np.int64)
    idx = _index(("small", D), db, pos)
    qd = torch.as_tensor(q).cuda()
    raw, raw_found = idx.match_topn(qd, torch.as_tensor(labels).cuda(), [0], [n], 2, to_host=False)
    nominated = idx.decode_results(raw)[0]
    assert sorted(nominated["song"].tolist()) == sorted([A, B])
    assert nominated["song"][0] == B or nominated["offset"][0] != off
    top, n_found = idx.match_songs_dense(qd, [0], [n], raw)
    want = sc.songs_dense_oracle(q, db, pos, [0], [n], [[A, B]])
    assert not dt.differing(top, n_found, None, want)
    assert top["song"][0, 0] == A and top["offset"][0, 0] == off
    assert top["score"][0, 0] == float((q.astype(np.float64) ** 2).sum()) / n > nominated["score"][0]


# ------------------------------------------------------------------------------------------------ pass-through, empties
def test_long_and_empty_queries_and_empty_lists(torch_cuda):
    torch = torch_cuda
    from pfann_amd.database import DeviceIndex
    db, pos, q, _, _ = dc.small_world()
    idx = _index(("small", D), db, pos)
    qlen = [65, 0, 19, 19, 64]
    qstart = [0, 65, 65, 84, 84]
    m = 6
    cand = np.zeros((5, m), DeviceIndex.RESULT_DTYPE)
    rng = np.random.default_rng(3)
    cand["song"] = rng.integers(0, len(pos) - 1, (5, m))
    cand["offset"], cand["shift"], cand["n_cand"] = rng.integers(-9, 9, (5, m)), 7, rng.integers(1, 50, (5, m))
    cand["score"] = rng.standard_normal((5, m))
    cand["song"][2] = -1                                                 # nothing but padding
    cand["song"][0, 4] = -1
    raw = torch.from_numpy(cand.view(np.uint8).reshape(5, m, 24)).cuda()
    top, n_found = idx.match_songs_dense(torch.as_tensor(q).cuda(), qstart, qlen, raw)
    assert top[0].tobytes() == cand[0].tobytes() and n_found[0] == -1, "a 65-row query is not handed through unchanged"
    pad = np.asarray([dt.PAD] * m, DeviceIndex.RESULT_DTYPE)
    assert top[1].tobytes() == pad.tobytes() and n_found[1] == 0
    assert top[2].tobytes() == pad.tobytes() and n_found[2] == 0
    want = sc.songs_dense_oracle(q, db, pos, qstart[3:], qlen[3:], cand["song"][3:])
    assert not dt.differing(top[3:], n_found[3:], None, want)
    # the input is read, never written
    assert raw.cpu().numpy().tobytes() == cand.tobytes()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched(torch_cuda):
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    lib = L.load()
    db, pos = mx.std_world(41, D)
    whole = _index("std", db, pos)
    lo, hi = 10, 30
    shard = DeviceIndex(D, 0)
    shard.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    half = _index("std", db, pos, "f16")
    half_shard = DeviceIndex(D, 0, "f16")
    half_shard.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    q = torch.as_tensor(db[:30]).cuda()
    qs = torch.zeros(1, dtype=torch.int64).cuda()
    ql = torch.full((1,), 30, dtype=torch.int32).cuda()
    cand = torch.zeros((64 * 24,), dtype=torch.uint8).cuda()             # 64 entries, all naming song 1
    cand.view(torch.int32)[::6] = 1

    def call(idx, m):
        outs = [torch.full((size,), 0xA5, dtype=torch.uint8).cuda() for size in (65 * ctypes.sizeof(L.MatchResult), 4)]
        rc = lib.pfann_match_songs_dense(idx.handle, q.data_ptr(), qs.data_ptr(), ql.data_ptr(), 1, cand.data_ptr(), m,
                                         outs[0].data_ptr(), outs[1].data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, [bool((o.cpu() == 0xA5).all()) for o in outs]

    rc, _, untouched = call(whole, 3)                    # the control: the same call on a good handle writes both
    assert rc == 0 and not any(untouched)
    for idx, m, word in ((shard, 3, "shard"), (half, 3, "fp16"), (whole, 0, "m=0"), (whole, 65, "m=65"),
                         (half_shard, 3, "shard"), (shard, 0, "shard"), (half, 65, "fp16")):       # two at once: the first one
        rc, msg, untouched = call(idx, m)
        assert rc == -1 and msg and word in msg and all(untouched), (m, word, rc, msg, untouched)
    try:
        shard.match_windows_dense_topn(q, [0], [30], 5, 1, 3)
    except L.PfannError as e:
        dense_msg = str(e).split(": ", 1)[1]
    assert call(shard, 3)[1] == dense_msg, "a shard is refused with another message than the dense matcher's"
    with pytest.raises(L.PfannError, match="shard"):
        shard.match_songs_dense(q, [0], [30], [[1, 2]])


# ------------------------------------------------------------------------------------------------ the Database layer
def test_database_query_rescore_batch(torch_cuda, self_world):
    """answers equal query_dense_batch's wherever the dense answer's song is among the nominated N; with N = 64 and every song
    nominated that is every query.  The refusals of _dense_check and of a sharded database."""
    from pfann_amd import database as dbm
    from pfann_amd import lib as L
    from pfann_amd.utils import read_config
    torch = torch_cuda
    dirname, emb, pos, q, qstart, qlen = self_world
    cfg = read_config(os.path.join(dirname, "configs.json"))
    db = dbm.Database(dirname, cfg["indexer"], cfg["hop_size"], d=D)
    assert db.frame_shift_mul == 1 and db.score_alpha == 0
    qd = torch.as_tensor(q).cuda()
    dense_answers, dense_ranked = db.query_dense_batch(qd, qstart, qlen, n=64)
    # the nominated lists of this very search: which songs does the matcher name?
    named = db.query_topn_batch(qd, qstart, qlen, 64)
    long_enough = [j for j, n in enumerate(qlen) if n >= 19]
    assert len(long_enough) >= 5
    for j in long_enough:                                # k = 100 labels per row over 11 short songs: every song is nominated
        assert {s for _, (s, _) in named[j]} == {s for _, (s, _) in dense_ranked[j]}, j
    answers, ranked = db.query_rescore_batch(qd, qstart, qlen, 64)
    assert len(answers) == len(ranked) == len(qlen) and all(a[2] is None for a in answers)
    for j in long_enough:
        assert answers[j][:2] == dense_answers[j][:2] and ranked[j] == dense_ranked[j], j
    for n in (1, 3):
        answers, ranked = db.query_rescore_batch(qd, qstart, qlen, n)
        checked = 0
        for j in range(len(qlen)):
            assert len(ranked[j]) <= n and ranked[j][0] == answers[j][:2]
            if dense_answers[j][1][0] in {s for _, (s, _) in named[j][:n]}:
                assert answers[j][:2] == dense_answers[j][:2], (n, j)
                checked += 1
        assert checked >= 5, "the comparison was nearly empty"
    alone, _ = db.query_rescore_batch(qd[qstart[3]:qstart[3] + qlen[3]], [0], [qlen[3]], 3)
    assert alone[0] == answers[3], "a query's answer depends on what it was batched with"
    for change, word in (({"frame_shift_mul": 2}, "frame_shift_mul"), ({"score_alpha": 2.0}, "score_alpha")):
        other = dbm.Database(dirname, dict(cfg["indexer"], **change), cfg["hop_size"], d=D)
        with pytest.raises(L.PfannError, match=word):
            other.query_rescore_batch(qd, qstart, qlen, 4)
    with pytest.raises(L.PfannError, match="1..64"):
        db.query_rescore_launch(qd, qstart, qlen, 65)
