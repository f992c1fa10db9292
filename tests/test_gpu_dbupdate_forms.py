"""Database updates on the GPU, the dense and nominated query forms: an updated handle (pfann_db_append / pfann_db_remove_songs)
answers pfann_match_windows_dense_stats, _dense_topn, _dense_topn_stats, pfann_match_songs_dense, pfann_nominate_songs_dense,
pfann_nominate_windows_dense and the part / merge pairs with the bytes of a fresh handle loaded with the resulting rows -- with
queries that copy the GHOST ROWS an update leaves past `n`, and with every form called before the update as well, so that
scratch, bounds and guards set for the smaller or louder database are in play.  On grid rows the same answers are held against
the float64 oracles of tests/dense_topn_cases.py, tests/songs_dense_cases.py and tests/dense_stats_cases.py.  Every comparison
is equality of bytes or `==`: there is no tolerance in this file."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

import dense_stats_cases as ds
import dense_topn_cases as dt
import match_exact as mx
import songs_dense_cases as sd
import test_gpu_dbupdate as du
from test_gpu_dbupdate import N_SONGS, BIG, REMOVE_CASES, b, keep_rows, new_index, pos_of

pytestmark = pytest.mark.gpu
REPO = du.REPO
LONG, SHORT, FILL = 33, 12, 36               # the 300-row song, the 5-row song, the song whose length puts pos[39] on a tile edge
TILE = 128
REC = (130, 70)                              # rows of the ordinary and of the ghost recording
LIVE = 20                                    # the ghost recording: the last LIVE rows below the new n, then the rows from n on
QLEN = (5, 7, 20, 11, 19, 8, 13, 20, 6, 16)  # queries 0-4 are noisy copies of song 6, queries 5-9 lie in the ghost recording
SHAPES = ((19, 7), (8, 4))
_worlds = {}


def world(d, exact=False):
    """test_gpu_dbupdate.rows(d)'s 40 songs (5 and 20 without rows, BIG loud) with three lengths set on purpose: LONG has 300 rows
    (two tile edges inside it), SHORT has 5 (shorter than the smallest window, 8), the last song has 200 (no other is longer than
    199, so the ghosts of "first" and "big" all duplicate rows of the last song), and FILL is stretched until the last song starts
    on a multiple of 128.  Real-valued unit rows with BIG at norm 50; with exact=True rows on the grid k/16 of
    tests/match_exact.py with BIG times 8 (norm ~54), on which the fp32 totals are exact.  -> (x, lens)"""
    if (d, exact) not in _worlds:
        lens = du.rows(d)[1].copy()
        lens[LONG], lens[SHORT], lens[N_SONGS - 1] = 300, 5, 200
        lens[FILL] += (-int(pos_of(lens)[N_SONGS - 1])) % TILE
        n = int(lens.sum())
        pos = pos_of(lens)
        if exact:
            x = mx.grid_rows(2000 + d, "dbupdate-forms/db", n, d)
            x[pos[BIG]:pos[BIG + 1]] *= 8.0
        else:
            x = np.random.default_rng(2000 + d).standard_normal((n, d)).astype(np.float32)
            x /= np.linalg.norm(x, axis=1, keepdims=True)
            x[pos[BIG]:pos[BIG + 1]] *= 50.0
        _worlds[(d, exact)] = (np.ascontiguousarray(x, np.float32), lens)
    return _worlds[(d, exact)]


def noisy(rows, exact, seed):
    """ordinary queries: real rows plus 0.05 noise per coordinate, renormalised; grid rows with a fifth of the values redrawn"""
    rng = np.random.default_rng(seed)
    if exact:
        other = mx.grid_rows(seed, "dbupdate-forms/noise", rows.shape[0], rows.shape[1])
        return np.where(rng.random(rows.shape) < 0.2, other, rows).astype(np.float32)
    q = rows / np.linalg.norm(rows, axis=1, keepdims=True) + 0.05 * rng.standard_normal(rows.shape)
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)


def inputs(d, exact=False, n_new=None):
    """The recordings and queries of one snapshot -> dict(q, rstart, rlen, qstart, qlen, ghost).

    Recording 0 (130 rows): noisy copies of rows 10.. of song 3 (songs 3, 4, 6 and 7 are in no removal case and in every append
    stage).  Recording 1 (70 rows), with n_new = the handle's row count after a removal: rows [n_new - 20, n_new + 50) of the OLD
    matrix, exact copies.  A removal moves rows down to destinations below n_new and writes nothing from n_new on, so on the
    device the rows [n_new, n_old) are still the old rows of that range -- the ghosts; the test cannot read them, it copies
    them from the world: after "last" they are the removed last song, after "first" the last rows of the old last song, after
    "big" and "scattered" what the last chunk of the move left behind.  The first 20 rows are the live rows right below n_new,
    so the windows in between straddle n as a tile does.  Without n_new (appends; a removal that removes no row) recording 1
    is a noisy copy of song 7.  Queries 0-4 are noisy copies of song 6, queries 5-9 slices of recording 1."""
    x, lens = world(d, exact)
    pos = pos_of(lens)
    ghost = n_new is not None and x.shape[0] - n_new >= REC[1] - LIVE
    rec0 = noisy(x[pos[3] + 10:pos[3] + 10 + REC[0]], exact, 11)
    rec1 = x[n_new - LIVE:n_new - LIVE + REC[1]] if ghost else noisy(x[pos[7]:pos[7] + REC[1]], exact, 12)
    assert rec0.shape[0] == REC[0] and rec1.shape[0] == REC[1]
    own = noisy(x[pos[6]:pos[6] + sum(QLEN[:5])], exact, 13)
    q = np.ascontiguousarray(np.concatenate([rec0, rec1, own]), np.float32)
    qstart = [sum(REC) + sum(QLEN[:j]) for j in range(5)] + [REC[0] + sum(QLEN[5:j]) for j in range(5, 10)]
    assert max(s + n for s, n in zip(qstart[5:], QLEN[5:])) <= sum(REC) and min(QLEN) == 5 and max(QLEN) == 20
    return dict(q=q, rstart=[0, REC[0]], rlen=list(REC), qstart=qstart, qlen=list(QLEN), ghost=ghost)


def song_lists(song_pos, m):
    """songs_dense_cases.make_lists on the handle's own song_pos (a database with fewer than two songs with rows: fixed ids)"""
    n_songs = len(song_pos) - 1
    if int((np.diff(song_pos) > 0).sum()) < 2:
        return np.resize(np.asarray([0, n_songs - 1, -1, n_songs], np.int32), (len(QLEN), m))
    return sd.make_lists(song_pos, len(QLEN), m, 77)


def snapshot_dense(idx, inp, monkeypatch, nominate=True):
    """the bytes of every output of every dense and nominated form -> dict by form, in call order.  nominate=False: without the
    two forms that read the fp16 copy."""
    import torch
    q = torch.from_numpy(inp["q"]).cuda()
    rstart, rlen, qstart, qlen = inp["rstart"], inp["rlen"], inp["qstart"], inp["qlen"]
    excl = [3, min(38, idx.n_songs - 1)]
    for name in ("PFANN_NOMINATE_QUERIES", "PFANN_NOMINATE_WINDOWS"):
        monkeypatch.delenv(name, raising=False)
    out = {}
    for w, h in SHAPES:
        for ex in (None, excl):
            tag = "(%d, %d%s)" % (w, h, "" if ex is None else ", excl")
            (res, st), _ = idx.match_windows_dense_stats(q, rstart, rlen, w, h, exclude_song=ex, to_host=False)
            out["match_windows_dense_stats" + tag] = b(res) + b(st)
            (top, nf, ss), _ = idx.match_windows_dense_topn(q, rstart, rlen, w, h, 3, exclude_song=ex, want_song_scores=True, to_host=False)
            out["match_windows_dense_topn" + tag] = b(top) + b(nf) + b(ss)
            (top2, nf2, ss2, st2), _ = idx.match_windows_dense_topn_stats(q, rstart, rlen, w, h, 3, exclude_song=ex,
                                                                          want_song_scores=True, to_host=False)
            out["match_windows_dense_topn_stats" + tag] = b(top2) + b(nf2) + b(ss2) + b(st2)
            # the part and merge pairs on the whole handle as a one-part job: the whole-handle call's bytes
            (words, pst), _ = idx.match_windows_dense_part(q, rstart, rlen, w, h, exclude_song=ex, stats=True)
            mres, mst = idx.dense_merge(words[None], pst[None], rlen, w, h, exclude_song=ex)
            out["match_windows_dense_part / dense_merge" + tag] = b(words) + b(pst) + b(mres) + b(mst)
            assert b(mres) + b(mst) == b(res) + b(st), "dense_merge%s differs from match_windows_dense_stats on the same handle" % tag
            (ptop, pnf), _ = idx.match_windows_dense_topn_part(q, rstart, rlen, w, h, 3, exclude_song=ex)
            mtop, mnf = idx.dense_topn_merge(ptop[None], pnf[None])
            out["match_windows_dense_topn_part / dense_topn_merge" + tag] = b(ptop) + b(pnf) + b(mtop) + b(mnf)
            assert b(mtop) + b(mnf) == b(top) + b(nf), "dense_topn_merge%s differs from match_windows_dense_topn on the same handle" % tag
    lens = np.diff(idx.song_pos)
    for m in (3, 64):
        lists = song_lists(idx.song_pos, m)
        if m == 64 and (lens == 300).any():
            assert np.isin(np.flatnonzero(lens == 300), lists).all(), "the 300-row song is in no candidate list"
        if m == 64 and (lens == 0).any():
            assert np.isin(lists, np.flatnonzero(lens == 0)).any(), "no emptied song is in a candidate list"
        top, nf = idx.match_songs_dense(q, qstart, qlen, lists, to_host=False)
        out["match_songs_dense(m %d)" % m] = b(top) + b(nf)
    if nominate:
        for n in (4, 1):
            out["nominate_songs_dense(n %d)" % n] = b"".join(b(t) for t in idx.nominate_songs_dense(q, qstart, qlen, n, to_host=False))
        monkeypatch.setenv("PFANN_NOMINATE_QUERIES", "3")                # ten queries: four chunks
        out["nominate_songs_dense(n 4, 3 queries per chunk)"] = b"".join(b(t) for t in idx.nominate_songs_dense(q, qstart, qlen, 4, to_host=False))
        monkeypatch.delenv("PFANN_NOMINATE_QUERIES")
        assert out["nominate_songs_dense(n 4, 3 queries per chunk)"] == out["nominate_songs_dense(n 4)"], "the bytes depend on the chunking"
        for w, h, ex in ((19, 2, None), (64, 70, None), (19, 2, excl)):
            tag = "(%d, %d%s)" % (w, h, "" if ex is None else ", excl")
            out["nominate_windows_dense" + tag] = b"".join(b(t) for t in idx.nominate_windows_dense(q, rstart, rlen, w, h, 4, exclude_song=ex,
                                                                                                    to_host=False)[0])
        monkeypatch.setenv("PFANN_NOMINATE_WINDOWS", "1")                # one row-tile slot per chunk
        out["nominate_windows_dense(19, 2, one slot per chunk)"] = b"".join(b(t) for t in idx.nominate_windows_dense(q, rstart, rlen, 19, 2, 4,
                                                                                                                     to_host=False)[0])
        monkeypatch.delenv("PFANN_NOMINATE_WINDOWS")
        assert out["nominate_windows_dense(19, 2, one slot per chunk)"] == out["nominate_windows_dense(19, 2)"], "the bytes depend on the chunking"
    torch.cuda.synchronize()
    return out


def assert_same_dense(idx, emb, lens, inp, monkeypatch, mode="copy", nominate=True):
    """form by form the bytes of a fresh handle of the resulting rows -> (the updated handle's snapshot, the fresh handle)"""
    fresh = new_index(idx.d, mode, emb, lens)
    assert np.array_equal(idx.song_pos, fresh.song_pos) and idx.ntotal == fresh.ntotal
    got = snapshot_dense(idx, inp, monkeypatch, nominate)
    want = snapshot_dense(fresh, inp, monkeypatch, nominate)
    assert list(got) == list(want)
    for name in want:
        assert len(want[name]) > 0 and got[name] == want[name], "%s differs from a fresh handle's" % name
    return got, fresh


# ------------------------------------------------------------------------------------------------ appends
@pytest.mark.parametrize("d,mode", [(128, "copy"), (128, "f32"), (64, "copy")])
def test_appends_give_the_fresh_handles_bytes(monkeypatch, d, mode):
    """the three stages of test_gpu_dbupdate.py: within a reservation, beyond it, device-resident rows with songs without rows;
    every form runs before each append too (and its answer is dropped)"""
    import torch
    x, lens = world(d)
    pos = pos_of(lens)
    inp = inputs(d)
    s1, s2, s3 = 13, 22, 30
    idx = new_index(d, mode, x[:pos[s1]], lens[:s1])
    snapshot_dense(idx, inp, monkeypatch)
    cap = idx.reserve(int(pos[s2]) + 7, s2)
    idx.append(x[pos[s1]:pos[s2]], lens[s1:s2])
    assert idx.capacity() == cap and idx.ntotal == pos[s2] < cap      # the reservation's last rows were never written
    assert_same_dense(idx, x[:pos[s2]], lens[:s2], inp, monkeypatch, mode)
    idx.append(x[pos[s2]:pos[s3]], lens[s2:s3])
    assert idx.capacity() > cap
    assert_same_dense(idx, x[:pos[s3]], lens[:s3], inp, monkeypatch, mode)
    tail = np.concatenate([lens[s3:35], [0], lens[35:]])
    assert lens[:s3].max() < 300 == tail.max(), "the longest song comes with the last append"
    idx.append(torch.from_numpy(x[pos[s3]:]).cuda(), tail)
    idx.append(np.zeros((0, d), np.float32), [0])
    assert_same_dense(idx, x, np.concatenate([lens[:s3], tail, [0]]), inp, monkeypatch, mode)


def test_forms_called_on_13_songs_then_on_41(monkeypatch):
    """the scratch the three call families share is sized from n_songs: both nominations and the ranked dense matcher on 13
    songs, then on 41 with the 300-row song among them"""
    import torch
    d = 128
    x, lens = world(d)
    pos = pos_of(lens)
    inp = inputs(d)
    q = torch.from_numpy(inp["q"]).cuda()
    idx = new_index(d, "copy", x[:pos[13]], lens[:13])

    def call():
        return (idx.nominate_songs_dense(q, inp["qstart"], inp["qlen"], 4, to_host=False),
                idx.nominate_windows_dense(q, inp["rstart"], inp["rlen"], 19, 2, 4, to_host=False)[0],
                idx.match_windows_dense_topn(q, inp["rstart"], inp["rlen"], 19, 7, 3, want_song_scores=True, to_host=False)[0])
    small = call()
    assert small[2][2].shape[1] == 13
    extra = noisy(x[pos[LONG] + 100:pos[LONG] + 137], False, 14)
    idx.append(np.concatenate([x[pos[13]:], extra]), np.concatenate([lens[13:], [37]]))
    assert idx.n_songs == 41 and np.diff(idx.song_pos).max() == 300
    large = call()
    assert large[2][2].shape[1] == 41
    assert_same_dense(idx, np.concatenate([x, extra]), np.concatenate([lens, [37]]), inp, monkeypatch)


# ------------------------------------------------------------------------------------------------ removals
STRADDLE = {"last": lambda r: r == 0, "first": lambda r: r not in (0, TILE - 1), "big": lambda r: r not in (0, TILE - 1)}


@pytest.mark.parametrize("case", sorted(REMOVE_CASES))
@pytest.mark.parametrize("d,mode", [(128, "copy"), (128, "f32"), (64, "copy")])
def test_removals_give_the_fresh_handles_bytes(monkeypatch, d, mode, case):
    """every entry of REMOVE_CASES, moved in chunks of 64 rows; recording 1 and queries 5-9 copy the rows left past the new n"""
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")
    x, lens = world(d)
    gone = REMOVE_CASES[case]
    kept, new_lens = keep_rows(x, lens, gone)
    n_new = kept.shape[0]
    if case in STRADDLE:                                  # "last" leaves n on a tile edge, "first" and "big" inside a tile
        assert STRADDLE[case](n_new % TILE), (case, n_new, n_new % TILE)
    inp = inputs(d, n_new=n_new)
    assert inp["ghost"] == (case != "no_rows")
    idx = new_index(d, mode, x, lens)
    snapshot_dense(idx, inp, monkeypatch)                 # on the larger, louder database: dropped
    idx.remove_songs(gone)
    assert idx.ntotal == n_new and idx.capacity() >= x.shape[0]
    assert_same_dense(idx, kept, new_lens, inp, monkeypatch, mode)
    if mode == "copy":
        assert (idx.row_norm_max() < 1.01) == (BIG in gone)


def test_remove_all_then_append(monkeypatch):
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")
    d = 128
    x, lens = world(d)
    pos = pos_of(lens)
    idx = new_index(d, "copy", x, lens)
    inp = inputs(d, n_new=x.shape[0] - int(lens[BIG]))     # the last rows of x: what the second removal and append leave past n
    snapshot_dense(idx, inp, monkeypatch)
    idx.remove_songs(list(range(N_SONGS)))
    assert idx.ntotal == 0
    idx.append(x, lens)                                   # the ids go on behind the removed ones
    none = np.zeros(N_SONGS, np.int64)
    assert_same_dense(idx, x, np.concatenate([none, lens]), inp, monkeypatch)
    idx.remove_songs([N_SONGS + 3, N_SONGS + BIG])
    kept, new_lens = keep_rows(x, lens, [3, BIG])
    idx.append(x[pos[3]:pos[4]], [lens[3]])
    assert_same_dense(idx, np.concatenate([kept, x[pos[3]:pos[4]]]), np.concatenate([none, new_lens, [lens[3]]]), inp, monkeypatch)


def test_fp16_storage_is_still_refused_after_an_update(monkeypatch):
    """the dense forms score fp32 rows: an updated "f16" handle refuses them with a fresh one's message"""
    import torch
    from pfann_amd.lib import PfannError
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")
    d = 128
    x, lens = world(d)
    pos = pos_of(lens)
    inp = inputs(d)
    q = torch.from_numpy(inp["q"]).cuda()
    rs, rl, qs, ql = inp["rstart"], inp["rlen"], inp["qstart"], inp["qlen"]
    idx = new_index(d, "f16", x[:pos[30]], lens[:30])
    idx.append(x[pos[30]:], lens[30:])
    idx.remove_songs([0, BIG])
    kept, new_lens = keep_rows(x, lens, [0, BIG])
    fresh = new_index(d, "f16", kept, new_lens)
    calls = {"match_windows_dense_stats": lambda i: i.match_windows_dense_stats(q, rs, rl, 19, 7),
             "match_windows_dense_topn": lambda i: i.match_windows_dense_topn(q, rs, rl, 19, 7, 3),
             "match_windows_dense_topn_stats": lambda i: i.match_windows_dense_topn_stats(q, rs, rl, 19, 7, 3),
             "match_songs_dense": lambda i: i.match_songs_dense(q, qs, ql, song_lists(i.song_pos, 3)),
             "nominate_songs_dense": lambda i: i.nominate_songs_dense(q, qs, ql, 4),
             "nominate_windows_dense": lambda i: i.nominate_windows_dense(q, rs, rl, 19, 2, 4),
             "match_windows_dense_part": lambda i: i.match_windows_dense_part(q, rs, rl, 19, 7, stats=True),
             "match_windows_dense_topn_part": lambda i: i.match_windows_dense_topn_part(q, rs, rl, 19, 7, 3)}
    for name, call in calls.items():
        said = []
        for handle in (fresh, idx):
            with pytest.raises(PfannError, match="fp16") as refused:
                call(handle)
            said.append(str(refused.value))
        assert said[0] == said[1], name


# ------------------------------------------------------------------------------------------------ ghosts against the oracles
@pytest.mark.parametrize("case", ["last", "first", "big"])
def test_ghost_rows_against_the_host_references(monkeypatch, case):
    """Equality with a fresh handle proves nothing if both are wrong alike: on grid rows (every fp32 total exact) the updated
    handle's ranked lists, rescored lists and statistics are the float64 oracles' on the resulting rows, no ranked list names a
    removed song, and where the nomination certifies a window or query, rescoring its list gives the ranked dense matcher's
    entry 0 byte for byte (the contract of tests/test_gpu_nominate_dense.py and tests/test_gpu_nominate_windows.py)."""
    import torch
    from pfann_amd.database import window_queries
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")
    d = 128
    x, lens = world(d, exact=True)
    mx.assert_exact_domain(max(QLEN) * 8, d)              # (BIG's rows are 8 times the grid's)
    gone = REMOVE_CASES[case]
    kept, new_lens = keep_rows(x, lens, gone)
    n_new, pos = kept.shape[0], pos_of(new_lens)
    assert STRADDLE[case](n_new % TILE), (case, n_new % TILE)
    inp = inputs(d, exact=True, n_new=n_new)
    assert inp["ghost"]
    qn, rstart, rlen, qstart, qlen = inp["q"], inp["rstart"], inp["rlen"], inp["qstart"], inp["qlen"]
    q = torch.from_numpy(qn).cuda()
    idx = new_index(d, "copy", x, lens)
    snapshot_dense(idx, inp, monkeypatch)
    idx.remove_songs(gone)
    _, fresh = assert_same_dense(idx, kept, new_lens, inp, monkeypatch)
    removed = np.asarray(sorted(set(gone)))
    key = ("dbupdate-forms", case)
    for w, h in SHAPES:
        # ---- the ranked dense matcher and the statistics
        (top, n_found, block), wfirst = idx.match_windows_dense_topn(q, rstart, rlen, w, h, 3, want_song_scores=True)
        want = dt.dense_topn_oracle(qn, kept, pos, w, h, rstart, rlen, 3, key=key)
        bad = dt.differing(top, n_found, block, want)
        assert not bad, "window %d hop %d: %d of %d windows differ\n%s" % (w, h, len(bad), len(want), "\n".join(bad[:6]))
        assert not np.isin(top["song"], removed).any() and (block[:, removed] == 0).all()
        assert (n_found == int((new_lens > 0).sum())).all()
        ((res, stats), _) = idx.match_windows_dense_stats(q, rstart, rlen, w, h)
        swant = ds.stats_oracle(qn, kept, pos, w, h, rstart, rlen, key=key)
        bad = ds.differing(stats, swant)
        assert not bad, "window %d hop %d: %d of %d windows differ\n%s" % (w, h, len(bad), len(swant), "\n".join(bad[:6]))
        for j, sw in enumerate(swant):
            assert (int(res["song"][j]), int(res["offset"][j]), float(res["score"][j])) == (sw["song"], sw["offset"], sw["score"]), j
        # ---- the windows that lie wholly in the ghost rows: the oracle's best score, which for "last" (the removed song's own
        # rows; nothing like them is left) is below what an exact copy scores.  After "first" and "big" the ghosts duplicate
        # the last song's rows, which are still in the database: there the copy's score is the right answer, at the live rows.
        starts = np.arange(int(wfirst[2] - wfirst[1])) * h
        whole = int(wfirst[1]) + np.flatnonzero(starts >= LIVE)
        assert whole.size >= 5
        for j in whole:
            r0 = rstart[1] + int(starts[j - int(wfirst[1])])
            copy_score = float((qn[r0:r0 + w].astype(np.float64) ** 2).sum() / w)
            assert float(top["score"][j, 0]) == want[j]["top"][0][4]
            if case == "last":
                assert want[j]["top"][0][4] < copy_score, "the oracle itself finds a copy: the inputs say nothing"
                assert float(top["score"][j, 0]) < copy_score
            else:
                assert want[j]["top"][0][4] == copy_score and int(top["song"][j, 0]) == N_SONGS - 1
    # ---- the rescoring stage
    for m in (3, 64):
        lists = song_lists(idx.song_pos, m)
        top, n_found = idx.match_songs_dense(q, qstart, qlen, lists)
        want = sd.songs_dense_oracle(qn, kept, pos, qstart, qlen, lists, key=key)
        bad = dt.differing(top, n_found, None, want)
        assert not bad, "m %d: %d of %d queries differ\n%s" % (m, len(bad), len(want), "\n".join(bad[:6]))
        assert not np.isin(top["song"], removed).any()
    # ---- the certificate's contract, windows then queries
    N = 4
    (ref, _, _), wfirst = idx.match_windows_dense_topn(q, rstart, rlen, 19, 2, N)
    ws, wl, _ = window_queries(rstart, rlen, 19, 2)
    (cand, cfound, n_close), _ = idx.nominate_windows_dense(q, rstart, rlen, 19, 2, N, to_host=False)
    top, _ = idx.match_songs_dense(q, ws, wl, cand)
    n_close = n_close.cpu().numpy()
    assert not np.isin(idx.topn_to_host(cand, cfound)[0]["song"], removed).any()
    sure = np.flatnonzero((n_close >= 0) & (n_close <= N))
    for j in sure:
        assert top[j, 0:1].tobytes() == ref[j, 0:1].tobytes(), ("window", j, top[j, 0], ref[j, 0])
    # a condition on the inputs, taken on the fresh handle: at least half of the ghost recording's windows are certified
    (_, _, fclose), _ = fresh.nominate_windows_dense(q, rstart, rlen, 19, 2, N)
    fclose = fclose[int(wfirst[1]):int(wfirst[2])]
    assert 2 * int(((fclose >= 0) & (fclose <= N)).sum()) >= fclose.size > 20, fclose.tolist()
    (ref, _, _), _ = idx.match_windows_dense_topn(q, qstart, qlen, 64, 1, N)
    cand, cfound, n_close = idx.nominate_songs_dense(q, qstart, qlen, N, to_host=False)
    top, _ = idx.match_songs_dense(q, qstart, qlen, cand)
    n_close = n_close.cpu().numpy()
    assert not np.isin(idx.topn_to_host(cand, cfound)[0]["song"], removed).any()
    sure = np.flatnonzero((n_close >= 0) & (n_close <= N))
    assert sure.size >= 5, n_close.tolist()
    for j in sure:
        assert top[j, 0:1].tobytes() == ref[j, 0:1].tobytes(), ("query", j, top[j, 0], ref[j, 0])


# ------------------------------------------------------------------------------------------------ the fp16 copy gone and back
def test_the_nominations_refuse_while_the_fp16_copy_is_gone_and_answer_from_the_rebuilt_one(monkeypatch):
    """test_gpu_dbupdate.py's scenario for the other two readers of the fp16 copy.  The removal rebuilds the copy: allocated for
    the capacity, written for the rows left"""
    import torch
    from pfann_amd import lib as L
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")
    d = 128
    x, lens = world(d)
    idx = new_index(d, "copy", x, lens)
    huge = (x[:30] * 2.0e4).astype(np.float32)
    inp = inputs(d)
    # the ghosts of the removal below are the 30 rows of norm 2e4 behind the last song: the recording copies them at norm 1 (the
    # same directions; at 2e4 the squares of the totals would leave the statistics' 64 bits)
    inp["q"][REC[0] + LIVE:REC[0] + LIVE + 30] = x[:30]
    snapshot_dense(idx, inp, monkeypatch)
    idx.append(huge, [30])
    assert idx.set_prefilter(True) is False
    q = torch.from_numpy(inp["q"]).cuda()
    for call in (lambda: idx.nominate_songs_dense(q, inp["qstart"], inp["qlen"], 4),
                 lambda: idx.nominate_windows_dense(q, inp["rstart"], inp["rlen"], 19, 2, 4)):
        with pytest.raises(L.PfannError, match="keeps no fp16 copy"):
            call()
    # the refusals leave caller-provided outputs untouched (tests/test_gpu_nominate_windows.py)
    lib = L.load()
    nQ, nW = len(QLEN), 6
    qs = torch.as_tensor(inp["qstart"], dtype=torch.int64).cuda()
    ql = torch.as_tensor(inp["qlen"], dtype=torch.int32).cuda()
    rs = torch.zeros(1, dtype=torch.int64).cuda()
    rl = torch.full((1,), 30, dtype=torch.int32).cuda()
    wf = torch.as_tensor([0, nW], dtype=torch.int64).cuda()              # window 19, hop 2 over 30 rows
    fill = lambda rows: [torch.full((rows * size,), 0xA5, dtype=torch.uint8).cuda() for size in (4 * ctypes.sizeof(L.MatchResult), 4, 4)]
    outs = fill(nQ)
    rc = lib.pfann_nominate_songs_dense(idx.handle, q.data_ptr(), qs.data_ptr(), ql.data_ptr(), nQ, 20, 4, outs[0].data_ptr(),
                                        outs[1].data_ptr(), outs[2].data_ptr(), None)
    msg = L.last_error()
    torch.cuda.synchronize()
    assert rc == -1 and "keeps no fp16 copy" in msg and all(bool((o.cpu() == 0xA5).all()) for o in outs), (rc, msg)
    outs = fill(nW)
    rc = lib.pfann_nominate_windows_dense(idx.handle, q.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, 19, 2, wf.data_ptr(), nW, None, 4,
                                          outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None)
    msg = L.last_error()
    torch.cuda.synchronize()
    assert rc == -1 and "keeps no fp16 copy" in msg and all(bool((o.cpu() == 0xA5).all()) for o in outs), (rc, msg)
    # the exact dense forms still answer, with a fresh handle's bytes
    assert_same_dense(idx, np.concatenate([x, huge]), np.concatenate([lens, [30]]), inp, monkeypatch, nominate=False)
    idx.remove_songs([N_SONGS])
    assert idx.set_prefilter(True) is True and idx.capacity() > idx.ntotal == x.shape[0]
    got, _ = assert_same_dense(idx, x, np.concatenate([lens, [0]]), inp, monkeypatch)
    assert any(name.startswith("nominate_windows_dense") for name in got) and any(name.startswith("nominate_songs_dense") for name in got)


# ------------------------------------------------------------------------------------------------ through Database
def _canon(v):
    """nested answers -> something `==` compares by bytes"""
    if isinstance(v, np.ndarray):
        return (str(v.dtype), v.shape, np.ascontiguousarray(v).tobytes())
    if isinstance(v, (list, tuple)):
        return tuple(_canon(e) for e in v)
    if isinstance(v, (float, np.floating)):
        return np.float64(v).tobytes()
    return v


def test_an_open_database_answers_the_dense_forms_as_a_reopened_one(tmp_path):
    """configs/tiny.json, eight synthetic songs through builder.py; a Database held open across add_songs and remove_songs gives
    query_dense_stats_batch, query_nominate_rescore_batch and monitor_nominate_launch / _finish the answers of a Database opened
    on the updated directory.  The rows asked about include the ghosts of the removal."""
    import torch
    from pfann_amd import synth
    from pfann_amd.database import Database
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    d = params["model"]["d"]
    sd_ = synth.make_state_dict(params, seed=321)
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd_.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "tiny.json"), str(mdir / "configs.json"))
    music = []
    for s in range(8):
        path = str(tmp_path / ("song%02d.wav" % s))
        synth.write_wav(path, synth.make_song(700 + s, seconds=6.0 + s))
        music.append(path)
    mlist = str(tmp_path / "music.txt")
    open(mlist, "w").write("".join(p + "\n" for p in music))
    env = dict(os.environ, PYTHONPATH=REPO)
    env.pop("PFANN_GPUS", None)
    dbdir = str(tmp_path / "db")
    du._run([os.path.join(REPO, "builder.py"), mlist, dbdir, str(mdir)], str(tmp_path), env)
    emb = np.fromfile(os.path.join(dbdir, "embeddings"), np.float32).reshape(-1, d)
    hop = params["hop_size"]
    held = Database(dbdir, params["indexer"], hop, d=d)
    lens = np.diff(held.song_pos)
    pos = held.song_pos.copy()
    assert len(lens) == 8 and lens.min() >= 8
    added = np.ascontiguousarray(emb[pos[4]:pos[4] + 9][::-1])
    gone = [2, 7]
    n_new = emb.shape[0] + 9 - int(lens[2] + lens[7])
    stored = np.concatenate([emb, added])                 # the matrix between the two updates; its rows from n_new on are the ghosts
    assert stored.shape[0] - n_new >= 12
    rows = np.ascontiguousarray(np.concatenate([emb[pos[1]:pos[1] + 20], stored[n_new - 8:n_new + 12], emb[pos[5] + 2:pos[5] + 22]]))
    q = torch.from_numpy(rows).cuda()
    qstart, qlen = [0, 20, 28, 40], [20, 8, 12, 20]       # query 2 is all ghost rows

    def answers(db):
        a = db.query_dense_stats_batch(q, qstart, qlen, n=3)
        c = db.query_nominate_rescore_batch(q, qstart, qlen, 3)
        m = db.monitor_nominate_finish(db.monitor_nominate_launch(q, [0, 20], [20, 40], 8, 2, 3, edge_window=4))
        return {"query_dense_stats_batch": _canon(a), "query_nominate_rescore_batch": _canon(c), "monitor_nominate": _canon(m)}
    answers(held)                                         # on the directory as built: dropped
    assert held.add_songs(["x.wav", "y.wav"], added, [9, 0]) == 8
    assert held.remove_songs(gone) == gone
    assert int(held.song_pos[-1]) == n_new
    opened = Database(dbdir, params["indexer"], hop, d=d)
    assert np.array_equal(held.song_pos, opened.song_pos) and held.songList == opened.songList and len(opened.songList) == 10
    got, want = answers(held), answers(opened)
    for name in want:
        assert got[name] == want[name], "%s differs from a reopened Database's" % name
    ranked = held.query_dense_stats_batch(q, qstart, qlen, n=3)[1]
    assert all(song not in gone for per in ranked for _, (song, _) in per)
