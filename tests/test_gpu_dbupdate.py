"""Database updates on the GPU: an updated handle (pfann_db_append / pfann_db_remove_songs) answers every query form with
the bytes of a fresh handle loaded with the resulting rows, and an updated directory is the one a build writes.  Every
comparison is equality of bytes: there is no tolerance in this file."""
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

from pfann_amd import synth

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_SONGS, BIG, K = 40, 17, 100
MODES = {"copy": ("f32", True), "f32": ("f32", False), "f16": ("f16", True)}       # storage, pre-filter
_rows = {}


def rows(d):
    """~5,000 unit-norm rows in 40 songs of ragged lengths (songs 5 and 20 have none), song 17 scaled to norm 50;
    query rows are noisy copies of database rows"""
    if d not in _rows:
        rng = np.random.default_rng(1000 + d)
        lens = rng.integers(60, 200, N_SONGS)
        lens[[5, 20]] = 0
        x = rng.standard_normal((int(lens.sum()), d)).astype(np.float32)
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        pos = np.pad(np.cumsum(lens), (1, 0)).astype(np.int64)
        x[pos[BIG]:pos[BIG + 1]] *= 50.0
        pick = rng.integers(0, x.shape[0], 200)
        q = x[pick] / np.linalg.norm(x[pick], axis=1, keepdims=True) + 0.05 * rng.standard_normal((200, d)).astype(np.float32)
        q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
        _rows[d] = (x, lens.astype(np.int64), q)
    return _rows[d]


def pos_of(lens):
    return np.pad(np.cumsum(lens), (1, 0)).astype(np.int64)


def new_index(d, mode, emb=None, lens=None):
    from pfann_amd.database import DeviceIndex
    storage, pre = MODES[mode]
    idx = DeviceIndex(d, 0, storage=storage)
    if emb is not None:
        idx.load(np.ascontiguousarray(emb), pos_of(lens))
    idx.set_prefilter(pre)
    return idx


def b(t):
    import torch
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).tobytes()


def snapshot(idx, q_np, dense=True):
    """the bytes of every answer the issue lists -> (dict, kernels the compared searches ran)"""
    import torch
    q = torch.from_numpy(q_np).cuda()
    out, kernels = {}, []
    pos = idx.song_pos
    for nq in (1, 19, 76, 200):
        D, I = idx.search(q[:nq], K)
        out["search%d" % nq] = b(D) + b(I)
        stages, flags = idx.search_plan(nq, K)
        out["plan%d" % nq] = repr((stages, sorted(flags.items())))
        kernels += [s[0] for s in stages]
    songs = np.arange(76) % max(idx.n_songs, 1)
    D, I = idx.search(q[:76], K, exclude=(pos[songs], pos[songs + 1]))
    out["excl"] = b(D) + b(I)
    out["plan_excl"] = repr(idx.search_plan(76, K, excl=True))
    c = idx.search_bound(q[:76], K, 4)
    lb = idx.reduce_bound(c[None], K)
    D, I = idx.search_bounded(q[:76], K, lb)
    out["bound"] = b(c) + b(lb) + b(D) + b(I)
    D, I = idx.search(q, K)
    qstart, qlen = np.arange(10) * 20, np.full(10, 20)
    res, ss = idx.match(q, I, qstart, qlen, want_song_scores=True)
    out["match"] = b(res) + b(ss)
    top, found = idx.match_topn(q, I, qstart, qlen, 5)
    out["match_topn"] = b(top) + b(found)
    rstart, rlen = [0, 100], [100, 100]
    res, wfirst = idx.match_windows(q, I, rstart, rlen, 19, 7)
    out["windows"] = b(res) + b(wfirst)
    (top, found), wfirst = idx.match_windows_topn(q, I, rstart, rlen, 19, 7, 3)
    out["windows_topn"] = b(top) + b(found)
    if dense and idx.storage == "f32":
        res, wfirst = idx.match_windows_dense(q[:40], [0], [40], 8, 4)
        out["dense"] = b(res)
    out["owned"] = repr(idx.owned_songs())
    out["norm_max"] = struct.pack("<f", idx.row_norm_max())
    out["counts"] = repr((idx.ntotal, idx.n_songs, int(idx.lib.pfann_db_ntotal(idx.handle)), int(idx.lib.pfann_db_bytes(idx.handle))))
    out["song_pos"] = b(idx.song_pos)
    torch.cuda.synchronize()
    return out, kernels


def assert_same(idx, d, mode, emb, lens, need_f16_scan=True):
    x, _, q = rows(d)
    fresh = new_index(d, mode, emb, lens)
    got, kernels = snapshot(idx, q)
    want, _ = snapshot(fresh, q)
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name
    if need_f16_scan and mode != "f32":
        assert any(kn.startswith("scan_f16") for kn in kernels), kernels     # the fp16 rows' tail is really read
    return got


def keep_rows(x, lens, gone):
    pos = pos_of(lens)
    keep = np.ones(x.shape[0], bool)
    new = lens.copy()
    for s in gone:
        keep[pos[s]:pos[s + 1]] = False
        new[s] = 0
    return x[keep], new


@pytest.mark.parametrize("d,mode", [(128, "copy"), (128, "f32"), (128, "f16"), (64, "copy")])
def test_appends_give_the_fresh_handles_bytes(d, mode):
    import torch
    x, lens, q = rows(d)
    pos = pos_of(lens)
    s1, s2, s3 = 13, 22, 30               # song 20 (no rows) is part of the second append
    idx = new_index(d, mode, x[:pos[s1]], lens[:s1])
    # 1. within a reservation: no reallocation
    cap = idx.reserve(int(pos[s2]) + 7, s2)
    assert cap >= pos[s2] + 7 and idx.capacity() == cap
    assert idx.append(x[pos[s1]:pos[s2]], lens[s1:s2]) == s1
    assert idx.capacity() == cap and idx.ntotal == pos[s2] and idx.n_songs == s2
    assert_same(idx, d, mode, x[:pos[s2]], lens[:s2], need_f16_scan=False)
    # 2. beyond it: geometric growth
    idx.append(x[pos[s2]:pos[s3]], lens[s2:s3])
    assert idx.capacity() >= max(int(pos[s3]), cap + cap // 2)
    assert_same(idx, d, mode, x[:pos[s3]], lens[:s3], need_f16_scan=False)
    # 3. device-resident rows, a song without rows among them, then nothing but a song without rows
    tail = np.concatenate([lens[s3:35], [0], lens[35:]])
    idx.append(torch.from_numpy(x[pos[s3]:]).cuda(), tail)
    idx.append(np.zeros((0, d), np.float32), [0])
    assert_same(idx, d, mode, x, np.concatenate([lens[:s3], tail, [0]]))
    assert idx.capacity() >= idx.ntotal == x.shape[0]


REMOVE_CASES = {"first": [0], "last": [N_SONGS - 1], "adjacent": [8, 9, 10], "scattered": [30, 2, 14, 25, 2], "no_rows": [5],
                "big": [BIG], "first_and_big": [0, BIG, 39]}


@pytest.mark.parametrize("case", sorted(REMOVE_CASES))
@pytest.mark.parametrize("d,mode", [(128, "copy"), (128, "f32"), (128, "f16"), (64, "copy")])
def test_removals_give_the_fresh_handles_bytes(monkeypatch, d, mode, case):
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")       # many chunks: a chunk's destination is a later chunk's source
    x, lens, q = rows(d)
    gone = REMOVE_CASES[case]
    idx = new_index(d, mode, x, lens)
    before = idx.row_norm_max()
    idx.remove_songs(gone)
    kept, new_lens = keep_rows(x, lens, gone)
    got = assert_same(idx, d, mode, kept, new_lens)
    if mode != "f32":
        assert 49.0 < before < 51.0
        after = struct.unpack("<f", got["norm_max"])[0]
        assert (after < 1.01) == (BIG in gone) and (BIG in gone or after == before)


@pytest.mark.parametrize("mode", ["copy", "f16"])
def test_remove_all_then_append(monkeypatch, mode):
    monkeypatch.setenv("PFANN_DB_MOVE_ROWS", "64")
    d = 128
    x, lens, q = rows(d)
    pos = pos_of(lens)
    idx = new_index(d, mode, x, lens)
    idx.remove_songs(list(range(N_SONGS)))
    assert idx.ntotal == 0 and idx.row_norm_max() == 0.0
    assert_same(idx, d, mode, x[:0], np.zeros(N_SONGS, np.int64), need_f16_scan=False)       # an empty database
    idx.append(x, lens)                                   # the ids go on behind the removed ones
    assert_same(idx, d, mode, x, np.concatenate([np.zeros(N_SONGS, np.int64), lens]))
    # remove, append, remove again: the moved rows and the appended tail together
    idx.remove_songs([N_SONGS + 3, N_SONGS + BIG])
    kept, new_lens = keep_rows(x, lens, [3, BIG])
    idx.append(x[pos[3]:pos[4]], [lens[3]])
    assert_same(idx, d, mode, np.concatenate([kept, x[pos[3]:pos[4]]]),
                np.concatenate([np.zeros(N_SONGS, np.int64), new_lens, [lens[3]]]))


def test_a_norm_beyond_the_fp16_copys_range_drops_it_and_its_removal_brings_it_back():
    """pfann_db_load's 1e4 rule, as a fresh load would apply it after every update"""
    d = 128
    x, lens, q = rows(d)
    idx = new_index(d, "copy", x, lens)
    huge = (x[:30] * 2.0e4).astype(np.float32)
    idx.append(huge, [30])
    assert idx.set_prefilter(True) is False
    assert_same(idx, d, "copy", np.concatenate([x, huge]), np.concatenate([lens, [30]]), need_f16_scan=False)
    idx.remove_songs([N_SONGS])
    assert idx.set_prefilter(True) is True
    assert_same(idx, d, "copy", x, np.concatenate([lens, [0]]))


def test_refused_calls_leave_the_handle_unchanged():
    import torch
    from pfann_amd.lib import PfannError
    d = 128
    x, lens, q = rows(d)
    pos = pos_of(lens)
    qd = torch.from_numpy(q).cuda()

    def answers(idx):
        D, I = idx.search(qd, K)
        return b(D) + b(I) + repr((idx.ntotal, idx.n_songs, idx.capacity(), idx.owned_songs())).encode() + b(idx.song_pos)

    for mode in ("copy", "f16"):
        idx = new_index(d, mode, x, lens)
        before = answers(idx)
        with pytest.raises(PfannError, match="rows"):
            idx.append(x[:10], [4, 5])                    # row-count mismatch
        with pytest.raises(PfannError):
            idx.append(x[:10], [12, -2])
        with pytest.raises(PfannError, match="outside"):
            idx.remove_songs([3, N_SONGS])                # a bad song id beside a good one
        with pytest.raises(PfannError):
            idx.remove_songs([-1])
        if mode == "f16":
            bad = x[:300].copy()
            bad[299] *= 7.0e4                             # beyond capacity, so the call had grown its buffers before it saw the row
            with pytest.raises(PfannError, match="fp16"):
                idx.append(bad, [300])
        assert answers(idx) == before
    # a shard of a song-sharded database (label_base > 0)
    from pfann_amd.database import DeviceIndex
    shard = DeviceIndex(d, 0)
    shard.load(x[pos[20]:], pos, label_base=int(pos[20]), song_range=(20, N_SONGS))
    before = answers(shard)
    with pytest.raises(PfannError, match="shard of the database"):
        shard.append(x[:10], [10])
    with pytest.raises(PfannError, match="shard of the database"):
        shard.remove_songs([25])
    assert answers(shard) == before


# ------------------------------------------------------------------------------------------------ Database and the CLIs
def _run(args, cwd, env):
    r = subprocess.run([sys.executable] + args, capture_output=True, text=True, env=env, cwd=cwd, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_incremental_directory_is_the_built_one_and_an_open_database_follows(tmp_path):
    import torch
    from pfann_amd import dbfiles
    from pfann_amd.database import Database
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    d = params["model"]["d"]
    sd = synth.make_state_dict(params, seed=321)
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "tiny.json"), str(mdir / "configs.json"))
    music, songs = [], {}
    for s in range(9):
        path = str(tmp_path / ("song%02d.wav" % s))
        if s == 6:
            open(path, "wb").write(b"garbage")           # unreadable, in B: a song without rows
        else:
            songs[s] = synth.make_song(200 + s, seconds=8.0 + s)
            synth.write_wav(path, songs[s], sr=16000 if s == 7 else 8000)       # song 7 (in B) is stored at 16 kHz
        music.append(path)
    lists = {}
    for name, part in (("a", music[:5]), ("b", music[5:]), ("ab", music)):
        lists[name] = str(tmp_path / (name + ".txt"))
        open(lists[name], "w").write("".join(p + "\n" for p in part))
    queries = []
    for j, s in enumerate([0, 2, 3, 5, 8]):
        qw, _ = synth.make_query(songs[s], j, 4.0, snr_db=20.0)
        path = str(tmp_path / ("q%02d.wav" % j))
        synth.write_wav(path, qw)
        queries.append(path)
    qlist = str(tmp_path / "queries.txt")
    open(qlist, "w").write("".join(p + "\n" for p in queries))
    env = dict(os.environ, PYTHONPATH=REPO)
    env.pop("PFANN_GPUS", None)
    cwd = str(tmp_path)
    whole, grown = str(tmp_path / "db_whole"), str(tmp_path / "db_grown")
    _run([os.path.join(REPO, "builder.py"), lists["ab"], whole, str(mdir)], cwd, env)
    _run([os.path.join(REPO, "builder.py"), lists["a"], grown, str(mdir)], cwd, env)
    out = _run([os.path.join(REPO, "dbupdate.py"), "add", lists["b"], grown], cwd, env)
    assert "selfmatch.py %s dup.tsv --songs 5:9" % grown in out
    files = ("embeddings", "landmarkValue", "landmarkKey", "songList.txt")
    for f in files:
        assert open(os.path.join(grown, f), "rb").read() == open(os.path.join(whole, f), "rb").read(), f
    key = dbfiles.read_key(grown)
    assert key[6] == 0 and key[7] > 0 and (key[:5] > 0).all()

    def match(db, tag):
        res = str(tmp_path / (tag + ".txt"))
        _run([os.path.join(REPO, "matcher.py"), qlist, db, res], cwd, env)
        stem = os.path.splitext(res)[0]
        return [open(p, "rb").read() for p in (res, stem + "_detail.csv", res + ".bin")]
    assert match(grown, "r_grown") == match(whole, "r_whole")

    # ---- a Database held open across the removal, then the removal on disk
    hop = params["hop_size"]
    held = Database(grown, params["indexer"], hop, d=d)
    emb_before = np.fromfile(os.path.join(grown, "embeddings"), np.float32).reshape(-1, d)
    rm = str(tmp_path / "rm.txt")
    open(rm, "w").write(music[2] + "\n#5\n")
    _run([os.path.join(REPO, "dbupdate.py"), "remove", rm, grown], cwd, env)
    kept, new_key = keep_rows(emb_before, key.astype(np.int64), [2, 5])
    assert np.fromfile(os.path.join(grown, "embeddings"), np.float32).tobytes() == kept.tobytes()
    from pfann_amd import faissio
    assert faissio.read_index_flat(os.path.join(grown, "landmarkValue"))[0].tobytes() == kept.tobytes()
    assert np.array_equal(dbfiles.read_key(grown), new_key.astype(np.int32))
    assert open(os.path.join(grown, "songList.txt"), "rb").read() == open(os.path.join(whole, "songList.txt"), "rb").read()
    res = match(grown, "r_removed")[0].decode("utf8")
    assert music[2] not in res.replace(queries[1], "") and music[5] not in res and len(res.splitlines()) == len(queries)

    assert held.remove_songs([music[2], 5], persist=False) == [2, 5]
    opened = Database(grown, params["indexer"], hop, d=d)
    assert np.array_equal(held.song_pos, opened.song_pos) and held.songList == opened.songList
    q = torch.from_numpy(np.ascontiguousarray(emb_before[:60])).cuda()
    qstart, qlen = [0, 20, 40], [20, 20, 20]
    a = held.query_batch(q, qstart, qlen, want_song_scores=True)
    c = opened.query_batch(q, qstart, qlen, want_song_scores=True)
    assert len(a) == len(c) == 3
    for ra, rc in zip(a, c):
        assert ra[:2] == rc[:2] and ra[2].tobytes() == rc[2].tobytes()
    # self-match reads the rows of the updated file (the memory map of the old one was dropped)
    sa = [(s, r.tobytes()) for s, r in held.self_match(0, 9, 8, 4)]
    sc = [(s, r.tobytes()) for s, r in opened.self_match(0, 9, 8, 4)]
    assert sa == sc and len(sa) == 9 and held._embeddings_map().shape[0] == kept.shape[0]

    # ---- and an add through the open Database: the files are the ones the CLI's add wrote before
    again = str(tmp_path / "db_again")
    shutil.copytree(grown, again)
    db2 = Database(again, params["indexer"], hop, d=d)
    first = db2.add_songs(["x.wav", "y.wav"], emb_before[:30], [30, 0])
    assert first == 9 and len(db2.songList) == 11 and db2.song_pos[-1] == kept.shape[0] + 30
    reopened = Database(again, params["indexer"], hop, d=d)
    assert np.array_equal(reopened.song_pos, db2.song_pos) and reopened.songList == db2.songList
    a = db2.query_batch(q, qstart, qlen, want_song_scores=True)
    c = reopened.query_batch(q, qstart, qlen, want_song_scores=True)
    for ra, rc in zip(a, c):
        assert ra[:2] == rc[:2] and ra[2].tobytes() == rc[2].tobytes()
