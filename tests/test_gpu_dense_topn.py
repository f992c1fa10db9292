"""The ranked dense matcher on the GPU (pfann_match_windows_dense_topn, csrc/dense.hip): every entry of every window, n_found
and the per-song block against the float64 oracle of tests/dense_topn_cases.py with `==` on the exact grid; the product's own
pfann_match_topn with every row as a label; entry 0 against pfann_match_windows_dense and the prefix rule on real-valued rows;
the byte contract across hops, batching, chunking and runs; ties, the exclusion, database updates, the refusals; and
matcher.py --dense / Database.self_match(top=) with it."""
import csv
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_topn_cases as dt
import match_exact as mx
import monitor_cases as mc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
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


def _topn(torch, idx, q, rstart, rlen, window, hop, n, block=True, **kw):
    """-> (top [nW, n], n_found [nW], block [nW, n_songs, 2] or None, wfirst)"""
    (top, n_found, ss), wfirst = idx.match_windows_dense_topn(torch.as_tensor(q).cuda(), rstart, rlen, window, hop, n,
                                                              want_song_scores=block, **kw)
    return top, n_found, ss, wfirst


def _grid_world(d, seed=300):
    world = mx.std_world(41, d, long_rows=300)
    db, pos, q, _, rstart, rlen = mc.grid_recordings(d, 20, world=world, seed=seed)
    return db, pos, q, rstart, rlen


# ------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("window", mc.WINDOWS)
def test_every_window_equals_the_ranked_oracle(torch_cuda, window):
    """the grid world of tests/test_gpu_dense.py; windows 1 / 5 / 19 / 64 x hops 1 / 2 / 7 x n 1 / 3 / 64 (more than the
    songs: padding): every field of every entry, n_found and the block, =="""
    db, pos, q, rstart, rlen = _grid_world(D)
    assert np.diff(pos).max() == 300 > 128 and 0 < np.diff(pos)[np.diff(pos) > 0].min() < 5 and 11 in rlen and 0 in rlen
    assert int((np.diff(pos) > 0).sum()) < 64
    mx.assert_exact_domain(window, D)
    idx = _index("grid", db, pos)
    for hop in mc.HOPS:
        for n in (1, 3, 64):
            want = dt.dense_topn_oracle(q, db, pos, window, hop, rstart, rlen, n, key="grid")
            top, n_found, block, wfirst = _topn(torch_cuda, idx, q, rstart, rlen, window, hop, n, block=n == 3)
            assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop)) and top.shape == (len(want), n) and len(want) > 0
            bad = dt.differing(top, n_found, block, want)
            assert not bad, "window %d hop %d n %d: %d of %d windows differ\n%s" % (window, hop, n, len(bad), len(want), "\n".join(bad[:6]))
            if n == 64:
                assert (top["song"][:, -1] == -1).all() and np.isneginf(top["score"][:, -1]).all()


@pytest.mark.parametrize("window", [5, 19])
def test_packed_world(torch_cuda, window):
    """128 distinct songs in one tile, up to `window` pieces on one stretch, empty songs between them, songs longer than a tile"""
    db, pos, q, rstart, rlen = dt.packed_world(D)
    assert (np.diff(pos) == 1).sum() == 200 and (np.diff(pos) == 0).sum() > 5 and (np.diff(pos) == 300).sum() == 2
    mx.assert_exact_domain(window, D)
    idx = _index("packed", db, pos)
    for hop in (1, 3):
        want = dt.dense_topn_oracle(q, db, pos, window, hop, rstart, rlen, 64, key="packed")
        top, n_found, block, _ = _topn(torch_cuda, idx, q, rstart, rlen, window, hop, 64)
        bad = dt.differing(top, n_found, block, want)
        assert not bad, "window %d hop %d: %d of %d windows differ\n%s" % (window, hop, len(bad), len(want), "\n".join(bad[:6]))
        assert (n_found == 202).all()


@pytest.mark.parametrize("d", [64, 256])
def test_other_row_widths(torch_cuda, d):
    db, pos, q, rstart, rlen = _grid_world(d, seed=340)
    mx.assert_exact_domain(19, d)
    want = dt.dense_topn_oracle(q, db, pos, 19, 3, rstart, rlen, 5, key=("grid-d", d))
    top, n_found, block, _ = _topn(torch_cuda, _index(("grid-d", d), db, pos), q, rstart, rlen, 19, 3, 5)
    bad = dt.differing(top, n_found, block, want)
    assert not bad, "d %d: %d of %d windows differ\n%s" % (d, len(bad), len(want), "\n".join(bad[:6]))


def test_equals_match_topn_with_every_row_as_a_label(torch_cuda):
    """the product's own ranked matcher on the expanded windows, labels = all rows, k = ntotal: every field =="""
    db, pos, q, rstart, rlen = dc.small_world()
    window, n = 19, 5
    assert window * db.shape[0] <= mx.MAXC
    idx = _index("small", db, pos)
    labels = dc.all_labels(q.shape[0], db.shape[0])
    for hop in (1, 2):
        top, n_found, _, _ = _topn(torch_cuda, idx, q, rstart, rlen, window, hop, n, block=False)
        qs, ql = mc.expand(rstart, rlen, window, hop)
        ref, ref_found = idx.match_topn(torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda(), qs, ql, n)
        for f in dt.FIELDS:
            assert np.array_equal(top[f], ref[f]), "hop %d: field %s differs in %d entries" % (hop, f, int((top[f] != ref[f]).sum()))
        assert np.array_equal(n_found, ref_found)


# ------------------------------------------------------------------------------------------------ real-valued rows
@pytest.fixture(scope="module")
def unit400():
    return mc.unit_case(7, 120, D, 100, 400)


def test_entry_0_is_the_dense_answer_and_the_prefix_rule(torch_cuda, unit400):
    db, pos, q, _ = unit400
    window, hop, L = 19, 2, q.shape[0]
    idx = _index("unit400", db, pos)
    res, _ = idx.match_windows_dense(torch_cuda.as_tensor(q).cuda(), [0], [L], window, hop)
    t10, f10, _, _ = _topn(torch_cuda, idx, q, [0], [L], window, hop, 10, block=False)
    t3, f3, _, _ = _topn(torch_cuda, idx, q, [0], [L], window, hop, 3, block=False)
    assert len(res) == len(t10) == len(t3) > 100
    for f in ("song", "offset", "shift"):
        assert np.array_equal(t10[f][:, 0], res[f]), f
    assert t10["score"][:, 0].tobytes() == res["score"].tobytes(), "entry 0 has other score bytes than pfann_match_windows_dense"
    assert t3.tobytes() == np.ascontiguousarray(t10[:, :3]).tobytes() and np.array_equal(f3, f10)
    assert (np.diff(t10["score"], axis=1) <= 0).all() and (f10 == 120).all()
    assert len({float(x) for x in t10["score"][:, 0]}) > len(t10) // 2, "the scores are not real-valued"


def test_a_window_has_the_same_bytes_whatever_reached_it(torch_cuda, monkeypatch):
    """hop 1 at the default chunk size against hops 3 and 7, alone and batched behind a second recording of 137 rows,
    PFANN_DENSE_TOPN_WINDOWS = 1 and 7 (one row-tile slot per chunk: the 300 rows span several), twice in a row"""
    db, pos, q, _ = mc.unit_case(11, 40, D, 10, 300)
    window, L, other, n = 19, q.shape[0], 137, 4
    assert L == 300
    idx = _index("unit300", db, pos)
    monkeypatch.delenv("PFANN_DENSE_TOPN_WINDOWS", raising=False)
    base = _topn(torch_cuda, idx, q, [0], [L], window, 1, n)[:3]
    q2 = np.concatenate([q[:other][::-1], q])

    def same(got, step, what, first=0):
        for a, b, name in zip(base, got, ("top", "n_found", "block")):
            assert np.ascontiguousarray(a[::step]).tobytes() == np.ascontiguousarray(b[first:]).tobytes(), "%s: other %s bytes" % (what, name)

    same(_topn(torch_cuda, idx, q, [0], [L], window, 1, n)[:3], 1, "twice in a row")
    for hop in (3, 7):
        same(_topn(torch_cuda, idx, q, [0], [L], window, hop, n)[:3], hop, "hop %d" % hop)
        *got, wf = _topn(torch_cuda, idx, q2, [0, other], [other, L], window, hop, n)
        same(got, hop, "hop %d behind another recording" % hop, int(wf[1]))
    *got, wf = _topn(torch_cuda, idx, q2, [0, other], [other, L], window, 1, n)
    same(got, 1, "behind another recording", int(wf[1]))
    for cap in ("1", "7"):
        monkeypatch.setenv("PFANN_DENSE_TOPN_WINDOWS", cap)
        same(_topn(torch_cuda, idx, q, [0], [L], window, 1, n)[:3], 1, "PFANN_DENSE_TOPN_WINDOWS=" + cap)
        same(_topn(torch_cuda, idx, q, [0], [L], window, 3, n)[:3], 3, "hop 3, PFANN_DENSE_TOPN_WINDOWS=" + cap)
        *got, wf = _topn(torch_cuda, idx, q2, [0, other], [other, L], window, 1, n)
        same(got, 1, "behind another recording, PFANN_DENSE_TOPN_WINDOWS=" + cap, int(wf[1]))
    assert len({float(x) for x in base[0]["score"][:, 0]}) > len(base[0]) // 2, "the scores are not real-valued"


# ------------------------------------------------------------------------------------------------ ties
def test_ties_go_to_the_lower_song_and_the_lower_offset(torch_cuda):
    """a window cut from inside the copied, periodic song 5 of the standard world (copy: song 9, period 4): both copies tie
    exactly, song 5 ranks first, and each reports the smallest of its tying offsets"""
    db, pos, _, _, _ = _grid_world(D)
    a, b = mx.STD_COPIES[0]
    assert (a, 4) == mx.STD_PERIODIC[0] and np.array_equal(db[pos[a]:pos[a + 1]], db[pos[b]:pos[b + 1]])
    la = int(pos[a + 1] - pos[a])
    assert la >= 5 + 8, "song %d is too short for a window of 5 rows at two periods" % a
    q = db[pos[a] + 4:pos[a] + 9]
    top, n_found, _, _ = _topn(torch_cuda, _index("grid", db, pos), q, [0], [5], 5, 1, 3, block=False)
    e0, e1 = top[0, 0], top[0, 1]
    assert (int(e0["song"]), int(e1["song"])) == (a, b) and float(e0["score"]) == float(e1["score"]), top[0]
    assert int(e0["offset"]) == int(e1["offset"]) == 0, "the periodic song ties at offsets 0, 4, 8, ..: the lowest wins (%r)" % top[0]
    assert float(e0["score"]) == float(np.sum(q.astype(np.float64) ** 2) / 5)


# ------------------------------------------------------------------------------------------------ exclusion
def test_excluded_song(torch_cuda):
    db, pos, _, _, _ = _grid_world(D)
    A = int(np.flatnonzero(np.diff(pos) == 300)[0])
    cut = db[pos[A] + 40:pos[A] + 150]
    q = np.concatenate([cut, cut])
    rstart, rlen, excl = [0, cut.shape[0]], [cut.shape[0]] * 2, [A, -1]
    idx = _index("grid", db, pos)
    window, hop, n = 19, 2, 64
    top, n_found, block, _ = _topn(torch_cuda, idx, q, rstart, rlen, window, hop, n, exclude_song=excl)
    want = dt.dense_topn_oracle(q, db, pos, window, hop, rstart, rlen, n, excl=excl)
    bad = dt.differing(top, n_found, block, want)
    assert not bad, "%d windows differ\n%s" % (len(bad), "\n".join(bad[:6]))
    half = len(top) // 2
    assert (top["song"][:half] != A).all() and (top["song"][half:, 0] == A).all()
    assert (n_found[half:] - n_found[:half] == 1).all()
    assert (block[:half, A] == 0).all() and (block[half:, A, 0] > 0).all()
    none = _topn(torch_cuda, idx, q, rstart, rlen, window, hop, n)
    minus = _topn(torch_cuda, idx, q, rstart, rlen, window, hop, n, exclude_song=[-1, -1])
    for x, y in zip(none[:3], minus[:3]):
        assert x.tobytes() == y.tobytes(), "NULL and all -1 give different bytes"
    one = _index("one-song", cut, np.asarray([0, cut.shape[0]], np.int64))
    top, n_found, block, _ = _topn(torch_cuda, one, q, rstart, rlen, window, hop, 3, exclude_song=[0, 0])
    assert len(top) > 0 and (top["song"] == -1).all() and np.isneginf(top["score"]).all() and (top["n_cand"] == 0).all()
    assert (n_found == 0).all() and (block == 0).all()


# ------------------------------------------------------------------------------------------------ updates
def test_after_an_update_the_call_answers_as_a_fresh_handle(torch_cuda):
    from pfann_amd.database import DeviceIndex
    db, pos, q, rstart, rlen = dc.small_world()
    lens = np.diff(pos)
    idx = DeviceIndex(D, 0)
    idx.load(db, pos)
    before = _topn(torch_cuda, idx, q, rstart, rlen, 19, 2, 5)            # (sizes the workspace for the old number of songs)
    extra = mx.grid_rows(91, "topn/append", 37, D)
    idx.append(extra, [37])
    gone = int(np.flatnonzero(lens > 20)[0])
    idx.remove_songs([gone])
    keep = np.ones(db.shape[0], bool)
    keep[pos[gone]:pos[gone + 1]] = False
    new_lens = np.concatenate([lens, [37]])
    new_lens[gone] = 0
    new_pos = np.pad(np.cumsum(new_lens), (1, 0)).astype(np.int64)
    fresh = DeviceIndex(D, 0)
    fresh.load(np.concatenate([db[keep], extra]), new_pos)
    got = _topn(torch_cuda, idx, q, rstart, rlen, 19, 2, 5)
    ref = _topn(torch_cuda, fresh, q, rstart, rlen, 19, 2, 5)
    for x, y, name in zip(got[:3], ref[:3], ("top", "n_found", "block")):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s differs from a fresh handle's" % name
    assert got[2].shape[1] == len(lens) + 1 and (got[1] == before[1]).all() and (got[0]["song"] != gone).all()
    want = dt.dense_topn_oracle(q, np.concatenate([db[keep], extra]), new_pos, 19, 2, rstart, rlen, 5)
    assert not dt.differing(*got[:3], want)


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
    rs = torch.zeros(1, dtype=torch.int64).cuda()
    rl = torch.full((1,), 30, dtype=torch.int32).cuda()
    n_songs = len(pos) - 1

    def call(idx, window, hop, n):
        nW = int(mc.wfirst_of([30], max(window, 1), max(hop, 1))[-1])
        wf = torch.as_tensor(np.asarray([0, nW], np.int64)).cuda()
        outs = [torch.full((max(nW, 1) * size,), 0xA5, dtype=torch.uint8).cuda()
                for size in (max(n, 64) * ctypes.sizeof(L.MatchResult), 4, n_songs * 8)]
        rc = lib.pfann_match_windows_dense_topn(idx.handle, q.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, window, hop, wf.data_ptr(),
                                                nW, None, n, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, [bool((o.cpu() == 0xA5).all()) for o in outs]

    rc, _, untouched = call(whole, 5, 1, 3)               # the control: the same call on a good handle writes all three
    assert rc == 0 and not any(untouched)
    for idx, window, hop, n, word in ((whole, 5, 1, 0, "n="), (whole, 5, 1, 65, "n="), (whole, 65, 1, 3, "window"), (whole, 0, 1, 3, "window"),
                                      (whole, 5, 0, 3, "hop"), (half, 5, 1, 3, "fp16"), (shard, 5, 1, 3, "shard"),
                                      (shard, 5, 1, 0, "n=0"), (half_shard, 5, 1, 3, "shard")):   # two at once: the first one
        rc, msg, untouched = call(idx, window, hop, n)
        assert rc == -1 and msg and word in msg and all(untouched), (window, hop, n, word, rc, msg, untouched)
    try:
        shard.match_windows(q, torch.zeros((30, 4), dtype=torch.int64).cuda(), [0], [30], 5, 1)
    except L.PfannError as e:
        nominated = str(e).split(": ", 1)[1]
    assert call(shard, 5, 1, 3)[1] == nominated, "a shard is refused with another message than pfann_match_windows'"
    with pytest.raises(L.PfannError, match="shard"):
        shard.match_windows_dense_topn(q, [0], [30], 5, 1, 3)


# ------------------------------------------------------------------------------------------------ matcher.py --dense
def _rows(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.reader(f))


def test_matcher_cli_dense_end_to_end(torch_cuda, tmp_path):
    """the synthetic dataset of tests/test_gpu_cli_topn.py (12 songs, 12 five-second queries at SNR 0 and one unreadable file),
    builder.py once, then matcher.py plain, --dense, --dense --top 3 and --dense --top 3 --no-bin"""
    import json
    import shutil
    from pfann_amd import synth
    from pfann_amd.builder import embed_files
    from pfann_amd.database import Database
    from pfann_amd.engine import Engine
    from pfann_amd.musicdata import MusicDataset
    torch = torch_cuda
    params = json.load(open(os.path.join(REPO, "configs", "tiny.json")))
    sd = synth.make_state_dict(params, seed=11)
    mdir = tmp_path / "model"
    mdir.mkdir()
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, str(mdir / "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "tiny.json"), str(mdir / "configs.json"))
    env = dict(os.environ, PYTHONPATH=REPO)
    data = str(tmp_path / "data")

    def run(*cmd):
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable] + list(cmd), capture_output=True, text=True, env=env,
                           cwd=str(tmp_path), timeout=460)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]

    run(os.path.join(REPO, "tools", "gen_synth_dataset.py"), data, "--songs", "12", "--queries", "12", "--seconds", "5",
        "--song-seconds", "12", "--snr", "0")
    qlist = os.path.join(data, "query_snr0", "list.txt")
    open(qlist, "a").write(os.path.join(data, "nope.wav") + "\n")
    dbdir = str(tmp_path / "db")
    run(os.path.join(REPO, "builder.py"), os.path.join(data, "music.txt"), dbdir, str(mdir))
    out = {}
    for name, flags in (("plain", []), ("dense", ["--dense"]), ("top", ["--dense", "--top", "3"]),
                        ("nobin", ["--dense", "--top", "3", "--no-bin"])):
        out[name] = str(tmp_path / (name + ".txt"))
        run(os.path.join(REPO, "matcher.py"), qlist, dbdir, out[name], *flags)
    stem = lambda p: os.path.splitext(p)[0]
    songs = [ln.rstrip("\n") for ln in open(os.path.join(dbdir, "songList.txt"), encoding="utf8")]
    tsv = {k: [ln.rstrip("\n").split("\t") for ln in open(p, encoding="utf8")] for k, p in out.items()}
    detail = {k: _rows(stem(p) + "_detail.csv") for k, p in out.items()}
    nq = len(tsv["plain"])
    assert nq == 13 and tsv["dense"][-1][1] == "error" and detail["dense"][0] == detail["plain"][0]
    assert tsv["dense"] == tsv["top"] == tsv["nobin"] and detail["dense"] == detail["top"] == detail["nobin"]
    assert [r[0] for r in tsv["dense"]] == [r[0] for r in tsv["plain"]]
    # the same embeddings through Database.query_dense_batch
    cfg = json.load(open(os.path.join(dbdir, "configs.json")))
    dataset = MusicDataset(qlist, cfg)
    engine = Engine(cfg, 0, max_batch=9728)
    engine.set_plan_batch(9728)
    if not engine.weights_loaded:
        engine.load_state_dict(torch.load(os.path.join(dbdir, "model.pt"), map_location="cpu"))
    embs = [(i, n, e) for i, n, e in embed_files(engine, dataset, dataset.hop, batch_windows=9728) if n]
    assert [i for i, _, _ in embs] == list(range(12)) and max(n for _, n, _ in embs) <= 64
    db = Database(dbdir, cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])
    qlen = [n for _, n, _ in embs]
    answers, ranked = db.query_dense_batch(torch.cat([e for _, _, e in embs]), np.concatenate([[0], np.cumsum(qlen)[:-1]]), qlen, n=3,
                                           want_song_scores=True)
    for j, (score, (song, time_s), block) in enumerate(answers):
        name, ans, sco, tim = detail["dense"][1 + j][:4]
        assert ans == tsv["dense"][j][1] == songs[song] and abs(float(sco) - score) <= 1e-6 and abs(float(tim) - time_s) <= 1e-6, (j, detail["dense"][1 + j], score, song, time_s)
        assert float(sco) >= float(detail["plain"][1 + j][2]) - 1e-6, "query %d: the dense score is below the nominated one" % j
        assert ranked[j][0] == (score, (song, time_s)) and block.shape == (len(songs), 2)
    # _top.csv: rank 1 is the TSV's answer; the error row; the same file without a .bin
    top = _rows(stem(out["top"]) + "_top.csv")
    assert top[0] == ["query", "rank", "answer", "score", "time"] and top == _rows(stem(out["nobin"]) + "_top.csv")
    first = [r for r in top[1:] if r[1] == "1"]
    assert [(r[0], r[2]) for r in first] == [(r[0], r[1]) for r in tsv["top"]]
    assert [r[3:] for r in first[:-1]] == [r[2:4] for r in detail["top"][1:-1]]
    assert max(int(r[1]) for r in top[1:]) == 3 and not os.path.exists(stem(out["dense"]) + "_top.csv")
    # .bin: n_queries x n_songs x 2 float32, each query's best score is its TSV score to float32
    for k in ("dense", "top"):
        blocks = np.fromfile(out[k] + ".bin", dtype=np.float32)
        assert blocks.size == nq * len(songs) * 2
        blocks = blocks.reshape(nq, len(songs), 2)
        assert (blocks[-1] == 0).all()
        for j in range(12):
            assert blocks[j, :, 0].max() == np.float32(float(detail[k][1 + j][2])), (k, j)
            assert np.array_equal(blocks[j], answers[j][2]), (k, j)
    assert np.fromfile(out["dense"] + ".bin", dtype=np.float32).tobytes() == np.fromfile(out["top"] + ".bin", dtype=np.float32).tobytes()
    assert not os.path.exists(out["nobin"] + ".bin")


# ------------------------------------------------------------------------------------------------ self-match
def test_self_match_dense_top_names_both_other_copies(torch_cuda, tmp_path):
    """song 2 is stored three times (songs 2, 7 and 12): with top=3 the merged tracks name both other copies over the whole song
    from song 2's side; top=1 names exactly one of them"""
    from pfann_amd.database import Database
    from pfann_amd.monitor import merge_window_tracks, merge_windows
    from pfann_amd.utils import read_config
    emb, pos = dt.triple_world(str(tmp_path))
    cfg = read_config(os.path.join(str(tmp_path), "configs.json"))
    db = Database(str(tmp_path), cfg["indexer"], cfg["hop_size"], d=cfg["model"]["d"])
    n2 = int(pos[3] - pos[2])
    win = min(dc.SELF_WINDOW, n2)
    ranked = dict(db.self_match(2, 3, dc.SELF_WINDOW, dc.SELF_HOP, dense=True, top=3))[2]
    assert ranked.shape == (len(mc.window_starts(n2, dc.SELF_WINDOW, dc.SELF_HOP)), 3)
    assert all({int(s) for s in row["song"][:2]} == {7, 12} for row in ranked) and (ranked["song"] != 2).all()
    assert ranked["score"][:, :2].min() > 0.99 > ranked["score"][:, 2].max()
    dets = merge_window_tracks(ranked, win, dc.SELF_HOP, dc.SELF_HOP_S, min_windows=2)
    whole = {int(d[2]): d for d in dets if d[6] == len(ranked)}
    assert set(whole) == {7, 12}, dets
    tol = dc.SELF_HOP * dc.SELF_HOP_S                  # (merge_windows' score-ratio edges move by a fraction of a hop: the copies carry 1e-3 noise)
    for d in whole.values():
        assert abs(d[0]) <= tol and abs(d[1] - n2 * dc.SELF_HOP_S) <= tol and abs(d[3] - d[0]) <= 1e-6, d
    single = dict(db.self_match(2, 3, dc.SELF_WINDOW, dc.SELF_HOP, dense=True, top=1))[2]
    assert single.ndim == 1 and len(single) == len(ranked) and {int(s) for s in single["song"]} <= {7, 12}
    assert np.array_equal(single["song"], ranked["song"][:, 0]) and np.array_equal(single["score"], ranked["score"][:, 0])
    over_all = {int(d[2]) for d in merge_windows(single, win, dc.SELF_HOP, dc.SELF_HOP_S, min_windows=2) if d[6] == len(single)}
    assert len(over_all) <= 1, "one answer per window cannot report both copies over the whole song"
    # the nominated path takes top= too (pfann_match_windows_topn on the masked search's labels)
    nominated = dict(db.self_match(2, 3, dc.SELF_WINDOW, dc.SELF_HOP, top=3))[2]
    assert nominated.shape == ranked.shape and all({int(s) for s in row["song"][:2]} == {7, 12} for row in nominated)


# ------------------------------------------------------------------------------------------------ the Database layer
def test_database_ranked_dense_methods(torch_cuda, tmp_path, monkeypatch):
    """monitor_dense_topn: entry 0 of every window is monitor_dense's row and the edge pass is ranked too; query_dense_batch:
    a query's answer does not depend on what it was batched with, and equals the one-window call; the refusals of _dense_check"""
    from pfann_amd import database as dbm
    from pfann_amd import lib as L
    from pfann_amd.utils import read_config
    torch = torch_cuda
    emb, pos = dc.selfmatch_world(str(tmp_path))
    cfg = read_config(os.path.join(str(tmp_path), "configs.json"))
    db = dbm.Database(str(tmp_path), cfg["indexer"], cfg["hop_size"], d=D)
    rec = torch.as_tensor(np.concatenate([emb[pos[2] + 5:pos[2] + 35], emb[pos[4]:pos[4] + 40]])).cuda()
    one = db.monitor_finish(db.monitor_dense_launch(rec, [0], [70], 19, 2, edge_window=7))
    p = db.monitor_dense_topn_launch(rec, [0], [70], 19, 2, 3, edge_window=7)
    (rows,), (n_found,) = db.monitor_dense_topn_finish(p)
    assert rows.shape == (len(one[0]), 3) and (n_found == 11).all() and p["edge_rows"][0].shape == (64, 3)
    for f in ("w0", "score", "song", "time_s"):
        assert np.array_equal(rows[f][:, 0], one[0][f]), f
    assert {int(s) for s in rows["song"][0, :2]} == {2, 7} and int(rows["votes"][0, 0]) == int(pos[3] - pos[2]) + 18
    qlen = [19, 7, 33, 1]
    qstart = np.concatenate([[0], np.cumsum(qlen)[:-1]])
    answers, ranked = db.query_dense_batch(rec[:60], qstart, qlen, n=3, want_song_scores=True)
    assert len(answers) == len(ranked) == 4 and all(len(r) == 3 for r in ranked)
    for j, (s, m) in enumerate(zip(qstart, qlen)):
        (alone,), (alone_ranked,) = db.query_dense_batch(rec[s:s + m], [0], [m], n=3, want_song_scores=True)
        assert alone[:2] == answers[j][:2] and alone_ranked == ranked[j] and alone[2].tobytes() == answers[j][2].tobytes(), j
        assert ranked[j][0] == answers[j][:2] and answers[j][2].shape == (12, 2)
        (top, _, _), _ = db.index.match_windows_dense_topn(rec[s:s + m], [0], [m], m, 1, 1)
        assert float(top["score"][0, 0]) == answers[j][0] and int(top["song"][0, 0]) == answers[j][1][0]
        best = int(np.argmax(answers[j][2][:, 0]))
        assert best == answers[j][1][0] and answers[j][2][best, 0] == np.float32(answers[j][0])
        assert answers[j][2][best, 1] == np.float32(answers[j][1][1]), "the block's alignment is in seconds"
    with pytest.raises(L.PfannError, match="64"):
        db.query_dense_batch(torch.zeros((65, D)).cuda(), [0], [65])
    for change, word in (({"frame_shift_mul": 2}, "frame_shift_mul"), ({"score_alpha": 2.0}, "score_alpha")):
        other = dbm.Database(str(tmp_path), dict(cfg["indexer"], **change), cfg["hop_size"], d=D)
        for call in (lambda: other.monitor_dense_topn_launch(rec, [0], [70], 19, 2, 3), lambda: other.query_dense_launch(rec[:19], [0], [19]),
                     lambda: other.self_match_launch(0, 12, 19, 2, dense=True, top=3)):
            with pytest.raises(L.PfannError, match=word):
                call()
    monkeypatch.setattr(dbm, "cpp_accelerate", True)
    with pytest.raises(L.PfannError, match="native"):
        db.query_dense_batch(rec[:19], [0], [19])
