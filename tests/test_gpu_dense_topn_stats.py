"""The ranked dense matcher with background statistics on the GPU (pfann_match_windows_dense_topn_stats, csrc/dense.hip): one
pass gives the bytes of pfann_match_windows_dense_topn AND the bytes of pfann_match_windows_dense_stats, which equal the
integer oracle of tests/dense_stats_cases.py; chunking, the byte contract, the refusals, updates, the Database layer and
matcher.py --dense --max-fa."""
import csv
import ctypes
import json
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_stats_cases as sc
import dense_topn_cases as dt
import match_exact as mx
import monitor_cases as mc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
HOPS = (1, 2, 3)


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


def _one_pass(torch, idx, q, rstart, rlen, window, hop, n, block=True, **kw):
    """-> (top, n_found, block or None, stats) of the one-pass call"""
    (top, n_found, ss, stats), _ = idx.match_windows_dense_topn_stats(torch.as_tensor(q).cuda(), rstart, rlen, window, hop, n,
                                                                      want_song_scores=block, **kw)
    return top, n_found, ss, stats


def _both_parents(torch, idx, q, rstart, rlen, window, hop, n, block=True, **kw):
    """the one-pass call, asserted byte-equal to match_windows_dense_topn (top, n_found, block) and to match_windows_dense_stats
    (stats) for the same arguments -> (top, n_found, block or None, stats, wfirst)"""
    qd = torch.as_tensor(q).cuda()
    (top, n_found, ss, stats), wfirst = idx.match_windows_dense_topn_stats(qd, rstart, rlen, window, hop, n, want_song_scores=block, **kw)
    (top0, nf0, ss0), wf0 = idx.match_windows_dense_topn(qd, rstart, rlen, window, hop, n, want_song_scores=block, **kw)
    (_, stats0), wf1 = idx.match_windows_dense_stats(qd, rstart, rlen, window, hop, **kw)
    what = "window %d hop %d n %d" % (window, hop, n)
    assert np.array_equal(wfirst, wf0) and np.array_equal(wfirst, wf1) and top.shape == top0.shape and stats.shape == stats0.shape
    assert top.tobytes() == top0.tobytes(), what + ": top is not match_windows_dense_topn's"
    assert n_found.tobytes() == nf0.tobytes(), what + ": n_found is not match_windows_dense_topn's"
    assert (ss is None) == (ss0 is None) and (ss is None or ss.tobytes() == ss0.tobytes()), what + ": the block is not match_windows_dense_topn's"
    assert stats.tobytes() == stats0.tobytes(), what + ": %d windows' stats are not match_windows_dense_stats'" % int((stats != stats0).sum())
    return top, n_found, ss, stats, wfirst


def _grid_world(d, seed=300):
    world = mx.std_world(41, d, long_rows=300)
    db, pos, q, _, rstart, rlen = mc.grid_recordings(d, 20, world=world, seed=seed)
    return db, pos, q, rstart, rlen


# ------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("window", mc.WINDOWS)
def test_one_pass_equals_both_parents_and_the_integer_oracle(torch_cuda, window):
    """the grid world of test_gpu_dense_stats.py -- songs of 300 rows (longer than a tile), songs shorter than the window, empty
    songs, copies, five recordings in one call with an 11-row one (one window of its own rows) and an empty one, a database
    whose rows are no multiple of the tile's own columns --, windows 1 / 5 / 19 / 64 x hops 1 / 2 / 3 x n 1 / 3 / 64"""
    db, pos, q, rstart, rlen = _grid_world(D)
    lens = np.diff(pos)
    assert lens.max() == 300 > 128 and 0 < lens[lens > 0].min() < 5 and (lens == 0).any() and 11 in rlen and 0 in rlen and len(rlen) >= 3
    assert int(pos[-1]) % (128 - (window - 1)) != 0
    mx.assert_exact_domain(window, D)
    idx = _index("grid", db, pos)
    for hop in HOPS:
        want = sc.stats_oracle(q, db, pos, window, hop, rstart, rlen, key="grid")
        for n in (1, 3, 64):
            top, n_found, block, stats, wfirst = _both_parents(torch_cuda, idx, q, rstart, rlen, window, hop, n, block=n == 3)
            assert np.array_equal(wfirst, mc.wfirst_of(rlen, window, hop)) and stats.shape[0] == len(want) > 0
            bad = sc.differing(stats, want)
            assert not bad, "window %d hop %d n %d: %d of %d windows differ\n%s" % (window, hop, n, len(bad), len(want), "\n".join(bad[:6]))
    assert any(w["sum_q"] != 0 for w in want) and any(w["sumsq_q"] != 0 for w in want)


@pytest.mark.parametrize("window", [5, 19])
def test_packed_world(torch_cuda, window):
    """more than 128 one-row songs in one tile with empty songs between them, then two songs longer than a tile: up to `window`
    pieces on one stretch and none of them full until the long songs; and the one-row songs alone: no full piece at all"""
    db, pos, q, rstart, rlen = dt.packed_world(D)
    assert (np.diff(pos) == 1).sum() == 200 and (np.diff(pos) == 0).sum() > 5 and (np.diff(pos) == 300).sum() == 2
    mx.assert_exact_domain(window, D)
    idx = _index("packed", db, pos)
    for hop in (1, 3):
        want = sc.stats_oracle(q, db, pos, window, hop, rstart, rlen, key="packed")
        *_, stats, _ = _both_parents(torch_cuda, idx, q, rstart, rlen, window, hop, 64)
        bad = sc.differing(stats, want)
        assert not bad, "window %d hop %d: %d of %d windows differ\n%s" % (window, hop, len(bad), len(want), "\n".join(bad[:6]))
        assert (stats["n_full"] == 2 * (300 - window + 1)).all()
    cut = int(np.flatnonzero(np.diff(pos) == 300)[0])    # the one-row songs alone: every song is shorter than the window
    short = _index("packed-short", db[:pos[cut]], pos[:cut + 1])
    top, n_found, _, stats, _ = _both_parents(torch_cuda, short, q, rstart, rlen, window, 1, 3)
    assert len(stats) > 0 and not stats.view(np.int64).any() and (n_found == 200).all() and (top["song"] >= 0).all()


@pytest.mark.parametrize("d", [64, 256])
def test_other_row_widths(torch_cuda, d):
    db, pos, q, rstart, rlen = _grid_world(d, seed=340)
    mx.assert_exact_domain(19, d)
    for hop in (1, 3):
        want = sc.stats_oracle(q, db, pos, 19, hop, rstart, rlen, key=("grid-d", d))
        *_, stats, _ = _both_parents(torch_cuda, _index(("grid-d", d), db, pos), q, rstart, rlen, 19, hop, 3)
        bad = sc.differing(stats, want)
        assert not bad, "d %d hop %d: %d of %d windows differ\n%s" % (d, hop, len(bad), len(want), "\n".join(bad[:6]))


def test_excluded_song(torch_cuda):
    """dense_cases.small_world, one excluded song per recording: the statistics omit exactly that song's full pieces"""
    db, pos, q, rstart, rlen = dc.small_world()
    lens = np.diff(pos)
    order = np.argsort(-lens, kind="stable")
    excl = [int(order[0]), -1, int(order[1])]
    idx = _index("small", db, pos)
    for window, hop in ((5, 1), (19, 2)):
        mx.assert_exact_domain(window, db.shape[1])
        top, _, _, stats, wfirst = _both_parents(torch_cuda, idx, q, rstart, rlen, window, hop, 3, exclude_song=excl)
        want = sc.stats_oracle(q, db, pos, window, hop, rstart, rlen, excl=excl)
        bad = sc.differing(stats, want)
        assert not bad, "window %d hop %d: %d windows differ\n%s" % (window, hop, len(bad), "\n".join(bad[:6]))
        none = _one_pass(torch_cuda, idx, q, rstart, rlen, window, hop, 3)[3]
        for r, ex in enumerate(excl):
            a, b = int(wfirst[r]), int(wfirst[r + 1])
            gone = max(int(lens[ex]) - min(window, rlen[r]) + 1, 0) if ex >= 0 else 0
            assert b > a and (none["n_full"][a:b] - stats["n_full"][a:b] == gone).all(), (window, r)
            assert ex < 0 or (gone > 0 and (top["song"][a:b] != ex).all())


# ------------------------------------------------------------------------------------------------ chunking, the byte contract
def test_chunking_and_the_byte_contract(torch_cuda, monkeypatch):
    """real-valued rows, 300 of them: three row-tile slots at window 19.  PFANN_DENSE_TOPN_WINDOWS = 1 walks one slot per chunk
    (three chunks and more: a memset per chunk, or a window index local to the chunk, would change the statistics), 7 rounds up
    to the same; a window's 24 stats bytes are the same alone, behind another recording of 137 rows, and reached by hop 3"""
    db, pos, q, _ = mc.unit_case(11, 40, D, 10, 300)
    window, L, other, n = 19, q.shape[0], 137, 4
    assert L == 300 and (L - window + 1) // (128 - (window - 1)) + 1 >= 3
    idx = _index("unit300", db, pos)
    monkeypatch.delenv("PFANN_DENSE_TOPN_WINDOWS", raising=False)
    base = _both_parents(torch_cuda, idx, q, [0], [L], window, 1, n)[:4]
    q2 = np.concatenate([q[:other][::-1], q])
    names = ("top", "n_found", "block", "stats")

    def same(got, step, what, first=0):
        for a, b, name in zip(base, got, names):
            assert np.ascontiguousarray(a[::step]).tobytes() == np.ascontiguousarray(b[first:]).tobytes(), "%s: other %s bytes" % (what, name)

    same(_one_pass(torch_cuda, idx, q, [0], [L], window, 1, n), 1, "twice in a row")
    same(_both_parents(torch_cuda, idx, q, [0], [L], window, 3, n)[:4], 3, "hop 3")
    *got, wf = _both_parents(torch_cuda, idx, q2, [0, other], [other, L], window, 1, n)
    same(got, 1, "behind another recording", int(wf[1]))
    *got, wf = _both_parents(torch_cuda, idx, q2, [0, other], [other, L], window, 3, n)
    same(got, 3, "hop 3 behind another recording", int(wf[1]))
    for cap in ("1", "7"):
        monkeypatch.setenv("PFANN_DENSE_TOPN_WINDOWS", cap)
        same(_one_pass(torch_cuda, idx, q, [0], [L], window, 1, n), 1, "PFANN_DENSE_TOPN_WINDOWS=" + cap)
        same(_one_pass(torch_cuda, idx, q, [0], [L], window, 3, n), 3, "hop 3, PFANN_DENSE_TOPN_WINDOWS=" + cap)
        (t, f, s, st), wf = idx.match_windows_dense_topn_stats(torch_cuda.as_tensor(q2).cuda(), [0, other], [other, L], window, 1, n,
                                                               want_song_scores=True)
        same((t, f, s, st), 1, "behind another recording, PFANN_DENSE_TOPN_WINDOWS=" + cap, int(wf[1]))
    monkeypatch.delenv("PFANN_DENSE_TOPN_WINDOWS")
    same(_one_pass(torch_cuda, idx, q, [0], [L], window, 1, n), 1, "the default chunk size again")
    stats = base[3]
    assert stats.dtype.itemsize == 24 and len({int(x) for x in stats["sum_q"]}) > len(stats) // 2, "the sums are not real-valued"


# ------------------------------------------------------------------------------------------------ updates
def test_after_an_update_the_call_answers_as_a_fresh_handle(torch_cuda):
    from pfann_amd.database import DeviceIndex
    db, pos, q, rstart, rlen = dc.small_world()
    lens = np.diff(pos)
    idx = DeviceIndex(D, 0)
    idx.load(db, pos)
    _one_pass(torch_cuda, idx, q, rstart, rlen, 19, 2, 5)                 # (sizes the workspace for the old number of songs)
    extra = mx.grid_rows(91, "topn/append", 37, D)
    idx.append(extra, [37])
    gone = int(np.flatnonzero(lens > 20)[0])
    idx.remove_songs([gone])
    keep = np.ones(db.shape[0], bool)
    keep[pos[gone]:pos[gone + 1]] = False
    new_lens = np.concatenate([lens, [37]])
    new_lens[gone] = 0
    new_pos = np.pad(np.cumsum(new_lens), (1, 0)).astype(np.int64)
    new_db = np.concatenate([db[keep], extra])
    fresh = DeviceIndex(D, 0)
    fresh.load(new_db, new_pos)
    got = _both_parents(torch_cuda, idx, q, rstart, rlen, 19, 2, 5)
    ref = _one_pass(torch_cuda, fresh, q, rstart, rlen, 19, 2, 5)
    for x, y, name in zip(got[:4], ref, ("top", "n_found", "block", "stats")):
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), "%s differs from a fresh handle's" % name
    assert not sc.differing(got[3], sc.stats_oracle(q, new_db, new_pos, 19, 2, rstart, rlen))
    assert not dt.differing(*got[:3], dt.dense_topn_oracle(q, new_db, new_pos, 19, 2, rstart, rlen, 5))


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_every_output_untouched(torch_cuda):
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
    q = torch.as_tensor(db[:30]).cuda()
    rs = torch.zeros(1, dtype=torch.int64).cuda()
    rl = torch.full((1,), 30, dtype=torch.int32).cuda()
    n_songs = len(pos) - 1

    def call(idx, window, hop, n, null_stats=False, parent=False):
        nW = int(mc.wfirst_of([30], min(max(window, 1), 64), max(hop, 1))[-1])
        wf = torch.as_tensor(np.asarray([0, nW], np.int64)).cuda()
        outs = [torch.full((max(nW, 1) * size,), 0xA5, dtype=torch.uint8).cuda()
                for size in (max(n, 64) * ctypes.sizeof(L.MatchResult), 4, n_songs * 8, 24)]
        args = [idx.handle, q.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, window, hop, wf.data_ptr(), nW, None, n,
                outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr()]
        if parent:
            rc = lib.pfann_match_windows_dense_topn(*args, None)
        else:
            rc = lib.pfann_match_windows_dense_topn_stats(*args, None if null_stats else outs[3].data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, [bool((o.cpu() == 0xA5).all()) for o in outs]

    rc, _, untouched = call(whole, 5, 1, 3)               # the control: the same call on a good handle writes all four
    assert rc == 0 and not any(untouched)
    rc, msg, untouched = call(whole, 5, 1, 3, null_stats=True)
    assert rc == -1 and "stats_dev" in msg and all(untouched), (rc, msg, untouched)
    tail = lambda m: m.split(": ", 1)[1]
    for idx, window, hop, n, word in ((whole, 5, 1, 0, "n="), (whole, 5, 1, 65, "n="), (whole, 65, 1, 3, "window"), (whole, 0, 1, 3, "window"),
                                      (whole, 5, 0, 3, "hop"), (half, 5, 1, 3, "fp16"), (shard, 5, 1, 3, "shard"),
                                      (shard, 5, 1, 65, "n=65"), (half, 65, 1, 3, "fp16")):      # two at once: the parent's first one
        rc, msg, untouched = call(idx, window, hop, n)
        assert rc == -1 and msg and word in msg and all(untouched), (window, hop, n, word, rc, msg, untouched)
        prc, pmsg, _ = call(idx, window, hop, n, parent=True)
        assert prc == -1 and (msg == pmsg or tail(msg) == tail(pmsg)), "pfann_match_windows_dense_topn refuses with %r, the one-pass call with %r" % (pmsg, msg)
    with pytest.raises(L.PfannError, match="shard"):
        shard.match_windows_dense_topn_stats(q, [0], [30], 5, 1, 3)
    with pytest.raises(L.PfannError, match="n=65"):
        whole.match_windows_dense_topn_stats(q, [0], [30], 5, 1, 65)


# ------------------------------------------------------------------------------------------------ the Database layer
def test_database_query_dense_stats(torch_cuda, tmp_path, monkeypatch):
    """queries of 1, 2, 19, 33 and 64 rows in one call: (answers, ranked) are query_dense_batch's, entry 0's log10_fa is
    significance.log10_false_alarm fed from match_windows_dense_stats of the query alone, the values obey the prefix rule, and
    stats=False launches what it always launched"""
    from pfann_amd import database as dbm
    from pfann_amd import lib as L
    from pfann_amd import significance as sg
    from pfann_amd.utils import read_config
    torch = torch_cuda
    emb, pos = dc.selfmatch_world(str(tmp_path))
    cfg = read_config(os.path.join(str(tmp_path), "configs.json"))
    db = dbm.Database(str(tmp_path), cfg["indexer"], cfg["hop_size"], d=D)
    lens = np.diff(pos)
    qlen = [1, 2, 19, 33, 64]
    qstart = np.concatenate([[0], np.cumsum(qlen)[:-1]])
    rows = np.concatenate([emb[pos[2] + 3:pos[2] + 3 + 22], emb[pos[4]:pos[4] + 33], emb[pos[8]:pos[8] + 40], emb[pos[10]:pos[10] + 24]])
    assert rows.shape[0] == sum(qlen)
    rec = torch.as_tensor(rows).cuda()
    answers, ranked, fa = db.query_dense_stats_batch(rec, qstart, qlen, n=3, want_song_scores=True)
    answers0, ranked0 = db.query_dense_batch(rec, qstart, qlen, n=3, want_song_scores=True)
    assert ranked == ranked0 and [a[:2] for a in answers] == [a[:2] for a in answers0]
    assert all(a[2].tobytes() == b[2].tobytes() for a, b in zip(answers, answers0))
    fa8 = db.query_dense_stats_batch(rec, qstart, qlen, n=8)[2]
    hists = sg.OverlapHistograms(lens)
    for j, (s, m) in enumerate(zip(qstart, qlen)):
        assert fa[j].dtype == np.float64 and fa[j].shape == (len(ranked[j]),) == (3,) and (fa[j] <= 0.0).all()
        assert np.array_equal(fa8[j][:3], fa[j]), "query %d: a value depends on the length of the list" % j
        (res, stats), _ = db.index.match_windows_dense_stats(rec[s:s + m], [0], [m], m, 1)
        want = sg.log10_false_alarm(res["score"][0], m, res["song"][0], res["offset"][0],
                                    (stats["n_full"][0], stats["sum_q"][0], stats["sumsq_q"][0]), hists(m), lens)
        assert fa[j][0] == want, (j, fa[j][0], want)
    # song 2 is stored twice (song 7): a query from inside it names both copies, both far below any threshold; the third is noise
    assert {ranked[2][0][1][0], ranked[2][1][1][0]} == {2, 7} and fa[2][0] < -6.0 and fa[2][1] < -6.0 and fa[2][2] > -3.0, (ranked[2], fa[2])
    # stats=False: the launch of the parent commit, call for call and byte for byte
    calls = []
    for name in ("match_windows_dense_topn", "match_windows_dense_topn_stats"):
        real = getattr(db.index, name)
        monkeypatch.setattr(db.index, name, lambda *a, _real=real, _name=name, **k: (calls.append(_name), _real(*a, **k))[1])
    p = db.query_dense_launch(rec, qstart, qlen, 3, True)
    assert calls == ["match_windows_dense_topn"] and "stats" not in p and "rows_of" not in p
    p1 = db.query_dense_launch(rec, qstart, qlen, 3, True, stats=True)
    assert calls == ["match_windows_dense_topn", "match_windows_dense_topn_stats"] and p1["stats"].shape == (5, 3)
    torch.cuda.synchronize()
    for k in ("res", "n_found", "ss"):
        assert p[k].cpu().numpy().tobytes() == p1[k].cpu().numpy().tobytes(), k
    assert db.query_dense_finish(p)[1] == ranked0
    monkeypatch.setattr(db, "ranks", object())
    with pytest.raises(L.PfannError, match="not song-sharded"):
        db.query_dense_launch(rec, qstart, qlen, 3, stats=True)


# ------------------------------------------------------------------------------------------------ matcher.py --dense --max-fa
MAX_FA = "3.54e-2"                                      # log10: -1.451, see the docstring of test_matcher_cli_max_fa


def _rows(path):
    with open(path, encoding="utf8", newline="") as f:
        return list(csv.reader(f))


def matcher_scenario(root, run, torch):
    """the synthetic songs of test_gpu_dense_topn.py::test_matcher_cli_dense_end_to_end's generator (12 songs of 20 s, 12
    ten-second queries cut from them at SNR 0) with a 13th song that carries seconds 2..14 of song 3 at its own seconds 4..16,
    and three more queries: seconds 3..13 of song 3 at SNR 0 (planted twice), two of noise alone; then an unreadable file.
    The default configuration with the calibrated seeded weights, as dense_cases.four_excerpts: under the tiny configuration
    (d 16) the float64 oracle does not even name the right song for most of these queries, with either set of weights, so
    nothing separates there.  Writes the model directory, the songs and the lists under root
    -> (model dir, music list, query list, names)"""
    from pfann_amd import synth
    params = json.load(open(os.path.join(REPO, "configs", "default.json")))
    sd = synth.make_state_dict_calibrated(params, seed=123)
    mdir = os.path.join(root, "model")
    os.makedirs(mdir)
    torch.save({n: torch.from_numpy(v) for n, v in sd.items()}, os.path.join(mdir, "model.pt"))
    shutil.copy(os.path.join(REPO, "configs", "default.json"), os.path.join(mdir, "configs.json"))
    data = os.path.join(root, "data")
    run(os.path.join(REPO, "tools", "gen_synth_dataset.py"), data, "--songs", "12", "--queries", "12", "--seconds", "10",
        "--song-seconds", "20", "--snr", "0")
    sr = 8000
    song3 = synth.make_song(3, 20.0)
    twin = synth.make_song(40, 20.0)
    twin[4 * sr:16 * sr] = song3[2 * sr:14 * sr]
    twin_path = os.path.join(data, "music", "song00012.wav")
    synth.write_wav(twin_path, twin)
    music = os.path.join(data, "music.txt")
    open(music, "a").write(twin_path + "\n")
    qdir = os.path.join(data, "query_snr0")
    qlist = os.path.join(qdir, "list.txt")
    names = {"planted": [ln.rstrip("\n") for ln in open(qlist)]}
    double = os.path.join(qdir, "double.wav")
    synth.write_wav(double, synth.make_query(song3[3 * sr:13 * sr], 700, 10.0, 0.0)[0])
    names["double"], names["noise"] = double, []
    for j in range(2):
        p = os.path.join(qdir, "noise%d.wav" % j)
        nz = synth.normal(4242 + j, "fa/noise", 10 * sr).astype(np.float64)
        synth.write_wav(p, np.round(nz / np.abs(nz).max() * 30000.0).astype(np.int16))
        names["noise"].append(p)
    names["missing"] = os.path.join(data, "nope.wav")
    open(qlist, "a").write("".join(p + "\n" for p in [double] + names["noise"] + [names["missing"]]))
    names["twin_song"], names["song3"] = twin_path, os.path.join(data, "music", "song00003.wav")
    return mdir, music, qlist, names


def test_matcher_cli_max_fa(torch_cuda, tmp_path):
    """matcher_scenario, builder.py once, then matcher.py --dense --top 3 without and with --max-fa X, --dense --no-bin --max-fa=X,
    and --top 3 --max-fa X without --dense (status 2).
    X from the float64 oracle on the CPU (the oracle's encoder on the same files and weights, totals rounded to float32, every
    query one window of its 19 rows, log10_false_alarms_ranked on the oracle's ranked list): rank 1 of the 12 planted queries has
    log10_fa -7.57 .. -2.32, the doubly planted query -4.69 at rank 1 and -5.44 at rank 2 (the query of song 3 overlaps the
    planted stretch too: -2.67 and -3.02), and of the six entries of the two noise queries the most significant has -0.58; the
    ranks below a true match have -0.43 .. 0.  The classes are 1.74 decades apart; X = 10^-1.451 lies halfway in log10.
    Asserted: the four existing files byte for byte, the header and the row counts of _fa.csv, its first five columns equal to
    _top.csv's, detected == (log10_fa <= log10 X), every planted query detected at rank 1 with its song, the doubly planted one
    at ranks 1 and 2 with both songs, no detected row for a noise query, the error row.
    Wall time on an MI355X: 26 s (builder.py and four matcher.py processes on the default configuration;
    test_gpu_dense_topn.py::test_matcher_cli_dense_end_to_end, five processes on the tiny one, takes 19 s beside it)."""
    env = dict(os.environ, PYTHONPATH=REPO)

    def run(*cmd, rc=0):
        r = subprocess.run(["timeout", "-k", "10", "400", sys.executable] + list(cmd), capture_output=True, text=True, env=env,
                           cwd=str(tmp_path), timeout=460)
        assert r.returncode == rc, r.stdout[-3000:] + r.stderr[-3000:]
        return r

    mdir, music, qlist, names = matcher_scenario(str(tmp_path), run, torch_cuda)
    dbdir = str(tmp_path / "db")
    run(os.path.join(REPO, "builder.py"), music, dbdir, mdir)
    out = {k: str(tmp_path / (k + ".txt")) for k in ("plain", "fa", "one")}
    run(os.path.join(REPO, "matcher.py"), qlist, dbdir, out["plain"], "--dense", "--top", "3")
    run(os.path.join(REPO, "matcher.py"), qlist, dbdir, out["fa"], "--dense", "--top", "3", "--max-fa", MAX_FA)
    run(os.path.join(REPO, "matcher.py"), qlist, dbdir, out["one"], "--dense", "--no-bin", "--max-fa=" + MAX_FA)
    r = run(os.path.join(REPO, "matcher.py"), qlist, dbdir, str(tmp_path / "refused.txt"), "--top", "3", "--max-fa", MAX_FA, rc=2)
    assert "--dense" in r.stderr and len(r.stderr.strip().splitlines()) == 1 and not os.path.exists(str(tmp_path / "refused.txt"))
    stem = lambda p: os.path.splitext(p)[0]
    for suffix in (".txt", "_detail.csv", ".txt.bin", "_top.csv"):       # the four existing files: byte for byte
        a, b = (open(stem(out[k]) + suffix, "rb").read() for k in ("plain", "fa"))
        assert a == b and len(a) > 0, "%s changed under --max-fa" % suffix
    assert not os.path.exists(stem(out["plain"]) + "_fa.csv") and not os.path.exists(out["one"] + ".bin")
    fa = _rows(stem(out["fa"]) + "_fa.csv")
    top = _rows(stem(out["fa"]) + "_top.csv")
    assert fa[0] == ["query", "rank", "answer", "score", "time", "log10_fa", "detected"]
    assert [r[:5] for r in fa[1:]] == top[1:], "the first five columns are _top.csv's"
    log10_x = math.log10(float(MAX_FA))
    per = {}
    for r in fa[1:]:
        assert len(r) == 7 and float(r[5]) <= 0.0 and int(r[6]) == int(float(r[5]) <= log10_x), r
        per.setdefault(r[0], []).append(r)
    queries = names["planted"] + [names["double"]] + names["noise"] + [names["missing"]]
    assert list(per) == queries
    assert per[names["missing"]] == [[names["missing"], "1", "error", "-inf", "0", "0.0", "0"]]
    expected = {r[0]: r[1] for r in _rows(os.path.join(os.path.dirname(qlist), "expected.csv"))[1:]}
    print("log10_fa of the planted queries, rank 1: " + " ".join("%.2f" % float(per[p][0][5]) for p in names["planted"]))
    print("log10_fa of the doubly planted query: " + " ".join("%.2f" % float(r[5]) for r in per[names["double"]]))
    print("log10_fa of the noise queries: " + " / ".join(" ".join("%.2f" % float(r[5]) for r in per[p]) for p in names["noise"]))
    for p in names["planted"]:
        # (song 3's own query overlaps the stretch that is stored twice: there both copies tie, and either may lead)
        ok = {expected[p]} | ({names["twin_song"]} if expected[p] == names["song3"] else set())
        assert [r[1] for r in per[p]] == ["1", "2", "3"] and per[p][0][2] in ok and per[p][0][6] == "1", per[p]
    d = per[names["double"]]
    assert {d[0][2], d[1][2]} == {names["song3"], names["twin_song"]} and d[0][6] == d[1][6] == "1", d
    for p in names["noise"]:
        assert len(per[p]) == 3 and all(r[6] == "0" for r in per[p]), per[p]
    # without --top: one row per query, the values of rank 1
    one = _rows(stem(out["one"]) + "_fa.csv")
    assert one[0] == fa[0] and [r for r in one[1:]] == [r for r in fa[1:] if r[1] == "1"]
    assert not os.path.exists(stem(out["one"]) + "_top.csv")
    assert open(out["one"], "rb").read() == open(out["plain"], "rb").read()
