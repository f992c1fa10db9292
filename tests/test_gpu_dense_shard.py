"""The song-sharded dense matcher on the GPU, one process: several DeviceIndex shard handles beside a whole one
(pfann_match_windows_dense_part / _merge / _topn_part / _topn_merge, csrc/dense.hip).  For every cut of the song list the
merged results, statistics, ranked lists and n_found are the BYTES the existing whole-handle calls write, and == the oracles,
whatever the order of the parts; on the exact grid and on real-valued rows; with exclusions; and every refusal writes nothing."""
import ctypes

import numpy as np
import pytest

import dense_cases as dc
import dense_shard_cases as sh
import dense_stats_cases as ds
import dense_topn_cases as dt
import match_exact as mx
import monitor_cases as mc

pytestmark = pytest.mark.gpu
D = 128
N_TOP = (1, 5, 64)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


_HANDLES, _WHOLE = {}, {}


def _whole_index(key, db, pos, storage="f32"):
    from pfann_amd.database import DeviceIndex
    if (key, storage) not in _HANDLES:
        idx = DeviceIndex(db.shape[1], 0, storage)
        idx.load(db, pos)
        _HANDLES[(key, storage)] = idx
    return _HANDLES[(key, storage)]


def _shards(key, db, pos, cut, storage="f32"):
    """one handle per (song_lo, song_hi) of the cut: its own rows only, the global song_pos, the cut stated to the library"""
    from pfann_amd.database import DeviceIndex
    k = (key, tuple(cut), storage)
    if k not in _HANDLES:
        out = []
        for lo, hi in cut:
            ix = DeviceIndex(db.shape[1], 0, storage)
            ix.load(np.ascontiguousarray(db[pos[lo]:pos[hi]]), pos, int(pos[lo]), song_range=(lo, hi))
            assert ix.owned_songs() == (lo, hi)
            out.append(ix)
        _HANDLES[k] = out
    return _HANDLES[k]


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _whole_answers(torch, key, idx, q, rstart, rlen, window, hop, excl=None):
    """the existing whole-handle calls, once per (world, window, hop, exclusion): bytes of the results, the statistics and the
    ranked lists / n_found for every n of N_TOP"""
    k = (key, window, hop, None if excl is None else tuple(excl))
    if k not in _WHOLE:
        (res, st), wfirst = idx.match_windows_dense_stats(q, rstart, rlen, window, hop, exclude_song=excl, to_host=False)
        plain, _ = idx.match_windows_dense(q, rstart, rlen, window, hop, exclude_song=excl, to_host=False)
        assert _bytes(plain) == _bytes(res)
        ranked = {}
        for n in N_TOP:
            (top, nf, _), _ = idx.match_windows_dense_topn(q, rstart, rlen, window, hop, n, exclude_song=excl, to_host=False)
            ranked[n] = (_bytes(top), _bytes(nf))
        _WHOLE[k] = (_bytes(res), _bytes(st), ranked, wfirst)
    return _WHOLE[k]


def _sharded_answers(torch, merger, shards, q, rstart, rlen, window, hop, excl=None, n_top=N_TOP):
    """part on every handle, merge on `merger` -> (results, statistics, {n: (top, n_found)}) device tensors, wfirst"""
    parts = [ix.match_windows_dense_part(q, rstart, rlen, window, hop, exclude_song=excl, stats=True) for ix in shards]
    wfirst = parts[0][1]
    words, stats = torch.stack([p[0][0] for p in parts]), torch.stack([p[0][1] for p in parts])
    res, st = merger.dense_merge(words, stats, rlen, window, hop, exclude_song=excl)
    bare = [ix.match_windows_dense_part(q, rstart, rlen, window, hop, exclude_song=excl)[0] for ix in shards]
    assert all(b[1] is None for b in bare) and _bytes(torch.stack([b[0] for b in bare])) == _bytes(words), "words with and without stats"
    res2, none = merger.dense_merge(words, None, rlen, window, hop, exclude_song=excl)
    assert none is None and _bytes(res2) == _bytes(res)
    ranked = {}
    for n in n_top:
        lists = [ix.match_windows_dense_topn_part(q, rstart, rlen, window, hop, n, exclude_song=excl)[0] for ix in shards]
        ranked[n] = merger.dense_topn_merge(torch.stack([t for t, _ in lists]), torch.stack([f for _, f in lists]))
    return res, st, ranked, wfirst


def _assert_same_bytes(got, want, what):
    res, st, ranked, wfirst = got
    assert np.array_equal(wfirst, want[3]) and int(wfirst[-1]) > 0, what
    assert _bytes(res) == want[0], "%s: merged results differ from the whole handle's bytes" % what
    assert _bytes(st) == want[1], "%s: merged statistics differ from the whole handle's bytes" % what
    for n, (top, nf) in ranked.items():
        assert _bytes(top) == want[2][n][0], "%s n %d: merged ranked lists differ from the whole handle's bytes" % (what, n)
        assert _bytes(nf) == want[2][n][1], "%s n %d: merged n_found differs from the whole handle's" % (what, n)


def _grid_world():
    world = mx.std_world(41, D, long_rows=300)
    db, pos, q, _, rstart, rlen = mc.grid_recordings(D, 20, world=world)
    return db, pos, q, rstart, rlen


# ------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("window", [1, 19, 64])
def test_every_cut_gives_the_whole_handles_bytes_and_the_oracles(torch_cuda, window):
    """the grid world of tests/test_gpu_dense.py (300-row songs longer than a tile, songs shorter than the window, exact ties, an
    11-row recording, an empty one); hops 1 / 7; shard_songs for 2 / 3 / 8 ranks, a cut after the first song with rows, and -- on
    the world with a rowless song appended -- that song alone on the second shard and no song at all on it."""
    from pfann_amd.database import DeviceIndex
    from pfann_amd.significance import STATS_DTYPE
    torch = torch_cuda
    db, pos, q, rstart, rlen = _grid_world()
    lens = np.diff(pos)
    assert lens.max() == 300 > 128 and 0 < lens[lens > 0].min() < 5 and 11 in rlen and 0 in rlen
    mx.assert_exact_domain(window, D)
    pos_x, more = sh.with_rowless_tail(pos)
    cases = [(name, cut, pos, "grid") for name, cut in sh.cuts_of(pos).items()] + [(name, cut, pos_x, "grid-x") for name, cut in more.items()]
    SI = 128 - (window - 1)
    assert any(int(pos[lo]) % SI != 0 for _, cut, p, _ in cases for lo, _ in cut[1:]), "no cut falls inside a tile of the whole handle"
    lo, hi = sh.cuts_of(pos)["first"][0]
    assert window == 1 or 0 < pos[hi] - pos[lo] < window - 1, "the first shard holds fewer rows than window - 1"
    assert all(p[hi] == p[lo] for _, cut, p, key in cases if key == "grid-x" for lo, hi in cut[1:])
    qt = torch.as_tensor(q).cuda()
    for hop in (1, 7):
        for name, cut, p, key in cases:
            what = "window %d hop %d cut %s" % (window, hop, name)
            whole = _whole_index(key, db, p)
            want = _whole_answers(torch, key, whole, qt, rstart, rlen, window, hop)
            shards = _shards(key, db, p, cut)
            got = _sharded_answers(torch, whole, shards, qt, rstart, rlen, window, hop)
            _assert_same_bytes(got, want, what)
            # the parts in reversed order, merged on a shard handle: the same bytes
            back = _sharded_answers(torch, shards[-1], shards[::-1], qt, rstart, rlen, window, hop, n_top=(5,))
            _assert_same_bytes(back, want, what + " reversed")
            # ... and they are the oracles' answers, ==
            res = DeviceIndex.decode_results(got[0])
            bad = mc.differing(res, dc.dense_oracle(q, db, p, window, hop, rstart, rlen, key=key))
            bad += ds.differing(DeviceIndex.stats_to_host(got[1]), ds.stats_oracle(q, db, p, window, hop, rstart, rlen, key=key))
            for n, (top, nf) in got[2].items():
                bad += dt.differing(DeviceIndex.decode_results(top), nf.cpu().numpy(), None,
                                    dt.dense_topn_oracle(q, db, p, window, hop, rstart, rlen, n, key=key))
            assert not bad, "%s: %d differences from the oracles\n%s" % (what, len(bad), "\n".join(bad[:6]))
    assert STATS_DTYPE.itemsize == 24


def test_a_part_holds_its_own_songs_only(torch_cuda):
    """the raw outputs of one part: the word decodes to a candidate of an owned song (or is 0), the statistics and the ranked
    list are those of tests/dense_shard_cases.py for that shard, and a shard without rows leaves zeros and padding"""
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    db, pos, q, rstart, rlen = _grid_world()
    pos_x, more = sh.with_rowless_tail(pos)
    window, hop, n = 19, 7, 5
    qt = torch.as_tensor(q).cuda()
    G = q.astype(np.float64) @ db.astype(np.float64).T
    sg = np.searchsorted(pos_x[:-1], np.arange(int(pos_x[-1])), side="right") - 1
    for cut in (sh.cuts_of(pos_x)["3"], more["rowless-right"], more["rowless-left"]):
        for ix, (lo, hi) in zip(_shards("grid-x", db, pos_x, cut), cut):
            (words, st), _ = ix.match_windows_dense_part(qt, rstart, rlen, window, hop, stats=True)
            (top, nf), _ = ix.match_windows_dense_topn_part(qt, rstart, rlen, window, hop, n)
            words, st = words.cpu().numpy().view(np.uint64), st.cpu().numpy()
            top, nf = DeviceIndex.decode_results(top), nf.cpu().numpy()
            for j, (r0, m, ex) in enumerate(sh._windows(rstart, rlen, window, hop, None)):
                want = sh.part_of_window(G, pos_x, sg, r0, m, ex, lo, hi)
                if want["word"] is None:
                    assert int(words[j]) == 0 and pos_x[hi] == pos_x[lo]
                else:
                    tot, b = want["word"]
                    assert 0xFFFFFFFF - (int(words[j]) & 0xFFFFFFFF) == b, (j, lo, hi)
                    hi32 = np.uint32(int(words[j]) >> 32)
                    bits = np.uint32(hi32 & np.uint32(0x7FFFFFFF)) if hi32 & np.uint32(0x80000000) else np.uint32(~hi32)
                    assert float(bits.view(np.float32)) == tot, (j, lo, hi)
                assert tuple(int(x) for x in st[j]) == want["stats"], (j, lo, hi)
                got = [tuple(e[f].item() for f in dt.FIELDS) for e in top[j]]
                assert got == want["heads"][:n] + [dt.PAD] * max(0, n - len(want["heads"])) and int(nf[j]) == len(want["heads"]), (j, lo, hi)


@pytest.mark.parametrize("d", [64, 256])
def test_other_row_widths(torch_cuda, d):
    torch = torch_cuda
    world = mx.std_world(41, d, long_rows=300)
    db, pos, q, _, rstart, rlen = mc.grid_recordings(d, 20, world=world, seed=340)
    key = ("grid-d", d)
    whole = _whole_index(key, db, pos)
    qt = torch.as_tensor(q).cuda()
    want = _whole_answers(torch, key, whole, qt, rstart, rlen, 19, 3)
    got = _sharded_answers(torch, whole, _shards(key, db, pos, sh.cuts_of(pos)["3"]), qt, rstart, rlen, 19, 3)
    _assert_same_bytes(got, want, "d %d" % d)


# ------------------------------------------------------------------------------------------------ real-valued rows
def test_real_valued_rows(torch_cuda):
    """unit-norm random rows, where no two totals coincide by construction of the inputs: the four outputs are still the whole
    handle's bytes -- the exact grid's coincidences are not what made the test above pass"""
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    db, pos, q, _ = mc.unit_case(7, 120, D, 100, 400)
    rstart, rlen, window, hop = [0], [400], 19, 2
    whole = _whole_index("unit", db, pos)
    qt = torch.as_tensor(q).cuda()
    want = _whole_answers(torch, "unit", whole, qt, rstart, rlen, window, hop)
    cuts = sh.cuts_of(pos)
    for name in ("2", "3", "8"):
        got = _sharded_answers(torch, whole, _shards("unit", db, pos, cuts[name]), qt, rstart, rlen, window, hop)
        _assert_same_bytes(got, want, "unit rows, cut %s" % name)
    scores = np.frombuffer(want[0], dtype=DeviceIndex.RESULT_DTYPE)["score"]
    assert np.unique(scores).shape[0] > scores.shape[0] // 2
    ranked = np.frombuffer(want[2][5][0], dtype=DeviceIndex.RESULT_DTYPE)["score"]
    assert np.unique(ranked).shape[0] > ranked.shape[0] // 2


# ------------------------------------------------------------------------------------------------ exclusion
def test_exclusion_counts_as_on_the_whole_handle(torch_cuda):
    """the excluded song in the winner's shard, in another shard, and a rowless one: n_cand and n_found are the whole handle's"""
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    db, pos, q, rstart, rlen = _grid_world()
    window, hop = 19, 7
    whole = _whole_index("grid", db, pos)
    qt = torch.as_tensor(q).cuda()
    plain = np.frombuffer(_whole_answers(torch, "grid", whole, qt, rstart, rlen, window, hop)[0], dtype=DeviceIndex.RESULT_DTYPE)
    cut = sh.cuts_of(pos)["3"]
    winner = int(plain["song"][0])
    other = next(s for lo, hi in cut if not lo <= winner < hi for s in range(lo, hi) if pos[s + 1] > pos[s])
    rowless = int(np.flatnonzero(np.diff(pos) == 0)[1])
    assert winner >= 0 and pos[rowless + 1] == pos[rowless]
    for ex in (winner, other, rowless):
        excl = [ex, -1, ex, ex, -1]
        want = _whole_answers(torch, "grid", whole, qt, rstart, rlen, window, hop, excl)
        got = _sharded_answers(torch, whole, _shards("grid", db, pos, cut), qt, rstart, rlen, window, hop, excl)
        _assert_same_bytes(got, want, "excluded song %d" % ex)
        res = np.frombuffer(want[0], dtype=DeviceIndex.RESULT_DTYPE)
        assert (res["song"][:int(got[3][1])] != ex).all()
        if ex == winner:
            assert (res["n_cand"][0] < plain["n_cand"][0]) and res["song"][0] != winner
        if ex == rowless:
            assert want[0] == plain.tobytes()


def test_a_whole_handle_as_the_single_part_is_the_existing_call(torch_cuda):
    torch = torch_cuda
    db, pos, q, rstart, rlen = _grid_world()
    whole = _whole_index("grid", db, pos)
    qt = torch.as_tensor(q).cuda()
    for window, hop in ((19, 1), (64, 7)):
        want = _whole_answers(torch, "grid", whole, qt, rstart, rlen, window, hop)
        _assert_same_bytes(_sharded_answers(torch, whole, [whole], qt, rstart, rlen, window, hop), want, "one part")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_write_nothing(torch_cuda):
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    torch = torch_cuda
    lib = L.load()
    db, pos = mx.std_world(41, D)
    lo, hi = 10, 30
    shard = DeviceIndex(D, 0)
    shard.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    half = DeviceIndex(D, 0, "f16")
    half.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
    odd = DeviceIndex(6, 0)                                  # d % 4 != 0
    odd.load(np.ones((8, 6), np.float32), np.array([0, 8], np.int64))
    huge = DeviceIndex(D, 0)                                 # a rowless shard of a database whose ids do not fit 32 bits
    huge.load(np.zeros((0, D), np.float32), np.array([0, 1 << 32], np.int64), 0, song_range=(0, 0))
    q = torch.as_tensor(db[:30]).cuda()
    q6 = torch.ones((30, 6)).cuda()
    rs = torch.zeros(1, dtype=torch.int64).cuda()
    rl = torch.full((1,), 30, dtype=torch.int32).cuda()
    RES = ctypes.sizeof(L.MatchResult)

    def run(call, window, hop, sizes):
        """call(wf, nW, *sentinel-filled buffers) -> (rc, message, every buffer untouched, the buffers).  sizes: bytes per window,
        or (bytes, fill) for an input whose one-part sum must not look like the outputs' sentinel"""
        nW = int(mc.wfirst_of([30], min(max(window, 1), 64), max(hop, 1))[-1])
        wf = torch.as_tensor(np.asarray([0, nW], np.int64)).cuda()
        sizes = [s if isinstance(s, tuple) else (s, 0xA5) for s in sizes]
        bufs = [torch.full((max(nW, 1) * s,), fill, dtype=torch.uint8).cuda() for s, fill in sizes]
        rc = call(wf, nW, *bufs)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, all(bool((b.cpu() == fill).all()) for b, (_, fill) in zip(bufs, sizes)), bufs

    def part(idx, window, hop, null=None, qq=q):
        return run(lambda wf, nW, words, st: lib.pfann_match_windows_dense_part(
            idx.handle, qq.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, window, hop, wf.data_ptr(), nW, None,
            None if null == "words" else words.data_ptr(), st.data_ptr(), None), window, hop, (8, 24))

    def topn_part(idx, window, hop, n=3, null=None, qq=q):
        return run(lambda wf, nW, top, nf: lib.pfann_match_windows_dense_topn_part(
            idx.handle, qq.data_ptr(), rs.data_ptr(), rl.data_ptr(), 1, window, hop, wf.data_ptr(), nW, None, n,
            None if null == "top" else top.data_ptr(), nf.data_ptr(), None), window, hop, (RES * 64, 4))

    def merge(idx, window, n_parts=1, null=None):
        return run(lambda wf, nW, words, pst, res, st: lib.pfann_match_windows_dense_merge(
            idx.handle, None if null == "words" else words.data_ptr(), None if null == "part_stats" else pst.data_ptr(), n_parts,
            rl.data_ptr(), 1, window, wf.data_ptr(), nW, None, None if null == "results" else res.data_ptr(),
            None if null == "stats" else st.data_ptr(), None), window, 1, (8, (24, 0x11), RES, 24))

    def topn_merge(idx, n=3, n_parts=1, null=None):
        return run(lambda wf, nW, tops, nfp, top, nf: lib.pfann_match_windows_dense_topn_merge(
            idx.handle, None if null == "tops" else tops.data_ptr(), None if null == "n_found_parts" else nfp.data_ptr(), n_parts, nW, n,
            None if null == "top" else top.data_ptr(), None if null == "n_found" else nf.data_ptr(), None), 5, 1, (RES * 64, (4, 0x11), RES * 64, 4))

    # the controls: the same calls on the good shard write their outputs
    for rc, _, untouched, _ in (part(shard, 5, 1), topn_part(shard, 5, 1)):
        assert rc == 0 and not untouched
    rc, _, _, (words, pst, res, st) = merge(shard, 5)
    assert rc == 0 and not bool((res.cpu() == 0xA5).all()) and not bool((st.cpu() == 0xA5).all())
    rc, _, _, (tops, nfp, top, nf) = topn_merge(shard)
    assert rc == 0 and not bool((top.cpu()[:3 * RES] == 0xA5).all()) and not bool((nf.cpu() == 0xA5).all())

    refused = [
        (part(half, 5, 1), "fp16"), (topn_part(half, 5, 1), "fp16"),
        (part(shard, 0, 1), "window"), (part(shard, 65, 1), "window"), (topn_part(shard, 0, 1), "window"),
        (topn_part(shard, 65, 1), "window"), (merge(shard, 0), "window"), (merge(shard, 65), "window"),
        (part(shard, 5, 0), "hop"), (topn_part(shard, 5, 0), "hop"),
        (part(odd, 5, 1, qq=q6), "d % 4"), (topn_part(odd, 5, 1, qq=q6), "d % 4"),
        (topn_part(shard, 5, 1, n=0), "n=0"), (topn_part(shard, 5, 1, n=65), "n=65"), (topn_merge(shard, n=0), "n=0"),
        (topn_merge(shard, n=65), "n=65"),
        (merge(shard, 5, n_parts=0), "n_parts"), (topn_merge(shard, n_parts=0), "n_parts"),
        (part(shard, 5, 1, null="words"), "null"), (topn_part(shard, 5, 1, null="top"), "null"),
        (merge(shard, 5, null="words"), "null"), (merge(shard, 5, null="results"), "null"),
        (topn_merge(shard, null="tops"), "null"), (topn_merge(shard, null="top"), "null"),
        (merge(shard, 5, null="part_stats"), "go together"), (merge(shard, 5, null="stats"), "go together"),
        (topn_merge(shard, null="n_found_parts"), "go together"), (topn_merge(shard, null="n_found"), "go together"),
        (part(huge, 5, 1), "32-bit"), (topn_part(huge, 5, 1), "32-bit"), (merge(huge, 5), "32-bit"),
        # two refusals at once: the first one, in the order of the call's checks, is reported
        (part(shard, 65, 1, null="words"), "null"), (part(half, 65, 1), "fp16"), (part(shard, 65, 0), "window=65"),
        (topn_part(shard, 5, 1, n=65, null="top"), "n=65"), (merge(shard, 0, n_parts=0), "n_parts"),
        (part(odd, 65, 1, qq=q6), "d % 4"), (part(huge, 5, 0), "32-bit"), (topn_part(huge, 5, 0), "32-bit"),
    ]
    for i, ((rc, msg, untouched, _), word) in enumerate(refused):
        assert rc == -1 and word in msg and untouched, (i, word, rc, msg, untouched)
    # the existing calls still refuse the shard, with their old message
    old = "the handle holds a shard of the database (monitor mode is not song-sharded)"
    for call in (lambda: shard.match_windows_dense(q, [0], [30], 5, 1), lambda: shard.match_windows_dense_stats(q, [0], [30], 5, 1),
                 lambda: shard.match_windows_dense_topn(q, [0], [30], 5, 1, 3)):
        with pytest.raises(L.PfannError) as e:
            call()
        assert old in str(e.value)
