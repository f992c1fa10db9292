"""The host paths of the windowed matchers (csrc/api.hip windows_call and grow_scratch, DeviceIndex._match_windows and
_dense_call): the seams that only the host code decides and that no other test reaches -- a second step of the general path,
the one routing of the ranked and the unranked call, calls without a window, the order and text of the Python refusals, and
scratch buffers that grow between two calls.  All data is on the exact grid of tests/match_exact.py, so every comparison is
on bytes.

Run as a script (`python tests/test_gpu_windows_host_paths.py routing`) it prints what test_one_routing_on_either_path
compares, as the environment routes the calls: the test starts it in a fresh process with PFANN_WINDOWS_GENERAL=1."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dense_topn_cases as dtc
import match_exact as mx
import monitor_cases as mc

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, K = 64, 100
WINDOWED = ("match_windows", "match_windows_topn")
DENSE = ("match_windows_dense", "match_windows_dense_stats", "match_windows_dense_topn", "match_windows_dense_topn_stats",
         "match_windows_dense_part", "match_windows_dense_topn_part")
FORMS = WINDOWED + DENSE
RANKED = tuple(f for f in FORMS if "topn" in f)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _new_index(db, pos):
    from pfann_amd.database import DeviceIndex
    idx = DeviceIndex(db.shape[1], 0)
    idx.load(db, pos)
    return idx


@pytest.fixture(scope="module")
def long_case(torch_cuda):
    """200 songs of 40 rows, d 64; a recording of 1528 rows and one of 5 rows behind it, k 100 labels per row (the true
    alignment of its piece in one column).  -> (index, db, pos, q, labels on the host, q, labels on the device, rstart, rlen)"""
    db, pos = mx.make_world(61, "hostpaths", [40] * 200, D)
    a = mx.aligned(62, db, pos, [40] * 38 + [8], K)
    b = mx.aligned(63, db, pos, [5], K)
    q, labels = np.concatenate([a.q, b.q]), np.concatenate([a.labels, b.labels])
    assert a.q.shape[0] == 1528 and q.shape[0] == 1533
    return (_new_index(db, pos), db, pos, q, labels, torch_cuda.as_tensor(q).cuda(), torch_cuda.as_tensor(labels).cuda(),
            [0, 1528], [1528, 5])


def _four(res):
    """the bytes of (song, offset, shift, score), field by field: everything but n_cand, which a ranked entry defines as the
    candidates of its song alone (include/pfann_amd.h)"""
    return b"".join(np.ascontiguousarray(res[f]).tobytes() for f in ("song", "offset", "shift", "score"))


def _tags_of(fn):
    """-> (fn(), the profiling tags of the kernels it launched)"""
    from pfann_amd import lib as L
    lib = L.load()
    lib.pfann_prof_enable(1)
    lib.pfann_prof_reset()
    try:
        out = fn()
        buf = ctypes.create_string_buffer(4096)
        lib.pfann_prof_tags(buf, 4096)
    finally:
        lib.pfann_prof_enable(0)
    return out, buf.value.decode().split(",")


# ------------------------------------------------------------------------------------------------ the step loop
def test_the_general_path_takes_a_second_step(long_case):
    """window 128 x k 100 = 12800 > 8192 candidate slots: the call takes the general path by itself, with lists of P = 16384
    slots (the next power of two).  include/pfann_amd.h's slab bound of 256 MB at 12 bytes per slot gives
    (256 << 20) // (16384 * 12) = 1365 windows per step, so the 1402 windows of this call need a second step, whose 37 windows
    -- the short one of the 5-row recording among them -- are written at results + 1365, top + 1365 * n and n_found + 1365.
    Every window is, byte for byte, what `match` / `match_topn` answer for its slice."""
    idx, _, _, _, _, q, labels, rstart, rlen = long_case
    window, hop, per_step = 128, 1, (256 << 20) // (16384 * 12)
    mx.assert_exact_domain(window, D)
    qs, ql = mc.expand(rstart, rlen, window, hop)
    assert per_step == 1365 and len(qs) == 1402 > per_step and ql[-1] == 5 and window * K > mx.MAXC
    (res, wfirst), tags = _tags_of(lambda: idx.match_windows(q, labels, rstart, rlen, window, hop))
    assert "seq_match_windows" not in tags and "seq_match" in tags, tags
    assert wfirst.tolist() == [0, 1401, 1402] and res.shape == (1402,)
    ref, _ = idx.match(q, labels, qs, ql)
    diff = np.flatnonzero(res != ref)
    assert res.tobytes() == ref.tobytes(), "windows %r differ from match on their slices" % diff[:8].tolist()
    assert (res["song"] >= 0).all() and len(set(res["song"][per_step:].tolist())) > 1      # (real answers behind the seam)

    ((top, n_found), wfirst), tags = _tags_of(lambda: idx.match_windows_topn(q, labels, rstart, rlen, window, hop, 3))
    assert "seq_match_windows_topn" not in tags, tags
    rtop, rfound = idx.match_topn(q, labels, qs, ql, 3)
    assert wfirst.tolist() == [0, 1401, 1402] and top.shape == (1402, 3) and n_found.dtype == np.int32
    assert top.tobytes() == rtop.tobytes(), "ranked windows %r differ" % np.flatnonzero((top != rtop).any(1))[:8].tolist()
    assert n_found.tobytes() == rfound.tobytes(), "n_found of windows %r differs" % np.flatnonzero(n_found != rfound)[:8].tolist()
    assert _four(top[:, 0]) == _four(res) and (n_found[per_step:] > 1).any()


# ------------------------------------------------------------------------------------------------ one routing
def _routing(torch):
    """window 19, hop 2, k 20 over the grid recordings of monitor_cases: entry 0 of the ranked call (n = 1, 3) is the unranked
    call's answer byte for byte (n_cand aside, _four).  -> {"tags": the kernels' tags per call, "sha": of the unranked bytes}"""
    d, k, window, hop = 128, 20, 19, 2
    db, pos, q, labels, rstart, rlen = mc.grid_recordings(d, k)
    idx = _new_index(db, pos)
    q, labels = torch.as_tensor(q).cuda(), torch.as_tensor(labels).cuda()
    (res, _), tags = _tags_of(lambda: idx.match_windows(q, labels, rstart, rlen, window, hop))
    out = {"tags": {"0": tags}, "sha": hashlib.sha256(res.tobytes()).hexdigest(), "windows": int(res.shape[0])}
    for n in (1, 3):
        ((top, n_found), _), out["tags"][str(n)] = _tags_of(lambda: idx.match_windows_topn(q, labels, rstart, rlen, window, hop, n))
        assert top.shape == (res.shape[0], n) and _four(top[:, 0]) == _four(res), "n %d: entry 0 differs from match_windows" % n
    return out


def test_one_routing_on_either_path(torch_cuda):
    """the fast path here, the general path in a fresh process under PFANN_WINDOWS_GENERAL=1: on each, both calls took that
    path and entry 0 is the unranked answer; the exact grid makes the two paths' unranked bytes equal as well"""
    assert "PFANN_WINDOWS_GENERAL" not in os.environ
    fast = _routing(torch_cuda)
    assert fast["tags"] == {"0": ["seq_match_windows"], "1": ["seq_match_windows_topn"], "3": ["seq_match_windows_topn"]}, fast["tags"]
    env = dict(os.environ, PYTHONPATH=REPO, PFANN_WINDOWS_GENERAL="1")
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), "routing"], capture_output=True,
                       text=True, env=env, cwd=REPO, timeout=150)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    general = json.loads(r.stdout.strip().splitlines()[-1])
    for n, tags in general["tags"].items():
        assert tags and not any(t.startswith("seq_match_windows") for t in tags), "n %s took %r under PFANN_WINDOWS_GENERAL=1" % (n, tags)
    assert general["windows"] == fast["windows"] > 100 and general["sha"] == fast["sha"]


# ------------------------------------------------------------------------------------------------ the eight Python forms
def _call(idx, form, q, labels, rstart, rlen, window, hop, n=3, exclude_song=None, **kw):
    args = ((q, labels) if form in WINDOWED else (q,)) + (rstart, rlen, window, hop) + ((n,) if form in RANKED else ())
    if form in DENSE:
        kw["exclude_song"] = exclude_song
    return getattr(idx, form)(*args, **kw)


def _flat(x):
    return sum((_flat(y) for y in x), ()) if isinstance(x, tuple) else (x,)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("a call without a window called %s" % name)


@pytest.mark.parametrize("rlen", [[0, 0, 0], []], ids=["empty-recordings", "no-recording"])
@pytest.mark.parametrize("form", FORMS)
def test_a_call_without_a_window_makes_no_library_call(torch_cuda, long_case, form, rlen):
    """recordings of length 0, and no recording: the documented dtypes and shapes on the device, empty arrays on the host"""
    from pfann_amd.database import DeviceIndex
    from pfann_amd.significance import STATS_DTYPE
    idx, _, _, _, _, q, labels, _, _ = long_case
    t, n, songs = torch_cuda, 3, idx.n_songs
    res, top, found = ((0, 24), t.uint8), ((0, n, 24), t.uint8), ((0,), t.int32)
    stats, block, words = ((0, 3), t.int64), ((0, songs, 2), t.float32), ((0,), t.int64)
    want = {"match_windows": (res,), "match_windows_topn": (top, found), "match_windows_dense": (res,),
            "match_windows_dense_stats": (res, stats), "match_windows_dense_topn": (top, found, block),
            "match_windows_dense_topn_stats": (top, found, block, stats), "match_windows_dense_part": (words, stats),
            "match_windows_dense_topn_part": (top, found)}[form]
    host = {res: ((0,), DeviceIndex.RESULT_DTYPE), top: ((0, n), DeviceIndex.RESULT_DTYPE), found: ((0,), np.dtype(np.int32)),
            stats: ((0,), STATS_DTYPE), block: ((0, songs, 2), np.dtype(np.float32))}
    kw = {"match_windows_dense_topn": {"want_song_scores": True}, "match_windows_dense_topn_stats": {"want_song_scores": True},
          "match_windows_dense_part": {"stats": True}}.get(form, {})
    has_to_host = "part" not in form
    lib, idx.lib = idx.lib, _NoLibrary()
    try:
        out, wfirst = _call(idx, form, q, labels, [0] * len(rlen), rlen, 19, 2, n, **kw, **({"to_host": False} if has_to_host else {}))
        assert wfirst.dtype == np.int64 and wfirst.tolist() == [0] * (len(rlen) + 1)
        assert [(tuple(x.shape), x.dtype) for x in _flat(out)] == list(want) and all(x.is_cuda for x in _flat(out))
        if has_to_host:
            out, wfirst = _call(idx, form, q, labels, [0] * len(rlen), rlen, 19, 2, n, **kw)
            assert wfirst.tolist() == [0] * (len(rlen) + 1)
            assert [(x.shape, x.dtype) for x in _flat(out)] == [host[w] for w in want]
    finally:
        idx.lib = lib


@pytest.mark.parametrize("form", FORMS)
def test_refusals_keep_their_order_and_text(long_case, form):
    """each with an otherwise valid call: window 0 (ValueError), n 65 (PfannError), recordings past the rows of q
    (AssertionError), exclude_song of the wrong length (ValueError), and -- in that order -- when two of them come together.
    match_windows_dense_topn_part alone refuses n before window and hop."""
    from pfann_amd.lib import PfannError
    idx, _, _, _, _, q, labels, rstart, rlen = long_case
    past = [rlen[0], rlen[1] + 1]                       # the second recording ends one row behind the last row of q

    def refused(exc, text, **kw):
        a = dict(rstart=rstart, rlen=rlen, window=19, hop=2)
        a.update(kw)
        with pytest.raises(exc, match=text):
            _call(idx, form, q, labels, **a)

    refused(ValueError, "^%s: window and hop are positive" % form, window=0)
    refused(ValueError, "^%s: window and hop are positive" % form, hop=0)
    refused(AssertionError, "recordings exceed the rows given", rlen=past)
    refused(ValueError, "^%s: window and hop are positive" % form, rlen=past, window=0)
    if form in RANKED:
        refused(PfannError, "^%s: n=65 outside 1\\.\\.64" % form, n=65)
        refused(PfannError, "^%s: n=0 outside 1\\.\\.64" % form, n=0)
        refused(PfannError, "^%s: n=65 outside 1\\.\\.64" % form, n=65, rlen=past)
        if form == "match_windows_dense_topn_part":
            refused(PfannError, "^%s: n=65 outside 1\\.\\.64" % form, n=65, window=0)
        else:
            refused(ValueError, "^%s: window and hop are positive" % form, n=65, window=0)
    if form in DENSE:
        refused(ValueError, "^%s: exclude_song wants one song id per recording \\(2\\)" % form, exclude_song=[-1])
        refused(AssertionError, "recordings exceed the rows given", exclude_song=[-1], rlen=past)
        refused(AssertionError, "one start per recording", rstart=rstart[:1], exclude_song=[-1])
        if form in RANKED:
            refused(PfannError, "^%s: n=65 outside 1\\.\\.64" % form, n=65, exclude_song=[-1])


# ------------------------------------------------------------------------------------------------ scratch growth
def test_match_scratch_grows_between_two_calls(long_case):
    """2 queries (the phased plan: a slab of 2 x 2048 slots), then 65 queries of 128 rows (65 x 16384 slots: the slab grows),
    then the 2 again: the first and the third answer are the same bytes, and the exact oracle's"""
    _, db, pos, hq, hlabels, q, labels, _, _ = long_case
    idx = _new_index(db, pos)                           # (its own handle: the scratch starts empty)
    small = ([3, 700], [19, 19])
    assert mx.match_plan(2, 19, K)[0] == "phased_rank" and mx.match_plan(65, 128, K)[0] == "single_hbm"
    want = [mx.exact_match(hq[s:s + n], hlabels[s:s + n], mx.IntRows(db), pos, 1, 0) for s, n in zip(*small)]
    first, _ = idx.match(q, labels, *small)
    big, _ = idx.match(q, labels, [20 * j for j in range(65)], [128] * 65)
    third, _ = idx.match(q, labels, *small)
    assert (big["song"] >= 0).all()
    assert not mc.differing(first, want), mc.differing(first, want)
    assert first.tobytes() == third.tobytes()


def test_dense_workspace_grows_between_two_calls(long_case):
    """match_windows_dense_topn on 1 window (one row-tile slot), on 40 windows at hop 8 (three slots: the workspace grows), on
    the 1 again: the same bytes before and after, the exact oracle's, and window 0 of the larger call"""
    _, db, pos, hq, _, q, _, _, _ = long_case
    idx = _new_index(db, pos)
    window, hop, n = 8, 8, 3
    one = lambda: idx.match_windows_dense_topn(q, [0], [window], window, hop, n)
    (top1, found1, _), wfirst = one()
    (top40, found40, _), wfirst40 = idx.match_windows_dense_topn(q, [0], [window + 39 * hop], window, hop, n)
    (top3, found3, _), _ = one()
    assert wfirst.tolist() == [0, 1] and wfirst40.tolist() == [0, 40]
    want = dtc.dense_topn_oracle(hq, db, pos, window, hop, [0], [window], n)
    bad = dtc.differing(top1, found1, None, want)
    assert not bad, bad
    assert top1.tobytes() == top3.tobytes() and found1.tobytes() == found3.tobytes()
    assert top40[:1].tobytes() == top1.tobytes() and found40[:1].tobytes() == found1.tobytes()


if __name__ == "__main__":
    assert sys.argv[1:] == ["routing"], sys.argv
    import torch
    print(json.dumps(_routing(torch)))
