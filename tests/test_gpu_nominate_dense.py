"""Dense song nomination on the GPU (pfann_nominate_songs_dense, csrc/nominate.hip): `==` against the ranked dense matcher on
the exact grid; tile edges; the margin E and the certificate n_close on real-valued rows; the byte contract across batch,
max_qlen, chunking and n; special queries and refusals; Database.query_nominate_rescore_batch and the matcher CLI."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_topn_cases as dt
import match_exact as mx
from fp16_margin_cases import margin_ref as _margin      # E_j as the select kernel forms it: fp32 eps_t and norms, the rest in double

pytestmark = pytest.mark.gpu
D = 128
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _starts(qlen):
    return [int(x) for x in np.pad(np.cumsum(qlen), (1, 0))[:-1]]


def _dense_ref(idx, qd, qstart, qlen, n):
    """the ranked dense matcher on one-window recordings of the queries' rows -> (top [nQ, n], n_found)"""
    (ref, ref_found, _), wfirst = idx.match_windows_dense_topn(qd, qstart, qlen, 64, 1, n)
    assert wfirst.tolist() == list(range(len(qlen) + 1))
    return ref, ref_found


def _assert_equals_dense(idx, torch, q, qstart, qlen, n, max_qlen=None, what=""):
    """songs, scores, n_cand and n_found of every entry == the ranked dense matcher's; offset and shift 0"""
    qd = torch.as_tensor(q).cuda()
    ref, ref_found = _dense_ref(idx, qd, qstart, qlen, n)
    cand, n_found, n_close = idx.nominate_songs_dense(qd, qstart, qlen, n, max_qlen=max_qlen)
    assert cand.shape == (len(qlen), n)
    for f in ("song", "n_cand", "score"):
        bad = np.argwhere(cand[f] != ref[f])
        assert bad.size == 0, "%s n %d field %s: query %d entry %d: %r, the dense matcher %r" % (
            what, n, f, bad[0][0], bad[0][1], cand[f][tuple(bad[0])], ref[f][tuple(bad[0])])
    assert (cand["offset"] == 0).all() and (cand["shift"] == 0).all()
    assert np.array_equal(n_found, ref_found), (what, n_found.tolist(), ref_found.tolist())
    assert ((n_close >= 1) | (ref_found == 0)).all() and (n_close <= ref_found).all()
    return cand, n_found, n_close


# ------------------------------------------------------------------------------------------------ exact arithmetic
@pytest.mark.parametrize("d", [128, 64])
def test_exact_on_the_grid(torch_cuda, d):
    """every value is k/16: fp16 products and fp32 sums are exact, so the approximate score IS the dense score"""
    db, pos = mx.std_world(41, d, long_rows=300)
    assert len(pos) - 1 == 61
    mx.assert_exact_domain(64, d)
    idx = _index(("std300", d), db, pos)
    lens = [1, 5, 19, 64]
    batches = [mx.aligned(701, db, pos, lens * 2, 2), mx.tie_storm(702, db, pos, lens * 2, 2, mx.STD_COPIES, mx.STD_PERIODIC),
               mx.edges(703, db, pos, lens * 2, 2)]
    q = np.concatenate([b.q for b in batches])
    qlen = [n for b in batches for n in b.qlen]
    qstart = _starts(qlen)
    for n in (1, 3, 64):
        cand, n_found, _ = _assert_equals_dense(idx, torch_cuda, q, qstart, qlen, n, what="std d %d" % d)
        if n == 64:
            assert (n_found == int((np.diff(pos) > 0).sum())).all() and (cand["song"][:, -1] == -1).all()
    # a cut from song 5, whose copy is song 9: they tie, the lower song first
    s = int(pos[5])
    cand, _, n_close = idx.nominate_songs_dense(torch_cuda.as_tensor(db[s:s + 19]).cuda(), [0], [19], 3)
    assert cand["song"][0, :2].tolist() == [5, 9] and cand["score"][0, 0] == cand["score"][0, 1] and n_close[0] >= 2


# ------------------------------------------------------------------------------------------------ tile edges
def test_tile_edges(torch_cuda):
    torch = torch_cuda
    db, pos, q, _, _ = dt.packed_world(D)
    lens = np.diff(pos)
    assert (lens == 1).sum() == 200 and (lens == 0).sum() > 5 and db.shape[0] % (128 - 18) != 0
    idx = _index("packed", db, pos)
    # seven queries of 19 rows: P = 6 slots per tile, query 5 sits in the last slot, query 6 alone in its tile
    qlen = [19] * 7
    for n in (1, 64):
        _assert_equals_dense(idx, torch, q[:133], _starts(qlen), qlen, n, what="packed 7 x 19")
    # max_qlen 1: SJ = 128, 128 one-row queries per tile (130: a second tile); max_qlen 64: SJ = 65, two slots
    _assert_equals_dense(idx, torch, q[:130], list(range(130)), [1] * 130, 64, max_qlen=1, what="packed max_qlen 1")
    qlen = [64, 1, 64, 33, 2]
    _assert_equals_dense(idx, torch, q[:164], _starts(qlen), qlen, 64, max_qlen=64, what="packed max_qlen 64")
    # mixed lengths in slots of 19, and of 40 (three slots)
    qlen = [19, 3, 1, 17, 19, 8, 19, 19]
    for m in (19, 40):
        _assert_equals_dense(idx, torch, q[100:205], _starts(qlen), qlen, 5, max_qlen=m, what="packed mixed, max_qlen %d" % m)
    # a database smaller than one tile
    full, fpos = mx.std_world(41, D)
    sdb = np.ascontiguousarray(full[fpos[3]:fpos[7]])
    spos = (fpos[3:8] - fpos[3]).astype(np.int64)
    sq = np.concatenate([sdb[10:29], mx.grid_rows(9, "tiny/q", 8, D)])
    assert 0 < sdb.shape[0] < 110
    sidx = _index("tiny", sdb, spos)
    qlen = [19, 7, 1]
    _assert_equals_dense(sidx, torch, sq[:27], _starts(qlen), qlen, 64, what="tiny")


# ------------------------------------------------------------------------------------------------ the margin, the certificate
EXCERPT_SONGS = (0, 1, 3, 6, 8, 10, 11, 0, 3)            # none of the self-match world's duplicates (2/7, 4/9)


@pytest.fixture(scope="module")
def noisy_world(tmp_path_factory):
    """dense_cases.selfmatch_world and nine excerpts of 5 / 19 / 40 rows plus noise of 0.3 / 1 / 2 times the signal, then three
    pure-noise queries -> (dir, emb, pos, q, qstart, qlen, number of excerpts)"""
    d = str(tmp_path_factory.mktemp("nominate_self"))
    emb, pos = dc.selfmatch_world(d)
    rng = np.random.default_rng(31)
    rows, qlen = [], []
    for i, (n, level) in enumerate((n, level) for n in (5, 19, 40) for level in (0.3, 1.0, 2.0)):
        s = EXCERPT_SONGS[i]
        a = int(pos[s]) + i
        assert a + n <= pos[s + 1]
        noise = rng.standard_normal((n, D)) / np.sqrt(D)
        x = emb[a:a + n].astype(np.float64) + level * noise
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
        qlen.append(n)
    for n in (5, 19, 40):
        x = rng.standard_normal((n, D))
        rows.append(x / np.linalg.norm(x, axis=1, keepdims=True))
        qlen.append(n)
    return d, emb, pos, np.concatenate(rows).astype(np.float32), _starts(qlen), qlen, 9


def test_bound_and_certificate(torch_cuda, noisy_world):
    torch = torch_cuda
    _, emb, pos, q, qstart, qlen, n_excerpts = noisy_world
    idx = _index("self", emb, pos)
    qd = torch.as_tensor(q).cuda()
    have = int((np.diff(pos) > 0).sum())
    ref, ref_found = _dense_ref(idx, qd, qstart, qlen, 64)
    cand, n_found, n_close = idx.nominate_songs_dense(qd, qstart, qlen, 64)
    assert (n_found == have).all() and np.array_equal(n_found, ref_found)
    xmax = idx.row_norm_max()
    worst = 0.0
    for j, n in enumerate(qlen):
        E = _margin(q[qstart[j]:qstart[j] + n], D, xmax)
        assert 0 < E < 0.06 * max(1.0, n / 19.0)
        T = {int(e["song"]): float(np.float32(e["score"] * n)) for e in ref[j][:have]}
        A = {int(e["song"]): float(np.float32(e["score"] * n)) for e in cand[j][:have]}
        assert sorted(A) == sorted(T)
        err = max(abs(A[s] - T[s]) for s in T)
        worst = max(worst, err / E)
        print("query %d (%d rows): max |A - T| = %.3g, E = %.3g, n_close = %d" % (j, n, err, E, int(n_close[j])))
        assert err <= E, (j, err, E)
        a = np.asarray(sorted(A.values(), reverse=True))
        assert np.abs(a - (a[0] - 2 * E)).min() > 1e-4 * E, "a song sits on the threshold: the recount is not decisive"
        assert int(n_close[j]) == int((a >= a[0] - 2 * E).sum()), j
        if j < n_excerpts:                               # the condition of the issue: gaps of 1.8 .. 38 against 2 E <= 0.11
            assert int(n_close[j]) == 1 and int(cand["song"][j, 0]) == EXCERPT_SONGS[j], j
    print("largest |A - T| / E: %.4f" % worst)
    for N in (1, 3):
        raw, _, close = idx.nominate_songs_dense(qd, qstart, qlen, N, to_host=False)
        top, _ = idx.match_songs_dense(qd, qstart, qlen, raw)
        close = close.cpu().numpy()
        assert np.array_equal(close, n_close)
        sure = [j for j in range(len(qlen)) if 0 <= close[j] <= N]
        assert len(sure) >= n_excerpts
        for j in sure:
            assert top[j, 0:1].tobytes() == ref[j, 0:1].tobytes(), (N, j)


# ------------------------------------------------------------------------------------------------ the byte contract
def test_byte_contract(torch_cuda, noisy_world):
    torch = torch_cuda
    _, emb, pos, q, qstart, qlen, _ = noisy_world
    idx = _index("self", emb, pos)
    j0 = 4                                               # 19 rows
    mine = q[qstart[j0]:qstart[j0] + qlen[j0]]

    def alone(n, **kw):
        c, f, cl = idx.nominate_songs_dense(torch.as_tensor(mine).cuda(), [0], [qlen[j0]], n, **kw)
        return c[0].tobytes(), int(f[0]), int(cl[0])
    want = alone(64)
    assert alone(64) == want, "two runs differ"
    full, f, cl = idx.nominate_songs_dense(torch.as_tensor(q).cuda(), qstart, qlen, 64)           # max_qlen 40, longer neighbours
    assert (full[j0].tobytes(), int(f[j0]), int(cl[j0])) == want, "the bytes depend on the batch or on max_qlen"
    assert alone(64, max_qlen=64) == want and alone(64, max_qlen=23) == want
    os.environ["PFANN_NOMINATE_QUERIES"] = "1"
    try:
        one, f1, cl1 = idx.nominate_songs_dense(torch.as_tensor(q).cuda(), qstart, qlen, 64)
    finally:
        del os.environ["PFANN_NOMINATE_QUERIES"]
    assert one.tobytes() == full.tobytes() and np.array_equal(f, f1) and np.array_equal(cl, cl1), "the bytes depend on the chunking"
    three, f3, cl3 = idx.nominate_songs_dense(torch.as_tensor(q).cuda(), qstart, qlen, 3)
    assert three.tobytes() == np.ascontiguousarray(full[:, :3]).tobytes() and np.array_equal(f3, f) and np.array_equal(cl3, cl)


# ------------------------------------------------------------------------------------------------ special queries, refusals
def test_special_queries(torch_cuda, noisy_world):
    torch = torch_cuda
    from pfann_amd.database import DeviceIndex
    _, emb, pos, q, _, _, _ = noisy_world
    idx = _index("self", emb, pos)
    rows = q[:60].copy()
    rows[30, 7] = np.nan                                 # query 3
    rows[45] *= 1e5                                      # query 4: a norm outside fp16's range
    qlen = [19, 0, 11, 15, 10, 5]
    qstart = [0, 19, 19, 30, 45, 55]
    cand, n_found, n_close = idx.nominate_songs_dense(torch.as_tensor(rows).cuda(), qstart, qlen, 4, max_qlen=15)
    pad = np.asarray([dt.PAD] * 4, DeviceIndex.RESULT_DTYPE).tobytes()
    assert n_found.tolist() == [-1, 0, 11, -1, -1, 11] and n_close[[0, 1, 3, 4]].tolist() == [-1, 0, -1, -1]
    for j in (0, 1, 3, 4):
        assert cand[j].tobytes() == pad, j
    for j in (2, 5):                                     # their neighbours do not touch them
        a, f, c = idx.nominate_songs_dense(torch.as_tensor(rows[qstart[j]:qstart[j] + qlen[j]]).cuda(), [0], [qlen[j]], 4)
        assert a[0].tobytes() == cand[j].tobytes() and f[0] == n_found[j] and c[0] == n_close[j] and c[0] >= 1


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
    db12, pos12 = mx.std_world(41, 12)
    no_copy = _index("std12", db12, pos12)
    q = torch.as_tensor(db[:30]).cuda()
    q12 = torch.as_tensor(db12[:30]).cuda()
    qs = torch.zeros(1, dtype=torch.int64).cuda()
    ql = torch.full((1,), 30, dtype=torch.int32).cuda()

    def call(idx, n, max_qlen, nQ=1):
        outs = [torch.full((size,), 0xA5, dtype=torch.uint8).cuda() for size in (65 * ctypes.sizeof(L.MatchResult), 4, 4)]
        rc = lib.pfann_nominate_songs_dense(idx.handle, (q12 if idx is no_copy else q).data_ptr(), qs.data_ptr(), ql.data_ptr(), nQ,
                                            max_qlen, n, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None)
        msg = L.last_error()
        torch.cuda.synchronize()
        return rc, msg, [bool((o.cpu() == 0xA5).all()) for o in outs]

    rc, _, untouched = call(whole, 3, 30)                # the control: the same call on a good handle writes all three
    assert rc == 0 and not any(untouched)
    for idx, n, m, nQ, word in ((shard, 3, 30, 1, "shard"), (half, 3, 30, 1, "fp16-only"), (no_copy, 3, 30, 1, "no fp16 copy"),
                                (whole, 0, 30, 1, "n=0"), (whole, 65, 30, 1, "n=65"), (whole, 3, 0, 1, "max_qlen=0"),
                                (whole, 3, 65, 1, "max_qlen=65"), (whole, 3, 30, -1, "nQ=-1"),
                                (shard, 0, 65, 1, "shard"), (half, 65, 0, 1, "fp16-only"), (no_copy, 0, 0, 1, "no fp16 copy"),
                                (whole, 0, 0, -1, "n=0"), (whole, 3, 0, -1, "max_qlen=0")):      # several at once: the first one
        rc, msg, untouched = call(idx, n, m, nQ)
        assert rc == -1 and msg and word in msg and all(untouched), (n, m, nQ, word, rc, msg, untouched)
    with pytest.raises(L.PfannError) as refused:
        shard.match_windows_dense_topn(q, [0], [30], 5, 1, 3)
    dense_msg = str(refused.value).split(": ", 1)[1]
    assert call(shard, 3, 30)[1] == dense_msg, "a shard is refused with another message than the dense matcher's"
    with pytest.raises(L.PfannError) as refused:
        half.match_songs_dense(q, [0], [30], [[1, 2]])
    half_msg = str(refused.value).split(": ", 1)[1]
    assert "fp16-only" in half_msg and call(half, 3, 30)[1] == half_msg.replace("match_songs_dense", "nominate_songs_dense")
    with pytest.raises(L.PfannError, match="1..64"):
        whole.nominate_songs_dense(q, [0], [30], 65)


# ------------------------------------------------------------------------------------------------ the Database layer
def test_database_query_nominate_rescore_batch(torch_cuda, noisy_world):
    from pfann_amd import database as dbm
    from pfann_amd import lib as L
    from pfann_amd.utils import read_config
    torch = torch_cuda
    dirname, emb, pos, q, qstart, qlen, n_excerpts = noisy_world
    cfg = read_config(os.path.join(dirname, "configs.json"))
    db = dbm.Database(dirname, cfg["indexer"], cfg["hop_size"], d=D)
    qd = torch.as_tensor(q).cuda()
    dense_answers, dense_ranked = db.query_dense_batch(qd, qstart, qlen, n=64)
    for n in (1, 3, 64):
        answers, ranked, certified = db.query_nominate_rescore_batch(qd, qstart, qlen, n)
        assert len(answers) == len(ranked) == len(certified) == len(qlen) and all(a[2] is None for a in answers)
        assert all(bool(c) for c in certified[:n_excerpts])
        for j in range(len(qlen)):
            assert len(ranked[j]) <= n and ranked[j][0] == answers[j][:2]
            if certified[j]:
                assert answers[j][:2] == dense_answers[j][:2], (n, j)
        if n == 64:                                      # every song is listed: certified, and the whole list is the dense list
            assert all(bool(c) for c in certified) and ranked == dense_ranked
    for change, word in (({"frame_shift_mul": 2}, "frame_shift_mul"), ({"score_alpha": 2.0}, "score_alpha")):
        other = dbm.Database(dirname, dict(cfg["indexer"], **change), cfg["hop_size"], d=D)
        with pytest.raises(L.PfannError, match=word):
            other.query_nominate_rescore_batch(qd, qstart, qlen, 4)
    with pytest.raises(L.PfannError, match="1..64"):
        db.query_nominate_rescore_launch(qd, qstart, qlen, 65)


# ------------------------------------------------------------------------------------------------ the CLI
def _run(script, args, cwd, env=None):
    """one command-line tool as a child under the suite's limits (tests/test_gpu_dense.py::_run)"""
    return subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.join(REPO, script)] + args, cwd=cwd,
                          capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=REPO, **(env or {})), timeout=460)


def _matcher(args, cwd, env=None):
    return _run("matcher.py", args, cwd, env)


def test_cli_nominate_dense(torch_cuda, tmp_path):
    """--rescore 3 --no-bin --nominate dense --top 3 writes the TSV and _detail.csv of --dense --no-bin, and _nominate.csv"""
    from pfann_amd import synth
    params, mdir, music, truth = dc.four_excerpts(tmp_path)
    r = _run("builder.py", [str(tmp_path / "music.txt"), str(tmp_path / "db"), mdir], str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    sr = 8000
    names = []
    for i, (t0, t1, s, o) in enumerate(truth):
        sig = synth.make_song(500 + s, seconds=40.0 + (s % 7))[int(o) * sr:int(o + 10) * sr].astype(np.float64)
        noise = synth.normal(78, "nom/cli/%d" % i, sig.shape[0]).astype(np.float64)
        x = sig + noise * np.sqrt(np.mean(sig ** 2))     # SNR 0 dB
        path = str(tmp_path / ("q%d.wav" % i))
        synth.write_wav(path, np.clip(x / np.abs(x).max() * 30000.0, -32768, 32767).astype(np.int16))
        names.append(path)
    names.append(str(tmp_path / "missing.wav"))
    (tmp_path / "queries.txt").write_text("".join(p + "\n" for p in names))
    lst, dbdir = str(tmp_path / "queries.txt"), str(tmp_path / "db")
    r = _matcher([lst, dbdir, str(tmp_path / "dense.tsv"), "--dense", "--no-bin"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    r = _matcher([lst, dbdir, str(tmp_path / "nom.tsv"), "--rescore", "3", "--no-bin", "--nominate", "dense", "--top", "3"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    assert (tmp_path / "nom.tsv").read_bytes() == (tmp_path / "dense.tsv").read_bytes()
    assert (tmp_path / "nom_detail.csv").read_bytes() == (tmp_path / "dense_detail.csv").read_bytes()
    rows = (tmp_path / "nom_nominate.csv").read_text().splitlines()
    assert rows[0] == "query,n_close,certified" and len(rows) == len(names) + 1
    for name, row in zip(names[:-1], rows[1:]):
        got = row.rsplit(",", 2)
        assert got[0] == name and int(got[1]) >= 1 and got[2] == "1", row
    assert rows[-1].rsplit(",", 2)[1:] == ["-1", "0"]
    top = (tmp_path / "nom_top.csv").read_text().splitlines()
    assert top[0] == "query,rank,answer,score,time" and len(top) > len(names)
    tsv = (tmp_path / "nom.tsv").read_text().splitlines()
    for (t0, t1, s, o), line in zip(truth, tsv):
        assert line.split("\t")[1].endswith("song%02d.wav" % s), line
    assert not (tmp_path / "nom.tsv.bin").exists()
    for args, env, word in ((["--no-bin", "--nominate", "dense"], None, "--rescore"),
                            (["--rescore", "3", "--no-bin", "--nominate", "sparse"], None, "dense"),
                            (["--rescore", "3", "--no-bin", "--nominate", "dense"], {"PFANN_GPUS": "2"}, "multi-GPU")):
        out = tmp_path / "refused.tsv"
        r = _matcher([lst, dbdir, str(out)] + args, str(tmp_path), env)
        assert r.returncode == 2 and word in r.stderr and len(r.stderr.strip().splitlines()) == 1, (args, r.returncode, r.stderr)
        assert not out.exists() and not (tmp_path / "refused_nominate.csv").exists()
