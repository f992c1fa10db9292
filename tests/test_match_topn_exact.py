"""Pins tests/match_topn_exact.py (the exact oracle of pfann_match_topn) against match_exact.exact_match and against the
reference-derived oracle/seqscore.py, checks that the generators reach every input regime the GPU tests rely on, and covers the
host-only part of the matcher CLI's --top / --no-bin flags.  No tolerance anywhere."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import match_exact as mx
import match_topn_exact as tx
from oracle import seqscore as osq
from pfann_amd.database import _fine_to_time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 32
K = 20
QLENS = [1, 2, 3, 5, 8, 11, 16, 19, 4, 7, 13, 6]
FAMILIES = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2)]


def _world():
    return mx.std_world(41, D)


def _batches(fsm):
    db, pos = _world()
    return {"aligned": mx.aligned(1, db, pos, QLENS, K, fsm),
            "tie_storm": mx.tie_storm(2, db, pos, QLENS, K, mx.STD_COPIES, mx.STD_PERIODIC, fsm),
            "edges": mx.edges(3, db, pos, QLENS, K, fsm),
            "collapse": mx.collapse(4, db, pos, QLENS, K, fsm)}


def _queries(b):
    return [(b.q[s:s + n], b.labels[s:s + n]) for s, n in zip(b.qstart, b.qlen)]


def _check_against_block(t, ss, n, what):
    """the float32 relation between a ranked list and a per-song block ss [n_songs, 2] (score, alignment in fine frames)"""
    ent = [e for e in t["top"] if e[0] >= 0 and np.float32(e[4]) > 0]
    for e, alone in zip(t["top"], t["f32_alone"]):
        if e[0] >= 0 and np.float32(e[4]) > 0:
            assert np.float32(e[4]) == ss[e[0], 0], (what, e)
            if alone:
                assert np.float32(e[1] * t["fsm"] - e[2]) == ss[e[0], 1], (what, e)
    if n >= t["n_found"]:
        assert {e[0] for e in ent} == set(np.flatnonzero(ss[:, 0] > 0).tolist()), what


@pytest.mark.parametrize("mode,fsm", FAMILIES)
@pytest.mark.parametrize("n", [1, 5, 64])
def test_helper_agrees_with_exact_match(mode, fsm, n):
    db, pos = _world()
    rows = mx.IntRows(db)
    for gen, b in _batches(fsm).items():
        for j, (q, lab) in enumerate(_queries(b)):
            w = mx.exact_match(q, lab, rows, pos, fsm, mode)
            t = tx.exact_topn(q, lab, rows, pos, fsm, mode, n)
            e = t["top"][0]
            assert (e[0], e[1], e[2], e[4]) == (w["song"], w["offset"], w["shift"], w["score"]), (gen, j, e, w["top"])
            assert len(t["top"]) == n and sum(x[3] for x in t["top"]) <= w["n_cand"]
            if n >= t["n_found"]:
                assert sum(x[3] for x in t["top"]) == w["n_cand"], (gen, j)          # every candidate votes for one song
                assert t["top"][t["n_found"]:] == [tx.PAD] * (n - t["n_found"])
            sc = [x[4] for x in t["top"]]
            assert sc == sorted(sc, reverse=True) and len({x[0] for x in t["top"] if x[0] >= 0}) == min(n, t["n_found"])
            t["fsm"] = fsm
            _check_against_block(t, w["ss"], n, (gen, j))


@pytest.mark.parametrize("fsm", [1, 2])
def test_helper_agrees_with_the_reference_derived_oracle(fsm):
    """oracle/seqscore.py (database.py:129-163 restated): its winner is entry 0, its song-score output obeys the same float32
    relation"""
    db, pos = _world()
    rows = mx.IntRows(db)
    for gen, b in _batches(fsm).items():
        for j, (q, lab) in enumerate(_queries(b)):
            if q.shape[0] < fsm:            # the reference itself stops here
                continue
            score, (song, tm), ss = osq.query_embeddings_base(q.astype(np.float64), lab, db.astype(np.float64), pos, 1.0, fsm)
            t = tx.exact_topn(q, lab, rows, pos, fsm, 0, 64)
            e = t["top"][0]
            assert (e[0], e[4]) == (song, score), (gen, j)
            if song >= 0:
                assert tm == e[1] - e[2] / fsm
            for x, alone in zip(t["top"], t["f32_alone"]):
                if x[0] >= 0 and np.float32(x[4]) > 0:
                    assert np.float32(x[4]) == ss[x[0], 0], (gen, j, x)
                    if alone:
                        assert np.float32(_fine_to_time(x[1] * fsm - x[2], fsm, 1.0)) == ss[x[0], 1], (gen, j, x)
            assert t["n_found"] <= 64
            assert {x[0] for x in t["top"] if x[0] >= 0 and np.float32(x[4]) > 0} == set(np.flatnonzero(ss[:, 0] > 0).tolist())


@pytest.mark.parametrize("mode,fsm", FAMILIES)
def test_generators_reach_every_regime(mode, fsm):
    """checked on the oracle alone, n = 5: more songs than n, fewer than n, none, two songs tied at a ranked position, a best
    score below 0"""
    db, pos = _world()
    rows = mx.IntRows(db)
    n = 5
    seen = set()
    for gen, b in _batches(fsm).items():
        for q, lab in _queries(b):
            t = tx.exact_topn(q, lab, rows, pos, fsm, mode, n)
            nf = t["n_found"]
            seen.add("more" if nf > n else "fewer" if 0 < nf < n else "none" if nf == 0 else "n")
            real = [x for x in t["top"] if x[0] >= 0]
            if any(a[4] == c[4] and a[0] != c[0] for a, c in zip(real, real[1:])):
                seen.add("tied")
            if real and real[0][4] < 0:
                seen.add("negative")
    assert {"more", "fewer", "none", "tied", "negative"} <= seen, seen


# ------------------------------------------------------------------------------------------------ host side of the CLI
def _matcher(args, **env):
    e = dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="", **env)
    return subprocess.run([sys.executable, os.path.join(REPO, "matcher.py"), "no_list.txt", "no_db", "no_result.txt"] + args,
                          capture_output=True, text=True, env=e, timeout=300)


@pytest.mark.parametrize("args,env", [(["--top", "0"], {}), (["--top", "65"], {}), (["--top", "5"], {"PFANN_GPUS": "2"}),
                                      (["--no-bin"], {"WORLD_SIZE": "2"})])
def test_cli_refuses_bad_flags_before_it_touches_anything(args, env, tmp_path):
    """(the list, the database and a GPU do not exist here: anything but the early exit would fail otherwise)"""
    r = _matcher(args, **env)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert len(r.stderr.strip().splitlines()) == 1 and r.stdout == ""


def test_header_declares_and_lib_binds_the_call():
    header = open(os.path.join(REPO, "include", "pfann_amd.h")).read()
    assert re.search(r"\bint\s+pfann_match_topn\s*\(", header)
    from pfann_amd import lib
    assert len(lib.SYMBOLS["pfann_match_topn"][1]) == 16
    from pfann_amd.database import Database, DeviceIndex
    assert callable(DeviceIndex.match_topn) and callable(Database.query_topn_batch)
