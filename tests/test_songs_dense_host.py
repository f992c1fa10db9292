"""Host side of the rescoring stage (pfann_match_songs_dense, matcher.py --rescore): the oracle of tests/songs_dense_cases.py
against the ranked dense oracle, the declaration and the binding, and every refusal of the command line."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dense_cases as dc
import dense_topn_cases as dt
import songs_dense_cases as sc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world", ["small", "packed"])
def test_with_every_song_listed_the_oracle_is_the_ranked_dense_oracle(world):
    """queries as one-window recordings of the ranked dense matcher (window 64: a shorter recording is one window over all its
    rows); lists that name every song, in descending order and with repeats: the lists are equal with =="""
    db, pos, q, _, _ = dc.small_world() if world == "small" else dt.packed_world()
    n_songs = len(pos) - 1
    qstart, qlen = sc.cut_queries(q.shape[0], lengths=(1, 19, 64))
    lists = [list(range(n_songs))[::-1] + [0, n_songs - 1, -1, n_songs] for _ in qlen]
    m = len(lists[0])
    got = sc.songs_dense_oracle(q, db, pos, qstart, qlen, lists)
    want = dt.dense_topn_oracle(q, db, pos, 64, 1, qstart, qlen, m)
    assert len(got) == len(want) == len(qlen) > 0
    for j, (g, w) in enumerate(zip(got, want)):
        assert g["top"] == w["top"] and g["n_found"] == w["n_found"] == int((np.diff(pos) > 0).sum()), j
    # a shorter list is the same ranking restricted to its songs
    have = np.flatnonzero(np.diff(pos) > 0)
    few = [[int(have[-1]), -1, int(have[0]), int(have[-1])] for _ in qlen]
    for g, w in zip(sc.songs_dense_oracle(q, db, pos, qstart, qlen, few), want):
        keep = [h for h in w["top"] if h[0] in (int(have[0]), int(have[-1]))]
        assert g["top"] == keep + [dt.PAD] * 2 and g["n_found"] == 2
    assert sc.songs_dense_oracle(q, db, pos, [0], [0], [[0, 1]])[0] == dict(top=[dt.PAD] * 2, n_found=0, block=None)


def test_header_declares_and_lib_binds_the_call():
    header = open(os.path.join(REPO, "include", "pfann_amd.h")).read()
    assert re.search(r"\bint\s+pfann_match_songs_dense\s*\(", header)
    assert re.search(r"#define\s+PFANN_SONGS_DENSE_MAX_ROWS\s+64\b", header)
    from pfann_amd import lib
    assert len(lib.SYMBOLS["pfann_match_songs_dense"][1]) == 10
    from pfann_amd.build import SOURCES
    assert "dense_songs.hip" in SOURCES
    from pfann_amd.database import Database, DeviceIndex
    assert callable(DeviceIndex.match_songs_dense) and callable(Database.query_rescore_batch)
    assert callable(Database.query_rescore_launch) and callable(Database.query_rescore_finish)


def test_rescore_flag_parser():
    from pfann_amd.launch import matcher_dense_flag, matcher_flags, matcher_rescore_flag
    assert matcher_rescore_flag([]) == (0, None) and matcher_rescore_flag(["--top", "5", "--no-bin"]) == (0, None)
    assert matcher_rescore_flag(["--rescore", "8", "--no-bin", "--top", "3"]) == (8, None)
    assert matcher_rescore_flag(["--no-bin", "--rescore=64", "--top=64"]) == (64, None)
    assert matcher_flags(["--rescore", "8", "--no-bin", "--top", "3"]) == (3, True, None)       # (the other parsers skip the flag)
    assert matcher_dense_flag(["--rescore", "8", "--no-bin"]) == (False, None)
    for args in (["--rescore"], ["--rescore", "x", "--no-bin"], ["--rescore", "0", "--no-bin"], ["--rescore=65", "--no-bin"]):
        n, err = matcher_rescore_flag(args)
        assert n == 0 and "1 to 64" in err, args
    assert "--dense" in matcher_rescore_flag(["--rescore", "8", "--no-bin", "--dense"])[1]
    assert "out of scope" in matcher_rescore_flag(["--rescore", "8"])[1]
    assert "--top 9" in matcher_rescore_flag(["--rescore", "8", "--no-bin", "--top", "9"])[1]


def _matcher(args, **env):
    e = dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="", **env)
    return subprocess.run([sys.executable, os.path.join(REPO, "matcher.py"), "no_list.txt", "no_db", "no_result.txt"] + args,
                          capture_output=True, text=True, env=e, timeout=300)


@pytest.mark.parametrize("args,env,word", [(["--rescore", "0", "--no-bin"], {}, "1 to 64"),
                                           (["--rescore", "65", "--no-bin"], {}, "1 to 64"),
                                           (["--rescore", "8", "--no-bin", "--dense"], {}, "--dense"),
                                           (["--rescore", "8"], {}, "--no-bin"),
                                           (["--rescore", "8", "--no-bin", "--top", "9"], {}, "--top"),
                                           (["--rescore", "8", "--no-bin"], {"PFANN_GPUS": "2"}, "multi-GPU"),
                                           (["--rescore", "8", "--no-bin"], {"WORLD_SIZE": "2"}, "multi-GPU")])
def test_cli_refuses_bad_flags_before_it_touches_anything(args, env, word):
    """(the list, the database and a GPU do not exist here: anything but the early exit would fail otherwise)"""
    r = _matcher(args, **env)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:], r.stderr[-500:])
    assert len(r.stderr.strip().splitlines()) == 1 and r.stdout == "" and word in r.stderr
