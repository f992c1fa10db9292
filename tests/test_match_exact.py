"""Pins tests/match_exact.py on the CPU before the GPU module trusts it: the integer oracle against the project's two oracles
of the sequence matcher, the label generators against what they claim, and the plan names against the shapes the GPU module
uses.  No tolerance anywhere."""
import numpy as np
import pytest

import match_exact as mx
from oracle import native
from oracle import seqscore as osq
from pfann_amd.database import _fine_to_time

D = 32
QLENS = [1, 2, 3, 5, 8, 11, 16, 19, 4, 7, 13, 6]


def _world():
    return mx.std_world(7, D)


def _batches(db, pos, fsm, k=6):
    return {
        "aligned": mx.aligned(11, db, pos, QLENS, k, fsm),
        "tie_storm": mx.tie_storm(12, db, pos, QLENS, k, mx.STD_COPIES, mx.STD_PERIODIC, fsm),
        "edges": mx.edges(13, db, pos, QLENS + [9, 10, 12], k, fsm),
        "collapse": mx.collapse(14, db, pos, QLENS, k, fsm),
        "full": mx.full(15, db, pos, [4, 8, 16, 2], 8, fsm),
    }


def _ladder_batch(n_songs, fsm, k=5):
    db, pos = mx.ladder_world(21, n_songs, 16)
    return db, pos, mx.ladder(22, db, pos, [1, 4, 7, 9, 3, 5], k, fsm)


def _each(b):
    for j, (s, n) in enumerate(zip(b.qstart, b.qlen)):
        yield j, b.q[s:s + n], b.labels[s:s + n]


def _check_python_oracle(db, pos, b, fsm, what):
    rows = mx.IntRows(db)
    for j, q, lab in _each(b):
        if q.shape[0] < fsm:        # the reference itself stops here (np.concatenate of no arrays for the shifts without rows)
            continue
        w = mx.exact_match(q, lab, rows, pos, fsm, 0)
        want_ss = w["ss"].copy()
        want_ss[:, 1] = _fine_to_time(want_ss[:, 1].astype(np.int64), fsm, 1.0)
        for dt in (np.float32, np.float64):                 # both must agree with the integers: the exactness claim itself
            score, (song, tm), ss = osq.query_embeddings_base(q.astype(dt), lab, db.astype(dt), pos, 1.0, fsm)
            assert song == w["song"], (what, j, dt, song, tm, score, w["top"])
            assert score == w["score"], (what, j, dt, score, w["top"])
            if song >= 0:
                assert tm == w["offset"] - w["shift"] / fsm, (what, j, dt)
            assert np.array_equal(ss, want_ss), (what, j, dt)


def _check_c_oracle(db, pos, b, fsm, what):
    rows = mx.IntRows(db)
    for j, q, lab in _each(b):
        w = mx.exact_match(q, lab, rows, pos, fsm, 1)
        best, ss = native.seq_score(db, pos, q, lab, fsm, 0.0)
        assert best == w["song"], (what, j, best, w["top"])
        assert np.array_equal(ss, w["ss"]), (what, j)
        if best >= 0 and w["score"] > 0:
            assert ss[best, 0] == w["score"] and ss[best, 1] == w["offset"] * fsm - w["shift"], (what, j)


@pytest.mark.parametrize("fsm", [1, 2, 3])
def test_exact_match_equals_python_oracle(fsm):
    db, pos = _world()
    for name, b in _batches(db, pos, fsm).items():
        _check_python_oracle(db, pos, b, fsm, name)


@pytest.mark.parametrize("fsm", [1, 2, 3])
def test_exact_match_equals_c_oracle(fsm):
    db, pos = _world()
    for name, b in _batches(db, pos, fsm).items():
        _check_c_oracle(db, pos, b, fsm, name)


@pytest.mark.parametrize("n_songs", mx.LADDER)
def test_exact_match_equals_oracles_on_the_song_ladder(n_songs):
    for fsm in (1, 2):
        db, pos, b = _ladder_batch(n_songs, fsm)
        _check_python_oracle(db, pos, b, fsm, "ladder %d" % n_songs)
        _check_c_oracle(db, pos, b, fsm, "ladder %d" % n_songs)


def test_exact_match_owned_songs_only():
    """song_range: the candidates of the other songs are gone, the block's other rows stay 0"""
    db, pos = _world()
    b = mx.tie_storm(12, db, pos, QLENS, 6, mx.STD_COPIES, mx.STD_PERIODIC)
    for j, q, lab in _each(b):
        whole = mx.exact_match(q, lab, db, pos, 1, 0)
        parts = [mx.exact_match(q, lab, db, pos, 1, 0, (lo, hi)) for lo, hi in ((0, 8), (8, 25), (25, 56))]
        assert sum(p["n_cand"] for p in parts) == whole["n_cand"]
        assert np.array_equal(sum(p["ss"] for p in parts), whole["ss"])
        best = max(p["score"] for p in parts)
        assert best == whole["score"]
        assert [p for p in parts if p["score"] == best][0]["song"] == whole["song"]


def test_grid_rows_are_on_the_grid_and_pure():
    a = mx.grid_rows(3, "x", 500, 24)
    assert a.dtype == np.float32 and np.array_equal(a, mx.grid_rows(3, "x", 500, 24))
    assert not np.array_equal(a, mx.grid_rows(4, "x", 500, 24))
    j = a.astype(np.float64) * 16
    assert np.array_equal(j, np.rint(j)) and j.min() == -16 and j.max() == 16
    assert np.array_equal(a.astype(np.float16).astype(np.float32), a)
    u = mx.unit_grid_rows(3, "u", 200, 64)
    assert np.array_equal((u.astype(np.float64) ** 2).sum(1), np.ones(200)) and mx.IntRows(u).n == 200


def test_exact_domain_is_asserted():
    mx.assert_exact_domain(512, 128)
    with pytest.raises(AssertionError):
        mx.assert_exact_domain(513, 128)


@pytest.mark.parametrize("fsm", [1, 2])
def test_generators_produce_what_they_claim(fsm):
    db, pos = _world()
    k = 6
    bs = _batches(db, pos, fsm, k)
    rows = mx.IntRows(db)
    # tie_storm: at least two distinct candidates at the top score in at least half of the queries; an all-zero query whose
    # block stays zero; a query whose best score is negative
    b = bs["tie_storm"]
    tied = [mx.n_top_ties(q, lab, rows, pos, fsm, 0) >= 2 for _, q, lab in _each(b)]
    assert 2 * sum(tied) >= len(tied), tied
    ws = [mx.exact_match(q, lab, rows, pos, fsm, 0) for _, q, lab in _each(b)]
    zero = [w for (_, q, _), w in zip(_each(b), ws) if not q.any()]
    assert zero and all(w["score"] == 0.0 and w["song"] >= 0 and not w["ss"].any() for w in zero)
    assert any(w["score"] < 0 for w in ws)
    # the copied song loses the tie to the lower song id
    copies = dict((dst, src) for src, dst in mx.STD_COPIES)
    cut = [w for j, w in enumerate(ws) if j % 2 == 0]           # the queries cut from a song (kinds 0 and 2)
    assert all(w["song"] in copies.values() and w["score"] > 0 for w in cut)
    # edges: negative offsets, alignments past the end, -1 rows, a query without candidates
    b = bs["edges"]
    neg = past = 0
    lowest = 0
    for _, q, lab in _each(b):
        t, i = np.nonzero(lab >= 0)
        if t.size == 0:
            continue
        song = np.searchsorted(pos[:-1], lab[t, i], side="right") - 1
        off = lab[t, i] - pos[song] - t // fsm
        neg += int((off < 0).sum())
        lowest = min(lowest, int(off.min()) + (q.shape[0] - 1) // fsm)
        past += int((off + (q.shape[0] - 1) // fsm >= pos[song + 1] - pos[song]).sum())
        assert (np.diff(pos)[song] > 0).all()
    assert neg > 0 and past > 0 and lowest == 0          # offsets down to -(qlen - 1) // fsm
    assert any((lab == -1).all(1).any() and not (lab == -1).all() for _, _, lab in _each(b))
    assert any((lab == -1).any() and not (lab == -1).all(1).any() for _, _, lab in _each(b))
    none = [mx.exact_match(q, lab, rows, pos, fsm, 0) for _, q, lab in _each(b) if (lab == -1).all()]
    assert none and all(w["song"] == -1 and w["n_cand"] == 0 and w["score"] == -np.inf for w in none)
    for b_name in ("full", "collapse"):
        for _, q, lab in _each(bs[b_name]):
            for mode in (0, 1):
                n = mx.exact_match(q, lab, rows, pos, fsm, mode)["n_cand"]
                assert n == (lab.size if b_name == "full" else min(fsm, q.shape[0])), (b_name, n)


@pytest.mark.parametrize("n_songs", mx.LADDER)
def test_ladder_labels_sit_on_both_sides_of_coarse_entries(n_songs):
    db, pos, b = _ladder_batch(n_songs, 1, 40)
    ent = set(mx.coarse_entries(n_songs))
    assert n_songs < 1024 or len(ent) < n_songs
    song = np.searchsorted(pos[:-1], b.labels.ravel(), side="right") - 1
    hit = set(int(s) for s in song)
    rows_of = np.diff(pos)
    for e in (min(ent), max(e for e in ent if e < n_songs)):
        for s in (e - 1, e, e + 1):
            if 0 <= s < n_songs and rows_of[s] > 0:
                assert s in hit, (n_songs, e, s)
    lab = set(int(x) for x in b.labels.ravel())
    assert any(int(pos[s]) in lab and int(pos[s + 1] - 1) in lab for s in hit)


def test_match_plan_names_every_plan():
    # the shapes of tests/test_gpu_match_exact.py
    import test_gpu_match_exact as g
    seen = set()
    for name, nQ, max_qlen, k in g.plan_shapes():
        plan, dedup = mx.match_plan(nQ, max_qlen, k)
        assert plan == name, (name, nQ, max_qlen, k, plan)
        seen.add((plan, dedup))
    assert {p for p, _ in seen} == set(mx.PLANS)
    assert {d for _, d in seen} == {"count", "compact", "resort"}
    assert mx.match_plan(64, 1, 1024)[0] == "phased_rank" and mx.match_plan(65, 1, 1024)[0] == "single_lds"
    assert mx.match_plan(1, 1, 1023)[0] == "phased_rank" and mx.match_plan(1, 1, 512)[0] == "phased_lds"
    assert mx.match_plan(1, 2, 4096)[0] == "phased_lds" and mx.match_plan(1, 1, 8193)[0] == "phased_hbm"
    assert mx.match_plan(65, 1, 8192)[0] == "single_lds" and mx.match_plan(65, 1, 8193)[0] == "single_hbm"


@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("fsm", [1, 2])
def test_score_alpha_inputs_keep_the_oracles_gap_above_the_tolerance(fsm, d):
    """the inputs of the GPU module's score_alpha case, judged by the C oracle alone: the best song leads the runner-up by more
    than the tolerance in at least 99 % of the queries, or ties with its copy exactly (the tie queries)"""
    import test_gpu_match_exact as g
    db, pos, b, n_al = g.alpha_case(d, fsm)
    want = g.alpha_oracle(db, pos, b, fsm)
    clear = sum(1 for best, ss, gap in want[:n_al] if gap > 10 * g.ALPHA_TOL)
    assert clear * 100 >= 99 * n_al, (clear, n_al)
    copies = {dst: src for src, dst in mx.STD_COPIES}
    for best, ss, gap in want[n_al:]:
        twin = [dst for dst, src in copies.items() if src == best]
        assert twin and ss[best, 0] == ss[twin[0], 0] > 0 and gap > 10 * g.ALPHA_TOL
