"""The merge of the song-sharded dense matcher is exact: tests/dense_shard_cases.py -- per shard the best (total, id) word among
its own songs' candidates, its own integer sums and its own ranked songs; then the maximum word, the sums and the ranked merge --
gives, for every cut of the song list, ==, what the whole-database oracles give.  CPU only; the GPU tests compare the kernels
with the same functions."""
import numpy as np
import pytest

import dense_cases as dc
import dense_shard_cases as sh
import dense_stats_cases as ds
import dense_topn_cases as dt

WINDOWS, HOPS, N_TOP = (1, 5, 19), (1, 3), (1, 5, 64)


def _whole(q, db, pos, window, hop, rstart, rlen, n, excl, key):
    return (dc.dense_oracle(q, db, pos, window, hop, rstart, rlen, excl=excl, key=key),
            ds.stats_oracle(q, db, pos, window, hop, rstart, rlen, excl=excl, key=key),
            dt.dense_topn_oracle(q, db, pos, window, hop, rstart, rlen, n, excl=excl, key=key))


def test_the_cuts_are_cuts():
    db, pos, q, rstart, rlen = dc.small_world()
    cuts = sh.cuts_of(pos)
    pos_x, more = sh.with_rowless_tail(pos)
    for name, cut, p in [(k, v, pos) for k, v in cuts.items()] + [(k, v, pos_x) for k, v in more.items()]:
        assert cut[0][0] == 0 and cut[-1][1] == len(p) - 1 and all(a[1] == b[0] for a, b in zip(cut, cut[1:])), name
    assert len(cuts["8"]) == 8 and len(cuts["first"]) == 2
    lo, hi = cuts["first"][0]
    assert 0 < pos[hi] - pos[lo] < 18, "the first shard holds fewer rows than a window of 19 has, less one"
    assert all(pos_x[hi] == pos_x[lo] for lo, hi in (more["rowless-right"][1], more["rowless-left"][1]))
    assert more["rowless-left"][1][0] == more["rowless-left"][1][1]      # no song at all


@pytest.mark.parametrize("window", WINDOWS)
def test_every_cut_merges_to_the_whole_database(window):
    db, pos, q, rstart, rlen = dc.small_world()
    pos_x, more = sh.with_rowless_tail(pos)
    cases = [(name, cut, pos, "small") for name, cut in sh.cuts_of(pos).items()]
    cases += [(name, cut, pos_x, "small-x") for name, cut in more.items()]
    for hop in HOPS:
        for n in N_TOP:
            for name, cut, p, key in cases:
                whole = _whole(q, db, p, window, hop, rstart, rlen, n, None, key)
                got = sh.sharded_oracle(q, db, p, window, hop, rstart, rlen, cut, n, key="small")
                bad = sh.against_whole(got, *whole)
                assert not bad and len(got) > 0, "cut %s window %d hop %d n %d: %d of %d windows differ\n%s" % (
                    name, window, hop, n, len(bad), len(got), "\n".join(bad[:6]))
                if n == 5 and hop == 1:
                    assert sh.sharded_oracle(q, db, p, window, hop, rstart, rlen, cut, n, key="small", reverse=True) == got


def test_exclusion_in_and_outside_the_winners_shard():
    """a recording's excluded song is no candidate of any part, and leaves n_cand and n_found as the whole database counts them"""
    db, pos, q, rstart, rlen = dc.small_world()
    pos_x, more = sh.with_rowless_tail(pos)
    window, hop, n = 19, 2, 5
    plain = dc.dense_oracle(q, db, pos, window, hop, rstart, rlen, key="small")
    winner = int(plain[0]["song"])
    cut = sh.cuts_of(pos)["3"]
    other = next(s for lo, hi in cut if not lo <= winner < hi for s in range(lo, hi) if pos[s + 1] > pos[s])
    rowless = len(pos_x) - 2
    for what, ex in (("winner", winner), ("other shard", other), ("rowless", rowless)):
        excl = [ex] * len(rlen)
        for name, c in list(sh.cuts_of(pos_x).items()) + list(more.items()):
            whole = _whole(q, db, pos_x, window, hop, rstart, rlen, n, excl, "small-x")
            got = sh.sharded_oracle(q, db, pos_x, window, hop, rstart, rlen, c, n, excl=excl, key="small")
            bad = sh.against_whole(got, *whole)
            assert not bad, "excluded %s, cut %s: %d windows differ\n%s" % (what, name, len(bad), "\n".join(bad[:6]))
    assert dc.dense_oracle(q, db, pos_x, window, hop, rstart, rlen, excl=[winner] * len(rlen), key="small-x")[0]["song"] != winner


def test_the_ranked_merge_order_is_the_word_order():
    """score = (double)total / (double)n is injective on float32 totals for n <= 64: neighbouring float32 totals give different
    float64 scores for every divisor the matcher uses, so ranking merged entries by (score, song) is ranking words"""
    rng = np.random.default_rng(5)
    t = np.concatenate([rng.standard_normal(4000).astype(np.float32) * 64, np.float32([1.0, 2.0 ** -20, 63.999996, 2.0 ** -126])])
    up = np.nextafter(t, np.float32(np.inf))
    for n in range(1, 65):
        assert (t.astype(np.float64) / n < up.astype(np.float64) / n).all(), n
