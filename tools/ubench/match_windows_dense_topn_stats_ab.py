"""The ranked dense matcher with statistics in ONE pass (pfann_match_windows_dense_topn_stats) against the pair of calls that
gives the same outputs without it, pfann_match_windows_dense_topn and then pfann_match_windows_dense_stats on the same stream:
one process, one database, one box, rounds pair / one pass / pair / one pass.

    python tools/ubench/match_windows_dense_topn_stats_ab.py [--rows 1000000] [--window 19] [--hop 1] [--n 5]
        [--shapes 1x7199,64x1199] [--rounds 4] [--reps 5] [--out FILE]

Before any timing both forms run once per shape (the warm-up, which also sizes the ranked workspace) and the bytes are compared:
top and n_found of the one pass against pfann_match_windows_dense_topn's, its statistics against pfann_match_windows_dense_stats'.
Also timed, in the same rounds, are the two calls of the pair alone.

The one pass exists to be cheaper than the pair.  The verdict uses the pair's own spread, the range of its round medians: CHEAPER
when the median of the one pass's round medians is below the pair's fastest round by more than that range, NOT CHEAPER otherwise.
The exit status is 0 either way: this is a record, not a gate."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hop", type=int, default=1)
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--shapes", default="1x7199,64x1199")
    ap.add_argument("--rounds", type=int, default=4, help="rounds per form (at least 4)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert a.rounds >= 4, "the pair's spread wants at least four rounds"
    import torch
    import match_windows_dense_sharded as sh
    from pfann_amd.database import DeviceIndex
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    db, pos = sh.world(a.rows, dev, g)
    idx = DeviceIndex(sh.D, 0)
    idx.load(db, pos)
    W, hop, n = a.window, a.hop, a.n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("ranked dense matcher with statistics: pfann_match_windows_dense_topn_stats (one pass) against pfann_match_windows_dense_topn "
        "+ pfann_match_windows_dense_stats issued one after the other (pair), one process: %d db rows, %d songs, window %d, hop %d, "
        "n = %d; %d rounds per form, pair / one pass alternating, median of %d per round, ms.  margin = the range of the pair's round "
        "medians; CHEAPER: median(one pass) < min(pair) - margin." % (db.shape[0], len(pos) - 1, W, hop, n, a.rounds, a.reps))
    say("%-16s | %-34s | %-34s | %8s %8s %9s | %-18s | %s" % ("shape", "pair rounds", "one pass rounds", "pair", "one pass", "one/pair",
                                                          "topn / stats alone", "margin  verdict"))
    for name, rlen in sh.shapes_of(a.shapes):
        q = torch.cat([sh.recording(db, m, g) for m in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        topn = lambda: idx.match_windows_dense_topn(q, rstart, rlen, W, hop, n, to_host=False)[0]
        stats = lambda: idx.match_windows_dense_stats(q, rstart, rlen, W, hop, to_host=False)[0]
        one = lambda: idx.match_windows_dense_topn_stats(q, rstart, rlen, W, hop, n, to_host=False)[0]
        pair = lambda: (topn(), stats())
        (t0, f0, _), (_, s0) = pair()                      # the warm-up of both forms, and the bytes
        t1, f1, _, s1 = one()
        same = lambda x, y: x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()
        assert same(t0, t1) and same(f0, f1), "%s: the one pass ranks differently from pfann_match_windows_dense_topn" % name
        assert same(s0, s1), "%s: the one pass counts differently from pfann_match_windows_dense_stats" % name
        med = {"pair": [], "one": [], "topn": [], "stats": []}
        for _ in range(a.rounds):
            for k, fn in (("pair", pair), ("one", one), ("topn", topn), ("stats", stats)):
                med[k].append(sh.timed(fn, a.reps, 0)[0])
        p, o = float(np.median(med["pair"])), float(np.median(med["one"]))
        margin = max(med["pair"]) - min(med["pair"])
        cheaper = o < min(med["pair"]) - margin
        say("%-16s | %-34s | %-34s | %8.3f %8.3f %8.4fx | %8.3f %8.3f | %.3f (%.2f%%) %s"
            % (name, " ".join("%.3f" % x for x in med["pair"]), " ".join("%.3f" % x for x in med["one"]), p, o, o / p,
               float(np.median(med["topn"])), float(np.median(med["stats"])), margin, 100.0 * margin / p,
               "CHEAPER" if cheaper else "NOT CHEAPER"))
    say("the one pass's top and n_found are byte-identical to pfann_match_windows_dense_topn's and its statistics to "
        "pfann_match_windows_dense_stats' on these shapes")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
