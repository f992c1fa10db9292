"""Every call of the dense matcher, this build against another build of the library, in ONE process: same database, same
recordings, same box, rounds parent / new / parent / new.  For a change that must leave bytes and speed as they are.

    python tools/ubench/match_windows_dense_ab.py --parent-lib <libpfann_amd.so of the parent commit> [--rows 1000000]
        [--new-lib <another libpfann_amd.so>] [--window 19] [--hop 1] [--shapes 1x7199,64x1199] [--rounds 4] [--reps 5]
        [--calls dense,dense_stats,..] [--out FILE]

--parent-lib: check the parent commit out into a scratch tree, `python -m pfann_amd.build` there, pass its
pfann_amd/libpfann_amd.so.  It must already have every call timed here (the three tools match_windows_dense*.py beside this one
are for a parent that does NOT have the call they introduce).  --new-lib: time that library instead of this build's (an
experiment built in a scratch tree).

Timed: dense, dense_stats, dense_topn (n = 5) on a handle of the whole database; dense_part, dense_part_stats, dense_topn_part
(n = 5) on the first shard of a 2-way dist.shard_songs cut.  Before any timing every call runs once per shape on both libraries
(the warm-up) and every output buffer of the two must be byte-identical.

The baseline is the parent's library in the same process.  The margin is the parent's own spread, the range of its round medians:
a call PASSES when the median of the new library's round medians is not above the parent's slowest round median by more than that
range.  Exit status 1 if any call fails."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_TOP = 5
CALLS = ("dense", "dense_stats", "dense_topn", "dense_part", "dense_part_stats", "dense_topn_part")


def run_call(name, whole, shard, q, rstart, rlen, W, hop):
    """-> the call's output buffers (device tensors)"""
    if name == "dense":
        return [whole.match_windows_dense(q, rstart, rlen, W, hop, to_host=False)[0]]
    if name == "dense_stats":
        return list(whole.match_windows_dense_stats(q, rstart, rlen, W, hop, to_host=False)[0])
    if name == "dense_topn":
        return list(whole.match_windows_dense_topn(q, rstart, rlen, W, hop, N_TOP, to_host=False)[0][:2])
    if name == "dense_part":
        return [shard.match_windows_dense_part(q, rstart, rlen, W, hop)[0][0]]
    if name == "dense_part_stats":
        return list(shard.match_windows_dense_part(q, rstart, rlen, W, hop, stats=True)[0])
    if name == "dense_topn_part":
        return list(shard.match_windows_dense_topn_part(q, rstart, rlen, W, hop, N_TOP)[0])
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--new-lib", default=None)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hop", type=int, default=1)
    ap.add_argument("--shapes", default="1x7199,64x1199")
    ap.add_argument("--rounds", type=int, default=4, help="rounds per library (at least 4)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", default=",".join(CALLS))
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    assert a.rounds >= 4, "the parent's spread wants at least four rounds"
    calls = a.calls.split(",")
    assert all(c in CALLS for c in calls), "unknown call in --calls"
    import torch
    import match_windows_dense_sharded as sh
    from pfann_amd.database import DeviceIndex
    from pfann_amd.dist import shard_songs
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    db, pos = sh.world(a.rows, dev, g)
    lo, hi = shard_songs(pos, 2)[0]
    plib = sh.other_lib(a.parent_lib)
    assert hasattr(plib, "pfann_match_windows_dense_topn_part"), "--parent-lib lacks the sharded calls: not the parent commit"
    handles = {}
    nlib = sh.other_lib(a.new_lib) if a.new_lib else None
    for lib_name, make in (("parent", lambda: sh.index_of(plib, dev)),
                           ("new", lambda: sh.index_of(nlib, dev) if nlib is not None else DeviceIndex(sh.D, 0))):
        whole, shard = make(), make()
        whole.load(db, pos)
        shard.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
        handles[lib_name] = (whole, shard)

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    W, hop = a.window, a.hop
    say("dense matcher, %s (new) against the parent commit's library (parent) in one process: %d db rows, %d songs, the parts "
        "on songs [%d, %d) of a 2-way cut, window %d, hop %d, n = %d; %d rounds per library, parent / new alternating, median of %d "
        "per round, ms.  margin = the range of the parent's round medians; PASS: median(new) <= max(parent) + margin."
        % (a.new_lib or "this build", db.shape[0], len(pos) - 1, lo, hi, W, hop, N_TOP, a.rounds, a.reps))
    work = []
    for name, rlen in sh.shapes_of(a.shapes):
        q = torch.cat([sh.recording(db, n, g) for n in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        for c in calls:                                  # the warm-up of every shape, and the bytes
            outs = {k: [o.cpu().numpy().tobytes() for o in run_call(c, *handles[k], q, rstart, rlen, W, hop)] for k in handles}
            assert outs["parent"] == outs["new"], "%s, %s: the two libraries' outputs differ" % (name, c)
        work.append((name, q, rstart, rlen))
    say("every output buffer of every call is byte-identical between the two libraries on these shapes")
    say("%-16s %-16s | %-38s | %-38s | %8s %8s %9s | %s" % ("shape", "call", "parent rounds", "new rounds", "parent", "new", "new/parent",
                                                         "margin  verdict"))
    failed = 0
    for name, q, rstart, rlen in work:
        for c in calls:
            med = {"parent": [], "new": []}
            for _ in range(a.rounds):
                for k in ("parent", "new"):
                    med[k].append(sh.timed(lambda: run_call(c, *handles[k], q, rstart, rlen, W, hop), a.reps, 0)[0])
            p, n = float(np.median(med["parent"])), float(np.median(med["new"]))
            margin = max(med["parent"]) - min(med["parent"])
            ok = n <= max(med["parent"]) + margin
            failed += not ok
            say("%-16s %-16s | %-38s | %-38s | %8.3f %8.3f %8.4fx | %.3f (%.2f%%) %s"
                % (name, c, " ".join("%.3f" % x for x in med["parent"]), " ".join("%.3f" % x for x in med["new"]), p, n, n / p, margin,
                   100.0 * margin / p, "PASS" if ok else "FAIL"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
