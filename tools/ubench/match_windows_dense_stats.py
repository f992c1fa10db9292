"""What the background statistics cost: pfann_match_windows_dense_stats against pfann_match_windows_dense -- the same tile kernel
without the moments -- on the same rows, same process, same box, A/B/A/B.

    python tools/ubench/match_windows_dense_stats.py [--parent-lib libpfann_amd.so of the parent commit] [--rows 1000000]
        [--window 19] [--hops 1,2] [--reps 5] [--out FILE]

--parent-lib: a build of the commit BEFORE the statistics call (check it out into a scratch tree, `python -m pfann_amd.build` there,
pass its pfann_amd/libpfann_amd.so).  It is loaded beside this build's library and given the same database; its
pfann_match_windows_dense is the baseline ("parent"), and this build's pfann_match_windows_dense ("plain") is timed in the same
rounds: the plain entry point must not get slower, i.e. lie within the spread of the two parent rounds.  Without --parent-lib
the baseline is this build's plain call.

Database, recordings and shapes are those of tools/ubench/match_windows_dense.py.  Prints per shape and hop the median
milliseconds of every path in both rounds, the medians over both rounds, the ratios to the baseline, the baseline's own
run-to-run spread (|round 1 - round 2| / median), and per-tag event times of one profiled call of each kind (pfann_prof_*).
The statistics call's results are checked against the plain answer, and its counts against the song lengths."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hops", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="1x7199,64x1199")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from pfann_amd import lib as L
    from pfann_amd.database import DeviceIndex
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    d, song_rows = 128, 250
    n_songs = a.rows // song_rows
    n_rows = n_songs * song_rows
    db = torch.nn.functional.normalize(torch.randn((n_rows, d), device=dev, generator=g), dim=1)
    pos = np.arange(n_songs + 1, dtype=np.int64) * song_rows
    idx = DeviceIndex(d, 0)
    idx.load(db, pos)
    lib = L.load()

    parent = None
    if a.parent_lib:
        plib = ctypes.CDLL(os.path.abspath(a.parent_lib))
        assert not hasattr(plib, "pfann_match_windows_dense_stats"), "--parent-lib already has the statistics call: not the parent commit"
        for name, (res, args) in L.SYMBOLS.items():
            if hasattr(plib, name):
                fn = getattr(plib, name)
                fn.restype, fn.argtypes = res, args

        class ParentIndex(DeviceIndex):
            def __init__(self):
                self.lib, self.d, self.device = plib, d, dev
                self.handle = plib.pfann_db_create(d, 0)
                assert self.handle and plib.pfann_db_set_storage(self.handle, 0) == 0
                self.storage, self.ntotal, self.label_base, self.n_songs = "f32", 0, 0, 0
                self._small_args, self._prefilter, self._host_res = {}, True, None
        parent = ParentIndex()
        parent.load(db, pos)

    def recording(n):
        rows = []
        while len(rows) < n:
            s = int(torch.randint(0, n_songs, (1,), generator=g, device=dev))
            o = int(torch.randint(0, song_rows - 60, (1,), generator=g, device=dev))
            rows += list(range(s * song_rows + o, s * song_rows + o + 60))
        r = torch.as_tensor(rows[:n], device=dev)
        return torch.nn.functional.normalize(db[r] + 0.08 * torch.randn((n, d), device=dev, generator=g), dim=1)

    shapes = []
    for spec in a.shapes.split(","):
        nrec, rows = (int(x) for x in spec.split("x"))
        shapes.append(("%d x %d rows" % (nrec, rows), [rows] * nrec))
    hops = [int(x) for x in a.hops.split(",")]

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return float(np.median(ts)), out

    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("pfann_match_windows_dense_stats (stats) vs pfann_match_windows_dense of %s (baseline) and of this build (plain), "
        "%d db rows, %d songs, window %d, %d reps after %d warm-ups, rounds A/B/A/B, median ms"
        % ("the parent commit's library" if parent is not None else "this build", n_rows, n_songs, a.window, a.reps, a.warmup))
    paths = ["baseline", "plain", "stats"]
    say("%-16s %4s %8s | %s | %s | %10s %10s | %7s" % (
        "shape", "hop", "windows", " ".join("%12s" % (p + " r1") for p in paths) + " " + " ".join("%12s" % (p + " r2") for p in paths),
        " ".join("%12s" % p for p in paths), "plain/base", "stats/base", "spread"))
    profile = []
    for name, rlen in shapes:
        q = torch.cat([recording(n) for n in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        for hop in hops:
            fns = {
                "baseline": lambda: (parent if parent is not None else idx).match_windows_dense(q, rstart, rlen, a.window, hop, to_host=False),
                "plain": lambda: idx.match_windows_dense(q, rstart, rlen, a.window, hop, to_host=False),
                "stats": lambda: idx.match_windows_dense_stats(q, rstart, rlen, a.window, hop, to_host=False),
            }
            med, out = {}, {}
            for rnd in (1, 2):
                for p in paths:
                    med[(p, rnd)], out[p] = timed(fns[p])
            m = {p: float(np.median([med[(p, 1)], med[(p, 2)]])) for p in paths}
            spread = abs(med[("baseline", 1)] - med[("baseline", 2)]) / m["baseline"]
            wfirst = out["plain"][1]
            base = idx.results_to_host(out["baseline"][0])
            plain = idx.results_to_host(out["plain"][0])
            with_stats = idx.results_to_host(out["stats"][0][0])
            stats = idx.stats_to_host(out["stats"][0][1])
            assert base.tobytes() == plain.tobytes(), "the plain call answers differently from the baseline"
            assert with_stats.tobytes() == plain.tobytes(), "the statistics call's results are not the plain answer"
            assert (stats["n_full"] == n_songs * (song_rows - a.window + 1)).all() and (stats["sumsq_q"] > 0).all(), "the counts are off"
            say("%-16s %4d %8d | %s | %s | %9.3fx %9.3fx | %6.1f%%" % (
                name, hop, int(wfirst[-1]), " ".join("%12.3f" % med[(p, r)] for r in (1, 2) for p in paths),
                " ".join("%12.3f" % m[p] for p in paths), m["plain"] / m["baseline"], m["stats"] / m["baseline"], 100.0 * spread))
            # one profiled call each: the tile kernel with and without the moments
            lib.pfann_prof_enable(1)
            for p in ("plain", "stats"):
                lib.pfann_prof_reset()
                fns[p]()
                torch.cuda.synchronize()
                parts = []
                for tag in (b"seq_match_windows_dense", b"seq_match_windows_dense_stats"):
                    cnt = ctypes.c_int64(0)
                    ms = lib.pfann_prof_elapsed_ms(tag, ctypes.byref(cnt))
                    if cnt.value:
                        parts.append("%s %.3f ms in %d launches" % (tag.decode(), ms, cnt.value))
                profile.append("%-16s hop %d %-13s %s" % (name, hop, p + ":", "; ".join(parts)))
            lib.pfann_prof_enable(0)
    say("per-tag event times of one profiled call (launches run back to back; the tags bracket single kernels):")
    for s in profile:
        say(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
