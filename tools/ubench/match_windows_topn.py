"""A/B of the ranked windowed matcher: pfann_match_windows_topn's kernel (csrc/monitor.hip) against its own general path
(PFANN_WINDOWS_GENERAL=1: the windows expanded and run through pfann_match_topn -- what the library could do before the
kernel existed), same process, same inputs, same box, A/B/A/B (boxes differ by up to 9 %, tools/ubench/ab_cmd.sh).

    python tools/ubench/match_windows_topn.py [--rows 1000000] [--k 100] [--window 19] [--hops 1,2,10] [--ns 1,8,64] [--reps 5]

Database, recordings and shapes are those of tools/ubench/match_windows.py.  Prints per shape, hop and n the median
milliseconds of both paths in both rounds, the medians over both rounds, their ratio, the baseline's own run-to-run spread
(|round 1 - round 2| / median of the general path: a ratio inside 1 +- spread says nothing), the floor (pfann_match_windows,
top-1, fast path) and how many list entries differ between the two paths in (song, offset).  On real-valued rows the two
paths sum a window in different orders (include/pfann_amd.h), so neighbours in a ranking that are closer than fp32 rounding
may swap: the count is reported, not required to be 0; entry 0 of the fast path must equal pfann_match_windows bytewise."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hops", default="1,2,10")
    ap.add_argument("--ns", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
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

    def recording(L):
        rows = []
        while len(rows) < L:
            s = int(torch.randint(0, n_songs, (1,), generator=g, device=dev))
            o = int(torch.randint(0, song_rows - 60, (1,), generator=g, device=dev))
            rows += list(range(s * song_rows + o, s * song_rows + o + 60))
        r = torch.as_tensor(rows[:L], device=dev)
        return torch.nn.functional.normalize(db[r] + 0.08 * torch.randn((L, d), device=dev, generator=g), dim=1)

    shapes = [("1 x 7199 rows", [7199]), ("64 x 1199 rows", [1199] * 64)]
    hops = [int(x) for x in a.hops.split(",")]
    ns = [int(x) for x in a.ns.split(",")]

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

    print("pfann_match_windows_topn: ranked shared-dot kernel (fast) vs PFANN_WINDOWS_GENERAL=1 (general), %d db rows, k %d, "
          "window %d, %d reps after %d warm-ups, rounds A/B/A/B, median ms" % (n_rows, a.k, a.window, a.reps, a.warmup))
    print("%-16s %4s %3s %8s | %9s %10s %9s %10s | %9s %9s %7s %7s | %9s | %9s %9s" % (
        "shape", "hop", "n", "windows", "fast r1", "general r1", "fast r2", "general r2", "fast", "general", "ratio", "spread",
        "top-1 ms", "entries", "differ"))
    ok = True
    for name, rlen in shapes:
        q = torch.cat([recording(L) for L in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        _, I = idx.search(q, a.k)
        for hop in hops:
            os.environ.pop("PFANN_WINDOWS_GENERAL", None)
            floor, (res1, _) = timed(lambda: idx.match_windows(q, I, rstart, rlen, a.window, hop, to_host=False))
            res1 = idx.results_to_host(res1)
            for n in ns:
                med, tops = {}, {}
                for rnd in (1, 2):
                    for path in ("fast", "general"):
                        if path == "general":
                            os.environ["PFANN_WINDOWS_GENERAL"] = "1"
                        else:
                            os.environ.pop("PFANN_WINDOWS_GENERAL", None)
                        med[(path, rnd)], ((top, n_found), wfirst) = timed(
                            lambda: idx.match_windows_topn(q, I, rstart, rlen, a.window, hop, n, to_host=False))
                        tops[path] = idx.topn_to_host(top, n_found)[0]
                os.environ.pop("PFANN_WINDOWS_GENERAL", None)
                f = float(np.median([med[("fast", 1)], med[("fast", 2)]]))
                gm = float(np.median([med[("general", 1)], med[("general", 2)]]))
                spread = abs(med[("general", 1)] - med[("general", 2)]) / gm
                differ = int(((tops["fast"]["song"] != tops["general"]["song"]) | (tops["fast"]["offset"] != tops["general"]["offset"])).sum())
                ok &= all(np.ascontiguousarray(tops["fast"][:, 0][fld]).tobytes() == np.ascontiguousarray(res1[fld]).tobytes()
                          for fld in ("song", "offset", "shift", "score"))
                print("%-16s %4d %3d %8d | %9.3f %10.3f %9.3f %10.3f | %9.3f %9.3f %6.2fx %6.1f%% | %9.3f | %9d %9d" % (
                    name, hop, n, int(wfirst[-1]), med[("fast", 1)], med[("general", 1)], med[("fast", 2)], med[("general", 2)], f, gm,
                    gm / f, 100.0 * spread, floor, tops["fast"].size, differ))
    print("entry 0 of the fast path equals pfann_match_windows bytewise: %s" % ("yes" if ok else "NO"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
