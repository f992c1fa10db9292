"""A/B of the windowed matcher: pfann_match_windows' shared-dot kernel (csrc/monitor.hip) against its own general path
(PFANN_WINDOWS_GENERAL=1: the existing matcher on the expanded, overlapping windows -- what the library could do before the
kernel existed), same process, same inputs, same box, A/B/A/B (boxes differ by up to 9 %, tools/ubench/ab_cmd.sh).

    python tools/ubench/match_windows.py [--rows 1000000] [--k 100] [--window 19] [--hops 1,2,10] [--reps 10]

Database: synthetic unit-norm rows (songs of 250 rows) on the device.  Recordings: consecutive excerpts of random songs with
noise added, so every row's top-k holds its true alignment among chance neighbours, as real traffic does.  Shapes: one
one-hour recording (7199 rows) and 64 ten-minute recordings (1199 rows each).  Prints per shape and hop the median
milliseconds of both paths over both rounds, their ratio, a CRC of all decisions (song, offset) of each path -- the two
must be equal -- and the search time for the same rows."""
import argparse
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hops", default="1,2,10")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch
    from pfann_amd.database import DeviceIndex
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    d, song_rows = 128, 250
    n_songs = a.rows // song_rows
    n = n_songs * song_rows
    db = torch.nn.functional.normalize(torch.randn((n, d), device=dev, generator=g), dim=1)
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
        return ts, out

    print("pfann_match_windows: shared-dot kernel (fast) vs PFANN_WINDOWS_GENERAL=1 (general), %d db rows, k %d, window %d, "
          "%d reps after %d warm-ups, rounds A/B/A/B, median ms" % (n, a.k, a.window, a.reps, a.warmup))
    print("%-16s %4s %8s | %9s %9s %9s %9s | %9s %9s %7s | %10s %10s | %9s" % (
        "shape", "hop", "windows", "fast r1", "general r1", "fast r2", "general r2", "fast", "general", "ratio", "crc fast", "crc general", "search ms"))
    ok = True
    for name, rlen in shapes:
        q = torch.cat([recording(L) for L in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        ts_search, (_, I) = timed(lambda: idx.search(q, a.k))
        for hop in hops:
            med, crc, nw = {}, {}, 0
            for rnd in (1, 2):
                for path in ("fast", "general"):
                    if path == "general":
                        os.environ["PFANN_WINDOWS_GENERAL"] = "1"
                    else:
                        os.environ.pop("PFANN_WINDOWS_GENERAL", None)
                    ts, (res, wfirst) = timed(lambda: idx.match_windows(q, I, rstart, rlen, a.window, hop, to_host=False))
                    res = idx.results_to_host(res)
                    med[(path, rnd)] = float(np.median(ts))
                    crc[path] = zlib.crc32(res["song"].tobytes() + res["offset"].tobytes())
                    nw = int(wfirst[-1])
            os.environ.pop("PFANN_WINDOWS_GENERAL", None)
            f = float(np.median([med[("fast", 1)], med[("fast", 2)]]))
            gm = float(np.median([med[("general", 1)], med[("general", 2)]]))
            ok &= crc["fast"] == crc["general"]
            print("%-16s %4d %8d | %9.3f %9.3f %9.3f %9.3f | %9.3f %9.3f %6.2fx |   %08x    %08x | %9.3f" % (
                name, hop, nw, med[("fast", 1)], med[("general", 1)], med[("fast", 2)], med[("general", 2)], f, gm, gm / f,
                crc["fast"], crc["general"], float(np.median(ts_search))))
    print("decisions of both paths equal: %s" % ("yes" if ok else "NO"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
