"""What `--dense` costs: pfann_match_windows_dense (csrc/dense.hip: every alignment of every window) against the nominated
pipeline on the same rows -- the search (k neighbours per row) + pfann_match_windows --, same process, same inputs, same box,
A/B/A/B (boxes differ by up to 9 %, tools/ubench/ab_cmd.sh).

    python tools/ubench/match_windows_dense.py [--rows 1000000] [--k 100] [--window 19] [--hops 1,2] [--reps 5] [--out FILE]

Database, recordings and shapes are those of tools/ubench/match_windows_topn.py.  Prints per shape and hop the median
milliseconds of both paths in both rounds, the medians over both rounds, their ratio, the baseline's own run-to-run spread
(|round 1 - round 2| / median of the nominated path), the algorithmic rate of the dense call (2 * rows * ntotal * d / t: the
product every window's answer is defined on, not the halo the tiles compute twice) and its fraction of the 157.3 TFLOP/s
fp32 MFMA peak, a CRC of both paths' decisions (song, offset) and the number of windows where they differ.  The dense
matcher does strictly more work than the nominated path; the table states the cost, it is not a race."""
import argparse
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
PEAK_TF = 157.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hops", default="1,2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the table to this file")
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

    say("pfann_match_windows_dense (dense) vs search k=%d + pfann_match_windows (nominated), %d db rows, window %d, %d reps after "
        "%d warm-ups, rounds A/B/A/B, median ms" % (a.k, n_rows, a.window, a.reps, a.warmup))
    say("%-16s %4s %8s | %9s %12s %9s %12s | %9s %10s %7s %7s | %8s %6s | %8s %8s %7s" % (
        "shape", "hop", "windows", "dense r1", "nominated r1", "dense r2", "nominated r2", "dense", "nominated", "ratio", "spread",
        "TFLOP/s", "peak", "crc dense", "crc nom", "differ"))
    crc = lambda r: zlib.crc32(np.ascontiguousarray(r["song"]).tobytes() + np.ascontiguousarray(r["offset"]).tobytes()) & 0xFFFFFFFF
    for name, rlen in shapes:
        q = torch.cat([recording(L) for L in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])

        def nominated(hop):
            _, I = idx.search(q, a.k)
            return idx.match_windows(q, I, rstart, rlen, a.window, hop, to_host=False)

        for hop in hops:
            med, out = {}, {}
            for rnd in (1, 2):
                med[("dense", rnd)], (res, wfirst) = timed(lambda: idx.match_windows_dense(q, rstart, rlen, a.window, hop, to_host=False))
                out["dense"] = idx.results_to_host(res)
                med[("nom", rnd)], (res, _) = timed(lambda: nominated(hop))
                out["nom"] = idx.results_to_host(res)
            dm = float(np.median([med[("dense", 1)], med[("dense", 2)]]))
            nm = float(np.median([med[("nom", 1)], med[("nom", 2)]]))
            spread = abs(med[("nom", 1)] - med[("nom", 2)]) / nm
            tf = 2.0 * q.shape[0] * n_rows * d / (dm * 1e-3) / 1e12
            differ = int(((out["dense"]["song"] != out["nom"]["song"]) | (out["dense"]["offset"] != out["nom"]["offset"])).sum())
            say("%-16s %4d %8d | %9.3f %12.3f %9.3f %12.3f | %9.3f %10.3f %6.2fx %6.1f%% | %8.2f %5.1f%% | %08x %08x %7d" % (
                name, hop, int(wfirst[-1]), med[("dense", 1)], med[("nom", 1)], med[("dense", 2)], med[("nom", 2)], dm, nm, dm / nm,
                100.0 * spread, tf, 100.0 * tf / PEAK_TF, crc(out["dense"]), crc(out["nom"]), differ))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
