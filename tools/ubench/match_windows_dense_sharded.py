"""What song sharding buys the dense matcher, as a ONE-GPU kernel-time model: every shard's part alone, plus the merge, against
the whole-handle call -- same rows, same process, same box, A/B/A/B.

    python tools/ubench/match_windows_dense_sharded.py [--parent-lib libpfann_amd.so of the parent commit] [--rows 1000000]
        [--window 19] [--hop 1] [--shards 2,4,8] [--reps 5] [--out FILE]

--parent-lib: a build of the commit BEFORE the sharded calls (check it out into a scratch tree, `python -m pfann_amd.build` there,
pass its pfann_amd/libpfann_amd.so).  It is loaded beside this build's library and given the same database; its
pfann_match_windows_dense is the baseline ("parent"), and this build's pfann_match_windows_dense ("whole") is timed in the same
rounds: the existing entry point must not get slower, i.e. lie within the spread of the two parent rounds.  Without
--parent-lib the baseline is this build's whole-handle call.

For 2 / 4 / 8 shards (dist.shard_songs) every shard is a handle of its own on this GPU; each part
(pfann_match_windows_dense_part) is timed ALONE, then the merge (pfann_match_windows_dense_merge) of all parts' words.  A rank's
time in an N-GPU job is modelled as the slowest part plus the merge.  By construction a part runs ceil((n_r + W-1) / SI) column
tiles of the whole call's ceil((N + W-1) / SI), SI = 128 - (W-1): that ratio is printed beside the measured one.

This is a kernel-time model on one GPU.  The all-gather of the words (8 bytes per window and rank) is NOT in it: nothing here
is measured over xGMI.  The merged results are checked against the whole-handle bytes."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


D, SONG_ROWS = 128, 250


def world(rows, dev, g):
    """-> (db [n_rows, D] unit rows on the device, song_pos): songs of SONG_ROWS rows"""
    import torch
    n_songs = rows // SONG_ROWS
    db = torch.nn.functional.normalize(torch.randn((n_songs * SONG_ROWS, D), device=dev, generator=g), dim=1)
    return db, np.arange(n_songs + 1, dtype=np.int64) * SONG_ROWS


def other_lib(path):
    """another build's libpfann_amd.so, loaded beside this build's, with the prototypes of the calls it has"""
    from pfann_amd import lib as L
    plib = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in L.SYMBOLS.items():
        if hasattr(plib, name):
            fn = getattr(plib, name)
            fn.restype, fn.argtypes = res, args
    return plib


def index_of(plib, dev):
    """an empty fp32 DeviceIndex whose calls go to plib"""
    from pfann_amd.database import DeviceIndex

    class OtherIndex(DeviceIndex):
        def __init__(self):
            self.lib, self.d, self.device = plib, D, dev
            self.handle = plib.pfann_db_create(D, 0)
            assert self.handle and plib.pfann_db_set_storage(self.handle, 0) == 0
            self.storage, self.ntotal, self.label_base, self.n_songs = "f32", 0, 0, 0
            self._small_args, self._prefilter, self._host_res = {}, True, None
    return OtherIndex()


def recording(db, n, g):
    """n noisy rows: stretches of 60 consecutive rows of random songs"""
    import torch
    dev, n_songs = db.device, db.shape[0] // SONG_ROWS
    rows = []
    while len(rows) < n:
        s = int(torch.randint(0, n_songs, (1,), generator=g, device=dev))
        o = int(torch.randint(0, SONG_ROWS - 60, (1,), generator=g, device=dev))
        rows += list(range(s * SONG_ROWS + o, s * SONG_ROWS + o + 60))
    r = torch.as_tensor(rows[:n], device=dev)
    return torch.nn.functional.normalize(db[r] + 0.08 * torch.randn((n, D), device=dev, generator=g), dim=1)


def shapes_of(spec):
    """"1x7199,64x1199" -> [(name, rlen)]"""
    shapes = []
    for one in spec.split(","):
        nrec, rows = (int(x) for x in one.split("x"))
        shapes.append(("%d x %d rows" % (nrec, rows), [rows] * nrec))
    return shapes


def timed(fn, reps, warmup):
    """-> (median ms of reps runs after warmup runs, the last run's value)"""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hop", type=int, default=1)
    ap.add_argument("--shards", default="2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="1x7199,64x1199")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    a = ap.parse_args()
    import torch
    from pfann_amd.database import DeviceIndex
    from pfann_amd.dist import shard_songs
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    d = D
    db, pos = world(a.rows, dev, g)
    n_rows, n_songs = int(db.shape[0]), len(pos) - 1
    idx = DeviceIndex(d, 0)
    idx.load(db, pos)

    parent = None
    if a.parent_lib:
        plib = other_lib(a.parent_lib)
        assert not hasattr(plib, "pfann_match_windows_dense_part"), "--parent-lib already has the sharded calls: not the parent commit"
        parent = index_of(plib, dev)
        parent.load(db, pos)

    sharded = {}
    for G in (int(x) for x in a.shards.split(",")):
        handles = []
        for lo, hi in shard_songs(pos, G):
            ix = DeviceIndex(d, 0)
            ix.load(db[pos[lo]:pos[hi]], pos, int(pos[lo]), song_range=(lo, hi))
            handles.append(ix)
        sharded[G] = handles

    shapes = shapes_of(a.shapes)
    run = lambda fn: timed(fn, a.reps, a.warmup)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    W, hop = a.window, a.hop
    SI = 128 - (W - 1)
    tiles = lambda n: -(-(n + W - 1) // SI)
    say("song-sharded dense matcher, one-GPU kernel-time model: every part alone + the merge vs pfann_match_windows_dense of %s "
        "(baseline) and of this build (whole); %d db rows, %d songs, window %d, hop %d, %d reps after %d warm-ups, rounds A/B/A/B, "
        "median ms.  Nothing here is measured over xGMI: the all-gather of the words is not in the model."
        % ("the parent commit's library" if parent is not None else "this build", n_rows, n_songs, W, hop, a.reps, a.warmup))
    for name, rlen in shapes:
        q = torch.cat([recording(db, n, g) for n in rlen])
        rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
        base_ix = parent if parent is not None else idx
        fns = {"baseline": lambda: base_ix.match_windows_dense(q, rstart, rlen, W, hop, to_host=False),
               "whole": lambda: idx.match_windows_dense(q, rstart, rlen, W, hop, to_host=False)}
        med, out = {}, {}
        part_ms = {G: [[] for _ in hs] for G, hs in sharded.items()}
        merge_ms = {G: [] for G in sharded}
        for rnd in (1, 2):
            for p in ("baseline", "whole"):
                med[(p, rnd)], out[p] = run(fns[p])
            for G, hs in sharded.items():
                words = []
                for r, ix in enumerate(hs):
                    ms, ((w, _), _) = run(lambda ix=ix: ix.match_windows_dense_part(q, rstart, rlen, W, hop))
                    part_ms[G][r].append(ms)
                    words.append(w)
                allw = torch.stack(words)
                ms, (res, _) = run(lambda: idx.dense_merge(allw, None, rlen, W, hop))
                merge_ms[G].append(ms)
                assert res.cpu().numpy().tobytes() == out["whole"][0].cpu().numpy().tobytes(), "%d shards: the merge is not the whole answer" % G
        assert out["baseline"][0].cpu().numpy().tobytes() == out["whole"][0].cpu().numpy().tobytes(), "whole answers differently from the baseline"
        m = {p: float(np.median([med[(p, 1)], med[(p, 2)]])) for p in ("baseline", "whole")}
        spread = abs(med[("baseline", 1)] - med[("baseline", 2)]) / m["baseline"]
        say("%s, %d windows: baseline r1 %.3f r2 %.3f (median %.3f, spread %.1f%%); whole r1 %.3f r2 %.3f (median %.3f, %.3fx baseline)"
            % (name, int(out["whole"][1][-1]), med[("baseline", 1)], med[("baseline", 2)], m["baseline"], 100.0 * spread,
               med[("whole", 1)], med[("whole", 2)], m["whole"], m["whole"] / m["baseline"]))
        say("  %6s | %12s %12s %10s | %12s | %10s %10s | %s" % ("shards", "slowest part", "fastest part", "merge", "rank = s + m",
                                                             "rank/base", "tile ratio", "parts (median of both rounds)"))
        for G, hs in sharded.items():
            parts = [float(np.median(x)) for x in part_ms[G]]
            mg = float(np.median(merge_ms[G]))
            rank = max(parts) + mg
            ratio = max(tiles(ix.ntotal) for ix in hs) / tiles(n_rows)
            say("  %6d | %12.3f %12.3f %10.3f | %12.3f | %9.3fx %9.3fx | %s" % (G, max(parts), min(parts), mg, rank, rank / m["baseline"],
                                                                              ratio, " ".join("%.3f" % x for x in parts)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
