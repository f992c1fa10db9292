"""What a database update costs against the full reload it replaces (include/pfann_amd.h: "Database updates").

    python tools/ubench/db_update.py [--rows 1000000] [--append 10000] [--remove 100] [--reps 5] [--storage f32|f16]

Database: synthetic unit-norm rows, d = 128, songs of 250 rows, in host memory.  Three things are timed, each as the median
of --reps runs in this one process (wall clock around the blocking call; every call synchronises the device itself):

    append   pfann_db_append of --append rows (songs of 250) from host memory into RESERVED capacity
    remove   pfann_db_remove_songs of --remove songs scattered evenly over the list (the move starts behind the first)
    reload   pfann_db_load of the same final rows from host memory: the cost without this feature

Every repetition starts from a fresh load of the --rows rows, so the three are timed on the same state.  Prints one table
row per storage mode and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--append", type=int, default=10000)
    ap.add_argument("--remove", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--storage", default="f32,f16")
    a = ap.parse_args()
    import torch
    from pfann_amd.database import DeviceIndex
    d, song_rows = 128, 250
    n_songs = a.rows // song_rows
    n = n_songs * song_rows
    new_songs = max(1, a.append // song_rows)
    rng = np.random.default_rng(7)
    x = rng.standard_normal((n + new_songs * song_rows, d), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    base, tail = x[:n], x[n:]
    lens = np.full(n_songs, song_rows, np.int64)
    pos = np.pad(np.cumsum(lens), (1, 0)).astype(np.int64)
    gone = np.linspace(0, n_songs - 1, a.remove).astype(np.int64)
    keep = np.ones(n, bool)
    for s in gone:
        keep[pos[s]:pos[s + 1]] = False
    final_rm = np.ascontiguousarray(base[keep])
    lens_rm = lens.copy()
    lens_rm[gone] = 0
    pos_rm = np.pad(np.cumsum(lens_rm), (1, 0)).astype(np.int64)
    out = {}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for storage in a.storage.split(","):
        t = {"append": [], "remove": [], "reload": []}
        idx = DeviceIndex(d, 0, storage=storage)
        for _ in range(a.reps + 1):                       # (the first round warms the code objects up and is dropped)
            idx.load(base, pos)
            idx.reserve(n + tail.shape[0], n_songs + new_songs)
            t["append"].append(timed(lambda: idx.append(tail, np.full(new_songs, song_rows))))
            idx.load(base, pos)
            t["remove"].append(timed(lambda: idx.remove_songs(gone)))
            t["reload"].append(timed(lambda: idx.load(final_rm, pos_rm)))
        out[storage] = {k: statistics.median(v[1:]) for k, v in t.items()}
        del idx
    print("%-8s %14s %14s %14s" % ("storage", "append ms", "remove ms", "reload ms"))
    for storage, r in out.items():
        print("%-8s %14.3f %14.3f %14.3f" % (storage, r["append"], r["remove"], r["reload"]))
    print(json.dumps({"rows": n, "d": d, "append_rows": int(tail.shape[0]), "removed_songs": int(a.remove), "reps": a.reps, "ms": out}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
