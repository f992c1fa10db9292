"""What the row mask of pfann_search_topk_excl costs: pfann_search_topk against pfann_search_topk_excl with self-match-shaped
ranges -- 1,000,000 unit rows at d = 128 in songs of 59 rows (the bench database's average), the queries are consecutive
database rows and every row leaves its own song out -- for 19 query rows (the streaming path) and 9728 (one launch group).
A/B/A/B in ONE process on one box (boxes differ by up to 9 %): the yardstick is the plain call of the same run.  Also
timed: the masked call with every range empty (the mask's fixed cost: one range kernel, the per-tile tests).
    python tools/ubench/search_excl.py [rounds]        -> one line per shape, and a JSON line"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from pfann_amd.database import DeviceIndex                     # noqa: E402

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 4
d, n, k, SONG = 128, 1000000, 100, 59
g = torch.Generator(device="cuda")
g.manual_seed(5)
db = torch.randn((n, d), device="cuda", generator=g)
heads = db[::SONG].repeat_interleave(SONG, 0)[:n]
db = heads + 0.6 * db
db = (db / db.norm(dim=1, keepdim=True)).contiguous()
ix = DeviceIndex(d, 0)
ix.load(db, np.array([0, n], np.int64), 0)


def timeit(f, reps):
    f()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t) / reps


out = []
for nq, reps in ((19, 200), (9728, 10)):
    rows = torch.arange(nq, device="cuda") + 59 * 4000
    q = db[rows].contiguous()
    lo = (rows // SONG) * SONG
    hi = torch.clamp(lo + SONG, max=n)
    none = torch.zeros_like(lo)
    path = ix.search_plan(nq, k)[1]["path"]
    assert ix.search_plan(nq, k, excl=True)[1]["path"] == path
    D, I = ix.search(q, k, exclude=(lo, hi))
    assert not ((I >= lo[:, None]) & (I < hi[:, None])).any() and (I >= 0).all()
    a, b, c = [], [], []
    for _ in range(ROUNDS):
        a.append(timeit(lambda: ix.search(q, k), reps))
        b.append(timeit(lambda: ix.search(q, k, exclude=(lo, hi)), reps))
        c.append(timeit(lambda: ix.search(q, k, exclude=(none, none)), reps))
    ma, mb, mc = float(np.median(a)), float(np.median(b)), float(np.median(c))
    print("%5d x %d rows, k %d, path %s: plain %.4f ms, own song excluded %.4f ms (x %.3f), empty ranges %.4f ms (x %.3f)   rounds plain %s masked %s"
          % (nq, n, k, path, ma, mb, mb / ma, mc, mc / ma, ["%.4f" % x for x in a], ["%.4f" % x for x in b]))
    out.append({"nq": nq, "n": n, "d": d, "k": k, "path": path, "plain_ms": ma, "masked_ms": mb, "ratio": mb / ma, "empty_ranges_ms": mc,
                "plain_rounds_ms": a, "masked_rounds_ms": b})
print(json.dumps({"search_excl": out}))
