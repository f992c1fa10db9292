"""What a ranked list costs, at the bench shape (4096 queries x 19 rows, k = 100, 16,950 songs, fp32 storage):
  (a) pfann_match without the per-song block                                  -- the floor: top-N cannot be cheaper
  (b) pfann_match with the block + its zeroing + song_scores_to_seconds + the device-to-host copy of the block
                                                                              -- what a ranked list cost before pfann_match_topn
  (c) pfann_match_topn at n = 10 + the copy of its lists
One line per leg: `leg ms-per-call (median of REPS) min max`.  (a) and (b) run on any build of the library, (c) is skipped
when the library has no pfann_match_topn, so tools/ubench/ab_cmd.sh can alternate this command between two builds.
    python tools/ubench/match_topn.py [nQ] [n] [reps]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

from pfann_amd.database import DeviceIndex

nQ = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
n_songs, seg, d, k, ql = 16950, 59, 128, 100, 19
n = n_songs * seg
g = torch.Generator(device="cuda")
g.manual_seed(1)
db = torch.randn((n, d), device="cuda", generator=g)
db /= db.norm(dim=1, keepdim=True)
pos = np.arange(n_songs + 1, dtype=np.int64) * seg
idx = DeviceIndex(d, 0)
idx.load(db, pos, 0)
src = (torch.arange(nQ, device="cuda") * 1931 + 7) % (n - 40)
rows = (src[:, None] + torch.arange(ql, device="cuda")[None, :]).reshape(-1)
q = db[rows] + 0.7 * torch.randn((nQ * ql, d), device="cuda", generator=g)
q /= q.norm(dim=1, keepdim=True)
I = torch.cat([idx.search(q[i:i + 16384], k)[1] for i in range(0, q.shape[0], 16384)])
qs, qn = np.arange(nQ, dtype=np.int64) * ql, np.full(nQ, ql, np.int32)
land = torch.empty((nQ, n_songs, 2), dtype=torch.float32, pin_memory=True)


def leg_a():
    res, _ = idx.match(q, I, qs, qn, 1, 0.0, 0, False, False, to_host=False)
    return idx.results_to_host(res)


def leg_b():
    res, ss = idx.match(q, I, qs, qn, 1, 0.0, 0, False, True, to_host=False)        # (match zeroes the block it allocates)
    idx.song_scores_to_seconds(ss, 1, 0.5)
    land.copy_(ss, non_blocking=True)
    return idx.results_to_host(res)


def leg_c():
    return idx.match_topn(q, I, qs, qn, N, 1, 0.0, 0)


def timed(fn):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


legs = [("a match", leg_a), ("b match+block+copy", leg_b)]
if hasattr(idx, "match_topn") and hasattr(idx.lib, "pfann_match_topn"):
    legs.append(("c match_topn n=%d" % N, leg_c))
for name, fn in legs:
    print("%-22s nQ=%d  %.3f ms  (min %.3f max %.3f, %d reps)" % ((name, nQ) + timed(fn) + (REPS,)), flush=True)
if len(legs) == 3:
    top, nf = leg_c()
    res = leg_a()
    same = all((top[:, 0][f] == res[f]).all() for f in ("song", "offset", "shift", "score"))
    print("entry 0 == pfann_match: %s; mean n_found %.1f" % (same, nf.mean()), flush=True)
