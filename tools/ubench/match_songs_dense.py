"""The rescoring stage alone (pfann_match_songs_dense), beside the search + pfann_match_topn it follows and the dense matcher it
stands in for, in ONE process on the same queries: same database, same box, rounds A / B / A / B.

    python tools/ubench/match_songs_dense.py [--rows 1000000] [--queries 4096] [--segs 19] [--k 100] [--rounds 4] [--reps 5]
        [--out FILE]

Database: --rows random unit rows in songs of 59 rows (bench.py's mean song).  Queries: --queries crops of --segs rows at random
places of the database plus noise, so that the search nominates the true song and the matcher's lists are full.  For N = 4, 16, 64
the lists are what pfann_match_topn(N) leaves on the device; the rescoring call is timed on them alone.  Per round every call is
timed --reps times with device events around the call (after a warm-up of every shape); a round's figure is the median of its
repetitions, the report gives the median and the range of the round medians.  The rounds interleave the calls (rescore N = 4, 16,
64, search + match_topn, dense, and again), so a drift of the box shows as spread, not as a difference.  No gate: by work count
(N songs x 59 rows of a million) the stage should be far below the search; the report says where it stands."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SEG_PER_SONG = 59
NS = (4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--segs", type=int, default=19)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-queries", type=int, default=512, help="queries of the dense call (its time is scaled to --queries)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfann_amd import lib as plib
    from pfann_amd.database import DeviceIndex
    plib.require_gpu()
    lib = plib.load()
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(5)
    n_songs = a.rows // SEG_PER_SONG
    n_rows = n_songs * SEG_PER_SONG
    song_pos = np.arange(n_songs + 1, dtype=np.int64) * SEG_PER_SONG
    rows = torch.nn.functional.normalize(torch.randn((n_rows, a.d), device=dev, generator=g), dim=1)
    index = DeviceIndex(a.d, 0)
    index.load(rows, song_pos)
    Q, S = a.queries, a.segs
    rng = np.random.default_rng(6)
    at = rng.integers(0, n_rows - S, Q)
    take = torch.as_tensor((at[:, None] + np.arange(S)[None, :]).reshape(-1)).to(dev)
    q = torch.nn.functional.normalize(rows[take] + 0.08 * torch.randn((Q * S, a.d), device=dev, generator=g), dim=1).contiguous()
    qstart = np.arange(Q, dtype=np.int64) * S
    qlen = np.full(Q, S, dtype=np.int32)
    qs, ql = index._upload_ranges(qstart, qlen)
    stream = index._stream()
    rsz = 24

    _, I = index.search(q, a.k)
    lists, outs = {}, {}
    for n in NS:
        lists[n] = index.match_topn(q, I, qstart, qlen, n, to_host=False)[0]
        outs[n] = (torch.empty((Q, n, rsz), device=dev, dtype=torch.uint8), torch.empty((Q,), device=dev, dtype=torch.int32))
    Qd = min(Q, a.dense_queries)

    def rescore(n):
        plib.check(lib.pfann_match_songs_dense(index.handle, q.data_ptr(), qs.data_ptr(), ql.data_ptr(), Q, lists[n].data_ptr(), n,
                                               outs[n][0].data_ptr(), outs[n][1].data_ptr(), stream), "pfann_match_songs_dense")

    def search_topn():
        _, lab = index.search(q, a.k)
        index.match_topn(q, lab, qstart, qlen, 16, to_host=False)

    def dense():
        index.match_windows_dense_topn(q[:Qd * S], qstart[:Qd], qlen[:Qd], S, 1, 16, to_host=False)

    calls = [("rescore N=%d" % n, (lambda n=n: rescore(n))) for n in NS] + [("search + match_topn(16)", search_topn), ("dense topn(16)", dense)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _, fn in calls:                                  # warm-up: code objects, workspaces, every shape
        fn()
        fn()
    torch.cuda.synchronize()
    med = {name: [] for name, _ in calls}
    for _ in range(a.rounds):
        for name, fn in calls:
            med[name].append(float(np.median([timed(fn) for _ in range(a.reps)])))
    found = {n: outs[n][1].cpu().numpy() for n in NS}
    tops = {n: index.decode_results(outs[n][0]) for n in NS}
    true_song = at // SEG_PER_SONG
    out = ["match_songs_dense: %d db rows (%d songs of %d), %d queries of %d rows, d %d, k %d; %d rounds x median of %d, ms per call"
           % (n_rows, n_songs, SEG_PER_SONG, Q, S, a.d, a.k, a.rounds, a.reps)]
    for name, _ in calls:
        m = med[name]
        scale = Q / Qd if name.startswith("dense") else 1.0
        note = "   (%d queries timed, x %.0f = %.1f ms for %d)" % (Qd, scale, float(np.median(m)) * scale, Q) if scale != 1.0 else ""
        out.append("%-26s median %9.3f   range of round medians %9.3f .. %9.3f%s" % (name, float(np.median(m)), min(m), max(m), note))
    for n in NS:
        out.append("N %2d: listed songs per query mean %.1f; answer names the crop's song in %d of %d queries; %.1f ns per (query, listed song)"
                   % (n, float(found[n].mean()), int((tops[n]["song"][:, 0] == true_song).sum()), Q,
                      1e6 * float(np.median(med["rescore N=%d" % n])) / max(1.0, float(found[n].sum()))))
    print("\n".join(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
