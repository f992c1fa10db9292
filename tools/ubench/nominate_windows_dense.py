"""The windowed dense nomination (pfann_nominate_windows_dense) on monitor mode's workload, alone and with the rescoring behind it,
beside the expansion it replaces (pfann_nominate_songs_dense on the windows as queries: PFANN_NOMINATE_WINDOWS_GENERAL=1) and the
fp32 ranked dense pass, in ONE process on the same recordings: rounds A / B / A / B.

    python tools/ubench/nominate_windows_dense.py [--rows 1000000] [--recordings 8] [--rec-rows 1042] [--window 19] [--hop 2]
        [--edge-window 7] [--rounds 4] [--reps 5] [--out FILE]

The method of tools/ubench/nominate_dense.py: --rows random unit rows in songs of 59; --recordings recordings of --rec-rows rows
cut from the database plus noise (8 x 1042 rows: 4,096 windows at (19, 2), 8,288 at the edge pass's (7, 1)).  Per round every call
is timed --reps times with device events around the call (after a warm-up of every shape); a round's figure is the median of its
repetitions, the report gives the median and the range of the round medians.  With the profiler on, one more pass gives the per-tag
kernel times of the windowed call and of the expansion.  The fp32 dense pass is timed on --dense-recordings recordings and scaled.
No gate: the report says which of the two nominations is faster, whatever the ratio is."""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SEG_PER_SONG = 59
NS = (4, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--recordings", type=int, default=8)
    ap.add_argument("--rec-rows", type=int, default=1042)
    ap.add_argument("--window", type=int, default=19)
    ap.add_argument("--hop", type=int, default=2)
    ap.add_argument("--edge-window", type=int, default=7)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dense-recordings", type=int, default=1, help="recordings of the fp32 dense call (its time is scaled to --recordings)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from pfann_amd import lib as plib
    from pfann_amd.database import DeviceIndex, window_queries
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
    R, L = a.recordings, a.rec_rows
    rng = np.random.default_rng(6)
    at = rng.integers(0, n_rows - L, R)
    take = torch.as_tensor((at[:, None] + np.arange(L)[None, :]).reshape(-1)).to(dev)
    q = torch.nn.functional.normalize(rows[take] + 0.08 * torch.randn((R * L, a.d), device=dev, generator=g), dim=1).contiguous()
    rstart = np.arange(R, dtype=np.int64) * L
    rlen = np.full(R, L, dtype=np.int32)
    Rd = min(R, a.dense_recordings)
    shapes = {"long": (a.window, a.hop), "edge": (a.edge_window, 1)}
    queries = {k: window_queries(rstart, rlen, w, h) for k, (w, h) in shapes.items()}

    def windowed(kind, n):
        w, h = shapes[kind]
        return index.nominate_windows_dense(q, rstart, rlen, w, h, n, to_host=False)[0]

    def expanded(kind, n):
        qs, ql, _ = queries[kind]
        return index.nominate_songs_dense(q, qs, ql, n, to_host=False, max_qlen=shapes[kind][0])

    def rescored(nominate, kind, n):
        qs, ql, _ = queries[kind]
        cand, _, close = nominate(kind, n)
        return index.match_songs_dense(q, qs, ql, cand, to_host=False)[0], close

    def dense():
        index.match_windows_dense_topn(q[:Rd * L], rstart[:Rd], rlen[:Rd], a.window, a.hop, 16, to_host=False)

    calls = [("windowed long N=16", lambda: windowed("long", 16)), ("windowed edge N=16", lambda: windowed("edge", 16)),
             ("expansion long N=16", lambda: expanded("long", 16)), ("expansion edge N=16", lambda: expanded("edge", 16))]
    calls += [("windowed + rescore long N=%d" % n, (lambda n=n: rescored(windowed, "long", n))) for n in NS]
    calls += [("expansion + rescore long N=%d" % n, (lambda n=n: rescored(expanded, "long", n))) for n in NS]
    calls += [("fp32 dense topn(16) long", dense)]

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
    # the two nominations give the same bytes, here too
    same = all(bool((x == y).all()) for kind in shapes for x, y in zip(windowed(kind, 16), expanded(kind, 16)))
    tags = {}
    lib.pfann_prof_enable(1)
    for kind in shapes:
        for name, fn, names in (("windowed", windowed, ("seq_nominate_windows_prep", "seq_nominate_windows_tiles", "seq_nominate_windows_select")),
                                ("expansion", expanded, ("seq_nominate_prep", "seq_nominate_tiles", "seq_nominate_select"))):
            lib.pfann_prof_reset()
            fn(kind, 16)
            torch.cuda.synchronize()
            for tag in names:
                cnt = ctypes.c_int64(0)
                tags[(kind, name, tag)] = (float(lib.pfann_prof_elapsed_ms(tag.encode(), ctypes.byref(cnt))), int(cnt.value),
                                           float(lib.pfann_prof_work(tag.encode())))
    lib.pfann_prof_enable(0)
    nW = {k: int(v[2][-1]) for k, v in queries.items()}
    out = ["nominate_windows_dense: %d db rows (%d songs of %d), %d recordings of %d rows, d %d: %d windows at (%d, %d), %d at (%d, 1); "
           "%d rounds x median of %d, ms per call" % (n_rows, n_songs, SEG_PER_SONG, R, L, a.d, nW["long"], a.window, a.hop, nW["edge"],
                                                      a.edge_window, a.rounds, a.reps)]
    for name, _ in calls:
        m = med[name]
        scale = R / Rd if name.startswith("fp32 dense") else 1.0
        note = "   (%d recording(s) timed, x %.0f = %.1f ms for %d)" % (Rd, scale, float(np.median(m)) * scale, R) if scale != 1.0 else ""
        out.append("%-32s median %9.3f   range of round medians %9.3f .. %9.3f%s" % (name, float(np.median(m)), min(m), max(m), note))
    mid = lambda name: float(np.median(med[name]))
    dense_all = mid("fp32 dense topn(16) long") * R / Rd
    for kind in shapes:
        out.append("%s: expansion / windowed = %.2f x" % (kind, mid("expansion %s N=16" % kind) / mid("windowed %s N=16" % kind)))
    for n in NS:
        top, close = rescored(windowed, "long", n)
        close = close.cpu().numpy()
        out.append("N %2d: fp32 dense pass / (windowed + rescoring) = %.1f x, / (expansion + rescoring) = %.1f x; certified %d of %d windows"
                   % (n, dense_all / mid("windowed + rescore long N=%d" % n), dense_all / mid("expansion + rescore long N=%d" % n),
                      int(((close >= 0) & (close <= n)).sum()), nW["long"]))
    out.append("the two nominations give the same bytes: %s" % same)
    for (kind, name, tag), (ms, cnt, work) in tags.items():
        out.append("%-5s %-10s %-28s %9.3f ms in %d launch(es)%s" % (
            kind, name, tag, ms, cnt, "   %.1f TFLOP/s of tile products" % (work / ms / 1e9) if tag.endswith("tiles") and ms > 0 else ""))
    print("\n".join(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
