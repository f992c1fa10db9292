"""Monitor mode: go through long recordings and say what played when.
    python monitor.py <recording list> <database dir> <result file> [--window N] [--hop N] [--min-score X] [--max-gap N] [--min-windows N] [--edge-window N]

Every recording is embedded once, all its rows are searched once, and the windowed sequence matcher
(pfann_match_windows, csrc/monitor.hip) answers every window of `--window` segments, `--hop` segments apart, exactly as
matcher.py would answer that slice as a query.  merge_windows then joins consecutive windows that agree on the song and on
the diagonal (song time minus recording time) into detections.

Outputs: `<result file>`, a TSV with one line per detection
    recording  start_s  end_s  song  song_start_s  mean_score  best_score  n_windows
(an unreadable recording gives the line "recording<TAB>error"), and `<result-stem>_windows.csv` with one row per window
(recording, w0, start_s, song, score, time): Database.monitor_finish as it stands.
"""
import argparse
import csv
import os
import sys

import numpy as np

DEFAULT_HOP = 2
# default --min-score, chosen from the float64 oracle's window scores of the end-to-end case of tests/test_gpu_monitor.py
# (four excerpts at SNR 0, noise between them; DESIGN.md, "Monitor mode"): windows of noise alone score up to 0.182, windows
# inside an excerpt at least 0.211.
DEFAULT_MIN_SCORE = 0.2
# a detection needs this many agreeing windows when its recording has that many: a window that half overlaps a song can
# name a chance alignment at a song-like score, but chance does not repeat on one diagonal
DEFAULT_MIN_WINDOWS = 2


def default_window(params):
    """segments of a 10-second clip under the database's config (19 for configs/default.json)"""
    sr = params["sample_rate"]
    seg = int(sr * params["segment_size"])
    hop = int(sr * params["hop_size"]) // params["indexer"].get("frame_shift_mul", 1)
    return (max(10 * sr, seg) - seg) // hop + 1


def merge_windows(rows, window, hop, hop_size, min_score=DEFAULT_MIN_SCORE, max_gap=0, refine=True, min_windows=1, edge_rows=None,
                  edge_window=0):
    """Per-window answers of ONE recording -> detections.  Pure host code.

    rows: sequence of (w0, score, song, time_s) in ascending w0 (Database.monitor_finish), w0 = first segment of the window,
    time_s = where in the song the window starts; window, hop in segments (a recording shorter than `window` has one
    window over all its rows); hop_size = seconds between two segments.
    Consecutive windows that name the same song on the same diagonal (time_s - w0 * hop_size, equal to within a
    thousandth of a segment) with score >= min_score form one detection.  A window below min_score, or one that names
    another song or diagonal, ends it -- unless at most `max_gap` such windows in a row are followed by one that continues
    it; bridged windows count in n_windows but not in the scores.  The same song at another diagonal is a new detection.
    -> list of (rec_start_s, rec_end_s, song, song_start_s, mean_score, best_score, n_windows).
    edge_rows, edge_window: the same recording answered in short windows of edge_window segments at hop 1
    (Database.monitor_launch(edge_window=...)).  The short windows between a run's first window and the end of its last that
    name the run's song on its diagonal place the edges: the detection runs from the first of them to the end of the last.
    A chance alignment does not land on one given diagonal, so they are sparse at worst, not wrong; without any, the
    score-ratio edges below stand.
    min_windows: runs with fewer member windows are dropped, unless the recording has fewer windows than that (the CLI
    asks for DEFAULT_MIN_WINDOWS).
    refine: a window that only partly overlaps the song scores about that part of the full score (the other rows add ~0),
    so the first / last window of a run place the edges at w0 + window * (1 - s / best) and w0 + window * s / best instead
    of at the windows' own edges; the start is also clipped to where the song begins."""
    del hop                                              # (the spacing is in the w0 column; kept for the call's symmetry)
    tol = 1e-3 * hop_size
    tab = [(int(w0), float(score), int(song), float(time_s)) for w0, score, song, time_s in rows]
    runs, cur, i = [], None, 0
    while i < len(tab):
        w0, score, song, time_s = tab[i]
        diag = time_s - w0 * hop_size
        good = song >= 0 and score >= min_score
        if cur is None:
            if good:
                cur = {"song": song, "diag": diag, "w": [(w0, score)], "first": i, "last": i}
        elif good and song == cur["song"] and abs(diag - cur["diag"]) <= tol:
            cur["w"].append((w0, score))
            cur["last"] = i
        elif i - cur["last"] > max_gap:
            # too many disagreeing windows: the run ended at its last member, and what follows it starts over
            runs.append(cur)
            i, cur = cur["last"] + 1, None
            continue
        i += 1
    if cur is not None:
        runs.append(cur)
    out = []
    for run in runs:
        if len(run["w"]) < min(min_windows, len(tab)):
            continue
        w = run["w"]
        sc = np.asarray([s for _, s in w], np.float64)
        best = float(sc.max())
        first, last = w[0], w[-1]
        lo, hi = float(first[0]), float(last[0] + window)
        if refine and best > 0:
            lo = first[0] + window * (1.0 - min(1.0, max(0.0, first[1] / best)))
            hi = last[0] + window * min(1.0, max(0.0, last[1] / best))
            if hi <= lo:                                 # a single partly overlapping window: keep its own edges
                lo, hi = float(first[0]), float(last[0] + window)
        if edge_rows is not None and edge_window > 0:
            on = [int(w0) for w0, score, song, time_s in edge_rows
                  if first[0] <= int(w0) <= last[0] + window - min(edge_window, window) and int(song) == run["song"]
                  and abs(float(time_s) - int(w0) * hop_size - run["diag"]) <= tol]
            if on:
                lo, hi = float(on[0]), float(on[-1] + edge_window)
        start_s, end_s = lo * hop_size, hi * hop_size
        start_s = max(start_s, -run["diag"])             # the song cannot have begun before its first second
        out.append((start_s, end_s, run["song"], run["diag"] + start_s, float(sc.mean()), best, run["last"] - run["first"] + 1))
    return out


def parse_args(argv):
    ap = argparse.ArgumentParser(prog=os.path.basename(argv[0]), description="what played when in long recordings")
    ap.add_argument("recordings", help="text file with one recording (16-bit PCM WAV) per line")
    ap.add_argument("db", help="database directory written by builder.py")
    ap.add_argument("result", help="TSV of detections; <result-stem>_windows.csv gets one row per window")
    ap.add_argument("--window", type=int, default=None, help="segments per window (default: a 10-second clip)")
    ap.add_argument("--hop", type=int, default=DEFAULT_HOP, help="segments between two windows (default %d)" % DEFAULT_HOP)
    ap.add_argument("--min-score", type=float, default=DEFAULT_MIN_SCORE, help="windows below it separate detections")
    ap.add_argument("--min-windows", type=int, default=DEFAULT_MIN_WINDOWS,
                    help="agreeing windows a detection needs (default %d; recordings with fewer windows: all of them)" % DEFAULT_MIN_WINDOWS)
    ap.add_argument("--edge-window", type=int, default=None,
                    help="short windows (segments, hop 1) that place a detection's edges (default window // 3 + 1; 0: off)")
    ap.add_argument("--max-gap", type=int, default=0, help="disagreeing windows one detection may bridge")
    return ap.parse_args(argv[1:])


def main(argv=None):
    argv = sys.argv if argv is None else argv
    args = parse_args(argv)
    if int(os.environ.get("PFANN_GPUS", "1") or 1) > 1 or int(os.environ.get("WORLD_SIZE", "1") or 1) > 1:
        print("monitor: a recording is matched on ONE GPU against the whole database; song-sharded multi-GPU monitor mode "
              "is not supported (unset PFANN_GPUS)", file=sys.stderr)
        return 2
    if args.hop < 1 or (args.window is not None and args.window < 1):
        print("monitor: --window and --hop are positive numbers of segments", file=sys.stderr)
        return 2
    import torch
    from .builder import embed_file_batches
    from .database import Database, launch_ahead
    from .engine import Engine
    from .musicdata import MusicDataset
    from .utils import StageTimer, init_logger, read_config

    params = read_config(os.path.join(args.db, "configs.json"))
    init_logger("monitor")
    window = args.window if args.window is not None else default_window(params)
    edge_window = args.edge_window if args.edge_window is not None else window // 3 + 1
    fsm = params["indexer"].get("frame_shift_mul", 1)
    seg_step_s = params["hop_size"] / fsm                # seconds between two segments
    max_batch = int(os.environ.get("PFANN_MAX_BATCH", "9728"))
    dataset = MusicDataset(args.recordings, params)
    engine = Engine(params, 0, max_batch=max_batch)
    engine.set_plan_batch(max_batch)
    if not engine.weights_loaded:
        engine.load_state_dict(torch.load(os.path.join(args.db, "model.pt"), map_location="cpu"))
    db = Database(args.db, params["indexer"], params["hop_size"], device=0, d=params["model"]["d"])
    timer = StageTimer()
    db.timer = timer
    stem = os.path.splitext(args.result)[0]
    n_windows = n_det = 0
    with open(args.result, "w", encoding="utf8", newline="\n") as fout, \
            open(stem + "_windows.csv", "w", encoding="utf8", newline="\n") as fwin:
        wcsv = csv.writer(fwin)
        wcsv.writerow(["recording", "w0", "start_s", "song", "score", "time"])

        def launch(items):
            good = [(i, n, e) for i, n, e in items if n]
            p = None
            if good:
                emb = torch.cat([e for _, _, e in good])
                rlen = [n for _, n, _ in good]
                rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
                p = db.monitor_launch(emb, rstart, rlen, window, args.hop, edge_window=edge_window)
            return items, good, p

        def finish(launched):
            nonlocal n_windows, n_det
            items, good, p = launched
            per = dict(zip([i for i, _, _ in good], db.monitor_finish(p))) if p is not None else {}
            edge = dict(zip([i for i, _, _ in good], p.get("edge_rows") or [])) if p is not None else {}
            for i, n, _ in items:                         # list order, error rows in their places
                name = dataset.files[i]
                if n == 0:
                    fout.write("%s\terror\n" % name)
                    wcsv.writerow([name, "error", "", "", -1e999, 0])
                    continue
                rows = per[i]
                for w0, score, song, time_s in rows:
                    wcsv.writerow([name, int(w0), int(w0) * seg_step_s, db.songList[int(song)] if song >= 0 else "",
                                   float(score), float(time_s)])
                n_windows += len(rows)
                for d0, d1, song, s0, mean, best, nw in merge_windows(rows, min(window, n), args.hop, seg_step_s, args.min_score,
                                                                      args.max_gap, min_windows=args.min_windows,
                                                                      edge_rows=edge.get(i), edge_window=min(edge_window, n)):
                    fout.write("%s\t%.3f\t%.3f\t%s\t%.3f\t%.6f\t%.6f\t%d\n" % (name, d0, d1, db.songList[song], s0, mean, best, nw))
                    n_det += 1

        for launched in launch_ahead(embed_file_batches(engine, dataset, dataset.hop, batch_windows=max_batch, timer=timer), launch):
            finish(launched)
    timer.resolve(wait=True)
    for name, secs in timer.t.items():
        print("%s %.6fs" % (name, secs))
    print("monitor: %d recordings, %d windows (window %d, hop %d), %d detections" % (len(dataset), n_windows, window, args.hop, n_det))
    return 0


if __name__ == "__main__":
    sys.exit(main())
