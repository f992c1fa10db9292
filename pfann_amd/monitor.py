"""Monitor mode: go through long recordings and say what played when.
    python monitor.py <recording list> <database dir> <result file> [--window N] [--hop N] [--min-score X] [--max-gap N] [--min-windows N] [--edge-window N] [--top N] [--dense] [--max-fa X] [--nominate N]

Every recording is embedded once, all its rows are searched once, and the windowed sequence matcher
(pfann_match_windows, csrc/monitor.hip) answers every window of `--window` segments, `--hop` segments apart, exactly as
matcher.py would answer that slice as a query.  merge_windows then joins consecutive windows that agree on the song and on
the diagonal (song time minus recording time) into detections.

Outputs: `<result file>`, a TSV with one line per detection
    recording  start_s  end_s  song  song_start_s  mean_score  best_score  n_windows
(an unreadable recording gives the line "recording<TAB>error"), and `<result-stem>_windows.csv` with one row per window
(recording, w0, start_s, song, score, time): Database.monitor_finish as it stands.

`--top N` (N > 1) ranks the N best songs of every window (pfann_match_windows_topn) and merges every (song, diagonal) track
by itself (merge_window_tracks), so that two songs that play at once -- a crossfade, music under a jingle -- both come out,
as detections that overlap in time.  The detections file then has a ninth column, best_rank (the best rank a member window
gave the song), and the windows file one row per (window, rank) with two more columns, rank (1-based) and votes (the
alignments of that song the window nominated); its rank-1 rows are the rows of `--top 1`, which is the default and writes
both files exactly as described above.

`--dense` answers every window with the dense matcher (pfann_match_windows_dense, csrc/dense.hip): no search, EVERY alignment
of every song is a candidate of every window, so the answers do not depend on the indexer's top_k.  Same files, same
columns; windows of at most 64 segments; not together with `--top N` > 1 here: ranked dense answers exist
(pfann_match_windows_dense_topn, Database.monitor_dense_topn_launch / monitor_dense_topn_finish), this tool does not route
`--dense --top N` to them yet.

`PFANN_GPUS=N python monitor.py ... --dense [--max-fa X]` (or the same command under torch.distributed.run) shards the
database by whole songs over N GPUs: every rank scores every window against its own songs' rows only
(pfann_match_windows_dense_part), the ranks' words and integer sums are all-gathered and merged
(pfann_match_windows_dense_merge), and rank 0 writes both files -- byte for byte the files of one process.  Without `--dense`
several ranks are refused (status 2): the nominated forms are not song-sharded.

`--max-fa X` (with `--dense`, 0 < X <= 1) replaces the fixed `--min-score` by a threshold calibrated per window: the dense
matcher also returns the mean and the variance of the window's other alignments (pfann_match_windows_dense_stats), and
pfann_amd/significance.py turns the best score into log10_fa, log10 of the chance that the best of that many chance alignments
scores as high.  A window then counts when it names a song and log10_fa <= log10(X); `--min-score` is not consulted.  The
windows file gets a seventh column, log10_fa, and the detections file a ninth, min_log10_fa: the most significant member
window.  What score chance reaches depends on the window length, the size of the database and the model; X does not.

`--dense --nominate N` (1 <= N <= 64) gives `--dense`'s answers without the fp32 dense pass: the fp16 MFMA names N songs per
window over every alignment (pfann_nominate_windows_dense, csrc/nominate_windows.hip: the windows of a recording share their
row dots), pfann_match_songs_dense scores those songs exactly, and the window's n_close <= N proves that its row is `--dense`'s
row byte for byte (Database.monitor_nominate_launch / monitor_nominate_finish).  Both files keep `--dense`'s columns;
`<result-stem>_nominate.csv` gets one row per long window, recording,w0,n_close,certified (an unreadable recording:
recording,error,-1,0).  Not together with `--max-fa` (the background statistics come from the fp32 dense pass), `--top N` > 1 or
several ranks.
"""
import argparse
import csv
import math
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
DENSE_MAX_WINDOW = 64                                    # pfann_match_windows_dense


def default_window(params):
    """segments of a 10-second clip under the database's config (19 for configs/default.json)"""
    sr = params["sample_rate"]
    seg = int(sr * params["segment_size"])
    hop = int(sr * params["hop_size"]) // params["indexer"].get("frame_shift_mul", 1)
    return (max(10 * sr, seg) - seg) // hop + 1


def merge_windows(rows, window, hop, hop_size, min_score=DEFAULT_MIN_SCORE, max_gap=0, refine=True, min_windows=1, edge_rows=None,
                  edge_window=0, good=None):
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
    of at the windows' own edges; the start is also clipped to where the song begins.
    good: one truth value per row that replaces the test score >= min_score (a window still has to name a song)."""
    return [det for det, _, _ in _merge_runs(rows, window, hop, hop_size, min_score, max_gap, refine, min_windows, edge_rows, edge_window,
                                             good)]


def _merge_runs(rows, window, hop, hop_size, min_score, max_gap, refine, min_windows, edge_rows, edge_window, good=None):
    """merge_windows' work -> [(detection, (first, last), members)]: the detection, the rows[] range its run spans and the
    indices of its member windows"""
    del hop                                              # (the spacing is in the w0 column; kept for the call's symmetry)
    tol = 1e-3 * hop_size
    tab = [(int(w0), float(score), int(song), float(time_s)) for w0, score, song, time_s in rows]
    passes = [score >= min_score for _, score, _, _ in tab] if good is None else [bool(g) for g in good]
    assert len(passes) == len(tab), "good wants one value per row"
    runs, cur, i = [], None, 0
    while i < len(tab):
        w0, score, song, time_s = tab[i]
        diag = time_s - w0 * hop_size
        ok = song >= 0 and passes[i]
        if cur is None:
            if ok:
                cur = {"song": song, "diag": diag, "w": [(w0, score)], "idx": [i], "first": i, "last": i}
        elif ok and song == cur["song"] and abs(diag - cur["diag"]) <= tol:
            cur["w"].append((w0, score))
            cur["idx"].append(i)
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
        det = (start_s, end_s, run["song"], run["diag"] + start_s, float(sc.mean()), best, run["last"] - run["first"] + 1)
        out.append((det, (run["first"], run["last"]), run["idx"]))
    return out


def _ranked(rows):
    """ranked rows in either form -> [[(w0, score, song, time_s), ..] per window]: a [windows, n] structured array
    (Database.monitor_topn_finish), nested sequences, or one answer per window (Database.monitor_finish: one rank)"""
    if isinstance(rows, np.ndarray) and rows.dtype.names:
        flat = rows.ndim == 1
    else:
        flat = len(rows) > 0 and np.ndim(rows[0][0]) == 0
    entry = lambda e: (int(e[0]), float(e[1]), int(e[2]), float(e[3]))
    return [[entry(row)] if flat else [entry(e) for e in row] for row in rows]


def merge_window_tracks(ranked_rows, window, hop, hop_size, min_score=DEFAULT_MIN_SCORE, max_gap=0, refine=True, min_windows=1,
                        edge_rows=None, edge_window=0):
    """Ranked per-window answers of ONE recording -> detections that may overlap in time.  Pure host code.

    ranked_rows: per window, in ascending w0, its entries best first, each (w0, score, song, time_s[, votes])
    (Database.monitor_topn_finish; padding entries have song -1).  The other arguments are merge_windows'; edge_rows are the
    ranked short windows of the edge pass.
    A track is a (song, diagonal) pair that some entry of some window names with score >= min_score, diagonals equal to
    within merge_windows' tolerance.  Every track is merged BY ITSELF: merge_windows runs over the sequence that holds the
    track's entry where a window has one and (w0, -inf, -1, 0) where it has none, with the edge pass restricted to the
    track in the same way.  -> the union over the tracks, sorted by (start, song):
    [(rec_start_s, rec_end_s, song, song_start_s, mean_score, best_score, n_windows, best_rank)], best_rank = the best
    (smallest, 1-based) rank a member window gave the track.
    With one rank and max_gap = 0 these are merge_windows' detections exactly (a run is then a maximal stretch of
    consecutive windows on one track, either way), in (start, song) order.  With max_gap > 0 they can differ: take three
    windows U T U at max_gap = 1.  merge_windows bridges the middle window -- one detection of U over three windows, and
    T, swallowed by the bridge, is never reported; here track U still bridges its missing window, and track T, merged by
    itself, is a detection of its own."""
    tol = 1e-3 * hop_size
    tab = _ranked(ranked_rows)
    edge = _ranked(edge_rows) if edge_rows is not None and edge_window > 0 else None
    tracks = []                                          # (song, diagonal of the first entry that named it)
    for row in tab:
        for w0, score, song, time_s in row:
            diag = time_s - w0 * hop_size
            if song >= 0 and score >= min_score and not any(s == song and abs(diag - g) <= tol for s, g in tracks):
                tracks.append((song, diag))

    def restrict(rows, song, diag):
        """-> (the track's entry or a blank per window, the 1-based rank it held or 0)"""
        seq, rank = [], []
        for row in rows:
            hit = [j for j, (w0, score, s, time_s) in enumerate(row) if s == song and abs(time_s - w0 * hop_size - diag) <= tol]
            seq.append(row[hit[0]] if hit else (row[0][0], -np.inf, -1, 0.0))
            rank.append(hit[0] + 1 if hit else 0)
        return seq, rank

    out = []
    for song, diag in tracks:
        seq, rank = restrict(tab, song, diag)
        eseq = restrict(edge, song, diag)[0] if edge is not None else None
        for det, (first, last), _ in _merge_runs(seq, window, hop, hop_size, min_score, max_gap, refine, min_windows, eseq, edge_window):
            members = [rank[i] for i in range(first, last + 1) if rank[i] and seq[i][1] >= min_score]
            out.append(det + (min(members),))
    return sorted(out, key=lambda det: (det[0], det[2]))


WINDOWS_HEADER = ["recording", "w0", "start_s", "song", "score", "time"]


def ranked_window_csv(name, ranked_rows, seg_step_s, song_names):
    """rows of `<stem>_windows.csv` under --top N > 1 for one recording: WINDOWS_HEADER + ["rank", "votes"], one row per
    (window, rank); rank 1 is always written (it is the --top 1 row), padding entries behind it are not"""
    out = []
    for row in ranked_rows:
        for j, (w0, score, song, time_s, votes) in enumerate(row):
            if j == 0 or song >= 0:
                out.append([name, int(w0), int(w0) * seg_step_s, song_names[int(song)] if song >= 0 else "", float(score),
                            float(time_s), j + 1, int(votes)])
    return out


NOMINATE_HEADER = ["recording", "w0", "n_close", "certified"]


def nominate_csv(name, rows, n_close, certified):
    """rows of `<stem>_nominate.csv` for one recording: NOMINATE_HEADER, one row per long window in the order of the windows
    file; rows: the recording's (w0, ..) rows, n_close / certified: one value per row (Database.monitor_nominate_finish)"""
    assert len(rows) == len(n_close) == len(certified), "one n_close and one certificate per window"
    return [[name, int(row[0]), int(c), 1 if ok else 0] for row, c, ok in zip(rows, n_close, certified)]


def check_nominate(args, several=False):
    """-> the message that refuses this use of --nominate, or None"""
    if args.nominate is None:
        return None
    if not args.dense:
        return "--nominate names the songs that the dense arithmetic then scores; it needs --dense"
    if args.max_fa is not None:
        return "--nominate cannot be combined with --max-fa: the background statistics come from the fp32 dense pass"
    if args.top > 1:
        return "--nominate gives one answer per window; it cannot be combined with --top %d" % args.top
    if not 1 <= args.nominate <= 64:
        return "--nominate lists 1..64 songs per window"
    if several:
        return "--nominate rescoring runs on ONE GPU against the whole database; song-sharded multi-GPU is not supported (unset PFANN_GPUS)"
    return None


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
    ap.add_argument("--top", type=int, default=1,
                    help="songs ranked per window (1..64, default 1); above 1 detections may overlap in time: every (song, "
                         "diagonal) is merged by itself, and both files get the extra columns described above")
    ap.add_argument("--dense", action="store_true",
                    help="score every alignment of every song in every window instead of the ones a top-k search nominates "
                         "(window <= 64, --top 1)")
    ap.add_argument("--max-fa", type=float, default=None,
                    help="with --dense: a window counts when the chance that its best score is a chance alignment is at most X "
                         "(0 < X <= 1), judged from the window's own background; replaces --min-score")
    ap.add_argument("--nominate", type=int, default=None, metavar="N",
                    help="with --dense: the fp16 MFMA names N songs per window (1..64), only those are scored exactly; "
                         "<result-stem>_nominate.csv says which windows are certified to be --dense's")
    return ap.parse_args(argv[1:])


def main(argv=None):
    argv = sys.argv if argv is None else argv
    args = parse_args(argv)
    several = int(os.environ.get("PFANN_GPUS", "1") or 1) > 1 or int(os.environ.get("WORLD_SIZE", "1") or 1) > 1
    if several and not args.dense:                       # (only the dense matcher merges song shards: pfann_amd/dist.py)
        print("monitor: a recording is matched on ONE GPU against the whole database; song-sharded multi-GPU monitor mode "
              "is not supported (unset PFANN_GPUS)", file=sys.stderr)
        return 2
    refused = check_nominate(args, several)
    if refused is not None:
        print("monitor: " + refused, file=sys.stderr)
        return 2
    if args.hop < 1 or (args.window is not None and args.window < 1):
        print("monitor: --window and --hop are positive numbers of segments", file=sys.stderr)
        return 2
    if not 1 <= args.top <= 64:
        print("monitor: --top ranks 1..64 songs per window", file=sys.stderr)
        return 2
    if args.dense and args.top > 1:
        print("monitor: --dense gives one answer per window; it cannot be combined with --top %d" % args.top, file=sys.stderr)
        return 2
    if args.dense and args.window is not None and args.window > DENSE_MAX_WINDOW:
        print("monitor: --dense takes windows of at most %d segments" % DENSE_MAX_WINDOW, file=sys.stderr)
        return 2
    if args.max_fa is not None and not args.dense:
        print("monitor: --max-fa judges a window by the background of the dense matcher; it needs --dense", file=sys.stderr)
        return 2
    if args.max_fa is not None and not 0.0 < args.max_fa <= 1.0:
        print("monitor: --max-fa is a false-alarm probability, 0 < X <= 1", file=sys.stderr)
        return 2
    from .dist import self_launch_if_asked
    rc = self_launch_if_asked(argv)                      # PFANN_GPUS=N: N ranks of this command, one per GPU
    if rc is not None:
        return rc
    import torch
    from .builder import embed_file_batches, gather_round
    from .database import Database, launch_ahead
    from .dist import finish_ranks, init_ranks
    from .engine import Engine
    from .musicdata import MusicDataset
    from .utils import StageTimer, init_logger, read_config

    # several ranks (--dense only): every rank holds the rows of its own songs, reads and embeds its share of the recordings,
    # gets the others' fingerprints (gather_round) and takes part in every launch; all ranks hold the same answers and rank 0
    # writes them -- byte for byte the files of a single process
    ranks = init_ranks()                                 # None: a plain single-process run
    multi = ranks is not None and ranks.world > 1
    rank0 = ranks is None or ranks.rank == 0
    dev = ranks.device if ranks is not None else 0
    params = read_config(os.path.join(args.db, "configs.json"))
    if rank0:
        init_logger("monitor")
    window = args.window if args.window is not None else default_window(params)
    edge_window = args.edge_window if args.edge_window is not None else window // 3 + 1
    fsm = params["indexer"].get("frame_shift_mul", 1)
    seg_step_s = params["hop_size"] / fsm                # seconds between two segments
    max_batch = int(os.environ.get("PFANN_MAX_BATCH", "9728"))
    dataset = MusicDataset(args.recordings, params)
    engine = Engine(params, dev, max_batch=max_batch)
    engine.set_plan_batch(max_batch)                     # (fingerprint bits do not depend on the batch a recording is embedded in)
    if not engine.weights_loaded:
        engine.load_state_dict(torch.load(os.path.join(args.db, "model.pt"), map_location="cpu"))
    db = Database(args.db, params["indexer"], params["hop_size"], device=dev, d=params["model"]["d"], ranks=ranks)
    timer = StageTimer()
    db.timer = timer
    stem = os.path.splitext(args.result)[0]
    n_windows = n_det = 0
    with open(args.result if rank0 else os.devnull, "w", encoding="utf8", newline="\n") as fout, \
            open(stem + "_windows.csv" if rank0 else os.devnull, "w", encoding="utf8", newline="\n") as fwin, \
            open(stem + "_nominate.csv" if rank0 and args.nominate is not None else os.devnull, "w", encoding="utf8", newline="\n") as fnom:
        wcsv, ncsv = csv.writer(fwin), csv.writer(fnom)
        ncsv.writerow(NOMINATE_HEADER)
        wcsv.writerow(WINDOWS_HEADER + (["rank", "votes"] if args.top > 1 else []) + (["log10_fa"] if args.max_fa is not None else []))

        def launch(items):
            good = [(i, n, e) for i, n, e in items if n]
            p = None
            if good:
                emb = torch.cat([e for _, _, e in good])
                rlen = [n for _, n, _ in good]
                rstart = np.concatenate([[0], np.cumsum(rlen)[:-1]])
                if args.nominate is not None:
                    p = db.monitor_nominate_launch(emb, rstart, rlen, window, args.hop, args.nominate, edge_window=edge_window)
                elif args.dense:
                    p = db.monitor_dense_launch(emb, rstart, rlen, window, args.hop, edge_window=edge_window,
                                                stats=args.max_fa is not None)
                elif args.top > 1:
                    p = db.monitor_topn_launch(emb, rstart, rlen, window, args.hop, args.top, edge_window=edge_window)
                else:
                    p = db.monitor_launch(emb, rstart, rlen, window, args.hop, edge_window=edge_window)
            return items, good, p

        def finish(launched):
            nonlocal n_windows, n_det
            items, good, p = launched
            fa, cert = {}, {}
            if p is not None and args.nominate is not None:
                rows, close, sure = db.monitor_nominate_finish(p)
                per, cert = dict(zip([i for i, _, _ in good], rows)), dict(zip([i for i, _, _ in good], zip(close, sure)))
            elif p is not None and args.max_fa is not None:
                rows, log10_fa = db.monitor_dense_stats_finish(p)
                per, fa = dict(zip([i for i, _, _ in good], rows)), dict(zip([i for i, _, _ in good], log10_fa))
            elif p is not None and args.top > 1:
                per = dict(zip([i for i, _, _ in good], db.monitor_topn_finish(p)[0]))
            else:
                per = dict(zip([i for i, _, _ in good], db.monitor_finish(p))) if p is not None else {}
            edge = dict(zip([i for i, _, _ in good], p.get("edge_rows") or [])) if p is not None else {}
            for i, n, _ in items:                         # list order, error rows in their places
                name = dataset.files[i]
                if n == 0:
                    fout.write("%s\terror\n" % name)
                    wcsv.writerow([name, "error", "", "", -1e999, 0] + ([0.0] if args.max_fa is not None else []))
                    ncsv.writerow([name, "error", -1, 0])
                    continue
                rows = per[i]
                if args.nominate is not None:
                    ncsv.writerows(nominate_csv(name, rows, *cert[i]))
                if args.top > 1:
                    wcsv.writerows(ranked_window_csv(name, rows, seg_step_s, db.songList))
                    n_windows += len(rows)
                    for d0, d1, song, s0, mean, best, nw, rank in merge_window_tracks(
                            rows, min(window, n), args.hop, seg_step_s, args.min_score, args.max_gap, min_windows=args.min_windows,
                            edge_rows=edge.get(i), edge_window=min(edge_window, n)):
                        fout.write("%s\t%.3f\t%.3f\t%s\t%.3f\t%.6f\t%.6f\t%d\t%d\n" % (name, d0, d1, db.songList[song], s0, mean, best, nw, rank))
                        n_det += 1
                    continue
                if args.max_fa is not None:              # the calibrated threshold: --min-score is not consulted
                    for (w0, score, song, time_s), x in zip(rows, fa[i]):
                        wcsv.writerow([name, int(w0), int(w0) * seg_step_s, db.songList[int(song)] if song >= 0 else "",
                                       float(score), float(time_s), float(x)])
                    n_windows += len(rows)
                    for (d0, d1, song, s0, mean, best, nw), _, members in _merge_runs(
                            rows, min(window, n), args.hop, seg_step_s, args.min_score, args.max_gap, True, args.min_windows,
                            edge.get(i), min(edge_window, n), good=fa[i] <= math.log10(args.max_fa)):
                        fout.write("%s\t%.3f\t%.3f\t%s\t%.3f\t%.6f\t%.6f\t%d\t%.3f\n"
                                   % (name, d0, d1, db.songList[song], s0, mean, best, nw, min(float(fa[i][j]) for j in members)))
                        n_det += 1
                    continue
                for w0, score, song, time_s in rows:
                    wcsv.writerow([name, int(w0), int(w0) * seg_step_s, db.songList[int(song)] if song >= 0 else "",
                                   float(score), float(time_s)])
                n_windows += len(rows)
                for d0, d1, song, s0, mean, best, nw in merge_windows(rows, min(window, n), args.hop, seg_step_s, args.min_score,
                                                                      args.max_gap, min_windows=args.min_windows,
                                                                      edge_rows=edge.get(i), edge_window=min(edge_window, n)):
                    fout.write("%s\t%.3f\t%.3f\t%s\t%.3f\t%.6f\t%.6f\t%d\n" % (name, d0, d1, db.songList[song], s0, mean, best, nw))
                    n_det += 1

        groups = embed_file_batches(engine, dataset, dataset.hop, batch_windows=max_batch, timer=timer, ranks=ranks)
        if multi:
            groups = (gather_round(ranks, rnd, engine.d, engine.device) for rnd in groups)
        for launched in launch_ahead(groups, launch):
            finish(launched)
    timer.resolve(wait=True)
    if rank0:
        for name, secs in timer.t.items():
            print("%s %.6fs" % (name, secs))
        print("monitor: %d recordings, %d windows (window %d, hop %d), %d detections" % (len(dataset), n_windows, window, args.hop, n_det))
    finish_ranks(ranks)
    return 0


if __name__ == "__main__":
    sys.exit(main())
