"""Self-match: ask a database about itself -- which entries are the same recording under two names, which song contains a
stretch of another.
    python selfmatch.py <db dir> <result.tsv> [--window N] [--hop N] [--min-score X] [--min-windows N] [--max-gap N] [--songs A:B] [--topk K] [--dense] [--top N]

Needs no model and no audio: it reads configs.json, songList.txt, landmarkKey and embeddings of a directory written by
builder.py.  Every song's own fingerprints are the recording: each row is searched with its own song's rows left out
(pfann_search_topk_excl -- exact; a song queried against its own database would otherwise fill its top-k with its own
rows, which overlap by half), the windowed matcher answers every window exactly as matcher.py would answer that slice,
and monitor.merge_windows joins the windows into detections, unchanged.

Outputs: `<result.tsv>`, one line per detection
    song A  start_s  end_s  song B  offset_in_B_s  mean_score  best_score  n_windows
("seconds start_s .. end_s of A are B from offset_in_B_s on"), and `<stem>_windows.csv` with one row per window as the
monitor writes it (song A in the recording column).  A duplicate pair appears twice, as A in B and as B in A: that is
intended -- nothing is de-duplicated.  A partial containment appears from the contained side and, where the windows fit
into the shared stretch, from the container's side.  --songs A:B limits the songs QUERIED, not the songs searched.
--dense: no search; the dense matcher (pfann_match_windows_dense) scores every alignment of every other song in every window
(the song's own alignments are excluded), so nothing depends on --topk.  Same files, same columns; windows of at most 64 rows.
--top N (1..64; 1 is the default and writes both files exactly as described above): the N best OTHER songs of every window
(pfann_match_windows_dense_topn with --dense, pfann_match_windows_topn on the masked search's labels without), every (song,
diagonal) track merged by itself with monitor.merge_window_tracks, as monitor.py --top does -- a stretch stored three times
is then reported against BOTH other copies.  The detections file gets the ninth column best_rank, the windows file one row
per (window, rank) with the columns rank and votes."""
import argparse
import csv
import os
import sys

from .monitor import (DEFAULT_HOP, DEFAULT_MIN_SCORE, DEFAULT_MIN_WINDOWS, WINDOWS_HEADER, default_window, merge_window_tracks,
                      merge_windows, ranked_window_csv)


def parse_songs(text, n_songs):
    """"A:B" -> (A, B) with Python's slice defaults ("" = all, "7:8", ":10", "5:"), clipped to the song list"""
    if text is None or text == "":
        return 0, n_songs
    a, sep, b = text.partition(":")
    if not sep:
        raise ValueError("--songs wants A:B (got %r)" % text)
    lo = int(a) if a else 0
    hi = int(b) if b else n_songs
    if lo < 0 or hi < lo:
        raise ValueError("--songs %r: want 0 <= A <= B" % text)
    return min(lo, n_songs), min(hi, n_songs)


def parse_args(argv):
    ap = argparse.ArgumentParser(prog=os.path.basename(argv[0]), description="which songs of a database contain another")
    ap.add_argument("db", help="database directory written by builder.py")
    ap.add_argument("result", help="TSV of detections; <result-stem>_windows.csv gets one row per window")
    ap.add_argument("--window", type=int, default=None, help="rows per window (default: a 10-second clip)")
    ap.add_argument("--hop", type=int, default=DEFAULT_HOP, help="rows between two windows (default %d)" % DEFAULT_HOP)
    ap.add_argument("--min-score", type=float, default=DEFAULT_MIN_SCORE, help="windows below it separate detections")
    ap.add_argument("--min-windows", type=int, default=DEFAULT_MIN_WINDOWS,
                    help="agreeing windows a detection needs (default %d; songs with fewer windows: all of them)" % DEFAULT_MIN_WINDOWS)
    ap.add_argument("--max-gap", type=int, default=0, help="disagreeing windows one detection may bridge")
    ap.add_argument("--songs", default=None, help="A:B: query only the songs A..B-1 of the list (all are searched)")
    ap.add_argument("--topk", type=int, default=None, help="neighbours per row (default: the indexer's top_k)")
    ap.add_argument("--dense", action="store_true",
                    help="score every alignment of every other song in every window instead of the nominated ones (window <= 64)")
    ap.add_argument("--top", type=int, default=1,
                    help="other songs ranked per window (1..64, default 1); above 1 every (song, diagonal) is merged by itself "
                         "and both files get the extra columns of monitor.py --top")
    return ap.parse_args(argv[1:])


def detection_line(name_a, det, song_list):
    """one TSV line (without the newline) of a merge_windows detection of song A"""
    d0, d1, song, s0, mean, best, nw = det
    return "%s\t%.3f\t%.3f\t%s\t%.3f\t%.6f\t%.6f\t%d" % (name_a, d0, d1, song_list[song], s0, mean, best, nw)


def write_song(fout, wcsv, name_a, rows, song_list, window, hop, seg_step_s, min_score, max_gap, min_windows):
    """the windows of one song (window: rows per window, at most the song's rows) -> CSV rows and detection lines;
    returns (windows, detections)"""
    for w0, score, song, time_s in rows:
        wcsv.writerow([name_a, int(w0), int(w0) * seg_step_s, song_list[int(song)] if song >= 0 else "", float(score), float(time_s)])
    dets = merge_windows(rows, window, hop, seg_step_s, min_score, max_gap, min_windows=min_windows)
    for det in dets:
        fout.write(detection_line(name_a, det, song_list) + "\n")
    return len(rows), len(dets)


def write_song_ranked(fout, wcsv, name_a, rows, song_list, window, hop, seg_step_s, min_score, max_gap, min_windows):
    """write_song for the ranked [windows, n] rows of --top N > 1: one CSV row per (window, rank), every (song, diagonal)
    track merged by itself, detection lines with the ninth column best_rank"""
    wcsv.writerows(ranked_window_csv(name_a, rows, seg_step_s, song_list))
    dets = merge_window_tracks(rows, window, hop, seg_step_s, min_score, max_gap, min_windows=min_windows)
    for det in dets:
        fout.write(detection_line(name_a, det[:7], song_list) + "\t%d\n" % det[7])
    return len(rows), len(dets)


def main(argv=None):
    argv = sys.argv if argv is None else argv
    args = parse_args(argv)
    if args.hop < 1 or (args.window is not None and args.window < 1) or (args.topk is not None and not 1 <= args.topk <= 1024):
        print("selfmatch: --window and --hop are positive numbers of rows, --topk is 1..1024", file=sys.stderr)
        return 2
    if not 1 <= args.top <= 64:
        print("selfmatch: --top ranks 1..64 songs per window", file=sys.stderr)
        return 2
    if args.dense and args.window is not None and args.window > 64:
        print("selfmatch: --dense takes windows of at most 64 rows", file=sys.stderr)
        return 2
    from . import lib as _l
    from .utils import read_config
    params = read_config(os.path.join(args.db, "configs.json"))
    _l.require_gpu()                                     # (PfannError: there is no CPU path)
    from .database import Database
    from .utils import StageTimer, init_logger
    init_logger("selfmatch")
    window = args.window if args.window is not None else default_window(params)
    seg_step_s = params["hop_size"]                      # the rows are database rows: one per hop_size
    db = Database(args.db, params["indexer"], params["hop_size"], device=0, d=params["model"]["d"])
    song_lo, song_hi = parse_songs(args.songs, len(db.songList))
    timer = StageTimer()
    db.timer = timer
    stem = os.path.splitext(args.result)[0]
    n_windows = n_det = 0
    with open(args.result, "w", encoding="utf8", newline="\n") as fout, \
            open(stem + "_windows.csv", "w", encoding="utf8", newline="\n") as fwin:
        wcsv = csv.writer(fwin)
        wcsv.writerow(WINDOWS_HEADER + (["rank", "votes"] if args.top > 1 else []))
        write = write_song_ranked if args.top > 1 else write_song
        for s, rows in db.self_match(song_lo, song_hi, window, args.hop, args.topk, dense=args.dense, top=args.top):
            n_song = int(db.song_pos[s + 1] - db.song_pos[s])
            nw, nd = write(fout, wcsv, db.songList[s], rows, db.songList, min(window, n_song) if n_song else window, args.hop,
                                seg_step_s, args.min_score, args.max_gap, args.min_windows)
            n_windows += nw
            n_det += nd
    timer.resolve(wait=True)
    for name, secs in timer.t.items():
        print("%s %.6fs" % (name, secs))
    print("selfmatch: %d songs, %d windows (window %d, hop %d), %d detections" % (song_hi - song_lo, n_windows, window, args.hop, n_det))
    return 0


if __name__ == "__main__":
    sys.exit(main())
