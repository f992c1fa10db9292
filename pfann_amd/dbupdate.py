"""Database updates: add songs to and remove songs from a database directory without a rebuild.
    python dbupdate.py add    <music list> <db> [--allow-duplicates]
    python dbupdate.py remove <song list>  <db>      # lines: a path as in songList.txt, or #<id>
    python dbupdate.py check  <db> [--repair]

add     embeds the files of <music list> with the model of the DIRECTORY (its configs.json and model.pt, so the model cannot
        differ from the one the database was built with), the engine set up exactly as builder.py sets it up (PFANN_MAX_BATCH,
        set_plan_batch: a song's fingerprint bytes do not depend on the batch it was embedded in), and appends them through
        pfann_amd/dbfiles.py.  The directory is then byte for byte the one builder.py writes for the longer list.  The new
        songs get the ids behind the last one; an unreadable file becomes a song without rows, as in the builder.  Paths
        already in songList.txt stop it (exit code 2) unless --allow-duplicates is given.  Single-process.
remove  the listed songs lose their rows and keep their ids (landmarkKey 0: "this id has no rows"); O(database) file I/O.
check   says whether the directory is a clean database; --repair rolls an interrupted update forward or back (no GPU).

remove and check need no GPU and never import torch."""
import argparse
import os
import sys


def parse_args(argv):
    ap = argparse.ArgumentParser(prog=os.path.basename(argv[0]), description="add songs to / remove songs from a database directory")
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("add", help="embed the files of a music list and append them")
    a.add_argument("list", help="music list: one path per line, as builder.py takes it")
    a.add_argument("db", help="database directory written by builder.py")
    a.add_argument("--allow-duplicates", action="store_true", help="add paths that songList.txt already holds")
    r = sub.add_parser("remove", help="take songs out (they keep their ids, without rows)")
    r.add_argument("list", help="one song per line: a path as in songList.txt, or #<id>")
    r.add_argument("db")
    c = sub.add_parser("check", help="is the directory a clean database?")
    c.add_argument("db")
    c.add_argument("--repair", action="store_true", help="roll an interrupted update forward (journal) or back (none)")
    return ap.parse_args(argv[1:])


def _clean_or_say(db):
    from . import dbfiles
    bad = dbfiles.problems(db)
    if bad:
        print("dbupdate: %s is not a clean database (run `dbupdate.py check %s --repair`):" % (db, db), file=sys.stderr)
        for ln in bad:
            print("  " + ln, file=sys.stderr)
    return not bad


def resolve_songs(lines, names):
    """lines of a remove list -> (sorted ids, unknown lines); a path names every song of that name"""
    ids, unknown = set(), []
    for ln in lines:
        if not ln.strip():
            continue
        if ln.startswith("#"):
            try:
                i = int(ln[1:])
            except ValueError:
                i = -1
            if 0 <= i < len(names):
                ids.add(i)
            else:
                unknown.append(ln)
            continue
        hit = [i for i, n in enumerate(names) if n == ln]
        if hit:
            ids.update(hit)
        else:
            unknown.append(ln)
    return sorted(ids), unknown


def cmd_check(args):
    from . import dbfiles
    bad = dbfiles.problems(args.db)
    if not bad:
        print("dbupdate: %s is a clean database" % args.db)
        return 0
    for ln in bad:
        print(ln)
    if not args.repair:
        print("dbupdate: run `dbupdate.py check %s --repair`" % args.db)
        return 1
    dbfiles.repair(args.db)
    left = dbfiles.problems(args.db)
    for ln in left:
        print("still: " + ln)
    print("dbupdate: repaired" if not left else "dbupdate: could not repair")
    return 0 if not left else 1


def cmd_remove(args):
    from . import dbfiles
    from .utils import read_file_list
    names = dbfiles.read_names(args.db)
    ids, unknown = resolve_songs(read_file_list(args.list), names)
    if unknown:
        print("dbupdate remove: not in the database: " + ", ".join(repr(u) for u in unknown[:10]) +
              (" ... (%d in all)" % len(unknown) if len(unknown) > 10 else ""), file=sys.stderr)
        return 2
    if not _clean_or_say(args.db):
        return 2
    key = dbfiles.read_key(args.db)
    rows = int(key[ids].astype("int64").sum()) if ids else 0
    dbfiles.remove_songs(args.db, ids)
    print("dbupdate remove: %d songs, %d rows taken out of %s (the whole row files were written again)" % (len(ids), rows, args.db))
    return 0


def cmd_add(args):
    from . import dbfiles
    from .utils import read_config, read_file_list
    if int(os.environ.get("PFANN_GPUS", "1") or 1) > 1:
        print("dbupdate add: single-process (PFANN_GPUS=%s): the new songs of a day are no job for several GPUs"
              % os.environ["PFANN_GPUS"], file=sys.stderr)
        return 2
    new = read_file_list(args.list)
    have = set(dbfiles.read_names(args.db))
    dup = [n for n in new if n in have]
    if dup and not args.allow_duplicates:
        print("dbupdate add: already in songList.txt (--allow-duplicates adds them again): " +
              ", ".join(repr(u) for u in dup[:10]) + (" ... (%d in all)" % len(dup) if len(dup) > 10 else ""), file=sys.stderr)
        return 2
    if not _clean_or_say(args.db):
        return 2
    params = read_config(os.path.join(args.db, "configs.json"))
    params["model_dir"] = args.db
    # ---- from here on: the GPU, exactly as builder.py sets it up
    import numpy as np
    import torch
    from .builder import embed_file_batches
    from .engine import Engine
    from .musicdata import MusicDataset
    from .utils import StageTimer, init_logger
    init_logger("dbupdate")
    max_batch = int(os.environ.get("PFANN_MAX_BATCH", "9728"))
    engine = Engine(params, 0, max_batch=max_batch)
    engine.set_plan_batch(max_batch)
    if not engine.weights_loaded:
        engine.load_state_dict(torch.load(os.path.join(args.db, "model.pt"), map_location="cpu"))
    engine.warmup(windows=max_batch, group_hop=int(params["sample_rate"] * params["hop_size"]))
    params["indexer"]["frame_shift_mul"] = 1                               # builder.py:64
    dataset = MusicDataset(args.list, params)
    d = params["model"]["d"]
    key = np.zeros(len(dataset), dtype=np.int32)
    parts = []
    timer = StageTimer()
    for items in embed_file_batches(engine, dataset, dataset.hop, batch_windows=max_batch, timer=timer):
        for idx, n_seg, emb in items:
            key[idx] = n_seg
            if n_seg:
                parts.append(emb.cpu().numpy())
    emb = np.concatenate(parts) if parts else np.zeros((0, d), np.float32)
    first, last = dbfiles.add_songs(args.db, new, emb, key)
    print("dbupdate add: songs %d..%d, %d rows added to %s" % (first, last - 1, emb.shape[0], args.db))
    print("check the new songs for duplicates of old ones:")
    print("    python selfmatch.py %s dup.tsv --songs %d:%d" % (args.db, first, last))
    return 0


def main(argv=None):
    argv = sys.argv if argv is None else argv
    args = parse_args(argv)
    return {"add": cmd_add, "remove": cmd_remove, "check": cmd_check}[args.cmd](args)


if __name__ == "__main__":
    sys.exit(main())
