"""Updates of a database DIRECTORY (`embeddings`, `landmarkValue`, `landmarkKey`, `songList.txt`) without a rebuild:
numpy and faissio only -- no torch, no GPU.

    add_songs     the new rows are appended in place to `embeddings` and behind the header of `landmarkValue`
                  (O(new rows)), the longer `songList.txt` and `landmarkKey` are written, the header count rewritten.
    remove_songs  `embeddings` and `landmarkValue` are written again without the songs' rows, streamed in bounded pieces
                  (never a whole file in memory; O(database) file I/O -- there is no way to cut rows out of the middle of
                  a file), `landmarkKey` gets 0 at those ids ("this id has no rows", what the builder writes for an
                  unreadable file), `songList.txt` stays as it is: every song keeps its id.

An updated directory is byte for byte the one a build of the same rows writes.

Crash rule.  At every instant the directory is one `Database()` opens (old or new state), or one that `repair` turns
into exactly the old or exactly the new state:
    1. everything new is written beside the old (`*.new`, fsynced); for add the rows go behind the counted rows, where no
       reader looks (readers take the row count from `landmarkKey` / the `landmarkValue` header);
    2. `dbupdate.journal` is written: the operation and the final counts.  This is the commit;
    3. the new files are renamed into place, the header count is rewritten;
    4. the journal is deleted.
`repair` WITHOUT a journal rolls back: row files are truncated to sum(landmarkKey) rows, the header is set to that count,
`*.new` are deleted.  WITH a journal it rolls forward: steps 3 and 4 again, each of them idempotent.  `Database()` refuses
a directory with a journal.  STEPS_ADD / STEPS_REMOVE name the steps; FAIL_AFTER (tests only) raises InjectedFailure after
the named one.
"""
import json
import os
import struct

import numpy as np

from . import faissio

JOURNAL = "dbupdate.journal"
ROW_FILES = ("embeddings", "landmarkValue")
NEW_FILES = ("embeddings", "landmarkValue", "landmarkKey", "songList.txt")
PIECE_BYTES = 64 << 20

# after each of these steps a crash leaves ...                        (repair gives)
STEPS_ADD = ("rows",          # the rows behind the counted rows            old
             "new",           # + landmarkKey.new, songList.txt.new         old
             "journal",       # + the journal: committed                    new
             "header",        # landmarkValue counts the new rows           new
             "key",           # landmarkKey.new in place                    new
             "songlist",      # songList.txt.new in place                   new
             "done")          # journal deleted: the new state              new (nothing to repair)
STEPS_REMOVE = ("new",        # embeddings.new, landmarkValue.new, landmarkKey.new    old
                "journal",    # + the journal: committed                    new
                "embeddings", "value", "key",      # renamed into place, one by one       new
                "done")       # journal deleted                             new (nothing to repair)
STATE_AFTER = {"add": dict(zip(STEPS_ADD, ("old", "old", "new", "new", "new", "new", "new"))),
               "remove": dict(zip(STEPS_REMOVE, ("old", "new", "new", "new", "new", "new")))}

FAIL_AFTER = None       # test hook: the name of a step


class InjectedFailure(RuntimeError):
    pass


class DbFilesError(RuntimeError):
    pass


def _step(name):
    if FAIL_AFTER == name:
        raise InjectedFailure(name)


def _p(db, name):
    return os.path.join(db, name)


def _fsync_dir(db):
    fd = os.open(db, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def _write_synced(path, data):
    with open(path, "wb") as f:
        f.write(data)
        f.flush()
        os.fsync(f.fileno())


def _rename(db, name):
    """name.new -> name; nothing to do when it has been renamed already"""
    if os.path.exists(_p(db, name + ".new")):
        os.replace(_p(db, name + ".new"), _p(db, name))
        _fsync_dir(db)


def read_key(db):
    return np.fromfile(_p(db, "landmarkKey"), dtype=np.int32)


def read_names(db):
    with open(_p(db, "songList.txt"), "r", encoding="utf8") as fin:
        return [ln[:-1] if ln.endswith("\n") else ln for ln in fin]


def _value_header(path):
    """-> (d, n, metric) of a flat index file"""
    with open(path, "rb") as f:
        head = f.read(faissio.HEADER_BYTES)
    if len(head) < faissio.HEADER_BYTES or head[:4] not in (b"IxFI", b"IxF2"):
        raise DbFilesError("%s is not a flat index written by the builder" % path)
    d, n, _, _, _, metric = struct.unpack("<iqqqBi", head[4:4 + 4 + 8 * 3 + 1 + 4])
    return d, n, metric


def row_dim(db):
    """d of the directory: the landmarkValue header, else configs.json"""
    if os.path.exists(_p(db, "landmarkValue")):
        return _value_header(_p(db, "landmarkValue"))[0]
    with open(_p(db, "configs.json"), "r") as fin:
        return int(json.load(fin)["model"]["d"])


def _row_file_layout(db):
    """[(name, bytes before row 0)] of the row files the directory has"""
    out = []
    if os.path.exists(_p(db, "embeddings")):
        out.append(("embeddings", 0))
    if os.path.exists(_p(db, "landmarkValue")):
        out.append(("landmarkValue", faissio.HEADER_BYTES))
    return out


def write_database(db, names, emb, rows_per_song):
    """The four files written in one go, as the builder writes them (the tests' reference)."""
    emb = np.ascontiguousarray(emb, dtype="<f4")
    os.makedirs(db, exist_ok=True)
    emb.tofile(_p(db, "embeddings"))
    faissio.write_index_flat(_p(db, "landmarkValue"), emb)
    np.asarray(rows_per_song, dtype=np.int32).tofile(_p(db, "landmarkKey"))
    with open(_p(db, "songList.txt"), "w", encoding="utf8", newline="\n") as f:
        f.write("".join(n + "\n" for n in names))


# ---------------------------------------------------------------------------------------------------- check / repair
def problems(db):
    """What keeps the directory from being a clean database, as a list of lines (empty: clean).  Reads only."""
    out = []
    if os.path.exists(_p(db, JOURNAL)):
        try:
            j = read_journal(db)
            out.append("journal: an interrupted '%s' (committed: %d rows, %d songs)" % (j["op"], j["rows"], j["songs"]))
        except (ValueError, KeyError) as x:
            out.append("journal: unreadable (%s)" % x)
    for name in NEW_FILES:
        if os.path.exists(_p(db, name + ".new")):
            out.append("%s.new: left by an interrupted update" % name)
    if os.path.exists(_p(db, JOURNAL + ".tmp")):
        out.append("%s.tmp: left by an interrupted update" % JOURNAL)
    key = read_key(db)
    rows = int(key.astype(np.int64).sum())
    n_names = len(read_names(db))
    if n_names != key.shape[0]:
        out.append("songList.txt has %d songs, landmarkKey %d" % (n_names, key.shape[0]))
    d = row_dim(db)
    for name, head in _row_file_layout(db):
        size = os.path.getsize(_p(db, name))
        if size != head + rows * d * 4:
            out.append("%s holds %d bytes, %d rows of %d floats are %d" % (name, size, rows, d, head + rows * d * 4))
        if head:
            _, n, _ = _value_header(_p(db, name))
            if n != rows:
                out.append("%s counts %d rows, landmarkKey %d" % (name, n, rows))
    return out


def read_journal(db):
    with open(_p(db, JOURNAL), "r") as fin:
        j = json.load(fin)
    if j.get("op") not in ("add", "remove"):
        raise ValueError("unknown operation %r" % (j.get("op"),))
    return {"op": j["op"], "rows": int(j["rows"]), "songs": int(j["songs"]), "d": int(j["d"])}


def _write_journal(db, op, rows, songs, d):
    _write_synced(_p(db, JOURNAL + ".tmp"), json.dumps({"op": op, "rows": int(rows), "songs": int(songs), "d": int(d)}).encode())
    os.replace(_p(db, JOURNAL + ".tmp"), _p(db, JOURNAL))
    _fsync_dir(db)


def _set_rows(db, rows, d):
    """row files cut to `rows` rows, the flat index counting them (both idempotent)"""
    for name, head in _row_file_layout(db):
        path = _p(db, name)
        with open(path, "r+b") as f:
            if os.path.getsize(path) > head + rows * d * 4:
                f.truncate(head + rows * d * 4)
            if head:
                metric = _value_header(path)[2]
                faissio.write_header(f, d, rows, metric)
            f.flush()
            os.fsync(f.fileno())


def _forward_add(db, j, steps=True):
    _set_rows(db, j["rows"], j["d"])
    if steps:
        _step("header")
    _rename(db, "landmarkKey")
    if steps:
        _step("key")
    _rename(db, "songList.txt")
    if steps:
        _step("songlist")
    os.remove(_p(db, JOURNAL))
    _fsync_dir(db)
    if steps:
        _step("done")


def _forward_remove(db, j, steps=True):
    for name, step in (("embeddings", "embeddings"), ("landmarkValue", "value"), ("landmarkKey", "key")):
        _rename(db, name)
        if steps:
            _step(step)
    os.remove(_p(db, JOURNAL))
    _fsync_dir(db)
    if steps:
        _step("done")


def repair(db):
    """Rolls an interrupted update forward (journal present) or back (none) -> the lines `problems` gave before."""
    found = problems(db)
    if os.path.exists(_p(db, JOURNAL)):
        j = read_journal(db)
        (_forward_add if j["op"] == "add" else _forward_remove)(db, j, steps=False)
    else:
        for name in NEW_FILES:
            if os.path.exists(_p(db, name + ".new")):
                os.remove(_p(db, name + ".new"))
        if os.path.exists(_p(db, JOURNAL + ".tmp")):
            os.remove(_p(db, JOURNAL + ".tmp"))
        _set_rows(db, int(read_key(db).astype(np.int64).sum()), row_dim(db))
        _fsync_dir(db)
    return found


def _require_clean(db):
    bad = problems(db)
    if bad:
        raise DbFilesError("%s is not a clean database (run `dbupdate.py check --repair`):\n  %s" % (db, "\n  ".join(bad)))


# ---------------------------------------------------------------------------------------------------- add
def add_songs(db, names, emb, rows_per_song):
    """names: one line of songList.txt per new song; emb float32 [sum(rows_per_song), d]; rows_per_song may hold zeros.
    -> (id of the first new song, one past the last)"""
    rps = np.asarray(rows_per_song, dtype=np.int64).reshape(-1)
    names = list(names)
    if len(names) != rps.shape[0] or (rps < 0).any() or any("\n" in n for n in names):
        raise ValueError("add_songs: %d names, %d row counts (all >= 0, names without line breaks)" % (len(names), rps.shape[0]))
    _require_clean(db)
    d = row_dim(db)
    emb = np.ascontiguousarray(emb, dtype="<f4").reshape(-1, d)
    if emb.shape[0] != int(rps.sum()):
        raise ValueError("add_songs: the songs have %d rows, emb has %d" % (int(rps.sum()), emb.shape[0]))
    key = read_key(db)
    rows0 = int(key.astype(np.int64).sum())
    rows1 = rows0 + emb.shape[0]
    # 1. the rows, behind the counted ones
    for name, head in _row_file_layout(db):
        with open(_p(db, name), "r+b") as f:
            f.seek(head + rows0 * d * 4)
            if emb.size:
                f.write(memoryview(emb).cast("B"))
            f.flush()
            os.fsync(f.fileno())
    _step("rows")
    # 2. the longer key and song list, beside the old
    _write_synced(_p(db, "landmarkKey.new"), np.concatenate([key, rps.astype(np.int32)]).tobytes())
    with open(_p(db, "songList.txt"), "rb") as f:
        old = f.read()
    if old and not old.endswith(b"\n"):
        old += b"\n"
    _write_synced(_p(db, "songList.txt.new"), old + "".join(n + "\n" for n in names).encode("utf8"))
    _step("new")
    # 3. the commit, 4. into place
    j = {"op": "add", "rows": rows1, "songs": key.shape[0] + len(names), "d": d}
    _write_journal(db, **j)
    _step("journal")
    _forward_add(db, j)
    return key.shape[0], key.shape[0] + len(names)


# ---------------------------------------------------------------------------------------------------- remove
def kept_runs(key, ids):
    """-> [(first row, rows)] of the rows that stay, neighbouring songs joined, and the new key"""
    key = np.asarray(key, dtype=np.int32)
    new_key = key.copy()
    new_key[np.asarray(ids, dtype=np.int64)] = 0
    pos = np.pad(np.cumsum(key, dtype=np.int64), (1, 0))
    runs = []
    for s in np.flatnonzero(new_key):
        lo, n = int(pos[s]), int(key[s])
        if runs and runs[-1][0] + runs[-1][1] == lo:
            runs[-1][1] += n
        else:
            runs.append([lo, n])
    return [tuple(r) for r in runs], new_key


def _copy_runs(src, head, dst, runs, d, piece_rows):
    """the runs' rows of file src (rows start at byte `head`) appended to the open file dst, at most piece_rows at a time"""
    with open(src, "rb") as f:
        for lo, n in runs:
            f.seek(head + lo * d * 4)
            while n:
                m = min(n, piece_rows)
                buf = f.read(m * d * 4)
                if len(buf) != m * d * 4:
                    raise DbFilesError("%s is shorter than landmarkKey says" % src)
                dst.write(buf)
                n -= m


def remove_songs(db, ids, piece_rows=None):
    """ids: songs that lose their rows (any order, duplicates allowed).  piece_rows: rows per piece of the streaming copy
    (default: 64 MB)."""
    _require_clean(db)
    key = read_key(db)
    ids = np.asarray(ids, dtype=np.int64).reshape(-1)
    if ids.size and (ids.min() < 0 or ids.max() >= key.shape[0]):
        raise ValueError("remove_songs: ids outside 0..%d" % (key.shape[0] - 1))
    d = row_dim(db)
    piece_rows = max(1, PIECE_BYTES // (d * 4)) if piece_rows is None else max(1, int(piece_rows))
    runs, new_key = kept_runs(key, ids)
    rows1 = int(new_key.astype(np.int64).sum())
    # 1. everything new beside the old
    for name, head in _row_file_layout(db):
        with open(_p(db, name + ".new"), "wb") as f:
            if head:
                f.write(faissio._header(d, rows1, _value_header(_p(db, name))[2]))
            _copy_runs(_p(db, name), head, f, runs, d, piece_rows)
            f.flush()
            os.fsync(f.fileno())
    _write_synced(_p(db, "landmarkKey.new"), new_key.tobytes())
    _step("new")
    # 2. the commit, 3. into place
    j = {"op": "remove", "rows": rows1, "songs": key.shape[0], "d": d}
    _write_journal(db, **j)
    _step("journal")
    _forward_remove(db, j)
    return new_key
