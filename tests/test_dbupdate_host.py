"""Database updates, the parts that need no GPU: pfann_amd/dbfiles.py (add, remove, the crash rule and its repair) and the
argument rules of dbupdate.py.  Every comparison is equality of bytes."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from pfann_amd import dbfiles

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ("embeddings", "landmarkValue", "landmarkKey", "songList.txt")
D = 16
KEY = [5, 0, 7, 3, 1, 0, 9, 4]          # two songs without rows, as the builder writes unreadable files


def make(tmp, name, key=KEY, seed=1):
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((int(sum(key)), D)).astype(np.float32)
    names = ["/music/%s_%02d.wav" % (name, i) for i in range(len(key))]
    db = str(tmp / name)
    dbfiles.write_database(db, names, emb, key)
    return db, names, emb


def snapshot(db):
    return {f: open(os.path.join(db, f), "rb").read() for f in sorted(os.listdir(db))}


def test_add_equals_the_files_written_in_one_go(tmp_path):
    db, names, emb = make(tmp_path, "a")
    rng = np.random.default_rng(2)
    key_b = [4, 0, 6]
    emb_b = rng.standard_normal((10, D)).astype(np.float32)
    names_b = ["/music/b_%d.wav" % i for i in range(3)]
    assert dbfiles.add_songs(db, names_b, emb_b, key_b) == (len(KEY), len(KEY) + 3)
    ref = str(tmp_path / "ref")
    dbfiles.write_database(ref, names + names_b, np.concatenate([emb, emb_b]), KEY + key_b)
    assert snapshot(db) == snapshot(ref) and sorted(snapshot(db)) == sorted(FILES)
    assert dbfiles.problems(db) == []
    # a second add, of songs without rows only, and one of nothing
    dbfiles.add_songs(db, ["x", "y"], np.zeros((0, D), np.float32), [0, 0])
    dbfiles.add_songs(db, [], np.zeros((0, D), np.float32), [])
    dbfiles.write_database(ref, names + names_b + ["x", "y"], np.concatenate([emb, emb_b]), KEY + key_b + [0, 0])
    assert snapshot(db) == snapshot(ref)
    with pytest.raises(ValueError):
        dbfiles.add_songs(db, ["z"], emb_b, [9])             # 9 rows announced, 10 brought
    assert snapshot(db) == snapshot(ref)


REMOVE_CASES = {"first": [0], "last": [7], "adjacent": [2, 3], "separated": [2, 6], "no_rows": [1], "every": list(range(8)),
                "any_order_twice": [6, 0, 6]}


@pytest.mark.parametrize("case", sorted(REMOVE_CASES))
@pytest.mark.parametrize("piece_rows", [None, 2])          # 2: the streaming copy takes several pieces per run
def test_remove_keeps_the_other_rows(tmp_path, case, piece_rows):
    db, names, emb = make(tmp_path, "a")
    ids = REMOVE_CASES[case]
    before = snapshot(db)
    dbfiles.remove_songs(db, ids, piece_rows=piece_rows)
    key = np.asarray(KEY, np.int32)
    pos = np.pad(np.cumsum(key), (1, 0))
    keep = np.ones(emb.shape[0], bool)
    for s in ids:
        keep[pos[s]:pos[s + 1]] = False
    new_key = key.copy()
    new_key[ids] = 0
    ref = str(tmp_path / "ref")
    dbfiles.write_database(ref, names, emb[keep], new_key)
    after = snapshot(db)
    assert after == snapshot(ref)
    assert after["songList.txt"] == before["songList.txt"]
    assert np.frombuffer(after["embeddings"], np.float32).reshape(-1, D).tobytes() == emb[keep].tobytes()
    assert (np.frombuffer(after["landmarkKey"], np.int32)[ids] == 0).all()
    assert dbfiles.problems(db) == []
    with pytest.raises(ValueError):
        dbfiles.remove_songs(db, [8])
    assert snapshot(db) == after


def _crash(db, step, op):
    dbfiles.FAIL_AFTER = step
    try:
        with pytest.raises(dbfiles.InjectedFailure):
            op(db)
    finally:
        dbfiles.FAIL_AFTER = None


def _check_cli(db, *more):
    return subprocess.run([sys.executable, os.path.join(REPO, "dbupdate.py"), "check", db] + list(more), capture_output=True,
                          text=True, timeout=120, cwd=REPO)


@pytest.mark.parametrize("kind,step", [("add", s) for s in dbfiles.STEPS_ADD] + [("remove", s) for s in dbfiles.STEPS_REMOVE])
def test_a_crash_after_any_step_is_repaired_to_the_old_or_the_new_state(tmp_path, kind, step):
    """dbfiles.STATE_AFTER states, per step, which of the two it is: old before the journal is written, new from then on."""
    db, names, emb = make(tmp_path, "a")
    rng = np.random.default_rng(3)
    emb_b = rng.standard_normal((6, D)).astype(np.float32)
    if kind == "add":
        def op(path):
            dbfiles.add_songs(path, ["n0", "n1", "n2"], emb_b, [2, 0, 4])
    else:
        def op(path):
            dbfiles.remove_songs(path, [0, 3, 6], piece_rows=3)
    old = snapshot(db)
    done = str(tmp_path / "done")
    shutil.copytree(db, done)
    op(done)
    new = snapshot(done)
    assert old != new
    _crash(db, step, op)
    want = {"old": old, "new": new}[dbfiles.STATE_AFTER[kind][step]]
    crashed = snapshot(db)
    clean = crashed == want
    # `check` alone reports and changes nothing
    r = _check_cli(db)
    assert r.returncode == (0 if clean else 1), r.stdout + r.stderr
    assert snapshot(db) == crashed
    assert (dbfiles.problems(db) == []) == clean
    if not clean:
        with pytest.raises(dbfiles.DbFilesError):           # no update on top of an interrupted one
            op(db)
        assert snapshot(db) == crashed
    r = _check_cli(db, "--repair")
    assert r.returncode == 0, r.stdout + r.stderr
    assert snapshot(db) == want
    assert _check_cli(db).returncode == 0
    # the repair is idempotent, and the directory takes the update now
    dbfiles.repair(db)
    assert snapshot(db) == want
    if want is old:
        op(db)
        assert snapshot(db) == new


def test_repair_is_idempotent_at_every_step_of_its_own(tmp_path):
    """a roll forward interrupted in turn: the journal stays until the last step, every step can run twice"""
    db, names, emb = make(tmp_path, "a")
    done = str(tmp_path / "done")
    shutil.copytree(db, done)
    dbfiles.remove_songs(done, [2])
    _crash(db, "journal", lambda p: dbfiles.remove_songs(p, [2]))
    j = dbfiles.read_journal(db)
    for step in ("embeddings", "value", "key"):
        dbfiles.FAIL_AFTER = step
        try:
            with pytest.raises(dbfiles.InjectedFailure):
                dbfiles._forward_remove(db, j)
        finally:
            dbfiles.FAIL_AFTER = None
        assert os.path.exists(os.path.join(db, dbfiles.JOURNAL))
    dbfiles.repair(db)
    assert snapshot(db) == snapshot(done)


CLI = """
import sys
sys.path.insert(0, %r)
from pfann_amd import dbupdate
rc = dbupdate.main(["dbupdate.py"] + sys.argv[1:])
print("RC", rc, "torch" in sys.modules)
"""


def test_cli_refusals_write_nothing_and_do_not_import_torch(tmp_path):
    db, names, emb = make(tmp_path, "a")
    script = tmp_path / "cli.py"
    script.write_text(CLI % REPO)
    before = snapshot(db)
    env = {k: v for k, v in os.environ.items() if k != "PFANN_GPUS"}

    def run(args, **more):
        r = subprocess.run([sys.executable, str(script)] + args, capture_output=True, text=True, timeout=120, cwd=str(tmp_path),
                           env=dict(env, **more))
        assert snapshot(db) == before
        return r.stdout.split()[-3:], r.stderr

    dup = tmp_path / "dup.txt"
    dup.write_text("/music/new.wav\n" + names[3] + "\n")
    out, err = run(["add", str(dup), db])
    assert out == ["RC", "2", "False"] and names[3] in err
    fresh = tmp_path / "fresh.txt"
    fresh.write_text("/music/new.wav\n")
    out, err = run(["add", str(fresh), db], PFANN_GPUS="2")
    assert out == ["RC", "2", "False"] and "PFANN_GPUS" in err
    unknown = tmp_path / "unknown.txt"
    unknown.write_text(names[0] + "\n/music/nobody.wav\n")
    out, err = run(["remove", str(unknown), db])
    assert out == ["RC", "2", "False"] and "nobody" in err
    badid = tmp_path / "badid.txt"
    badid.write_text("#1\n#8\n")
    out, err = run(["remove", str(badid), db])
    assert out == ["RC", "2", "False"] and "#8" in err
    out, err = run(["check", db])
    assert out == ["RC", "0", "False"]
    # and the one that works: a path and an id, through the root script
    ok = tmp_path / "ok.txt"
    ok.write_text(names[2] + "\n#6\n")
    r = subprocess.run([sys.executable, os.path.join(REPO, "dbupdate.py"), "remove", str(ok), db], capture_output=True, text=True,
                       timeout=120, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    ref = str(tmp_path / "ref")
    shutil.copytree(str(tmp_path / "a"), ref, dirs_exist_ok=True)
    for f, data in before.items():
        open(os.path.join(ref, f), "wb").write(data)
    dbfiles.remove_songs(ref, [2, 6])
    assert snapshot(db) == snapshot(ref) != before


def test_database_refuses_a_directory_with_a_journal(tmp_path):
    from pfann_amd.database import Database
    from pfann_amd.lib import PfannError
    db, names, emb = make(tmp_path, "a")
    _crash(db, "journal", lambda p: dbfiles.remove_songs(p, [0]))
    with pytest.raises(PfannError, match="dbupdate.py check .* --repair"):
        Database(db, {"top_k": 10}, 0.5, d=D)
