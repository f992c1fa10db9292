#!/usr/bin/env python
"""Database updates: `python dbupdate.py add <music list> <db> [--allow-duplicates]`, `python dbupdate.py remove <song list> <db>`,
`python dbupdate.py check <db> [--repair]` add songs to and remove songs from a database directory without a rebuild
(pfann_amd/dbupdate.py)."""
import sys

if __name__ == "__main__":
    from pfann_amd.dbupdate import main
    sys.exit(main(sys.argv))
