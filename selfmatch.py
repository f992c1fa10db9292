#!/usr/bin/env python
"""Self-match: `python selfmatch.py <db dir> <result.tsv> [--window N] [--hop N] [--min-score X] [--min-windows N] [--max-gap N]
[--songs A:B] [--topk K]` finds the songs of a database that contain (a stretch of) another (pfann_amd/selfmatch.py)."""
import sys

if __name__ == "__main__":
    from pfann_amd.selfmatch import main
    sys.exit(main(sys.argv))
