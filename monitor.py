#!/usr/bin/env python
"""Monitor mode: `python monitor.py <recording list> <db dir> <result file> [--window N] [--hop N] [--min-score X] [--max-gap N]`
says what played when in long recordings (pfann_amd/monitor.py)."""
import sys

if __name__ == "__main__":
    from pfann_amd.monitor import main
    sys.exit(main(sys.argv))
