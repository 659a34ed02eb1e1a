#!/usr/bin/env python3
"""How consecutive bet steps overlap on the GPU, from a rocprofv3 --kernel-trace database (rocpd sqlite) of a C2 run.
Steps are matched by dispatch order: the j-th k_rank_lean belongs to the j-th k_select_mx3 and precedes the (j+1)-th k_hist_i8.
usage: step_overlap.py results.db [--last N]   (N: only the last N steps, i.e. the timed ones; default 20)"""
import sqlite3
import sys

import numpy as np


def spans(c, pat):
    rows = c.execute("select start, end from kernels where name like ? order by start", ("%" + pat + "%",)).fetchall()
    return np.array(rows, dtype=np.float64).reshape(-1, 2) / 1e3          # ns -> us


def main():
    path = sys.argv[1]
    last = int(sys.argv[sys.argv.index("--last") + 1]) if "--last" in sys.argv else 20
    c = sqlite3.connect(path)
    sel, rank, hist, guess = (spans(c, p) for p in ("k_select_mx3", "k_rank_lean", "k_hist_i8", "k_guess_direct"))
    n = min(len(sel), len(rank), len(hist), len(guess))
    sel, rank, hist, guess = sel[-n:], rank[-n:], hist[-n:], guess[-n:]
    k = min(last, n)
    j = np.arange(n - k, n - 1)                                            # step j and step j + 1, both timed
    print("steps in trace %d, pairs analysed %d (the last %d steps)" % (n, len(j), k))
    dur = lambda s: s[n - k:, 1] - s[n - k:, 0]
    for name, s in (("k_hist_i8", hist), ("k_guess_direct", guess), ("k_select_mx3", sel), ("k_rank_lean", rank)):
        d = dur(s)
        print("  %-16s avg %8.2f us  median %8.2f us" % (name, d.mean(), np.median(d)))
    ov_h = rank[j, 1] - hist[j + 1, 0]        # > 0: step j + 1's sampled pass started before step j's rank ended
    ov_g = rank[j, 1] - guess[j + 1, 0]
    gap = sel[j + 1, 0] - sel[j, 1]           # the select's critical path: idle between one select's end and the next one's start
    period = sel[j + 1, 0] - sel[j, 0]
    print("  next k_hist_i8 starts before this k_rank_lean ends: %d of %d pairs (median lead %.1f us)" % ((ov_h > 0).sum(), len(j), np.median(ov_h)))
    print("  next k_guess_direct starts before this k_rank_lean ends: %d of %d pairs (median lead %.1f us)" % ((ov_g > 0).sum(), len(j), np.median(ov_g)))
    print("  select end -> next select start: median %.1f us (min %.1f, max %.1f)" % (np.median(gap), gap.min(), gap.max()))
    print("  select start -> next select start (step period): median %.1f us, mean %.1f us" % (np.median(period), period.mean()))


if __name__ == "__main__":
    main()
