"""Rows by length, as include/mgx/row_bodies.hpp sorts them: the one statement of the classes that the models of the
label propagation, Louvain, multi-source BFS and the random walks' setup count their bins with."""
import numpy as np

NONE, LANE, WAVE, LONG = 0, 1, 2, 3
KEYS = ("none", "short", "wave", "long")


def classes(lengths, short_max, wave_max):
    """row_cuts_t::body_of of every length.  wave_max as the kernel gets it: every path raises it to short_max"""
    ln = np.asarray(lengths, dtype=np.int64)
    wave_max = max(wave_max, short_max)
    return np.where(ln == 0, NONE, np.where(ln <= short_max, LANE, np.where(ln <= wave_max, WAVE, LONG)))


def bodies(lengths, short_max, wave_max, seg=None):
    """-> {"none", "short", "wave", "long"}: the rows per class; with seg also "segments": the long rows' pieces of seg entries"""
    ln = np.asarray(lengths, dtype=np.int64)
    cl = classes(ln, short_max, wave_max)
    out = {k: int((cl == c).sum()) for c, k in enumerate(KEYS)}
    if seg is not None:
        out["segments"] = int(((ln[cl == LONG] + seg - 1) // seg).sum())
    return out
