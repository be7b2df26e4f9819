"""Reference for the cd histograms (dg_corr_cd_hist), numpy only: the bin rule, and the edge-mass bound the GPU tests hold the
library's counts to.

Bin rule: torch.histc's over [lo, hi] with `bins` uniform bins - bin = floor((v - lo) * bins / (hi - lo)), v == hi in the last bin -
with one difference: a value outside [lo, hi] counts in the nearest end bin instead of being dropped, so the counts sum to v.size.

Edge-mass bound.  Let C(e) be the number of elements below interior bin edge e (the running sum of the bins left of it).  Two sets
of values that differ by at most `delta` per element can disagree in C(e) only through elements within `delta` of e, so
|C_a(e) - C_b(e)| <= #{b : |b - e| <= delta}: a bound computed from ONE of the two sets, tight wherever that set has no mass at an edge.
"""
import numpy as np


def clamped_histc(values, bins, lo, hi):
    """int64 (bins,) counts of `values` (any shape) under the rule above; arithmetic in float64."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    b = np.floor((v - lo) * bins / (hi - lo))
    return np.bincount(np.clip(b, 0, bins - 1).astype(np.int64), minlength=bins).astype(np.int64)


def interior_edges(bins, lo, hi):
    """The bins - 1 edges between neighbouring bins."""
    return lo + (hi - lo) * np.arange(1, bins, dtype=np.float64) / bins


def below_edges(counts):
    """C(e) for every interior edge from a histogram: the running sums of the bins left of the edge."""
    return np.cumsum(np.asarray(counts, dtype=np.int64))[:-1]


def edge_mass(values, bins, lo, hi, delta):
    """int64 (bins - 1,): how many of `values` lie within `delta` of each interior edge (both ends included)."""
    v = np.sort(np.asarray(values, dtype=np.float64).reshape(-1))
    e = interior_edges(bins, lo, hi)
    return (np.searchsorted(v, e + delta, side="right") - np.searchsorted(v, e - delta, side="left")).astype(np.int64)
