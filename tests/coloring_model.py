"""numpy model of the graph colouring (include/mgx/color_fused.hpp): the definition the fused path and the
operator path must both reproduce bit for bit.

    fmix32(h):  h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35; h ^= h >> 16      (uint32, wrapping)
    salt_i   = fmix32(seed + 0x9E3779B9 * (i + 1))
    key_i(v) = fmix32(v ^ salt_i)
    round i, every v uncoloured at the start of the round:
      lo = min key_i(u) over uncoloured u in N(v) (UINT32_MAX if none), hi = max (0 if none)
      key_i(v) <= lo -> 2i + 1;  else key_i(v) >= hi -> 2i + 2
    stop after max_iter rounds or when none is left; max_iter <= 0: until none is left.
"""
import numpy as np

SEED = 15485863
MAX_ITER = 10
U32_MAX = np.uint32(0xFFFFFFFF)


def fmix32(h):
    h = np.array(h, dtype=np.uint32, copy=True)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def salt(seed, i):
    return fmix32((int(seed) + 0x9E3779B9 * (i + 1)) & 0xFFFFFFFF)


def keys(n, s):
    return fmix32(np.arange(n, dtype=np.uint32) ^ np.uint32(s))


def color(row_offsets, col_indices, seed=SEED, max_iter=MAX_ITER):
    """-> (colours int32[n], active vertices at the start of every round run int64[rounds], vertices left uncoloured)"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    n = len(ro) - 1
    half = (n + 1) // 2
    cap = min(max_iter, half) if max_iter > 0 else half
    colours = np.zeros(n, dtype=np.int32)
    trace = []
    act = np.arange(n, dtype=np.int64)          # the active vertices, and the entries of their rows
    e_ro, e_ci = ro - ro[0], ci[ro[0]:ro[-1]]
    for i in range(cap):
        if len(act) == 0:
            break
        trace.append(len(act))
        k = keys(n, salt(seed, i))
        deg = np.diff(e_ro)
        uncoloured = np.zeros(n, dtype=bool)
        uncoloured[act] = True
        kc = k[e_ci]
        unc = uncoloured[e_ci]
        lo = np.full(len(act), U32_MAX, dtype=np.uint32)
        hi = np.zeros(len(act), dtype=np.uint32)
        rows = deg > 0                          # empty rows keep the identities (reduceat would hand them a neighbour's value)
        if rows.any():
            starts = e_ro[:-1][rows]
            lo[rows] = np.minimum.reduceat(np.where(unc, kc, U32_MAX), starts)
            hi[rows] = np.maximum.reduceat(np.where(unc, kc, np.uint32(0)), starts)
        kv = k[act]
        low = kv <= lo
        high = ~low & (kv >= hi)
        colours[act[low]] = 2 * i + 1
        colours[act[high]] = 2 * i + 2
        keep = ~(low | high)
        e_ci = e_ci[np.repeat(keep, deg)]
        e_ro = np.concatenate([[0], np.cumsum(deg[keep])])
        act = act[keep]
    return colours, np.array(trace, dtype=np.int64), len(act)


def conflicts(row_offsets, col_indices, colours):
    """entries (v, u), u != v, whose ends carry the same non-zero colour"""
    ro = np.asarray(row_offsets, dtype=np.int64)
    ci = np.asarray(col_indices, dtype=np.int64)
    c = np.asarray(colours)
    rows = np.repeat(np.arange(len(ro) - 1, dtype=np.int64), np.diff(ro))
    return int(((rows != ci) & (c[rows] == c[ci]) & (c[rows] != 0)).sum())


def csr(n, src, dst, symmetric=True):
    """CSR of the pairs (row src, neighbour dst), rows and neighbours ascending; symmetric: the swapped copies too"""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if symmetric:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    order = np.lexsort((dst, src))
    ro = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=ro[1:])
    return ro.astype(np.int32), dst[order].astype(np.int32)


def clique(n):
    v = np.arange(n)
    s, d = np.meshgrid(v, v, indexing="ij")
    m = s != d
    return csr(n, s[m], d[m], symmetric=False)
