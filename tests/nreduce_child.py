"""The neighbour-reduce's checks on a GPU, shared by tests/test_gpu_nreduce_paths.py (in-process) and by the child interpreter that
file starts for the switches the library reads ONCE PER PROCESS (MGX_NR_SLICED, MGX_NR_SUBSET: function-local statics of
include/gunrock/neighborhood.hxx):

    python -m tests.nreduce_child sliced0|subset0      (with the switch in the environment)

runs check_full and check_subsets for every operator on the edge graph and prints ONE JSON line: the bodies mgx_graph_nr_last_call
reported and the special degrees that were compared.  A failed check is an AssertionError: a traceback and a non-zero exit status.

Every comparison is against nreduce_cases.reduce_f64: exact for integer min / max and for float sums of small integers, within
nreduce_cases.sum_bound (derived from float32's unit roundoff, atol 0) for real-valued sums."""
import json
import sys

import numpy as np

from tests import nreduce_cases as nc

SENTINEL = {"f32_plus": -777.0, "i32_min": 12345, "i32_max": 12345}          # what reduced[] holds before a call: no input produces it


class Case:
    """one CPU graph, its value sets and every reference computed on it (once: shared by the tests, never modified)"""

    def __init__(self, ro, ci, special=None, seed=0):
        self.ro, self.ci, self.special = ro, ci, special or {}
        self.n, self.m = len(ro) - 1, len(ci)
        self.deg = np.diff(ro).astype(np.int64)
        self.seed = seed
        self._vals, self._fold, self._front = {}, {}, None

    def values(self, kind):
        if kind not in self._vals:
            rng = np.random.default_rng(self.seed * 16 + len(self._vals))
            make = {"small": lambda: nc.small_int_values(self.n, rng), "real": lambda: nc.real_values(self.n, rng),
                    "any": lambda: nc.int_values(self.n, rng, 0), "pos": lambda: nc.int_values(self.n, rng, 1),
                    "neg": lambda: nc.int_values(self.n, rng, -1)}[kind]
            self._vals[kind] = make()
        return self._vals[kind]

    def frontiers(self):
        if self._front is None:
            f = dict(nc.subset_frontiers(self.n, self.special, self.seed))
            f["full"] = np.arange(self.n, dtype=np.int32)
            f["permuted"] = np.random.default_rng(self.seed + 7).permutation(self.n).astype(np.int32)
            dup = f["inside"].copy(); dup[5] = dup[4]                   # ascending, not STRICTLY
            f["duplicate"] = dup
            self._front = f
        return self._front

    def want(self, fkey, ids, vkey, vals, op, identity):
        """(reduced by frontier position, bound or None, edges); cached under (fkey, vkey, op) when both keys are given"""
        key = (fkey, vkey, op)
        hit = self._fold.get(key) if fkey and vkey else None
        if hit is None:
            out, edges = nc.reduce_f64(self.ro, self.ci, ids, vals, 0, op)
            bound = nc.sum_bound(self.ro, self.ci, ids, vals) if vkey == "real" or (op == "f32_plus" and vkey is None) else None
            hit = (out, self.deg[ids] == 0, bound, edges)
            if fkey and vkey:
                self._fold[key] = hit
        out, empty, bound, edges = hit
        out = out.copy()
        out[empty] = np.float64(np.float32(identity)) if op == "f32_plus" else int(identity)
        return out, bound, edges


_CASES = {}


def edge_case(long_min=64):
    if long_min not in _CASES:
        ro, ci, special = nc.edge_graph(long_min, seed=long_min)
        _CASES[long_min] = Case(ro, ci, special, seed=long_min)
    return _CASES[long_min]


def value_sets(op, identities="neutral"):
    """[(value kind, identity, exact)]; identities: "neutral", or "other" -- identities that are NOT the operator's neutral element
    (f32_plus: 100.0 and the "no neighbours" sentinel -1.0; i32_min: 0 under all-positive values; i32_max: 0 under all-negative ones)"""
    if identities == "neutral":
        return {"f32_plus": [("small", 0.0, True), ("real", 0.0, False)], "i32_min": [("any", nc.INT_MAX, True)],
                "i32_max": [("any", nc.INT_MIN, True)]}[op]
    return {"f32_plus": [("small", 100.0, True), ("small", -1.0, True), ("real", -1.0, False)], "i32_min": [("pos", 0, True)],
            "i32_max": [("neg", 0, True)]}[op]


def reduce_on_gpu(ctx, g, ids, vals, identity, op, push=True):
    """one mgx_segreduce_* call: (reduced as numpy, edges returned, nr_last_call())"""
    import torch
    import mini_amd
    f = mini_amd.Frontier(ctx, max(len(ids), 1)).load(np.ascontiguousarray(ids, dtype=np.int32))
    dv = torch.from_numpy(np.ascontiguousarray(vals)).cuda()
    red = torch.full((max(len(ids), 1),), SENTINEL[op], dtype=torch.float32 if op == "f32_plus" else torch.int32, device="cuda")
    nz = mini_amd.segreduce(g, f, dv, identity, red, op, push)
    info = g.nr_last_call()
    got = red.cpu().numpy()[:len(ids)]
    f.close()
    return got, nz, info


def compare(tag, got, want, bound, op):
    """exact (bound None) or |got - want| <= bound per row, atol 0"""
    assert got.dtype == (np.float32 if op == "f32_plus" else np.int32), tag
    g = got.astype(np.float64 if op == "f32_plus" else np.int64)
    if op == "f32_plus" and not np.all(np.isfinite(g)):
        bad = np.nonzero(~np.isfinite(g))[0]
        raise AssertionError("%s: %d non-finite results, first at position %d: %r" % (tag, len(bad), bad[0], got[bad[0]]))
    err = np.abs(g - want)
    bad = np.nonzero(err > (0 if bound is None else bound))[0]
    if len(bad):
        i = bad[0]
        raise AssertionError("%s: %d of %d results differ, first at frontier position %d: got %r, want %r%s" % (
            tag, len(bad), len(got), i, got[i], want[i], "" if bound is None else " (bound %g)" % bound[i]))
    if bound is not None and np.any(bound > 0):
        print("%s: largest error / bound = %.4f" % (tag, float(np.max(err[bound > 0] / bound[bound > 0]))))


def expect(tag, info, nz, body, frontier, rejected, edges):
    assert nz == edges, "%s: %d edges returned, want %d" % (tag, nz, edges)
    want = {"body": body, "frontier": frontier, "rejected": rejected, "edges": edges}
    if body is None:                                                     # (the child: one of the layout's bodies, reported to the parent)
        assert info["body"] in (1, 2), "%s: nr_last_call() says %r, want a layout body" % (tag, info)
        want["body"] = info["body"]
    assert info == want, "%s: nr_last_call() says %r, want %r" % (tag, info, want)


def plant_in_layout_space(g, case, where, is_max):
    """planted() on the LAYOUT's rows -- what the unit blocks are cut from: position p of a layout row is entry p % 64 of its unit
    p / 64 -- carried back to original ids: [(values by original id, {original row: extreme})]"""
    lro, lci, n2o, o2n = g.layout_arrays()
    back = {int(n2o[v]): v for v in case.special.values()}
    out = []
    for vals_new, want in nc.planted(lro, lci, list(back), where, is_max, seed=case.seed):
        vals = np.empty_like(vals_new)
        vals[o2n] = vals_new
        out.append((vals, {back[r]: x for r, x in want.items()}))
    return out


def check_full(ctx, g, case, op, body, identities="neutral", planted=True, tag=""):
    """the full frontier 0 .. n - 1 (expect `body`; None: whatever it is) and a permutation of it (the layout's kernels are entered, the
    device's verdict rejects it, the general kernel answers): values, edge count and path report.  Returns the bodies seen."""
    fr = case.frontiers()
    bodies = set()
    for fkey, rejected in (("full", 0), ("permuted", 1)):
        ids = fr[fkey]
        for vkey, identity, exact in value_sets(op, identities):
            t = "%s %s/%s/%s identity=%r" % (tag, op, fkey, vkey, identity)
            vals = case.values(vkey)
            got, nz, info = reduce_on_gpu(ctx, g, ids, vals, identity, op)
            want, bound, edges = case.want(fkey, ids, vkey, vals, op, identity)
            assert edges == case.m
            rej = rejected if body != 0 else 0                           # (without a layout nothing is entered, nothing rejected)
            expect(t, info, nz, 0 if rejected else body, 1, rej, edges)
            compare(t, got, want, None if exact else bound, op)
            bodies.add(info["body"])
    if planted and op != "f32_plus":
        ids = fr["full"]
        for where in nc.WHERE:
            for k, (vals, rows) in enumerate(plant_in_layout_space(g, case, where, op == "i32_max")):
                t = "%s %s/planted %s, batch %d" % (tag, op, where, k)
                got, nz, info = reduce_on_gpu(ctx, g, ids, vals, 0, op)          # (0: not neutral, and in no row's values)
                expect(t, info, nz, body, 1, 0, case.m)
                for r, x in rows.items():
                    assert got[r] == x, "%s: the row of %d entries gives %d, its planted extreme is %d" % (t, case.deg[r], got[r], x)
                want, _, _ = case.want(None, ids, None, vals, op, 0)
                compare(t, got, want, None, op)
    return sorted(bodies)


def check_subsets(ctx, g, case, op, body, identities="neutral", subset_on=True, tag=""):
    """ascending subsets: the special rows inside / outside the frontier and exactly ceil(n / 8) ids take the layout's kernels (`body`),
    one id fewer the general kernel; an ascending list with a duplicate is rejected on the device.  Results by frontier POSITION.
    subset_on = False (MGX_NR_SUBSET=0): every subset is an "other" frontier on the general kernel.  Returns the bodies seen."""
    fr = case.frontiers()
    bodies = set()
    for fkey in ("inside", "outside", "eighth", "below_eighth", "duplicate"):
        ids = fr[fkey]
        for vkey, identity, exact in value_sets(op, identities):
            t = "%s %s/%s/%s identity=%r" % (tag, op, fkey, vkey, identity)
            vals = case.values(vkey)
            got, nz, info = reduce_on_gpu(ctx, g, ids, vals, identity, op)
            want, bound, edges = case.want(fkey, ids, vkey, vals, op, identity)
            assert edges == int(case.deg[ids].sum())
            if not subset_on or body == 0 or fkey == "below_eighth":
                expect(t, info, nz, 0, 2 if subset_on and fkey != "below_eighth" else 0, 0, edges)
            elif fkey == "duplicate":
                expect(t, info, nz, 0, 2, 1, edges)
            else:
                expect(t, info, nz, body, 2, 0, edges)
            compare(t, got, want, None if exact else bound, op)
            bodies.add(info["body"])
    return sorted(bodies)


def main(mode):
    import torch
    import mini_amd
    assert mode in ("sliced0", "subset0"), mode
    assert torch.cuda.is_available(), "no GPU"
    ctx = mini_amd.Context(0, torch.cuda.current_stream().cuda_stream)
    case = edge_case(64)
    g = mini_amd.Graph.from_host(ctx, case.ro, case.ci).build_layout()
    assert g.layout_info()["units"] > 0
    out = {"mode": mode, "full_bodies": [], "subset_bodies": [], "degrees": sorted(case.special), "slices": None}
    for op in nc.OPS:
        for identities in ("neutral", "other"):
            # MGX_NR_SLICED=0: the unit blocks (body 1) for full frontiers and subsets; MGX_NR_SUBSET=0: full frontiers as always (body 2)
            out["full_bodies"] += check_full(ctx, g, case, op, None, identities, planted=identities == "neutral", tag=mode)
            out["subset_bodies"] += check_subsets(ctx, g, case, op, None if mode == "sliced0" else 0, identities,
                                                  subset_on=mode == "sliced0", tag=mode)
    out["full_bodies"] = sorted(set(out["full_bodies"])); out["subset_bodies"] = sorted(set(out["subset_bodies"]))
    out["slices"] = g.nr_slices_info()["mini_units"]
    out["big_rows_checked"] = [d for d in out["degrees"] if d > 64 * 64]
    g.close()
    sys.stdout.flush()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
