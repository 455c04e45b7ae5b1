"""CPU suite: the inputs of tests/test_gpu_nreduce_paths.py (tests/nreduce_cases.py) are what they promise, and the reference the
GPU is judged by (nreduce_cases.reduce_f64) agrees bit for bit with the oracle's serial restatement of the operator wherever float32
sums are exact -- with neutral and with non-neutral identities."""
import numpy as np
import pytest

from tests import nreduce_cases as nc


@pytest.fixture(scope="module")
def graphs():
    return {lm: nc.edge_graph(lm, seed=lm) for lm in (64, 17, 32)}


@pytest.mark.parametrize("long_min", [64, 17, 32])
def test_edge_graph_yields_exactly_the_requested_degrees(graphs, long_min):
    ro, ci, special = graphs[long_min]
    n = nc.N
    deg = np.diff(ro)
    assert len(ro) == n + 1 and ro[0] == 0 and ro[-1] == len(ci) and ci.dtype == np.int32 and ro.dtype == np.int32
    assert ci.min() >= 0 and ci.max() < n < 2 ** 23
    assert sorted(special) == list(nc.edge_degrees(long_min)) and len(set(special.values())) == len(special)
    for must in (0, 1, 4, 5, 16, 17, long_min - 1, long_min, long_min + 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 4160, 4161,
                 65535, 65536, 65537):
        assert must in special
    for d, v in special.items():
        row = ci[ro[v]:ro[v + 1]]
        assert deg[v] == d == len(row)
        assert np.all(np.diff(row) > 0), "a special row's neighbours are distinct and ascending"
        if d >= 4096:
            assert row[0] < n // 8 and row[-1] >= n - n // 8, "drawn over the whole id range"
    rest = np.ones(n, dtype=bool); rest[list(special.values())] = False
    assert deg[rest].max() == 8 and deg[rest].min() == 0
    assert 600_000 < len(ci) < 900_000
    # rows sorted by neighbour everywhere; the one vertex of the largest degree is unique (layout id 0 of a hub-first layout)
    row = np.repeat(np.arange(n), deg)
    assert np.all((np.diff(ci) >= 0) | (np.diff(row) > 0))
    assert int(np.argmax(deg)) == special[65537] and np.count_nonzero(deg == 65537) == 1


def test_transpose_is_the_transpose(graphs):
    ro, ci, _ = graphs[17]
    co, ri = nc.transpose(ro, ci)
    a = np.stack([np.repeat(np.arange(nc.N), np.diff(ro)), ci], 1)
    b = np.stack([ri, np.repeat(np.arange(nc.N), np.diff(co))], 1)
    assert np.array_equal(a[np.lexsort((a[:, 1], a[:, 0]))], b[np.lexsort((b[:, 1], b[:, 0]))])
    assert not np.array_equal(co, ro)


def _frontiers(special):
    f = dict(nc.subset_frontiers(nc.N, special))
    f["full"] = np.arange(nc.N, dtype=np.int32)
    f["permuted"] = np.random.default_rng(5).permutation(nc.N).astype(np.int32)
    return f


def test_subset_frontiers_are_what_they_say(graphs):
    _, _, special = graphs[64]
    f = nc.subset_frontiers(nc.N, special)
    sp = set(special.values())
    for name, ids in f.items():
        assert ids.dtype == np.int32 and np.all(np.diff(ids) > 0) and ids[0] >= 0 and ids[-1] < nc.N, name
    assert sp <= set(f["inside"].tolist()) and sp <= set(f["eighth"].tolist()) and sp <= set(f["below_eighth"].tolist())
    assert not (sp & set(f["outside"].tolist()))
    assert len(f["eighth"]) * 8 >= nc.N > (len(f["eighth"]) - 1) * 8 and len(f["below_eighth"]) == len(f["eighth"]) - 1


@pytest.mark.parametrize("identity", [0.0, 100.0, -1.0])
def test_reduce_f64_equals_the_oracle_on_small_integer_sums(oracle, graphs, identity):
    ro, ci, special = graphs[64]
    vals = nc.small_int_values(nc.N, np.random.default_rng(1))
    assert vals.min() == 1 and vals.max() == 8
    for name, ids in _frontiers(special).items():
        want, edges = nc.reduce_f64(ro, ci, ids, vals, identity, "f32_plus")
        got, nz = oracle.neighbor_reduce_f32_plus(ro, ci, ids, vals, identity)
        assert nz == edges == int(np.diff(ro)[ids].sum()), name
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want), "a sum float32 cannot hold"
        assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), name
        empty = np.diff(ro)[ids] == 0
        assert empty.any() and np.all(want[empty] == identity)
        if identity:
            assert not np.any(want[~empty] == identity)          # (8 d is neither 100 nor -1 for the sums that occur: checked, not assumed)


@pytest.mark.parametrize("op,identity,sign", [("i32_min", nc.INT_MAX, 0), ("i32_max", nc.INT_MIN, 0), ("i32_min", 0, 1), ("i32_max", 0, -1)])
def test_reduce_f64_equals_the_oracle_on_integers(oracle, graphs, op, identity, sign):
    ro, ci, special = graphs[32]
    vals = nc.int_values(nc.N, np.random.default_rng(2), sign)
    assert sign == 0 or np.all(vals * sign > 0)
    for name, ids in _frontiers(special).items():
        want, edges = nc.reduce_f64(ro, ci, ids, vals, identity, op)
        got, nz = oracle.neighbor_reduce_i32(ro, ci, ids, vals, identity, op == "i32_max")
        assert nz == edges, name
        assert np.array_equal(got.astype(np.int64), want), name
        empty = np.diff(ro)[ids] == 0
        assert np.all(want[empty] == identity)
        if sign:
            assert np.all(want[~empty] * sign > 0), "the non-neutral identity 0 is in no row that has entries"


@pytest.mark.parametrize("is_max", [False, True])
@pytest.mark.parametrize("where", nc.WHERE)
def test_planted_extremes_are_unique_and_where_they_should_be(graphs, where, is_max):
    ro, ci, special = graphs[64]
    deg = np.diff(ro)
    rows = list(special.values())
    batches = nc.planted(ro, ci, rows, where, is_max)
    covered = []
    assert 1 <= len(batches) <= 6
    for vals, want in batches:
        assert vals.dtype == np.int32 and (np.all(vals < 0) if is_max else np.all(vals > 0))
        for r, x in want.items():
            row = vals[ci[ro[r]:ro[r + 1]]]
            p = nc.position(int(deg[r]), where)
            assert row[p] == x == (row.max() if is_max else row.min()), (where, int(deg[r]))
            assert np.count_nonzero(row == x) == 1, "the extreme is unique in its row"
            covered.append(r)
    assert sorted(covered) == sorted(r for r in rows if nc.position(int(deg[r]), where) is not None)
    assert len(covered) == {"first": 22, "last": 22, "unit_end": 16, "tail_first": 10}[where]       # (of the 23 degrees at long_min = 64)


def test_positions():
    assert [nc.position(d, "unit_end") for d in (63, 64, 65, 128, 4161)] == [None, 63, 63, 127, 4159]
    assert [nc.position(d, "tail_first") for d in (63, 64, 65, 128, 129, 4161)] == [None, None, 64, None, 128, 4160]
    assert nc.position(0, "first") is None and nc.position(1, "last") == 0


def test_sum_bound_holds_for_a_serial_and_a_pairwise_float32_fold(graphs):
    """the derived bound on two orders a CPU can run: np.cumsum (serial float32) and a pairwise fold, on the longest row"""
    ro, ci, special = graphs[64]
    vals = nc.real_values(nc.N, np.random.default_rng(3))
    assert vals.min() >= -3 and vals.max() < 3 and (vals < 0).any()
    ids = np.array(sorted(special.values()), dtype=np.int32)
    want, _ = nc.reduce_f64(ro, ci, ids, vals, 0.0, "f32_plus")
    bound = nc.sum_bound(ro, ci, ids, vals)
    for i, v in enumerate(ids):
        x = vals[ci[ro[v]:ro[v + 1]]]
        if not len(x):
            assert bound[i] == 0
            continue
        serial = np.cumsum(x, dtype=np.float32)[-1]
        y = x.copy()
        while len(y) > 1:
            if len(y) & 1:
                y = np.concatenate([y, np.zeros(1, dtype=np.float32)])
            y = y[0::2] + y[1::2]
        assert abs(float(serial) - want[i]) <= bound[i] and abs(float(y[0]) - want[i]) <= bound[i], len(x)
        if len(x) == 1:
            assert bound[i] == 0 and float(serial) == want[i]
