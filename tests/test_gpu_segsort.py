"""GPU suite (-m gpu): the segmented sort (mgx_segmented_sort_i32, include/mgx/segsort.hpp) against numpy's stable sort per
segment: keys only and pairs, ascending and descending, few distinct keys (stability), every length band and its edges."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _want(keys, vals, heads, descending):
    bounds = [0] + list(heads) + [len(keys)]
    k, v = keys.copy(), vals.copy()
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b - a < 2:
            continue
        seg = keys[a:b]
        order = np.argsort(-seg.astype(np.int64) if descending else seg, kind="stable")
        k[a:b], v[a:b] = seg[order], vals[a:b][order]
    return k, v


def _check(ctx, torch, keys, heads, descending, pairs):
    import mini_amd
    vals = np.arange(len(keys), dtype=np.int32)
    dk = torch.from_numpy(keys).cuda()
    dv = torch.from_numpy(vals).cuda() if pairs else None
    ds = torch.from_numpy(np.asarray(heads, dtype=np.int32)).cuda()
    mini_amd.segmented_sort(ctx, dk, ds, dv, descending)
    wk, wv = _want(keys, vals, heads, descending)
    got = dk.cpu().numpy()
    assert np.array_equal(got, wk), "%d of %d keys differ" % (int((got != wk).sum()), len(wk))
    if pairs:
        assert np.array_equal(dv.cpu().numpy(), wv)


LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 65537]


@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("distinct", [3, 1 << 30])
def test_band_edges(gpu_ctx, torch_mod, pairs, descending, distinct):
    rng = np.random.default_rng(distinct % 1000 + 2 * pairs + descending)
    lens = LENGTHS + list(rng.permutation(LENGTHS))
    heads = np.cumsum([0] + lens[:-1]).astype(np.int32)[1:]      # the first segment starts at 0 (no head)
    count = int(sum(lens))
    keys = rng.integers(-distinct, distinct, count).astype(np.int32)
    _check(gpu_ctx, torch_mod, keys, heads, descending, pairs)


@pytest.mark.parametrize("pairs", [False, True])
def test_empty_runs_and_first_head_above_zero(gpu_ctx, torch_mod, pairs):
    rng = np.random.default_rng(9)
    count = 20000
    heads = np.sort(np.concatenate([rng.integers(100, count, 300), [500] * 7, [count] * 3])).astype(np.int32)
    keys = rng.integers(0, 10, count).astype(np.int32)
    _check(gpu_ctx, torch_mod, keys, heads, False, pairs)
    _check(gpu_ctx, torch_mod, keys, heads, True, pairs)


def test_many_short_segments(gpu_ctx, torch_mod):
    rng = np.random.default_rng(4)
    lens = rng.integers(0, 80, 50000)
    heads = np.cumsum(lens)[:-1].astype(np.int32)
    keys = rng.integers(0, 5, int(lens.sum())).astype(np.int32)
    _check(gpu_ctx, torch_mod, keys, heads, True, True)


@pytest.mark.parametrize("pairs", [False, True])
def test_one_segment_of_2_24(gpu_ctx, torch_mod, pairs):
    rng = np.random.default_rng(24)
    count = 1 << 24
    keys = rng.integers(0, 1000, count).astype(np.int32)
    heads = np.array([5, 5, count - 3], np.int32)                # a long middle segment between two short ones
    _check(gpu_ctx, torch_mod, keys, heads, False, pairs)
