"""GPU suite (-m gpu): the fused k-core (mgx_kcore_run, include/mgx/kcore_fused.hpp) against the operator path (mgx_kcore_enact)
on a second handle, the numpy worklist model (tests/kcore_model.py) and the reference's goldens.  Integer work: core numbers,
largest k-core, final working degrees and the stats are compared bit for bit."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import kcore_model as model
from tests.golden_inputs import case_path, matches

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CASES = [c for c in json.load(open(os.path.join(GOLD, "reference_goldens.json")))["cases"] if "kcore_largest" in c]


def _graph(ctx, ro, ci):
    import mini_amd
    return mini_amd.Graph.from_host(ctx, ro, ci, None)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fused_kcore_matches_reference_goldens(gpu_ctx, oracle, case, tmp_path):
    import mini_amd
    n, ro, ci, w, _ = oracle.load_mtx(case_path(case, oracle, tmp_path, GOLD), undir=True)
    kc = mini_amd.KcoreProblem(_graph(gpu_ctx, ro, ci))
    largest, st = kc.run()
    assert largest == case["kcore_largest"]
    assert matches(case, "kcore_num_cores", kc.num_cores(), np.int32)
    kc.close()


def _uniform16(ctx, oracle):
    from mini_amd import rmat
    d = rmat.uniform_csr(ctx, 16, 16)
    return d["row_offsets"].cpu().numpy(), d["col_indices"].cpu().numpy()


GRAPHS = {
    "rmat10": lambda ctx, o: o.rmat_csr(10, 16, 10)[1:3],
    "rmat12": lambda ctx, o: o.rmat_csr(12, 8, 12)[1:3],
    "rmat14": lambda ctx, o: o.rmat_csr(14, 4, 14)[1:3],
    "rmat16": lambda ctx, o: o.rmat_csr(16, 16, 16)[1:3],
    "rmat18_stranded": lambda ctx, o: o.rmat_csr(18, 16, 18)[1:3],
    "uniform16": _uniform16,
    "grid256": lambda ctx, o: model.grid(256, 256),
    "star_forest": lambda ctx, o: model.star_forest(),
    "k40_tripled_cap": lambda ctx, o: model.tripled_clique(),
    "directed_ragged": lambda ctx, o: model.ragged_directed(),
    "path3": lambda ctx, o: model.path3(),
    "no_entries": lambda ctx, o: model.no_entries(),
    "single": lambda ctx, o: model.single(False),
    "single_loop": lambda ctx, o: model.single(True),
}


@pytest.mark.parametrize("name", list(GRAPHS))
def test_fused_equals_operator_path_and_model(gpu_ctx, oracle, name):
    import mini_amd
    ro, ci = GRAPHS[name](gpu_ctx, oracle)
    g = _graph(gpu_ctx, ro, ci)
    fused, oper = mini_amd.KcoreProblem(g), mini_amd.KcoreProblem(g)
    largest, st = fused.run()
    elargest, est = oper.enact()
    mcores, mlargest, mdeg, mst = model.decompose(ro, ci)
    print(name, "fused", largest, st, "operator", elargest, est)
    assert largest == elargest == mlargest
    cores, deg = fused.num_cores(), fused.degrees()
    assert np.array_equal(cores, oper.num_cores()) and np.array_equal(cores, mcores)
    assert np.array_equal(deg, oper.degrees()) and np.array_equal(deg, mdeg)
    assert {k: st[k] for k in model.STAT_NAMES} == mst
    assert st["passes"] == est["passes"] - est["rounds"] and st["expanded"] == est["expanded"] and st["removed"] == est["removed"]
    # which launches the run was: the plan's, then idle ones up to the end of the host's last batch
    plan = model.launch_plan(ro, ci)
    assert np.array_equal(plan.cores, mcores) and plan.stats == mst
    kinds = fused.step_kinds()
    waits, launches = model.host_waits_and_launches(len(plan.kinds))
    assert kinds[:len(plan.kinds)].tolist() == plan.kinds and (kinds[len(plan.kinds):] == model.IDLE).all()
    assert len(kinds) == launches and st["host_waits"] == waits
    if name == "rmat18_stranded":
        assert st["stranded"] == 1
    if name == "path3":
        assert cores.tolist() == [1, 0, 1]
    if name == "grid256":
        assert st["passes"] >= 255
    fused.close()
    oper.close()
    g.close()


def test_fused_runs_start_afresh_and_handles_are_independent(gpu_ctx, oracle):
    import mini_amd
    n, ro, ci, w = oracle.rmat_csr(14, 4, 14)
    mcores, mlargest, mdeg, mst = model.decompose(ro, ci)
    g = _graph(gpu_ctx, ro, ci)
    a, b = mini_amd.KcoreProblem(g), mini_amd.KcoreProblem(g)

    def same(kc, largest):
        return largest == mlargest and np.array_equal(kc.num_cores(), mcores) and np.array_equal(kc.degrees(), mdeg)
    l1, s1 = a.run()
    assert same(a, l1)
    l2, s2 = a.run()                                   # twice in a row
    assert same(a, l2) and s1 == s2
    le, est = b.enact()
    assert same(b, le)
    assert same(a, l2)                                 # b's run left a's answers alone
    lr, sr = b.run()                                   # straight after an enact, no reset
    assert same(b, lr) and {k: sr[k] for k in model.STAT_NAMES} == mst
    b.reset()
    le2, est2 = b.enact()                              # the operator path after a fused run
    assert same(b, le2) and est2 == est
    assert same(a, l2)
    a.close()
    b.close()
    g.close()


def test_fused_null_largest_is_invalid(gpu_ctx):
    import mini_amd
    ro, ci = model.path3()
    g = _graph(gpu_ctx, ro, ci)
    kc = mini_amd.KcoreProblem(g)
    assert mini_amd.lib.mgx_kcore_run(kc._h, None, None) == mini_amd.MGX_E_INVALID
    largest = C.c_int()
    assert mini_amd.lib.mgx_kcore_run(kc._h, C.byref(largest), None) == 0 and largest.value == 1      # stats may be NULL
    kc.close()
    g.close()


def test_fused_host_waits_do_not_follow_levels_or_passes(gpu_ctx, oracle):
    """RMAT-16 has 108 levels and 332 removing passes (the model's count): a path that waits once per level or pass fails"""
    import mini_amd
    n, ro, ci, w = oracle.rmat_csr(16, 16, 16)
    g = _graph(gpu_ctx, ro, ci)
    kc = mini_amd.KcoreProblem(g)
    largest, st = kc.run()
    print("rmat16", st)
    assert st["levels"] == 108 and st["passes"] == 332
    waits, launches = model.host_waits_and_launches(len(model.launch_plan(ro, ci).kinds))
    assert waits < 108
    assert st["host_waits"] == waits and len(kc.step_kinds()) == launches
    kc.close()
    g.close()
