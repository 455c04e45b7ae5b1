"""GPU suite (-m gpu): WHICH launches a fused k-core run (mgx_kcore_run, include/mgx/kcore_fused.hpp) consists of.  Every launch
decides on the device what it is -- MIN, LIST, EXPAND, FILTER, MINI or idle -- and mgx_kcore_step_kinds keeps the choice.  The
sequence is a function of the graph (fronts and candidates are sets), so tests/kcore_model.launch_plan predicts it exactly; the
inputs of tests/kcore_cases.py put a front, a row or the scan's last id on each of the header's thresholds.  Integer work: kinds,
core numbers, degrees, largest k-core, stats, launches and host waits are compared with ==."""
import ctypes as C

import numpy as np
import pytest

from tests import kcore_cases as cases
from tests import kcore_model as model

pytestmark = pytest.mark.gpu


def _graph(ctx, ro, ci):
    import mini_amd
    return mini_amd.Graph.from_host(ctx, ro, ci, None)


def check_run(kc, largest, st, plan):
    """a finished fused run on handle kc against the plan: results, stats, and every launch"""
    assert largest == plan.largest
    assert np.array_equal(kc.num_cores(), plan.cores)
    assert np.array_equal(kc.degrees(), plan.degrees)
    assert {k: st[k] for k in model.STAT_NAMES} == plan.stats
    kinds = kc.step_kinds()
    waits, launches = model.host_waits_and_launches(len(plan.kinds))
    print("kinds", " ".join(model.KIND_NAMES.get(int(k), str(int(k))) for k in kinds[:len(plan.kinds) + 2]), "of", len(kinds),
          "waits", st["host_waits"], "plan", len(plan.kinds), launches, waits)
    assert kinds[:len(plan.kinds)].tolist() == plan.kinds
    assert (kinds[len(plan.kinds):] == model.IDLE).all()
    assert len(kinds) == launches
    assert st["host_waits"] == waits


@pytest.mark.parametrize("name", list(cases.CASES))
def test_case_runs_the_planned_launches(gpu_ctx, name):
    import mini_amd
    ro, ci = cases.get(name)
    plan = cases.plan(name)
    g = _graph(gpu_ctx, ro, ci)
    fused, oper = mini_amd.KcoreProblem(g), mini_amd.KcoreProblem(g)
    largest, st = fused.run()
    elargest, est = oper.enact()
    print(name, "fused", largest, st, "operator", elargest, est)
    check_run(fused, largest, st, plan)
    assert elargest == plan.largest
    assert np.array_equal(oper.num_cores(), plan.cores) and np.array_equal(oper.degrees(), plan.degrees)
    assert st["passes"] == est["passes"] - est["rounds"] and st["expanded"] == est["expanded"] and st["removed"] == est["removed"]
    fused.close()
    oper.close()
    g.close()


def test_candidate_stage_on_one_unit(gpu_ctx, torch_mod, monkeypatch):
    """4096 disjoint paths a - b - c.  Level 2's front is the 8192 ends, short rows all (8192 entries: an EXPAND of the device);
    every b is decremented twice and becomes a candidate once.  On a one-unit context the step is 4 workgroups -- 16 waves, which
    share the 4096 candidates, so one of them at least holds 256: its stage of 128 goes out inside the loop and again behind it
    (on the session context no wave sees more than 64 rows).  The candidates are then stranded at degree 0."""
    import mini_amd
    from tests.grid_cus import one_cu_context
    paths = 4096
    a, b, c = np.arange(paths), paths + np.arange(paths), 2 * paths + np.arange(paths)
    ro, ci = cases._symmetric(3 * paths, np.concatenate([a, b]), np.concatenate([b, c]))
    plan = model.launch_plan(ro, ci)
    assert plan.kinds[:4] == [model.MIN, model.LIST, model.EXPAND, model.FILTER] and plan.stats["stranded"] == paths
    with one_cu_context(monkeypatch, torch_mod) as one_cu:
        for ctx in (one_cu, gpu_ctx):
            g = _graph(ctx, ro, ci)
            kc = mini_amd.KcoreProblem(g)
            largest, st = kc.run()
            check_run(kc, largest, st, plan)
            kc.close()
            g.close()


def _uniform16(ctx, oracle):
    from mini_amd import rmat
    d = rmat.uniform_csr(ctx, 16, 16)
    return d["row_offsets"].cpu().numpy(), d["col_indices"].cpu().numpy()


MIXES = {
    "rmat13": lambda ctx, o: o.rmat_csr(13, 16, 13)[1:3],
    "rmat16": lambda ctx, o: o.rmat_csr(16, 16, 16)[1:3],
    "uniform16": _uniform16,
}


@pytest.mark.parametrize("name", list(MIXES))
def test_real_mixes_run_the_planned_launches(gpu_ctx, oracle, name):
    import mini_amd
    ro, ci = MIXES[name](gpu_ctx, oracle)
    plan = model.launch_plan(ro, ci)
    if name == "rmat16":
        assert set(plan.kinds) == {model.MIN, model.LIST, model.EXPAND, model.FILTER, model.MINI, model.IDLE}
    g = _graph(gpu_ctx, ro, ci)
    kc = mini_amd.KcoreProblem(g)
    largest, st = kc.run()
    check_run(kc, largest, st, plan)
    kc.close()
    g.close()


def test_state_does_not_leak_from_run_to_run(gpu_ctx):
    """the ring, the totals and the log start afresh with every run, and belong to the handle"""
    import mini_amd
    names = ("broom2048", "stairs2_40")
    graphs = {name: _graph(gpu_ctx, *cases.get(name)) for name in names}
    kcs = {name: mini_amd.KcoreProblem(graphs[name]) for name in names}
    seen = []
    for name in ("broom2048", "stairs2_40", "broom2048", "broom2048", "stairs2_40"):       # interleaved, and one handle twice in a row
        largest, st = kcs[name].run()
        check_run(kcs[name], largest, st, cases.plan(name))
        seen.append((name, largest, st, kcs[name].step_kinds().tolist()))
    # the other handle's log still describes ITS last run
    check_run(kcs["broom2048"], seen[3][1], seen[3][2], cases.plan("broom2048"))
    for name in names:
        runs = [s[1:] for s in seen if s[0] == name]
        assert all(r == runs[0] for r in runs)                       # same call, same kinds, same stats
    # a run() straight after an enact(), no reset: the stairs' 192 launches behind the broom's 64 on a handle that has peeled already
    kc = kcs["stairs2_40"]
    kc.reset()
    elargest, est = kc.enact()
    assert elargest == cases.plan("stairs2_40").largest
    largest, st = kc.run()
    check_run(kc, largest, st, cases.plan("stairs2_40"))
    for name in names:
        kcs[name].close()
        graphs[name].close()


def test_step_kinds_contract(gpu_ctx):
    import mini_amd
    lib = mini_amd.lib
    g = _graph(gpu_ctx, *cases.get("stairs2_40"))
    kc = mini_amd.KcoreProblem(g)
    n = C.c_int64(-7)
    three = (C.c_int * 4)(-1, -1, -1, -1)
    assert lib.mgx_kcore_step_kinds(kc._h, three, 3, C.byref(n)) == mini_amd.MGX_E_INVALID      # no fused run yet
    largest, est = kc.enact()
    assert lib.mgx_kcore_step_kinds(kc._h, three, 3, C.byref(n)) == mini_amd.MGX_E_INVALID      # (an enact is none)
    assert n.value == -7 and list(three) == [-1] * 4
    kc.run()
    assert lib.mgx_kcore_step_kinds(kc._h, three, 3, C.byref(n)) == 0
    assert n.value == 192 and list(three) == cases.plan("stairs2_40").kinds[:3] + [-1]           # cap entries, no more
    n.value = -7
    assert lib.mgx_kcore_step_kinds(kc._h, None, 0, C.byref(n)) == 0 and n.value == 192          # launches only
    assert lib.mgx_kcore_step_kinds(kc._h, three, 3, None) == mini_amd.MGX_E_INVALID
    assert lib.mgx_kcore_step_kinds(kc._h, three, -1, C.byref(n)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_kcore_step_kinds(kc._h, None, 3, C.byref(n)) == mini_amd.MGX_E_INVALID
    assert lib.mgx_kcore_step_kinds(None, three, 3, C.byref(n)) == mini_amd.MGX_E_INVALID
    kc.close()
    g.close()
