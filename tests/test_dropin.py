"""Drop-in boundary: the reference's own BFS/SSSP/PR (and k-core) enactors, problems, functors and test
drivers, unmodified, compiled against this repo's operator headers (oracle/build_ref.sh)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.mark.skipif(not os.path.isdir("/root/reference/gunrock/src"), reason="reference tree not present")
def test_reference_sources_compile_unchanged_against_our_operator_headers():
    subprocess.check_call(["bash", os.path.join(ROOT, "oracle", "build_ref.sh")])
    for t in ("bfs", "sssp", "pr", "kcore"):
        assert os.path.exists(os.path.join(BIN, "ref_test_" + t))


def _run(name, *args):
    exe = os.path.join(BIN, name)
    if not os.path.exists(exe):
        pytest.skip("%s not prebuilt (built only where the reference tree is present)" % name)
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ["bfs_test.mtx", "pr_test.mtx", "kcore_test.mtx", "sssp_test.mtx"])
def test_reference_bfs_driver_validates_on_our_operators(fixture):
    """test_bfs.cu runs bfs_enactor_t::enact_pushpull (reference code) on our advance/filter kernels and
    compares with the reference's own bfs_problem_t::cpu: it must print "Correct." (test_bfs.cu:49-52)."""
    for extra in ([], ["--alpha=0.5"], ["--src=3"]):
        r = _run("ref_test_bfs", "--file=" + os.path.join(GOLD, fixture), *extra)
        assert r.returncode == 0, r.stderr
        assert "Correct." in r.stdout and "Validation Error" not in r.stdout, r.stdout


@pytest.mark.gpu
def test_reference_sssp_and_pr_drivers_run_on_our_operators():
    """test_sssp.cu validates preds, which are racy upstream, so only completion is
    required; test_pr.cu validates nothing (test_pr.cu:36-43)."""
    r = _run("ref_test_sssp", "--file=" + os.path.join(GOLD, "sssp_test.mtx"), "--queue-sizing=1.5")
    assert r.returncode == 0 and ("Correct" in r.stdout or "Validation Error" in r.stdout), r.stdout + r.stderr
    r = _run("ref_test_sssp", "--file=" + os.path.join(GOLD, "sssp_test.mtx"), "--undirected", "--queue-sizing=2")
    assert r.returncode == 0, r.stderr
    r = _run("ref_test_pr", "--file=" + os.path.join(GOLD, "pr_test.mtx"), "--max_iter=5")
    assert r.returncode == 0 and "finished iteration:0" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ["kcore_test.mtx", "bfs_test.mtx"])
def test_reference_kcore_driver_validates_on_our_operators(fixture):
    """k-core is outside the hot-path scope but free coverage: test_kcore.cu drives filter with three
    functors and a has_output=false advance whose functor does atomicAdd, then compares core numbers with the
    reference's own CPU routine (kcore_problem.hxx:54-105)."""
    r = _run("ref_test_kcore", "--file=" + os.path.join(GOLD, fixture))
    assert r.returncode == 0, r.stderr
    assert "Correct." in r.stdout and "Validation Error" not in r.stdout, r.stdout
