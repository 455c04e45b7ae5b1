"""The host side of a launch chain (include/mgx/launch_chain.hpp) in Python: the one statement of run_launch_chain that
the suites of the six chained paths -- k-core, k-truss, SCC, label propagation, multi-source BFS, Louvain -- hold the device against.

A run's launches are numbered from 0.  K is the number of the run's first DONE / IDLE launch plus one: the length of a model's
`kinds` with its final idle.  The host enqueues batches of BATCH_MIN, 2 x, 4 x ... up to BATCH_MAX launches and waits once behind
each; the run ends at the first wait whose batches cover launch K - 1.  K is always predicted -- by a model, a closed form, or (SCC
on general graphs) read from the device's log -- and never taken from the `launches` a run reports: that number is what the host
loop enqueued, and an expectation computed from it holds for any loop."""

BATCH_MIN = 64            # CHAIN_BATCH_MIN, CHAIN_BATCH_MAX: launches per host wait, doubling
BATCH_MAX = 256
LOG_CAP = 1 << 16         # CHAIN_LOG_CAP: the launches (multi-source BFS: the levels) whose kind a run keeps

# K one below, at and one above the first three waits' last launch: 64 | 65, 192 | 193, 448 | 449 decide whether the host needs
# another batch
SEAMS = (63, 64, 65, 191, 192, 193, 447, 448, 449)


def waits_and_launches(n_kinds):
    """(host waits, launches enqueued) of a run whose first idle launch is launch n_kinds - 1: batches of BATCH_MIN, doubling up to
    BATCH_MAX, one wait behind each; the run ends at the first wait whose batches cover the idle launch"""
    waits, launches, batch = 0, 0, BATCH_MIN
    while True:
        launches += batch
        waits += 1
        if launches >= n_kinds:
            return waits, launches
        batch = min(batch * 2, BATCH_MAX)


def logged(kinds, idle, launches=None):
    """what a run's step_kinds holds: the model's kinds (its final idle included), then idle up to the launches enqueued, the first
    LOG_CAP of all that"""
    kinds = list(kinds)
    if launches is None:
        launches = waits_and_launches(len(kinds))[1]
    return (kinds + [idle] * (launches - len(kinds)))[:LOG_CAP]
