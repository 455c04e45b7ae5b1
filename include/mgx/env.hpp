// mgx/env.hpp -- the ONE place the library reads its environment.
//
// Every switch the product (and the lab build) knows is a row of the table below: name + what it does.  `mgx::env(name)` is the only
// caller of getenv in the tree: it returns the value, NULL when the variable is unset OR EMPTY (an exported `MGX_X=` is not a zero), and
// refuses a name that is not in the table (a typo in the sources aborts at the first call instead of silently reading nothing).
// `mgx_env_switches` (include/mgx.h) hands the table to tools and tests: tests/test_capi_boundary.py checks that every MGX_* variable the
// tests, the tools and the bench scripts set is a switch the library really reads (a typo there used to test nothing, silently).
//
// The switches select between PRODUCT paths that the default thresholds pick by size -- the parity tests force each of them on small
// graphs; none changes a result.  DESIGN.md 6.1 says which families exist; the rows are the documentation of the individual ones.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace mgx {

struct env_switch_t { const char* name; const char* what; };

inline const env_switch_t* env_switches(int* count) {
  static const env_switch_t table[] = {
    // ---- fused BFS (bfs_run_opts_t::from_env: read once per handle) and the layout it runs on
    {"MGX_BFS_DENSE", "0 / N: unit-block body for long rows off / a level takes it from frontier edges >= units / N"},
    {"MGX_BFS_VSHORT", "0 / N: short rows vertex by vertex off / threshold divisor"},
    {"MGX_BFS_LAZY", "0 / N: lazy queues off / the build writes no queues behind a push that stored >= n / N marks"},
    {"MGX_BFS_COLD", "0 / 2 (lab: 1): cold-edge pass off / on"},
    {"MGX_BFS_COLD_LISTS", "0 / 1 (lab: 2): whether the layout builds the long rows' cold-edge lists"},
    {"MGX_BFS_COLD_PACK", "0: keep the 8-byte cold pairs instead of the packed 4-byte ones"},
    {"MGX_BFS_COLD_TEST", "0 / 1: bitmap probe of cold neighbours off / on (default: by graph size)"},
    {"MGX_BFS_FLAT_LISTS", "0: a flat graph keeps the ordinary layout instead of all-entry pair lists"},
    {"MGX_BFS_HOT_UNITS", "0: no second copy of the unit blocks without the cold lists' entries"},
    {"MGX_BFS_PACK24", "0: 32-bit unit-block entries instead of the 24-bit copy"},
    {"MGX_BFS_PACK20", "0: the unit blocks without the cold lists' entries at 24 bits per entry instead of 20"},
    {"MGX_BFS_MINI", "0 / 2: no M launches / M launches on every graph (default: from 2^22 vertices on)"},
    {"MGX_BFS_BATCH_OVERLAP", "0: a batch of sources runs in one traversal state, no launch shared by two traversals"},
    {"MGX_BFS_SEED_CHAIN", "0: the chain of small levels at the start runs inside slot 0's push launch"},
    {"MGX_BFS_TAIL_CHAIN", "0: no in-place chain launch behind the last slots"},
    {"MGX_BFS_TAIL_FRONT", "0: no chain in front of the last slots"},
    {"MGX_BFS_CHAIN_BIG_EDGES", "largest level an in-place chain launch runs (edges)"},
    {"MGX_BFS_CHAIN_MAX_EDGES", "largest level block 0 runs inside the push launch (0: no chains)"},
    {"MGX_BFS_MERGED_PUSH", "0: the parts of a slot's push as separate launches"},
    {"MGX_BFS_MERGED_PULL", "0: direction-optimising runs: the bottom-up sweep as a launch of its own"},
    {"MGX_BFS_DO_CHAIN", "0: direction-optimising runs: no chains of small top-down levels"},
    {"MGX_BFS_DEFER", "0 / N: deferred hot marks off / a workgroup flushes its bitmap above N claims"},
    {"MGX_BFS_DEFER_REACH", "\"mul/div\": a level defers its hot marks while reached * mul < range * div"},
    {"MGX_BFS_DEFER_WORDS", "words of the bitmap prefix whose marks are deferred (default: all)"},
    {"MGX_BFS_BUILD_LIST", "1: the list-based queue build of round 1"},
    {"MGX_BFS_LEVEL_BYTES", "0: under a layout the queue build scatters labels itself (no level bytes, no translation pass)"},
    {"MGX_BFS_SRC_PLAN", "0: no per-source launch plan"},
    {"MGX_BFS_LONG_MIN", "long-row threshold of the layout (entries)"},
    {"MGX_BFS_HOT_MIN_EDGES", "smallest level that copies the bitmap prefix to LDS (edges)"},
    {"MGX_BFS_FLAGS", "(lab) instrumented stream kernel; results wrong by design"},
    {"MGX_BFS_BUILD_DIAG", "(lab) parts of the queue build switched off; results wrong by design"},
    {"MGX_BFS_DENSE_DIAG", "(lab) parts of the unit-block body switched off; results wrong by design"},
    // ---- fused SSSP
    {"MGX_SSSP_DENSE", "0 / N: no sweep for heavy iterations / an iteration is heavy from m / N frontier edges"},
    {"MGX_SSSP_HOT_MIN_EDGES", "smallest iteration that keeps the hubs' distance bounds in LDS (edges)"},
    {"MGX_SSSP_BUILD_LIST", "1: list-based queue build"},
    // ---- triangle counting (tc_opts_t::from_env: read once per handle)
    {"MGX_TC_SHORT_MAX", "oriented rows of at most N entries are counted an entry a lane (default 16)"},
    {"MGX_TC_WAVE_MAX", "longer rows of at most N entries are staged in LDS by a wave, the rest by a workgroup (default 256)"},
    {"MGX_TC_STAGE", "entries of an LDS stage; a longer row is staged in chunks (default and at most 4096; a wave's: 512)"},
    // ---- k-truss decomposition (ktruss_opts_t::from_env: read once per handle; both defaults are unmeasured guesses)
    {"MGX_KTRUSS_SHORT_MAX", "front edges whose shorter adjacency row has at most N entries are expanded a lane each, the rest by waves (default 16)"},
    {"MGX_KTRUSS_SEG", "entries of the shorter row one wave expands; a longer row goes out as (edge, segment) items (default 512)"},
    {"MGX_SCC_LONG_MIN", "out- or in-rows of at least N entries of a front vertex go out as (vertex, segment) items, a wave each; shorter ones take a lane (default 32, an unmeasured guess)"},
    {"MGX_SCC_SEG", "entries of a long row one wave takes (default 256, an unmeasured guess)"},
    // ---- label propagation (lpa_opts_t::from_env: read once per handle; all four defaults are unmeasured guesses)
    {"MGX_LPA_SHORT_MAX", "vertices whose rows have at most N entries find their label a lane each, the labels in registers (default and at most 16)"},
    {"MGX_LPA_WAVE_MAX", "longer rows of at most N entries take a wave each and a wave-private LDS table; the rest a workgroup (default 256, at most 512)"},
    {"MGX_LPA_TABLE", "labels a workgroup's LDS table holds, a power of two in [32, 2048]; a row with more distinct labels is passed over by hash class (default 2048)"},
    {"MGX_LPA_LIST_DIV", "0 / N: every iteration runs over all vertices / over the active set when it has at most n / N vertices (default 8; 1: always)"},
    // ---- multi-source BFS (msbfs_opts_t::from_env: read once per handle; all four defaults are unmeasured guesses)
    {"MGX_MSBFS_SHORT_MAX", "rows of at most N entries are expanded a lane each (default 32)"},
    {"MGX_MSBFS_WAVE_MAX", "longer rows of at most N entries take a wave each, the rest go out as (vertex, segment) items (default 1024)"},
    {"MGX_MSBFS_SEG", "entries of a segmented row one wave takes (default 1024)"},
    {"MGX_MSBFS_PULL_DIV", "0 / N: every level pushes / a level pulls when its front's out-entries x N >= m (default 8; 2^30: whenever the front has an out-entry)"},
    // ---- random walks (rw_opts_t::from_env: read once per handle; the three cuts are unmeasured guesses)
    {"MGX_RW_TRIES", "candidates a weighted or second-order step draws before it falls back to the row's first maximum-weight entry (default 64)"},
    {"MGX_RW_TILE", "path slots a workgroup stages in LDS before it stores them transposed, a power of two in [1, 64] (default 16; 1: every slot on its own)"},
    {"MGX_RW_SHORT_MAX", "the setup finds the maximum weight of rows of at most N entries a lane each (default 32)"},
    {"MGX_RW_WAVE_MAX", "longer rows of at most N entries take a wave each, the rest go out as (vertex, segment) items (default 1024)"},
    {"MGX_RW_SEG", "entries of a segmented row one wave takes (default 1024)"},
    // ---- neighbour sampling (ns_opts_t::from_env: read once per handle; all three defaults are unmeasured guesses)
    {"MGX_NSAMPLE_SHORT_MAX", "a hop that takes whole rows (fan-out -1) copies rows of at most N entries a lane each (default 32)"},
    {"MGX_NSAMPLE_WAVE_MAX", "longer rows of at most N entries take a wave each, the rest go out as (row, segment) items (default 1024)"},
    {"MGX_NSAMPLE_SEG", "entries of a segmented row one wave copies (default 1024)"},
    // ---- neighbour feature aggregation (agg_seg_from_env: read once per handle, at its first call; 256 against 64 and 1024: DESIGN 3.23)
    {"MGX_AGG_SEG", "entries of a row's segment, a power of two in [64, 4096]: a row of at most N entries is one left-to-right fold by a team of lanes, a longer one goes out as (row, segment) items whose values are combined in segment order (default 256); part of the result's definition"},
    // ---- vertex similarity (sim_opts_t::from_env: read once per handle; short_max and wave_max are unmeasured guesses)
    {"MGX_SIM_SHORT_MAX", "pairs whose shorter adjacency row has at most N entries take a lane each: every entry searched in the longer row (default 16)"},
    {"MGX_SIM_PROBE_RATIO", "longer short rows against rows of at least N times their length take a group of 16 lanes searching the long row in global memory; the rest are staged (default 8: measured at rows of 256)"},
    {"MGX_SIM_WAVE_MAX", "staged pairs whose shorter row has at most N entries take a wave and its LDS stage, the rest a workgroup (default 512)"},
    {"MGX_SIM_STAGE", "entries of an LDS stage of the shorter row; a longer one is staged in chunks against slices of the long row (default and at most 4096; a wave's: 512)"},
    {"MGX_LOUVAIN_SHORT_MAX", "Louvain: vertices whose rows have at most N entries score their candidates a lane each, labels and weights in registers (default and at most 16)"},
    {"MGX_LOUVAIN_WAVE_MAX", "Louvain: longer rows of at most N entries take a wave each and a wave-private LDS table; the rest go out as (vertex, segment) items into a table in device memory (default 256, at most 512)"},
    {"MGX_LOUVAIN_SEG", "Louvain: entries of a long row one wave takes, a power of two in [64, 1024] (default 256)"},
    // ---- betweenness centrality (bc_opts_t::from_env: read once per handle; all four defaults are unmeasured guesses)
    {"MGX_BC_LANE_MAX", "rows of at most N entries are folded by one lane (default 16)"},
    {"MGX_BC_HUGE_MIN", "rows of at least N entries are cut into segments folded by several workgroups, the rest by a wave (default 8192)"},
    {"MGX_BC_SEG", "entries of a huge row's segment (default 8192)"},
    {"MGX_BC_CHAIN", "0 / N: no chain / levels of at most N vertices in a row run in one workgroup's launch (default 1024)"},
    // ---- minimum spanning forest (mst_opts_t::from_env: read per run; both defaults are unmeasured guesses)
    {"MGX_MST_LONG_MIN", "rows with at least N entries left behind the cursor are scanned by a wave, 64 entries a step (default 64)"},
    {"MGX_MST_SEG", "entries of a long row's window, a wave each; rounded up to a multiple of 64 (default 2048)"},
    // ---- neighbour-reduce
    {"MGX_NR_SLICED", "0: the unit blocks instead of the long rows by slice of their destinations"},
    {"MGX_NR_SLICES", "number of hot slices (default: by graph size; at most what the id range holds)"},
    {"MGX_NR_FOLD_DEGS", "\"a/b/c\": the fold's tiers (a workgroup / a wave / eight lanes per row) from these degrees"},
    {"MGX_NR_SUBSET", "0: subset frontiers take the general kernel"},
    {"MGX_NR_PARTS", "1 / 2 / 3: timing runs of the short rows only / the long rows only / both"},
    // ---- partitioned BFS (rank engines)
    {"MGX_DIST_SPEC", "0: a host look per level instead of the level plan"},
    {"MGX_DIST_SPARSE_PUSH", "0: every level sweeps the marks"},
    {"MGX_DIST_DECLARE_MUL", "a sweep fills its id list unless the push stored > N x capacity marks (0: always)"},
    {"MGX_DIST_FUSED_MERGE", "0: OR-merge and queue build as two launches"},
    {"MGX_DIST_BUILD_LIST", "1: list-based queue build on the ranks"},
    {"MGX_DIST_PUSH_SPLIT", "1: the parts of a rank's push as separate launches (statistics)"},
    {"MGX_DIST_DEFER", "0: no deferred hot marks on the ranks"},
    {"MGX_DIST_DENSE_DIV", "a level reads the unit blocks when it holds >= 1 / N of the rank's units"},
    {"MGX_DIST_VSHORT", "0 / N: short rows vertex by vertex never / threshold divisor"},
    {"MGX_DIST_COLD", "0: no cold-edge lists per rank"},
    {"MGX_DIST_COLD_WGS", "cold workgroups per rank (measurements)"},
    {"MGX_DIST_COLD_REDUCE", "0: the sweep ORs the cold bitmaps itself"},
    {"MGX_DIST_HOT_UNITS", "0: unit blocks with all entries on the ranks"},
    {"MGX_LOOPBACK_TIMEOUT_S", "deadline of every wait of the loopback communicator (seconds, default 120)"},
    // ---- every context (standard_context_t: read once when the context is created)
    {"MGX_GRID_CUS", "(tests) N: the context counts min(N, the device's) compute units, at least 1 (a non-number counts as 1): chip-sized grids shrink to N * 8 workgroups"},
  };
  *count = (int)(sizeof(table) / sizeof(table[0]));
  return table;
}

// value of a switch; NULL when unset or empty.  A name that is not in the table is a bug in the caller.
inline const char* env(const char* name) {
  int n = 0;
  const env_switch_t* t = env_switches(&n);
  bool known = false;
  for (int i = 0; i < n && !known; ++i) known = std::strcmp(t[i].name, name) == 0;
  if (!known) {
    std::fprintf(stderr, "mgx: environment switch %s is not in the table of include/mgx/env.hpp\n", name);
    std::abort();
  }
  const char* e = std::getenv(name);
  return (e && *e) ? e : nullptr;
}

// an integer switch: `fallback` when unset or empty, else its value clamped to [lo, hi] (no digits: 0, then clamped)
inline int env_int(const char* name, int lo, int hi, int fallback) {
  const char* e = env(name);
  if (!e) return fallback;
  const long long v = std::strtoll(e, nullptr, 10);
  return (int)(v < lo ? lo : (v > hi ? hi : v));
}

}  // namespace mgx
