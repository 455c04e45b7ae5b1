// mgx/row_layout.hpp -- the derived layout of the rows a fused BFS runs on: the unit blocks of the long rows, the
// degree classes of the short rows, the cold-edge lists.  One type for a graph's hub-first layout (graph_device_t::rows) and for
// a rank's shard of the partitioned traversal (d2_state_t::rows); one set of build steps (mini_amd/csrc/mgx_layout.hip) that
// both builders in mgx_capi.hip call, each with its own policy.  Every array is owned here.
#pragma once
#include <vector>
#include "runtime.hpp"

namespace mgx {

// Rows of at least a minimum degree copied into 64-entry units (mgx_layout.hip: mgx_units_build_device, bfs_fused_dense.hpp)
struct unit_blocks_t {
  mem_t<int> col;                    // (units_pad << 6) + 4 entries, padding -1; empty when only the 24-bit copy is kept
  mem_t<unsigned> col24;             // the same, 24 bits each (3 bytes: 4 entries = 12 bytes, -1 = 0xFFFFFF); empty: none
  mem_t<unsigned> col20;             // the same, 20 bits each in chunks of 512 entries (mgx/pack20.hpp, -1 = 0xFFFFF): only for blocks whose ids
                                     // all lie below 2^20 - 1 (the ones without the cold-edge lists' entries), INSTEAD of col24; empty: none
  mem_t<int> owner;                  // units_pad: the row of unit u (padding units: a vertex that is never in a frontier)
  mem_t<unsigned char> cnt;          // real entries of every unit (a graph's full blocks: the neighbour-reduce counts them)
  mem_t<int> first;                  // n + 1: the units of row v are [first[v], first[v + 1]) (a graph's full blocks)
  long long units = 0, units_pad = 0;
};

struct row_layout_t {
  static constexpr int MAX_SLICES = 64;   // (== BFS_COLD_MAX_SLICES: bfs_fused_run.hpp checks)
  // the long rows' unit blocks: rows of >= ub_min_degree entries
  unit_blocks_t ub;
  int ub_min_degree = 0;
  // the same rows WITHOUT the entries that live in the cold-edge lists (what is left points into the LDS prefix): 20 bits per entry
  // on a whole graph (MGX_BFS_PACK20=0: 24), 24 on a rank, whatever the graph's size, owners of their own; a rank keeps the 32-bit
  // entries too (and drops the full blocks)
  unit_blocks_t ubh;
  // degree classes of the short rows (bfs_fused_vshort.hpp): class boundaries of the degree-sorted rows, edges of [vs_v[0], vs_v[3]),
  // the long-row threshold they were cut for, index of four -1 behind the neighbour array (0: not available)
  unsigned vs_v[4] = {0, 0, 0, 0};
  unsigned vs_v9 = 0;                // first row of degree < 9 (inside [vs_v[1], vs_v[2]]): degrees 5 .. 8 take two lanes per vertex
  unsigned vs_edges = 0, vs_dummy = 0;
  int vs_long_min = 0;
  // cold-edge lists (bfs_fused_cold.hpp): the long rows' entries behind the LDS prefix as (owner, dst) pairs grouped by slice of
  // the id range, the same at four bytes each with their 64-chunks' owners (mgx_cold_pack_device), the short rows' pairs
  mem_t<int> cold_owner;
  mem_t<int> cold_dst;
  mem_t<unsigned> cold_pk;
  mem_t<unsigned> cold_cbase;
  unsigned cold_cb[MAX_SLICES + 1] = {0};
  unsigned long long cold_pk_mask = 0;
  mem_t<int> colds_owner;
  mem_t<int> colds_dst;
  long long cold_pairs = 0, colds_pairs = 0;
  int cold_slices = 0;               // slices that hold pairs: first vertex, where their pairs start, their cold workgroups
  unsigned cold_lo[MAX_SLICES] = {0}, cold_off[MAX_SLICES + 1] = {0}, colds_off[MAX_SLICES + 1] = {0}, cold_wgs[MAX_SLICES + 1] = {0};
  unsigned cold_hot_n = 0;           // first vertex the lists cover (0: a flat graph's lists hold every entry)
  int cold_long_min = 0;
  bool cold_majority = false;        // the long rows' entries behind the LDS prefix were too many for lists (more than a quarter of them): a FLAT graph
  bool cold_all = false;             // (round 6) a FLAT graph: the lists hold EVERY entry of every row, slices from vertex 0 on (cold_hot_n == 0)
};

// a rank's local rows -> global ids (mgx/bfs_dist2.hpp: vertex v of rank r is v * ranks + r); ranks == 0: the ids stay
struct owner_remap_t {
  int ranks = 0, rank = 0, n_local = 0, n_global = 0;
};

// ---- build steps (mini_amd/csrc/mgx_layout.hip); device arrays on `s`, a HIP failure throws -----------------------------------
// Unit blocks of the rows [0, n) of at least min_deg entries (hot_limit != 0: only their entries below it), owners remapped;
// keep_index: cnt and first stay.  units == 0: nothing built.
void build_unit_blocks(unit_blocks_t& ub, const int* ro, const int* ci, int n, int min_deg, unsigned hot_limit, const owner_remap_t& remap,
                       bool keep_index, hipStream_t s);
// their 24-bit copy (ub.units > 0), for which the 32-bit entries go unless keep_col
void pack_unit_blocks24(unit_blocks_t& ub, bool keep_col, hipStream_t s);
// their 20-bit copy (ub.units > 0, every id below 2^20 - 1), for which the 32-bit entries go
void pack_unit_blocks20(unit_blocks_t& ub, hipStream_t s);
// first row of fewer than d entries, of rows [0, n) by non-increasing degree (h_ro: a host copy of their n + 1 offsets)
unsigned first_row_below(const std::vector<int>& h_ro, size_t n, int d);
// vs_v, vs_v9 and vs_edges of those rows for the long-row threshold long_min
void cut_degree_classes(row_layout_t& L, const std::vector<int>& h_ro, size_t n, int long_min);
// The (owner, dst) pairs of the rows [row0, row0 + rows) of at least min_deg entries by slice (mgx_cold_build_device); off: per-slice
// offsets (slices + 1).  Returns the pair count; `tolerate`: a HIP failure returns -1 (nothing allocated) instead of throwing.
long long build_cold_pairs(mem_t<int>& owner, mem_t<int>& dst, std::vector<int>& off, const int* ro, const int* ci, int n, int row0, int rows,
                           int min_deg, unsigned hot_n, unsigned slice_n, int slices, hipStream_t s, bool tolerate = false);
// The cold lists around the pairs in L (cold_owner / cold_dst, cold_pairs; colds_* and colds_pairs: the short rows', may be empty) and
// their per-slice offsets off_l / off_s (slice k: [lo0 + k * slice_n, ...)): owners remapped, the slice table of the slices that hold
// pairs, their shares of `wgs` cold workgroups (at least one each), and with `pack` the four-byte copy.  False when more than
// MAX_SLICES slices hold pairs: the lists are dropped.
bool cut_cold_lists(row_layout_t& L, const std::vector<int>& off_l, const std::vector<int>& off_s, unsigned lo0, unsigned slice_n, long long wgs,
                    const owner_remap_t& remap, bool pack, hipStream_t s);

}  // namespace mgx
