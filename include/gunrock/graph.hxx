// gunrock/graph.hxx -- host CSR, device graph, MTX loader.
// Drop-in for the reference's gunrock/src/graph.hxx (csr_t :19-26, graph_t :28-35,
// graph_device_t :37-58, graph_to_device :60-83, load_graph :96-223): same type and member
// names, so problem/enactor/functor code written against the reference compiles against
// this file.  Memory layer is mgx::mem_t (HIP), not moderngpu.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <limits>
#include <memory>
#include <tuple>
#include <vector>

#include "../mgx/runtime.hpp"
#include "../mgx/row_layout.hpp"
#include "../mgx/src_shapes.hpp"

// The reference's sources say `using namespace mgpu;` and `mgpu::fill<...>` for the memory
// layer (graph.hxx:15, bfs_enactor.hxx:83); mgx is that layer here.
namespace mgpu = mgx;
using namespace mgx;

namespace gunrock {

struct csr_t {
  int num_nodes;
  int num_edges;
  std::vector<int> offsets;
  std::vector<int> indices;
  std::vector<float> edge_weights;
  std::vector<int> sources;
};

struct graph_t {
  bool undirected;
  int num_nodes;
  int num_edges;
  std::shared_ptr<csr_t> csr;
  std::shared_ptr<csr_t> csc;
};

struct graph_device_t {
  int num_nodes;
  int num_edges;
  mem_t<int> d_row_offsets;
  mem_t<int> d_col_indices;
  mem_t<float> d_col_values;
  mem_t<int> d_col_offsets;
  mem_t<int> d_row_indices;
  mem_t<float> d_row_values;
  mem_t<int> d_csr_srcs;
  mem_t<int> d_csc_srcs;

  // exclusive degree scan of the frontier currently being advanced (advance.hxx:28,40).
  // The reference sizes it num_nodes although it is indexed by frontier slot;
  // here operators grow it once to the input frontier's capacity (ensure_scanned).
  mem_t<int> d_scanned_row_offsets;

  // true when the CSC slots alias the CSR arrays (what the reference always has)
  bool csc_is_csr = true;

  // Optional hub-first layout for the fused traversal (not in the reference): the same graph with
  // vertex ids renumbered by descending degree, plus both id maps.  Operators keep using the
  // arrays above; results are always reported in original ids.
  mem_t<int> d_layout_row_offsets;
  mem_t<int> d_layout_col_indices;
  mem_t<float> d_layout_col_values;   // optional: weights in layout order (fused SSSP)
  bool has_layout_weights = false;
  mem_t<int> d_new_of_old;
  mem_t<int> d_old_of_new;
  bool has_layout = false;
  // What the fused BFS runs on, derived from the layout (mgx/row_layout.hpp): the unit blocks of its long rows (built with the layout;
  // for graphs of at most 2^23 vertices their entries at 24 bits only -- MGX_BFS_PACK24=0 keeps the 32-bit ones), the degree classes
  // of its short rows (only for a layout the library built itself: sorted by degree, eight ints of -1 behind its neighbour array), the
  // cold-edge lists and the unit blocks without their entries (when the cold entries are a small share of the long rows').
  mgx::row_layout_t rows;
  mem_t<unsigned long long> d_nr_pos;   // neighbour-reduce over a SUBSET frontier (mgx/nreduce.hpp): (epoch, frontier position) per layout vertex; allocated and zeroed at the first such call
  mem_t<float> d_ub_w;               // weights of the unit blocks' entries (fused SSSP's heavy iterations); built on first use
  mem_t<unsigned short> d_ub_w16;    // the same weights as IEEE halves, kept only when every one of them is exact that way (fused SSSP's sweep, 24-bit entries)
  bool ub_w_tried = false;
  // What a traversal FROM vertex v starts with, by original id, on the host (mgx::bfs_src_shape_t, bfs_fused_run.hpp): the
  // source's own row and the level behind it -- its distinct neighbours other than itself that have entries: true edges,
  // rows below and from the long-row threshold.  The fused BFS sizes a traversal's launch sequence from it before the
  // first kernel is enqueued (which of the two small-level launches in front of the device-wide slots will find work).
  // Built by mgx_graph_build_layout (rows sorted by neighbour: duplicates are adjacent); empty: not available.
  // what a traversal from a source starts with (mgx/src_shapes.hpp): computed for the sources that are asked for and remembered --
  // round 6; until then 16 bytes per VERTEX of host memory, filled by a kernel that read 9.8 GB on RMAT-22 when the layout was built
  mgx::src_shape_cache_t src_shape_cache;
  bool src_shapes_enabled = true;    // (false: every traversal gets the graph-wide launch sequence; MGX_BFS_SRC_PLAN=0 is the run-time switch)
  unsigned nr_big_rows = 0;          // layout rows [0, nr_big_rows) hold more than mgx::NR_BIG_UNITS units (degree-sorted layouts)
  // The long rows by slice of their destinations for the full-frontier neighbour-reduce (mgx/nreduce.hpp: k_nrs_edges; built by the
  // library at the graph's first such reduce, mgx_layout.hip: mgx_nrs_build_device): 16-byte mini-units (4 words each), where a
  // row's mini-units of a slice start, the slices' first mini-units.  Empty: not built (the unit blocks serve).
  mem_t<unsigned> d_nrs_mu;
  mem_t<unsigned> d_nrs_off;
  unsigned nrs_first[98] = {0};      // (mgx::NRS_MAX_SLICES + 2)
  unsigned nrs_slices = 0, nrs_rows = 0;
  unsigned nrs_tier[3] = {0, 0, 0};  // k_nrs_fold: rows [0, t0) a workgroup each, [t0, t1) a wave, [t1, t2) eight lanes, the others a thread
  long long nrs_units = 0;
  bool nrs_tried = false;

  graph_device_t() : num_nodes(0), num_edges(0) {}

  void ensure_scanned(size_t slots, standard_context_t& ctx) {
    if (d_scanned_row_offsets.size() >= slots + 1) return;
    ctx.synchronize();
    d_scanned_row_offsets = mem_t<int>(slots + 1, ctx);
  }
};

// graph.hxx:60-83.  The reference uploads the CSC copies as separate buffers; the CSC slots
// here borrow the CSR buffers unless the host graph carries a genuine CSC.
inline void graph_to_device(std::shared_ptr<graph_device_t> d_graph, std::shared_ptr<graph_t> graph,
                            standard_context_t& context) {
  d_graph->num_nodes = graph->num_nodes;
  d_graph->num_edges = graph->num_edges;
  d_graph->d_row_offsets = to_mem(graph->csr->offsets, context);
  d_graph->d_col_values = to_mem(graph->csr->edge_weights, context);
  d_graph->d_col_indices = to_mem(graph->csr->indices, context);
  d_graph->d_csr_srcs = to_mem(graph->csr->sources, context);
  const bool own_csc = graph->csc && graph->csc != graph->csr;
  if (own_csc) {
    d_graph->d_col_offsets = to_mem(graph->csc->offsets, context);
    d_graph->d_row_indices = to_mem(graph->csc->indices, context);
    d_graph->d_row_values = to_mem(graph->csc->edge_weights, context);
    d_graph->d_csc_srcs = to_mem(graph->csc->sources, context);
    d_graph->csc_is_csr = false;
  } else {
    d_graph->d_col_offsets = mem_t<int>::borrow(d_graph->d_row_offsets.data(), d_graph->d_row_offsets.size());
    d_graph->d_row_indices = mem_t<int>::borrow(d_graph->d_col_indices.data(), d_graph->d_col_indices.size());
    d_graph->d_row_values = mem_t<float>::borrow(d_graph->d_col_values.data(), d_graph->d_col_values.size());
    d_graph->d_csc_srcs = mem_t<int>::borrow(d_graph->d_csr_srcs.data(), d_graph->d_csr_srcs.size());
    d_graph->csc_is_csr = true;
  }
  d_graph->d_scanned_row_offsets = mem_t<int>((size_t)graph->num_nodes + 1, context);
  // every operator on this graph may scan/compact up to num_edges work items
  context.reserve_scratch((size_t)graph->num_edges / 2 + ((size_t)graph->num_nodes + 4096) * 2 + (1 << 20));
}

inline void display_csr(std::shared_ptr<csr_t> csr) {
  std::cout << "offsets: \n";
  for (int x : csr->offsets) std::cout << x << ' ';
  std::cout << "\nindices: \n";
  for (int x : csr->indices) std::cout << x << ' ';
  std::cout << std::endl;
}

// Build a CSR whose row is tuple field `row_field` and whose neighbour is the other field,
// rows ascending, neighbours ascending inside a row, duplicates and self loops kept.
inline std::shared_ptr<csr_t> csr_from_tuples(int num_vertices, std::vector<std::tuple<int, int, float>> tuples,
                                              int row_field) {
  auto row_of = [row_field](const std::tuple<int, int, float>& t) { return row_field ? std::get<1>(t) : std::get<0>(t); };
  auto nbr_of = [row_field](const std::tuple<int, int, float>& t) { return row_field ? std::get<0>(t) : std::get<1>(t); };
  std::stable_sort(tuples.begin(), tuples.end(),
                   [&](const std::tuple<int, int, float>& a, const std::tuple<int, int, float>& b) {
                     if (row_of(a) != row_of(b)) return row_of(a) < row_of(b);
                     return nbr_of(a) < nbr_of(b);
                   });
  const int m = (int)tuples.size();
  auto out = std::make_shared<csr_t>();
  out->num_nodes = num_vertices;
  out->num_edges = m;
  out->offsets.assign((size_t)num_vertices + 1, m);
  out->indices.resize(m);
  out->sources.resize(m);
  out->edge_weights.resize(m);
  int cur = -1;
  for (int e = 0; e < m; ++e) {
    while (cur < row_of(tuples[e])) out->offsets[++cur] = e;
    out->sources[e] = cur;
    out->indices[e] = nbr_of(tuples[e]);
    out->edge_weights[e] = std::get<2>(tuples[e]);
  }
  return out;
}

// MTX text loader with the reference's conventions (graph.hxx:96-223):
//  * first non-'%' line "rows cols nnz"; entries "a b [w]", 1-based;
//  * a line "a b" becomes CSR row b-1 with neighbour a-1 (row = 2nd field);
//  * _undir appends the swapped copy of every entry, nothing is de-duplicated;
//  * missing weight -> 1.0f, or rand()%64 when _random_edge_value;
//  * the returned csc IS the csr (the reference builds a genuine CSC into a shadowed local
//    and discards it); pass _genuine_csc to get the transpose instead (needed for pull-BFS
//    on directed inputs, BASELINE config 4).
// Returns nullptr when the file cannot be opened (as the reference) and also on a parse
// error (the reference prints and exit(0)s there).
inline std::shared_ptr<graph_t> load_graph(const char* _name, bool _undir = false, bool _random_edge_value = false,
                                           bool _genuine_csc = false) {
  FILE* f = fopen(_name, "r");
  if (!f) return nullptr;
  char line[100];
  bool header = false;
  while (fgets(line, 100, f)) {
    if (line[0] != '%') { header = true; break; }
  }
  int height, width, nnz;
  if (!header || 3 != sscanf(line, "%d %d %d", &height, &width, &nnz) || height < 0 || nnz < 0 ||
      (long long)nnz * (_undir ? 2 : 1) > 2147483647LL) {
    printf("Error reading %s\n", _name);
    fclose(f);
    return nullptr;
  }
  std::vector<std::tuple<int, int, float>> tuples;
  // (room for what the size line promises -- up to a point: the line is not believed before the entries have been read; a
  //  file that claims 2 G entries and holds two must not cost a 24 GB reservation first)
  tuples.reserve(std::min((size_t)nnz * (_undir ? 2 : 1), (size_t)1 << 24));
  for (int e = 0; e < nnz; ++e) {
    int a, b, items;
    float w;
    if (!fgets(line, 100, f) || (items = sscanf(line, "%d %d %f", &a, &b, &w)) < 2) {
      printf("Error reading edge lists %s\n", _name);
      fclose(f);
      return nullptr;
    }
    // ids are 1-based and index an n x n adjacency (num_nodes = height): an id outside [1, height] would index past
    // offsets[] in csr_from_tuples and past every per-vertex device array later (the reference has the same hole)
    if (a < 1 || b < 1 || a > height || b > height) {
      printf("Error reading edge lists %s: entry %d (%d %d) outside 1..%d\n", _name, e, a, b, height);
      fclose(f);
      return nullptr;
    }
    if (items == 2) w = _random_edge_value ? (float)(rand() % 64) : 1.0f;
    tuples.emplace_back(a - 1, b - 1, w);
  }
  fclose(f);
  if (_undir) {
    for (int e = 0; e < nnz; ++e)
      tuples.emplace_back(std::get<1>(tuples[e]), std::get<0>(tuples[e]), std::get<2>(tuples[e]));
  }
  auto csr = csr_from_tuples(height, tuples, 1);
  std::shared_ptr<csr_t> csc = csr;
  if (_genuine_csc && !_undir) csc = csr_from_tuples(height, tuples, 0);
  auto g = std::make_shared<graph_t>();
  g->undirected = _undir;
  g->num_nodes = height;
  g->num_edges = (int)tuples.size();
  g->csr = csr;
  g->csc = csc;
  return g;
}

// ---- binary CSR cache ----------------------------------------------------------------------------------
// load_graph parses MatrixMarket TEXT and sorts the tuples on every run: minutes for a 69 M-edge file.  save_graph_cache
// writes what it produced -- CSR (and the CSC when it is a genuine one) -- as raw arrays behind a small header;
// load_graph_cache maps it back into a graph_t without parsing or sorting.  Layout (little endian, as the host):
//   char magic[8] = "MGXCSR2\0"; int32 num_nodes, num_edges, undirected, has_csc; uint64 checksum (FNV-1a over the four header
//   words and the arrays: a flipped `undirected` flag is a corrupt file too -- version 1 hashed the arrays only)
//   int32 offsets[n + 1]; int32 indices[m]; float weights[m];  [ int32 col_offsets[n + 1]; int32 row_indices[m]; float row_weights[m] ]
// A file that is truncated, has another magic or fails the checksum is rejected (nullptr / false): a cache is never trusted.
namespace detail {
inline unsigned long long fnv1a(const void* data, size_t bytes, unsigned long long h) {
  const unsigned char* p = (const unsigned char*)data;
  for (size_t i = 0; i < bytes; ++i) { h ^= p[i]; h *= 1099511628211ull; }
  return h;
}
inline unsigned long long csr_checksum(const csr_t& c, unsigned long long h) {
  h = fnv1a(c.offsets.data(), c.offsets.size() * sizeof(int), h);
  h = fnv1a(c.indices.data(), c.indices.size() * sizeof(int), h);
  return fnv1a(c.edge_weights.data(), c.edge_weights.size() * sizeof(float), h);
}
}  // namespace detail

inline bool save_graph_cache(const char* path, const graph_t& g) {
  if (!g.csr || (int)g.csr->offsets.size() != g.num_nodes + 1 || (int)g.csr->indices.size() != g.num_edges ||
      (int)g.csr->edge_weights.size() != g.num_edges)
    return false;
  const bool has_csc = g.csc && g.csc != g.csr;
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  const char magic[8] = {'M', 'G', 'X', 'C', 'S', 'R', '2', 0};
  const int head[4] = {g.num_nodes, g.num_edges, g.undirected ? 1 : 0, has_csc ? 1 : 0};
  unsigned long long sum = detail::fnv1a(head, sizeof(head), 1469598103934665603ull);
  sum = detail::csr_checksum(*g.csr, sum);
  if (has_csc) sum = detail::csr_checksum(*g.csc, sum);
  bool ok = fwrite(magic, 1, 8, f) == 8 && fwrite(head, sizeof(int), 4, f) == 4 && fwrite(&sum, sizeof(sum), 1, f) == 1;
  auto put = [&](const csr_t& c) {
    ok = ok && fwrite(c.offsets.data(), sizeof(int), c.offsets.size(), f) == c.offsets.size();
    ok = ok && fwrite(c.indices.data(), sizeof(int), c.indices.size(), f) == c.indices.size();
    ok = ok && fwrite(c.edge_weights.data(), sizeof(float), c.edge_weights.size(), f) == c.edge_weights.size();
  };
  put(*g.csr);
  if (has_csc) put(*g.csc);
  ok = (fclose(f) == 0) && ok;
  return ok;
}

inline std::shared_ptr<graph_t> load_graph_cache(const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) return nullptr;
  char magic[8];
  int head[4];
  unsigned long long sum = 0;
  const char want[8] = {'M', 'G', 'X', 'C', 'S', 'R', '2', 0};
  if (fread(magic, 1, 8, f) != 8 || memcmp(magic, want, 8) != 0 || fread(head, sizeof(int), 4, f) != 4 ||
      fread(&sum, sizeof(sum), 1, f) != 1 || head[0] < 0 || head[1] < 0) {
    fclose(f);
    return nullptr;
  }
  const size_t n = (size_t)head[0], m = (size_t)head[1];
  {
    // the header is not believed before the file's LENGTH agrees with it: nothing is allocated by numbers a truncated or
    // corrupt file merely claims (a flipped bit in num_nodes used to cost a multi-gigabyte allocation before the short read
    // was noticed)
    const unsigned long long per_csr = (unsigned long long)(n + 1) * sizeof(int) + (unsigned long long)m * (sizeof(int) + sizeof(float));
    const unsigned long long expect = 8ull + 4ull * sizeof(int) + sizeof(sum) + per_csr * (head[3] ? 2ull : 1ull);
    const long at = ftell(f);
    bool size_ok = at >= 0 && fseek(f, 0, SEEK_END) == 0;
    const long end = size_ok ? ftell(f) : -1;
    size_ok = size_ok && end >= 0 && (unsigned long long)end == expect && (head[3] == 0 || head[3] == 1) && fseek(f, at, SEEK_SET) == 0;
    if (!size_ok) {
      fclose(f);
      return nullptr;
    }
  }
  auto get = [&](std::shared_ptr<csr_t>& c) -> bool {
    c = std::make_shared<csr_t>();
    c->num_nodes = (int)n; c->num_edges = (int)m;
    c->offsets.resize(n + 1); c->indices.resize(m); c->edge_weights.resize(m);
    if (fread(c->offsets.data(), sizeof(int), n + 1, f) != n + 1 || fread(c->indices.data(), sizeof(int), m, f) != m ||
        fread(c->edge_weights.data(), sizeof(float), m, f) != m)
      return false;
    // structural sanity before anything indexes with these arrays
    if (c->offsets[0] != 0 || c->offsets[n] != (int)m) return false;
    for (size_t v = 0; v < n; ++v) if (c->offsets[v] > c->offsets[v + 1]) return false;
    for (size_t e = 0; e < m; ++e) if (c->indices[e] < 0 || (size_t)c->indices[e] >= n) return false;
    c->sources.resize(m);
    for (size_t v = 0; v < n; ++v) for (int e = c->offsets[v]; e < c->offsets[v + 1]; ++e) c->sources[e] = (int)v;
    return true;
  };
  auto g = std::make_shared<graph_t>();
  g->num_nodes = (int)n; g->num_edges = (int)m; g->undirected = head[2] != 0;
  bool ok = get(g->csr);
  if (ok && head[3]) ok = get(g->csc); else g->csc = g->csr;
  char extra;
  ok = ok && fread(&extra, 1, 1, f) == 0;                 // nothing behind the arrays
  fclose(f);
  if (!ok) return nullptr;
  unsigned long long have = detail::fnv1a(head, sizeof(head), 1469598103934665603ull);
  have = detail::csr_checksum(*g->csr, have);
  if (g->csc != g->csr) have = detail::csr_checksum(*g->csc, have);
  return have == sum ? g : nullptr;
}

}  // namespace gunrock
