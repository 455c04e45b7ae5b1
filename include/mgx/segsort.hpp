// mgx/segsort.hpp -- stable segmented sort by a comparator (moderngpu's segmented_sort shape), new HIP for gfx950.
//
// Segments: `heads` are segment heads, ascending, duplicates allowed (empty segments).  Segment s of the num_segments + 1
// pieces is [s == 0 ? 0 : heads[s - 1], s == num_segments ? count : heads[s]): whatever lies before the first head is a
// segment of its own, as a moderngpu tile breaks only at heads.  Each segment is sorted by comp (a strict weak order), stably:
// equal keys keep their order.  Keys are any trivially copyable type of at most 8 bytes; values (optional) ride along.
//
// Shaped by segment length, one classification pass and ONE host wait (the list sizes and the longest segment):
//   * 2 .. SEGSORT_WAVE_MAX items: a wave each, rank sort from a wave-private LDS copy (every lane counts the keys before it);
//   * .. SEGSORT_TILE items: a workgroup each, in LDS: an odd-even transposition of 8 items per thread in registers, then
//     merge passes in which every item finds its place in the partner run by a binary search (stable: ties go left first);
//   * longer: the same workgroup sort on every SEGSORT_TILE tile of the segment, then merge passes confined to the segment,
//     run width SEGSORT_TILE, 2 SEGSORT_TILE, ... : each workgroup writes one tile of output, found by two merge-path searches
//     over the pair of runs, merged in LDS the same way; ping-pong between the keys and a scratch copy, copied back at the end
//     when the number of passes is odd.
// Positions are int: count < 2^31 (the operator path's limit everywhere).
#pragma once
#include <algorithm>
#include <climits>
#include <type_traits>

#include "runtime.hpp"
#include "wave.hpp"
#include "worklist.hpp"

namespace mgx {

constexpr int SEGSORT_WAVE_MAX = WAVE;
constexpr int SEGSORT_PER_THREAD = 8;
constexpr int SEGSORT_TILE = BLOCK * SEGSORT_PER_THREAD;          // 2048

struct segsort_no_value_t {};

template <typename K, typename V>
struct segsort_args_t {
  K* keys;
  V* vals;                 // unused without values
  K* keys_tmp;             // the long band's ping-pong copy (count items; may be null when no segment is long)
  V* vals_tmp;
  int count;
  const int* heads;
  int num_segments;
  int* short_list;         // segments of 2 .. SEGSORT_WAVE_MAX items
  int* mid_list;           // .. SEGSORT_TILE items
  int2* tile_list;         // (segment, tile) of the longer ones
  int* cnt;                // [0] short, [1] mid, [2] tiles, [3] the longest segment
};

__device__ __forceinline__ void segsort_bounds(const int* heads, int ns, int count, int s, int& b, int& e) {
  b = s == 0 ? 0 : heads[s - 1];
  e = s == ns ? count : heads[s];
}

// segment s of len items (0: no segment in this lane) into the list of its band; a longer one a (segment, tile) item per tile.
// All lanes of the wave call it.
template <typename K, typename V>
__device__ __forceinline__ void segsort_classify_one(const segsort_args_t<K, V>& a, int s, int len) {
  wave_append(len >= 2 && len <= SEGSORT_WAVE_MAX, s, a.short_list, a.cnt + 0);
  wave_append(len > SEGSORT_WAVE_MAX && len <= SEGSORT_TILE, s, a.mid_list, a.cnt + 1);
  wave_append_segments(len > SEGSORT_TILE, s, len, SEGSORT_TILE, a.tile_list, a.cnt + 2);
}

template <typename K, typename V>
__global__ __launch_bounds__(BLOCK) void k_segsort_classify(segsort_args_t<K, V> a) {
  const int total = a.num_segments + 1;
  for (long long base = (long long)blockIdx.x * BLOCK; base < total; base += (long long)gridDim.x * BLOCK) {
    const int s = (int)base + (int)threadIdx.x;
    int len = 0;
    if (s < total) {
      int b, e;
      segsort_bounds(a.heads, a.num_segments, a.count, s, b, e);
      len = e - b;
    }
    segsort_classify_one(a, s, len);
    if (len > SEGSORT_TILE) atomicMax(a.cnt + 3, len);
  }
}

// Segments of 2 .. 64 items, a wave each: rank(i) = #{j : comp(k_j, k_i)} + #{j < i : k_j equivalent to k_i}
template <typename K, typename V, typename C>
__global__ __launch_bounds__(BLOCK) void k_segsort_wave(segsort_args_t<K, V> a, C comp) {
  constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
  __shared__ K s_keys[WAVES_PER_BLOCK][SEGSORT_WAVE_MAX];
  K* const sk = s_keys[threadIdx.x / WAVE];
  const int lane = lane_id();
  const int n_items = a.cnt[0];
  const int waves = (int)(gridDim.x * WAVES_PER_BLOCK);
  for (int it = (int)(blockIdx.x * WAVES_PER_BLOCK + threadIdx.x / WAVE); it < n_items; it += waves) {
    int b, e;
    segsort_bounds(a.heads, a.num_segments, a.count, a.short_list[it], b, e);
    const int len = e - b;
    const bool in = lane < len;
    K k{};
    V v{};
    if (in) {
      k = a.keys[b + lane];
      if constexpr (HAS_V) v = a.vals[b + lane];
      sk[lane] = k;
    }
    wave_lds_fence();
    int rank = 0;
    for (int j = 0; j < len; ++j) {
      const K o = sk[j];
      rank += (comp(o, k) || (j < lane && !comp(k, o))) ? 1 : 0;
    }
    if (in) {
      a.keys[b + rank] = k;
      if constexpr (HAS_V) a.vals[b + rank] = v;
    }
    wave_lds_fence();                                       // (read before the next segment fills the copy)
  }
}

// items [lo, hi) of a sorted LDS run: how many come before key (strictly below it when !UPPER, not above it when UPPER)
template <bool UPPER, typename K, typename C>
__device__ __forceinline__ int segsort_search(const K* run, int lo, int hi, K key, C comp) {
  const int base = lo;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const bool before = UPPER ? !comp(key, run[mid]) : comp(run[mid], key);
    if (before) lo = mid + 1;
    else hi = mid;
  }
  return lo - base;
}

// One workgroup sorts len <= SEGSORT_TILE items of src into dst (may be the same array), through sk / sv.
template <typename K, typename V, typename C>
__device__ __forceinline__ void segsort_block(const K* src_k, const V* src_v, K* dst_k, V* dst_v, int len, C comp, K* sk, V* sv) {
  constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
  const int t = (int)threadIdx.x;
  // 8 consecutive items per thread, sorted in registers (odd-even transposition: swaps only on strictly-before, so stable)
  K k[SEGSORT_PER_THREAD];
  V v[SEGSORT_PER_THREAD];
  const int i0 = t * SEGSORT_PER_THREAD;
#pragma unroll
  for (int r = 0; r < SEGSORT_PER_THREAD; ++r) {
    if (i0 + r < len) {
      k[r] = src_k[i0 + r];
      if constexpr (HAS_V) v[r] = src_v[i0 + r];
    }
  }
#pragma unroll
  for (int round = 0; round < SEGSORT_PER_THREAD; ++round) {
#pragma unroll
    for (int r = round & 1; r + 1 < SEGSORT_PER_THREAD; r += 2) {
      if (i0 + r + 1 < len && comp(k[r + 1], k[r])) {
        const K tk = k[r]; k[r] = k[r + 1]; k[r + 1] = tk;
        if constexpr (HAS_V) { const V tv = v[r]; v[r] = v[r + 1]; v[r + 1] = tv; }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < SEGSORT_PER_THREAD; ++r) {
    if (i0 + r < len) {
      sk[i0 + r] = k[r];
      if constexpr (HAS_V) sv[i0 + r] = v[r];
    }
  }
  __syncthreads();
  for (int w = SEGSORT_PER_THREAD; w < len; w <<= 1) {
    int pos[SEGSORT_PER_THREAD];
#pragma unroll
    for (int r = 0; r < SEGSORT_PER_THREAD; ++r) {
      const int i = i0 + r;
      pos[r] = -1;
      if (i < len) {
        k[r] = sk[i];
        if constexpr (HAS_V) v[r] = sv[i];
        const int p = (i / (2 * w)) * (2 * w);
        const int mid = min(p + w, len), end = min(p + 2 * w, len);
        if (i < mid) pos[r] = i + segsort_search<false>(sk, mid, end, k[r], comp);            // left run: after strictly-below of the right
        else pos[r] = p + (i - mid) + segsort_search<true>(sk, p, mid, k[r], comp);          // right run: after not-above of the left
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < SEGSORT_PER_THREAD; ++r) {
      if (pos[r] >= 0) {
        sk[pos[r]] = k[r];
        if constexpr (HAS_V) sv[pos[r]] = v[r];
      }
    }
    __syncthreads();
  }
  for (int i = t; i < len; i += BLOCK) {
    dst_k[i] = sk[i];
    if constexpr (HAS_V) dst_v[i] = sv[i];
  }
  __syncthreads();                                          // (the LDS copy is refilled by the next item)
}

// Segments of 65 .. SEGSORT_TILE items (TILES = false) or every SEGSORT_TILE tile of the longer ones (TILES = true)
template <typename K, typename V, typename C, bool TILES>
__global__ __launch_bounds__(BLOCK) void k_segsort_block(segsort_args_t<K, V> a, C comp) {
  constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
  __shared__ K sk[SEGSORT_TILE];
  __shared__ V sv[HAS_V ? SEGSORT_TILE : 1];
  const int n_items = TILES ? a.cnt[2] : a.cnt[1];
  for (int it = (int)blockIdx.x; it < n_items; it += (int)gridDim.x) {
    int s, t = 0;
    if (TILES) { const int2 x = a.tile_list[it]; s = x.x; t = x.y; }
    else s = a.mid_list[it];
    int b, e;
    segsort_bounds(a.heads, a.num_segments, a.count, s, b, e);
    b += t * SEGSORT_TILE;
    const int len = min(e - b, SEGSORT_TILE);
    segsort_block(a.keys + b, a.vals + (HAS_V ? b : 0), a.keys + b, a.vals + (HAS_V ? b : 0), len, comp, sk, sv);
  }
}

// merge path: how many of the first `diag` outputs of merge(A[0, na), B[0, nb)) come from A (ties: A first)
template <typename K, typename C>
__device__ __forceinline__ int segsort_merge_path(const K* A, int na, const K* B, int nb, int diag, C comp) {
  int lo = max(0, diag - nb), hi = min(diag, na);
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (!comp(B[diag - 1 - mid], A[mid])) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One merge pass of the long band, run width w: a workgroup per output tile of a long segment, src -> dst
template <typename K, typename V, typename C>
__global__ __launch_bounds__(BLOCK) void k_segsort_merge(segsort_args_t<K, V> a, const K* src_k, const V* src_v, K* dst_k, V* dst_v,
                                                         int w, C comp) {
  constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
  __shared__ K sk[SEGSORT_TILE];
  __shared__ V sv[HAS_V ? SEGSORT_TILE : 1];
  __shared__ int s_split[2];
  const int n_items = a.cnt[2];
  for (int it = (int)blockIdx.x; it < n_items; it += (int)gridDim.x) {
    const int2 x = a.tile_list[it];
    int b, e;
    segsort_bounds(a.heads, a.num_segments, a.count, x.x, b, e);
    const int len = e - b;
    const int o0 = x.y * SEGSORT_TILE, o1 = min(o0 + SEGSORT_TILE, len);
    const int p = (o0 / (2 * w)) * (2 * w);
    const int mid = min(p + w, len), end = min(p + 2 * w, len);
    const K* const A = src_k + b + p;
    const K* const B = src_k + b + mid;
    const int na = mid - p, nb = end - mid;
    if (threadIdx.x < 2) s_split[threadIdx.x] = nb == 0 ? (threadIdx.x ? o1 : o0) - p
                                                      : segsort_merge_path(A, na, B, nb, (threadIdx.x ? o1 : o0) - p, comp);
    __syncthreads();
    const int a0 = s_split[0], a1 = s_split[1];
    const int b0 = (o0 - p) - a0, b1 = (o1 - p) - a1;
    const int la = a1 - a0, lb = b1 - b0;
    // A's part then B's part into LDS
    for (int i = (int)threadIdx.x; i < la + lb; i += BLOCK) {
      const int g = i < la ? b + p + a0 + i : b + mid + b0 + (i - la);
      sk[i] = src_k[g];
      if constexpr (HAS_V) sv[i] = src_v[g];
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < la + lb; i += BLOCK) {
      const K key = sk[i];
      const int out = i < la ? i + segsort_search<false>(sk, la, la + lb, key, comp)
                             : (i - la) + segsort_search<true>(sk, 0, la, key, comp);
      dst_k[b + o0 + out] = key;
      if constexpr (HAS_V) dst_v[b + o0 + out] = sv[i];
    }
    __syncthreads();
  }
}

// the long segments' tiles back from the scratch copy (after an odd number of passes)
template <typename K, typename V>
__global__ __launch_bounds__(BLOCK) void k_segsort_copy_back(segsort_args_t<K, V> a) {
  constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
  const int n_items = a.cnt[2];
  for (int it = (int)blockIdx.x; it < n_items; it += (int)gridDim.x) {
    const int2 x = a.tile_list[it];
    int b, e;
    segsort_bounds(a.heads, a.num_segments, a.count, x.x, b, e);
    const int o0 = b + x.y * SEGSORT_TILE, o1 = min(o0 + SEGSORT_TILE, e);
    for (int i = o0 + (int)threadIdx.x; i < o1; i += BLOCK) {
      a.keys[i] = a.keys_tmp[i];
      if constexpr (HAS_V) a.vals[i] = a.vals_tmp[i];
    }
  }
}

// Buffers a caller may own so that a sort allocates nothing: sized once for the largest count and number of segments it will sort
template <typename K, typename V>
struct segsort_workspace_t {
  long long count_cap = 0;
  int segs_cap = 0;
  mem_t<int> short_list, mid_list, cnt;
  mem_t<int2> tile_list;
  mem_t<K> ktmp;
  mem_t<V> vtmp;
  segsort_workspace_t() {}
  segsort_workspace_t(long long count, int num_segments, context_t& ctx) : count_cap(count), segs_cap(num_segments + 1) {
    constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
    short_list = mem_t<int>((size_t)segs_cap, ctx);
    mid_list = mem_t<int>((size_t)segs_cap, ctx);
    cnt = mem_t<int>(4, ctx);
    tile_list = mem_t<int2>((size_t)(2 * (count / SEGSORT_TILE) + 2), ctx);
    ktmp = mem_t<K>((size_t)std::max<long long>(count, 1), ctx);
    vtmp = mem_t<V>(HAS_V ? (size_t)std::max<long long>(count, 1) : 0, ctx);
  }
};

// Host side.  Sorts keys[0, count) (and vals with them, unless V is segsort_no_value_t) in place on the context's stream.
// One host wait for the list sizes; without a workspace the lists and the scratch copy are allocated per call and a second wait
// precedes their release.  With one (large enough, else MGX_E_INVALID) nothing is allocated and the sort returns behind the one
// wait, its last launches still on the stream.  Returns the number of merge passes it ran.
template <typename K, typename V, typename C>
int segmented_sort_impl(K* keys, V* vals, long long count, const int* heads, int num_segments, C comp, standard_context_t& ctx,
                        segsort_workspace_t<K, V>* ws = nullptr) {
  static_assert(sizeof(K) <= 8 && std::is_trivially_copyable<K>::value, "segmented_sort: keys are trivially copyable, at most 8 bytes");
  constexpr bool HAS_V = !std::is_same<V, segsort_no_value_t>::value;
  if (count < 0 || count > INT_MAX || num_segments < 0) throw mgx_error(MGX_E_INVALID, "segmented_sort: count must fit int32");
  if (count < 2) return 0;
  const hipStream_t st = ctx.stream();
  const int segs = num_segments + 1;
  const long long tile_cap = 2 * (count / SEGSORT_TILE) + 2;
  if (ws && (count > ws->count_cap || segs > ws->segs_cap)) throw mgx_error(MGX_E_INVALID, "segmented_sort: the workspace is too small");
  segsort_workspace_t<K, V> own;
  if (!ws) {
    own.short_list = mem_t<int>((size_t)segs, ctx);
    own.mid_list = mem_t<int>((size_t)segs, ctx);
    own.cnt = mem_t<int>(4, ctx);
    own.tile_list = mem_t<int2>((size_t)tile_cap, ctx);
  }
  segsort_workspace_t<K, V>& w = ws ? *ws : own;
  MGX_HIP(hipMemsetAsync(w.cnt.data(), 0, 4 * sizeof(int), st));
  segsort_args_t<K, V> a;
  a.keys = keys; a.vals = vals; a.keys_tmp = nullptr; a.vals_tmp = nullptr;
  a.count = (int)count; a.heads = heads; a.num_segments = num_segments;
  a.short_list = w.short_list.data(); a.mid_list = w.mid_list.data(); a.tile_list = w.tile_list.data(); a.cnt = w.cnt.data();
  const int max_blocks = std::max(ctx.num_cus, 1) * 8;
  hipLaunchKernelGGL((k_segsort_classify<K, V>), dim3(grid_for(segs, BLOCK, max_blocks)), dim3(BLOCK), 0, st, a);
  int h[4];
  MGX_HIP(hipMemcpyAsync(h, w.cnt.data(), sizeof(h), hipMemcpyDeviceToHost, st));
  MGX_HIP(hipStreamSynchronize(st));
  if (h[0] > 0)
    hipLaunchKernelGGL((k_segsort_wave<K, V, C>), dim3(grid_for(h[0], WAVES_PER_BLOCK, max_blocks)), dim3(BLOCK), 0, st, a, comp);
  if (h[1] > 0)
    hipLaunchKernelGGL((k_segsort_block<K, V, C, false>), dim3(std::min(h[1], max_blocks)), dim3(BLOCK), 0, st, a, comp);
  int passes = 0;
  if (h[2] > 0) {
    hipLaunchKernelGGL((k_segsort_block<K, V, C, true>), dim3(std::min(h[2], max_blocks)), dim3(BLOCK), 0, st, a, comp);
    if (!ws) {
      own.ktmp = mem_t<K>((size_t)count, ctx);
      own.vtmp = mem_t<V>(HAS_V ? (size_t)count : 0, ctx);
    }
    a.keys_tmp = w.ktmp.data();
    a.vals_tmp = HAS_V ? w.vtmp.data() : nullptr;
    K* src_k = keys; V* src_v = vals; K* dst_k = a.keys_tmp; V* dst_v = a.vals_tmp;
    for (long long wd = SEGSORT_TILE; wd < h[3]; wd *= 2) {
      hipLaunchKernelGGL((k_segsort_merge<K, V, C>), dim3(std::min(h[2], max_blocks)), dim3(BLOCK), 0, st, a, src_k, src_v, dst_k,
                         dst_v, (int)wd, comp);
      std::swap(src_k, dst_k);
      std::swap(src_v, dst_v);
      ++passes;
    }
    if (passes & 1) hipLaunchKernelGGL((k_segsort_copy_back<K, V>), dim3(std::min(h[2], max_blocks)), dim3(BLOCK), 0, st, a);
  }
  MGX_CHECK_LAUNCH("segmented_sort");
  if (!ws) MGX_HIP(hipStreamSynchronize(st));              // (the scratch copy and the lists are freed on return)
  return passes;
}

}  // namespace mgx
