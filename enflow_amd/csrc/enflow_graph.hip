// enflow_graph.hip -- the plumbing around the edge-list kernels (enflow_list.hip,
// the list backward), built once per topology instead of once per call: a
// caller's (row, col) as the CSR those kernels read, the CSC view the backward's
// column sums read, and the two per-call moves of coord_diff between the
// caller's edge order and the sorted one.
//
// The sort is a stable least-significant-digit radix sort on 8-bit digits of the
// clamped row (the CSC: of the sorted list's col).  Keys are below num_nodes <=
// 2^22, so it runs ceil(bits(num_nodes - 1) / 8) = 1 .. 3 passes of
//
//   gr_hist_kernel     one wave per tile of WTILE consecutive edges: how many of
//                      them carry each digit, hist[digit][tile]
//   gr_scan_kernel     one workgroup per digit: exclusive scan of its hist row
//                      over the tiles, the digit's total
//   gr_scatter_kernel  the same tiles: an edge goes to (digits below) + (its
//                      digit in earlier tiles) + (its digit earlier in the tile)
//
// and closes with gr_finish_kernel: row_ptr[r] = the first sorted edge whose key
// is >= r (binary search, one thread per row: empty rows and a row that holds
// every edge cost the same) and, for the CSR, col through the order, clamped to
// [-1, num_nodes] before the int32 cast.
//
// Equal digits inside a tile are ranked by ballot: eight ballots give each lane
// the mask of lanes that hold its digit, the popcount below the lane is its rank
// among them and the lowest of them adds the group to the wave's counter.  A list
// whose edges all share one row is 64 equal lanes: one broadcast LDS read and one
// write per 64 edges, like any other list.  Waves never share a counter, so there
// is no atomic in the placement and no barrier; the only atomic is the OR of
// ENFLOW_ERR_INDEX into the bad-row word.  Integer work only: two builds are
// bitwise equal, and equal to torch.sort(stable=True) on the same keys.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "enflow_hip.h"
#include "enflow_timing.h"

namespace {

constexpr int GR_BLOCK = 256;                      // 4 waves
constexpr int GR_WAVES = GR_BLOCK / 64;
constexpr int GR_ITEMS = 8;                        // rounds of 64 edges per wave
constexpr int GR_WTILE = 64 * GR_ITEMS;            // edges per wave: 512
constexpr int GR_TILE = GR_WAVES * GR_WTILE;       // edges per workgroup: 2048
constexpr int GR_DIGITS = 256;
constexpr int GR_MAX_NODES = 1 << 22;

// A wave's own LDS traffic is FIFO; this keeps the compiler from moving LDS
// accesses across the point and drains outstanding ones.
__device__ __forceinline__ void gr_wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

struct GrPass {
  const void* src_key;      // first pass: the caller's row (int32 / int64) or the sorted col (int32); later: uint32 keys
  const uint32_t* src_val;  // null in the first pass: the edge's own index
  uint32_t* dst_key;
  int32_t* dst_val;
  int32_t* hist;            // [GR_DIGITS][tiles]
  int32_t* total;           // [GR_DIGITS]
  int32_t* bad;             // first pass of the CSR: ENFLOW_ERR_INDEX for a clamped row (may be null)
  int num_nodes, num_edges, tiles, shift;
};

// the key of edge e: SRC 0 the previous pass's uint32 keys; 4 / 8 an int32 /
// int64 index clamped to [0, num_nodes) (changed: the index was out of range)
template <int SRC>
__device__ __forceinline__ uint32_t gr_key(const GrPass& P, int e, bool& changed) {
  if constexpr (SRC == 0) {
    return static_cast<const uint32_t*>(P.src_key)[e];
  } else {
    long long v;
    if constexpr (SRC == 4) v = static_cast<const int32_t*>(P.src_key)[e];
    else v = static_cast<const int64_t*>(P.src_key)[e];
    const long long c = v < 0 ? 0 : (v > P.num_nodes - 1 ? P.num_nodes - 1 : v);
    changed = c != v;
    return (uint32_t)c;
  }
}

// lanes of the wave that hold `digit` among the valid ones (wave-uniform control flow)
__device__ __forceinline__ uint64_t gr_peers(uint32_t digit, bool valid) {
  uint64_t peers = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const uint64_t bal = __ballot(bit);
    peers &= bit ? bal : ~bal;
  }
  return peers;
}

template <int SRC>
__global__ void __launch_bounds__(GR_BLOCK) gr_hist_kernel(GrPass P) {
  __shared__ int32_t cnt[GR_WAVES][GR_DIGITS];
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x * GR_WAVES + w;   // wave-uniform; no block barrier below
  if (tile >= P.tiles) return;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
  for (int k = 0; k < GR_DIGITS / 64; ++k) cnt[w][k * 64 + lane] = 0;
  gr_wave_lds_sync();
  const long long e0 = (long long)tile * GR_WTILE;
  bool any_bad = false;
  for (int r = 0; r < GR_ITEMS; ++r) {
    const long long e = e0 + r * 64 + lane;
    const bool valid = e < P.num_edges;
    bool changed = false;
    const uint32_t key = valid ? gr_key<SRC>(P, (int)e, changed) : 0u;
    any_bad |= changed;
    const uint32_t d = (key >> P.shift) & (GR_DIGITS - 1);
    const uint64_t peers = gr_peers(d, valid);
    // one lane per digit present: no two lanes touch a counter in the same round
    if (valid && (peers & lt) == 0) cnt[w][d] += __popcll(peers);
    gr_wave_lds_sync();
  }
#pragma unroll
  for (int k = 0; k < GR_DIGITS / 64; ++k) {
    const int d = k * 64 + lane;
    P.hist[(size_t)d * P.tiles + tile] = cnt[w][d];
  }
  if constexpr (SRC != 0) {
    if (P.bad && __ballot(any_bad) && lane == 0) atomicOr(P.bad, ENFLOW_ERR_INDEX);
  }
}

// exclusive scan of one digit's hist row over the tiles (contiguous chunks per
// thread, fixed order) and the digit's total
__global__ void __launch_bounds__(GR_BLOCK) gr_scan_kernel(GrPass P) {
  __shared__ int32_t part[GR_BLOCK];
  const int d = blockIdx.x, tid = threadIdx.x;
  int32_t* row = P.hist + (size_t)d * P.tiles;
  const int per = (P.tiles + GR_BLOCK - 1) / GR_BLOCK;
  const int c0 = min(P.tiles, tid * per), c1 = min(P.tiles, c0 + per);
  int32_t s = 0;
  for (int t = c0; t < c1; ++t) s += row[t];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int32_t acc = 0;
    for (int k = 0; k < GR_BLOCK; ++k) { const int32_t v = part[k]; part[k] = acc; acc += v; }
    P.total[d] = acc;
  }
  __syncthreads();
  int32_t acc = part[tid];
  for (int t = c0; t < c1; ++t) {
    const int32_t v = row[t];
    row[t] = acc;
    acc += v;
  }
}

template <int SRC>
__global__ void __launch_bounds__(GR_BLOCK) gr_scatter_kernel(GrPass P) {
  __shared__ int32_t cnt[GR_WAVES][GR_DIGITS];   // the next slot of every digit, per wave
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x * GR_WAVES + w;   // wave-uniform; no block barrier below
  if (tile >= P.tiles) return;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  // digits below: lane l owns digits 4 l .. 4 l + 3; exclusive scan of the lane sums by shuffle
  int32_t tot[4];
  int32_t mine = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) { tot[k] = P.total[lane * 4 + k]; mine += tot[k]; }
  int32_t incl = mine;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const int32_t up = __shfl_up(incl, s, 64);
    if (lane >= s) incl += up;
  }
  int32_t base = incl - mine;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = lane * 4 + k;
    cnt[w][d] = base + P.hist[(size_t)d * P.tiles + tile];
    base += tot[k];
  }
  gr_wave_lds_sync();
  const long long e0 = (long long)tile * GR_WTILE;
  for (int r = 0; r < GR_ITEMS; ++r) {
    const long long e = e0 + r * 64 + lane;
    const bool valid = e < P.num_edges;
    bool changed = false;
    const uint32_t key = valid ? gr_key<SRC>(P, (int)e, changed) : 0u;
    const uint32_t d = (key >> P.shift) & (GR_DIGITS - 1);
    const uint64_t peers = gr_peers(d, valid);
    const int32_t first = cnt[w][d];   // equal lanes: one broadcast read
    gr_wave_lds_sync();
    if (valid) {
      const int32_t dst = first + __popcll(peers & lt);
      if ((uint32_t)dst < (uint32_t)P.num_edges) {   // a permutation by construction; never write past the list
        P.dst_key[dst] = key;
        P.dst_val[dst] = P.src_val ? (int32_t)P.src_val[e] : (int32_t)e;
      }
      if ((peers & lt) == 0) cnt[w][d] = first + __popcll(peers);
    }
    gr_wave_lds_sync();
  }
}

struct GrFinish {
  const uint32_t* key;     // sorted
  const int32_t* order;    // sorted edge -> the caller's index
  const void* col;         // the caller's col (null: pointers only, the CSC)
  int col_bytes;
  int32_t* ptr;            // [num_nodes + 1]
  int32_t* col_sorted;     // [num_edges]
  int num_nodes, num_edges;
};

__global__ void __launch_bounds__(GR_BLOCK) gr_finish_kernel(GrFinish F) {
  const long long stride = (long long)gridDim.x * GR_BLOCK;
  const long long work = max((long long)F.num_nodes + 1, (long long)F.num_edges);
  for (long long i = (long long)blockIdx.x * GR_BLOCK + threadIdx.x; i < work; i += stride) {
    if (i <= F.num_nodes) {   // the first sorted edge with key >= i
      int lo = 0, hi = F.num_edges;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if ((long long)F.key[mid] < i) lo = mid + 1; else hi = mid;
      }
      F.ptr[i] = lo;
    }
    if (F.col && i < F.num_edges) {
      int32_t o = F.order[i];
      o = o < 0 ? 0 : (o > F.num_edges - 1 ? F.num_edges - 1 : o);
      // an index past int32 must not wrap into range: -1 and num_nodes stand for every bad col
      long long c = F.col_bytes == 8 ? (long long)static_cast<const int64_t*>(F.col)[o]
                                     : (long long)static_cast<const int32_t*>(F.col)[o];
      c = c < -1 ? -1 : (c > F.num_nodes ? F.num_nodes : c);
      F.col_sorted[i] = (int32_t)c;
    }
  }
}

// coord_diff[order] -> contiguous fp32 (gather) and the sorted d coord_diff back
// to the caller's order and dtype (scatter); one thread per component
template <typename T>
__global__ void __launch_bounds__(GR_BLOCK) gr_gather_kernel(const T* src, const int32_t* order, float* dst, int num_edges) {
  const long long stride = (long long)gridDim.x * GR_BLOCK, work = 3ll * num_edges;
  for (long long t = (long long)blockIdx.x * GR_BLOCK + threadIdx.x; t < work; t += stride) {
    const int i = (int)(t / 3), c = (int)(t - 3ll * i);
    const int32_t o = order[i];
    if ((uint32_t)o < (uint32_t)num_edges) dst[t] = (float)src[(size_t)o * 3 + c];
  }
}

template <typename T>
__global__ void __launch_bounds__(GR_BLOCK) gr_scatter_back_kernel(const float* src, const int32_t* order, T* dst, int num_edges) {
  const long long stride = (long long)gridDim.x * GR_BLOCK, work = 3ll * num_edges;
  for (long long t = (long long)blockIdx.x * GR_BLOCK + threadIdx.x; t < work; t += stride) {
    const int i = (int)(t / 3), c = (int)(t - 3ll * i);
    const int32_t o = order[i];
    if ((uint32_t)o < (uint32_t)num_edges) dst[(size_t)o * 3 + c] = (T)src[t];
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
inline size_t gr_al256(size_t x) { return (x + 255) & ~(size_t)255; }

struct GrWorkspace { size_t key_a, key_b, val, hist, total, bytes; };
GrWorkspace gr_workspace(int64_t num_edges) {
  GrWorkspace W;
  const size_t E = (size_t)num_edges, tiles = (E + GR_WTILE - 1) / GR_WTILE;
  size_t o = 0;
  W.key_a = o; o = gr_al256(o + E * 4);
  W.key_b = o; o = gr_al256(o + E * 4);
  W.val = o; o = gr_al256(o + E * 4);
  W.hist = o; o = gr_al256(o + tiles * GR_DIGITS * 4);
  W.total = o; o = gr_al256(o + GR_DIGITS * 4);
  W.bytes = o;
  return W;
}

int gr_check(int num_nodes, int64_t num_edges) {
  if (num_nodes < 0 || num_edges < 0) return -1;
  if (num_nodes > GR_MAX_NODES || num_edges > (int64_t)INT32_MAX - 1024) return -3;
  return 0;
}

int gr_grid(long long work) {   // grid-stride launches: at most 2048 workgroups
  const long long g = (work + GR_BLOCK - 1) / GR_BLOCK;
  return (int)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

template <int SRC>
void gr_launch_pass(hipStream_t st, const GrPass& P) {
  const int grid = (P.tiles + GR_WAVES - 1) / GR_WAVES;
  ENFLOW_TIMED("gr_hist_kernel", st, hipLaunchKernelGGL((gr_hist_kernel<SRC>), dim3(grid), dim3(GR_BLOCK), 0, st, P));
  ENFLOW_TIMED("gr_scan_kernel", st, hipLaunchKernelGGL(gr_scan_kernel, dim3(GR_DIGITS), dim3(GR_BLOCK), 0, st, P));
  ENFLOW_TIMED("gr_scatter_kernel", st, hipLaunchKernelGGL((gr_scatter_kernel<SRC>), dim3(grid), dim3(GR_BLOCK), 0, st, P));
}

// stable sort of the edges by clamp(index, 0, num_nodes - 1): order_out [E] and
// the pointer array; col != null: the CSR's clamped col through the order as well
int gr_sort(int num_nodes, int64_t num_edges, const void* index, int index_bytes, const void* col, int col_bytes,
            int32_t* ptr_out, int32_t* col_sorted, int32_t* order_out, int32_t* bad, void* workspace, hipStream_t st) {
  const GrWorkspace W = gr_workspace(num_edges);
  char* base = static_cast<char*>(workspace);
  uint32_t* keys[2] = {reinterpret_cast<uint32_t*>(base + W.key_a), reinterpret_cast<uint32_t*>(base + W.key_b)};
  int32_t* val = reinterpret_cast<int32_t*>(base + W.val);
  const int E = (int)num_edges;
  int bits = 1;
  while (bits < 22 && (1ll << bits) < (long long)num_nodes) ++bits;   // keys < num_nodes <= 2^22
  const int passes = (bits + 7) / 8;
  const uint32_t* sorted = keys[0];
  if (E > 0) {
    GrPass P{};
    P.hist = reinterpret_cast<int32_t*>(base + W.hist);
    P.total = reinterpret_cast<int32_t*>(base + W.total);
    P.num_nodes = num_nodes; P.num_edges = E;
    P.tiles = (E + GR_WTILE - 1) / GR_WTILE;
    for (int p = 0; p < passes; ++p) {
      // values alternate between the workspace and order_out so that the last pass writes order_out
      int32_t* vout = ((passes - 1 - p) & 1) ? val : order_out;
      P.shift = 8 * p;
      P.dst_key = keys[p & 1];
      P.dst_val = vout;
      if (p == 0) {
        P.src_key = index; P.src_val = nullptr; P.bad = bad;
        if (index_bytes == 8) gr_launch_pass<8>(st, P); else gr_launch_pass<4>(st, P);
      } else {
        P.src_key = keys[(p - 1) & 1];
        P.src_val = reinterpret_cast<const uint32_t*>(((passes - p) & 1) ? val : order_out);
        P.bad = nullptr;
        gr_launch_pass<0>(st, P);
      }
      sorted = P.dst_key;
    }
  }
  GrFinish F{};
  F.key = sorted; F.order = order_out; F.col = E > 0 ? col : nullptr; F.col_bytes = col_bytes;
  F.ptr = ptr_out; F.col_sorted = col_sorted; F.num_nodes = num_nodes; F.num_edges = E;
  const long long work = (long long)num_nodes + 1 > (long long)E ? (long long)num_nodes + 1 : (long long)E;
  ENFLOW_TIMED("gr_finish_kernel", st, hipLaunchKernelGGL(gr_finish_kernel, dim3(gr_grid(work)), dim3(GR_BLOCK), 0, st, F));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace

extern "C" {

int enflow_graph_sort_tile(void) { return GR_TILE; }

int64_t enflow_graph_workspace_size(int num_nodes, int64_t num_edges) {
  const int rc = gr_check(num_nodes, num_edges);
  if (rc) return rc;
  return (int64_t)gr_workspace(num_edges).bytes;
}

int enflow_graph_csr_build(int num_nodes, int64_t num_edges, const void* row, int row_bytes, const void* col,
                           int col_bytes, int32_t* row_ptr, int32_t* col_sorted, int32_t* order, int32_t* bad_row,
                           void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = gr_check(num_nodes, num_edges);
  if (rc) return rc;
  if ((row_bytes != 4 && row_bytes != 8) || (col_bytes != 4 && col_bytes != 8)) return -1;
  if (!row_ptr || !bad_row || !workspace || (num_edges > 0 && (!row || !col || !col_sorted || !order))) return -1;
  if (workspace_bytes < (int64_t)gr_workspace(num_edges).bytes) return -6;
  if (num_nodes == 0) return 0;   // nothing to build: the forward refuses an edge on a batch without nodes
  return gr_sort(num_nodes, num_edges, row, row_bytes, col, col_bytes, row_ptr, col_sorted, order, bad_row, workspace,
                 reinterpret_cast<hipStream_t>(stream));
}

int enflow_graph_csc_build(int num_nodes, int64_t num_edges, const int32_t* col_sorted, int32_t* col_ptr,
                           int32_t* col_perm, void* workspace, int64_t workspace_bytes, void* stream) {
  const int rc = gr_check(num_nodes, num_edges);
  if (rc) return rc;
  if (!col_ptr || !workspace || (num_edges > 0 && (!col_sorted || !col_perm))) return -1;
  if (workspace_bytes < (int64_t)gr_workspace(num_edges).bytes) return -6;
  if (num_nodes == 0) return 0;
  return gr_sort(num_nodes, num_edges, col_sorted, 4, nullptr, 4, col_ptr, nullptr, col_perm, nullptr, workspace,
                 reinterpret_cast<hipStream_t>(stream));
}

int enflow_graph_gather_f32(int64_t num_edges, const void* coord_diff, int elem_bytes, const int32_t* order,
                            float* out, void* stream) {
  if (num_edges < 0 || (elem_bytes != 4 && elem_bytes != 8)) return -1;
  if (num_edges > (int64_t)INT32_MAX - 1024) return -3;
  if (num_edges == 0) return 0;
  if (!coord_diff || !order || !out) return -1;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int E = (int)num_edges, grid = gr_grid(3ll * E);
  if (elem_bytes == 8)
    ENFLOW_TIMED("gr_gather_kernel", st, hipLaunchKernelGGL((gr_gather_kernel<double>), dim3(grid), dim3(GR_BLOCK), 0, st, static_cast<const double*>(coord_diff), order, out, E));
  else
    ENFLOW_TIMED("gr_gather_kernel", st, hipLaunchKernelGGL((gr_gather_kernel<float>), dim3(grid), dim3(GR_BLOCK), 0, st, static_cast<const float*>(coord_diff), order, out, E));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int enflow_graph_scatter_f32(int64_t num_edges, const float* sorted, const int32_t* order, void* out, int elem_bytes,
                             void* stream) {
  if (num_edges < 0 || (elem_bytes != 4 && elem_bytes != 8)) return -1;
  if (num_edges > (int64_t)INT32_MAX - 1024) return -3;
  if (num_edges == 0) return 0;
  if (!sorted || !order || !out) return -1;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int E = (int)num_edges, grid = gr_grid(3ll * E);
  if (elem_bytes == 8)
    ENFLOW_TIMED("gr_scatter_back_kernel", st, hipLaunchKernelGGL((gr_scatter_back_kernel<double>), dim3(grid), dim3(GR_BLOCK), 0, st, sorted, order, static_cast<double*>(out), E));
  else
    ENFLOW_TIMED("gr_scatter_back_kernel", st, hipLaunchKernelGGL((gr_scatter_back_kernel<float>), dim3(grid), dim3(GR_BLOCK), 0, st, sorted, order, static_cast<float*>(out), E));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
