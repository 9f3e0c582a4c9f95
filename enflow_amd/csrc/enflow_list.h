// enflow_list.h -- el_layer_kernel, its argument block and instance selection:
// one EGCL layer on a caller-supplied edge list (see enflow_list.hip).  Included
// by enflow_list.hip and, with ENFLOW_LIST_TAPE defined first, by
// enflow_list_tape.hip: the same kernel then compiles as el_layer_tape_kernel,
// which also records the one-layer training tape (the rows' h, message sums and
// Q: what the list backward of enflow_backward.hip re-reads, as lg_layer_kernel
// tapes them).
#pragma once
#include "flow_device.h"

#ifdef ENFLOW_LIST_TAPE
#define ElLayerArgs ElTapeArgs   // a type of its own: one more field
#endif
struct ElLayerArgs {
  const int32_t* row_ptr;   // [n + 1]
  const int32_t* col;       // [E]
  const float* cdiff;       // [E][3]
  const float* h;           // [n][nf]
  const float* layer;       // packed EGCL layer
  float* Q;                 // [n]
  float* F;                 // [n][3]
  float* G;                 // [n][nf]
  int32_t* err;
  int n, num_edges, nf;
  float cw;
#ifdef ENFLOW_LIST_TAPE
  float* tape;              // TapeLayout of one layer over n nodes
#endif
};

#ifdef ENFLOW_LIST_TAPE
#define el_layer_kernel el_layer_tape_kernel
#define EL_KERNEL_NAME "el_layer_tape_kernel"
#else
#define EL_KERNEL_NAME "el_layer_kernel"
#endif

template <int H, int PREC, bool VAR>
__global__ void __launch_bounds__(BLOCK, 1) el_layer_kernel(ElLayerArgs B) {
  using S = Smem<H, 32, 32>;
  __shared__ S sm;
  __shared__ int roff[34];   // [0..32]: the block's row offsets, relative to [33] = the block's first edge
  constexpr int AST = S::AST;
  constexpr int PC = S::PC;
  const int tid = threadIdx.x;
  const int g0 = blockIdx.x * 32;   // first row (grid = ceil(n / 32): g0 < n)
  const int rb = min(32, B.n - g0);
  STAMP_DECL   // diagnostic builds only (-DENFLOW_STAMPS)
  const int nf = B.nf;
  const EgclLayout L = egcl_layout(H, nf);
  for (int e = tid; e < 32 * NFP; e += BLOCK) {   // rows zero-padded past nf and rb
    const int a = e / NFP, q = e - a * NFP;
    sm.h[e] = (a < rb && q < nf) ? B.h[(size_t)(g0 + a) * nf + q] : 0.f;
  }
  if (tid <= 32) roff[tid] = min(max(B.row_ptr[g0 + min(tid, rb)], 0), B.num_edges);
  __syncthreads();
  if (tid == 0) {
    sm.err = 0;
    sm.big = 0u;
    const int e0 = roff[0];
    int acc = e0;
    bool bad = false;
    for (int a = 0; a <= 32; ++a) {   // non-decreasing whatever the caller passed
      const int v = roff[a];
      bad |= v < acc || v != B.row_ptr[g0 + min(a, rb)];
      acc = max(acc, v);
      roff[a] = acc - e0;
    }
    roff[33] = e0;
    if (bad) sm.err = ENFLOW_ERR_INDEX;
  }
  __syncthreads();
  if (tid < 32) sm.cntrow[tid] = roff[tid + 1] - roff[tid];   // 0 past rb
  const int tot = roff[32], e0 = roff[33];
  __syncthreads();
  const MolRef M{};   // no molecule, no box (LIST)
  for (int p0 = 0;;) {   // at least one pass (zeroes the aggregates)
    const int cnt = min(PC, tot - p0);
    for (int e = tid; e < cnt; e += BLOCK) {
      const int pe = p0 + e;
      int lo = 0, hi = rb;   // row il: roff[il] <= pe < roff[il + 1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (roff[mid] <= pe) lo = mid;
        else hi = mid;
      }
      const int c = B.col[(size_t)e0 + pe];
      const bool ok = (uint32_t)c < (uint32_t)B.n;
      sm.pairs[e] = (uint32_t)lo | (ok ? ((uint32_t)c << 5) | (1u << 27) : 0u);
      if (!ok) {   // the reference's IndexError (h[col]); integer LDS atomics: order-free
        atomicSub(&sm.cntrow[lo], 1);
        atomicOr(&sm.err, ENFLOW_ERR_INDEX);
      }
    }
    if (tid == 0) sm.npairs = max(cnt, 0);
    __syncthreads();
    edge_tiles<H, 32, 32, PREC, VAR, true, true>(sm, B.layer, L, M, nf, tid, 0, rb, p0 == 0 STAMP_PASS, nullptr, B.h,
                                                 NoMid{}, false, B.cdiff + ((size_t)e0 + p0) * 3);
    p0 += PC;
    if (p0 >= tot) break;
  }
  if constexpr (PREC != PREC_F32) node_phase_x3<H, 32, 32, VAR>(sm, B.layer, L, rb, nf, tid, 0, rb);
  else node_phase<H, 32, 32, VAR>(sm, B.layer, L, rb, nf, tid, 0, rb);
  if constexpr (PREC == PREC_F16X3) {   // small-operand guard of the row block (BIGK_*)
    if (tid == 0 && small_operands(sm.big)) sm.err |= ENFLOW_ERR_SMALL;
  }
  if (tid == 0 && sm.err) atomicOr(B.err, sm.err);   // index guard; edge tiles' range check (split precision)

#ifdef ENFLOW_LIST_TAPE
  {   // training tape: the rows' h, message sums, Q (pos / vel / g / pair words: not on this path)
    const TapeLayout T = tape_layout(B.n, nf, H, 1);
    float* hx = B.tape + T.hx + (size_t)g0 * T.ldhx;
    for (int e = tid; e < rb * T.ldhx; e += BLOCK) {
      const int a = e / T.ldhx, c = e - a * T.ldhx;
      hx[e] = c < nf ? sm.h[a * NFP + c] : sm.agg[a * AST + (c - nf)];
    }
    for (int a = tid; a < rb; a += BLOCK) B.tape[T.q + g0 + a] = sm.Q[a];
  }
#endif
  for (int a = tid; a < rb; a += BLOCK) {
    const size_t ga = (size_t)(g0 + a);
    const float q = sm.Q[a];
    const float inv = 1.f / fmaxf((float)sm.cntrow[a], 1.f);   // helpers.py:63-70
    float F[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) F[d] = sm.agg[a * AST + H + d] * inv * B.cw;
    if constexpr (PREC != PREC_F32) {   // split-precision GEMM out of range (ENFLOW_ERR_RANGE)
      bool bad = !__builtin_isfinite(q) || !__builtin_isfinite(F[0]) || !__builtin_isfinite(F[1]) ||
                 !__builtin_isfinite(F[2]);
      for (int qf = 0; qf < nf; ++qf) bad |= !__builtin_isfinite(sm.G[a * NFP + qf]);
      if (bad) atomicOr(B.err, ENFLOW_ERR_RANGE);
    }
    B.Q[ga] = q;
    for (int d = 0; d < 3; ++d) B.F[ga * 3 + d] = F[d];
    for (int qf = 0; qf < nf; ++qf) B.G[ga * nf + qf] = sm.G[a * NFP + qf];
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <int HH, int PREC>
static void el_layer_launch(bool var, int grid, hipStream_t st, const ElLayerArgs& B) {
  if (var) ENFLOW_TIMED(EL_KERNEL_NAME, st, hipLaunchKernelGGL((el_layer_kernel<HH, PREC, true>), dim3(grid), dim3(BLOCK), 0, st, B));
  else ENFLOW_TIMED(EL_KERNEL_NAME, st, hipLaunchKernelGGL((el_layer_kernel<HH, PREC, false>), dim3(grid), dim3(BLOCK), 0, st, B));
}
template <int HH>
static void el_layer_prec(int prec, int grid, hipStream_t st, const ElLayerArgs& B) {
  const bool var = (prec & ENFLOW_EGCL_VARIANTS) != 0;
  if ((prec & 0xff) == ENFLOW_PREC_F16X3) el_layer_launch<HH, PREC_F16X3>(var, grid, st, B);
  else el_layer_launch<HH, PREC_F32>(var, grid, st, B);
}

// The body of the C entry of the including translation unit
// (enflow_egcl_forward_list_f32 / enflow_egcl_forward_list_tape_f32; tape: read
// with ENFLOW_LIST_TAPE only).
static inline int el_layer_forward(int num_nodes, int64_t num_edges, int nf, int H,
                                   const int32_t* row_ptr, const int32_t* col, const float* coord_diff,
                                   const float* h, const float* layer, float cw,
                                   float* Q, float* F, float* G, int32_t* err_flag,
                                   int gemm_precision, float* tape, void* stream) {
  if (num_nodes < 0 || num_edges < 0) return -1;
  const int p = gemm_precision & 0xff;
  if ((gemm_precision & ~(0xff | ENFLOW_EGCL_VARIANTS)) || !(p == ENFLOW_PREC_F32 || p == ENFLOW_PREC_F16X3)) return -1;
  if (nf < 1 || nf > NFMAX) return -4;
  if (!(H == 32 || H == 64 || H == 128)) return -5;
  // 22-bit column field of the pair words; int32 row_ptr with room for a pass past the last edge
  if (num_nodes > (1 << 22) || num_edges > (int64_t)INT32_MAX - 1024) return -3;
  if (!row_ptr || !h || !layer || !Q || !F || !G || !err_flag || (num_edges > 0 && (!col || !coord_diff))) return -1;
#ifdef ENFLOW_LIST_TAPE
  if (!tape) return -1;
#endif
  if (num_nodes == 0) return 0;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ElLayerArgs B{};
  B.row_ptr = row_ptr; B.col = col; B.cdiff = coord_diff; B.h = h; B.layer = layer;
  B.Q = Q; B.F = F; B.G = G; B.err = err_flag;
  B.n = num_nodes; B.num_edges = (int)num_edges; B.nf = nf; B.cw = cw;
#ifdef ENFLOW_LIST_TAPE
  B.tape = tape;
#endif
  const int grid = (num_nodes + 31) / 32;
  if (H == 32) el_layer_prec<32>(gemm_precision, grid, st, B);
  else if (H == 64) el_layer_prec<64>(gemm_precision, grid, st, B);
  else el_layer_prec<128>(gemm_precision, grid, st, B);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
