// enflow_bwd_wgrad.h -- the weight gradients of the training backward:
// outer_acc_kernel, outer_x3_kernel and reduce_part_kernel over the rows that
// lf_layer_bwd_kernel / argmax_bwd_kernel (enflow_bwd_layer.h) wrote.  Included by
// enflow_backward.hip.
#pragma once
#include "enflow_bwd_layer.h"

// ---------------------------------------------------------------------------
// weight gradients: C[m][n] = sum_rows DY[row][m] X[row][n] (+ bias column
// sum_rows DY[row][m]); rows chunked, one partial per chunk, fixed-order reduce
// ---------------------------------------------------------------------------
struct OuterDesc {
  const float* DY;
  const float* X;
  const int32_t* rows_dev;   // device row count (NULL: rows_static)
  float* part;
  float* outW;               // [M][N] row-major (torch Linear weight layout)
  float* outB;               // [M] (bias) or NULL
  int ldd, M, ldx, N, rows_static, mb, nb, nch;
  int tiled;                 // 0 row-major; 1 tile-blocked (trow layout; ldd / ldx = width);
                             // 2 tile-blocked on the F16X3 kernel (outer_x3_kernel);
                             // 3 partials written by another descriptor's pass (part2)
  int xf_x;                  // 1: X = silu(stored)
  const float* xrow;         // tile-blocked: X[row][n] *= xrow[row] after xf_x (or NULL)
  int xf_dy;                 // 1: DY[row][m] = rowv[row] * colv[m] * silu'(stored)
  const float* rowv;
  const float* colv;
  int chunk;                 // rows per workgroup / partial
  float* part2;              // outer_x3_kernel with xf_dy: partials of sum_rows rowv * silu(DY source)
  int recomp;                // outer_x3_kernel operands recomputed instead of read (RECOMP_*)
  const float* Lp;           // RECOMP_*: the layer's packed forward weights
  int nf;                    // RECOMP_X0: node features (xin row layout)
  const float* actp;         // the layer's act_fn (kind, p0, p1; packed layer + vfl + 1), NULL: SiLU
  int f32r;                  // RECOMP_*: recompute on the fp32 MFMA (the ENFLOW_BWD_F32 backward)
  const float* tmaxA;        // outer_x3_kernel: the producer's per-tile max |DY| / max |X| (BwdArgs::tmax
  const float* tmaxB;        //   + TMX_*, stride TMX_W)
};
// RECOMP_X0: X = silu(pre0), pre0 = edge_nn.0 . xin + be1 (the X source is xin, width ldx);
// RECOMP_PC: DY = rowv * silu'(pc), pc = coord_nn.0 . X + bc1 (X read; no DY source), and
//            part2 gets coord_nn.2's sum_rows rowv * silu(pc).
// Both are the layer backward's instruction sequences on the same operands: bitwise its values.
enum { RECOMP_NONE = 0, RECOMP_X0 = 1, RECOMP_PC = 2 };
#define OUTER_MAX 10
struct OuterBatch {
  OuterDesc d[OUTER_MAX];
  int nd;
  int start[OUTER_MAX + 1];   // first workgroup of each descriptor
};
#ifndef OA_CHUNK
#define OA_CHUNK 2048        // pair rows per partial
#endif
#ifndef OA_CHUNK_ATOM
#define OA_CHUNK_ATOM 256    // atom rows per partial (r04z: 256 -1 % of backward vs 512 on the F16X3 atom-row kernel)
#endif
static_assert(OA_CHUNK % 64 == 0 && OA_CHUNK_ATOM % 64 == 0, "partial chunks are whole row stages");

__device__ __forceinline__ int find_desc(const OuterBatch& ob, int bid) {
  int k = 0;
  while (k + 1 < ob.nd && bid >= ob.start[k + 1]) ++k;
  return k;
}

// One workgroup = one chunk of OA_CHUNK rows x a 128-column block of X, the
// whole M (<= 128) of DY.  Rows are staged through LDS 32 at a time (double
// buffered: the next stage's global loads are in flight during this stage's
// MFMAs).  Waves own 64 x 64 quadrants of the 128 x 128 output as four
// v_mfma_f32_32x32x2_f32 accumulators; each k-step (2 rows) reads its A / B
// fragments straight from the row-major LDS image (lanes along m / n:
// conflict-free).  M == 1 (coord_nn.2 / vel_scaling_nn.2) is a plain column
// reduction and runs on VALU.  The bias column (sum of DY) is accumulated by
// the n-block-0 workgroup from the same LDS image.
#define OB_ROWS 32
#define OB_LD 129   // LDS row stride: tile-blocked stages write down the columns
template <bool TILED, bool GEN = false>
__global__ void __launch_bounds__(256, 2) outer_acc_kernel(OuterBatch ob) {
  const int bid = blockIdx.x;
  const int k = find_desc(ob, bid);
  const OuterDesc& D = ob.d[k];
  const int local = bid - ob.start[k];
  const int chunk = local / D.nb, nbi = local - chunk * D.nb;
  const int rows = D.rows_dev ? D.rows_dev[0] : D.rows_static;
  const int r0 = chunk * D.chunk;
  if (r0 >= rows) return;
  const int r1 = min(rows, r0 + D.chunk);
  const int NB = D.N + (D.outB ? 1 : 0);
  const int n0 = nbi * 128;
  const int M = D.M, N = D.N;
  const Act act = GEN && D.actp ? act_of(D.actp) : act_silu();
  __shared__ float sd[2][OB_ROWS][OB_LD];
  __shared__ float sx[2][OB_ROWS][OB_LD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, j = lane & 31, hh = lane >> 5;
  const int mh = w & 1, nh = w >> 1;
  const bool do_bias = D.outB != nullptr && nbi == 0 && tid < M;
  float bsum = 0.f;
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16)0.f;
  float vacc = 0.f;   // M == 1 path: column n0 + tid (tid < 128)
  float rd[16], rx[16];
  const int nst = (r1 - r0 + OB_ROWS - 1) / OB_ROWS;
  constexpr bool tiled = TILED;
  // element q of this thread: (row r, column c) of the 32 x 128 stage; tile-blocked
  // sources are read down the columns (contiguous), row-major ones along the rows
  auto rc = [&](int q, int& r, int& c) {
    const int e = q * 256 + tid;
    if (tiled) { r = e & 31; c = e >> 5; } else { r = e >> 7; c = e & 127; }
  };
  // coord_nn.0's DY = aphi[row] * wc2[m] * silu'(pc): the row factor is applied
  // on load (a thread's 16 elements of a tile-blocked stage share one row), the
  // column factor wc2[m] to the finished sums
  float ra = 0.f, xa = 1.f;
  auto gload = [&](int st) {
    const int rb = r0 + st * OB_ROWS;
    const size_t rt = (size_t)(rb >> 5);
    if (tiled && D.xf_dy) ra = rb + (tid & 31) < r1 ? D.rowv[rb + (tid & 31)] : 0.f;
    if (tiled && D.xrow) xa = rb + (tid & 31) < r1 ? D.xrow[rb + (tid & 31)] : 0.f;
    const float* const dblk = D.DY + ((rt * D.ldd) << 5);            // wave-uniform tile blocks
    const float* const xblk = D.X + ((rt * D.ldx + n0) << 5);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      int r, c;
      rc(q, r, c);
      const int p = rb + r;
      const bool pv = p < r1;
      if (tiled) {
        const unsigned e = (unsigned)(q * 256 + tid);                // = c * 32 + r
        rd[q] = (pv && c < M) ? dblk[e] : 0.f;
        rx[q] = (pv && n0 + c < N) ? xblk[e] : 0.f;
      } else {
        rd[q] = (pv && c < M) ? D.DY[(size_t)p * D.ldd + c] : 0.f;
        rx[q] = (pv && n0 + c < N) ? D.X[(size_t)p * D.ldx + n0 + c] : 0.f;
      }
    }
  };
  auto lstore = [&](int buf) {
    if (tiled && D.xf_dy) {
#pragma unroll
      for (int q = 0; q < 16; ++q) rd[q] = ra * dact_v<GEN>(act, rd[q]);
    }
    if (tiled && D.xf_x) {
#pragma unroll
      for (int q = 0; q < 16; ++q) rx[q] = act_v<GEN>(act, rx[q]);
    }
    if (tiled && D.xrow) {
#pragma unroll
      for (int q = 0; q < 16; ++q) rx[q] *= xa;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      int r, c;
      rc(q, r, c);
      sd[buf][r][c] = rd[q];
      sx[buf][r][c] = rx[q];
    }
  };
  // wave-uniform: skip accumulator tiles that only see zero padding
  const bool use_m1 = mh * 64 + 32 < M, use_n0 = n0 + nh * 64 < N, use_n1 = n0 + nh * 64 + 32 < N;
  const bool live = mh * 64 < M && use_n0;
  gload(0);
  lstore(0);
  __syncthreads();
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    if (st + 1 < nst) gload(st + 1);
    if (M > 1) {
      if (live && !TILED) {
        // atom rows on the F16X3 MFMA (32x32x16, 3 products) instead of 32x32x2 fp32:
        // each lane gathers its operands' 8 rows per k-step from the row-major stage
        // (A: rows 16 ks + 8 hh + e of DY column m, B: the same rows of X column n),
        // a power-of-two scale per stage, wave and operand (max |x| -> [2^12, 2^13))
        // before the hi / lo split, the stage's sums added with the exact inverse scale
        float av[2][2][8], bv[2][2][8];
        float ma = 0.f, mb = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int r = 16 * ks + 8 * hh + e;
              av[a][ks][e] = sd[buf][r][mh * 64 + a * 32 + j];
              bv[a][ks][e] = sx[buf][r][nh * 64 + a * 32 + j];
              if (a == 0 || use_m1) ma = fmaxf(ma, fabsf(av[a][ks][e]));
              if (a == 0 || use_n1) mb = fmaxf(mb, fabsf(bv[a][ks][e]));
            }
        ma = wave_max(ma);
        mb = wave_max(mb);
        const int ea = pow2_exp(ma), eb = pow2_exp(mb);
        const float sa = ldexpf(1.f, ea), sbs = ldexpf(1.f, eb);
        const float un = ldexpf(ldexpf(1.f, -ea), -eb);
        f16x8 ah[2][2], al[2][2], bh[2][2], bl[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            f32x16 xa, xb;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              xa[e] = av[a][ks][e] * sa;
              xb[e] = bv[a][ks][e] * sbs;
            }
            split_f16(xa, 0, ah[a][ks], al[a][ks]);
            split_f16(xb, 0, bh[a][ks], bl[a][ks]);
          }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            if ((a == 1 && !use_m1) || (b == 1 && !use_n1)) continue;
            f32x16 t = (f32x16)0.f;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
              t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[a][ks], bh[b][ks], t, 0, 0, 0);
              t = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[a][ks], bl[b][ks], t, 0, 0, 0);
              t = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[a][ks], bh[b][ks], t, 0, 0, 0);
            }
            acc[a][b] += t * un;
          }
      } else if (live) {
        if (use_m1 && use_n1) {
#pragma unroll 4
          for (int s = 0; s < OB_ROWS / 2; ++s) {
            const int r = 2 * s + hh;
            const float a0 = sd[buf][r][mh * 64 + j], a1 = sd[buf][r][mh * 64 + 32 + j];
            const float b0 = sx[buf][r][nh * 64 + j], b1 = sx[buf][r][nh * 64 + 32 + j];
            acc[0][0] = mfma32(a0, b0, acc[0][0]);
            acc[0][1] = mfma32(a0, b1, acc[0][1]);
            acc[1][0] = mfma32(a1, b0, acc[1][0]);
            acc[1][1] = mfma32(a1, b1, acc[1][1]);
          }
        } else {
#pragma unroll 4
          for (int s = 0; s < OB_ROWS / 2; ++s) {
            const int r = 2 * s + hh;
            const float a0 = sd[buf][r][mh * 64 + j], a1 = sd[buf][r][mh * 64 + 32 + j];
            const float b0 = sx[buf][r][nh * 64 + j], b1 = sx[buf][r][nh * 64 + 32 + j];
            acc[0][0] = mfma32(a0, b0, acc[0][0]);
            if (use_n1) acc[0][1] = mfma32(a0, b1, acc[0][1]);
            if (use_m1) acc[1][0] = mfma32(a1, b0, acc[1][0]);
          }
        }
      }
    } else if (tid < 128) {
#pragma unroll 8
      for (int r = 0; r < OB_ROWS; ++r) vacc = fmaf(sd[buf][r][0], sx[buf][r][tid], vacc);
    }
    if (do_bias) {
#pragma unroll 8
      for (int r = 0; r < OB_ROWS; ++r) bsum += sd[buf][r][tid];
    }
    if (st + 1 < nst) lstore(buf ^ 1);
    __syncthreads();
  }
  float* out = D.part + (size_t)chunk * M * NB;
  const bool colf = tiled && D.xf_dy;
  if (M > 1) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int mm = mh * 64 + a * 32 + rho(r, hh), nn = n0 + nh * 64 + b * 32 + j;
          if (mm < M && nn < N) out[(size_t)mm * NB + nn] = colf ? acc[a][b][r] * D.colv[mm] : acc[a][b][r];
        }
  } else if (tid < 128 && n0 + tid < N) {
    out[n0 + tid] = vacc;
  }
  if (do_bias) out[(size_t)tid * NB + N] = colf ? bsum * D.colv[tid] : bsum;
}

// F16X3 form of outer_acc_kernel for the tile-blocked pair rows (M > 1): the
// stage's DY / X tiles go to LDS column-major ([column][row], rows contiguous),
// so an MFMA operand (8 consecutive rows of one column) is one ds_read_b128
// pair.  Each operand gets one power-of-two scale per chunk (max |x| of the
// chunk -> [2^12, 2^13), as the layer backward's adjoint tiles) before the
// hi / lo split: the chunk maximum is the max over the per-tile maxima the
// layer backward stored (BwdArgs::tmax), so no stage computes a maximum, the
// three products accumulate straight into acc, and the exact inverse scales
// are applied once to the finished sums.  (Per element the split keeps ~22
// bits relative to the chunk maximum; rows far below it lose low bits that
// the sum could not hold anyway.)
//
// Recomputed operands (OuterDesc::recomp) trade HBM bytes for MFMAs: the layer
// backward stores neither pre(edge_nn.0) nor pre(coord_nn.0) (2 x H floats per
// pair row written and read back), wave w rebuilds output tile w (features
// 32 w .. 32 w + 31) of the stage's 32 rows in the forward's "weights = A"
// orientation (lane = row, registers = features) from the packed forward
// fragments, and writes it to the LDS stage.
#define OX_LD 36   // LDS column stride (floats): 16-byte aligned operand reads
#ifndef ENFLOW_OUTER_WPS
#define ENFLOW_OUTER_WPS 2   // outer_x3_kernel occupancy hint (A/B knob)
#endif

// F32R (the ENFLOW_BWD_F32 backward): the recomputed operands come from the
// fp32 MFMA on the forward's fp32 fragments (we1f / wc1f), as that backward's
// own recompute -- an f16x3 split of operands that are entirely small would
// lose the accuracy the fp32 re-run was made for.
template <int H, int RCM, bool GEN = false, bool F32R = false>
__device__ __forceinline__ void outer_x3_body(const OuterDesc& D, int chunk, int nbi, int r0, int r1,
                                              float (*sd)[128][OX_LD], float (*sx)[128][OX_LD]) {
  constexpr int NT = H / 32;
  const int NB = D.N + (D.outB ? 1 : 0);
  const int n0 = nbi * 128;
  const int M = D.M, N = D.N;
  const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const int mh = w & 1, nh = w >> 1;
  constexpr int rcm = RCM;
  const bool do_bias = D.outB != nullptr && nbi == 0 && tid < M;
  const bool xf_dy = D.xf_dy != 0, xf_x = D.xf_x != 0;
  const bool fold = xf_dy && D.part2 != nullptr && nbi == 0;   // coord_nn.2's gradient rides along
  const Act act = GEN && D.actp ? act_of(D.actp) : act_silu();
  // recompute: the layer's packed forward weights
  const int nf = rcm ? D.nf : 1;
  const EgclLayout L = egcl_layout(H, nf);
  const rsrc_t W = weights_rsrc(rcm ? D.Lp : nullptr, rcm ? L.total : 0);
  float wacc[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) wacc[q] = 0.f;
  float bsum = 0.f;
  // edge_nn.0's fragments of output tile w (hi / lo per k-step): loop invariant,
  // loaded once per workgroup and kept in registers (RECOMP_X0)
  // (the first k-step's; nf = 8's second k-step is read when used)
  f32x4 wfh = (f32x4)0.f, wfl = (f32x4)0.f;
  if constexpr (rcm == RECOMP_X0 && !F32R) {
    if (w < NT) {
      wfh = bload4(W, lane * 32, (L.we1x + (w * KS0MAX) * 512) * 4);
      wfl = bload4(W, lane * 32 + 16, (L.we1x + (w * KS0MAX) * 512) * 4);
    }
  }
  f32x16 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (f32x16)0.f;
  // staged rows in registers, one stage ahead
  // a thread stages 4 consecutive rows of a column per 16-B load /
  // ds_write_b128 (float4 e4 = q * 256 + tid: column e4 / 8, rows 4 (e4 % 8) ..),
  // 4x fewer memory instructions than one dword per row; ra4 / xa4 the 4 rows'
  // factors, raj row j's (the recompute's lane row)
  struct Stage { float rd[16], rx[16]; bool pv; f32x4 ra4, xa4; float raj; const float* xb; float rad; };
  Stage S0;
  const int nst = (r1 - r0 + OB_ROWS - 1) / OB_ROWS;
  auto gload = [&](int st, Stage& G) {
    const int rb = r0 + st * OB_ROWS;
    const size_t rt = (size_t)(rb >> 5);
    const float* const dblk = D.DY + ((rt * D.ldd) << 5);
    const float* const xblk = D.X + ((rt * D.ldx + n0) << 5);
    const bool pv = rb + (tid & 31) < r1;
    G.pv = pv;
    G.xb = xblk;
    if (rcm == RECOMP_PC) G.raj = pv ? D.rowv[rb + j] : 0.f;
    if constexpr (rcm != RECOMP_X0) {
      // stage rows are whole 32-row tiles (pair rows are 32-aligned), so a float4
      // of rows is valid or not as a whole
      const int r4 = (tid & 7) * 4;
      const bool pv4 = rb + r4 + 3 < r1;
      G.ra4 = (f32x4)0.f;
      G.xa4 = (f32x4)1.f;
      if (xf_dy) G.ra4 = pv4 ? ld4(D.rowv + rb + r4) : (f32x4)0.f;
      if (D.xrow) G.xa4 = pv4 ? ld4(D.xrow + rb + r4) : (f32x4)0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e4 = q * 256 + tid, c = e4 >> 3;
        f32x4 d = (f32x4)0.f, x = (f32x4)0.f;
        if (rcm != RECOMP_PC && pv4 && c < M) d = ld4(dblk + 4 * e4);
        if (pv4 && n0 + c < N) x = ld4(xblk + 4 * e4);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          G.rd[4 * q + u] = d[u];
          G.rx[4 * q + u] = x[u];
        }
      }
    } else {   // RECOMP_X0: DY as float4 rows, then the X operand (xin)
      const int r4 = (tid & 7) * 4;
      const bool pv4 = rb + r4 + 3 < r1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e4 = q * 256 + tid, c = e4 >> 3;
        const f32x4 d = (pv4 && c < M) ? ld4(dblk + 4 * e4) : (f32x4)0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) G.rd[4 * q + u] = d[u];
      }
      // (F32R: the fp32 GEMM0 reads its operands from the xin rows in lstore, G.xb)
      if constexpr (!F32R) {
        // GEMM0's B operand of lane (row j, half hh), as the layer backward builds it
        // (k order gemm0_col): rx[8 ks + u] = k-slice ks, half 0 = h_i's features
        // 8 ks + u, half 1 = h_j's (+ radial in slot 7 of the last slice when that is
        // padding); nf = 8: rx[8] = radial (the second k-slice)
        if constexpr (NFMAX == 8) {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            const int q = hh ? nf + u : u;
            G.rx[u] = (pv && u < nf) ? xblk[q * 32 + j] : 0.f;
          }
          if (hh && nf <= 7) G.rx[7] = pv ? xblk[(2 * nf) * 32 + j] : 0.f;
          G.rx[8] = pv ? xblk[(2 * nf) * 32 + j] : 0.f;
        } else {   // features in two k-slices; nf 8 / 16: the radial in a slice of its own
          const int nch = gemm0_nch(nf);
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const int f = u, q = hh ? nf + f : f;
            G.rx[u] = (pv && f < nf && u < 8 * nch) ? xblk[q * 32 + j] : 0.f;
          }
          const float rad = pv ? xblk[(2 * nf) * 32 + j] : 0.f;
          G.rad = 0.f;
          if (gemm0_radial_slot7(nf)) {
            if (hh) {   // slot 8 nch - 1 (nch 1 / 2), by compile-time index: a runtime one puts Stage in scratch
#pragma unroll
              for (int u = 7; u < 16; u += 8)
                if (u == 8 * nch - 1) G.rx[u] = rad;
            }
          } else if (hh == 0) {
            if (nch == 1) G.rx[8] = rad;   // nf == 8: the radial's own (second) slice
            else G.rad = rad;              // nf == 16: the third slice
          }
        }
      }
    }
  };
  auto lstore = [&](int buf, Stage& G) {
    if constexpr (rcm != RECOMP_X0) {
      const int r4 = (tid & 7) * 4;
      if constexpr (rcm != RECOMP_PC) {
        if (xf_dy) {   // DY = aphi * silu'(pc) (wc2 applied at the end); d wc2 += aphi * silu(pc)
#pragma unroll
          for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
              const float z = G.rd[4 * q + u];
              float fz, dz;
              act_fd<GEN>(act, z, fz, dz);
              if (fold) wacc[q] = fmaf(G.ra4[u], fz, wacc[q]);
              G.rd[4 * q + u] = G.ra4[u] * dz;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
          st4(&sd[buf][(q * 256 + tid) >> 3][r4],
              (f32x4){G.rd[4 * q], G.rd[4 * q + 1], G.rd[4 * q + 2], G.rd[4 * q + 3]});
      }
      if (xf_x) {
#pragma unroll
        for (int q = 0; q < 16; ++q) G.rx[q] = act_v<GEN>(act, G.rx[q]);
      }
      if (D.xrow) {
#pragma unroll
        for (int q = 0; q < 16; ++q) G.rx[q] *= G.xa4[q & 3];
      }
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st4(&sx[buf][(q * 256 + tid) >> 3][r4], (f32x4){G.rx[4 * q], G.rx[4 * q + 1], G.rx[4 * q + 2], G.rx[4 * q + 3]});
    } else {   // RECOMP_X0: DY rows as float4 (no transform on edge_nn.2's DY)
      const int r4 = (tid & 7) * 4;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st4(&sd[buf][(q * 256 + tid) >> 3][r4],
            (f32x4){G.rd[4 * q], G.rd[4 * q + 1], G.rd[4 * q + 2], G.rd[4 * q + 3]});
      if constexpr (F32R) {
        if (w < NT) {   // output tile w of pre0 -> act -> X, fp32 MFMA (the forward's f32 GEMM0 k order)
          f32x16 x = (f32x16)0.f;
#pragma unroll
          for (int s = 0; s < NFMAX + 1; ++s) {
            int col = -1;
            if (s < NFMAX / 2) {
              const int f = 2 * s + hh;
              if (f < nf) col = f;
            } else if (s < NFMAX) {
              const int f = 2 * (s - NFMAX / 2) + hh;
              if (f < nf) col = nf + f;
            } else if (hh == 0) {
              col = 2 * nf;
            }
            const float b = (G.pv && col >= 0) ? G.xb[col * 32 + j] : 0.f;
            x = mfma32(bload(W, lane * 4, (L.we1f + (w * (NFMAX + 1) + s) * 64) * 4), b, x);
          }
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int f0 = 32 * w + 8 * g4 + 4 * hh;
            const f32x4 b = ld4(D.Lp + L.be1 + f0);
#pragma unroll
            for (int u = 0; u < 4; ++u) sx[buf][f0 + u][j] = G.pv ? act_v<GEN>(act, x[4 * g4 + u] + b[u]) : 0.f;
          }
        }
      } else {
        if (w < NT) {   // output tile w of pre0 -> silu -> X
          const int ks_n = gemm0_ksteps(nf);
          f32x16 x = (f32x16)0.f;
          for (int ks = 0; ks < ks_n; ++ks) {
            f32x16 in;
            if constexpr (NFMAX == 8) {
#pragma unroll
              for (int u = 0; u < 8; ++u) in[u] = ks == 0 ? G.rx[u] : 0.f;
              if (ks == 1 && hh == 0) in[0] = G.rx[8];
            } else {
#pragma unroll
              for (int u = 0; u < 8; ++u) in[u] = ks == 0 ? G.rx[u] : (ks == 1 ? G.rx[8 + u] : 0.f);
              if (ks == 2) in[0] = G.rad;   // nf 16's radial slice (0 on lane half 1)
            }
            f16x8 bh, bl;
            split_f16(in, 0, bh, bl);
            f32x4 ah = wfh, al = wfl;
            if (ks >= 1) {
              ah = bload4(W, lane * 32, (L.we1x + (w * KS0MAX + ks) * 512) * 4);
              al = bload4(W, lane * 32 + 16, (L.we1x + (w * KS0MAX + ks) * 512) * 4);
            }
            x = mfma_f16(ah, bh, x);
            x = mfma_f16(ah, bl, x);
            x = mfma_f16(al, bh, x);
          }
          x *= D.Lp[L.scl + 5];
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const int f0 = 32 * w + 8 * g4 + 4 * hh;
            const f32x4 b = ld4(D.Lp + L.be1 + f0);
#pragma unroll
            for (int u = 0; u < 4; ++u) sx[buf][f0 + u][j] = G.pv ? act_v<GEN>(act, x[4 * g4 + u] + b[u]) : 0.f;
          }
        }
      }
    }
  };
  // RECOMP_PC, after the stage's X is in LDS: pc = coord_nn.0 . X + bc1 (output
  // tile w), DY = aphi * silu'(pc) into LDS, d wc2 partial += aphi * silu(pc)
  float (&wacc2)[16] = wacc;   // RECOMP_PC's d wc2 partials (lane = row, registers = features)
  auto recomp_pc = [&](int buf, const Stage& G) {
    if (F32R && w < NT) {   // fp32 chain of output tile w on wc1f (the forward's f32 k order)
      f32x16 cacc = (f32x16)0.f;
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        f32x16 X;
#pragma unroll
        for (int r = 0; r < 16; ++r) X[r] = sx[buf][32 * t + rho(r, hh)][j];
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const f32x4 a4 = bload4(W, lane * 16, (L.wc1f + ((w * NT + t) * 4 + rg) * 256) * 4);
#pragma unroll
          for (int u = 0; u < 4; ++u) cacc = mfma32(a4[u], X[4 * rg + u], cacc);
        }
      }
      const float ra = G.raj;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int f0 = 32 * w + 8 * g4 + 4 * hh;
        const f32x4 b = ld4(D.Lp + L.bc1 + f0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float z = cacc[4 * g4 + u] + b[u];
          float fz, dz;
          act_fd<GEN>(act, z, fz, dz);
          wacc2[4 * g4 + u] = fmaf(ra, fz, wacc2[4 * g4 + u]);
          sd[buf][f0 + u][j] = ra * dz;
        }
      }
    } else if (w < NT) {
      // coord_nn.0's fragments of output tile w, requested half a chain at a time
      // (two L2 round trips per stage; resident they would cost 64 VGPRs across
      // the stage)
      constexpr int HALF = NT > 1 ? NT : 2;   // k-steps per request group
      f32x16 cacc = (f32x16)0.f;
#pragma unroll
      for (int g = 0; g < 2 * NT; g += HALF) {
        f32x4 ch[HALF], cl[HALF];
#pragma unroll
        for (int q = 0; q < HALF; ++q) {
          const int ts = g + q;
          const int so = (L.wc1x + ((w * NT + (ts >> 1)) * 2 + (ts & 1)) * 512) * 4;
          ch[q] = bload4(W, lane * 32, so);
          cl[q] = bload4(W, lane * 32 + 16, so);
        }
        // chain_x3_fill's per-tile order: k-steps ascending, hi.hi, hi.lo, lo.hi
#pragma unroll
        for (int q = 0; q < HALF; q += 2) {
          const int t = (g + q) >> 1;
          f32x16 X;   // input tile t in the accumulator layout (lane = row, registers = features)
#pragma unroll
          for (int r = 0; r < 16; ++r) X[r] = sx[buf][32 * t + rho(r, hh)][j];
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            f16x8 bh, bl;
            split_f16(X, s2, bh, bl);
            cacc = mfma_f16(ch[q + s2], bh, cacc);
            cacc = mfma_f16(ch[q + s2], bl, cacc);
            cacc = mfma_f16(cl[q + s2], bh, cacc);
          }
        }
      }
      const float inv2 = D.Lp[L.scl + 3];
      const float ra = G.raj;   // row j's aphi
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int f0 = 32 * w + 8 * g4 + 4 * hh;
        const f32x4 b = ld4(D.Lp + L.bc1 + f0);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float z = fmaf(cacc[4 * g4 + u], inv2, b[u]);
          float fz, dz;
          act_fd<GEN>(act, z, fz, dz);
          wacc2[4 * g4 + u] = fmaf(ra, fz, wacc2[4 * g4 + u]);
          sd[buf][f0 + u][j] = ra * dz;
        }
      }
    }
  };
  const bool use_m1 = mh * 64 + 32 < M, use_n0 = n0 + nh * 64 < N, use_n1 = n0 + nh * 64 + 32 < N;
  const bool live = mh * 64 < M && use_n0;
  // the chunk's scales (one per operand, from the producer's per-tile maxima):
  // max |x| of the chunk -> [2^12, 2^13) before the hi / lo split, so the three
  // products accumulate straight into acc and are un-scaled once at the end
  static_assert(OA_CHUNK <= 64 * 32, "a chunk's tile maxima fit one wave");
  int ea = 0, eb = 0;
  {
    const int t0 = r0 >> 5, ntl = (r1 - r0 + 31) >> 5;
    const float ma = lane < ntl ? D.tmaxA[(size_t)(t0 + lane) * TMX_W] : 0.f;
    const float mb = lane < ntl ? D.tmaxB[(size_t)(t0 + lane) * TMX_W] : 0.f;
    ea = pow2_exp(wave_max(ma));
    eb = pow2_exp(wave_max(mb));
  }
  const float sa = ldexpf(1.f, ea), sbs = ldexpf(1.f, eb);
  auto compute = [&](int buf) {
    if (live) {
      // operands of both k-steps: A[a][ks] (DY columns), B[b][ks] (X columns)
      f32x4 av[2][2][2], bv[2][2][2];   // [tile][ks][half]
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            av[a][ks][h2] = *reinterpret_cast<const f32x4*>(&sd[buf][mh * 64 + a * 32 + j][16 * ks + 8 * hh + 4 * h2]);
            bv[a][ks][h2] = *reinterpret_cast<const f32x4*>(&sx[buf][nh * 64 + a * 32 + j][16 * ks + 8 * hh + 4 * h2]);
          }
      f16x8 ah[2][2], al[2][2], bh[2][2], bl[2][2];
      // scaled hi / lo split: hi = f16(x s) by v_cvt_pk_f16_f32, lo = f16(x s - hi) by
      // v_fma_mix (split_f16; x s - hi is exact in fp32, so bitwise the plain form)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          f32x16 xa, xb;
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            xa[jj] = av[a][ks][jj >> 2][jj & 3] * sa;
            xb[jj] = bv[a][ks][jj >> 2][jj & 3] * sbs;
          }
          split_f16(xa, 0, ah[a][ks], al[a][ks]);
          split_f16(xb, 0, bh[a][ks], bl[a][ks]);
        }
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          if ((a == 1 && !use_m1) || (b == 1 && !use_n1)) continue;
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[a][ks], bh[b][ks], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[a][ks], bl[b][ks], acc[a][b], 0, 0, 0);
            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[a][ks], bh[b][ks], acc[a][b], 0, 0, 0);
          }
        }
    }
    if (do_bias) {
#pragma unroll 8
      for (int r = 0; r < OB_ROWS; ++r) bsum += sd[buf][tid][r];
    }
  };
  gload(0, S0);
  lstore(0, S0);
  __syncthreads();
  if constexpr (rcm == RECOMP_PC) {
    recomp_pc(0, S0);
    __syncthreads();
  }
  for (int st = 0; st < nst; ++st) {
    const int buf = st & 1;
    if (st + 1 < nst) gload(st + 1, S0);
    compute(buf);
    if (st + 1 < nst) lstore(buf ^ 1, S0);
    __syncthreads();
    if (rcm == RECOMP_PC && st + 1 < nst) {
      recomp_pc(buf ^ 1, S0);
      __syncthreads();
    }
  }
  float* out = D.part + (size_t)chunk * M * NB;
  const float ua = ldexpf(1.f, -ea), ub = ldexpf(1.f, -eb);   // exact inverse scales
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mm = mh * 64 + a * 32 + rho(r, hh), nn = n0 + nh * 64 + b * 32 + j;
        const float v = acc[a][b][r] * ua * ub;
        if (mm < M && nn < N) out[(size_t)mm * NB + nn] = xf_dy ? v * D.colv[mm] : v;
      }
  if (do_bias) out[(size_t)tid * NB + N] = xf_dy ? bsum * D.colv[tid] : bsum;
  if (fold && rcm == RECOMP_PC) {   // fixed-order sum over the 32 rows of each half-wave
    if (w < NT) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = wacc2[r];
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if (j == 0) D.part2[(size_t)chunk * M + 32 * w + rho(r, hh)] = v;
      }
    }
  } else if (fold) {   // fixed-order sum over the 8 row groups of each column
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float v = wacc[q];
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) v += __shfl_xor(v, off, 64);
      const int c = (q * 256 + tid) >> 3;
      if ((tid & 7) == 0 && c < M) D.part2[(size_t)chunk * M + c] = v;
    }
  }
}

template <bool GEN = false, bool F32R = false>
__global__ void __launch_bounds__(256, ENFLOW_OUTER_WPS) outer_x3_kernel(OuterBatch ob) {
  const int bid = blockIdx.x;
  const int k = find_desc(ob, bid);
  const OuterDesc& D = ob.d[k];
  const int local = bid - ob.start[k];
  const int chunk = local / D.nb, nbi = local - chunk * D.nb;
  const int rows = D.rows_dev ? D.rows_dev[0] : D.rows_static;
  const int r0 = chunk * D.chunk;
  if (r0 >= rows) return;
  const int r1 = min(rows, r0 + D.chunk);
  __shared__ float sd[2][128][OX_LD];
  __shared__ float sx[2][128][OX_LD];
  // recomputed operands need the layer's hidden width at compile time
  // (one register allocation per branch: the modes' staged operands differ)
  if (D.recomp == RECOMP_X0) {
    if (D.N == 128) outer_x3_body<128, RECOMP_X0, GEN, F32R>(D, chunk, nbi, r0, r1, sd, sx);
    else if (D.N == 64) outer_x3_body<64, RECOMP_X0, GEN, F32R>(D, chunk, nbi, r0, r1, sd, sx);
    else outer_x3_body<32, RECOMP_X0, GEN, F32R>(D, chunk, nbi, r0, r1, sd, sx);
  } else if (D.recomp == RECOMP_PC) {
    if (D.N == 128) outer_x3_body<128, RECOMP_PC, GEN, F32R>(D, chunk, nbi, r0, r1, sd, sx);
    else if (D.N == 64) outer_x3_body<64, RECOMP_PC, GEN, F32R>(D, chunk, nbi, r0, r1, sd, sx);
    else outer_x3_body<32, RECOMP_PC, GEN, F32R>(D, chunk, nbi, r0, r1, sd, sx);
  } else {
    outer_x3_body<128, RECOMP_NONE, GEN>(D, chunk, nbi, r0, r1, sd, sx);
  }
}

// Four fp64 sums per output (chunk mod 4, the leftover chunks into the first),
// one per thread of a 4-lane group, combined in the fixed order (s0 + s1) +
// (s2 + s3): 64 outputs per workgroup, so the partials stream through 4x as
// many workgroups with a quarter of the serial loads each
#define RP_OUT 64
__global__ void __launch_bounds__(256) reduce_part_kernel(OuterBatch ob) {
  const int bid = blockIdx.x;
  const int k = find_desc(ob, bid);
  const OuterDesc& D = ob.d[k];
  const int rows = D.rows_dev ? D.rows_dev[0] : D.rows_static;
  const int nch = (rows + D.chunk - 1) / D.chunk;
  const int NB = D.N + (D.outB ? 1 : 0);
  const int sub = threadIdx.x & 3;
  const int idx = (bid - ob.start[k]) * RP_OUT + (threadIdx.x >> 2);
  const bool live = idx < D.M * NB;   // (the whole 4-lane group agrees)
  const size_t cs = (size_t)D.M * NB;
  const float* src = D.part + (live ? idx : 0);
  double s = 0.0;
  const int G = nch >> 2;
  if (live) {
    // eight chunk groups per step into independent sums (eight loads in flight
    // per lane; the partials are read once: non-temporal), combined in a fixed
    // order: deterministic
    constexpr int U = 8;
    double su[U];
#pragma unroll
    for (int u = 0; u < U; ++u) su[u] = 0.0;
    int g = 0;
    for (; g + U <= G; g += U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) v[u] = __builtin_nontemporal_load(&src[(size_t)(4 * (g + u) + sub) * cs]);
#pragma unroll
      for (int u = 0; u < U; ++u) su[u] += (double)v[u];
    }
    for (; g < G; ++g) su[0] += (double)__builtin_nontemporal_load(&src[(size_t)(4 * g + sub) * cs]);
    s = ((su[0] + su[1]) + (su[2] + su[3])) + ((su[4] + su[5]) + (su[6] + su[7]));
    if (sub == 0)
      for (int ch = 4 * G; ch < nch; ++ch) s += (double)src[(size_t)ch * cs];
  }
  const double pair = s + __shfl_xor(s, 1, 64);      // lane 0: s0 + s1, lane 2: s2 + s3
  const double tot = pair + __shfl_xor(pair, 2, 64);  // lane 0: (s0 + s1) + (s2 + s3)
  if (!live || sub != 0) return;
  const int mm = idx / NB, nn = idx - mm * NB;
  if (nn < D.N) D.outW[(size_t)mm * D.N + nn] = (float)tot;
  else D.outB[mm] = (float)tot;
}
