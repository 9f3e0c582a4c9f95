// enflow_wide.h -- the 256-wide EGCL layer of the large-system path
// (enflow_wide.hip): packed layout and the launchers enflow_large.hip
// dispatches hidden width 256 to.
#ifndef ENFLOW_WIDE_H
#define ENFLOW_WIDE_H
#include "enflow_large.h"

#define ENFLOW_WIDE_H256 256

// Packed 256-wide layer (floats): every matrix row-major [out][k] with k padded
// to a multiple of 16 (rows 16-B aligned: one float4 holds a lane's k-slots of
// four fp32 MFMAs, one 16-B load its eight fp16 k-slots), vectors after them.
//   0 we1  [256][WIDE_K0]   edge_nn.0: k = h_i (NFMAX) | h_j (NFMAX) | radial | 0..
//   1 we2  [256][256]       edge_nn.2
//   2 wc1  [256][256]       coord_nn.0
//   3 wn1  [256][WIDE_KN]   node_nn.0: k = message sums (256) | h (NFMAX) | 0..
//   4 wv1  [256][WIDE_KV]   vel_scaling_nn.0: k = h (NFMAX) | 0..
//   5 wn2  [32][256]        node_nn.2 (rows past node_nf zero)
//   be1 be2 bc1 wc2 bn1 bv1 wv2 watt [256] each, bn2 [32]
//   misc [8]   bv2, att bias, EGCL_* flags, act kind, p0, p1, 0, 0
//   scl  [16]  egcl_scales_block's (2^s, 2^-s) of We2, Wc1, We1, Wv1, Wn1, Wn2
//   x3         the six matrices again at the same relative offsets, F16X3: each
//              section holds the scaled weights' fp16 hi parts [out][k], then
//              their lo parts [out][k]
struct WideLayout { int we1, we2, wc1, wn1, wv1, wn2, be1, be2, bc1, wc2, bn1, bv1, wv2, watt, bn2, misc, scl, x3, total; };
constexpr int WIDE_K0 = (2 * NFMAX + 1 + 15) & ~15;
constexpr int WIDE_KV = 16;
constexpr int WIDE_KN = ENFLOW_WIDE_H256 + 16;
struct WideMat { int off, rows, K, scl; };   // section, shape, index of its scale pair in scl
__host__ __device__ inline WideLayout wide_layout() {
  constexpr int H = ENFLOW_WIDE_H256;
  WideLayout L;
  int o = 0;
  L.we1 = o; o += H * WIDE_K0;
  L.we2 = o; o += H * H;
  L.wc1 = o; o += H * H;
  L.wn1 = o; o += H * WIDE_KN;
  L.wv1 = o; o += H * WIDE_KV;
  L.wn2 = o; o += 32 * H;
  L.be1 = o; o += H;
  L.be2 = o; o += H;
  L.bc1 = o; o += H;
  L.wc2 = o; o += H;
  L.bn1 = o; o += H;
  L.bv1 = o; o += H;
  L.wv2 = o; o += H;
  L.watt = o; o += H;
  L.bn2 = o; o += 32;
  L.misc = o; o += 8;
  L.scl = o; o += 16;
  o = (o + 63) & ~63;
  L.x3 = o; o += L.be1;   // the matrix sections again
  o = (o + 63) & ~63;
  L.total = o;
  return L;
}
__host__ __device__ inline WideMat wide_mat(const WideLayout& L, int m) {
  constexpr int H = ENFLOW_WIDE_H256;
  switch (m) {
    case 0: return WideMat{L.we1, H, WIDE_K0, 2};
    case 1: return WideMat{L.we2, H, H, 0};
    case 2: return WideMat{L.wc1, H, H, 1};
    case 3: return WideMat{L.wn1, H, WIDE_KN, 4};
    case 4: return WideMat{L.wv1, H, WIDE_KV, 3};
    default: return WideMat{L.wn2, 32, H, 5};
  }
}

// packed floats of one layer at a width the large-system entries take
static inline size_t lg_layer_stride(int H, int nf) {
  return H == ENFLOW_WIDE_H256 ? (size_t)wide_layout().total : (size_t)egcl_layout(H, nf).total;
}

// one 256-wide layer over the row blocks (lg_layer_kernel's modes); prec: ENFLOW_PREC_F32, or
// ENFLOW_PREC_F16X3 (ENFLOW_PREC_BF16 runs F16X3: the caller warns)
void lg_wide_layer(int prec, int grid, hipStream_t st, const LgArgs& B, int mode);
// the forward's dequantiser at width 256 (lg_dequant_kernel's contract)
void lg_wide_dequant(int grid, hipStream_t st, const LgArgs& B, int kind, const float* dq, const float* noise,
                     float scale);

#endif
