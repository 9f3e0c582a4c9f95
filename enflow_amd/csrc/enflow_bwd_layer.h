// enflow_bwd_layer.h -- the layer backward of the training backward: the packing of
// the backward weight section, BwdArgs, the LDS image and device helpers,
// lf_layer_bwd_kernel, argmax_bwd_kernel and the instance selection that launches
// them.  Included by enflow_backward.hip and enflow_backward_ldja.hip; each
// instantiates its own kernels through layer_bwd_launch / argmax_bwd_launch.
#pragma once
#include "enflow_large.h"
#include "enflow_host.h"

// The one place the two translation units differ.  enflow_backward_ldja.hip defines
// the macro tested here before it includes this header: the same lf_layer_bwd_kernel /
// argmax_bwd_kernel source then compiles under the names lf_layer_bwd_ldja_kernel /
// argmax_bwd_ldja_kernel with LDJA = true (ENFLOW_BWD_LDJ_ATOMS: adj_ldj holds one
// value per atom, the molecule's repeated).  A translation unit of its own, so that
// enflow_backward.hip's instances stay the code they were (profiles/forward_grad/);
// file-scope names, not a template parameter, so that every instance keeps its name.
#ifdef ENFLOW_BWD_LDJA_TU
#define lf_layer_bwd_kernel lf_layer_bwd_ldja_kernel
#define argmax_bwd_kernel argmax_bwd_ldja_kernel
constexpr bool LDJA = true;
#else
constexpr bool LDJA = false;
#endif

// ---------------------------------------------------------------------------
// packing of the backward weight section
// ---------------------------------------------------------------------------
__device__ __forceinline__ void pack_egcl_bwd_body(const float* __restrict__ raw, int H, int nf, float* __restrict__ out) {
  const EgclBwdLayout L = egcl_bwd_layout(H);
  const RawEgcl R = raw_egcl(H, nf);
  const int NT = H / 32;
  const int K1 = 2 * nf + 1;
  for (int idx = blockIdx.x * blockDim.x + threadIdx.x; idx < L.total; idx += gridDim.x * blockDim.x) {
    float v = 0.f;
    if (idx < L.we1T) {                     // W^T chain fragments: A[row][col] = W[col][row]
      const bool c1 = idx >= L.wc1T;
      const int e = idx - (c1 ? L.wc1T : L.we2T);
      const int u = e & 3, lane = (e >> 2) & 63, rg = (e >> 8) & 3, rest = e >> 10;
      const int t = rest % NT, tp = rest / NT;
      const int row = 32 * tp + (lane & 31), col = 32 * t + rho(4 * rg + u, lane >> 5);
      v = raw[(c1 ? R.Wc1 : R.We2) + col * H + row];
    } else if (idx < L.wv1T) {              // we1T[tp][rg][lane][4]: A[q][k] = We1[k][q]
      const int e = idx - L.we1T;
      const int u = e & 3, lane = (e >> 2) & 63, rg = (e >> 8) & 3, tp = e >> 10;
      const int q = lane & 31, k = 32 * tp + rho(4 * rg + u, lane >> 5);
      if (q < K1) v = raw[R.We1 + k * K1 + q];
    } else if (idx >= L.scl && idx < L.scl + 16) {
      continue;                             // written by egcl_bwd_scale_kernel
    } else if (idx >= L.we2Tx && idx < L.we1Tx) {   // F16X3 W^T chain fragments [tp][t][s][lane][hi|lo]
      const bool c1 = idx >= L.wc1Tx;
      const int e = idx - (c1 ? L.wc1Tx : L.we2Tx);
      const int d = e & 7, lane = (e >> 3) & 63, rest = e >> 9;
      const int sstep = rest & 1, t = (rest >> 1) % NT, tp = (rest >> 1) / NT;
      const float sc = out[L.scl + (c1 ? 2 : 0)];
      const int row = 32 * tp + (lane & 31);
      const int j0 = 2 * (d & 3);
      const int col0 = 32 * t + rho(8 * sstep + j0, lane >> 5), col1 = 32 * t + rho(8 * sstep + j0 + 1, lane >> 5);
      const int Wo = c1 ? R.Wc1 : R.We2;
      v = __builtin_bit_cast(float, f16_split_bits(raw[Wo + col0 * H + row] * sc, raw[Wo + col1 * H + row] * sc, d >= 4));
    } else if (idx >= L.we1Tx && idx < L.we1Tx + NT * 2 * 512) {   // F16X3 edge_nn.0^T [tp][s][lane][hi|lo]
      const int e = idx - L.we1Tx;
      const int d = e & 7, lane = (e >> 3) & 63, blk = e >> 9;
      const int tp = blk >> 1, s2 = blk & 1;
      const float sc = out[L.scl + 4];
      const int q = lane & 31, j0 = 2 * (d & 3);
      const int k0 = 32 * tp + rho(8 * s2 + j0, lane >> 5), k1 = 32 * tp + rho(8 * s2 + j0 + 1, lane >> 5);
      const float w0 = q < K1 ? raw[R.We1 + k0 * K1 + q] * sc : 0.f;
      const float w1 = q < K1 ? raw[R.We1 + k1 * K1 + q] * sc : 0.f;
      v = __builtin_bit_cast(float, f16_split_bits(w0, w1, d >= 4));
    } else if (idx >= L.wn2Tx && idx < L.wn1aTx + NT * (H / 16) * 512) {   // F16X3 node-backward fragments
      int e, sidx;
      if (idx < L.wvTx) { e = idx - L.wn2Tx; sidx = 0; }
      else if (idx < L.wnhTx) { e = idx - L.wvTx; sidx = 1; }
      else if (idx < L.wn1aTx) { e = idx - L.wnhTx; sidx = 2; }
      else { e = idx - L.wn1aTx; sidx = 3; }
      const int d = e & 7, lane = (e >> 3) & 63, blk = e >> 9;
      const int m = lane & 31, kh = lane >> 5;
      const float sc = out[L.scl + (sidx == 0 ? 10 : (sidx == 1 ? 6 : 8))];
      float w2[2];
      for (int q = 0; q < 2; ++q) {
        const int jj = 2 * (d & 3) + q;
        float w = 0.f;
        if (sidx == 0) {                 // blk = tp; k index = aG feature
          const int f = 8 * kh + jj;
          if (f < nf) w = raw[R.Wn2 + f * H + 32 * blk + m];
        } else if (sidx < 3) {           // blk = tp * 2 + s; rows f < nf
          const int tp = blk >> 1, s2 = blk & 1;
          const int k = 32 * tp + rho(8 * s2 + jj, kh);
          if (m < nf) w = sidx == 1 ? raw[R.Wv1 + k * nf + m] : raw[R.Wn1 + k * (H + nf) + m];
        } else {                         // blk = tp * (H / 16) + ks
          const int tp = blk / (H / 16), ks = blk % (H / 16);
          const int k = 16 * ks + 8 * kh + jj;
          w = raw[R.Wn1 + k * (H + nf) + nf + 32 * tp + m];
        }
        w2[q] = w * sc;
      }
      v = __builtin_bit_cast(float, f16_split_bits(w2[0], w2[1], d >= 4));
    } else if (idx < L.wn1T) {              // wv1T[f][k]
      const int e = idx - L.wv1T, f = e / H, k = e % H;
      if (f < nf) v = raw[R.Wv1 + k * nf + f];
    } else if (idx < L.scl) {               // wn1T[f][k]
      const int e = idx - L.wn1T, f = e / H, k = e % H;
      if (f < NFMAX) {
        if (f < nf) v = raw[R.Wn1 + k * (H + nf) + f];
      } else if (f - NFMAX < H) {
        v = raw[R.Wn1 + k * (H + nf) + nf + (f - NFMAX)];
      }
    }
    out[idx] = v;
  }
}

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float dsilu_f(float z) {   // d silu / dz
  const float s = sigmoid_f(z);
  return s * (1.f + z * (1.f - s));
}
// act'(z): the SiLU form above unless a generic (GEN) instance runs another act_fn
template <bool GEN>
__device__ __forceinline__ float dact_v(const Act& A, float z) {
  if (!GEN || A.k == ACT_SILU) return dsilu_f(z);
  return act_d(A, z);
}

// ---------------------------------------------------------------------------
// per-layer backward
// ---------------------------------------------------------------------------
struct BwdArgs {
  const int32_t* mol_ptr;
  const float* r_cut;
  const float* box;
  const float* tape;
  int num_atoms, num_mols, n_layers, layer, nf;
  const float* Lp;   // packed forward layer
  const float* Bp;   // packed backward section
  const float* Rp;   // raw (torch-layout) layer parameters
  float dt, cw;
  const float* adj_ldj;
  float* ah;         // [A][nf]  adjoints of h / g / pos / vel: layer output in, layer input out
  float* ag;
  float* apos;       // [A][3]
  float* avel;
  const int32_t* pair_off;   // this layer's [num_mols + 1] row offsets (32-aligned)
  // pair rows, tile-blocked (trow).  pre(edge_nn.0) and pre(coord_nn.0) are not
  // stored: this kernel recomputes pre0 for silu', outer_x3_kernel recomputes
  // pre0 from xin (X of edge_nn.2) and pre(coord_nn.0) from the message (DY of
  // coord_nn.0, X of coord_nn.2), bitwise as here.  pe is stored as the
  // pre-activation: outer_x3_kernel applies silu on load, this kernel re-reads it.
  float* xin;        // [P][16] h_i, h_j, radial                     (X of edge_nn.0)
  float* p0;         // p0 / pc: never read or written; they stay because this struct is the kernel
  float* pe;         // [P][H] pre(edge_nn.2)           silu -> X of coord_nn.0 (the message)
  float* pc;         // argument block and removing them moves every later kernarg offset
  float* dp0;        // [P][H] d pre(edge_nn.0)                      (DY of edge_nn.0)
  float* dpe;        // [P][H] d pre(edge_nn.2)                      (DY of edge_nn.2)
  float* aphi;       // [P]    d phi                                 (DY of coord_nn.2)
  float* patt;       // [P]    att of the pair (VAR; 1 without attention): X of coord_nn.0 is e * att
  float* dlogit;     // [P]    d att_nn logit (VAR; 0 without attention) (DY of att_nn.0)
  float* tmax;       // [P / 32][TMX_W] per 32-row tile: max |operand| of the pair-row weight-gradient
                     // products (TMX_*), the scales outer_x3_kernel puts on a whole chunk
  float* su;         // atom rows [A][H] silu(vel_scaling_nn.0)      (X of vel_scaling_nn.2)
  float* au;         // [A][H] d pre(vel_scaling_nn.0)               (DY of vel_scaling_nn.0)
  float* sn;         // [A][H] silu(node_nn.0)                       (X of node_nn.2)
  float* an;         // [A][H] d pre(node_nn.0)                      (DY of node_nn.0)
  float* aq;         // [A]    dQ                                    (DY of vel_scaling_nn.2)
  float* agr;        // [A][nf] dG                                   (DY of node_nn.2)
  int32_t* err;
  // standalone EGCL.forward backward (enflow_egcl_backward_f32): adjoints of the
  // network outputs Q [A], F [A][3], G [A][nf] given directly (NULL: the flow's
  // leapfrog adjoint); the layer-input adjoints then start at zero
  // fused path: the forward taped the layer's pair words / row counts (TapeLayout::pairs,
  // cnt) and its pair counts ([num_mols], this layer's): loaded, not rebuilt (0: rebuild,
  // the standalone EGCL backward's tape)
  const int32_t* pair_counts_l;
  int tape_pairs;
  const float* eg_dQ;
  const float* eg_dF;
  const float* eg_dG;
  // large systems (lf_layer_bwd_kernel<.., BIG = true>): one workgroup per block of
  // rbl rows; the rows' pair words come from the large path's neighbour search
  // (enflow_large.h), column atoms are read from the tape; each pair's column-side
  // d h / d pos goes to colc (summed per column by lg_colsum / lg_colfinal)
  const int32_t* blk_start;
  int rbl, max_n;
  const int32_t* npairs_g;    // [A] pair words of row a
  const int32_t* cntrow_g;    // [A] edges of row a
  const uint32_t* pairs_g;    // [A][max_n] (label << 5 | mult << 27)
  const int32_t* boff;        // [blocks] first pair row of the block (32-aligned)
  int32_t* rowstart;          // [A] out: first pair row of row atom a
  float* colc;                // [pair rows][CSTR] out
  long long prb;              // pair rows allocated
  // caller-supplied edge list (lf_layer_bwd_kernel<.., BIG, LIST>, enflow_list.hip's
  // forward): one workgroup per 32 consecutive rows of the CSR, num_atoms = the
  // nodes; coord_diff read per edge, its adjoint stored per edge; colc is [E][CSTR]
  // (by edge, summed per column by el_colsum_kernel); boff as above
  const int32_t* l_row_ptr;   // [n + 1]
  const int32_t* l_col;       // [E]
  const float* l_cdiff;       // [E][3]
  float* l_acd;               // [E][3] out: d coord_diff
  int l_edges;                // E
};
// weight-fragment ring depth of the layer backward's F16X3 chains (prefetch distance
// + 1 k-steps; each slot is 8 VGPRs of hi / lo fragments).  Depth 3 / 4 / 6 measured
// within 1 % of 2 (profiles/r04/r04l_ab_train_split_once_and_ring_depth.txt)
#ifndef ENFLOW_BWD_X3_DEPTH
#define ENFLOW_BWD_X3_DEPTH 2
#endif
// per-tile operand maxima (BwdArgs::tmax): X / DY of edge_nn.0, edge_nn.2, coord_nn.0
enum { TMX_XIN = 0, TMX_DP0 = 1, TMX_X1 = 2, TMX_DPE = 3, TMX_MSG = 4, TMX_DPC = 5, TMX_W = 8 };
// edge_nn.0 input rows [h_i, h_j, radial]: 2 nf + 1 columns rounded up to 16
__host__ __device__ inline int xin_width(int nf) { return (2 * nf + 1 + 15) & ~15; }
constexpr int CSTR = NFMAX + 4;   // colc row: d h_j [NFMAX], d pos_j [3], pad
// the transposed edge_nn.0 GEMM (d [h_i, h_j, radial]) has one 32-row output
// tile: training needs 2 nf + 1 <= 32
// node_nf the backward takes: every feature of the build (nf 16: the radial
// row of the transposed edge_nn.0 GEMM, q = 2 nf = 32, lies past its 32-row
// output tile and is a separate dot product, see lf_layer_bwd_kernel GEMM5)
constexpr int BWD_NFMAX = NFMAX;

// <= 80 KB at (H, NMAX) = (128, 64): two workgroups per CU.  The node-MLP
// adjoint rows go through LDS a chunk of Smem::NBCH atoms at a time, in the
// union the pair build uses later.
template <int H, int NMAX>
struct BwdSmem {
  using Img = Smem<H, NMAX, NMAX, true>;
  Img f;
  float ah[NMAX * NFP], ag[NMAX * NFP], aG[NMAX * NFP];
  float apos[NMAX * 3], avel[NMAX * 3], aF[NMAX * 3];
  float aQ[NMAX];
  uint32_t nmax[NMAX / 32];   // per atom tile: max |d pre(node_nn.0)| (float bits)
  alignas(16) float wrad[NFMAX == 16 ? H : 1];   // nf 16: edge_nn.0.weight[:, 2 nf] (the radial column)
};

// Adjoint tiles span many decades (coord_nn.2 starts at gain 0.001), so before
// an F16X3 product their values are scaled by a power of two that puts the
// tile's max |x| in [2^12, 2^13): hi / lo parts stay normal fp16.  Returns the
// exact inverse scale.
template <int NT>
__device__ __forceinline__ float lane_absmax(const f32x16 (&X)[NT]) {
  float m = 0.f;
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) m = fmaxf(m, fabsf(X[t][r]));
  return m;
}
// m: the wave's max |x| over X (wave-uniform)
template <int NT>
__device__ __forceinline__ float tile_pow2_scale(f32x16 (&X)[NT], float m) {
  int ex = 0;
  if (m > 0.f && isfinite(m)) {
    frexpf(m, &ex);
    ex = 13 - ex;
    ex = ex > 100 ? 100 : (ex < -100 ? -100 : ex);
  }
  const float s = ldexpf(1.f, ex);
#pragma unroll
  for (int t = 0; t < NT; ++t) X[t] *= s;
  return ldexpf(1.f, -ex);
}
template <int NT>
__device__ __forceinline__ float tile_pow2_scale(f32x16 (&X)[NT]) {
  return tile_pow2_scale(X, wave_max(lane_absmax(X)));
}


// power of two putting m in [2^12, 2^13) (0 for m == 0 / non-finite)
__device__ __forceinline__ int pow2_exp(float m) {
  int ex = 0;
  if (m > 0.f && isfinite(m)) {
    frexpf(m, &ex);
    ex = 13 - ex;
    ex = ex > 100 ? 100 : (ex < -100 ? -100 : ex);
  }
  return ex;
}

// Node MLPs backward on F16X3 MFMA, atoms on the lanes (the forward's node
// phase transposed): per item (32 hidden units tp, 32 atoms at) the
// pre-activations of vel_scaling_nn.0 and node_nn.0 are recomputed, d pre of
// both (rows su / au / sn / an for the weight gradients), then
//   d h   += vel_scaling_nn.0.weight^T d u + node_nn.0.weight[:, :nf]^T d pre
//            (per-item partials, fixed-order sum over tp),
//   d agg  = node_nn.0.weight[:, nf:]^T d pre   (into sm.agg, over the message sums).
// Adjoint operands carry power-of-two scales like the edge chain's.
template <int H, int NMAX, bool VAR = false>
__device__ __forceinline__ void node_bwd_x3(BwdSmem<H, NMAX>& sb, const BwdArgs& B, const EgclLayout& L,
                                            const EgclBwdLayout& LB, int a0, int n, int nf, int tid) {
  auto& sm = sb.f;
  constexpr int NT = H / 32, NA = NMAX / 32, KS = H / 16, NI = NT * NA, IPW = (NI + WAVES - 1) / WAVES;
  constexpr int AST = BwdSmem<H, NMAX>::Img::AST;
  static_assert(NT * NFMAX * NMAX <= BwdSmem<H, NMAX>::Img::NBW, "dh partials do not fit sm.u.nb");
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, hh = lane >> 5;
  const rsrc_t W = weights_rsrc(B.Lp, L.total), WB = weights_rsrc(B.Bp, LB.total);
  const int vo = lane * 32;
  const float inv_v1 = B.Lp[L.scl + 7], inv_n1 = B.Lp[L.scl + 9], inv_n2 = B.Lp[L.scl + 11];
  const Act act = VAR ? act_of(B.Lp + L.vfl + 1) : act_silu();
  float* const gp = sm.u.nb;   // d h partials [tp][q][atom]
  for (int k = tid; k < H; k += BLOCK) {
    sm.bias[k] = B.Lp[L.bv1 + k];
    sm.bias[H + k] = B.Lp[L.wv2 + k];
    sm.bias[2 * H + k] = B.Lp[L.bn1 + k];
  }
  if (tid < NA) sb.nmax[tid] = 0u;
  __syncthreads();
  auto mm3 = [&](const rsrc_t& r, int off_floats, const f16x8& bh, const f16x8& bl, f32x16 acc) {
    const f32x4 ah = bload4(r, vo, off_floats * 4), al = bload4(r, vo + 16, off_floats * 4);
    acc = mfma_f16(ah, bh, acc);
    acc = mfma_f16(ah, bl, acc);
    return mfma_f16(al, bh, acc);
  };
  f32x16 keep[IPW];
#pragma unroll
  for (int ii = 0; ii < IPW; ++ii) {
    const int item = w + WAVES * ii;
    if (item >= NI) break;
    const int tp = item % NT, at = item / NT;
    const int a = at * 32 + j;
    const bool va = a < n;
    const int ac = va ? a : 0;
    f32x16 hin = (f32x16)0.f, gin = (f32x16)0.f;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {   // k = feature 8 hh + jj (half 1: features 8..15)
      const bool on = va && 8 * hh + jj < nf;
      hin[jj] = on ? sm.h[ac * NFP + 8 * hh + jj] : 0.f;
      gin[jj] = on ? sb.aG[ac * NFP + 8 * hh + jj] : 0.f;
    }
    f16x8 bh, bl;
    split_f16(hin, 0, bh, bl);
    f32x16 zu = mm3(W, L.wv1x + tp * 512, bh, bl, (f32x16)0.f);
    f32x16 zn = mm3(W, L.wn1hx + tp * 512, bh, bl, (f32x16)0.f);
    const float* arow = &sm.agg[ac * AST];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      f32x16 av;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) av[jj] = va ? arow[16 * ks + 8 * hh + jj] : 0.f;
      split_f16(av, 0, bh, bl);
      zn = mm3(W, L.wn1ax + (tp * KS + ks) * 512, bh, bl, zn);
    }
    // d silu(node_nn.0) = node_nn.2.weight^T d G
    f32x16 gs[1] = {gin};
    const float ig = tile_pow2_scale(gs);
    split_f16(gs[0], 0, bh, bl);
    const f32x16 asn = mm3(WB, LB.wn2Tx + tp * 512, bh, bl, (f32x16)0.f);
    const float ug = inv_n2 * ig;
    const float aq = va ? sb.aQ[ac] : 0.f;
    f32x16 au, an;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int f0 = 32 * tp + 8 * g4 + 4 * hh;
      const f32x4 b1 = ld4(sm.bias + f0), w2 = ld4(sm.bias + H + f0), bn = ld4(sm.bias + 2 * H + f0);
      f32x4 su4, au4, sn4, an4;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int r = 4 * g4 + u;
        const float z1 = fmaf(zu[r], inv_v1, b1[u]), z2 = fmaf(zn[r], inv_n1, bn[u]);
        float f1, f2, d1, d2;
        act_fd<VAR>(act, z1, f1, d1);
        act_fd<VAR>(act, z2, f2, d2);
        su4[u] = f1;
        sn4[u] = f2;
        au4[u] = aq * w2[u] * d1;
        an4[u] = asn[r] * ug * d2;
        au[r] = au4[u];
        an[r] = an4[u];
      }
      if (va) {
        const size_t row = (size_t)(a0 + a) * H + f0;
        st4(B.su + row, su4);
        st4(B.au + row, au4);
        st4(B.sn + row, sn4);
        st4(B.an + row, an4);
      }
    }
    // d h partial over this item's hidden units (rows f = rho(r, hh) < nf: r < NFMAX / 2)
    f32x16 tu[1] = {au}, tn[1] = {an};
    const float iu = tile_pow2_scale(tu), in = tile_pow2_scale(tn);
    f32x16 dv = (f32x16)0.f, dn = (f32x16)0.f;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      split_f16(tu[0], s2, bh, bl);
      dv = mm3(WB, LB.wvTx + (tp * 2 + s2) * 512, bh, bl, dv);
      split_f16(tn[0], s2, bh, bl);
      dn = mm3(WB, LB.wnhTx + (tp * 2 + s2) * 512, bh, bl, dn);
    }
    if (va) {
#pragma unroll
      for (int r = 0; r < NFMAX / 2; ++r) {
        const int q = rho(r, hh);
        if (q < nf) gp[(tp * NFMAX + q) * NMAX + a] = dv[r] * (inv_v1 * iu) + dn[r] * (inv_n1 * in);
      }
    }
    keep[ii] = an;
    float mx = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) mx = fmaxf(mx, fabsf(an[r]));
    mx = wave_max(mx);
    if (lane == 0) atomicMax(&sb.nmax[at], __float_as_uint(mx));
  }
  __syncthreads();   // message-sum rows consumed; partials and tile maxima complete
  // d pre(node_nn.0) rows into sm.agg, scaled per atom tile
#pragma unroll
  for (int ii = 0; ii < IPW; ++ii) {
    const int item = w + WAVES * ii;
    if (item >= NI) break;
    const int tp = item % NT, at = item / NT, a = at * 32 + j;
    const float s = ldexpf(1.f, pow2_exp(__uint_as_float(sb.nmax[at])));
    if (a < n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sm.agg[a * AST + 32 * tp + rho(r, hh)] = keep[ii][r] * s;
    }
  }
  for (int e = tid; e < n * nf; e += BLOCK) {   // d h: fixed-order sum over the hidden tiles
    const int a = e / nf, q = e - a * nf;
    float acc = 0.f;
#pragma unroll
    for (int tp = 0; tp < NT; ++tp) acc += gp[(tp * NFMAX + q) * NMAX + a];
    sb.ah[a * NFP + q] += acc;
  }
  __syncthreads();
  // d agg = node_nn.0.weight[:, nf:]^T d pre
#pragma unroll
  for (int ii = 0; ii < IPW; ++ii) {
    const int item = w + WAVES * ii;
    if (item >= NI) break;
    const int tp = item % NT, at = item / NT, a = at * 32 + j;
    const bool va = a < n;
    const float* arow = &sm.agg[(va ? a : 0) * AST];
    f32x16 acc = (f32x16)0.f;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      f32x16 av;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) av[jj] = va ? arow[16 * ks + 8 * hh + jj] : 0.f;
      f16x8 bh, bl;
      split_f16(av, 0, bh, bl);
      acc = mm3(WB, LB.wn1aTx + (tp * KS + ks) * 512, bh, bl, acc);
    }
    keep[ii] = acc * (inv_n1 * ldexpf(1.f, -pow2_exp(__uint_as_float(sb.nmax[at]))));
  }
  __syncthreads();   // d pre rows consumed
#pragma unroll
  for (int ii = 0; ii < IPW; ++ii) {
    const int item = w + WAVES * ii;
    if (item >= NI) break;
    const int tp = item % NT, at = item / NT, a = at * 32 + j;
    if (a < n) {
#pragma unroll
      for (int r = 0; r < 16; ++r) sm.agg[a * AST + 32 * tp + rho(r, hh)] = keep[ii][r];
    }
  }
  __syncthreads();
}

// Pair rows are stored tile-blocked: the 32 rows of a tile are contiguous per
// feature, element (row p, feature f) of a W-wide array at
// ((p / 32) * W + f) * 32 + p % 32.  A wave's accumulator register (one
// feature per half-wave, pairs on the lanes) is then two full 128-byte lines,
// and outer_acc_kernel reads a tile as one contiguous W x 32 block.
__device__ __forceinline__ size_t trow(size_t rtile, int W, int f, int j) {
  return ((rtile * W + f) << 5) + j;
}
// LIST: the offsets of the 32 rows from g0 of a CSR the caller passed, as
// el_layer_kernel forms them: row_ptr clamped to [0, E] and made non-decreasing,
// relative to the block's first edge.  roff (NULL: only the count) gets [0..32];
// returns the block's edges, e0 its first edge, bad whether clamping changed a value.
__device__ __forceinline__ int list_block_offsets(const int32_t* __restrict__ row_ptr, int n, int E, int g0,
                                                  int* roff, int& e0, bool& bad) {
  const int rb = min(32, n - g0);
  e0 = min(max(row_ptr[g0], 0), E);
  int acc = e0;
  bad = false;
  for (int a = 0; a <= 32; ++a) {
    const int raw = row_ptr[g0 + min(a, rb)];
    const int v = min(max(raw, 0), E);
    bad |= v < acc || v != raw;
    acc = max(acc, v);
    if (roff) roff[a] = acc - e0;
  }
  return acc - e0;
}

// VAR: layers may carry EGCL_NORM_DIFF / EGCL_TANH (read per layer from the
// packed forward layer; a second instance so the default kernel keeps its
// register allocation).  EGCL_ATTENTION is refused by the host.
// LIST (with BIG): the rows are 32 consecutive rows of a caller-supplied CSR
// (BwdArgs::l_*), no molecule, no box, no neighbour search; standalone EGCL
// adjoints (eg_dQ / eg_dF / eg_dG) only.
// LDJA (file scope: true in enflow_backward_ldja.hip's compile of this source,
// ENFLOW_BWD_LDJ_ATOMS): BwdArgs::adj_ldj holds one value per atom, the
// molecule's repeated; a workgroup's atoms are one molecule's, so it reads its
// first atom's.
template <int H, int NMAX, bool VAR = false, int PREC = PREC_F16X3, bool BIG = false, bool LIST = false>
__global__ void __launch_bounds__(BLOCK, 2) lf_layer_bwd_kernel(BwdArgs B) {
  static_assert(PREC == PREC_F32 || PREC == PREC_F16X3, "backward: fp32-accurate precisions only");
  static_assert(!BIG || NMAX == 32, "large systems: 32-row blocks");
  static_assert(!LIST || BIG, "the edge-list mode runs on the large path's row blocks");
  __shared__ BwdSmem<H, NMAX> sb;
  // BIG: the rows' first pair word within the block; LIST: + [33] the block's first edge
  __shared__ int roff[BIG ? (LIST ? 34 : 33) : 1];
  using Img = typename BwdSmem<H, NMAX>::Img;
  Img& sm = sb.f;
  constexpr int NT = H / 32;
  constexpr int AST = Img::AST;
  constexpr int NBCH = Img::NBCH;
  const int tid = threadIdx.x;
  // fused: m = the molecule, a0 / n its atoms.  BIG: a0 / n = the block's rows,
  // ma0 / mn = their molecule's atoms
  int m, a0, n, ma0, mn;
  if constexpr (LIST) {   // grid = ceil(nodes / 32): a0 < num_atoms; one "molecule" of every node
    m = 0;
    ma0 = 0;
    mn = B.num_atoms;
    a0 = blockIdx.x * 32;
    n = min(32, mn - a0);
  } else if constexpr (BIG) {
    const int b = blockIdx.x;
    if (b >= B.blk_start[B.num_mols]) return;
    m = seg_of(B.blk_start, B.num_mols, b);
    ma0 = B.mol_ptr[m];
    mn = B.mol_ptr[m + 1] - ma0;
    const int r0 = (b - B.blk_start[m]) * B.rbl;
    a0 = ma0 + r0;
    n = min(B.rbl, mn - r0);
  } else {
    m = blockIdx.x;
    a0 = B.mol_ptr[m];
    n = B.mol_ptr[m + 1] - a0;
    ma0 = a0;
    mn = n;
  }
  if (n > NMAX || B.nf > BWD_NFMAX) {
    if (tid == 0) atomicOr(B.err, n > NMAX ? ENFLOW_ERR_TOO_MANY_ATOMS : ENFLOW_ERR_TOO_MANY_FEATURES);
    return;
  }
  const int nf = B.nf;
  const float dt = B.dt;
  const EgclLayout L = egcl_layout(H, nf);
  const EgclBwdLayout LB = egcl_bwd_layout(H);
  const RawEgcl R = raw_egcl(H, nf);
  const TapeLayout T = tape_layout(B.num_atoms, nf, H, B.n_layers);
  const size_t la = (size_t)B.layer * B.num_atoms + a0;
  const float* Rp = B.Rp;
  const float* Bp = B.Bp;

  STAMP_DECL
  // ---- layer-input state (tape), message sums, Q; adjoints of the layer output
  if constexpr (LIST) {   // no positions, velocities or g on this path; its tape holds h, message sums, Q
    for (int e = tid; e < n * 3; e += BLOCK) {
      sm.pos[e] = 0.f;
      sm.vel[e] = 0.f;
      sm.boxa[e] = 0.f;
      sb.apos[e] = 0.f;
      sb.avel[e] = 0.f;
    }
    for (int e = tid; e < n * NFP; e += BLOCK) {
      const int a = e / NFP, q = e - a * NFP;
      sm.h[e] = q < nf ? B.tape[T.hx + (la + a) * T.ldhx + q] : 0.f;
      sm.g[e] = 0.f;
      sb.ah[e] = 0.f;
      sb.ag[e] = 0.f;
    }
  } else {
  for (int e = tid; e < n * 3; e += BLOCK) {
    sm.pos[e] = B.tape[T.pos + la * 3 + e];
    sm.vel[e] = B.tape[T.vel + la * 3 + e];
    sm.boxa[e] = B.box[(size_t)a0 * 3 + e];
    sb.apos[e] = B.apos[(size_t)a0 * 3 + e];
    sb.avel[e] = B.avel[(size_t)a0 * 3 + e];
  }
  for (int e = tid; e < n * NFP; e += BLOCK) {
    const int a = e / NFP, q = e - a * NFP;
    const bool v = q < nf;
    sm.h[e] = v ? B.tape[T.hx + (la + a) * T.ldhx + q] : 0.f;
    sm.g[e] = v ? B.tape[T.g + (la + a) * nf + q] : 0.f;
    sb.ah[e] = v ? B.ah[(size_t)(a0 + a) * nf + q] : 0.f;
    sb.ag[e] = v ? B.ag[(size_t)(a0 + a) * nf + q] : 0.f;
  }
  }
  for (int e = tid; e < n * H; e += BLOCK) {
    const int a = e / H, k = e - a * H;
    sm.agg[a * AST + k] = B.tape[T.hx + (la + a) * T.ldhx + nf + k];
  }
  for (int a = tid; a < n; a += BLOCK) sm.Q[a] = B.tape[T.q + la + a];
  if (tid == 0) sm.err = 0;
  if constexpr (LIST) {
    if (tid == 0) {
      int e0;
      bool bad;
      list_block_offsets(B.l_row_ptr, mn, B.l_edges, a0, roff, e0, bad);
      roff[33] = e0;
      if (bad) sm.err = ENFLOW_ERR_INDEX;
    }
    __syncthreads();
    // edges of the rows (the mean's divisor; an edge whose col is refused leaves it below)
    for (int a = tid; a < n; a += BLOCK) sm.cntrow[a] = roff[a + 1] - roff[a];
  } else if constexpr (BIG) {
    for (int a = tid; a < n; a += BLOCK) sm.cntrow[a] = B.cntrow_g[a0 + a];
    if (tid == 0) {
      int acc = 0;
      for (int a = 0; a < n; ++a) { roff[a] = acc; acc += B.npairs_g[a0 + a]; }
      for (int a = n; a <= 32; ++a) roff[a] = acc;
    }
  }
  __syncthreads();
  if constexpr (BIG) {   // the host's pair-row bound comes from the forward's counts
    if ((long long)B.boff[blockIdx.x] + ((roff[32] + 31) & ~31) > B.prb) {
      if (tid == 0) atomicOr(B.err, ENFLOW_ERR_TOO_MANY_ATOMS);
      return;
    }
    if constexpr (!LIST)
      for (int a = tid; a < n; a += BLOCK) B.rowstart[a0 + a] = B.boff[blockIdx.x] + roff[a];
  }
  MolRef M;
  M.a0 = ma0;
  M.n = mn;
  M.rc = LIST ? 0.f : B.r_cut[m];
  if constexpr (LIST) {
    M.bx = M.by = M.bz = 0.f;
  } else if constexpr (BIG) {   // the molecule's edge box: its first atom's (base.py:130)
    M.bx = B.box[(size_t)ma0 * 3 + 0];
    M.by = B.box[(size_t)ma0 * 3 + 1];
    M.bz = B.box[(size_t)ma0 * 3 + 2];
  } else {
    M.bx = n > 0 ? sm.boxa[0] : 0.f;
    M.by = n > 0 ? sm.boxa[1] : 0.f;
    M.bz = n > 0 ? sm.boxa[2] : 0.f;
  }

  STAMP(0);
  // ---- leapfrog adjoint (dynamics.py:13-21 in reverse order)
  const float aldj = LIST ? 0.f : B.adj_ldj[LDJA && n > 0 ? a0 : 0];   // n == 0: a0 may be num_atoms
  if (B.eg_dQ) {   // EGCL.forward alone (egcl.py:76-92): d Q / d F / d G given
    for (int a = tid; a < n; a += BLOCK) {
      sb.aQ[a] = B.eg_dQ[a0 + a];
      for (int d = 0; d < 3; ++d) {
        sb.aF[a * 3 + d] = B.eg_dF[(size_t)(a0 + a) * 3 + d];
        sb.apos[a * 3 + d] = 0.f;
        sb.avel[a * 3 + d] = 0.f;
      }
      for (int q = 0; q < NFP; ++q) {
        sb.aG[a * NFP + q] = q < nf ? B.eg_dG[(size_t)(a0 + a) * nf + q] : 0.f;
        sb.ah[a * NFP + q] = 0.f;
        sb.ag[a * NFP + q] = 0.f;
      }
    }
  } else
  for (int a = tid; a < n; a += BLOCK) {
    const float eq = expf(sm.Q[a]);
    float s = 0.f;
    for (int d = 0; d < 3; ++d) {
      const float avt = sb.avel[a * 3 + d] + sb.apos[a * 3 + d] * dt;   // pos' = pbc(pos + vel' dt)
      s += sm.vel[a * 3 + d] * avt;
      sb.avel[a * 3 + d] = eq * avt;                                   // vel' = e^Q vel + F dt
      sb.aF[a * 3 + d] = avt * dt;
    }
    sb.aQ[a] = eq * s + aldj;                                          // + ldj += Q.sum()
    for (int q = 0; q < nf; ++q) {
      const float agt = sb.ag[a * NFP + q] + sb.ah[a * NFP + q] * dt;  // h' = h + g' dt
      sb.ag[a * NFP + q] = agt;                                        // g' = g + G dt
      sb.aG[a * NFP + q] = agt * dt;
    }
  }
  __syncthreads();

  STAMP(1);
  // ---- node MLPs backward (egcl.py:26-30, 51-54, 90-92)
  for (int a = tid; a < n; a += BLOCK) B.aq[a0 + a] = sb.aQ[a];
  for (int e = tid; e < n * nf; e += BLOCK) {
    const int a = e / nf, q = e - a * nf;
    B.agr[(size_t)a0 * nf + e] = sb.aG[a * NFP + q];
  }
  if constexpr (PREC == PREC_F16X3) {
    node_bwd_x3<H, NMAX, VAR>(sb, B, L, LB, a0, n, nf, tid);
  } else {
  // VALU form (fp32 mode), NBCH atoms at a time:
  //      threads = (hidden unit k, atom group); adjoint rows staged in sm.u.nb
  {
    constexpr int NG = BLOCK / H;
    const int k = tid % H, grp = tid / H;
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float bv1 = Rp[R.bv1 + k], bn1 = Rp[R.bn1 + k], wv2 = Rp[R.Wv2 + k];
    for (int c0 = 0; c0 < n; c0 += NBCH) {
      const int c1 = min(n, c0 + NBCH);
      for (int a = c0 + grp; a < c1; a += NG) {
        float u = bv1, nn = bn1;
        for (int f = 0; f < nf; ++f) {
          const float hv = sm.h[a * NFP + f];
          u = fmaf(Bp[LB.wv1T + f * H + k], hv, u);
          nn = fmaf(Bp[LB.wn1T + f * H + k], hv, nn);
        }
        const float* arow = &sm.agg[a * AST];
        const float* wcol = Bp + LB.wn1T + NFMAX * H + k;
#pragma unroll 8
        for (int f = 0; f < H; ++f) nn = fmaf(wcol[f * H], arow[f], nn);
        const Act act = VAR ? act_of(B.Lp + L.vfl + 1) : act_silu();
        float su_v, sn_v, du, dn;
        act_fd<VAR>(act, u, su_v, du);
        act_fd<VAR>(act, nn, sn_v, dn);
        const float au = sb.aQ[a] * wv2 * du;
        float asn = 0.f;
        for (int q = 0; q < nf; ++q) asn = fmaf(Rp[R.Wn2 + q * H + k], sb.aG[a * NFP + q], asn);
        const float an = asn * dn;
        const size_t row = (size_t)(a0 + a) * H + k;
        B.su[row] = su_v;
        B.au[row] = au;
        B.sn[row] = sn_v;
        B.an[row] = an;
        sm.u.nb[(a - c0) * 2 * H + k] = au;
        sm.u.nb[(a - c0) * 2 * H + H + k] = an;
      }
      __syncthreads();
      // d agg = node_nn.0.weight[:, nf:]^T d pre  (overwrites the chunk's message sums)
      for (int a = c0 + grp; a < c1; a += NG) {
        const float* anr = &sm.u.nb[(a - c0) * 2 * H + H];
        const float* wr = Rp + R.Wn1 + nf + k;
        float s = 0.f;
#pragma unroll 8
        for (int kk = 0; kk < H; ++kk) s = fmaf(wr[kk * (H + nf)], anr[kk], s);
        sm.agg[a * AST + k] = s;
      }
      // d h += vel_scaling_nn.0.weight^T d u + node_nn.0.weight[:, :nf]^T d pre:
      // one (atom, feature) per wave step, hidden units over the lanes
      for (int e = w; e < (c1 - c0) * nf; e += WAVES) {
        const int al = e / nf, f = e - al * nf;
        const float* aur = &sm.u.nb[al * 2 * H];
        float s = 0.f;
        for (int kk = lane; kk < H; kk += 64)
          s += Rp[R.Wv1 + kk * nf + f] * aur[kk] + Rp[R.Wn1 + kk * (H + nf) + f] * aur[H + kk];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (lane == 0) sb.ah[(c0 + al) * NFP + f] += s;
      }
      __syncthreads();
    }
  }
  }
  STAMP(2);
  for (int k = tid; k < H; k += BLOCK) {   // edge-chain biases (the node phase used sm.bias)
    sm.bias[k] = B.Lp[L.be1 + k];
    sm.bias[H + k] = B.Lp[L.be2 + k];
    sm.bias[2 * H + k] = B.Lp[L.bc1 + k];
    sm.bias[3 * H + k] = B.Lp[L.wc2 + k];
    if constexpr (NFMAX == 16) {
      if (2 * nf + 1 > 32) sb.wrad[k] = Rp[R.We1 + k * (2 * nf + 1) + 2 * nf];
    }
  }
  if constexpr (!BIG) {
    if (B.tape_pairs) {   // the forward's list of this layer (same positions -> the same pairs)
      const int np = B.pair_counts_l[m];
      const float* tp = B.tape + T.pairs + la * TAPE_PAIR_CAP;
      for (int e = tid; e < np; e += BLOCK) sm.pairs[e] = __float_as_uint(tp[e]);
      for (int a = tid; a < n; a += BLOCK) sm.cntrow[a] = __float_as_int(B.tape[T.cnt + la + a]);
      if (tid == 0) sm.npairs = np;
      __syncthreads();
    } else {
      build_pairs(sm, M, tid);   // same positions as the forward -> same pairs (reuses sm.u)
    }
  }

  STAMP(3);
  // ---- edge chain backward, one 32-pair tile per wave step (egcl.py:57-74, 76-89)
  {
    const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);   // wave index: SGPR
    const int j = lane & 31, hh = lane >> 5;
    const int P_all = BIG ? roff[32] : sm.npairs;   // pairs of the molecule / row block
    const int TT_all = (P_all + 31) >> 5;
    const rsrc_t W = weights_rsrc(B.Lp, L.total);
    const rsrc_t WB = weights_rsrc(B.Bp, LB.total);
    const float hbx = M.bx * 0.5f, hby = M.by * 0.5f, hbz = M.bz * 0.5f;
    const size_t prow0 = BIG ? (size_t)B.boff[blockIdx.x] : (size_t)B.pair_off[m];
    // BIG: column atoms from the tape (this layer's input state of the molecule)
    const float* cpos = B.tape + T.pos + ((size_t)B.layer * B.num_atoms + ma0) * 3;
    const float* chx = B.tape + T.hx + ((size_t)B.layer * B.num_atoms + ma0) * T.ldhx;
    int le0 = 0;   // LIST: the block's first edge
    if constexpr (LIST) le0 = roff[33];
    const bool x3 = PREC == PREC_F16X3;
    const float inv1 = x3 ? B.Lp[L.scl + 1] : 1.f;   // edge_nn.2 / coord_nn.0 / edge_nn.0 (and ^T)
    const float inv2 = x3 ? B.Lp[L.scl + 3] : 1.f;
    const float inv0 = x3 ? B.Lp[L.scl + 5] : 1.f;
    auto nofill = [](int) {};
    const int vfl = VAR ? (int)B.Lp[L.vfl] : 0;   // wave-uniform constructor variants
    const bool v_nd = VAR && (vfl & EGCL_NORM_DIFF) != 0, v_tanh = VAR && (vfl & EGCL_TANH) != 0;
    const bool v_att = VAR && (vfl & EGCL_ATTENTION) != 0;
    const Act act = VAR ? act_of(B.Lp + L.vfl + 1) : act_silu();   // act_fn (egcl.py:11)
    // the molecule's tile-blocked rows (trow): buffer resources on its first
    // row, per element a wave-uniform byte offset (tile, feature) + the lane's
    const size_t nrow = (size_t)TT_all * 32;
    const rsrc_t rpe = rows_rsrc(B.pe + prow0 * H, nrow * H);
    const rsrc_t rdp0 = rows_rsrc(B.dp0 + prow0 * H, nrow * H), rdpe = rows_rsrc(B.dpe + prow0 * H, nrow * H);
    // edge_nn.0 input rows [h_i, h_j, radial]: 16 wide, 32 when 2 nf + 1 > 16 (nf = 8)
    const int XW = xin_width(nf);
    const rsrc_t rxin = rows_rsrc(B.xin + prow0 * XW, nrow * XW);
    const int lob = (hh * 128 + j) * 4;   // lane bytes: (feature 4hh, row j)
    // d h / d pos of the edge part: each wave adds into its own [atom][nf + 3]
    // slab (one wave's LDS atomics apply in a fixed order), summed over the
    // waves in wave order afterwards -> bitwise reproducible
    const int EW = nf + 3;
    float* const wacc = sm.u.nb + (size_t)w * n * EW;
    for (int e = tid; e < WAVES * n * EW; e += BLOCK) sm.u.nb[e] = 0.f;
    __syncthreads();
    constexpr int PCAP = Img::PC;   // BIG: pair words per pass through sm.pairs
    static_assert(PCAP % 32 == 0, "passes of whole tiles");
    for (int pp0 = 0;; pp0 += PCAP) {
    int P = P_all;
    if constexpr (BIG) {   // the next pass of the rows' pair words (| local row)
      P = min(PCAP, P_all - pp0);
      for (int e = tid; e < P; e += BLOCK) {
        const int pe = pp0 + e;
        int lo = 0, hi = n;   // row il: roff[il] <= pe < roff[il + 1]
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (roff[mid] <= pe) lo = mid;
          else hi = mid;
        }
        if constexpr (LIST) {   // one word per edge, as el_layer_kernel builds them
          const int c = B.l_col[(size_t)le0 + pe];
          const bool ok = (uint32_t)c < (uint32_t)mn;
          sm.pairs[e] = (uint32_t)lo | (ok ? ((uint32_t)c << 5) | (1u << 27) : 0u);
          if (!ok) {   // no read through it, out of the row's divisor (integer LDS atomics: order-free)
            atomicSub(&sm.cntrow[lo], 1);
            atomicOr(&sm.err, ENFLOW_ERR_INDEX);
          }
        } else {
          sm.pairs[e] = B.pairs_g[(size_t)(a0 + lo) * B.max_n + (pe - roff[lo])] | (uint32_t)lo;
        }
      }
      __syncthreads();
    }
    const int TT = (P + 31) >> 5;
    const int tpw = (TT + WAVES - 1) / WAVES;
    const int t0 = w * tpw, t1 = min(TT, t0 + tpw);
    // GEMM0's first-k-step weight fragments (the same for every tile): loaded
    // here, re-requested by each tile's second GEMM0 and carried into the next
    // tile's first, which then waits on no load
    f32x4 cfh[NT], cfl[NT];
    if constexpr (PREC == PREC_F16X3) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const int so = (L.we1x + (t * KS0MAX) * 512) * 4;
        cfh[t] = bload4(W, lane * 32, so);
        cfl[t] = bload4(W, lane * 32 + 16, so);
      }
    }
    for (int tile = t0; tile < t1; ++tile) {
      const int p = tile * 32 + j;
      const bool valid = p < P;
      const uint32_t pr = valid ? sm.pairs[p] : 0u;
      int i, jl;
      float c;   // multiplicity; 0 on padding lanes
      if constexpr (BIG) {
        i = (int)(pr & 31u);
        jl = (int)((pr >> 5) & 0x3fffffu);
        c = (float)(pr >> 27);
      } else {
        i = (int)(pr & 0xffu);
        jl = (int)((pr >> 8) & 0xffu);
        c = (float)(pr >> 16);
      }
      const int gt = (pp0 >> 5) + tile;   // tile index within the molecule's / block's rows
      const size_t Rw = prow0 + (size_t)(pp0 + p);
      // the tile's max |operand| of each weight-gradient product (outer_x3_kernel's
      // chunk scales): wave-reduced, lane 0 stores
      float* const tmx = B.tmax + ((prow0 >> 5) + (size_t)gt) * TMX_W;
      auto put_max = [&](int op, float m) {
        m = wave_max(m);
        if (lane == 0) tmx[op] = m;
        return m;
      };
      const int tsb = gt * H * 128;   // tile byte offset in an H-wide array (16-wide: / (H / 16))
      float cx, cy, cz;   // column atom position
      if constexpr (LIST) {
        cx = cy = cz = 0.f;
      } else if constexpr (BIG) {
        cx = cpos[jl * 3 + 0];
        cy = cpos[jl * 3 + 1];
        cz = cpos[jl * 3 + 2];
      } else {
        cx = sm.pos[jl * 3 + 0];
        cy = sm.pos[jl * 3 + 1];
        cz = sm.pos[jl * 3 + 2];
      }
      auto colh = [&](int q) -> float {   // column atom feature q < nf
        if constexpr (BIG) return chx[(size_t)jl * T.ldhx + q];
        else return sm.h[jl * NFP + q];
      };
      float dx, dy, dz;
      const size_t ge = (size_t)le0 + (size_t)(pp0 + p);   // LIST: the pair's edge in the sorted list
      if constexpr (LIST) {   // the caller's coord_diff (not read for a refused edge)
        const bool live = valid && c != 0.f;
        dx = live ? B.l_cdiff[ge * 3 + 0] : 0.f;
        dy = live ? B.l_cdiff[ge * 3 + 1] : 0.f;
        dz = live ? B.l_cdiff[ge * 3 + 2] : 0.f;
      } else {
        dx = pbc1(sm.pos[i * 3 + 0] - cx, hbx);
        dy = pbc1(sm.pos[i * 3 + 1] - cy, hby);
        dz = pbc1(sm.pos[i * 3 + 2] - cz, hbz);
      }
      const float radial = dx * dx + dy * dy + dz * dz;

      // X row of edge_nn.0: [h_i, h_j, radial]
      float mxin = valid ? radial : 0.f;
      auto xin_col = [&](int q) -> float {
        float v = 0.f;
        if (q < nf) v = sm.h[i * NFP + q];
        else if (q < 2 * nf) v = colh(q - nf);
        else if (q == 2 * nf) v = radial;
        v = valid ? v : 0.f;
        mxin = fmaxf(mxin, fabsf(v));
        return v;
      };
      if constexpr (NFMAX == 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) bstore(rxin, (hh * 256 + j) * 4, gt * XW * 128 + u * 128, xin_col(8 * hh + u));
        if (XW > 16 && hh == 0)   // q = 16 = 2 nf: the radial of an nf = 8 layer
          bstore(rxin, j * 4, gt * XW * 128 + 16 * 128, valid ? radial : 0.f);
      } else {   // 16-column chunks, every column of the row written
        for (int c16 = 0; c16 < XW / 16; ++c16)
#pragma unroll
          for (int u = 0; u < 8; ++u)
            bstore(rxin, (hh * 256 + j) * 4, gt * XW * 128 + (16 * c16 + u) * 128, xin_col(16 * c16 + 8 * hh + u));
      }
      put_max(TMX_XIN, mxin);

      // GEMM0 (recompute): pre0 = edge_nn.0 [h_i, h_j, radial] + be1.  Run twice per
      // tile (here, and again for silu'(pre0) after GEMM4) instead of parking pre0
      // in HBM: the same instruction sequence on the same operands, so both are
      // bitwise the forward's pre0 (outer_x3_kernel recomputes it from xin, too)
      auto gemm0 = [&](f32x16 (&x0)[NT], bool fresh) {
#pragma unroll
      for (int t = 0; t < NT; ++t) x0[t] = (f32x16)0.f;
      if constexpr (PREC == PREC_F16X3) {
        const int ks_n = gemm0_ksteps(nf), nch = gemm0_nch(nf);
        // the first k-step's fragments: carried (cfh / cfl), or requested before
        // the operand build so their L2 round trip overlaps it
        auto& fh0 = cfh;
        auto& fl0 = cfl;
        if (fresh) {
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            const int so = (L.we1x + (t * KS0MAX) * 512) * 4;
            fh0[t] = bload4(W, lane * 32, so);
            fl0[t] = bload4(W, lane * 32 + 16, so);
          }
        }
        for (int ks = 0; ks < ks_n; ++ks) {   // k order gemm0_col (as the forward)
          f32x16 in;
          if (ks < nch) {
            const int f0 = 8 * ks;
            if (BIG && hh) {
#pragma unroll
              for (int jj = 0; jj < 8; ++jj) in[jj] = f0 + jj < nf ? colh(f0 + jj) : 0.f;
            } else {
              const float* hrow = &sm.h[(hh ? jl : i) * NFP + f0];   // rows zero-padded past nf
#pragma unroll
              for (int jj = 0; jj < 8; ++jj) in[jj] = hrow[jj];
            }
            if (hh && ks == nch - 1 && gemm0_radial_slot7(nf)) in[7] = radial;
          } else {
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) in[jj] = 0.f;
            if (hh == 0) in[0] = radial;
          }
          f16x8 bh, bl;
          split_f16(in, 0, bh, bl);
#pragma unroll
          for (int t = 0; t < NT; ++t) {
            f32x4 ah = fh0[t], al = fl0[t];
            if (ks) {
              const int so = (L.we1x + (t * KS0MAX + ks) * 512) * 4;
              ah = bload4(W, lane * 32, so);
              al = bload4(W, lane * 32 + 16, so);
            }
            x0[t] = mfma_f16(ah, bh, x0[t]);
            x0[t] = mfma_f16(ah, bl, x0[t]);
            x0[t] = mfma_f16(al, bh, x0[t]);
          }
        }
        const float inv0 = B.Lp[L.scl + 5];
#pragma unroll
        for (int t = 0; t < NT; ++t) x0[t] *= inv0;
      } else {
#pragma unroll
        for (int s = 0; s < NFMAX + 1; ++s) {
          const int qc = 2 * (s - NFMAX / 2) + hh;
          const float b = s < NFMAX / 2 ? sm.h[i * NFP + 2 * s + hh]
                        : (s < NFMAX ? (BIG ? (qc < nf ? colh(qc) : 0.f) : sm.h[jl * NFP + qc])
                                     : (hh == 0 ? radial : 0.f));
#pragma unroll
          for (int t = 0; t < NT; ++t)
            x0[t] = mfma32(bload(W, lane * 4, (L.we1f + (t * (NFMAX + 1) + s) * 64) * 4), b, x0[t]);
        }
      }
      };
      f32x16 x0[NT];
      gemm0(x0, false);
      STAMP(4);
      // x1 = silu(pre0) (kept: B operand of GEMM1)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int f0 = 32 * t + 8 * g4 + 4 * hh;
          const f32x4 b = ld4(sm.bias + f0);
#pragma unroll
          for (int u = 0; u < 4; ++u) x0[t][4 * g4 + u] = act_v<VAR>(act, x0[t][4 * g4 + u] + b[u]);
        }
      put_max(TMX_X1, lane_absmax(x0));
      __builtin_amdgcn_sched_barrier(0);   // keep the stage's stores ahead of the next chain
      STAMP(5);
      // GEMM1 (recompute): e = silu(edge_nn.2 x1 + be2); pre_e stored
      f32x16 ev[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) ev[t] = (f32x16)0.f;
      chain_prec_fill<PREC, NT, 1, ENFLOW_BWD_X3_DEPTH>(W, L.we2f, L.we2x, L.we2b, x0, ev, lane, nofill);
      STAMP(18);
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int f0 = 32 * t + 8 * g4 + 4 * hh;
          const f32x4 b = ld4(sm.bias + H + f0);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float z = fmaf(ev[t][4 * g4 + u], inv1, b[u]);
            bstore(rpe, lob, tsb + ((32 * t + 8 * g4 + u) << 7), z);
            ev[t][4 * g4 + u] = act_v<VAR>(act, z);
          }
        }
      float att = 1.f;
      if (v_att) {   // egcl.py:60-62: message = e * sigmoid(att_nn(e))
        float d = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int g4 = 0; g4 < 4; ++g4) {
            const f32x4 wa = ld4(B.Lp + L.watt + 32 * t + 8 * g4 + 4 * hh);
#pragma unroll
            for (int u = 0; u < 4; ++u) d = fmaf(wa[u], ev[t][4 * g4 + u], d);
          }
        att = sigm_f(d + __shfl_xor(d, 32, 64) + B.Lp[L.batt]);
#pragma unroll
        for (int t = 0; t < NT; ++t) ev[t] *= att;
      }
      put_max(TMX_MSG, lane_absmax(ev));
      __builtin_amdgcn_sched_barrier(0);   // keep the stage's stores ahead of the next chain
      STAMP(6);
      // GEMM2 (recompute): phi = coord_nn.2 silu(coord_nn.0 e + bc1)
      f32x16 cv[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) cv[t] = (f32x16)0.f;
      chain_prec_fill<PREC, NT, 1, ENFLOW_BWD_X3_DEPTH>(W, L.wc1f, L.wc1x, L.wc1b, ev, cv, lane, nofill);
      STAMP(19);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // pre_e rows landed
      float part = 0.f;
      float mdz = 0.f;   // max |silu'(c)| (DY of coord_nn.0 = d phi * silu'(c))
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int f0 = 32 * t + 8 * g4 + 4 * hh;
          const f32x4 b = ld4(sm.bias + 2 * H + f0);
          const f32x4 w2 = ld4(sm.bias + 3 * H + f0);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const float z = fmaf(cv[t][4 * g4 + u], inv2, b[u]);
            float dz;
            if (!VAR || act.k == ACT_SILU) {
              const float s = sigmoid_f(z);
              part = fmaf(w2[u], z * s, part);   // pc is not stored: outer_x3_kernel recomputes it
              dz = s * (1.f + z * (1.f - s));    // silu'(c)
            } else {
              part = fmaf(w2[u], act_f(act, z), part);
              dz = act_d(act, z);
            }
            mdz = fmaxf(mdz, fabsf(dz));
            cv[t][4 * g4 + u] = w2[u] * dz;      // wc2 * silu'(c)
          }
        }
      float phi = part + __shfl_xor(part, 32, 64);
      if (v_tanh) phi = tanhf(phi);                             // egcl.py:40-42
      // norm_diff: trans uses coord_diff / (|coord_diff| + 1) (egcl.py:82-84)
      const float rr = v_nd ? sqrtf(radial) : 0.f;
      const float nd = v_nd ? __builtin_amdgcn_rcpf(rr + 1.f) : 1.f;
      const float dxn = dx * nd, dyn = dy * nd, dzn = dz * nd;
      // d phi from dF (egcl.py:71-74: mean over the row's edges, clamp, coords_weight)
      const float inv = B.cw / fmaxf((float)sm.cntrow[i], 1.f);
      const float gx = fabsf(dxn * phi) <= 100.f ? sb.aF[i * 3 + 0] * inv : 0.f;
      const float gy = fabsf(dyn * phi) <= 100.f ? sb.aF[i * 3 + 1] * inv : 0.f;
      const float gz = fabsf(dzn * phi) <= 100.f ? sb.aF[i * 3 + 2] * inv : 0.f;
      float aph = c * (gx * dxn + gy * dyn + gz * dzn);
      if (v_tanh) aph *= 1.f - phi * phi;                       // d of coord_nn.2's output
      if (hh == 0) B.aphi[Rw] = aph;
      if (VAR && hh == 0) B.patt[Rw] = att;
      put_max(TMX_DPC, mdz * fabsf(aph));
      // d pre(coord_nn.0) = dphi * wc2 * silu'(c)   (not stored: outer_acc rebuilds it from pc)
#pragma unroll
      for (int t = 0; t < NT; ++t) cv[t] *= aph;
      __builtin_amdgcn_sched_barrier(0);   // keep the stage's stores ahead of the next chain
      STAMP(7);
      // GEMM3: d e = c * d agg[i] + coord_nn.0.weight^T d pre(coord_nn.0)
      f32x16 ae[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) ae[t] = (f32x16)0.f;
      float sc3 = 1.f;
      if constexpr (PREC == PREC_F16X3) sc3 = tile_pow2_scale(cv);   // cv already stored unscaled
      STAMP(16);
      chain_prec_fill<PREC, NT, 1, ENFLOW_BWD_X3_DEPTH>(WB, LB.wc1T, LB.wc1Tx, 0, cv, ae, lane, nofill);
      // the parked pre_e rows are re-read after the chain (during or before it: 0.8 % slower, r04u)
      f32x16 rl[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) rl[t][r] = bload(rpe, lob, tsb + ((32 * t + 8 * (r >> 2) + (r & 3)) << 7));
      STAMP(17);
      const float u3 = inv2 * sc3;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) ae[t][r] = fmaf(ae[t][r], u3, c * sm.agg[i * AST + 32 * t + rho(r, hh)]);
      if constexpr (VAR) {   // ae = d message; through message = e * att
        float dl = 0.f;
        if (v_att) {
          float s = 0.f;
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) s = fmaf(ae[t][r], act_v<VAR>(act, rl[t][r]), s);   // d message . e
          dl = (s + __shfl_xor(s, 32, 64)) * att * (1.f - att);                      // d logit
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const f32x4 wa = ld4(B.Lp + L.watt + 32 * t + 8 * g4 + 4 * hh);
#pragma unroll
              for (int u = 0; u < 4; ++u) ae[t][4 * g4 + u] = fmaf(ae[t][4 * g4 + u], att, wa[u] * dl);
            }
        }
        if (hh == 0) B.dlogit[Rw] = dl;
      }
      STAMP(8);
      // d pre(edge_nn.2) = d e * silu'(pre_e)
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int f0 = 32 * t + 8 * g4 + 4 * hh;
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            ae[t][4 * g4 + u] *= dact_v<VAR>(act, rl[t][4 * g4 + u]);
            bstore(rdpe, lob, tsb + ((32 * t + 8 * g4 + u) << 7), ae[t][4 * g4 + u]);
          }
        }
      __builtin_amdgcn_sched_barrier(0);   // keep the stage's stores ahead of the next chain
      STAMP(9);
      // GEMM4: d x1 = edge_nn.2.weight^T d pre(edge_nn.2);  d pre0 = d x1 * silu'(pre0)
      f32x16 ax[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) ax[t] = (f32x16)0.f;
      float sc4 = 1.f;
      const float mdpe = put_max(TMX_DPE, lane_absmax(ae));
      if constexpr (PREC == PREC_F16X3) sc4 = tile_pow2_scale(ae, mdpe);   // ae already stored unscaled
      chain_prec_fill<PREC, NT, 1, ENFLOW_BWD_X3_DEPTH>(WB, LB.we2T, LB.we2Tx, 0, ae, ax, lane, nofill);
      STAMP(10);
      gemm0(rl, true);   // pre0 again (bitwise the first pass's)
      const float u4 = inv1 * sc4;
#pragma unroll
      for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int f0 = 32 * t + 8 * g4 + 4 * hh;
          const f32x4 b = ld4(sm.bias + f0);
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            ax[t][4 * g4 + u] = ax[t][4 * g4 + u] * u4 * dact_v<VAR>(act, rl[t][4 * g4 + u] + b[u]);
            bstore(rdp0, lob, tsb + ((32 * t + 8 * g4 + u) << 7), ax[t][4 * g4 + u]);
          }
        }
      __builtin_amdgcn_sched_barrier(0);   // keep the stage's stores ahead of the next chain
      STAMP(11);
      // GEMM5: d [h_i, h_j, radial] = edge_nn.0.weight^T d pre0   (rows q < 2nf+1)
      f32x16 ain = (f32x16)0.f;
      float sc5 = 1.f;
      const float mdp0 = put_max(TMX_DP0, lane_absmax(ax));
      if constexpr (PREC == PREC_F16X3) {
        sc5 = tile_pow2_scale(ax, mdp0);   // ax already stored unscaled
#pragma unroll
        for (int tp = 0; tp < NT; ++tp)
#pragma unroll
          for (int s2 = 0; s2 < 2; ++s2) {
            const int so = (LB.we1Tx + (tp * 2 + s2) * 512) * 4;
            const f32x4 gh = bload4(WB, lane * 32, so), gl = bload4(WB, lane * 32 + 16, so);
            f16x8 bh, bl;
            split_f16(ax[tp], s2, bh, bl);
            ain = mfma_f16(gh, bh, ain);
            ain = mfma_f16(gh, bl, ain);
            ain = mfma_f16(gl, bh, ain);
          }
        ain *= inv0 * sc5;
      } else {
#pragma unroll
        for (int tp = 0; tp < NT; ++tp)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const f32x4 a4 = bload4(WB, lane * 16, (LB.we1T + (tp * 4 + rg) * 256) * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) ain = mfma32(a4[u], ax[tp][4 * rg + u], ain);
          }
      }
      STAMP(12);
      float arad = 0.f;
      // nf 16: the radial row q = 2 nf = 32 is past the 32-row tile: a dot product
      // of d pre0 (this lane half's features, scaled by 1 / sc5 in f16x3) with
      // the radial column, the two halves summed, held by lane half 0
      float arad16 = 0.f;
      if constexpr (NFMAX == 16) {
        if (2 * nf + 1 > 32) {
          float s = 0.f;
#pragma unroll
          for (int t = 0; t < NT; ++t)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
              const f32x4 wr = ld4(sb.wrad + 32 * t + 8 * g4 + 4 * hh);
#pragma unroll
              for (int u = 0; u < 4; ++u) s = fmaf(ax[t][4 * g4 + u], wr[u], s);
            }
          s += __shfl_xor(s, 32, 64);
          arad16 = hh == 0 ? s * sc5 : 0.f;
        }
      }
      if (valid) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int q = rho(r, hh);
          if (q < nf) atomicAdd(&wacc[i * EW + q], ain[r]);
          else if (q < 2 * nf) {
            if constexpr (LIST) B.colc[ge * CSTR + q - nf] = ain[r];
            else if constexpr (BIG) B.colc[Rw * CSTR + q - nf] = ain[r];
            else atomicAdd(&wacc[jl * EW + q - nf], ain[r]);
          } else if (q == 2 * nf) arad = ain[r];
        }
        if (NFMAX == 16 && 2 * nf + 1 > 32) arad = arad16;
      }
      // d coord_diff (radial = |cd|^2, trans = cd * phi), d pos_i += ., d pos_j -= .
      const float sF = hh == 0 ? c * phi : 0.f;
      float ux = sF * gx, uy = sF * gy, uz = sF * gz;             // d (normalised) coord_diff
      if (v_nd) {   // through cd / (|cd| + 1): nd u - nd^2 (u . cd) cd / |cd|
        const float k2 = rr > 0.f ? nd * nd * (ux * dx + uy * dy + uz * dz) / rr : 0.f;
        ux = nd * ux - k2 * dx;
        uy = nd * uy - k2 * dy;
        uz = nd * uz - k2 * dz;
      }
      const float tx = ux + 2.f * dx * arad;
      const float ty = uy + 2.f * dy * arad;
      const float tz = uz + 2.f * dz * arad;
      if constexpr (LIST) {   // d coord_diff of the edge: both half-waves' parts, one store, nothing to reduce
        const float sx = tx + __shfl_xor(tx, 32, 64), sy = ty + __shfl_xor(ty, 32, 64),
                    sz = tz + __shfl_xor(tz, 32, 64);
        if (valid && hh == 0) {
          B.l_acd[ge * 3 + 0] = sx;
          B.l_acd[ge * 3 + 1] = sy;
          B.l_acd[ge * 3 + 2] = sz;
        }
      } else if constexpr (BIG) {   // the column's d pos: both half-waves' parts, one store
        const float sx = tx + __shfl_xor(tx, 32, 64), sy = ty + __shfl_xor(ty, 32, 64),
                    sz = tz + __shfl_xor(tz, 32, 64);
        if (valid) {
          if (tx != 0.f || ty != 0.f || tz != 0.f) {
            atomicAdd(&wacc[i * EW + nf + 0], tx);
            atomicAdd(&wacc[i * EW + nf + 1], ty);
            atomicAdd(&wacc[i * EW + nf + 2], tz);
          }
          if (hh == 0) {
            B.colc[Rw * CSTR + NFMAX + 0] = -sx;
            B.colc[Rw * CSTR + NFMAX + 1] = -sy;
            B.colc[Rw * CSTR + NFMAX + 2] = -sz;
          }
        }
      } else if (valid && (tx != 0.f || ty != 0.f || tz != 0.f)) {
        atomicAdd(&wacc[i * EW + nf + 0], tx);
        atomicAdd(&wacc[i * EW + nf + 1], ty);
        atomicAdd(&wacc[i * EW + nf + 2], tz);
        atomicAdd(&wacc[jl * EW + nf + 0], -tx);
        atomicAdd(&wacc[jl * EW + nf + 1], -ty);
        atomicAdd(&wacc[jl * EW + nf + 2], -tz);
      }
    }
    if constexpr (!BIG) break;
    __syncthreads();   // sm.pairs consumed
    if (pp0 + PCAP >= P_all) break;
    }
    __syncthreads();
    for (int e = tid; e < n * EW; e += BLOCK) {
      float s = 0.f;
#pragma unroll
      for (int ww = 0; ww < WAVES; ++ww) s += sm.u.nb[(size_t)ww * n * EW + e];
      const int a = e / EW, q = e - a * EW;
      if (q < nf) sb.ah[a * NFP + q] += s;
      else sb.apos[a * 3 + q - nf] += s;
    }
  }
  __syncthreads();

  STAMP(13);
  // ---- adjoints of the layer input
  if constexpr (!LIST) {
    for (int e = tid; e < n * 3; e += BLOCK) {
      B.apos[(size_t)a0 * 3 + e] = sb.apos[e];
      B.avel[(size_t)a0 * 3 + e] = sb.avel[e];
    }
  }
  for (int e = tid; e < n * nf; e += BLOCK) {
    const int a = e / nf, q = e - a * nf;
    B.ah[(size_t)a0 * nf + e] = sb.ah[a * NFP + q];
    if constexpr (!LIST) B.ag[(size_t)a0 * nf + e] = sb.ag[a * NFP + q];
  }
  STAMP(14);
  STAMP_FLUSH
  if (tid == 0 && sm.err) atomicOr(B.err, sm.err);
}

// ---------------------------------------------------------------------------
// ArgMax.forward backward (enflow/nn/argmax.py:13-25): adjoint of z (= d h at
// the first layer's input) and of log_q (= d ldj) -> parameter-gradient rows.
// LDJA (file scope, ENFLOW_BWD_LDJ_ATOMS): adj_ldj holds one value per atom.
// ---------------------------------------------------------------------------
template <int H, int NMAX>
__global__ void __launch_bounds__(BLOCK) argmax_bwd_kernel(const int32_t* mol_ptr, int nf, const float* hdata,
                                                          const float* noise, const float* Draw, const float* az,
                                                          const float* adj_ldj, float* apre_rows, float* spre_rows,
                                                          float* anet_rows) {
  __shared__ float pre[NMAX][H + 1];
  __shared__ float spv[NMAX][H + 1];   // act(pre), once per (atom, unit): network.2's input
  __shared__ float net[NMAX][2 * NFMAX];
  __shared__ float anet[NMAX][2 * NFMAX];
  __shared__ float hs[NMAX][NFMAX];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  if (n > NMAX) return;
  const int rW1 = 0, rb1 = H * nf, rW2 = rb1 + H, rb2 = rW2 + 2 * nf * H;
  const Act am = act_of(Draw + rb2 + 2 * nf);   // network.1 (the raw vector's act trailer, ABI 10)
  for (int e = tid; e < n * nf; e += BLOCK) hs[e / nf][e % nf] = hdata[(size_t)a0 * nf + e];
  __syncthreads();
  constexpr int NG = BLOCK / H;
  const int k = tid % H, grp = tid / H;
  for (int a = grp; a < n; a += NG) {
    float v = Draw[rb1 + k];
    for (int f = 0; f < nf; ++f) v = fmaf(Draw[rW1 + k * nf + f], hs[a][f], v);
    pre[a][k] = v;
    const float sv = am.k == ACT_SILU ? v * sigmoid_f(v) : act_f(am, v);
    spv[a][k] = sv;
    spre_rows[(size_t)(a0 + a) * H + k] = sv;
  }
  __syncthreads();
  for (int e = tid; e < n * 2 * nf; e += BLOCK) {
    const int a = e / (2 * nf), o = e - a * 2 * nf;
    float s = Draw[rb2 + o];
    for (int kk = 0; kk < H; ++kk) s = fmaf(Draw[rW2 + o * H + kk], spv[a][kk], s);
    net[a][o] = s;
  }
  __syncthreads();
  // LDJA: the atom's own value -- a 32-atom window of the large path can hold atoms of two molecules
  const float aldj = LDJA ? (tid < n ? adj_ldj[a0 + tid] : 0.f) : adj_ldj[0];
  if (tid < n) {
    const int a = tid;
    float u[NFMAX], hv[NFMAX], sg[NFMAX], zz[NFMAX], els[NFMAX];
    float T = 0.f;
#pragma unroll
    for (int q = 0; q < NFMAX; ++q) {
      if (q < nf) {
        els[q] = expf(net[a][q]);
        u[q] = net[a][nf + q] + noise[(size_t)(a0 + a) * nf + q] * els[q];
        hv[q] = hs[a][q];
        zz[q] = az[(size_t)(a0 + a) * nf + q];
        T += hv[q] * u[q];
      }
    }
    float S = 0.f, Az = 0.f;
#pragma unroll
    for (int q = 0; q < NFMAX; ++q) {
      if (q < nf) {
        sg[q] = sigmoid_f(T - u[q]);
        const float w = (1.f - hv[q]) * (1.f - sg[q]);
        S += w;
        Az += zz[q] * w;
      }
    }
#pragma unroll
    for (int q = 0; q < NFMAX; ++q) {
      if (q < nf) {
        const float au = zz[q] * hv[q] + (1.f - hv[q]) * zz[q] * sg[q] + hv[q] * Az +
                         aldj * (-u[q] - hv[q] * S + (1.f - hv[q]) * (1.f - sg[q]));
        const float als = au * noise[(size_t)(a0 + a) * nf + q] * els[q] - aldj;
        anet[a][q] = als;
        anet[a][nf + q] = au;
        anet_rows[(size_t)(a0 + a) * 2 * nf + q] = als;
        anet_rows[(size_t)(a0 + a) * 2 * nf + nf + q] = au;
      }
    }
  }
  __syncthreads();
  for (int a = grp; a < n; a += NG) {
    float s = 0.f;
    for (int o = 0; o < 2 * nf; ++o) s = fmaf(Draw[rW2 + o * H + k], anet[a][o], s);
    const float p = pre[a][k];
    if (am.k == ACT_SILU) {
      const float sp = sigmoid_f(p);
      apre_rows[(size_t)(a0 + a) * H + k] = s * sp * (1.f + p * (1.f - sp));
    } else {
      apre_rows[(size_t)(a0 + a) * H + k] = s * act_d(am, p);
    }
  }
}

// ---------------------------------------------------------------------------
// instance selection (host)
// ---------------------------------------------------------------------------
// The two functions below are templates only to be instantiated where a translation
// unit first calls them: a code object lays its kernel instances out in the order of
// their first use, and that is the call site, not the point where this header is
// included.

// lf_layer_bwd_kernel of one layer: the fused instances (one workgroup per
// molecule of <= nmax atoms) or, big, the large-system row-block instances.
// f32b: the fp32 backward, on the generic (VAR) instance (any flags / act_fn).
// The kernels are laid out in the code object in the order they are named here.
template <int = 0>
static inline void layer_bwd_launch(int H, int nmax, bool big, bool f32b, bool variants, int grid, hipStream_t st,
                                    const BwdArgs& A) {
#define LAYER_BWD(HH, NN, VARF, PRECF, BIGF)                                                                      \
  ENFLOW_TIMED("lf_layer_bwd_kernel", st,                                                                         \
               hipLaunchKernelGGL((lf_layer_bwd_kernel<HH, NN, VARF, PRECF, BIGF>), dim3(grid), dim3(BLOCK), 0, st, A))
#define LAYER_BWD_BIG(HH, NN)                                             \
  do {                                                                    \
    if (f32b) LAYER_BWD(HH, NN, true, PREC_F32, true);                    \
    else if (variants) LAYER_BWD(HH, NN, true, PREC_F16X3, true);         \
    else LAYER_BWD(HH, NN, false, PREC_F16X3, true);                      \
  } while (0)
  if (!big) {
    if (f32b) DISPATCH_HN(H, nmax, LAYER_BWD, true, PREC_F32, false);
    else if (variants) DISPATCH_HN(H, nmax, LAYER_BWD, true, PREC_F16X3, false);
    else DISPATCH_HN(H, nmax, LAYER_BWD, false, PREC_F16X3, false);
  } else {
    DISPATCH_H(H, LAYER_BWD_BIG, 32);
  }
#undef LAYER_BWD_BIG
#undef LAYER_BWD
}

// argmax_bwd_kernel on `grid` molecules or atom chunks (ptr: their [grid + 1] atom
// offsets, <= nmax atoms each)
template <int = 0>
static inline void argmax_bwd_launch(int H, int nmax, int grid, hipStream_t st, const int32_t* ptr, int nf,
                                     const float* h_data, const float* noise, const float* dequant_raw,
                                     const float* adj_h, const float* adj_ldj, float* apre, float* spre, float* anet) {
#define CALL(HH, NN)                                                                                  \
  hipLaunchKernelGGL((argmax_bwd_kernel<HH, NN>), dim3(grid), dim3(BLOCK), 0, st, ptr, nf, h_data, noise, \
                     dequant_raw, adj_h, adj_ldj, apre, spre, anet)
  DISPATCH_HN(H, nmax, CALL);
#undef CALL
}

// The ENFLOW_BWD_LDJ_ATOMS launches: the two functions above on
// enflow_backward_ldja.hip's instances, under the same timer name.
void launch_layer_bwd_ldja(int H, int nmax, bool big, bool f32b, bool variants, int grid, hipStream_t st,
                           const BwdArgs& A);
void launch_argmax_bwd_ldja(int H, int nmax, int chunks, hipStream_t st, const int32_t* ptr, int nf, const float* h_data,
                            const float* noise, const float* dequant_raw, const float* adj_h, const float* adj_ldj,
                            float* apre, float* spre, float* anet);
