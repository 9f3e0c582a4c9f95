// enflow_wide.hip -- EGCL layers of hidden width 256 (hidden_nf 129..256,
// zero-padded) on the large-system path: inference, forward and reverse.
//
// enflow_large.hip runs a layer as images -> id_mapping -> pair words -> layer;
// only the last launch depends on the hidden width.  lg_wide_layer_kernel is
// that launch at width 256: one workgroup per row block, the block's pair
// words streamed through LDS in passes, tiles of 32 pairs.  At this width a
// tile's input and output accumulators do not both fit in registers, so the
// activations pass between the GEMMs through LDS: the four waves share one
// 32-pair tile, each wave computes 64 of the 256 output features of every
// GEMM (two 32x32 accumulators) on v_mfma_f32_32x32x2_f32, reads the tile's
// activations [pair][k] from one LDS buffer and writes act(. + bias) to the
// other.  Weights are row-major [out][k] in L2 (enflow_wide.h): lane
// (row, half) loads k-slots 8 q + 4 half .. + 3 as one float4, the matching
// activations as one ds_read_b128, and issues four MFMAs.
//
// Segment sums run in pair order, one thread per feature; dots over the
// hidden width (attention, coord_nn.2, vel_scaling_nn.2) by eight threads per
// pair with a butterfly: every reduction has a fixed order, results are
// bitwise reproducible.
//
// Precisions: PREC_F32 as above.  PREC_F16X3 (the default) runs every GEMM on
// v_mfma_f32_32x32x16_f16 with the hi / lo split of flow_device.h: weights
// pre-scaled by a power of two and split at pack time, activations split as
// they are read from LDS, three products hi*hi + hi*lo + lo*hi, and both ends
// of the range guarded as in the narrow kernels: ENFLOW_ERR_RANGE on
// non-finite results (and on a non-finite phi / attention logit before tanh,
// the clamp or the sigmoid squash it), ENFLOW_ERR_SMALL through the BIGK_*
// test of every operand kind.  The host then re-runs the batch with fp32 GEMMs.
#include "enflow_wide.h"
#include "enflow_host.h"

constexpr int WH = ENFLOW_WIDE_H256;
constexpr int WXS = WIDE_KN + 4;   // LDS row stride of the activation buffers (floats, 16-B rows)
constexpr int WAST = WH + 4;       // agg row: 256 message sums, 3 force sums
constexpr int WPC = 512;           // pair words per pass
static_assert(BLOCK == WH, "one thread per hidden feature in the segment sums");

struct WideSmem {
  alignas(16) float xa[32 * WXS];
  alignas(16) float xb[32 * WXS];
  alignas(16) float agg[32 * WAST];
  float pos[32 * 3];
  float h[32 * NFP], G[32 * NFP];
  float Q[32];
  uint32_t pairs[WPC];
  float pcd[32][4];   // coord_diff of the tile's pairs (after norm_diff)
  float pc[32];       // multiplicity
  int prow[32];       // row within the block
  float pdot[32];
  int cntrow[32];
  int roff[33];
  float red[WAVES];
  int err;
  uint32_t big;       // BIGK_* seen by this row block (F16X3 small-operand guard)
};

// acc[t] += W[f0 + 32 t + (lane & 31)][k] X[lane & 31][k] over k < K (K % 8 == 0)
template <int NTW>
__device__ __forceinline__ void wide_gemm(const float* __restrict__ W, int K, int f0, const float* X,
                                          f32x16 (&acc)[NTW], int lane) {
  const int j = lane & 31, hh = lane >> 5;
  const float* xr = X + j * WXS + 4 * hh;
  const float* wr = W + (size_t)(f0 + j) * K + 4 * hh;
#pragma unroll 2
  for (int k = 0; k < K; k += 8) {
    const f32x4 xv = ld4(xr + k);
    f32x4 wa[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) wa[t] = ld4(wr + (size_t)(32 * t) * K + k);
#pragma unroll
    for (int t = 0; t < NTW; ++t)
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[t] = mfma32(wa[t][u], xv[u], acc[t]);
  }
}

// the same in F16X3: Wx = the matrix's split section (hi [rows][K] fp16, then lo), scaled by 2^s;
// ohi collects the OR of the activations' packed hi words (or_hi: the small-operand guard)
template <int NTW>
__device__ __forceinline__ void wide_gemm_x3(const float* __restrict__ Wx, int rows, int K, int f0, const float* X,
                                             f32x16 (&acc)[NTW], int lane, uint32_t& ohi) {
  const int j = lane & 31, hh = lane >> 5;
  const _Float16* hi = reinterpret_cast<const _Float16*>(Wx);
  const _Float16* lo = hi + (size_t)rows * K;
  const float* xr = X + j * WXS + 8 * hh;
  const size_t wo = (size_t)(f0 + j) * K + 8 * hh;
#pragma unroll 2
  for (int k = 0; k < K; k += 16) {
    const f32x4 x0 = ld4(xr + k), x1 = ld4(xr + k + 4);
    f16x8 bh, bl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = e < 4 ? x0[e & 3] : x1[e & 3];
      const _Float16 h = (_Float16)x;
      bh[e] = h;
      bl[e] = (_Float16)(x - (float)h);
    }
    ohi = or_hi(ohi, bh);
    f16x8 ah[NTW], al[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      ah[t] = *reinterpret_cast<const f16x8*>(hi + wo + (size_t)(32 * t) * K + k);
      al[t] = *reinterpret_cast<const f16x8*>(lo + wo + (size_t)(32 * t) * K + k);
    }
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[t], bh, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[t], bl, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[t], bh, acc[t], 0, 0, 0);
    }
  }
}

// matrix m of the packed layer (wide_mat) times X, rows f0 ..; returns 1 / scale of the result
// (1 in fp32).  nvalid: rows of X that hold data; kind: the operand's BIGK_* bit, ORed into bigw
// when any of those rows holds a value >= 2^-7.
template <int PREC, int NTW>
__device__ __forceinline__ float wide_mm(const float* __restrict__ Lp, const WideLayout& L, int m, int f0,
                                         const float* X, f32x16 (&acc)[NTW], int lane, int nvalid, uint32_t kind,
                                         uint32_t& bigw) {
  const WideMat M = wide_mat(L, m);
#pragma unroll
  for (int t = 0; t < NTW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  if constexpr (PREC == PREC_F16X3) {
    uint32_t ohi = 0u;
    wide_gemm_x3<NTW>(Lp + L.x3 + M.off, M.rows, M.K, f0, X, acc, lane, ohi);
    if (__ballot((ohi & ENFLOW_BIG_BITS) != 0u && (lane & 31) < nvalid)) bigw |= kind;
    return Lp[L.scl + 2 * M.scl + 1];
  } else {
    wide_gemm<NTW>(Lp + M.off, M.K, f0, X, acc, lane);
    return 1.f;
  }
}

template <int NTW>
__device__ __forceinline__ void wide_zero(f32x16 (&acc)[NTW]) {
#pragma unroll
  for (int t = 0; t < NTW; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
}

// Y[pair][f] = act(acc + bias[f]) for the wave's features f0 .. f0 + 32 NTW - 1
// (register r of lane half hh holds feature rho(r, hh) of the tile)
template <int NTW>
__device__ __forceinline__ void wide_store_act(const f32x16 (&acc)[NTW], const float* __restrict__ bias, int f0,
                                               float* Y, int lane, const Act& act, float ik) {
  const int j = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int t = 0; t < NTW; ++t)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int fb = f0 + 32 * t + 8 * g4 + 4 * hh;
      const f32x4 bv = ld4(bias + fb);
      f32x4 v;
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = act_v<true>(act, fmaf(acc[t][4 * g4 + u], ik, bv[u]));
      st4(Y + j * WXS + fb, v);
    }
}

// out[p] = sum_f v[f] X[p][f], p < 32: eight threads per row, strided features, butterfly
__device__ __forceinline__ void wide_row_dot(const float* X, const float* __restrict__ v, float* out, int tid) {
  const int p = tid >> 3, s = tid & 7;
  float a = 0.f;
  for (int i = 0; i < WH / 8; ++i) {
    const int f = s + 8 * i;
    a = fmaf(v[f], X[p * WXS + f], a);
  }
  a += __shfl_xor(a, 1, 64);
  a += __shfl_xor(a, 2, 64);
  a += __shfl_xor(a, 4, 64);
  if (s == 0) out[p] = a;
}

// one 256-wide EGCL layer (+ leapfrog update) for one row block; modes as
// lg_layer_kernel: 0 flow forward, 1 flow reverse, 2 EGCL only, 3 reverse
// with its log|detJ|
template <int PREC>
__global__ void __launch_bounds__(BLOCK) lg_wide_layer_kernel(LgArgs B, int mode) {
  __shared__ WideSmem sm;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B.blk_start[B.num_mols]) return;
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m = seg_of(B.blk_start, B.num_mols, b);
  const int a0 = B.mol_ptr[m], n = B.mol_ptr[m + 1] - a0;
  const float hbx = B.box[(size_t)a0 * 3 + 0] * 0.5f, hby = B.box[(size_t)a0 * 3 + 1] * 0.5f,
              hbz = B.box[(size_t)a0 * 3 + 2] * 0.5f;
  const int r0 = (b - B.blk_start[m]) * B.rbl, rb = min(B.rbl, n - r0);
  const int g0 = a0 + r0;   // first row atom (global)
  const int nf = B.nf;
  const float* __restrict__ Lp = B.layer;
  const WideLayout L = wide_layout();
  const int vfl = (int)Lp[L.misc + 2];
  const bool v_att = (vfl & EGCL_ATTENTION) != 0, v_nd = (vfl & EGCL_NORM_DIFF) != 0, v_tanh = (vfl & EGCL_TANH) != 0;
  const Act act = act_of(Lp + L.misc + 3);
  const float batt = Lp[L.misc + 1];

  for (int e = tid; e < 32 * 3; e += BLOCK) sm.pos[e] = e < rb * 3 ? B.pos[(size_t)g0 * 3 + e] : 0.f;
  for (int e = tid; e < 32 * NFP; e += BLOCK) {   // rows zero-padded past nf and rb
    const int a = e / NFP, q = e - a * NFP;
    sm.h[e] = (a < rb && q < nf) ? B.h[(size_t)(g0 + a) * nf + q] : 0.f;
  }
  for (int e = tid; e < 32 * WAST; e += BLOCK) sm.agg[e] = 0.f;
  if (tid < 32) sm.cntrow[tid] = tid < rb ? B.cntrow[g0 + tid] : 0;
  if (tid == 0) {
    sm.err = 0;
    sm.big = 0u;
    int acc = 0;
    for (int a = 0; a < rb; ++a) { sm.roff[a] = acc; acc += B.npairs[g0 + a]; }
    for (int a = rb; a <= 32; ++a) sm.roff[a] = acc;
  }
  __syncthreads();
  const int tot = sm.roff[32];
  const float* cpos = B.pos + (size_t)a0 * 3;
  const float* ch = B.h + (size_t)a0 * nf;
  f32x16 acc[2];
  uint32_t bigw = 0u;   // wave-uniform
  float ik;
  for (int p0 = 0; p0 < tot; p0 += WPC) {
    const int cnt = min(WPC, tot - p0);
    for (int e = tid; e < cnt; e += BLOCK) {
      const int pe = p0 + e;
      int lo = 0, hi = rb;   // row il: roff[il] <= pe < roff[il + 1]
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (sm.roff[mid] <= pe) lo = mid;
        else hi = mid;
      }
      sm.pairs[e] = B.pairs[(size_t)(g0 + lo) * B.max_n + (pe - sm.roff[lo])] | (uint32_t)lo;
    }
    __syncthreads();
    for (int t0 = 0; t0 < cnt; t0 += 32) {
      const int np = min(32, cnt - t0);
      // edge_nn.0's input [h_i | h_j | radial | 0..] of the tile's pairs (egcl.py:57, 79); rows past np zero
      for (int e = tid; e < 32 * WIDE_K0; e += BLOCK) {
        const int p = e / WIDE_K0, k = e - p * WIDE_K0;
        float v = 0.f;
        if (p < np) {
          const uint32_t pr = sm.pairs[t0 + p];
          const int il = (int)(pr & 31u), jl = (int)((pr >> 5) & 0x3fffffu);
          if (k < NFMAX) v = sm.h[il * NFP + k];
          else if (k < 2 * NFMAX) v = (k - NFMAX) < nf ? ch[(size_t)jl * nf + (k - NFMAX)] : 0.f;
          else if (k == 2 * NFMAX) {
            // Edges.coord_diff with the reference's half-box image (base.py:15-19)
            float dx = pbc1(sm.pos[il * 3 + 0] - cpos[(size_t)jl * 3 + 0], hbx);
            float dy = pbc1(sm.pos[il * 3 + 1] - cpos[(size_t)jl * 3 + 1], hby);
            float dz = pbc1(sm.pos[il * 3 + 2] - cpos[(size_t)jl * 3 + 2], hbz);
            v = dx * dx + dy * dy + dz * dz;
            if (v_nd) {   // egcl.py:82-84
              const float inv = 1.f / (sqrtf(v) + 1.f);
              dx *= inv; dy *= inv; dz *= inv;
            }
            sm.pcd[p][0] = dx; sm.pcd[p][1] = dy; sm.pcd[p][2] = dz;
            sm.prow[p] = il;
            sm.pc[p] = (float)(pr >> 27);
          }
        }
        sm.xa[p * WXS + k] = v;
      }
      __syncthreads();
      // edge_nn.0 -> act (xb)
      ik = wide_mm<PREC, 2>(Lp, L, 0, 64 * w, sm.xa, acc, lane, np, BIGK_X0, bigw);
      wide_store_act<2>(acc, Lp + L.be1, 64 * w, sm.xb, lane, act, ik);
      __syncthreads();
      // edge_nn.2 -> act: the messages (xa)
      ik = wide_mm<PREC, 2>(Lp, L, 1, 64 * w, sm.xb, acc, lane, np, BIGK_Y0, bigw);
      wide_store_act<2>(acc, Lp + L.be2, 64 * w, sm.xa, lane, act, ik);
      __syncthreads();
      if (v_att) {   // egcl.py:60-62
        wide_row_dot(sm.xa, Lp + L.watt, sm.pdot, tid);
        __syncthreads();
        if (PREC != PREC_F32 && tid < np && !__builtin_isfinite(sm.pdot[tid])) atomicOr(&sm.err, ENFLOW_ERR_RANGE);
        for (int e = tid; e < 32 * WH; e += BLOCK) {
          const int p = e >> 8, f = e & (WH - 1);
          sm.xa[p * WXS + f] *= sigm_exact(sm.pdot[p] + batt);
        }
        __syncthreads();
      }
      // coord_nn.0 -> act (xb)
      ik = wide_mm<PREC, 2>(Lp, L, 2, 64 * w, sm.xa, acc, lane, np, BIGK_M, bigw);
      wide_store_act<2>(acc, Lp + L.bc1, 64 * w, sm.xb, lane, act, ik);
      {   // message segment sums (egcl.py:65), pair order, thread = feature
        const int f = tid;
        float s = 0.f;
        int cur = sm.prow[0];
        for (int p = 0; p < np; ++p) {
          const int r = sm.prow[p];
          if (r != cur) {
            sm.agg[cur * WAST + f] += s;
            s = 0.f;
            cur = r;
          }
          s = fmaf(sm.pc[p], sm.xa[p * WXS + f], s);
        }
        sm.agg[cur * WAST + f] += s;
      }
      __syncthreads();
      // coord_nn.2, tanh, clamp (egcl.py:35-42, 71-72) and the force sums
      wide_row_dot(sm.xb, Lp + L.wc2, sm.pdot, tid);
      __syncthreads();
      if (tid < 3) {
        for (int p = 0; p < np; ++p) {
          float phi = sm.pdot[p];
          if (PREC != PREC_F32 && !__builtin_isfinite(phi)) atomicOr(&sm.err, ENFLOW_ERR_RANGE);   // before tanh / clamp
          if (v_tanh) phi = tanhf(phi);
          sm.agg[sm.prow[p] * WAST + WH + tid] += sm.pc[p] * clamp100(sm.pcd[p][tid] * phi);
        }
      }
      __syncthreads();
    }
  }

  // vel_scaling_nn (egcl.py:51-54): Q
  for (int e = tid; e < 32 * WIDE_KV; e += BLOCK) {
    const int a = e / WIDE_KV, q = e - a * WIDE_KV;
    sm.xa[a * WXS + q] = q < NFMAX ? sm.h[a * NFP + q] : 0.f;
  }
  __syncthreads();
  ik = wide_mm<PREC, 2>(Lp, L, 4, 64 * w, sm.xa, acc, lane, rb, BIGK_HV, bigw);
  wide_store_act<2>(acc, Lp + L.bv1, 64 * w, sm.xb, lane, act, ik);
  __syncthreads();
  wide_row_dot(sm.xb, Lp + L.wv2, sm.pdot, tid);
  __syncthreads();
  if (tid < 32) sm.Q[tid] = sm.pdot[tid] + Lp[L.misc + 0];
  // node_nn (egcl.py:66-67) on [message sums | h]
  for (int e = tid; e < 32 * WIDE_KN; e += BLOCK) {
    const int a = e / WIDE_KN, k = e - a * WIDE_KN;
    sm.xa[a * WXS + k] = k < WH ? sm.agg[a * WAST + k] : (k - WH < NFMAX ? sm.h[a * NFP + (k - WH)] : 0.f);
  }
  __syncthreads();
  ik = wide_mm<PREC, 2>(Lp, L, 3, 64 * w, sm.xa, acc, lane, rb, BIGK_HA, bigw);
  wide_store_act<2>(acc, Lp + L.bn1, 64 * w, sm.xb, lane, act, ik);
  __syncthreads();
  if (w == 0) {
    f32x16 gacc[1];
    const float ikg = wide_mm<PREC, 1>(Lp, L, 5, 0, sm.xb, gacc, lane, rb, BIGK_NH, bigw);
    const int j = lane & 31, hh = lane >> 5;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int q = rho(r, hh);
      if (q < nf) sm.G[j * NFP + q] = fmaf(gacc[0][r], ikg, Lp[L.bn2 + q]);
    }
  }
  if constexpr (PREC == PREC_F16X3) {   // small-operand guard of the row block (BIGK_*)
    if (lane == 0) atomicOr(&sm.big, bigw | (tot > 0 ? (uint32_t)BIGK_EDGE : 0u) | (uint32_t)BIGK_NODE);
  }
  __syncthreads();
  if constexpr (PREC == PREC_F16X3) {
    if (tid == 0 && small_operands(sm.big)) sm.err |= ENFLOW_ERR_SMALL;
  }
  if (tid == 0 && sm.err) atomicOr(B.err, sm.err);

  float ldj = 0.f;
  for (int a = tid; a < rb; a += BLOCK) {
    const size_t ga = (size_t)(g0 + a);
    const float q = sm.Q[a];
    const float inv = 1.f / fmaxf((float)sm.cntrow[a], 1.f);   // helpers.py:63-70
    float F[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) F[d] = sm.agg[a * WAST + WH + d] * inv * B.cw;
    if constexpr (PREC != PREC_F32) {   // split-precision GEMM out of range (ENFLOW_ERR_RANGE)
      bool bad = !__builtin_isfinite(q) || !__builtin_isfinite(F[0]) || !__builtin_isfinite(F[1]) ||
                 !__builtin_isfinite(F[2]);
      for (int qf = 0; qf < nf; ++qf) bad |= !__builtin_isfinite(sm.G[a * NFP + qf]);
      if (bad) atomicOr(B.err, ENFLOW_ERR_RANGE);
    }
    if (mode == 2) {   // EGCL.forward outputs
      B.Qo[ga] = q;
      for (int d = 0; d < 3; ++d) B.Fo[ga * 3 + d] = F[d];
      for (int qf = 0; qf < nf; ++qf) B.Go[ga * nf + qf] = sm.G[a * NFP + qf];
    } else if (mode == 0) {   // dynamics.py:15-22
      const float eq = expf(q);
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        const float v = eq * B.vel[ga * 3 + d] + F[d] * B.dt;
        B.vel[ga * 3 + d] = v;
        B.pos2[ga * 3 + d] = pbc1(sm.pos[a * 3 + d] + v * B.dt, B.box[ga * 3 + d]);
      }
      for (int qf = 0; qf < nf; ++qf) {
        const float gn = B.g[ga * nf + qf] + sm.G[a * NFP + qf] * B.dt;
        B.g[ga * nf + qf] = gn;
        B.h2[ga * nf + qf] = sm.h[a * NFP + qf] + gn * B.dt;
      }
      ldj += q;
    } else {   // dynamics.py:32-35
      const float eq = expf(q);
      for (int qf = 0; qf < nf; ++qf) B.g[ga * nf + qf] -= sm.G[a * NFP + qf] * B.dt;
#pragma unroll
      for (int d = 0; d < 3; ++d) B.vel[ga * 3 + d] = (B.vel[ga * 3 + d] - F[d] * B.dt) / eq;
      if (mode == 3) ldj -= q;   // vel /= exp(Q)
    }
  }
  if (mode == 0 || mode == 3) {
    const float s = block_sum(sm, ldj);
    if (tid == 0) B.ldj_blk[b] += s;   // fixed layer order: one writer per block and launch
  }
}

// dequantize (forward) per row block at width 256: lg_dequant_kernel on
// argmax_dequant's own LDS image
__global__ void __launch_bounds__(BLOCK) lg_wide_dequant_kernel(LgArgs B, int kind, const float* __restrict__ dq,
                                                                const float* __restrict__ noise, float scale) {
  __shared__ DqSmem<WH, 32, 32> sm;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (b >= B.blk_start[B.num_mols]) return;
  const int m = seg_of(B.blk_start, B.num_mols, b);
  const int a0 = B.mol_ptr[m], n = B.mol_ptr[m + 1] - a0;
  const int r0 = (b - B.blk_start[m]) * B.rbl, rb = min(B.rbl, n - r0);
  const int g0 = a0 + r0, nf = B.nf;
  float lq = 0.f;
  if (kind == ENFLOW_DEQUANT_ARGMAX) {
    for (int e = tid; e < 32 * NFP; e += BLOCK) {
      const int a = e / NFP, q = e - a * NFP;
      sm.h[e] = (a < rb && q < nf) ? B.h[(size_t)(g0 + a) * nf + q] : 0.f;
    }
    __syncthreads();
    lq = argmax_dequant<WH, 32, 32, true>(sm, dq, NoiseSrc{noise, 0, 0}, g0, rb, nf);
    for (int e = tid; e < rb * nf; e += BLOCK) {
      const int a = e / nf, q = e - a * nf;
      B.h[(size_t)g0 * nf + e] = sm.h[a * NFP + q];
    }
  } else if (kind == ENFLOW_DEQUANT_FLOOR) {
    for (int e = tid; e < rb * nf; e += BLOCK) B.h[(size_t)g0 * nf + e] += scale * noise[(size_t)g0 * nf + e];
  }
  const float s = block_sum(sm, lq);
  if (tid == 0) B.ldj_blk[b] = s;
}

// ArgMax.forward alone (argmax.py:13-25) at width 256: blocks of 32 atoms
__global__ void __launch_bounds__(BLOCK) wide_argmax_kernel(int num_atoms, int nf, const float* __restrict__ h,
                                                            const float* __restrict__ dq,
                                                            const float* __restrict__ noise, float* __restrict__ z,
                                                            float* __restrict__ lq_blk) {
  __shared__ DqSmem<WH, 32, 32> sm;
  const int tid = threadIdx.x;
  const int g0 = blockIdx.x * 32, rb = min(32, num_atoms - g0);
  for (int e = tid; e < 32 * NFP; e += BLOCK) {
    const int a = e / NFP, q = e - a * NFP;
    sm.h[e] = (a < rb && q < nf) ? h[(size_t)(g0 + a) * nf + q] : 0.f;
  }
  __syncthreads();
  const float lq = argmax_dequant<WH, 32, 32, true>(sm, dq, NoiseSrc{noise, 0, 0}, g0, rb, nf);
  for (int e = tid; e < rb * nf; e += BLOCK) {
    const int a = e / nf, q = e - a * nf;
    z[(size_t)g0 * nf + e] = sm.h[a * NFP + q];
  }
  const float s = block_sum(sm, lq);
  if (tid == 0) lq_blk[blockIdx.x] = s;
}
// the blocks' log q in block order, in double, plus the batch constant
__global__ void wide_lq_total_kernel(const float* __restrict__ lq_blk, int nblk, double cst, float* __restrict__ total) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double s = cst;
    for (int b = 0; b < nblk; ++b) s += (double)lq_blk[b];
    total[0] = (float)s;
  }
}

// element (f, k) of packed matrix m (wide_mat) from the raw torch-order parameters
__device__ __forceinline__ float wide_weight(const float* __restrict__ raw, const RawEgcl& R, int nf, int m, int f,
                                             int k) {
  switch (m) {
    case 0: {
      const float* row = raw + R.We1 + f * (2 * nf + 1);
      if (k < NFMAX) return k < nf ? row[k] : 0.f;
      if (k < 2 * NFMAX) return (k - NFMAX) < nf ? row[nf + (k - NFMAX)] : 0.f;
      return k == 2 * NFMAX ? row[2 * nf] : 0.f;
    }
    case 1: return raw[R.We2 + f * WH + k];
    case 2: return raw[R.Wc1 + f * WH + k];
    case 3: {
      const float* row = raw + R.Wn1 + f * (WH + nf);
      if (k < WH) return row[nf + k];
      return (k - WH) < nf ? row[k - WH] : 0.f;
    }
    case 4: return k < nf ? raw[R.Wv1 + f * nf + k] : 0.f;
    default: return f < nf ? raw[R.Wn2 + f * WH + k] : 0.f;
  }
}
__device__ __forceinline__ int wide_mat_of(const WideLayout& L, int off) {   // off < L.be1
  return off < L.we2 ? 0 : off < L.wc1 ? 1 : off < L.wn1 ? 2 : off < L.wv1 ? 3 : off < L.wn2 ? 4 : 5;
}

// power-of-two scales of the six matrices (flow_device.h), one workgroup each
__global__ void __launch_bounds__(256) wide_scale_kernel(const float* __restrict__ raw, int nf, float* __restrict__ out) {
  egcl_scales_block(raw, WH, nf, out + wide_layout().scl);
}

// raw (torch order, raw_egcl(256, nf)) + att_nn.0 (weight [256], bias) -> enflow_wide.h's layout;
// after wide_scale_kernel (the split sections read its scales, this kernel leaves them alone)
__global__ void wide_pack_kernel(const float* __restrict__ raw, int nf, int flags, const float* __restrict__ att,
                                 int act_kind, float act_p0, float act_p1, float* __restrict__ out) {
  const WideLayout L = wide_layout();
  const RawEgcl R = raw_egcl(WH, nf);
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= L.total || (idx >= L.scl && idx < L.scl + 16)) return;
  float v = 0.f;
  if (idx < L.be1) {
    const int m = wide_mat_of(L, idx);
    const WideMat M = wide_mat(L, m);
    const int e = idx - M.off;
    v = wide_weight(raw, R, nf, m, e / M.K, e % M.K);
  } else if (idx >= L.x3 && idx < L.x3 + L.be1) {
    const int m = wide_mat_of(L, idx - L.x3);
    const WideMat M = wide_mat(L, m);
    const int half = M.rows * M.K / 2;              // floats of the hi (or lo) part
    int e = idx - L.x3 - M.off;
    const bool lo = e >= half;
    e = 2 * (lo ? e - half : e);                    // first of the word's two elements
    const float sc = out[L.scl + 2 * M.scl];
    const uint32_t bits = f16_split_bits(wide_weight(raw, R, nf, m, e / M.K, e % M.K) * sc,
                                         wide_weight(raw, R, nf, m, (e + 1) / M.K, (e + 1) % M.K) * sc, lo);
    v = __builtin_bit_cast(float, bits);
  } else if (idx >= L.x3) v = 0.f;
  else if (idx < L.be2) v = raw[R.be1 + (idx - L.be1)];
  else if (idx < L.bc1) v = raw[R.be2 + (idx - L.be2)];
  else if (idx < L.wc2) v = raw[R.bc1 + (idx - L.bc1)];
  else if (idx < L.bn1) v = raw[R.wc2 + (idx - L.wc2)];
  else if (idx < L.bv1) v = raw[R.bn1 + (idx - L.bn1)];
  else if (idx < L.wv2) v = raw[R.bv1 + (idx - L.bv1)];
  else if (idx < L.watt) v = raw[R.Wv2 + (idx - L.wv2)];
  else if (idx < L.bn2) v = att ? att[idx - L.watt] : 0.f;
  else if (idx < L.misc) {
    const int q = idx - L.bn2;
    v = q < nf ? raw[R.bn2 + q] : 0.f;
  } else if (idx < L.scl) {
    switch (idx - L.misc) {
      case 0: v = raw[R.bv2]; break;
      case 1: v = att ? att[WH] : 0.f; break;
      case 2: v = (float)(flags & (EGCL_ATTENTION | EGCL_NORM_DIFF | EGCL_TANH)); break;
      case 3: v = (float)act_kind; break;
      case 4: v = act_p0; break;
      case 5: v = act_p1; break;
      default: break;
    }
  }
  out[idx] = v;
}

void lg_wide_layer(int prec, int grid, hipStream_t st, const LgArgs& B, int mode) {
  if (prec == ENFLOW_PREC_F32)
    ENFLOW_TIMED("lg_wide_layer_kernel", st,
                 hipLaunchKernelGGL((lg_wide_layer_kernel<PREC_F32>), dim3(grid), dim3(BLOCK), 0, st, B, mode));
  else   // ENFLOW_PREC_BF16 runs the F16X3 form
    ENFLOW_TIMED("lg_wide_layer_kernel", st,
                 hipLaunchKernelGGL((lg_wide_layer_kernel<PREC_F16X3>), dim3(grid), dim3(BLOCK), 0, st, B, mode));
}
void lg_wide_dequant(int grid, hipStream_t st, const LgArgs& B, int kind, const float* dq, const float* noise,
                     float scale) {
  hipLaunchKernelGGL(lg_wide_dequant_kernel, dim3(grid), dim3(BLOCK), 0, st, B, kind, dq, noise, scale);
}

extern "C" {

int64_t enflow_egcl_wide_packed_size(int hidden_nf, int node_nf) {
  if (hidden_nf != WH || node_nf < 1 || node_nf > NFMAX) return -1;
  return wide_layout().total;
}

int enflow_pack_egcl_wide_f32(const float* raw, int H, int nf, int flags, int act_kind, float act_p0, float act_p1,
                              const float* att, float* packed, void* stream) {
  if (H != WH || nf < 1 || nf > NFMAX || !raw || !packed) return -1;
  if (flags & ~(ENFLOW_EGCL_ATTENTION | ENFLOW_EGCL_NORM_DIFF | ENFLOW_EGCL_TANH | ENFLOW_EGCL_ACT)) return -1;
  if ((flags & EGCL_ATTENTION) && !att) return -1;
  if (act_kind < 0 || act_kind >= ACT_COUNT || ((act_kind != ACT_SILU) != ((flags & ENFLOW_EGCL_ACT) != 0))) return -1;
  const int total = wide_layout().total;
  hipLaunchKernelGGL(wide_scale_kernel, dim3(6), dim3(256), 0, S(stream), raw, nf, packed);
  hipLaunchKernelGGL(wide_pack_kernel, dim3((total + 255) / 256), dim3(256), 0, S(stream), raw, nf, flags,
                     (flags & EGCL_ATTENTION) ? att : nullptr, act_kind, act_p0, act_p1, packed);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int enflow_argmax_forward_wide_f32(int num_atoms, int nf, int H, const float* h, const float* dequant,
                                   const float* noise, float* z, float* log_q_blk, float* log_q, void* stream) {
  if (H != WH || num_atoms < 0 || nf < 1 || nf > NFMAX) return -1;
  if (!dequant || !noise || !log_q || (num_atoms > 0 && (!h || !z || !log_q_blk))) return -1;
  const int nblk = (num_atoms + 31) / 32;
  if (nblk > 0)
    hipLaunchKernelGGL(wide_argmax_kernel, dim3(nblk), dim3(BLOCK), 0, S(stream), num_atoms, nf, h, dequant, noise, z,
                       log_q_blk);
  hipLaunchKernelGGL(wide_lq_total_kernel, dim3(1), dim3(64), 0, S(stream), log_q_blk, nblk,
                     -0.5 * 1.8378770664093453, log_q);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
