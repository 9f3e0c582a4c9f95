// enflow_bwd_aux.h -- the small kernels around the layer backward: Alchemical_NLL
// backward (whole batch and per molecule), the large-system and edge-list offset /
// column-sum kernels, the reverse-flow adjoints and the per-atom form of a
// per-molecule log|detJ| adjoint.  Included by enflow_backward.hip.
#pragma once
#include "enflow_bwd_layer.h"

// ---------------------------------------------------------------------------
// Alchemical_NLL backward (enflow/flow/loss.py:11-24)
// ---------------------------------------------------------------------------
template <int NMAX>
__global__ void __launch_bounds__(BLOCK) nll_bwd_kernel(const int32_t* mol_ptr, int num_mols, int nf, const float* h,
                                                      const float* g, const float* pos, const float* vel, float kBT,
                                                      float softening, const float* grad_loss, float* ah, float* ag,
                                                      float* apos, float* avel, float* adj_ldj) {
  __shared__ float spos[NMAX * 3];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  const float s = grad_loss ? grad_loss[0] : 1.f;
  const float invM = s / (float)num_mols;
  const float cH = invM / kBT;
  for (int e = tid; e < n * 3; e += BLOCK) {
    spos[e] = pos[(size_t)a0 * 3 + e];
    avel[(size_t)a0 * 3 + e] = cH * vel[(size_t)a0 * 3 + e];    // H = LJ + 0.5 vel^2
  }
  for (int e = tid; e < n * nf; e += BLOCK) {                    // -log_gaussian(h), (g)
    ah[(size_t)a0 * nf + e] = invM * h[(size_t)a0 * nf + e];
    ag[(size_t)a0 * nf + e] = invM * g[(size_t)a0 * nf + e];
  }
  __syncthreads();
  for (int e = tid; e < n * 3; e += BLOCK) {
    const int a = e / 3, d = e - a * 3;
    float f = 0.f;
    for (int b = 0; b < n; ++b) {
      if (b == a) continue;
      const float dx = spos[a * 3] - spos[b * 3], dy = spos[a * 3 + 1] - spos[b * 3 + 1],
                  dz = spos[a * 3 + 2] - spos[b * 3 + 2];
      const float d2 = dx * dx + dy * dy + dz * dz;
      if (d2 == 0.f) continue;                                   // dist_sq != 0 (loss.py:15)
      const float r = d2 + softening, ir = 1.f / r, ir2 = ir * ir, ir4 = ir2 * ir2;
      const float dEdR = 4.f * (-6.f * ir4 * ir2 * ir + 3.f * ir4);
      f += dEdR * 2.f * (spos[a * 3 + d] - spos[b * 3 + d]);
    }
    apos[(size_t)a0 * 3 + e] = cH * f;
  }
  if (m == 0 && tid == 0) adj_ldj[0] = -invM;                    // log_px += ldj
}

// ---------------------------------------------------------------------------
// large systems: pair-row offsets of the row blocks, column-side adjoint sums
// ---------------------------------------------------------------------------
// one workgroup: boff[b] = 32-aligned exclusive prefix of the blocks' pair words,
// total[0] = all rows (the weight-gradient passes' row count)
__device__ __forceinline__ int lg_block_words(const int32_t* mol_ptr, int num_mols, const int32_t* blk_start,
                                              int rbl, const int32_t* npairs, int b) {
  const int m = seg_of(blk_start, num_mols, b);
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  const int r0 = (b - blk_start[m]) * rbl, rb = min(rbl, n - r0);
  int t = 0;
  for (int a = 0; a < rb; ++a) t += npairs[a0 + r0 + a];
  return (t + 31) & ~31;
}
__global__ void __launch_bounds__(BLOCK) lg_bwd_offsets_kernel(const int32_t* mol_ptr, int num_mols,
                                                               const int32_t* blk_start, int rbl,
                                                               const int32_t* npairs, int32_t* boff,
                                                               int32_t* total) {
  __shared__ int part[BLOCK + 1];
  const int tid = threadIdx.x;
  const int nb = blk_start[num_mols];
  const int per = (nb + BLOCK - 1) / BLOCK;
  const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  int s = 0;
  for (int b = b0; b < b1; ++b) s += lg_block_words(mol_ptr, num_mols, blk_start, rbl, npairs, b);
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int k = 0; k < BLOCK; ++k) { const int v = part[k]; part[k] = acc; acc += v; }
    part[BLOCK] = acc;
    total[0] = acc;
  }
  __syncthreads();
  int acc = part[tid];
  for (int b = b0; b < b1; ++b) {
    boff[b] = acc;
    acc += lg_block_words(mol_ptr, num_mols, blk_start, rbl, npairs, b);
  }
}

// partial column sums: thread = column atom q of its molecule, blockIdx.y = a
// chunk of LG_RC rows; the rows' slots of q (smap, coalesced over q) locate the
// pair's column adjoints in colc; rows in increasing order -> deterministic
constexpr int LG_RC = 64;
__global__ void __launch_bounds__(BLOCK) lg_colsum_kernel(const int32_t* mol_ptr, int num_mols, int num_atoms,
                                                          int max_n, const int32_t* smap, const int32_t* rowstart,
                                                          const float* colc, int nf, float* part) {
  const int q = blockIdx.x * BLOCK + threadIdx.x, ch = blockIdx.y;
  if (q >= num_atoms) return;
  const int m = seg_of(mol_ptr, num_mols, q);
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0, ql = q - a0;
  const int i0 = min(n, ch * LG_RC), i1 = min(n, i0 + LG_RC);
  float acc[NFMAX + 3];
#pragma unroll
  for (int k = 0; k < NFMAX + 3; ++k) acc[k] = 0.f;
  for (int i = i0; i < i1; ++i) {
    const int k = smap[(size_t)(a0 + i) * max_n + ql];
    if (k >= 0) {
      const float* c = colc + (size_t)(rowstart[a0 + i] + k) * CSTR;
      for (int f = 0; f < nf; ++f) acc[f] += c[f];
#pragma unroll
      for (int d = 0; d < 3; ++d) acc[NFMAX + d] += c[NFMAX + d];
    }
  }
  float* o = part + ((size_t)ch * num_atoms + q) * CSTR;
#pragma unroll
  for (int k = 0; k < NFMAX + 3; ++k) o[k] = acc[k];
}

// column label c = id_mapping[q] (base.py:137): atom c receives the column sums
// of every q mapped to it, q and chunks in increasing order.  One wave per label:
// the lanes test 64 q at a time, the matches are taken in q order (ballot bits),
// lane k < nf + 3 sums component k
__global__ void __launch_bounds__(BLOCK) lg_colfinal_kernel(const int32_t* mol_ptr, int num_mols, int num_atoms,
                                                            const int32_t* idmap, const float* part, int nch,
                                                            int nf, float* ah, float* apos) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= num_atoms) return;   // wave-uniform
  const int m = seg_of(mol_ptr, num_mols, c);
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0, cl = c - a0;
  const int comp = lane < nf ? lane : (lane >= NFMAX && lane < NFMAX + 3 ? lane : -1);
  float acc = 0.f;
  for (int q0 = 0; q0 < n; q0 += 64) {
    const int q = q0 + lane;
    uint64_t hit = __ballot(q < n && idmap[a0 + q] == cl);
    while (hit) {   // wave-uniform loop over the matches, lowest q first
      const int qq = q0 + __builtin_ctzll(hit);
      hit &= hit - 1;
      if (comp >= 0)
        for (int ch = 0; ch < nch; ++ch) acc += part[((size_t)ch * num_atoms + a0 + qq) * CSTR + comp];
    }
  }
  if (lane < nf) ah[(size_t)c * nf + lane] += acc;
  else if (comp >= 0) apos[(size_t)c * 3 + (lane - NFMAX)] += acc;
}

// ---------------------------------------------------------------------------
// caller-supplied edge list: pair-row offsets of the row blocks, column sums
// ---------------------------------------------------------------------------
// one workgroup: boff[b] = 32-aligned exclusive prefix of the 32-row blocks' edges
// (list_block_offsets: what lf_layer_bwd_kernel<.., LIST> counts itself), total[0]
// = all pair rows.  A row_ptr whose blocks overrun the host's bound prb (a valid
// one cannot: the bound is E + 31 blocks) sets ENFLOW_ERR_INDEX; offsets and total
// are capped at prb and the blocks past it refuse to run.
__global__ void __launch_bounds__(BLOCK) el_bwd_offsets_kernel(const int32_t* row_ptr, int n, int E, long long prb,
                                                               int32_t* boff, int32_t* total, int32_t* err) {
  __shared__ long long part[BLOCK + 1];
  const int tid = threadIdx.x;
  const int nb = (n + 31) / 32;
  const int per = (nb + BLOCK - 1) / BLOCK;
  const int b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
  auto words = [&](int b) {
    int e0;
    bool bad;
    return (long long)((list_block_offsets(row_ptr, n, E, b * 32, nullptr, e0, bad) + 31) & ~31);
  };
  long long s = 0;
  for (int b = b0; b < b1; ++b) s += words(b);
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long acc = 0;
    for (int k = 0; k < BLOCK; ++k) { const long long v = part[k]; part[k] = acc; acc += v; }
    total[0] = (int32_t)(acc < prb ? acc : prb);
    if (acc > prb) atomicOr(err, ENFLOW_ERR_INDEX);
  }
  __syncthreads();
  long long acc = part[tid];
  for (int b = b0; b < b1; ++b) {
    boff[b] = (int32_t)(acc < prb ? acc : prb);
    acc += words(b);
  }
}

// d h[c] += the sum of colc over the edges whose col is c, for any graph.  The
// host supplies the CSC view of the row-sorted list: col_ptr [n + 1] and col_perm
// [E] (edge indices of the sorted list, per column in increasing order).  One
// wave per column: lane = (slot s, feature q), EL_SLOTS slots; slot s adds edges
// k0 + s, k0 + s + EL_SLOTS, .. in that order, then the slots are combined by a
// fixed butterfly: one association whatever the launch, no float atomics.  Neither
// array is trusted: col_ptr is clamped to [0, E] and made non-decreasing, a
// col_perm entry clamped to [0, E); either sets ENFLOW_ERR_INDEX.
constexpr int EL_SLOTS = 64 / NFMAX;
__global__ void __launch_bounds__(BLOCK) el_colsum_kernel(const int32_t* __restrict__ col_ptr,
                                                          const int32_t* __restrict__ col_perm, int n, int E,
                                                          const float* __restrict__ colc, int nf,
                                                          float* __restrict__ ah, int32_t* err) {
  const int lane = threadIdx.x & 63;
  const int c = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (c >= n) return;   // wave-uniform
  const int q = lane % NFMAX, s = lane / NFMAX;
  const int r0 = col_ptr[c], r1 = col_ptr[c + 1];
  const int k0 = min(max(r0, 0), E), k1 = max(min(max(r1, 0), E), k0);
  bool bad = k0 != r0 || k1 != r1;
  float acc = 0.f;
  for (int k = k0 + s; k < k1; k += EL_SLOTS) {
    const int e = col_perm[k];
    const int ec = min(max(e, 0), E - 1);   // k0 < k1 <= E: E >= 1
    bad |= ec != e;
    if (q < nf) acc += colc[(size_t)ec * CSTR + q];
  }
#pragma unroll
  for (int off = NFMAX; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);
  if (s == 0 && q < nf) ah[(size_t)c * nf + q] += acc;
  if (bad) atomicOr(err, ENFLOW_ERR_INDEX);
}

// atom chunks of <= 32 for the per-atom ArgMax backward on large systems
__global__ void __launch_bounds__(BLOCK) chunk_ptr_kernel(int num_atoms, int chunks, int32_t* ptr) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  if (k <= chunks) ptr[k] = min(32 * k, num_atoms);
}

// Alchemical_NLL backward for molecules past 64 atoms: one wave per atom (lanes
// over the molecule's other atoms, fixed butterfly reduction), positions from L2
__global__ void __launch_bounds__(BLOCK) nll_bwd_large_kernel(const int32_t* mol_ptr, int num_mols, int num_atoms,
                                                              int nf, const float* h, const float* g,
                                                              const float* pos, const float* vel, float kBT,
                                                              float softening, const float* grad_loss, float* ah,
                                                              float* ag, float* apos, float* avel,
                                                              float* adj_ldj) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float s = grad_loss ? grad_loss[0] : 1.f;
  const float invM = s / (float)num_mols;
  const float cH = invM / kBT;
  if (a == 0 && lane == 0) adj_ldj[0] = -invM;                   // log_px += ldj
  if (a >= num_atoms) return;                                    // wave-uniform
  const int m = seg_of(mol_ptr, num_mols, a);
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  if (lane < 3) avel[(size_t)a * 3 + lane] = cH * vel[(size_t)a * 3 + lane];   // H = LJ + 0.5 vel^2
  if (lane < nf) {                                               // -log_gaussian(h), (g)
    ah[(size_t)a * nf + lane] = invM * h[(size_t)a * nf + lane];
    ag[(size_t)a * nf + lane] = invM * g[(size_t)a * nf + lane];
  }
  const float px = pos[(size_t)a * 3], py = pos[(size_t)a * 3 + 1], pz = pos[(size_t)a * 3 + 2];
  float fx = 0.f, fy = 0.f, fz = 0.f;
  for (int b = a0 + lane; b < a0 + n; b += 64) {
    if (b == a) continue;
    const float dx = px - pos[(size_t)b * 3], dy = py - pos[(size_t)b * 3 + 1], dz = pz - pos[(size_t)b * 3 + 2];
    const float d2 = dx * dx + dy * dy + dz * dz;
    if (d2 == 0.f) continue;                                     // dist_sq != 0 (loss.py:15)
    const float r = d2 + softening, ir = 1.f / r, ir2 = ir * ir, ir4 = ir2 * ir2;
    const float dEdR = 4.f * (-6.f * ir4 * ir2 * ir + 3.f * ir4);
    fx += dEdR * 2.f * dx;
    fy += dEdR * 2.f * dy;
    fz += dEdR * 2.f * dz;
  }
  fx = wave_sum(fx);
  fy = wave_sum(fy);
  fz = wave_sum(fz);
  if (lane == 0) {
    apos[(size_t)a * 3 + 0] = cH * fx;
    apos[(size_t)a * 3 + 1] = cH * fy;
    apos[(size_t)a * 3 + 2] = cH * fz;
  }
}

// ---------------------------------------------------------------------------
// Per-molecule energies / NLLs backward (Alchemical_NLL.potential_grad,
// .per_molecule_grad): every molecule has its own upstream weight grad_out[m].
// The value is sum_k coef[k] * row_k + const with rows {LJ, sum vel^2, sum h^2,
// sum g^2} (enflow_alchemical_nll_f32's nll_mol), so atom a of molecule m gets
//   apos = w c0 dLJ_m/dpos_a,  avel = 2 w c1 vel_a,  ah = 2 w c2 h_a,  ag = 2 w c3 g_a
// with w = grad_out[m].  NULL ah / ag / avel: the potential (positions only).
// ---------------------------------------------------------------------------
struct NllCoef { float c[4]; };

// dE/d(r^2) of the softened 4 (r^-12 - r^-6), r^2 = d^2 + softening, times 2:
// the factor of (pos_a - pos_b) in dLJ/dpos_a; a d^2 == 0 pair is dropped (loss.py:15)
__device__ __forceinline__ float lj_pair_force(float d2, float softening) {
  if (d2 == 0.f) return 0.f;
  const float r = d2 + softening, ir = 1.f / r, ir2 = ir * ir, ir4 = ir2 * ir2;
  return 8.f * (3.f * ir4 - 6.f * ir4 * ir2 * ir);
}

// molecules of <= NMAX atoms: one workgroup per molecule, positions in LDS.  G
// lanes per atom (the largest power of two with n G <= BLOCK, at most a wave)
// share its partners, b = sub, sub + G, ...; each ordered pair is evaluated once
// and gives the three components; the G lanes are combined by a fixed butterfly
// (they are G consecutive lanes of one wave).  A zero weight writes exact zeros.
template <int NMAX>
__global__ void __launch_bounds__(BLOCK) nll_mol_bwd_kernel(const int32_t* __restrict__ mol_ptr, int nf,
                                                          const float* __restrict__ h, const float* __restrict__ g,
                                                          const float* __restrict__ pos,
                                                          const float* __restrict__ vel, float softening,
                                                          const float* __restrict__ grad_out, NllCoef coef,
                                                          float* __restrict__ ah, float* __restrict__ ag,
                                                          float* __restrict__ apos, float* __restrict__ avel) {
  __shared__ float spos[NMAX * 3];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  if (n < 1 || n > NMAX) return;                                 // (the host's max_mol_atoms bounds n)
  const float w = grad_out[m];
  if (avel) {
    const float cv = 2.f * w * coef.c[1];
    for (int e = tid; e < n * 3; e += BLOCK) avel[(size_t)a0 * 3 + e] = w == 0.f ? 0.f : cv * vel[(size_t)a0 * 3 + e];
  }
  if (ah) {
    const float ch = 2.f * w * coef.c[2];
    for (int e = tid; e < n * nf; e += BLOCK) ah[(size_t)a0 * nf + e] = w == 0.f ? 0.f : ch * h[(size_t)a0 * nf + e];
  }
  if (ag) {
    const float cg = 2.f * w * coef.c[3];
    for (int e = tid; e < n * nf; e += BLOCK) ag[(size_t)a0 * nf + e] = w == 0.f ? 0.f : cg * g[(size_t)a0 * nf + e];
  }
  if (w == 0.f) {                                                // block-uniform
    for (int e = tid; e < n * 3; e += BLOCK) apos[(size_t)a0 * 3 + e] = 0.f;
    return;
  }
  for (int e = tid; e < n * 3; e += BLOCK) spos[e] = pos[(size_t)a0 * 3 + e];
  __syncthreads();
  int G = 64;
  while (G > 1 && n * G > BLOCK) G >>= 1;
  const int a = tid / G, sub = tid - a * G;
  float fx = 0.f, fy = 0.f, fz = 0.f;
  if (a < n) {
    const float px = spos[a * 3], py = spos[a * 3 + 1], pz = spos[a * 3 + 2];
    for (int b = sub; b < n; b += G) {
      const float dx = px - spos[b * 3], dy = py - spos[b * 3 + 1], dz = pz - spos[b * 3 + 2];
      const float f = lj_pair_force(dx * dx + dy * dy + dz * dz, softening);   // b == a: d2 == 0
      fx = fmaf(f, dx, fx);
      fy = fmaf(f, dy, fy);
      fz = fmaf(f, dz, fz);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const float ox = __shfl_xor(fx, off, 64), oy = __shfl_xor(fy, off, 64), oz = __shfl_xor(fz, off, 64);
    if (off < G) { fx += ox; fy += oy; fz += oz; }
  }
  if (a < n && sub == 0) {
    const float cp = w * coef.c[0];
    apos[(size_t)(a0 + a) * 3 + 0] = cp * fx;
    apos[(size_t)(a0 + a) * 3 + 1] = cp * fy;
    apos[(size_t)(a0 + a) * 3 + 2] = cp * fz;
  }
}

// molecules past 256 atoms: one wave per atom (lanes over the molecule's other
// atoms, fixed butterfly reduction), positions from L2
__global__ void __launch_bounds__(BLOCK) nll_mol_bwd_large_kernel(const int32_t* __restrict__ mol_ptr, int num_mols,
                                                                int num_atoms, int nf, const float* __restrict__ h,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ pos,
                                                                const float* __restrict__ vel, float softening,
                                                                const float* __restrict__ grad_out, NllCoef coef,
                                                                float* __restrict__ ah, float* __restrict__ ag,
                                                                float* __restrict__ apos, float* __restrict__ avel) {
  const int lane = threadIdx.x & 63;
  const int a = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (a >= num_atoms) return;                                    // wave-uniform
  const int m = seg_of(mol_ptr, num_mols, a);
  const int a0 = mol_ptr[m], n = mol_ptr[m + 1] - a0;
  const float w = grad_out[m];
  if (avel && lane < 3) avel[(size_t)a * 3 + lane] = w == 0.f ? 0.f : 2.f * w * coef.c[1] * vel[(size_t)a * 3 + lane];
  if (ah)
    for (int q = lane; q < nf; q += 64) ah[(size_t)a * nf + q] = w == 0.f ? 0.f : 2.f * w * coef.c[2] * h[(size_t)a * nf + q];
  if (ag)
    for (int q = lane; q < nf; q += 64) ag[(size_t)a * nf + q] = w == 0.f ? 0.f : 2.f * w * coef.c[3] * g[(size_t)a * nf + q];
  if (w == 0.f) {                                                // wave-uniform
    if (lane < 3) apos[(size_t)a * 3 + lane] = 0.f;
    return;
  }
  const float px = pos[(size_t)a * 3], py = pos[(size_t)a * 3 + 1], pz = pos[(size_t)a * 3 + 2];
  float fx = 0.f, fy = 0.f, fz = 0.f;
  for (int b = a0 + lane; b < a0 + n; b += 64) {
    const float dx = px - pos[(size_t)b * 3], dy = py - pos[(size_t)b * 3 + 1], dz = pz - pos[(size_t)b * 3 + 2];
    const float f = lj_pair_force(dx * dx + dy * dy + dz * dz, softening);     // b == a: d2 == 0
    fx = fmaf(f, dx, fx);
    fy = fmaf(f, dy, fy);
    fz = fmaf(f, dz, fz);
  }
  fx = wave_sum(fx);
  fy = wave_sum(fy);
  fz = wave_sum(fz);
  if (lane == 0) {
    const float cp = w * coef.c[0];
    apos[(size_t)a * 3 + 0] = cp * fx;
    apos[(size_t)a * 3 + 1] = cp * fy;
    apos[(size_t)a * 3 + 2] = cp * fz;
  }
}

// ---------------------------------------------------------------------------
// LFIntegrator.reverse backward (dynamics.py:26-37): the two per-atom halves of
// one reverse layer's adjoint around the EGCL backward (one thread per atom,
// fp32, every atom written by its own thread).  The layer computed, from
// (h, g, x, v):  h' = h - dt g;  x' = pbc(x - dt v);  (Q, F, G) = EGCL(h', x');
// g' = g - dt G;  v' = (v - dt F) exp(-Q);  rev_ldj[mol] -= sum Q.
// ---------------------------------------------------------------------------
// before: the adjoints EGCL's outputs receive, from v' (the state tape), Q (the
// one-layer tape) and the adjoints of g', v' and of the molecule's rev_ldj
__global__ void __launch_bounds__(BLOCK) lf_rev_adj_pre(const int32_t* __restrict__ mol_ptr, int num_mols,
                                                        int num_atoms, int nf, float dt,
                                                        const float* __restrict__ vel_out,
                                                        const float* __restrict__ Q, const float* __restrict__ ag,
                                                        const float* __restrict__ av,
                                                        const float* __restrict__ adj_ldj, float* __restrict__ aQ,
                                                        float* __restrict__ aF, float* __restrict__ aG) {
  const int a = blockIdx.x * BLOCK + threadIdx.x;
  if (a >= num_atoms) return;
  const int m = seg_of(mol_ptr, num_mols, a);
  const float s = -dt * expf(-Q[a]);
  float dot = 0.f;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float w = av[(size_t)a * 3 + d];
    dot += vel_out[(size_t)a * 3 + d] * w;
    aF[(size_t)a * 3 + d] = s * w;
  }
  aQ[a] = -dot - adj_ldj[m];
  for (int q = 0; q < nf; ++q) aG[(size_t)a * nf + q] = -dt * ag[(size_t)a * nf + q];
}

// after: the adjoints of the layer's inputs, in place over those of its outputs
// (dh, dx: what the EGCL backward returned for h', x'; pbc has unit derivative)
__global__ void __launch_bounds__(BLOCK) lf_rev_adj_post(int num_atoms, int nf, float dt,
                                                         const float* __restrict__ Q,
                                                         const float* __restrict__ dh,
                                                         const float* __restrict__ dx, float* __restrict__ ah,
                                                         float* __restrict__ ag, float* __restrict__ ax,
                                                         float* __restrict__ av) {
  const int a = blockIdx.x * BLOCK + threadIdx.x;
  if (a >= num_atoms) return;
  const float e = expf(-Q[a]);
  for (int q = 0; q < nf; ++q) {
    const size_t i = (size_t)a * nf + q;
    const float h = ah[i] + dh[i];
    ah[i] = h;
    ag[i] = ag[i] - dt * h;
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const size_t i = (size_t)a * 3 + d;
    const float x = ax[i] + dx[i];
    ax[i] = x;
    av[i] = e * av[i] - dt * x;
  }
}

// ---------------------------------------------------------------------------
// LFIntegrator.forward_grad: the [num_mols] adjoint of the per-molecule log|detJ|
// as one value per atom (the molecule's, repeated), the form the flow backward
// reads under ENFLOW_BWD_LDJ_ATOMS.  One thread per atom, every atom written by
// its own thread.
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) ldj_mol_to_atoms_kernel(const int32_t* __restrict__ mol_ptr, int num_mols,
                                                                 int num_atoms, const float* __restrict__ adj_mol,
                                                                 float* __restrict__ adj_atoms) {
  const int a = blockIdx.x * BLOCK + threadIdx.x;
  if (a >= num_atoms) return;
  adj_atoms[a] = adj_mol[seg_of(mol_ptr, num_mols, a)];
}
