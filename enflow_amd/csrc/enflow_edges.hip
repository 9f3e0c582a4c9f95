// enflow_edges.hip -- Data.edges as an explicit list in the reference's own
// order (enflow/data/base.py:122-144), for any molecule size.
//
// The reference lists, per molecule, the hits of torch.nonzero over
// (surviving periodic image k', atom column q): k' ascending -- image shift s
// major, atom minor (helpers.py:17-27) -- then q ascending; both are mapped
// through id_mapping (row = the image's atom, col = id_mapping[q]), equal
// labels are dropped, duplicates from several images are kept.  The pair words
// of lg_pairs_kernel fold those duplicates into multiplicities per (row, col)
// and cannot be reordered afterwards, so the list is built here in two
// traversals around one host read of the edge count:
//
//   lg_images_kernel / lg_idmap_kernel   (enflow_large.hip, unchanged) masks,
//                      id_mapping, bounding boxes
//   el_rows_kernel<0>  one wave per row atom: the hit count of each of its
//                      images, cnt[mol][s][atom] -- the predicates, the
//                      bounding-box culling and the distance test of
//                      lg_pairs_kernel, so the hit set is the flow's
//   el_scan_kernel     one workgroup per molecule: exclusive scan of cnt in
//                      (s, atom) order = the rank of the first edge of every
//                      (image, atom); the molecule's total
//   el_rows_kernel<1>  the same traversal: the hits of (atom, s) in q order at
//                      mol_base + off, by ballot and popcount prefix
//
// Placement is by integer prefix sums only (no atomics): the list is bitwise
// reproducible.  Cross-lane operations (ballot, shuffle) run in wave-uniform
// control flow with every lane active.
#include "enflow_large.h"

struct ElArgs {
  const int32_t* mol_ptr;
  const float* r_cut;
  const float* box;
  const float* pos;
  const uint32_t* mask;     // [A]
  const int32_t* idmap;     // [A]
  const float* aabb;        // [M][6]
  int32_t* cnt;             // per molecule [27][n] at atom offset * 27: hits of (s, atom)
  int64_t* off;             // same layout: rank of the first of them within the molecule
  int64_t* mol_edges;       // [M]
  const int64_t* mol_base;  // [M] first edge of the molecule (fill)
  int64_t num_edges;
  int64_t* row;
  int64_t* col;
  float* cdiff;             // [E][3]
  int32_t* emol;            // [E]
  int32_t* err;
  int num_mols, num_atoms;
};

template <bool FILL>
__global__ void __launch_bounds__(BLOCK) el_rows_kernel(ElArgs E) {
  __shared__ float img[WAVES][27 * 3];   // the row's images, by shift index (per wave)
  const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int a = blockIdx.x * WAVES + w;   // wave-uniform; no block barrier below
  if (a >= E.num_atoms) return;
  const int m = seg_of(E.mol_ptr, E.num_mols, a);
  const int a0 = E.mol_ptr[m], n = E.mol_ptr[m + 1] - a0, il = a - a0;
  const float bx = E.box[(size_t)a0 * 3 + 0], by = E.box[(size_t)a0 * 3 + 1], bz = E.box[(size_t)a0 * 3 + 2];
  const float rc = E.r_cut[m], r_sq = rc * rc;
  const uint64_t lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  float bb[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) bb[k] = E.aabb[(size_t)m * 6 + k];
  const float px = E.pos[(size_t)a * 3 + 0], py = E.pos[(size_t)a * 3 + 1], pz = E.pos[(size_t)a * 3 + 2];
  // lane s < 27 owns image s of the row: surviving, and able to reach the
  // molecule's bounding box at all (lg_pairs_kernel's culling: it only skips
  // images no atom can hit)
  const uint32_t mk = E.mask[a];
  bool cand = false;
  if (lane < 27 && ((mk >> lane) & 1u)) {
    const int s = lane;
    const float ix = px + shift_of(s % 3, bx);
    const float iy = py + shift_of((s / 3) % 3, by);
    const float iz = pz + shift_of(s / 9, bz);
    const float ex = fmaxf(fmaxf(bb[0] - ix, ix - bb[3]), 0.f);
    const float ey = fmaxf(fmaxf(bb[1] - iy, iy - bb[4]), 0.f);
    const float ez = fmaxf(fmaxf(bb[2] - iz, iz - bb[5]), 0.f);
    cand = (ex * ex + ey * ey + ez * ez) <= r_sq * 1.0001f;
    img[w][s * 3 + 0] = ix;
    img[w][s * 3 + 1] = iy;
    img[w][s * 3 + 2] = iz;
  }
  const uint64_t cb = __ballot(cand);
  wave_lds_sync();
  const size_t slot = (size_t)a0 * 27 + (size_t)min(lane, 26) * n + il;
  // count: hits of image `lane` so far; fill: the rank of its next edge
  long long acc = 0;
  if constexpr (FILL) {
    if (cand) acc = E.mol_base[m] + E.off[slot];
  }
  const float hx = bx * 0.5f, hy = by * 0.5f, hz = bz * 0.5f;   // base.py:18
  bool bad = false;
  for (int qc = 0; qc < n; qc += 64) {
    const int q = qc + lane;
    int jl = il;   // lanes past the molecule: never a hit
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (q < n) {
      jl = E.idmap[a0 + q];
      qx = E.pos[(size_t)(a0 + q) * 3 + 0];
      qy = E.pos[(size_t)(a0 + q) * 3 + 1];
      qz = E.pos[(size_t)(a0 + q) * 3 + 2];
    }
    const bool other = jl != il;   // self pair by label (base.py:139)
    float cd[3] = {0.f, 0.f, 0.f};
    if constexpr (FILL) {
      if (other && jl >= 0) {   // pos[row] - pos[col], col = the column's label
        cd[0] = pbc1(px - E.pos[(size_t)(a0 + jl) * 3 + 0], hx);
        cd[1] = pbc1(py - E.pos[(size_t)(a0 + jl) * 3 + 1], hy);
        cd[2] = pbc1(pz - E.pos[(size_t)(a0 + jl) * 3 + 2], hz);
      }
    }
    for (uint64_t rem = cb; rem; rem &= rem - 1) {   // wave-uniform: every lane takes every step
      const int s = __ffsll((unsigned long long)rem) - 1;
      const float dx = img[w][s * 3 + 0] - qx, dy = img[w][s * 3 + 1] - qy, dz = img[w][s * 3 + 2] - qz;
      bool hit = other && (dx * dx + dy * dy + dz * dz < r_sq);
      if (hit && jl < 0) {   // a hit on column q past id_mapping: the reference's IndexError
        bad = true;
        hit = false;
      }
      const uint64_t bal = __ballot(hit);
      if constexpr (FILL) {
        const long long base = __shfl(acc, s, 64);
        const long long e = base + __popcll(bal & lt);
        if (hit && e < E.num_edges) {
          E.row[e] = a;
          E.col[e] = a0 + jl;
          E.cdiff[e * 3 + 0] = cd[0];
          E.cdiff[e * 3 + 1] = cd[1];
          E.cdiff[e * 3 + 2] = cd[2];
          E.emol[e] = m;
        }
      }
      if (lane == s) acc += __popcll(bal);
    }
  }
  if constexpr (!FILL) {
    if (bad) atomicOr(E.err, ENFLOW_ERR_FEW_IMAGES);
    if (lane < 27) E.cnt[slot] = (int32_t)acc;   // 0 for images that did not survive or cannot hit
  }
}

// exclusive scan of the molecule's cnt in (s, atom) order -- its memory order --
// over contiguous chunks per thread; int64, fixed order
__global__ void __launch_bounds__(BLOCK) el_scan_kernel(ElArgs E) {
  __shared__ long long part[BLOCK];
  const int m = blockIdx.x, tid = threadIdx.x;
  const int a0 = E.mol_ptr[m], n = E.mol_ptr[m + 1] - a0;
  const long long len = 27ll * n, per = (len + BLOCK - 1) / BLOCK;
  const long long c0 = min(len, tid * per), c1 = min(len, c0 + per);
  const int32_t* cnt = E.cnt + (size_t)a0 * 27;
  int64_t* off = E.off + (size_t)a0 * 27;
  long long s = 0;
  for (long long e = c0; e < c1; ++e) s += cnt[e];
  part[tid] = s;
  __syncthreads();
  if (tid == 0) {
    long long acc = 0;
    for (int k = 0; k < BLOCK; ++k) { const long long v = part[k]; part[k] = acc; acc += v; }
    E.mol_edges[m] = acc;
  }
  __syncthreads();
  long long acc = part[tid];
  for (long long e = c0; e < c1; ++e) {
    off[e] = acc;
    acc += cnt[e];
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct ElWorkspace { size_t mask, idmap, aabb, cnt, off, total; };
static ElWorkspace el_workspace(int num_mols, int num_atoms) {
  ElWorkspace W;
  const size_t A = (size_t)num_atoms;
  size_t o = 0;
  W.mask = o; o = al256(o + A * 4);
  W.idmap = o; o = al256(o + A * 4);
  W.aabb = o; o = al256(o + (size_t)num_mols * 6 * 4);
  W.cnt = o; o = al256(o + A * 27 * 4);
  W.off = o; o = al256(o + A * 27 * 8);
  W.total = o;
  return W;
}

static ElArgs el_args(int num_mols, int num_atoms, const int32_t* mol_ptr, const float* r_cut, const float* box,
                      const float* pos, void* ws) {
  const ElWorkspace W = el_workspace(num_mols, num_atoms);
  char* base = static_cast<char*>(ws);
  ElArgs E{};
  E.mol_ptr = mol_ptr; E.r_cut = r_cut; E.box = box; E.pos = pos;
  E.mask = reinterpret_cast<uint32_t*>(base + W.mask);
  E.idmap = reinterpret_cast<int32_t*>(base + W.idmap);
  E.aabb = reinterpret_cast<float*>(base + W.aabb);
  E.cnt = reinterpret_cast<int32_t*>(base + W.cnt);
  E.off = reinterpret_cast<int64_t*>(base + W.off);
  E.num_mols = num_mols; E.num_atoms = num_atoms;
  return E;
}

extern "C" {

int64_t enflow_edge_list_workspace_size(int num_mols, int num_atoms) {
  if (num_mols < 0 || num_atoms < 0) return -1;
  return (int64_t)el_workspace(num_mols, num_atoms).total;
}

int enflow_edge_list_count_f32(int num_mols, int num_atoms, const int32_t* mol_ptr, const float* r_cut,
                               const float* box, const float* pos, int64_t* mol_edges, int32_t* err_flag,
                               void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_mols < 0 || num_atoms < 0 || !workspace || !err_flag || !mol_edges) return -1;
  if (workspace_bytes < enflow_edge_list_workspace_size(num_mols, num_atoms)) return -6;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ElArgs E = el_args(num_mols, num_atoms, mol_ptr, r_cut, box, pos, workspace);
  E.mol_edges = mol_edges;
  E.err = err_flag;
  if (num_mols > 0) {
    if (num_atoms > 0) {
      LgArgs B{};   // the fields lg_images_kernel / lg_idmap_kernel read
      B.mol_ptr = mol_ptr; B.r_cut = r_cut; B.box = box;
      B.pos = const_cast<float*>(pos);
      B.nf = 1;
      B.mask = const_cast<uint32_t*>(E.mask);
      B.idmap = const_cast<int32_t*>(E.idmap);
      B.aabb = const_cast<float*>(E.aabb);
      B.err = err_flag;
      B.num_mols = num_mols; B.num_atoms = num_atoms;
      lg_image_maps(st, B);
      ENFLOW_TIMED("el_rows_kernel<count>", st, hipLaunchKernelGGL((el_rows_kernel<false>), dim3((num_atoms + WAVES - 1) / WAVES), dim3(BLOCK), 0, st, E));
    }
    ENFLOW_TIMED("el_scan_kernel", st, hipLaunchKernelGGL(el_scan_kernel, dim3(num_mols), dim3(BLOCK), 0, st, E));
  }
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

int enflow_edge_list_fill_f32(int num_mols, int num_atoms, const int32_t* mol_ptr, const float* r_cut,
                              const float* box, const float* pos, const int64_t* mol_base, int64_t num_edges,
                              int64_t* row, int64_t* col, float* coord_diff, int32_t* edge_mol,
                              void* workspace, int64_t workspace_bytes, void* stream) {
  if (num_mols < 0 || num_atoms < 0 || num_edges < 0 || !workspace) return -1;
  if (num_edges > 0 && (!mol_base || !row || !col || !coord_diff || !edge_mol)) return -1;
  if (workspace_bytes < enflow_edge_list_workspace_size(num_mols, num_atoms)) return -6;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ElArgs E = el_args(num_mols, num_atoms, mol_ptr, r_cut, box, pos, workspace);
  E.mol_base = mol_base;
  E.num_edges = num_edges;
  E.row = row; E.col = col; E.cdiff = coord_diff; E.emol = edge_mol;
  if (num_mols > 0 && num_atoms > 0 && num_edges > 0)
    ENFLOW_TIMED("el_rows_kernel<fill>", st, hipLaunchKernelGGL((el_rows_kernel<true>), dim3((num_atoms + WAVES - 1) / WAVES), dim3(BLOCK), 0, st, E));
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // extern "C"
