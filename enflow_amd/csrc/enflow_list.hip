// enflow_list.hip -- one EGCL layer (enflow/nn/egcl.py:76-92) on an edge list
// the caller supplies: row, col and coord_diff as the reference's EGCL.forward
// reads them from its `edges` argument.  No molecule structure is assumed: an
// edge may join any two nodes of the batch, repeat, be a self loop, and the
// list may come in any order (the host sorts it by row into a CSR).
//
//   el_layer_kernel    one workgroup per block of 32 consecutive rows: the
//                      rows' h in the LDS image, the rows' edges (row_ptr /
//                      col) streamed through the LDS pair buffer in passes of
//                      PC pair words (row | col << 5 | 1 << 27, the row within
//                      the block by binary search over the block's row
//                      offsets), the MFMA edge tiles of the flow kernels
//                      (edge_tiles<..., BIG, LIST>: column nodes' h and the
//                      pairs' coord_diff read from global memory), their
//                      segment sums and node phase, then Q, F, G of the rows.
//
// enflow_list_tape.hip compiles the same kernel (enflow_list.h) with
// ENFLOW_LIST_TAPE as el_layer_tape_kernel, behind
// enflow_egcl_forward_list_tape_f32.  A translation unit of its own, so the
// inference instances here compile to the code they were without it.
//
// Nothing the caller passes is trusted as an index: row_ptr values are clamped
// to [0, num_edges] and made non-decreasing, a col outside [0, num_nodes) gets
// a word of multiplicity 0 (no contribution, no read through it) and leaves
// the row's mean divisor; either sets ENFLOW_ERR_INDEX.  All sums run in a
// fixed order (per-wave head buffers, no float atomics): two launches on the
// same input are bitwise equal.
#include "enflow_list.h"

extern "C" {

int enflow_egcl_forward_list_f32(int num_nodes, int64_t num_edges, int nf, int H,
                                 const int32_t* row_ptr, const int32_t* col, const float* coord_diff,
                                 const float* h, const float* layer, float cw,
                                 float* Q, float* F, float* G, int32_t* err_flag,
                                 int gemm_precision, void* stream) {
  return el_layer_forward(num_nodes, num_edges, nf, H, row_ptr, col, coord_diff, h, layer, cw, Q, F, G, err_flag,
                          gemm_precision, nullptr, stream);
}

}  // extern "C"
