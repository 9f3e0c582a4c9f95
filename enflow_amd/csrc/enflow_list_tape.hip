// enflow_list_tape.hip -- the taped instances of enflow_list.h's kernel
// (el_layer_tape_kernel, enflow_egcl_forward_list_tape_f32: the training forward
// of EGCL on a caller-supplied edge list), compiled with ENFLOW_LIST_TAPE in a
// translation unit of its own: the inference instances of enflow_list.hip stay
// the code they were.
#define ENFLOW_LIST_TAPE
#include "enflow_list.h"

extern "C" {

int enflow_egcl_forward_list_tape_f32(int num_nodes, int64_t num_edges, int nf, int H,
                                      const int32_t* row_ptr, const int32_t* col, const float* coord_diff,
                                      const float* h, const float* layer, float cw,
                                      float* Q, float* F, float* G, int32_t* err_flag,
                                      int gemm_precision, float* tape, void* stream) {
  return el_layer_forward(num_nodes, num_edges, nf, H, row_ptr, col, coord_diff, h, layer, cw, Q, F, G, err_flag,
                          gemm_precision, tape, stream);
}

}  // extern "C"
