// enflow_backward_ldja.hip -- the ENFLOW_BWD_LDJ_ATOMS instances of
// enflow_bwd_layer.h's lf_layer_bwd_kernel and argmax_bwd_kernel
// (lf_layer_bwd_ldja_kernel, argmax_bwd_ldja_kernel: adj_ldj holds one value per
// atom, the backward of LFIntegrator.forward_grad) with their two launchers.  A
// translation unit of its own: the instances of enflow_backward.hip stay the code
// they were.
#define ENFLOW_BACKWARD_TU   // -DENFLOW_STAMPS_BWD stamps these kernels too
#define ENFLOW_BWD_LDJA_TU
#include "enflow_bwd_layer.h"

void launch_layer_bwd_ldja(int H, int nmax, bool big, bool f32b, bool variants, int grid, hipStream_t st,
                           const BwdArgs& A) {
  layer_bwd_launch(H, nmax, big, f32b, variants, grid, st, A);
}

void launch_argmax_bwd_ldja(int H, int nmax, int chunks, hipStream_t st, const int32_t* ptr, int nf, const float* h_data,
                            const float* noise, const float* dequant_raw, const float* adj_h, const float* adj_ldj,
                            float* apre, float* spre, float* anet) {
  argmax_bwd_launch(H, nmax, chunks, st, ptr, nf, h_data, noise, dequant_raw, adj_h, adj_ldj, apre, spre, anet);
}
