// enflow_backward_ldja.hip -- the ENFLOW_BWD_LDJ_ATOMS instances of
// enflow_backward.hip's lf_layer_bwd_kernel and argmax_bwd_kernel
// (lf_layer_bwd_ldja_kernel, argmax_bwd_ldja_kernel: adj_ldj holds one value per
// atom, the backward of LFIntegrator.forward_grad) with their two launchers.  The
// same source, compiled here with ENFLOW_BWD_LDJA_TU, in a translation unit of its
// own: the instances of enflow_backward.hip stay the code they were.
#define ENFLOW_BWD_LDJA_TU
#include "enflow_backward.hip"
