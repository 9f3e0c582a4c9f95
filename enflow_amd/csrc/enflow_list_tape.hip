// enflow_list_tape.hip -- the taped instances of enflow_list.hip's kernel
// (el_layer_tape_kernel, enflow_egcl_forward_list_tape_f32: the training forward
// of EGCL on a caller-supplied edge list).  The same source, compiled here with
// ENFLOW_LIST_TAPE, in a translation unit of its own: the inference instances
// of enflow_list.hip stay the code they were.
#define ENFLOW_LIST_TAPE
#include "enflow_list.hip"
