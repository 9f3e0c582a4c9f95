// enflow_host.h -- host-side helpers shared by the C ABI halves of
// enflow_flow.hip and enflow_backward.hip (and the instance selection of
// enflow_bwd_layer.h).
#pragma once

#include <hip/hip_runtime.h>

static inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
static inline int hid_ok(int H) { return H == 32 || H == 64 || H == 128; }
// the large-system path's inference-only width (enflow_wide.hip)
static inline int wide_ok(int H) { return H == 256; }

// CALL(HH, ...) with the compile-time hidden width HH of a checked H (hid_ok);
// further arguments are passed through
#define DISPATCH_H(H, CALL, ...)                              \
  do {                                                        \
    if (H == 32) { CALL(32, ##__VA_ARGS__); }                 \
    else if (H == 64) { CALL(64, ##__VA_ARGS__); }            \
    else { CALL(128, ##__VA_ARGS__); }                        \
  } while (0)
// CALL(HH, NN, ...): NN = 32 / 64, the LDS image that holds NMAXSEL (<= 64) atoms
#define DISPATCH_HN(H, NMAXSEL, CALL, ...)                    \
  do {                                                        \
    if (NMAXSEL <= 32) DISPATCH_H(H, CALL, 32, ##__VA_ARGS__); \
    else DISPATCH_H(H, CALL, 64, ##__VA_ARGS__);              \
  } while (0)
