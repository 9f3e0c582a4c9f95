// enflow_bwd_prep.h -- the launches that bracket a training backward: the packing of
// the backward weight section (pack_egcl_bwd_body of enflow_bwd_layer.h as kernels),
// the per-layer pair-row offsets, and the poisoning of the gradients of a backward
// that set its error word.  Included by enflow_backward.hip.
#pragma once
#include "enflow_bwd_layer.h"

__global__ void pack_egcl_bwd_kernel(const float* __restrict__ raw, int H, int nf, float* __restrict__ out) {
  pack_egcl_bwd_body(raw, H, nf, out);
}
// every layer at once: layer blockIdx.y at raw + y raw_stride, out + y stride
__global__ void pack_egcl_bwd_layers_kernel(const float* __restrict__ raw, int64_t raw_stride, int H, int nf,
                                            float* __restrict__ out, int64_t stride) {
  pack_egcl_bwd_body(raw + blockIdx.y * raw_stride, H, nf, out + blockIdx.y * stride);
}

__global__ void __launch_bounds__(256) egcl_bwd_scale_kernel(const float* __restrict__ raw, int H, int nf,
                                                             float* __restrict__ out) {
  egcl_scales_block(raw, H, nf, out + egcl_bwd_layout(H).scl);
}
__global__ void __launch_bounds__(256) egcl_bwd_scale_layers_kernel(const float* __restrict__ raw, int64_t raw_stride,
                                                                    int H, int nf, float* __restrict__ out,
                                                                    int64_t stride) {
  egcl_scales_block(raw + blockIdx.y * raw_stride, H, nf, out + blockIdx.y * stride + egcl_bwd_layout(H).scl);
}

// ---------------------------------------------------------------------------
// per-layer 32-aligned pair row offsets (exclusive scan, one block per layer)
// ---------------------------------------------------------------------------
// A backward whose error word is set leaves NaN in every gradient it produced,
// so an optimizer step that runs before the host reads the (deferred) word
// cannot apply wrong-but-finite updates silently.
__global__ void __launch_bounds__(256) poison_on_err_kernel(const int32_t* __restrict__ err, float* __restrict__ a,
                                                            long long na, float* __restrict__ b, long long nb) {
  if (__builtin_nontemporal_load(err) == 0) return;
  const float nan = __builtin_nanf("");
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < na; i += stride) a[i] = nan;
  if (b)
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += stride) b[i] = nan;
}

__global__ void __launch_bounds__(BLOCK) pair_offsets_kernel(const int32_t* counts, int num_mols, int32_t* offs) {
  __shared__ int wsum[WAVES];
  __shared__ int carry;
  const int l = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int32_t* cnt = counts + (size_t)l * num_mols;
  int32_t* out = offs + (size_t)l * (num_mols + 1);
  if (tid == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < num_mols; base += BLOCK) {
    const int mm = base + tid;
    const int v = mm < num_mols ? ((cnt[mm] + 31) & ~31) : 0;
    const int incl = wave_incl_scan(v);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int pre = carry;
    for (int k = 0; k < w; ++k) pre += wsum[k];
    if (mm < num_mols) out[mm] = pre + incl - v;
    __syncthreads();
    if (tid == BLOCK - 1) carry = pre + incl;
    __syncthreads();
  }
  if (tid == 0) out[num_mols] = carry;
}
