// Final step of a two-stage column sum: [n_chunks, cols] fp32 partials
// -> bf16 column sums, shared by gelu.hip and transpose.hip.  No atomics:
// each output is one fixed-order sum, so results repeat bit for bit.
#pragma once

#include "common.h"

// A block owns 32 columns and splits the chunks over 8 slices that meet
// in LDS, so cols = 20480 gives 640 blocks reading 128-byte row segments.
constexpr int kColsumFinalBlock = 256;
constexpr int kColsumFinalCols = 32;
constexpr int kColsumFinalSlices = kColsumFinalBlock / kColsumFinalCols;

static __global__ __launch_bounds__(kColsumFinalBlock) void colsum_final_kernel(
    const float* __restrict__ part, unsigned short* __restrict__ out, int cols,
    int n_chunks) {
  __shared__ float s_s[kColsumFinalSlices][kColsumFinalCols];
  const int c = threadIdx.x % kColsumFinalCols;
  const int slice = threadIdx.x / kColsumFinalCols;
  const int col = blockIdx.x * kColsumFinalCols + c;
  float s = 0.f;
  if (col < cols) {
#pragma unroll 4
    for (int ch = slice; ch < n_chunks; ch += kColsumFinalSlices)
      s += part[(long)ch * cols + col];
  }
  s_s[slice][c] = s;
  __syncthreads();
  if (slice == 0 && col < cols) {
#pragma unroll
    for (int k = 1; k < kColsumFinalSlices; ++k) s += s_s[k][c];
    out[col] = f32_to_bf16(s);
  }
}

static inline dim3 colsum_final_grid(long cols) {
  return dim3((unsigned)((cols + kColsumFinalCols - 1) / kColsumFinalCols));
}
