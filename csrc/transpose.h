// Launcher of csrc/transpose.hip's plain transpose for callers that own
// the destination (csrc/ltgemm.cpp's dgrad_tn writes W^T into its scratch
// buffer), and the grid of its kernels for kernels that move the same
// tiles (csrc/gelu.hip's gelu_fwd_t).
#pragma once

#include <hip/hip_runtime_api.h>

// bf16 x [R, C] contiguous -> y [C, R] contiguous, queued on `stream`.
// The caller guarantees R > 0, C > 0, C % 8 == 0, x 16-byte aligned and
// room for R * C elements at y (16-byte aligned when R % 8 == 0).  Same
// kernel and grid as transpose2d.
void transpose2d_launch(const void* x, void* y, long R, long C,
                        hipStream_t stream, const char* what);

// Grid of the 64 x 64-tile transpose kernels for an [R, C] input.
struct TransposePlan {
  dim3 grid;      // (column tiles, n_chunks)
  int tpb;        // 64-row tiles per block
  long n_chunks;  // grid.y, rows of the column-sum partials
};

// Raises (naming `what`) when the tensor is too large for a grid.
TransposePlan transpose_plan(long R, long C, const char* what);
