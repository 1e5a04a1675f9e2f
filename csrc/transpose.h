// Launcher of csrc/transpose.hip's plain transpose for callers that own
// the destination (csrc/ltgemm.cpp's dgrad_tn writes W^T into its scratch
// buffer).
#pragma once

#include <hip/hip_runtime_api.h>

// bf16 x [R, C] contiguous -> y [C, R] contiguous, queued on `stream`.
// The caller guarantees R > 0, C > 0, C % 8 == 0, x 16-byte aligned and
// room for R * C elements at y (16-byte aligned when R % 8 == 0).  Same
// kernel and grid as transpose2d.
void transpose2d_launch(const void* x, void* y, long R, long C,
                        hipStream_t stream, const char* what);
