// Host side of the streaming kernels' entry points; included where
// VITFSDP_KERNELS_ONLY is not defined.
#pragma once

#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include "colsum_final.h"
#include "common.h"
#include "stream_tiles.h"  // DropArgs

namespace {

inline void check_bf16_operand(const torch::Tensor& t, const char* op,
                               const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), op, ": ", name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": bf16 only, ", name,
              " is ", t.scalar_type());
}

// THE threshold of the hash mask: keep iff hash >= p * 2^32, formed in
// double and saturated, as ops.attention.dropout_mask_reference does.
inline unsigned hash_thresh(double p) {
  const uint64_t t64 = (uint64_t)(p * 4294967296.0);
  return t64 > 4294967295ull ? 4294967295u : (unsigned)t64;
}

// The element mask of `rows` flattened rows at 0 < p < 1.
inline DropArgs drop_args(const char* op, double p, long seed, long rows) {
  TORCH_CHECK(p > 0.0 && p < 1.0, op, ": p must be in (0, 1), got ", p);
  // the hash takes the flattened row as 32 bits
  TORCH_CHECK(rows < (1L << 32), op, ": rows must be below 2^32");
  return {hash_thresh(p), (float)(1.0 / (1.0 - p)), (unsigned)seed};
}

// Row chunks of a walking kernel, grid = (grid_x, n_chunks): about
// target_blocks blocks, at least min_rows rows per chunk.  The plan fixes
// the order of the column sums taken over the chunks.
struct ChunkPlan {
  long n_chunks;
  long rows_per_chunk;
};

inline ChunkPlan chunk_plan(long rows, long grid_x, long target_blocks,
                            long min_rows) {
  long n_chunks = std::max<long>(target_blocks / grid_x, 1);
  const long rows_per_chunk =
      std::max<long>((rows + n_chunks - 1) / n_chunks, min_rows);
  // rows_per_chunk >= rows / n_chunks, so the count below is no larger
  // than the one above: at most target_blocks, far inside grid.y's 65535
  n_chunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
  return {n_chunks, rows_per_chunk};
}

// part: fp32 [n_chunks, cols] -> out: bf16 [cols], in a fixed order
inline void colsum_finish(const torch::Tensor& part, torch::Tensor& out,
                          long cols, long n_chunks, hipStream_t stream) {
  hipLaunchKernelGGL(colsum_final_kernel, colsum_final_grid(cols),
                     dim3(kColsumFinalBlock), 0, stream,
                     part.data_ptr<float>(), (unsigned short*)out.data_ptr(),
                     (int)cols, (int)n_chunks);
  HIP_CHECK_LAST();
}

}  // namespace
