// bf16 [R, C] -> [C, R] transpose, optionally with the column sums of
// the input (a linear's bias gradient) from the same read.
//
// The weight gradient dW = dY^T X has both operands K-major (tokens are
// the slow dimension); transposed copies turn it into the library's TN
// form, the layout its fastest kernels are written for.  The transpose
// of dY reads every element of dY, so dY.sum(0) rides on it.
//
// Memory-bound: one read and one write of the tensor, 16-byte global
// accesses on both sides.  A block moves 64x64 tiles through 8 KB of
// LDS.  The tile is stored as rows of eight 16-byte slots with slot
// index v ^ (row / 8): the ds_write_b128 of the load phase fills whole
// 128-byte rows, and in the store phase the 8 lanes that assemble one
// 128-byte output row segment (rows 8s..8s+7 for s = 0..7, one column)
// land in 8 different slots, so the 16-bit column reads are free of
// bank conflicts without padding.
//
// Column sums: fp32; a thread sums its 8 rows in row order, adds that to
// its running sum over the block's tiles, the 8 lanes of a column meet
// in a shuffle tree, and the per-block partials [n_chunks, C] go through
// colsum_final_kernel.  Every order is fixed: no atomics.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "colsum_final.h"
#include "common.h"
#ifndef VITFSDP_KERNELS_ONLY
#include "transpose.h"
#endif

namespace {

constexpr int kBlock = 256;
constexpr int kTile = 64;  // rows and columns per tile
constexpr int kSlots = kTile / 8;

template <bool COLSUM>
__global__ __launch_bounds__(kBlock) void transpose_kernel(
    const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
    float* __restrict__ part, long R, long C, int tiles_per_block) {
  __shared__ ushort8_t tile[kTile * kSlots];
  const unsigned short* tile_s = reinterpret_cast<const unsigned short*>(tile);
  const int t = threadIdx.x;
  // load phase: lane -> input row hi + 32k, 16-byte column slot lo;
  // store phase: lane -> input column hi + 32k, 8-row group lo
  const int hi = t >> 3, lo = t & 7;
  const long c0 = (long)blockIdx.x * kTile;
  const bool col_ok = c0 + lo * 8 < C;
  const bool vec_store = (R & 7) == 0;  // output rows 16-byte aligned
  float acc[2] = {0.f, 0.f};

  const long tile_begin = (long)blockIdx.y * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const long r0 = (tile_begin + it) * kTile;
    if (r0 >= R) break;  // block-uniform
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = hi + 32 * k;
      ushort8_t v = {0, 0, 0, 0, 0, 0, 0, 0};  // zeros add nothing to a sum
      if (col_ok && r0 + r < R)
        v = *reinterpret_cast<const ushort8_t*>(x + (r0 + r) * C + c0 + lo * 8);
      tile[r * kSlots + (lo ^ ((r >> 3) & 7))] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = hi + 32 * k;
      const int slot = ((c >> 3) ^ lo) * 8 + (c & 7);
      ushort8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = tile_s[(lo * 8 + j) * kTile + slot];
      if (COLSUM) {
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += bf16_to_f32(o[j]);
        acc[k] += s;
      }
      const long r = r0 + lo * 8;
      if (c0 + c < C && r < R) {
        unsigned short* dst = y + (c0 + c) * R + r;
        if (vec_store) {
          *reinterpret_cast<ushort8_t*>(dst) = o;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (r + j < R) dst[j] = o[j];
        }
      }
    }
    __syncthreads();
  }

  if (COLSUM) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      float s = acc[k];
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      const long c = c0 + hi + 32 * k;
      if (lo == 0 && c < C) part[(long)blockIdx.y * C + c] = s;
    }
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports both variants
template __global__ void transpose_kernel<false>(const unsigned short*,
                                                 unsigned short*, float*, long,
                                                 long, int);
template __global__ void transpose_kernel<true>(const unsigned short*,
                                                unsigned short*, float*, long,
                                                long, int);
#endif

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

// Grid of both kernel variants for an [R, C] input.
struct TransposePlan {
  dim3 grid;
  int tpb;        // 64-row tiles per block
  long n_chunks;  // grid.y, rows of the column-sum partials
};

TransposePlan transpose_plan(long R, long C, const char* what) {
  const long col_tiles = (C + kTile - 1) / kTile;
  const long row_tiles = (R + kTile - 1) / kTile;
  // about 4096 blocks (256 CUs x 8 x 2) before a block takes more than
  // one tile; at most 8, which keeps the partials under 1/1000 of x
  const int tpb =
      (int)std::min<long>(8, std::max<long>(1, row_tiles * col_tiles / 4096));
  const long n_chunks = (row_tiles + tpb - 1) / tpb;
  TORCH_CHECK(n_chunks <= 65535 && col_tiles < (1L << 31), what,
              ": tensor too large");
  return {dim3((unsigned)col_tiles, (unsigned)n_chunks), tpb, n_chunks};
}

}  // namespace

void transpose2d_launch(const void* x, void* y, long R, long C,
                        hipStream_t stream, const char* what) {
  const TransposePlan p = transpose_plan(R, C, what);
  hipLaunchKernelGGL(transpose_kernel<false>, p.grid, dim3(kBlock), 0, stream,
                     (const unsigned short*)x, (unsigned short*)y,
                     (float*)nullptr, R, C, p.tpb);
  HIP_CHECK_LAST();
}

namespace {

// x: bf16 [R, C] contiguous, C % 8 == 0.  Returns {x^T} or {x^T, colsum}.
std::vector<torch::Tensor> transpose_run(const torch::Tensor& x, bool colsum,
                                         const char* what) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2, what, ": 2-D GPU tensor expected");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, what, ": bf16 only");
  TORCH_CHECK(x.is_contiguous(), what,
              ": input must be contiguous (no silent copy)");
  const long R = x.size(0), C = x.size(1);
  TORCH_CHECK(C > 0 && C % 8 == 0, what,
              ": columns must be a multiple of 8, got ", C);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, what,
              ": input must be 16-byte aligned");
  auto y = torch::empty({C, R}, x.options());
  torch::Tensor sums;
  if (colsum) sums = torch::empty({C}, x.options());
  if (R == 0) {
    if (colsum) sums.zero_();
    return colsum ? std::vector<torch::Tensor>{y, sums}
                  : std::vector<torch::Tensor>{y};
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  if (!colsum) {
    transpose2d_launch(x.data_ptr(), y.data_ptr(), R, C, stream, what);
    return {y};
  }
  const TransposePlan p = transpose_plan(R, C, what);
  const long n_chunks = p.n_chunks;
  auto* xp = (const unsigned short*)x.data_ptr();
  auto* yp = (unsigned short*)y.data_ptr();
  auto part = torch::empty({n_chunks, C}, x.options().dtype(torch::kFloat32));
  hipLaunchKernelGGL(transpose_kernel<true>, p.grid, dim3(kBlock), 0, stream,
                     xp, yp, part.data_ptr<float>(), R, C, p.tpb);
  HIP_CHECK_LAST();
  hipLaunchKernelGGL(colsum_final_kernel, colsum_final_grid(C),
                     dim3(kColsumFinalBlock), 0, stream,
                     part.data_ptr<float>(),
                     (unsigned short*)sums.data_ptr(), (int)C, (int)n_chunks);
  HIP_CHECK_LAST();
  return {y, sums};
}

}  // namespace

torch::Tensor transpose2d(torch::Tensor x) {
  return transpose_run(x, false, "transpose2d")[0];
}

std::vector<torch::Tensor> transpose_colsum(torch::Tensor x) {
  return transpose_run(x, true, "transpose_colsum");
}
#endif  // VITFSDP_KERNELS_ONLY
