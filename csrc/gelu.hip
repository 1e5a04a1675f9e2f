// Exact-erf GELU backward with the column sums of its result, for the
// MLP's fc1 bias gradient.
//
// In the stock backward, GeluBackward writes dgelu [rows, hid] (1.34 GB
// at rows = 32768, hid = 20480) and AddmmBackward's bias gradient reads
// all of it back one kernel later for dgelu.sum(0).  Here the column
// sums accumulate in the pass that produces dgelu, so that second read
// is gone; what is added is a [n_chunks, hid] fp32 partials buffer
// (17 MB at the shape above) and a small final reduction.
//
// Memory-bound: two bf16 streams in, one out, 16-byte vectors.  Each
// thread owns ONE 8-wide vector column and walks the rows of its chunk,
// so its 8 column sums stay in registers; grid = (hid/8/256, chunks).

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "common.h"
#include "gelu_math.h"  // gelu_bwd_one, shared with dropout.hip

namespace {

constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void gelu_bwd_colsum_kernel(
    const ushort8_t* __restrict__ dy, const ushort8_t* __restrict__ x,
    ushort8_t* __restrict__ dx, float* __restrict__ part, int nvec,
    long n_rows, int rows_per_chunk) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long row_end = min(row_begin + rows_per_chunk, n_rows);
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll 4
  for (long r = row_begin; r < row_end; ++r) {
    const long i = r * nvec + vc;
    const ushort8_t dv = dy[i], xv = x[i];
    ushort8_t out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      out[j] = f32_to_bf16(gelu_bwd_one(bf16_to_f32(dv[j]), bf16_to_f32(xv[j])));
      // the sum is over the ROUNDED values: it equals dx.sum(0)
      acc[j] += bf16_to_f32(out[j]);
    }
    dx[i] = out;
  }
  float4* p = reinterpret_cast<float4*>(part + ((long)blockIdx.y * nvec + vc) * 8);
  p[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  p[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
}

// [n_chunks, hid] fp32 partials -> bf16 column sums.  A block owns 32
// columns and splits the chunks over 8 slices that meet in LDS, so
// hid = 20480 gives 640 blocks reading 128-byte row segments.
constexpr int kFinalCols = 32;
constexpr int kFinalSlices = kBlock / kFinalCols;

__global__ __launch_bounds__(kBlock) void gelu_colsum_final_kernel(
    const float* __restrict__ part, unsigned short* __restrict__ out, int hid,
    int n_chunks) {
  __shared__ float s_s[kFinalSlices][kFinalCols];
  const int c = threadIdx.x % kFinalCols;
  const int slice = threadIdx.x / kFinalCols;
  const int col = blockIdx.x * kFinalCols + c;
  float s = 0.f;
  if (col < hid) {
#pragma unroll 4
    for (int ch = slice; ch < n_chunks; ch += kFinalSlices)
      s += part[(long)ch * hid + col];
  }
  s_s[slice][c] = s;
  __syncthreads();
  if (slice == 0 && col < hid) {
#pragma unroll
    for (int k = 1; k < kFinalSlices; ++k) s += s_s[k][c];
    out[col] = f32_to_bf16(s);
  }
}

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
// dy, x: bf16 [rows, hid] contiguous (any leading dims), hid % 8 == 0.
// Returns (dx like dy, colsum bf16 [hid]).
std::vector<torch::Tensor> gelu_bwd_colsum(torch::Tensor dy, torch::Tensor x) {
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.is_contiguous() &&
                  x.is_contiguous(),
              "gelu_bwd_colsum: contiguous GPU tensors");
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              "gelu_bwd_colsum: bf16 only");
  TORCH_CHECK(dy.dim() >= 1 && dy.sizes() == x.sizes(),
              "gelu_bwd_colsum: dy and x must have one shape");
  const long hid = dy.size(-1);
  TORCH_CHECK(hid > 0 && hid % 8 == 0,
              "gelu_bwd_colsum: last dim must be a multiple of 8, got ", hid);
  TORCH_CHECK(hid < (1L << 31), "gelu_bwd_colsum: last dim too large");
  const long n = dy.numel() / hid;
  auto dx = torch::empty_like(dy);
  auto colsum = torch::empty({hid}, dy.options());
  if (n == 0) {
    colsum.zero_();
    return {dx, colsum};
  }
  const int nvec = (int)(hid / 8);
  // row chunking: ~2048 blocks in all (256 CUs x 8), at least 16 rows
  // per chunk so the partials stay small against the tensor itself
  const int grid_x = (nvec + kBlock - 1) / kBlock;
  long n_chunks = std::max(1, 2048 / grid_x);
  long rows_per_chunk = std::max<long>((n + n_chunks - 1) / n_chunks, 16);
  n_chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
  TORCH_CHECK(n_chunks <= 65535, "gelu_bwd_colsum: too many rows");
  auto part = torch::empty({n_chunks, hid},
                           dy.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(gelu_bwd_colsum_kernel, dim3(grid_x, (unsigned)n_chunks),
                     dim3(kBlock), 0, stream, (const ushort8_t*)dy.data_ptr(),
                     (const ushort8_t*)x.data_ptr(), (ushort8_t*)dx.data_ptr(),
                     part.data_ptr<float>(), nvec, n, (int)rows_per_chunk);
  HIP_CHECK_LAST();
  hipLaunchKernelGGL(gelu_colsum_final_kernel,
                     dim3((unsigned)((hid + kFinalCols - 1) / kFinalCols)),
                     dim3(kBlock), 0, stream, part.data_ptr<float>(),
                     (unsigned short*)colsum.data_ptr(), (int)hid,
                     (int)n_chunks);
  HIP_CHECK_LAST();
  return {dx, colsum};
}
#endif  // VITFSDP_KERNELS_ONLY
