// Hidden dropout for the MLP, the attention projection and the
// pos-embed, with the mask generated in the kernel.
//
// The mask is the stateless hash of (seed, row, column) the attention
// kernels use (dropout_hash, common.h): element (r, c) of a [rows, C]
// tensor is kept iff dropout_hash(seed, r, c) >= thresh.  The backward
// regenerates it from the seed, so no mask is stored anywhere; at
// rows = 32768, hid = 20480 a bool mask would be 671 MB per site.
//
//   dropout_fwd        y = keep ? x * rscale : 0   (its own adjoint)
//   dropout_add_fwd    out = x + (keep ? res * rscale : 0)
//                      the MLP residual add with fc2's dropout folded in
//   gelu_dropout_fwd   y = keep ? gelu(x) * rscale : 0
//   gelu_dropout_bwd   dx = keep ? gelu'(x) * dy * rscale : 0
//
// gelu_dropout_bwd with the column sums of dx (fc1's bias gradient) and
// dx^T in the same pass is gelu_dropout_bwd_colsum(_t) in gelu.hip, next
// to the p = 0 kernels it shares everything but the element formula
// with; its dx is this file's bit for bit.
//
// Dropped elements are SELECTED to +0 (not multiplied by 0), so a
// non-finite value under a dropped position does not leak; at kept
// positions it propagates.  All arithmetic is fp32 with one bf16
// rounding at the store.
//
// Memory-bound: 16-byte vectors, one or two bf16 streams in and one
// out.  As in gelu.hip each thread owns ONE 8-wide vector column and
// walks the rows of its chunk, so the column half of the hash is
// computed once per thread and the row half once per row;
// grid = (C/8/256, row chunks).

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "common.h"
#include "gelu_math.h"

namespace {

constexpr int kBlock = 256;

enum DropOp { kDrop = 0, kDropAdd = 1, kGeluDrop = 2, kGeluDropBwd = 3 };

// a: x (kDrop, kDropAdd, kGeluDrop) or dy (kGeluDropBwd)
// b: res (kDropAdd) or x (kGeluDropBwd); unused otherwise
template <int OP>
__global__ __launch_bounds__(kBlock) void hidden_dropout_kernel(
    const ushort8_t* __restrict__ a, const ushort8_t* __restrict__ b,
    ushort8_t* __restrict__ out, int nvec, long n_rows, long rows_per_chunk,
    unsigned thresh, float rscale, unsigned seed) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long row_end = min(row_begin + rows_per_chunk, n_rows);
  const unsigned c0 = (unsigned)vc * 8u;
#pragma unroll 4
  for (long r = row_begin; r < row_end; ++r) {
    const long i = r * nvec + vc;
    const ushort8_t av = a[i];
    ushort8_t bv = {};
    if (OP == kDropAdd || OP == kGeluDropBwd) bv = b[i];
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const bool keep = dropout_hash(seed, (unsigned)r, c0 + j) >= thresh;
      const float af = bf16_to_f32(av[j]);
      if (OP == kDrop) {
        o[j] = keep ? f32_to_bf16(af * rscale) : (unsigned short)0;
      } else if (OP == kDropAdd) {
        // a dropped lane hands x through: x + 0 without a rounding step
        o[j] = keep ? f32_to_bf16(af + bf16_to_f32(bv[j]) * rscale) : av[j];
      } else if (OP == kGeluDrop) {
        o[j] = keep ? f32_to_bf16(gelu_erf_f32(af) * rscale)
                    : (unsigned short)0;
      } else {
        o[j] = keep ? f32_to_bf16(
                          gelu_bwd_one(af * rscale, bf16_to_f32(bv[j])))
                    : (unsigned short)0;
      }
    }
    out[i] = o;
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every op
#define VITFSDP_INSTANTIATE_DROPOUT(OP_)                                     \
  template __global__ void hidden_dropout_kernel<OP_>(                       \
      const ushort8_t*, const ushort8_t*, ushort8_t*, int, long, long,       \
      unsigned, float, unsigned);
VITFSDP_INSTANTIATE_DROPOUT(kDrop)
VITFSDP_INSTANTIATE_DROPOUT(kDropAdd)
VITFSDP_INSTANTIATE_DROPOUT(kGeluDrop)
VITFSDP_INSTANTIATE_DROPOUT(kGeluDropBwd)
#undef VITFSDP_INSTANTIATE_DROPOUT
#endif

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

void check_operand(const torch::Tensor& t, const char* op, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), op, ": ", name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, op, ": bf16 only, ", name,
              " is ", t.scalar_type());
}

// a, b as in hidden_dropout_kernel; b undefined for the one-input ops
template <int OP>
torch::Tensor launch(const char* op, const torch::Tensor& a,
                     const torch::Tensor& b, double p, long seed) {
  check_operand(a, op, OP == kGeluDropBwd ? "dy" : "x");
  if (OP == kDropAdd || OP == kGeluDropBwd) {
    check_operand(b, op, OP == kDropAdd ? "res" : "x");
    TORCH_CHECK(a.sizes() == b.sizes() && a.device() == b.device(), op,
                ": both operands must have one shape and device");
  }
  TORCH_CHECK(p > 0.0 && p < 1.0, op, ": p must be in (0, 1), got ", p);
  TORCH_CHECK(a.dim() >= 1, op, ": needs at least one dim");
  const long C = a.size(-1);
  TORCH_CHECK(C > 0 && C % 8 == 0, op,
              ": last dim must be a multiple of 8, got ", C);
  const long rows = a.numel() / C;
  TORCH_CHECK(C < (1L << 32) && rows < (1L << 32), op,
              ": rows and last dim must each be below 2^32");
  auto out = torch::empty_like(a);
  if (rows == 0) return out;

  // in double, as ops.attention.dropout_mask_reference does
  const uint64_t t64 = (uint64_t)(p * 4294967296.0);
  const unsigned thresh = t64 > 4294967295ull ? 4294967295u : (unsigned)t64;
  const float rscale = (float)(1.0 / (1.0 - p));

  const int nvec = (int)(C / 8);
  // row chunking: ~8192 blocks in all, so every CU holds its 8 blocks
  // for several rounds and the tail round is a small share
  const long grid_x = (nvec + kBlock - 1) / kBlock;
  long n_chunks = std::min<long>(std::max<long>(8192 / grid_x, 1), 65535);
  const long rows_per_chunk = (rows + n_chunks - 1) / n_chunks;
  n_chunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      hidden_dropout_kernel<OP>, dim3((unsigned)grid_x, (unsigned)n_chunks),
      dim3(kBlock), 0, stream, (const ushort8_t*)a.data_ptr(),
      b.defined() ? (const ushort8_t*)b.data_ptr() : nullptr,
      (ushort8_t*)out.data_ptr(), nvec, rows, rows_per_chunk, thresh, rscale,
      (unsigned)seed);
  HIP_CHECK_LAST();
  return out;
}

}  // namespace

// All entry points: bf16 contiguous [..., C], C % 8 == 0, rows = all
// leading dims flattened, 0 < p < 1.

torch::Tensor dropout_fwd(torch::Tensor x, double p, long seed) {
  return launch<kDrop>("dropout_fwd", x, torch::Tensor(), p, seed);
}

torch::Tensor dropout_add_fwd(torch::Tensor x, torch::Tensor res, double p,
                              long seed) {
  return launch<kDropAdd>("dropout_add_fwd", x, res, p, seed);
}

torch::Tensor gelu_dropout_fwd(torch::Tensor x, double p, long seed) {
  return launch<kGeluDrop>("gelu_dropout_fwd", x, torch::Tensor(), p, seed);
}

torch::Tensor gelu_dropout_bwd(torch::Tensor dy, torch::Tensor x, double p,
                               long seed) {
  return launch<kGeluDropBwd>("gelu_dropout_bwd", dy, x, p, seed);
}
#endif  // VITFSDP_KERNELS_ONLY
