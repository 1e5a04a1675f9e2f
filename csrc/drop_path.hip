// Stochastic depth (--drop_path_rate): a per-sample Bernoulli mask on a
// residual branch, with the branch's element dropout folded in.
//
// Sample b of the leading batch dimension is kept iff
// dropout_hash(seed_path, b, 0) >= thresh(p_path): the stateless hash of
// common.h at column 0, so the backward and the checkpoint recompute
// regenerate the mask from one integer and nothing is stored.  The
// element mask, where p_elem > 0, is dropout.hip's bit for bit: keyed on
// the flattened row and the column under seed_elem.
//
//   drop_path_fwd      y = keep_s && keep_e ? x * rscale : 0
//                      (its own adjoint: the backward is the same call)
//   drop_path_add_fwd  out = x + (keep_s && keep_e ? res * rscale : 0)
//
// rscale = 1 / ((1 - p_path) * (1 - p_elem)), computed in double and
// rounded once to fp32, so a kept element sees one multiply and one bf16
// rounding.  Dropped elements are SELECTED (to +0, or to x bit for bit
// in the add form), never multiplied by 0.
//
// The rows of a dropped sample are not loaded at all: the forward writes
// zeros, the add form copies x.  That is the point of fusing the two
// masks: at p_path the branch stream shrinks by that share, where the
// element-dropout kernels next door always read everything.
//
// Layout as in dropout.hip: each thread owns ONE 8-wide vector column
// and walks the rows of its chunk; grid = (C/8/256, row chunks).  A
// chunk's rows are the same for the whole block, so the chunk is cut
// into runs of rows of one sample in scalar registers (one 32-bit
// division at the chunk's first row, none per row) and the keep
// decision is a wave-uniform branch around each run's loads.  Chunks
// straddle sample boundaries freely.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "common.h"

namespace {

constexpr int kBlock = 256;

// x: the branch (forward) or the residual stream (ADD)
// res: the branch (ADD); unused otherwise
template <bool ADD, bool ELEM>
__global__ __launch_bounds__(kBlock) void drop_path_kernel(
    const ushort8_t* __restrict__ x, const ushort8_t* __restrict__ res,
    ushort8_t* __restrict__ out, int nvec, long n_rows, long rows_per_chunk,
    unsigned rows_per_sample, unsigned thresh_path, unsigned seed_path,
    unsigned thresh_elem, unsigned seed_elem, float rscale) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long row_end = min(row_begin + rows_per_chunk, n_rows);
  const unsigned c0 = (unsigned)vc * 8u;
  // rows < 2^32 (host check): the one division is a 32-bit one
  unsigned sample = (unsigned)row_begin / rows_per_sample;
  // the chunk, cut into runs of rows of one sample each
  long r = row_begin;
  long run_end = (long)(sample + 1u) * rows_per_sample;
  while (r < row_end) {
    const long stop = min(run_end, row_end);
    if (dropout_hash(seed_path, sample, 0u) >= thresh_path) {
#pragma unroll 4
      for (; r < stop; ++r) {
        const long i = r * nvec + vc;
        const ushort8_t xv = x[i];
        ushort8_t rv = {};
        if (ADD) rv = res[i];
        ushort8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool keep = !ELEM || dropout_hash(seed_elem, (unsigned)r,
                                                  c0 + j) >= thresh_elem;
          const float xf = bf16_to_f32(xv[j]);
          if (ADD) {
            // a dropped lane hands x through: x + 0 without a rounding
            o[j] = keep ? f32_to_bf16(xf + bf16_to_f32(rv[j]) * rscale)
                        : xv[j];
          } else {
            o[j] = keep ? f32_to_bf16(xf * rscale) : (unsigned short)0;
          }
        }
        out[i] = o;
      }
    } else {
      // dropped sample: the branch's rows are never read
#pragma unroll 4
      for (; r < stop; ++r) {
        const long i = r * nvec + vc;
        out[i] = ADD ? x[i] : ushort8_t{};
      }
    }
    ++sample;
    run_end += rows_per_sample;
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every variant
#define VITFSDP_INSTANTIATE_DROP_PATH(ADD_, ELEM_)                           \
  template __global__ void drop_path_kernel<ADD_, ELEM_>(                    \
      const ushort8_t*, const ushort8_t*, ushort8_t*, int, long, long,       \
      unsigned, unsigned, unsigned, unsigned, unsigned, float);
VITFSDP_INSTANTIATE_DROP_PATH(false, false)
VITFSDP_INSTANTIATE_DROP_PATH(false, true)
VITFSDP_INSTANTIATE_DROP_PATH(true, false)
VITFSDP_INSTANTIATE_DROP_PATH(true, true)
#undef VITFSDP_INSTANTIATE_DROP_PATH
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

// in double, as ops.attention.dropout_mask_reference does
unsigned hash_thresh(double p) {
  const uint64_t t64 = (uint64_t)(p * 4294967296.0);
  return t64 > 4294967295ull ? 4294967295u : (unsigned)t64;
}

// x, res as in drop_path_kernel; res undefined for the one-input op
template <bool ADD>
torch::Tensor launch(const char* op, const torch::Tensor& x,
                     const torch::Tensor& res, long n_samples, double p_path,
                     long seed_path, double p_elem, long seed_elem) {
  check_operand(x, op, "x");
  if (ADD) {
    check_operand(res, op, "res");
    TORCH_CHECK(x.sizes() == res.sizes() && x.device() == res.device(), op,
                ": both operands must have one shape and device");
  }
  TORCH_CHECK(p_path > 0.0 && p_path < 1.0, op,
              ": p_path must be in (0, 1), got ", p_path);
  TORCH_CHECK(p_elem >= 0.0 && p_elem < 1.0, op,
              ": p_elem must be in [0, 1), got ", p_elem);
  TORCH_CHECK(x.dim() >= 1, op, ": needs at least one dim");
  const long C = x.size(-1);
  TORCH_CHECK(C > 0 && C % 8 == 0, op,
              ": last dim must be a multiple of 8, got ", C);
  const long rows = x.numel() / C;
  TORCH_CHECK(C < (1L << 32) && rows < (1L << 32), op,
              ": rows and last dim must each be below 2^32");
  TORCH_CHECK(n_samples >= 1 && rows % n_samples == 0, op,
              ": n_samples must divide the ", rows, " rows, got ", n_samples);
  auto out = torch::empty_like(x);
  if (rows == 0) return out;

  const unsigned rows_per_sample = (unsigned)(rows / n_samples);
  // one rounding: the product of the two keep probabilities in double
  const float rscale = (float)(1.0 / ((1.0 - p_path) * (1.0 - p_elem)));

  const int nvec = (int)(C / 8);
  // row chunking as in dropout.hip: ~8192 blocks in all
  const long grid_x = (nvec + kBlock - 1) / kBlock;
  long n_chunks = std::min<long>(std::max<long>(8192 / grid_x, 1), 65535);
  const long rows_per_chunk = (rows + n_chunks - 1) / n_chunks;
  n_chunks = (rows + rows_per_chunk - 1) / rows_per_chunk;
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kernel = p_elem > 0.0 ? drop_path_kernel<ADD, true>
                             : drop_path_kernel<ADD, false>;
  hipLaunchKernelGGL(
      kernel, dim3((unsigned)grid_x, (unsigned)n_chunks), dim3(kBlock), 0,
      stream, (const ushort8_t*)x.data_ptr(),
      ADD ? (const ushort8_t*)res.data_ptr() : nullptr,
      (ushort8_t*)out.data_ptr(), nvec, rows, rows_per_chunk, rows_per_sample,
      hash_thresh(p_path), (unsigned)seed_path, hash_thresh(p_elem),
      (unsigned)seed_elem, rscale);
  HIP_CHECK_LAST();
  return out;
}

}  // namespace

// Both entry points: bf16 contiguous [..., C], C % 8 == 0, rows = all
// leading dims flattened, n_samples divides rows (row r belongs to
// sample r / (rows / n_samples)), 0 < p_path < 1, 0 <= p_elem < 1.

torch::Tensor drop_path_fwd(torch::Tensor x, long n_samples, double p_path,
                            long seed_path, double p_elem, long seed_elem) {
  return launch<false>("drop_path_fwd", x, torch::Tensor(), n_samples, p_path,
                       seed_path, p_elem, seed_elem);
}

torch::Tensor drop_path_add_fwd(torch::Tensor x, torch::Tensor res,
                                long n_samples, double p_path, long seed_path,
                                double p_elem, long seed_elem) {
  return launch<true>("drop_path_add_fwd", x, res, n_samples, p_path,
                      seed_path, p_elem, seed_elem);
}
#endif  // VITFSDP_KERNELS_ONLY
