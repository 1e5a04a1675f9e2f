// LayerScale (--layer_scale_init): a learnable per-channel vector gamma on
// a residual branch, x + drop_path(gamma * dropout(branch)), with the
// branch's element dropout, the per-sample stochastic-depth mask and the
// residual add folded into the same pass, and dgamma out of the backward's
// one read of dy and branch.
//
// The four factors (gamma[c], element keep, sample keep, the inverse keep
// probabilities) commute, so the whole branch epilogue is one kernel each
// way:
//
//   layer_scale_fwd      y = keep_s && keep_e ? x * gamma[c] * rscale : +0
//   layer_scale_add_fwd  out = keep ? x + res * gamma[c] * rscale : x
//   layer_scale_bwd      dbranch = keep ? dy * gamma[c] * rscale : +0
//                        dgamma[c] = sum_r (keep ? dy * branch : 0) * rscale
//
// keep_s is drop_path.hip's sample mask (dropout_hash(seed_path, sample,
// 0) >= thresh(p_path)), keep_e is dropout.hip's element mask under
// seed_elem, rscale = 1 / ((1 - p_path)(1 - p_elem)) is formed in double
// on the host.  Either probability may be 0: its mask then costs no hash
// (templates ELEM / PATH), and with both off the kernels are a pure
// per-channel scale, which is what eval runs.  All arithmetic is fp32:
// g[c] = gamma[c] * rscale is formed once per thread, a kept element sees
// one multiply (or one multiply-add) and one bf16 rounding.  Dropped
// elements are SELECTED (to +0, to x bit for bit in the add form, out of
// the dgamma sum), never multiplied by 0, and the rows of a dropped
// sample are not loaded at all, in the backward neither dy nor branch:
// a non-finite value under a dropped sample or element reaches no output.
//
// Layout: the row walk of dropout.hip / drop_path.hip.  A thread owns ONE
// 8-wide vector column and walks the rows of its chunk; a chunk is cut
// into runs of rows of one sample in scalar registers, the keep decision
// is a wave-uniform branch around each run's loads.  The thread keeps
// g[8] and, in the backward, its eight dgamma sums in fp32 registers for
// the whole walk, multiplies the sums by rscale once and writes them as
// one row segment of the fp32 partials [n_chunks, C]; colsum_final.h
// folds those in a fixed order.  No atomics, no LDS in the main kernel:
// dgamma repeats bit for bit.
//
// Launch geometry, chosen for E = 5120 (640 vector columns):
//   * kBlock = 128, two waves: 640 = 5 * 128, so no column block is half
//     empty at the model width (256 would leave the third block half
//     idle, 1/6 of all lanes).
//   * Forward: ~8192 blocks in all as in dropout.hip, but at least 4 rows
//     per chunk, the unroll depth.  At [32768, 5120] that is 1561 chunks
//     of 21 rows.
//   * Backward: ~2048 blocks in all and at least 16 rows per chunk, as in
//     gelu.hip, because every chunk costs a row of partials that is
//     written and read again: 409 chunks -> 405 of 81 rows at
//     [32768, 5120], partials 8.3 MB, 1.6 % of the op's 1007 MB (at 8192
//     blocks it would be 6.6 %).  2025 blocks of two waves are 4 waves per
//     SIMD on 256 CUs, all resident in one round.
//   * Resource table (profiles/raw/kernel_resources.txt): the forwards
//     take 32-57 VGPRs and the backward without a path mask 45-56, all at
//     occupancy 8; the backward with a path mask takes 85-86, occupancy
//     5, above the 4 waves per SIMD its grid supplies.  No scratch, no
//     spills anywhere.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "colsum_final.h"
#include "common.h"

// No packed fp32 VALU ops (v_pk_add/mul/fma_f32) in this file's kernels:
// the loops over 8-element vectors below are exactly what the compiler
// pairs into them.  (The host pass does not know the feature.)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "stream_tiles.h"

namespace {

constexpr int kBlock = 128;

enum ScaleOp { kScale = 0, kScaleAdd = 1, kScaleBwd = 2 };

// a: the branch x (kScale), the residual stream x (kScaleAdd), dy (kScaleBwd)
// b: the branch res (kScaleAdd) or branch (kScaleBwd); unused in kScale
// part: fp32 [gridDim.y, 8 * nvec], kScaleBwd only
template <int OP, bool ELEM, bool PATH>
__global__ __launch_bounds__(kBlock) void layer_scale_kernel(
    const ushort8_t* __restrict__ a, const ushort8_t* __restrict__ b,
    const ushort8_t* __restrict__ gamma, ushort8_t* __restrict__ out,
    float* __restrict__ part, int nvec, long n_rows, long rows_per_chunk,
    unsigned rows_per_sample, unsigned thresh_path, unsigned seed_path,
    unsigned thresh_elem, unsigned seed_elem, float rscale) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long chunk_end = row_begin + rows_per_chunk;
  const long row_end = chunk_end < n_rows ? chunk_end : n_rows;
  const unsigned c0 = (unsigned)vc * 8u;

  // gamma times the keep scale, once per thread
  float g[8];
  {
    const ushort8_t gv = gamma[vc];
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = widen(gv[j]) * rscale;
  }
  float acc[8] = {};

  // the chunk, cut into runs of rows of one sample each (one 32-bit
  // division at the chunk's first row: rows < 2^32 by the host check);
  // without a path mask the chunk is one run
  unsigned sample = PATH ? (unsigned)row_begin / rows_per_sample : 0u;
  long run_end = PATH ? (long)(sample + 1u) * rows_per_sample : row_end;
  long r = row_begin;
  while (r < row_end) {
    const long stop = run_end < row_end ? run_end : row_end;
    if (!PATH || hash_keep(seed_path, thresh_path, sample, 0u)) {
#pragma unroll 4
      for (; r < stop; ++r) {
        const long i = r * nvec + vc;
        const ushort8_t av = a[i];
        ushort8_t bv = {};
        if (OP != kScale) bv = b[i];
        ushort8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool keep =
              !ELEM || hash_keep(seed_elem, thresh_elem, (unsigned)r, c0 + j);
          const float af = widen(av[j]);
          if (OP == kScaleAdd) {
            // a dropped lane hands x through: x + 0 without a rounding
            o[j] = keep ? f32_to_bf16(af + widen(bv[j]) * g[j]) : av[j];
          } else {
            o[j] = keep ? f32_to_bf16(af * g[j]) : (unsigned short)0;
          }
          if (OP == kScaleBwd) {
            // bf16 * bf16 is exact in fp32; a dropped lane is left out
            const float t = af * widen(bv[j]);
            acc[j] += keep ? t : 0.f;
          }
        }
        out[i] = o;
      }
    } else {
      // dropped sample: neither operand's rows are read (kScaleAdd
      // copies the stream), nothing is added to the sums
#pragma unroll 4
      for (; r < stop; ++r) {
        const long i = r * nvec + vc;
        out[i] = OP == kScaleAdd ? a[i] : ushort8_t{};
      }
    }
    ++sample;
    run_end += rows_per_sample;
  }

  if (OP == kScaleBwd) {
    // one row segment of the partials: 32-byte aligned (C % 8 == 0)
    float4_t* p = (float4_t*)(part + (long)blockIdx.y * nvec * 8 + c0);
    p[0] = float4_t{acc[0] * rscale, acc[1] * rscale, acc[2] * rscale,
                    acc[3] * rscale};
    p[1] = float4_t{acc[4] * rscale, acc[5] * rscale, acc[6] * rscale,
                    acc[7] * rscale};
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every variant
#define VITFSDP_INSTANTIATE_LAYER_SCALE(OP_, ELEM_, PATH_)                   \
  template __global__ void layer_scale_kernel<OP_, ELEM_, PATH_>(            \
      const ushort8_t*, const ushort8_t*, const ushort8_t*, ushort8_t*,      \
      float*, int, long, long, unsigned, unsigned, unsigned, unsigned,       \
      unsigned, float);
#define VITFSDP_INSTANTIATE_LAYER_SCALE_OP(OP_)                              \
  VITFSDP_INSTANTIATE_LAYER_SCALE(OP_, false, false)                         \
  VITFSDP_INSTANTIATE_LAYER_SCALE(OP_, true, false)                          \
  VITFSDP_INSTANTIATE_LAYER_SCALE(OP_, false, true)                          \
  VITFSDP_INSTANTIATE_LAYER_SCALE(OP_, true, true)
VITFSDP_INSTANTIATE_LAYER_SCALE_OP(kScale)
VITFSDP_INSTANTIATE_LAYER_SCALE_OP(kScaleAdd)
VITFSDP_INSTANTIATE_LAYER_SCALE_OP(kScaleBwd)
#undef VITFSDP_INSTANTIATE_LAYER_SCALE_OP
#undef VITFSDP_INSTANTIATE_LAYER_SCALE
#endif

}  // namespace
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"

namespace {

// a, b as in layer_scale_kernel (b undefined for kScale), named for the
// messages; returns {out} or {dbranch, dgamma}
template <int OP>
std::vector<torch::Tensor> launch(const char* op, const torch::Tensor& a,
                                  const char* a_name, const torch::Tensor& b,
                                  const char* b_name,
                                  const torch::Tensor& gamma, long n_samples,
                                  double p_path, long seed_path, double p_elem,
                                  long seed_elem) {
  check_bf16_operand(a, op, a_name);
  if (OP != kScale) {
    check_bf16_operand(b, op, b_name);
    TORCH_CHECK(a.sizes() == b.sizes() && a.device() == b.device(), op, ": ",
                a_name, " and ", b_name,
                " must have one shape and device");
  }
  TORCH_CHECK(p_path >= 0.0 && p_path < 1.0, op,
              ": p_path must be in [0, 1), got ", p_path);
  TORCH_CHECK(p_elem >= 0.0 && p_elem < 1.0, op,
              ": p_elem must be in [0, 1), got ", p_elem);
  TORCH_CHECK(a.dim() >= 1, op, ": ", a_name, " needs at least one dim");
  const long C = a.size(-1);
  TORCH_CHECK(C > 0 && C % 8 == 0, op, ": last dim of ", a_name,
              " must be a multiple of 8, got ", C);
  check_bf16_operand(gamma, op, "gamma");
  TORCH_CHECK(gamma.dim() == 1 && gamma.size(0) == C &&
                  gamma.device() == a.device(),
              op, ": gamma must have shape [", C, "] on the device of ",
              a_name, ", got ", gamma.sizes());
  const long rows = a.numel() / C;
  TORCH_CHECK(C < (1L << 32) && rows < (1L << 32), op,
              ": rows and last dim of ", a_name,
              " must each be below 2^32");
  // colsum_final.h indexes columns with an int
  TORCH_CHECK(OP != kScaleBwd || C < (1L << 31), op, ": last dim of ", a_name,
              " must be below 2^31 for the column sums");
  TORCH_CHECK(n_samples >= 1 && rows % n_samples == 0, op,
              ": n_samples must divide the ", rows, " rows, got ", n_samples);
  auto out = torch::empty_like(a);
  if (rows == 0) {
    if (OP != kScaleBwd) return {out};
    return {out, torch::zeros({C}, gamma.options())};
  }

  const unsigned rows_per_sample = (unsigned)(rows / n_samples);
  // one rounding: the product of the two keep probabilities in double
  const float rscale = (float)(1.0 / ((1.0 - p_path) * (1.0 - p_elem)));

  const int nvec = (int)(C / 8);
  const long grid_x = (nvec + kBlock - 1) / kBlock;
  // row chunking (file header): ~8192 blocks of at least 4 rows, or for
  // the backward, whose chunks each cost a row of partials, ~2048 blocks
  // of at least 16 rows
  const long target = OP == kScaleBwd ? 2048 : 8192;
  const long min_rows = OP == kScaleBwd ? 16 : 4;
  const auto [n_chunks, rows_per_chunk] =
      chunk_plan(rows, grid_x, target, min_rows);

  torch::Tensor part, dgamma;
  if (OP == kScaleBwd) {
    // every (chunk, column) is written by exactly one thread
    part = torch::empty({n_chunks, C}, a.options().dtype(torch::kFloat32));
    dgamma = torch::empty({C}, gamma.options());
  }
  const bool elem = p_elem > 0.0, path = p_path > 0.0;
  auto kernel =
      elem ? (path ? layer_scale_kernel<OP, true, true>
                   : layer_scale_kernel<OP, true, false>)
           : (path ? layer_scale_kernel<OP, false, true>
                   : layer_scale_kernel<OP, false, false>);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(
      kernel, dim3((unsigned)grid_x, (unsigned)n_chunks), dim3(kBlock), 0,
      stream, (const ushort8_t*)a.data_ptr(),
      OP != kScale ? (const ushort8_t*)b.data_ptr() : nullptr,
      (const ushort8_t*)gamma.data_ptr(), (ushort8_t*)out.data_ptr(),
      OP == kScaleBwd ? part.data_ptr<float>() : nullptr, nvec, rows,
      rows_per_chunk, rows_per_sample, hash_thresh(p_path),
      (unsigned)seed_path, hash_thresh(p_elem), (unsigned)seed_elem, rscale);
  HIP_CHECK_LAST();
  if (OP != kScaleBwd) return {out};
  colsum_finish(part, dgamma, C, n_chunks, stream);
  return {out, dgamma};
}

}  // namespace

// All entry points: bf16 contiguous [..., C], C % 8 == 0, gamma bf16 [C],
// rows = all leading dims flattened, n_samples divides rows (row r belongs
// to sample r / (rows / n_samples)), 0 <= p_path < 1, 0 <= p_elem < 1.

torch::Tensor layer_scale_fwd(torch::Tensor x, torch::Tensor gamma,
                              long n_samples, double p_path, long seed_path,
                              double p_elem, long seed_elem) {
  return launch<kScale>("layer_scale_fwd", x, "x", torch::Tensor(), "", gamma,
                        n_samples, p_path, seed_path, p_elem, seed_elem)[0];
}

torch::Tensor layer_scale_add_fwd(torch::Tensor x, torch::Tensor res,
                                  torch::Tensor gamma, long n_samples,
                                  double p_path, long seed_path, double p_elem,
                                  long seed_elem) {
  return launch<kScaleAdd>("layer_scale_add_fwd", x, "x", res, "res", gamma,
                           n_samples, p_path, seed_path, p_elem,
                           seed_elem)[0];
}

std::vector<torch::Tensor> layer_scale_bwd(torch::Tensor dy,
                                           torch::Tensor branch,
                                           torch::Tensor gamma, long n_samples,
                                           double p_path, long seed_path,
                                           double p_elem, long seed_elem) {
  return launch<kScaleBwd>("layer_scale_bwd", dy, "dy", branch, "branch",
                           gamma, n_samples, p_path, seed_path, p_elem,
                           seed_elem);
}
#endif  // VITFSDP_KERNELS_ONLY
