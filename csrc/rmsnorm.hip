// RMSNorm forward/backward for CDNA4 (--norm_type rmsnorm):
//
//   y = x * rsqrt(mean(x^2 over D) + eps) * w          (no mean, no beta)
//
// Rows of D bf16 elements, fp32 arithmetic, 16-byte vector loads, one
// 256-thread block per row at a time.  Unlike csrc/layernorm.hip, whose
// second pass re-reads the row through L2, a thread here keeps its share
// of the row PACKED in registers between the statistic and the output:
// 4 VGPRs per ushort8_t, VPT (= vectors per thread, 1..4) of them per
// operand, so 12 VGPRs hold a thread's share of x at D = 5120.  Every
// input is read from memory exactly once, in both directions.  That is
// affordable because RMSNorm has one statistic and one block reduction
// per row where LayerNorm has two, and no dbeta accumulators.
//
// Serves D % 8 == 0 and D <= 8192 (VPT <= 4); the entry points refuse
// anything else and ops/rmsnorm.py routes it to the composition.
//
// Forward (rms_fwd_kernel<VPT, ADD>): load, (ADD: s = bf16(x + res) in
// registers, stored once; the statistic is taken from the rounded s as
// ln_add_fwd_kernel does), sum of squares, one block_sum, normalise from
// the registers.  One block per row: measured at (32768, 5120) against
// the same kernel walking the rows on a persistent grid with gamma held
// in registers, it won by 5-6 % (0.113 against 0.119-0.124 ms at 768 to
// 4096 blocks, add form 0.229 against 0.243-0.257 ms; three alternating
// series, each within 0.3 %), so gamma is read through L2 once per row.
//
// Backward (rms_bwd_kernel<VPT, ADD>): persistent, min(rows, 768) blocks.
// Per row dy and x (and dsum) are loaded once and held packed;
//   g = dy * w, xhat = x * rstd, c = mean(g * xhat), dx = rstd * (g - xhat * c)
// and dy * xhat accumulates into 8 * VPT fp32 registers per thread over
// all the block's rows (thread tid owns vector columns tid + k * 256 in
// every row), in a fixed order without atomics.  The [gridDim.x, D]
// partials are reduced by colsum_final_kernel.
//
// Resources on gfx950 (csrc/tools/check_resources.sh csrc/rmsnorm.hip;
// occ = waves per SIMD; no instantiation uses scratch):
//
//   kernel                       VGPR  occ
//   rms_fwd_kernel<1, false>       18    8
//   rms_fwd_kernel<3, false>       46    8
//   rms_fwd_kernel<3, true>        50    8
//   rms_fwd_kernel<4, false>       52    8
//   rms_fwd_kernel<4, true>        58    8
//   rms_bwd_kernel<1, false>       60    8
//   rms_bwd_kernel<3, false>      116    4
//   rms_bwd_kernel<3, true>       120    4
//   rms_bwd_kernel<4, false>      150    3
//   rms_bwd_kernel<4, true>       154    3
//
// ln_bwd_fused_kernel: 132 / 162 VGPRs at VPT 3 and 160 / 168 at VPT 4,
// 3 waves per SIMD throughout, with dy and x read twice.  Without
// keep_packed() below the backward took 140 / 148 and 174 / 184 VGPRs
// (2 waves per SIMD at VPT 4).  Measured times: profiles/PROFILES.md,
// "RMSNorm".

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "colsum_final.h"
#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / WAVE_SIZE;
constexpr int kMaxVpt = 4;       // D <= 8 * kMaxVpt * kBlock = 8192
constexpr int kBwdBlocks = 768;  // 256 CUs x 3 blocks, as ln_bwd_fused_kernel

// Slot k of thread tid is vector column tid + k * kBlock.  VPT is
// ceil(nvec / kBlock), so only the last slot can lie past the row's end.
template <int VPT>
__device__ __forceinline__ bool slot_in_row(int k, int i, int nvec) {
  return k < VPT - 1 || i < nvec;
}

// Makes the compiler forget what it knows about v's value (an empty
// statement that names v as read and written), so arithmetic on it is not
// shared with arithmetic done before this point.
__device__ __forceinline__ void keep_packed(ushort8_t& v) {
  asm volatile("" : "+v"(v));
}

template <int VPT, bool ADD>
__global__ __launch_bounds__(kBlock) void rms_fwd_kernel(
    const ushort8_t* __restrict__ x, const ushort8_t* __restrict__ res,
    const ushort8_t* __restrict__ w, ushort8_t* __restrict__ sum_out,
    ushort8_t* __restrict__ y, float* __restrict__ rstd_out, int nvec,
    float inv_d, float eps) {
  __shared__ float scratch[kWaves];
  const long row = blockIdx.x;
  const long base = row * nvec;
  ushort8_t wv[VPT], xv[VPT];
  float ss = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (slot_in_row<VPT>(k, i, nvec)) {
      wv[k] = w[i];
      xv[k] = x[base + i];
      if (ADD) {
        const ushort8_t rv = res[base + i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          xv[k][j] = f32_to_bf16(bf16_to_f32(xv[k][j]) + bf16_to_f32(rv[j]));
        sum_out[base + i] = xv[k];
      }
      // ADD: the statistic of the rounded sum, the values normalised below
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = bf16_to_f32(xv[k][j]);
        ss += f * f;
      }
    }
  }
  ss = block_sum<kWaves>(ss, scratch);
  const float rstd = rsqrtf(ss * inv_d + eps);
  if (threadIdx.x == 0) rstd_out[row] = rstd;

#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (slot_in_row<VPT>(k, i, nvec)) {
      ushort8_t out;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        out[j] = f32_to_bf16(bf16_to_f32(xv[k][j]) * rstd *
                             bf16_to_f32(wv[k][j]));
      y[base + i] = out;
    }
  }
}

// dx = rstd * (g - xhat * mean(g * xhat)) (+ dsum when ADD, in fp32
// before the one rounding).  ADD writes it to TWO buffers: the gradients
// of x and res are equal, but the autograd engine must receive distinct
// tensors that it may mutate independently (see ln_add_bwd_dx_kernel).
template <int VPT, bool ADD>
__global__ __launch_bounds__(kBlock) void rms_bwd_kernel(
    const ushort8_t* __restrict__ dy, const ushort8_t* __restrict__ dsum,
    const ushort8_t* __restrict__ x, const ushort8_t* __restrict__ w,
    const float* __restrict__ rstd_in, ushort8_t* __restrict__ dx1,
    ushort8_t* __restrict__ dx2, float* __restrict__ dw_part, int nvec,
    long n_rows, float inv_d) {
  __shared__ float scratch[kWaves];
  float dw_acc[VPT][8];
  ushort8_t wv[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (slot_in_row<VPT>(k, i, nvec)) wv[k] = w[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) dw_acc[k][j] = 0.f;
  }

  for (long row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const long base = row * nvec;
    const float rstd = rstd_in[row];
    ushort8_t dv[VPT], xv[VPT], av[VPT];
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int i = threadIdx.x + k * kBlock;
      if (slot_in_row<VPT>(k, i, nvec)) {
        dv[k] = dy[base + i];
        xv[k] = x[base + i];
        if (ADD) av[k] = dsum[base + i];
      }
    }

    float sgx = 0.f;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int i = threadIdx.x + k * kBlock;
      if (slot_in_row<VPT>(k, i, nvec)) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float g = bf16_to_f32(dv[k][j]) * bf16_to_f32(wv[k][j]);
          sgx += g * (bf16_to_f32(xv[k][j]) * rstd);
        }
      }
    }
    const float c = block_sum<kWaves>(sgx, scratch) * inv_d;

#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      // g and xhat are formed again from the packed row: without this
      // the compiler keeps the fp32 values of the loop above alive across
      // the reduction, 16 VGPRs per slot instead of 8
      keep_packed(dv[k]);
      keep_packed(xv[k]);
      const int i = threadIdx.x + k * kBlock;
      if (slot_in_row<VPT>(k, i, nvec)) {
        ushort8_t out;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dyf = bf16_to_f32(dv[k][j]);
          const float g = dyf * bf16_to_f32(wv[k][j]);
          const float xh = bf16_to_f32(xv[k][j]) * rstd;
          float r = rstd * (g - xh * c);
          if (ADD) r += bf16_to_f32(av[k][j]);
          out[j] = f32_to_bf16(r);
          dw_acc[k][j] += dyf * xh;
        }
        dx1[base + i] = out;
        if (ADD) dx2[base + i] = out;
      }
    }
  }

  const long part_row = (long)blockIdx.x * nvec * 8;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (slot_in_row<VPT>(k, i, nvec)) {
      float4* p = reinterpret_cast<float4*>(dw_part + part_row + (long)i * 8);
      p[0] = make_float4(dw_acc[k][0], dw_acc[k][1], dw_acc[k][2],
                         dw_acc[k][3]);
      p[1] = make_float4(dw_acc[k][4], dw_acc[k][5], dw_acc[k][6],
                         dw_acc[k][7]);
    }
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports the real configs
// (VPT = 3 is D = 5120, VPT = 4 the widest row)
#define VITFSDP_INSTANTIATE_RMS(VPT_, ADD_)                                  \
  template __global__ void rms_fwd_kernel<VPT_, ADD_>(                       \
      const ushort8_t*, const ushort8_t*, const ushort8_t*, ushort8_t*,      \
      ushort8_t*, float*, int, float, float);                                \
  template __global__ void rms_bwd_kernel<VPT_, ADD_>(                       \
      const ushort8_t*, const ushort8_t*, const ushort8_t*,                  \
      const ushort8_t*, const float*, ushort8_t*, ushort8_t*, float*, int,   \
      long, float);
VITFSDP_INSTANTIATE_RMS(1, false)
VITFSDP_INSTANTIATE_RMS(3, false)
VITFSDP_INSTANTIATE_RMS(3, true)
VITFSDP_INSTANTIATE_RMS(4, false)
VITFSDP_INSTANTIATE_RMS(4, true)
#undef VITFSDP_INSTANTIATE_RMS
#endif

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"

namespace {

// Operand checks.  The kernels read raw bf16 / fp32 pointers with sizes
// taken from x alone, so every other operand is checked against x before
// a launch: a wrong dtype would be reinterpreted, a short tensor read
// out of bounds.

// the [rows, D] input that fixes D, the row count and the device
void check_rows_input(const char* fn, const char* name,
                      const torch::Tensor& x) {
  TORCH_CHECK(x.is_cuda(), fn, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", x.scalar_type());
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0 && x.size(-1) % 8 == 0 &&
                  x.size(-1) <= 8 * kMaxVpt * kBlock,
              fn, ": ", name, " must have a last dimension D that is a "
              "positive multiple of 8 and at most ", 8 * kMaxVpt * kBlock,
              ", got shape ", x.sizes());
  TORCH_CHECK(x.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// another [rows, D] bf16 operand: res, dy, dsum
void check_rows_like(const char* fn, const char* name, const torch::Tensor& t,
                     const torch::Tensor& x) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == x.sizes(), fn, ": ", name, " must have shape ",
              x.sizes(), ", got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// gamma: bf16 of D elements
void check_weight(const char* fn, const torch::Tensor& t,
                  const torch::Tensor& x) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), fn,
              ": weight must be a GPU tensor on the device of the other "
              "operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn,
              ": weight must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.numel() == x.size(-1), fn, ": weight must have D = ",
              x.size(-1), " elements, got ", t.numel());
  TORCH_CHECK(t.is_contiguous(), fn, ": weight must be contiguous");
}

// saved rstd: fp32, one per row
void check_rstd(const char* fn, const torch::Tensor& t, const torch::Tensor& x,
                long rows) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), fn,
              ": rstd must be a GPU tensor on the device of the other "
              "operands");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, fn,
              ": rstd must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.numel() == rows, fn, ": rstd must have one element per row (",
              rows, "), got ", t.numel());
  TORCH_CHECK(t.is_contiguous(), fn, ": rstd must be contiguous");
}

// calls f(std::integral_constant<int, VPT>) for the row width
template <typename F>
void with_vpt(int nvec, F&& f) {
  switch ((nvec + kBlock - 1) / kBlock) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    default: f(std::integral_constant<int, 4>{}); break;
  }
}

template <bool ADD>
void launch_fwd(const torch::Tensor& x, const torch::Tensor* res,
                const torch::Tensor& w, torch::Tensor* sum, torch::Tensor& y,
                torch::Tensor& rstd, int d, long n, float eps) {
  const int nvec = d / 8;
  auto stream = at::cuda::getCurrentCUDAStream();
  with_vpt(nvec, [&](auto vpt) {
    hipLaunchKernelGGL(
        (rms_fwd_kernel<decltype(vpt)::value, ADD>), dim3((unsigned)n),
        dim3(kBlock), 0, stream, (const ushort8_t*)x.data_ptr(),
        ADD ? (const ushort8_t*)res->data_ptr() : nullptr,
        (const ushort8_t*)w.data_ptr(),
        ADD ? (ushort8_t*)sum->data_ptr() : nullptr, (ushort8_t*)y.data_ptr(),
        rstd.data_ptr<float>(), nvec, 1.f / d, eps);
  });
  HIP_CHECK_LAST();
}

template <bool ADD>
void launch_bwd(const torch::Tensor& dy, const torch::Tensor* dsum,
                const torch::Tensor& x, const torch::Tensor& w,
                const torch::Tensor& rstd, torch::Tensor& dx1,
                torch::Tensor* dx2, torch::Tensor& dw, int d, long n) {
  const int nvec = d / 8;
  const int n_blocks = (int)std::min<long>(n, kBwdBlocks);
  auto dw_part =
      torch::empty({n_blocks, d}, x.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  with_vpt(nvec, [&](auto vpt) {
    hipLaunchKernelGGL(
        (rms_bwd_kernel<decltype(vpt)::value, ADD>), dim3(n_blocks),
        dim3(kBlock), 0, stream, (const ushort8_t*)dy.data_ptr(),
        ADD ? (const ushort8_t*)dsum->data_ptr() : nullptr,
        (const ushort8_t*)x.data_ptr(), (const ushort8_t*)w.data_ptr(),
        rstd.data_ptr<float>(), (ushort8_t*)dx1.data_ptr(),
        ADD ? (ushort8_t*)dx2->data_ptr() : nullptr,
        dw_part.data_ptr<float>(), nvec, n, 1.f / d);
  });
  HIP_CHECK_LAST();
  colsum_finish(dw_part, dw, d, n_blocks, stream);
}

}  // namespace

std::vector<torch::Tensor> rmsnorm_fwd(torch::Tensor x, torch::Tensor w,
                                       double eps) {
  check_rows_input("rmsnorm_fwd", "x", x);
  check_weight("rmsnorm_fwd", w, x);
  const int d = x.size(-1);
  const long n = x.numel() / d;
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({n}, x.options().dtype(torch::kFloat32));
  if (n == 0) return {y, rstd};  // a zero-sized grid is a launch error
  launch_fwd<false>(x, nullptr, w, nullptr, y, rstd, d, n, (float)eps);
  return {y, rstd};
}

std::vector<torch::Tensor> rmsnorm_add_fwd(torch::Tensor x, torch::Tensor res,
                                           torch::Tensor w, double eps) {
  check_rows_input("rmsnorm_add_fwd", "x", x);
  check_rows_like("rmsnorm_add_fwd", "res", res, x);
  check_weight("rmsnorm_add_fwd", w, x);
  const int d = x.size(-1);
  const long n = x.numel() / d;
  auto sum = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto rstd = torch::empty({n}, x.options().dtype(torch::kFloat32));
  if (n == 0) return {sum, y, rstd};
  launch_fwd<true>(x, &res, w, &sum, y, rstd, d, n, (float)eps);
  return {sum, y, rstd};
}

std::vector<torch::Tensor> rmsnorm_bwd(torch::Tensor dy, torch::Tensor x,
                                       torch::Tensor w, torch::Tensor rstd) {
  check_rows_input("rmsnorm_bwd", "x", x);
  check_rows_like("rmsnorm_bwd", "dy", dy, x);
  check_weight("rmsnorm_bwd", w, x);
  const int d = x.size(-1);
  const long n = x.numel() / d;
  check_rstd("rmsnorm_bwd", rstd, x, n);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty_like(w);
  if (n == 0) {
    dw.zero_();
    return {dx, dw};
  }
  launch_bwd<false>(dy, nullptr, x, w, rstd, dx, nullptr, dw, d, n);
  return {dx, dw};
}

std::vector<torch::Tensor> rmsnorm_add_bwd(torch::Tensor dy,
                                           torch::Tensor dsum,
                                           torch::Tensor sum, torch::Tensor w,
                                           torch::Tensor rstd) {
  check_rows_input("rmsnorm_add_bwd", "sum", sum);
  check_rows_like("rmsnorm_add_bwd", "dy", dy, sum);
  check_rows_like("rmsnorm_add_bwd", "dsum", dsum, sum);
  check_weight("rmsnorm_add_bwd", w, sum);
  const int d = sum.size(-1);
  const long n = sum.numel() / d;
  check_rstd("rmsnorm_add_bwd", rstd, sum, n);
  auto dx1 = torch::empty_like(sum);
  auto dx2 = torch::empty_like(sum);
  auto dw = torch::empty_like(w);
  if (n == 0) {
    dw.zero_();
    return {dx1, dx2, dw};
  }
  launch_bwd<true>(dy, &dsum, sum, w, rstd, dx1, &dx2, dw, d, n);
  return {dx1, dx2, dw};
}

#endif  // VITFSDP_KERNELS_ONLY
