// RMS QK-norm (--qk_norm --qk_norm_type rmsnorm): RMSNorm over head_dim on
// the q and k slices of the fused qkv projection [B, T, 3, H, D], weight
// only, for every head dim fmha.hip serves (D % 16 == 0, 16..192).  The
// output is again [B, T, 3, H, D] with v copied through bit for bit, so
// fmha_fwd_qkv reads it unchanged.
//
// The scheme is that of qk_norm.hip (a group of lanes owns a row, the row
// lives in registers as packed 16-byte vectors, a lane never changes slice
// or position in its group for the whole walk), with the group's width a
// template parameter:
//
//   * A row belongs to a GROUP of L adjacent lanes.  Lane `sub` of the
//     group holds the 16-byte vectors sub, sub + L, sub + 2L, ... of the
//     row, V of them, so L * V = D / 8 must divide evenly:
//         D % 32 == 0 (32 .. 192):            L = 4, V = D / 32 = 1 .. 6
//         D = 16, 48, 80, 112, 144, 176:      L = 2, V = D / 16 = 1 .. 11
//     The lanes of a group read L * 16 consecutive bytes per load.
//   * A wave holds 64 / L CONSECUTIVE rows of one slice, a workgroup
//     kSliceWaves = 2 waves per slice (waves 0-1 q, 2-3 k and, in the
//     forward, 4-5 v, which only copy).  Geometry<L> below derives rows per
//     wave and per workgroup-iteration from L; the kernels, the row walk
//     and the host's Walk all read them there:
//         L = 4: 16 rows per wave, 32 per iteration;
//         L = 2: 32 rows per wave, 64 per iteration.
//   * RMSNorm has no mean and no bias: ONE reduction per row and one
//     parameter vector per lane in the forward, no dbeta in the backward.
//     The row sum is log2(L) DPP adds inside the quad (xor 1, then xor 2
//     at L = 4); the forward has no LDS and no barrier.
//   * Workgroups walk the rows grid-stride under the cap kBlocks = 512,
//     (token, head) advancing by a precomputed (step_tok, step_h) with one
//     carry.  The backward keeps its share of dw in 8 * V registers.  At
//     the end of the walk the groups of a wave fold by shuffles (xor L ..
//     32), the two waves of a slice meet in LDS, and the workgroup writes
//     one row of the fp32 partials [n_blocks, 2, D] (dwq, dwk).
//     colsum_final.h sums them in a fixed order: no atomics, results
//     repeat bit for bit.
//   * Residency under the cap: 512 workgroups = 2 per CU.  The backward's
//     workgroup is one wave per SIMD, so it needs 2 waves per SIMD, that
//     is at most 256 VGPRs; its widest instantiation (L = 2, V = 11: x, dy
//     and w packed in 3 * 44 registers, dw in 88) takes 234.  The
//     forward's 6 waves need 3 per SIMD for two workgroups per CU, at most
//     168 VGPRs, and take 106 at most.  No instantiation spills or uses
//     scratch (profiles/raw/kernel_resources.txt), and none has to lower
//     the cap.
//
// Arithmetic (fp32 throughout):
//   rstd = rsqrt(sum(x^2) * (1/D) + eps); y = bf16(x * rstd * w);
//   g = dy * w; xhat = x * rstd from the SAVED rstd;
//   dx = bf16(rstd * (g - xhat * mean(g * xhat))); dw = sum dy * xhat.
// Only rstd [B, T, 2, H] is saved.
//
// The backward is IN PLACE: dqkv holds the gradient of the output and
// leaves with the gradient of qkv on slices 0 and 1; slice 2 is neither
// read nor written.  Every lane writes exactly the vectors it has read.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "colsum_final.h"
#include "common.h"

// As in qk_norm.hip: no packed fp32 VALU ops in this file's kernels, and
// therefore builtins instead of the HIP headers' plain-inline functions,
// which would be called per element from a function without the feature.
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "stream_tiles.h"  // widen, lds_barrier

namespace {

constexpr int kSliceWaves = 2;                          // waves per slice
constexpr int kFwdBlock = 3 * kSliceWaves * WAVE_SIZE;  // q, k and v waves
constexpr int kBwdBlock = 2 * kSliceWaves * WAVE_SIZE;  // q and k waves
constexpr int kMinD = 16, kMaxD = 192;

// THE place where the shape of the walk follows from the lanes per row.
template <int L>
struct Geometry {
  static_assert(L == 2 || L == 4, "a group is part of one DPP quad");
  static constexpr int kLanes = L;
  static constexpr int kWaveRows = WAVE_SIZE / L;
  static constexpr int kRowsPerIter = kSliceWaves * kWaveRows;
  // Workgroup cap of the walk: 256 CUs x 2, all resident at once (file
  // header), so no workgroup waits for a second round.
  static constexpr int kBlocks = 512;
};

__device__ __forceinline__ float as_f32(unsigned u) {
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ int as_i32(float f) {
  return __builtin_bit_cast(int, f);
}

// sum over the L lanes of a group; every lane gets the same bits (each
// step adds the same two operands on both sides)
template <int L>
__device__ __forceinline__ float group_sum(float v) {
  // quad_perm [1,0,3,2]
  v += as_f32(__builtin_amdgcn_update_dpp(0, as_i32(v), 0xB1, 0xF, 0xF, true));
  if constexpr (L == 4)  // quad_perm [2,3,0,1]
    v += as_f32(
        __builtin_amdgcn_update_dpp(0, as_i32(v), 0x4E, 0xF, 0xF, true));
  return v;
}

// v of lane ^ off
__device__ __forceinline__ float lane_xor(float v, int lane, int off) {
  return as_f32(__builtin_amdgcn_ds_bpermute((lane ^ off) << 2, as_i32(v)));
}

// Makes the compiler forget what it knows about the packed vectors, so it
// cannot keep their unpacked fp32 copies (2x the registers) alive from one
// pass to the next.  No instruction is emitted.
template <int V>
__device__ __forceinline__ void keep_packed(ushort8_t (&v)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) asm volatile("" : "+v"(v[k]));
}

// Where a lane stands in the walk.  Row r of a slice is (token r / H,
// head r % H); vector offset of its first element in [N, 3, H, D].
template <int L>
struct RowWalk {
  using G = Geometry<L>;
  long tok;
  int h;
  int slice;  // wave-uniform
  int sub;

  __device__ __forceinline__ RowWalk(int heads) {
    const int wave = threadIdx.x / WAVE_SIZE;
    const int lane = threadIdx.x % WAVE_SIZE;
    slice = __builtin_amdgcn_readfirstlane(wave / kSliceWaves);
    sub = lane % L;
    const long r = (long)blockIdx.x * G::kRowsPerIter +
                   (wave % kSliceWaves) * G::kWaveRows + lane / L;
    tok = r / heads;
    h = (int)(r % heads);
  }
  __device__ __forceinline__ void advance(long step_tok, int step_h,
                                          int heads) {
    tok += step_tok;
    h += step_h;
    if (h >= heads) {
      h -= heads;
      ++tok;
    }
  }
  __device__ __forceinline__ long vec_offset(int heads, int nvec) const {
    return ((tok * 3 + slice) * heads + h) * nvec + sub;
  }
  __device__ __forceinline__ long stat_offset(int heads) const {
    return (tok * 2 + slice) * heads + h;
  }
};

template <int L, int V>
__global__ __launch_bounds__(kFwdBlock) void qk_rmsnorm_fwd_kernel(
    const ushort8_t* __restrict__ qkv, const ushort8_t* __restrict__ wq,
    const ushort8_t* __restrict__ wk, ushort8_t* __restrict__ out,
    float* __restrict__ rstd_out, long n_tok, int heads, long n_iters,
    long step_tok, int step_h, float inv_d, float eps) {
  constexpr int nvec = V * L;
  RowWalk<L> at(heads);

  if (at.slice == 2) {  // v: bit-for-bit copy
    for (long it = blockIdx.x; it < n_iters; it += gridDim.x) {
      if (at.tok < n_tok) {
        const long o = at.vec_offset(heads, nvec);
        ushort8_t xv[V];
#pragma unroll
        for (int k = 0; k < V; ++k) xv[k] = qkv[o + k * L];
#pragma unroll
        for (int k = 0; k < V; ++k) out[o + k * L] = xv[k];
      }
      at.advance(step_tok, step_h, heads);
    }
    return;
  }

  const ushort8_t* __restrict__ w = at.slice ? wk : wq;
  ushort8_t wv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) wv[k] = w[at.sub + k * L];

  for (long it = blockIdx.x; it < n_iters; it += gridDim.x) {
    // a group is live or not as a whole; the DPP adds stay inside it
    const bool live = at.tok < n_tok;
    const long o = at.vec_offset(heads, nvec);
    ushort8_t xv[V] = {};
    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) xv[k] = qkv[o + k * L];
    }
    keep_packed(wv);

    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = widen(xv[k][j]);
        ss += x * x;
      }
    const float rstd = __builtin_amdgcn_rsqf(group_sum<L>(ss) * inv_d + eps);
    keep_packed(xv);

    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        ushort8_t y;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          y[j] = f32_to_bf16(widen(xv[k][j]) * rstd * widen(wv[k][j]));
        out[o + k * L] = y;
      }
      if (at.sub == 0) rstd_out[at.stat_offset(heads)] = rstd;
    }
    at.advance(step_tok, step_h, heads);
  }
}

template <int L, int V>
__global__ __launch_bounds__(kBwdBlock) void qk_rmsnorm_bwd_kernel(
    ushort8_t* __restrict__ dqkv, const ushort8_t* __restrict__ qkv,
    const ushort8_t* __restrict__ wq, const ushort8_t* __restrict__ wk,
    const float* __restrict__ rstd_in, float* __restrict__ part, long n_tok,
    int heads, long n_iters, long step_tok, int step_h, float inv_d) {
  constexpr int nvec = V * L;
  constexpr int d = nvec * 8;
  // [wave][column]: the wave totals of the final fold
  __shared__ float fold[2 * kSliceWaves][d];
  RowWalk<L> at(heads);

  const ushort8_t* __restrict__ w = at.slice ? wk : wq;
  ushort8_t wv[V];
  float dw_acc[V][8];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    wv[k] = w[at.sub + k * L];
#pragma unroll
    for (int j = 0; j < 8; ++j) dw_acc[k][j] = 0.f;
  }

  for (long it = blockIdx.x; it < n_iters; it += gridDim.x) {
    const bool live = at.tok < n_tok;
    const long o = at.vec_offset(heads, nvec);
    ushort8_t xv[V] = {}, dv[V] = {};
    float rstd = 0.f;
    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        xv[k] = qkv[o + k * L];
        dv[k] = dqkv[o + k * L];
      }
      rstd = rstd_in[at.stat_offset(heads)];
    }
    keep_packed(wv);

    float sgx = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = widen(dv[k][j]) * widen(wv[k][j]);
        sgx += g * (widen(xv[k][j]) * rstd);
      }
    sgx = group_sum<L>(sgx) * inv_d;
    keep_packed(xv);
    keep_packed(dv);
    keep_packed(wv);

    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        ushort8_t dx;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dyf = widen(dv[k][j]);
          const float g = dyf * widen(wv[k][j]);
          const float xh = widen(xv[k][j]) * rstd;
          dx[j] = f32_to_bf16(rstd * (g - xh * sgx));
          dw_acc[k][j] += dyf * xh;
        }
        dqkv[o + k * L] = dx;
      }
    }
    at.advance(step_tok, step_h, heads);
  }

  // the groups of the wave: lanes with equal `sub` hold the same columns,
  // so xor L .. 32 leaves every lane with the wave's totals
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
#pragma unroll
  for (int off = L; off < WAVE_SIZE; off <<= 1)
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        dw_acc[k][j] += lane_xor(dw_acc[k][j], lane, off);
  if (lane < L) {
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j)
        fold[wave][(lane + k * L) * 8 + j] = dw_acc[k][j];
  }
  lds_barrier();
  // one row [2, D] of the partials: dwq, dwk
  float* prow = part + (long)blockIdx.x * 2 * d;
  for (int i = threadIdx.x; i < 2 * d; i += kBwdBlock) {
    const int w0 = (i / d) * kSliceWaves, col = i % d;
    float t = fold[w0][col];
#pragma unroll
    for (int u = 1; u < kSliceWaves; ++u) t += fold[w0 + u][col];
    prow[i] = t;
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every head dim
#define VITFSDP_INSTANTIATE_QK_RMSNORM(L_, V_)                               \
  template __global__ void qk_rmsnorm_fwd_kernel<L_, V_>(                    \
      const ushort8_t*, const ushort8_t*, const ushort8_t*, ushort8_t*,      \
      float*, long, int, long, long, int, float, float);                     \
  template __global__ void qk_rmsnorm_bwd_kernel<L_, V_>(                    \
      ushort8_t*, const ushort8_t*, const ushort8_t*, const ushort8_t*,      \
      const float*, float*, long, int, long, long, int, float);
VITFSDP_INSTANTIATE_QK_RMSNORM(4, 1)
VITFSDP_INSTANTIATE_QK_RMSNORM(4, 2)
VITFSDP_INSTANTIATE_QK_RMSNORM(4, 3)
VITFSDP_INSTANTIATE_QK_RMSNORM(4, 4)
VITFSDP_INSTANTIATE_QK_RMSNORM(4, 5)
VITFSDP_INSTANTIATE_QK_RMSNORM(4, 6)
VITFSDP_INSTANTIATE_QK_RMSNORM(2, 1)
VITFSDP_INSTANTIATE_QK_RMSNORM(2, 3)
VITFSDP_INSTANTIATE_QK_RMSNORM(2, 5)
VITFSDP_INSTANTIATE_QK_RMSNORM(2, 7)
VITFSDP_INSTANTIATE_QK_RMSNORM(2, 9)
VITFSDP_INSTANTIATE_QK_RMSNORM(2, 11)
#undef VITFSDP_INSTANTIATE_QK_RMSNORM
#endif

}  // namespace
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"

namespace {

// Operand checks, as in qk_norm.hip: the kernels read raw pointers with
// every size taken from qkv, so each other operand is checked against it.

// the [B, T, 3, H, D] tensor that fixes the sizes and the device
void check_qkv(const char* fn, const char* name, const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 5 && t.size(2) == 3 && t.size(3) > 0, fn, ": ", name,
              " must have shape [B, T, 3, H, D], got ", t.sizes());
  const long d = t.size(4);
  TORCH_CHECK(d >= kMinD && d <= kMaxD && d % 16 == 0, fn,
              ": head dim D must be a multiple of 16 in [16, 192], got ", d);
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

void check_qkv_like(const char* fn, const char* name, const torch::Tensor& t,
                    const torch::Tensor& qkv) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == qkv.sizes(), fn, ": ", name, " must have shape ",
              qkv.sizes(), ", got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// weight: bf16 [D]
void check_weight(const char* fn, const char* name, const torch::Tensor& t,
                  const torch::Tensor& qkv) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 1 && t.size(0) == qkv.size(4), fn, ": ", name,
              " must have shape [", qkv.size(4), "], got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// saved rstd: fp32 [B, T, 2, H]
void check_stat(const char* fn, const char* name, const torch::Tensor& t,
                const torch::Tensor& qkv) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, fn, ": ", name,
              " must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 4 && t.size(0) == qkv.size(0) &&
                  t.size(1) == qkv.size(1) && t.size(2) == 2 &&
                  t.size(3) == qkv.size(3),
              fn, ": ", name, " must have shape [B, T, 2, H] = [",
              qkv.size(0), ", ", qkv.size(1), ", 2, ", qkv.size(3),
              "], got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// the walk of a launch: iterations of Geometry<L>::kRowsPerIter rows per
// slice, the grid under the cap, and the (token, head) step between two
// visits
struct Walk {
  long n_tok, n_iters, step_tok;
  int heads, n_blocks, step_h;
  template <int L>
  Walk(const torch::Tensor& qkv, Geometry<L>)
      : n_tok(qkv.size(0) * qkv.size(1)), heads((int)qkv.size(3)) {
    using G = Geometry<L>;
    n_iters = (n_tok * heads + G::kRowsPerIter - 1) / G::kRowsPerIter;
    n_blocks = (int)std::min<long>(n_iters, G::kBlocks);
    const long stride = (long)n_blocks * G::kRowsPerIter;
    step_tok = n_blocks ? stride / heads : 0;
    step_h = n_blocks ? (int)(stride % heads) : 0;
  }
};

// f(Geometry<L>{}, V) for N = D / 16: an even N divides over L = 4 lanes,
// an odd one over 2 (file header)
template <int N, typename F>
void call_for(F& f) {
  constexpr int L = N % 2 ? 2 : 4;
  f(Geometry<L>{}, std::integral_constant<int, 2 * N / L>{});
}

template <typename F>
void dispatch_head_dim(long d, F&& f) {  // d was checked
  switch (d / 16) {
    case 1: call_for<1>(f); break;
    case 2: call_for<2>(f); break;
    case 3: call_for<3>(f); break;
    case 4: call_for<4>(f); break;
    case 5: call_for<5>(f); break;
    case 6: call_for<6>(f); break;
    case 7: call_for<7>(f); break;
    case 8: call_for<8>(f); break;
    case 9: call_for<9>(f); break;
    case 10: call_for<10>(f); break;
    case 11: call_for<11>(f); break;
    default: call_for<12>(f); break;
  }
}

}  // namespace

std::vector<torch::Tensor> qk_rmsnorm_fwd(torch::Tensor qkv, torch::Tensor wq,
                                          torch::Tensor wk, double eps) {
  const char* fn = "qk_rmsnorm_fwd";
  check_qkv(fn, "qkv", qkv);
  check_weight(fn, "wq", wq, qkv);
  check_weight(fn, "wk", wk, qkv);
  const long d = qkv.size(4);
  auto out = torch::empty_like(qkv);
  auto rstd = torch::empty({qkv.size(0), qkv.size(1), 2, qkv.size(3)},
                           qkv.options().dtype(torch::kFloat32));
  if (qkv.size(0) * qkv.size(1) == 0) return {out, rstd};  // no empty grid
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_head_dim(d, [&](auto geo, auto v) {
    constexpr int L = decltype(geo)::kLanes;
    const Walk wlk(qkv, geo);
    hipLaunchKernelGGL(
        (qk_rmsnorm_fwd_kernel<L, decltype(v)::value>), dim3(wlk.n_blocks),
        dim3(kFwdBlock), 0, stream, (const ushort8_t*)qkv.data_ptr(),
        (const ushort8_t*)wq.data_ptr(), (const ushort8_t*)wk.data_ptr(),
        (ushort8_t*)out.data_ptr(), rstd.data_ptr<float>(), wlk.n_tok,
        wlk.heads, wlk.n_iters, wlk.step_tok, wlk.step_h, 1.f / d,
        (float)eps);
  });
  HIP_CHECK_LAST();
  return {out, rstd};
}

std::vector<torch::Tensor> qk_rmsnorm_bwd(torch::Tensor dqkv,
                                          torch::Tensor qkv, torch::Tensor wq,
                                          torch::Tensor wk,
                                          torch::Tensor rstd) {
  const char* fn = "qk_rmsnorm_bwd";
  check_qkv(fn, "qkv", qkv);
  check_qkv_like(fn, "dqkv", dqkv, qkv);
  check_weight(fn, "wq", wq, qkv);
  check_weight(fn, "wk", wk, qkv);
  check_stat(fn, "rstd", rstd, qkv);
  const long d = qkv.size(4);
  // dwq, dwk as the rows of one [2, D] buffer
  auto grads = torch::empty({2, d}, wq.options());
  if (qkv.size(0) * qkv.size(1) == 0) {
    grads.zero_();
    return {grads[0], grads[1]};
  }
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_head_dim(d, [&](auto geo, auto v) {
    constexpr int L = decltype(geo)::kLanes;
    const Walk wlk(qkv, geo);
    auto part = torch::empty({wlk.n_blocks, 2, d},
                             qkv.options().dtype(torch::kFloat32));
    hipLaunchKernelGGL(
        (qk_rmsnorm_bwd_kernel<L, decltype(v)::value>), dim3(wlk.n_blocks),
        dim3(kBwdBlock), 0, stream, (ushort8_t*)dqkv.data_ptr(),
        (const ushort8_t*)qkv.data_ptr(), (const ushort8_t*)wq.data_ptr(),
        (const ushort8_t*)wk.data_ptr(), rstd.data_ptr<float>(),
        part.data_ptr<float>(), wlk.n_tok, wlk.heads, wlk.n_iters,
        wlk.step_tok, wlk.step_h, 1.f / d);
    HIP_CHECK_LAST();
    colsum_finish(part, grads, 2 * d, wlk.n_blocks, stream);
  });
  return {grads[0], grads[1]};
}

#endif  // VITFSDP_KERNELS_ONLY
