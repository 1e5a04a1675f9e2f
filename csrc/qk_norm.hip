// QK-norm (--qk_norm, kernel K4b): LayerNorm over head_dim on the q and k
// slices of the fused qkv projection [B, T, 3, H, D], in place of its
// layout: the output is again [B, T, 3, H, D] with v copied through, so
// fmha_fwd_qkv reads it unchanged.
//
// layernorm.hip gives a 256-thread block to a contiguous row of
// D = 5120.  Here a row is one head of one token, 32..192 elements, and
// there are 2 * B*T*H of them at stride 3*H*D between tokens.  So:
//
//   * A row belongs to a GROUP of kL = 4 adjacent lanes (one DPP quad).
//     Lane `sub` of the group holds the 16-byte vectors sub, sub + 4,
//     sub + 8, ... of the row: V = D/32 of them, 5 at D = 160.  The four
//     lanes of a group read 64 consecutive bytes per load.
//   * The whole row stays in registers: one global read of x per
//     direction, the mean first and the variance from centred values,
//     all three passes from registers.
//   * The row sums are two quad_perm DPP adds (xor 1, xor 2).  The
//     forward has no LDS and no barrier.
//   * A wave holds 16 groups = 16 CONSECUTIVE rows of one slice
//     (head h + 1 follows head h at a token, then the next token), a
//     workgroup kSliceWaves = 2 waves per slice: waves 0-1 q, 2-3 k and,
//     in the forward, 4-5 v, which only copy.  One workgroup-iteration is
//     kRowsPerIter = 32 rows of each slice.
//   * Workgroups walk the rows grid-stride under the cap kQkBlocks.  A
//     lane never changes slice or `sub`, so it owns the same 8 * V
//     columns of the same parameter pair for the whole walk, and the
//     backward keeps its share of dgamma / dbeta in 16 * V registers.
//     (token, head) advance by a precomputed (step_tok, step_h) with one
//     carry: one division per lane at the start, none per row.
//   * At the end of the walk the 16 groups of a wave fold by shuffles
//     (xor 4 .. 32), the two waves of a slice meet in LDS, and the
//     workgroup writes one row of the fp32 partials [n_blocks, 4, D]
//     (dwq, dbq, dwk, dbk).  colsum_final.h sums them in a fixed order:
//     no atomics, results repeat bit for bit.
//
// Arithmetic (tests/kernel_reference.py L2-L5, fp32 throughout):
//   mean = sum(x) * (1/D); var = max(sum((x - mean)^2) * (1/D), 0);
//   rstd = rsqrtf(var + eps); y = bf16((x - mean) * rstd * w + b);
//   g = dy * w; xhat = (x - mean) * rstd from the SAVED statistics;
//   dx = bf16(rstd * (g - mean(g) - xhat * mean(g * xhat)));
//   dgamma = sum dy * xhat; dbeta = sum dy.
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

// No packed fp32 VALU ops (v_pk_add/mul/fma_f32) in this file's kernels:
// the loops over 8-element vectors below are exactly what the compiler
// pairs into them.  (The host pass does not know the feature.)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "stream_tiles.h"  // widen

namespace {

constexpr int kL = 4;                              // lanes per row
constexpr int kWaveRows = WAVE_SIZE / kL;          // 16 rows per wave
constexpr int kSliceWaves = 2;                     // waves per slice
constexpr int kRowsPerIter = kSliceWaves * kWaveRows;  // 32 rows per slice
constexpr int kFwdBlock = 3 * kSliceWaves * WAVE_SIZE;  // q, k and v waves
constexpr int kBwdBlock = 2 * kSliceWaves * WAVE_SIZE;  // q and k waves
constexpr int kMinD = 32, kMaxD = 192;             // V = D/32 = 1..6
// Workgroup cap of the walk: 256 CUs x 2.  The backward's workgroup is
// one wave per SIMD and its widest instantiation (V = 6, 199 VGPRs) runs
// 2 waves per SIMD; the forward's 6 waves need 91 VGPRs at most (5 waves
// per SIMD, 3 workgroups per CU).  So in every instantiation all 512
// workgroups are resident at once and none waits for a second round.
constexpr int kQkBlocks = 512;

// Bit casts, the bf16 widening, rsqrt, max and the barrier by builtin.
// The HIP headers' plain-inline device functions (__uint_as_float,
// __shfl_xor, __syncthreads, ...) are compiled with the default target
// features; from the kernels of this file, which drop one, they are
// CALLED, per element, instead of inlined.  Nothing below calls one
// (__builtin_amdgcn_rsqf is the v_rsq_f32 that rsqrtf compiles to).
__device__ __forceinline__ float as_f32(unsigned u) {
  return __builtin_bit_cast(float, u);
}
__device__ __forceinline__ int as_i32(float f) {
  return __builtin_bit_cast(int, f);
}

// sum over the 4 lanes of a group; every lane gets the same bits (each
// step adds the same two operands on both sides)
__device__ __forceinline__ float group_sum(float v) {
  // quad_perm [1,0,3,2] and [2,3,0,1]
  v += as_f32(__builtin_amdgcn_update_dpp(0, as_i32(v), 0xB1, 0xF, 0xF, true));
  v += as_f32(__builtin_amdgcn_update_dpp(0, as_i32(v), 0x4E, 0xF, 0xF, true));
  return v;
}

// v of lane ^ off (__shfl_xor is a header function)
__device__ __forceinline__ float lane_xor(float v, int lane, int off) {
  return as_f32(__builtin_amdgcn_ds_bpermute((lane ^ off) << 2, as_i32(v)));
}

// Makes the compiler forget what it knows about the packed vectors at
// this point, so it cannot keep their unpacked fp32 copies (2x the
// registers) alive from one pass to the next; unpacking again is a shift
// or a mask per element.  No instruction is emitted.
template <int V>
__device__ __forceinline__ void keep_packed(ushort8_t (&v)[V]) {
#pragma unroll
  for (int k = 0; k < V; ++k) asm volatile("" : "+v"(v[k]));
}

// Where a lane stands in the walk.  Row r of a slice is (token r / H,
// head r % H); vector offset of its first element in [N, 3, H, D].
struct RowWalk {
  long tok;
  int h;
  int slice;  // wave-uniform
  int sub;

  __device__ __forceinline__ RowWalk(int heads) {
    const int wave = threadIdx.x / WAVE_SIZE;
    const int lane = threadIdx.x % WAVE_SIZE;
    slice = __builtin_amdgcn_readfirstlane(wave / kSliceWaves);
    sub = lane % kL;
    const long r = (long)blockIdx.x * kRowsPerIter +
                   (wave % kSliceWaves) * kWaveRows + lane / kL;
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

template <int V>
__global__ __launch_bounds__(kFwdBlock) void qk_norm_fwd_kernel(
    const ushort8_t* __restrict__ qkv, const ushort8_t* __restrict__ wq,
    const ushort8_t* __restrict__ bq, const ushort8_t* __restrict__ wk,
    const ushort8_t* __restrict__ bk, ushort8_t* __restrict__ out,
    float* __restrict__ mean_out, float* __restrict__ rstd_out, long n_tok,
    int heads, long n_iters, long step_tok, int step_h, float inv_d,
    float eps) {
  constexpr int nvec = V * kL;
  RowWalk at(heads);
  const long first = blockIdx.x;

  if (at.slice == 2) {  // v: bit-for-bit copy
    for (long it = first; it < n_iters; it += gridDim.x) {
      if (at.tok < n_tok) {
        const long o = at.vec_offset(heads, nvec);
        ushort8_t xv[V];
#pragma unroll
        for (int k = 0; k < V; ++k) xv[k] = qkv[o + k * kL];
#pragma unroll
        for (int k = 0; k < V; ++k) out[o + k * kL] = xv[k];
      }
      at.advance(step_tok, step_h, heads);
    }
    return;
  }

  const ushort8_t* __restrict__ w = at.slice ? wk : wq;
  const ushort8_t* __restrict__ b = at.slice ? bk : bq;
  ushort8_t wv[V], bv[V];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    wv[k] = w[at.sub + k * kL];
    bv[k] = b[at.sub + k * kL];
  }

  for (long it = first; it < n_iters; it += gridDim.x) {
    // a group is live or not as a whole; the DPP adds stay inside it
    const bool live = at.tok < n_tok;
    const long o = at.vec_offset(heads, nvec);
    ushort8_t xv[V] = {};
    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) xv[k] = qkv[o + k * kL];
    }
    keep_packed(wv);
    keep_packed(bv);

    float s = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) s += widen(xv[k][j]);
    const float mean = group_sum(s) * inv_d;
    keep_packed(xv);

    float ss = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float c = widen(xv[k][j]) - mean;
        ss += c * c;
      }
    const float var = __builtin_fmaxf(group_sum(ss) * inv_d, 0.f);
    const float rstd = __builtin_amdgcn_rsqf(var + eps);
    keep_packed(xv);

    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        ushort8_t y;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float xh = (widen(xv[k][j]) - mean) * rstd;
          y[j] = f32_to_bf16(xh * widen(wv[k][j]) +
                             widen(bv[k][j]));
        }
        out[o + k * kL] = y;
      }
      if (at.sub == 0) {
        const long so = at.stat_offset(heads);
        mean_out[so] = mean;
        rstd_out[so] = rstd;
      }
    }
    at.advance(step_tok, step_h, heads);
  }
}

template <int V>
__global__ __launch_bounds__(kBwdBlock) void qk_norm_bwd_kernel(
    ushort8_t* __restrict__ dqkv, const ushort8_t* __restrict__ qkv,
    const ushort8_t* __restrict__ wq, const ushort8_t* __restrict__ wk,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    float* __restrict__ part, long n_tok, int heads, long n_iters,
    long step_tok, int step_h, float inv_d) {
  constexpr int nvec = V * kL;
  constexpr int d = nvec * 8;
  // [wave][dgamma, dbeta][column]: the wave totals of the final fold
  __shared__ float fold[2 * kSliceWaves][2][d];
  RowWalk at(heads);

  const ushort8_t* __restrict__ w = at.slice ? wk : wq;
  ushort8_t wv[V];
  float dw_acc[V][8], db_acc[V][8];
#pragma unroll
  for (int k = 0; k < V; ++k) {
    wv[k] = w[at.sub + k * kL];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dw_acc[k][j] = 0.f;
      db_acc[k][j] = 0.f;
    }
  }

  for (long it = blockIdx.x; it < n_iters; it += gridDim.x) {
    const bool live = at.tok < n_tok;
    const long o = at.vec_offset(heads, nvec);
    ushort8_t xv[V] = {}, dv[V] = {};
    float mean = 0.f, rstd = 0.f;
    if (live) {
#pragma unroll
      for (int k = 0; k < V; ++k) {
        xv[k] = qkv[o + k * kL];
        dv[k] = dqkv[o + k * kL];
      }
      const long so = at.stat_offset(heads);
      mean = mean_in[so];
      rstd = rstd_in[so];
    }

    keep_packed(wv);

    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = widen(dv[k][j]) * widen(wv[k][j]);
        const float xh = (widen(xv[k][j]) - mean) * rstd;
        sg += g;
        sgx += g * xh;
      }
    sg = group_sum(sg) * inv_d;
    sgx = group_sum(sgx) * inv_d;
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
          const float xh = (widen(xv[k][j]) - mean) * rstd;
          dx[j] = f32_to_bf16(rstd * (g - sg - xh * sgx));
          dw_acc[k][j] += dyf * xh;
          db_acc[k][j] += dyf;
        }
        dqkv[o + k * kL] = dx;
      }
    }
    at.advance(step_tok, step_h, heads);
  }

  // the 16 groups of the wave: lanes with equal `sub` hold the same
  // columns, so xor 4 .. 32 leaves every lane with the wave's totals
  const int wave = threadIdx.x / WAVE_SIZE;
  const int lane = threadIdx.x % WAVE_SIZE;
#pragma unroll
  for (int off = kL; off < WAVE_SIZE; off <<= 1)
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dw_acc[k][j] += lane_xor(dw_acc[k][j], lane, off);
        db_acc[k][j] += lane_xor(db_acc[k][j], lane, off);
      }
  if (lane < kL) {
#pragma unroll
    for (int k = 0; k < V; ++k)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int col = (lane + k * kL) * 8 + j;
        fold[wave][0][col] = dw_acc[k][j];
        fold[wave][1][col] = db_acc[k][j];
      }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  // one row [4, D] of the partials: dwq, dbq, dwk, dbk
  float* prow = part + (long)blockIdx.x * 4 * d;
  for (int i = threadIdx.x; i < 4 * d; i += kBwdBlock) {
    const int kind = i / d, col = i % d;
    const int w0 = (kind / 2) * kSliceWaves;
    float t = fold[w0][kind % 2][col];
#pragma unroll
    for (int u = 1; u < kSliceWaves; ++u) t += fold[w0 + u][kind % 2][col];
    prow[i] = t;
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every head dim
#define VITFSDP_INSTANTIATE_QK_NORM(V_)                                      \
  template __global__ void qk_norm_fwd_kernel<V_>(                           \
      const ushort8_t*, const ushort8_t*, const ushort8_t*,                  \
      const ushort8_t*, const ushort8_t*, ushort8_t*, float*, float*, long,  \
      int, long, long, int, float, float);                                   \
  template __global__ void qk_norm_bwd_kernel<V_>(                           \
      ushort8_t*, const ushort8_t*, const ushort8_t*, const ushort8_t*,      \
      const float*, const float*, float*, long, int, long, long, int, float);
VITFSDP_INSTANTIATE_QK_NORM(1)
VITFSDP_INSTANTIATE_QK_NORM(2)
VITFSDP_INSTANTIATE_QK_NORM(3)
VITFSDP_INSTANTIATE_QK_NORM(4)
VITFSDP_INSTANTIATE_QK_NORM(5)
VITFSDP_INSTANTIATE_QK_NORM(6)
#undef VITFSDP_INSTANTIATE_QK_NORM
#endif

}  // namespace
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"

namespace {

// Operand checks, as in layernorm.hip: the kernels read raw pointers with
// every size taken from qkv, so each other operand is checked against it.

// the [B, T, 3, H, D] tensor that fixes the sizes and the device
void check_qkv(const char* fn, const char* name, const torch::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), fn, ": ", name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 5 && t.size(2) == 3 && t.size(3) > 0, fn, ": ", name,
              " must have shape [B, T, 3, H, D], got ", t.sizes());
  const long d = t.size(4);
  TORCH_CHECK(d >= kMinD && d <= kMaxD && d % 32 == 0, fn,
              ": head dim D must be one of 32, 64, 96, 128, 160, 192, got ",
              d);
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

// gamma / beta: bf16 [D]
void check_affine(const char* fn, const char* name, const torch::Tensor& t,
                  const torch::Tensor& qkv) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.dim() == 1 && t.size(0) == qkv.size(4), fn, ": ", name,
              " must have shape [", qkv.size(4), "], got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// saved mean / rstd: fp32 [B, T, 2, H]
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

// the walk of a launch: iterations of kRowsPerIter rows per slice, the
// grid under the cap, and the (token, head) step between two visits
struct Walk {
  long n_tok, n_iters, step_tok;
  int heads, n_blocks, step_h;
  explicit Walk(const torch::Tensor& qkv)
      : n_tok(qkv.size(0) * qkv.size(1)), heads((int)qkv.size(3)) {
    n_iters = (n_tok * heads + kRowsPerIter - 1) / kRowsPerIter;
    n_blocks = (int)std::min<long>(n_iters, kQkBlocks);
    const long stride = (long)n_blocks * kRowsPerIter;
    step_tok = n_blocks ? stride / heads : 0;
    step_h = n_blocks ? (int)(stride % heads) : 0;
  }
};

template <typename F>
void dispatch_head_dim(long d, F&& f) {
  switch (d / 32) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 3: f(std::integral_constant<int, 3>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 5: f(std::integral_constant<int, 5>{}); break;
    default: f(std::integral_constant<int, 6>{}); break;
  }
}

}  // namespace

std::vector<torch::Tensor> qk_norm_fwd(torch::Tensor qkv, torch::Tensor wq,
                                       torch::Tensor bq, torch::Tensor wk,
                                       torch::Tensor bk, double eps) {
  const char* fn = "qk_norm_fwd";
  check_qkv(fn, "qkv", qkv);
  check_affine(fn, "wq", wq, qkv);
  check_affine(fn, "bq", bq, qkv);
  check_affine(fn, "wk", wk, qkv);
  check_affine(fn, "bk", bk, qkv);
  const long d = qkv.size(4);
  auto out = torch::empty_like(qkv);
  auto opts = qkv.options().dtype(torch::kFloat32);
  auto mean = torch::empty({qkv.size(0), qkv.size(1), 2, qkv.size(3)}, opts);
  auto rstd = torch::empty_like(mean);
  const Walk wlk(qkv);
  if (wlk.n_tok == 0) return {out, mean, rstd};  // no zero-sized grid
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_head_dim(d, [&](auto v) {
    hipLaunchKernelGGL(
        (qk_norm_fwd_kernel<decltype(v)::value>), dim3(wlk.n_blocks),
        dim3(kFwdBlock), 0, stream, (const ushort8_t*)qkv.data_ptr(),
        (const ushort8_t*)wq.data_ptr(), (const ushort8_t*)bq.data_ptr(),
        (const ushort8_t*)wk.data_ptr(), (const ushort8_t*)bk.data_ptr(),
        (ushort8_t*)out.data_ptr(), mean.data_ptr<float>(),
        rstd.data_ptr<float>(), wlk.n_tok, wlk.heads, wlk.n_iters,
        wlk.step_tok, wlk.step_h, 1.f / d, (float)eps);
  });
  HIP_CHECK_LAST();
  return {out, mean, rstd};
}

std::vector<torch::Tensor> qk_norm_bwd(torch::Tensor dqkv, torch::Tensor qkv,
                                       torch::Tensor wq, torch::Tensor wk,
                                       torch::Tensor mean,
                                       torch::Tensor rstd) {
  const char* fn = "qk_norm_bwd";
  check_qkv(fn, "qkv", qkv);
  check_qkv_like(fn, "dqkv", dqkv, qkv);
  check_affine(fn, "wq", wq, qkv);
  check_affine(fn, "wk", wk, qkv);
  check_stat(fn, "mean", mean, qkv);
  check_stat(fn, "rstd", rstd, qkv);
  const long d = qkv.size(4);
  // dwq, dbq, dwk, dbk as the rows of one [4, D] buffer
  auto grads = torch::empty({4, d}, wq.options());
  const Walk wlk(qkv);
  if (wlk.n_tok == 0) {
    grads.zero_();
    return {grads[0], grads[1], grads[2], grads[3]};
  }
  auto part = torch::empty({wlk.n_blocks, 4, d},
                           qkv.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  dispatch_head_dim(d, [&](auto v) {
    hipLaunchKernelGGL(
        (qk_norm_bwd_kernel<decltype(v)::value>), dim3(wlk.n_blocks),
        dim3(kBwdBlock), 0, stream, (ushort8_t*)dqkv.data_ptr(),
        (const ushort8_t*)qkv.data_ptr(), (const ushort8_t*)wq.data_ptr(),
        (const ushort8_t*)wk.data_ptr(), mean.data_ptr<float>(),
        rstd.data_ptr<float>(), part.data_ptr<float>(), wlk.n_tok, wlk.heads,
        wlk.n_iters, wlk.step_tok, wlk.step_h, 1.f / d);
  });
  HIP_CHECK_LAST();
  colsum_finish(part, grads, 4 * d, wlk.n_blocks, stream);
  return {grads[0], grads[1], grads[2], grads[3]};
}

#endif  // VITFSDP_KERNELS_ONLY
