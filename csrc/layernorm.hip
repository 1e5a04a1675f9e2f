// LayerNorm forward/backward for CDNA4 (kernel K2).
//
// Replaces the torch LayerNorm in every ViT block (reference: timm Block
// norm1/norm2 and the final norm, run_vit_training.py:151).  Memory-bound:
// rows of D bf16 elements, fp32 statistics, 16-byte vectorized loads
// (guide G13: scalar bf16 loads cost ~2x).  One 256-thread block per row;
// the second pass re-reads x through L2 (a row is ~10 KB at D=5120, far
// inside the 4 MB per-XCD L2), which keeps register pressure flat across
// any D instead of caching the row in registers.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / WAVE_SIZE;

__global__ void ln_fwd_kernel(const ushort8_t* __restrict__ x,
                              const ushort8_t* __restrict__ w,
                              const ushort8_t* __restrict__ b,
                              ushort8_t* __restrict__ y,
                              float* __restrict__ mean_out,
                              float* __restrict__ rstd_out, int nvec,
                              float inv_d, float eps) {
  __shared__ float scratch[kWaves];
  const long row = blockIdx.x;
  const ushort8_t* xr = x + row * nvec;
  ushort8_t* yr = y + row * nvec;

  float s = 0.f, ss = 0.f;
  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t v = xr[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_to_f32(v[j]);
      s += f;
      ss += f * f;
    }
  }
  s = block_sum<kWaves>(s, scratch);
  ss = block_sum<kWaves>(ss, scratch);
  const float mean = s * inv_d;
  const float var = fmaxf(ss * inv_d - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }

  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t xv = xr[i], wv = w[i], bv = b[i], out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xh = (bf16_to_f32(xv[j]) - mean) * rstd;
      out[j] = f32_to_bf16(xh * bf16_to_f32(wv[j]) + bf16_to_f32(bv[j]));
    }
    yr[i] = out;
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g*xhat)), g = dy * w
__global__ void ln_bwd_dx_kernel(const ushort8_t* __restrict__ dy,
                                 const ushort8_t* __restrict__ x,
                                 const ushort8_t* __restrict__ w,
                                 const float* __restrict__ mean_in,
                                 const float* __restrict__ rstd_in,
                                 ushort8_t* __restrict__ dx, int nvec,
                                 float inv_d) {
  __shared__ float scratch[kWaves];
  const long row = blockIdx.x;
  const ushort8_t* dyr = dy + row * nvec;
  const ushort8_t* xr = x + row * nvec;
  ushort8_t* dxr = dx + row * nvec;
  const float mean = mean_in[row];
  const float rstd = rstd_in[row];

  float sg = 0.f, sgx = 0.f;
  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t dv = dyr[i], xv = xr[i], wv = w[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = bf16_to_f32(dv[j]) * bf16_to_f32(wv[j]);
      float xh = (bf16_to_f32(xv[j]) - mean) * rstd;
      sg += g;
      sgx += g * xh;
    }
  }
  sg = block_sum<kWaves>(sg, scratch) * inv_d;
  sgx = block_sum<kWaves>(sgx, scratch) * inv_d;

  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t dv = dyr[i], xv = xr[i], wv = w[i], out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = bf16_to_f32(dv[j]) * bf16_to_f32(wv[j]);
      float xh = (bf16_to_f32(xv[j]) - mean) * rstd;
      out[j] = f32_to_bf16(rstd * (g - sg - xh * sgx));
    }
    dxr[i] = out;
  }
}

// Column reductions for dgamma/dbeta: grid (D/256, row_chunks); each
// thread owns one column within its row chunk (coalesced across the
// 256 consecutive columns of the block), partials in fp32.
__global__ void ln_bwd_dwdb_partial_kernel(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    float* __restrict__ dw_part, float* __restrict__ db_part, int d,
    long n_rows, int rows_per_chunk) {
  const int col = blockIdx.x * kBlock + threadIdx.x;
  if (col >= d) return;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long row_end = min(row_begin + rows_per_chunk, n_rows);
  float dw = 0.f, db = 0.f;
  for (long r = row_begin; r < row_end; ++r) {
    float dyv = bf16_to_f32(dy[r * d + col]);
    float xh = (bf16_to_f32(x[r * d + col]) - mean_in[r]) * rstd_in[r];
    dw += dyv * xh;
    db += dyv;
  }
  dw_part[(long)blockIdx.y * d + col] = dw;
  db_part[(long)blockIdx.y * d + col] = db;
}

// Final stage of the dgamma/dbeta reduction over [n_chunks, d] fp32
// partials.  A block owns 32 columns and splits the chunks over 8
// slices (thread = (slice, column)), so d = 5120 gives 160 blocks that
// each stream 128-byte row segments; a one-column-per-thread layout
// would leave the 768-chunk buffers of the fused kernel below to 20
// blocks.  The 8 slice sums meet in LDS.
constexpr int kFinalCols = 32;
constexpr int kFinalSlices = kBlock / kFinalCols;

__global__ void ln_bwd_dwdb_final_kernel(const float* __restrict__ dw_part,
                                         const float* __restrict__ db_part,
                                         unsigned short* __restrict__ dw,
                                         unsigned short* __restrict__ db,
                                         int d, int n_chunks) {
  __shared__ float sw_s[kFinalSlices][kFinalCols];
  __shared__ float sb_s[kFinalSlices][kFinalCols];
  const int c = threadIdx.x % kFinalCols;
  const int slice = threadIdx.x / kFinalCols;
  const int col = blockIdx.x * kFinalCols + c;
  float sw = 0.f, sb = 0.f;
  if (col < d) {
#pragma unroll 4
    for (int ch = slice; ch < n_chunks; ch += kFinalSlices) {
      sw += dw_part[(long)ch * d + col];
      sb += db_part[(long)ch * d + col];
    }
  }
  sw_s[slice][c] = sw;
  sb_s[slice][c] = sb;
  __syncthreads();
  if (slice == 0 && col < d) {
#pragma unroll
    for (int s = 1; s < kFinalSlices; ++s) {
      sw += sw_s[s][c];
      sb += sb_s[s][c];
    }
    dw[col] = f32_to_bf16(sw);
    db[col] = f32_to_bf16(sb);
  }
}

// Single-pass backward: dx AND the dgamma/dbeta column partials from one
// read of dy and x.  The separate partial kernel above re-read both
// [N, D] tensors (671 MB at N = 32768, D = 5120) right after the dx
// kernel had streamed them.
//
// A block walks rows blockIdx.x, blockIdx.x + gridDim.x, ...  Thread tid
// always touches vector columns tid + k*256 (k < VPT), so it owns those
// columns in every row it sees, and dy*xhat / dy from the dx pass
// accumulate into 2 * 8 * VPT fp32 registers (48 at VPT = 3, D = 5120).
// At the end the block writes one row of the [gridDim.x, D] partials
// and ln_bwd_dwdb_final_kernel reduces them.
//
// The per-row dx arithmetic (expressions, per-thread accumulation order,
// block_sum) is that of ln_bwd_dx_kernel / ln_add_bwd_dx_kernel, so dx
// is bit-identical to the two-kernel path.
//
// Grid: kFusedBlocks = 768 = 256 CUs x 3 blocks.  A block is one wave
// per SIMD and the kernel needs 132-168 VGPRs (3 waves/SIMD), so exactly
// 768 blocks are resident at once and none waits for a second round.
// Partials at D = 5120: 768 x 5120 x 4 B x 2 = 31 MB written and 31 MB
// read back by the final kernel — 9% of the 671 MB re-read this
// replaces.
constexpr int kFusedBlocks = 768;
constexpr int kMaxVpt = 4;  // D <= 8192; wider rows take the two-kernel path

template <int VPT, bool ADD>
__global__ __launch_bounds__(kBlock) void ln_bwd_fused_kernel(
    const ushort8_t* __restrict__ dy, const ushort8_t* __restrict__ dsum,
    const ushort8_t* __restrict__ x, const ushort8_t* __restrict__ w,
    const float* __restrict__ mean_in, const float* __restrict__ rstd_in,
    ushort8_t* __restrict__ dx1, ushort8_t* __restrict__ dx2,
    float* __restrict__ dw_part, float* __restrict__ db_part, int nvec,
    long n_rows, float inv_d) {
  __shared__ float scratch[kWaves];
  float dw_acc[VPT][8], db_acc[VPT][8];
  ushort8_t wv[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (i < nvec) wv[k] = w[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      dw_acc[k][j] = 0.f;
      db_acc[k][j] = 0.f;
    }
  }

  for (long row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const ushort8_t* dyr = dy + row * nvec;
    const ushort8_t* xr = x + row * nvec;
    const float mean = mean_in[row];
    const float rstd = rstd_in[row];

    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int i = threadIdx.x + k * kBlock;
      if (i < nvec) {
        const ushort8_t dv = dyr[i], xv = xr[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float g = bf16_to_f32(dv[j]) * bf16_to_f32(wv[k][j]);
          float xh = (bf16_to_f32(xv[j]) - mean) * rstd;
          sg += g;
          sgx += g * xh;
        }
      }
    }
    sg = block_sum<kWaves>(sg, scratch) * inv_d;
    sgx = block_sum<kWaves>(sgx, scratch) * inv_d;

    // second pass re-reads the row through L2 like the one-row kernels
    // (holding it unpacked costs ~70 VGPRs and halves the occupancy)
#pragma unroll
    for (int k = 0; k < VPT; ++k) {
      const int i = threadIdx.x + k * kBlock;
      if (i < nvec) {
        const ushort8_t dv = dyr[i], xv = xr[i];
        ushort8_t av, out;
        if (ADD) av = dsum[row * nvec + i];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float dyf = bf16_to_f32(dv[j]);
          float g = dyf * bf16_to_f32(wv[k][j]);
          float xh = (bf16_to_f32(xv[j]) - mean) * rstd;
          if (ADD) {
            out[j] = f32_to_bf16(rstd * (g - sg - xh * sgx) +
                                 bf16_to_f32(av[j]));
          } else {
            out[j] = f32_to_bf16(rstd * (g - sg - xh * sgx));
          }
          dw_acc[k][j] += dyf * xh;
          db_acc[k][j] += dyf;
        }
        dx1[row * nvec + i] = out;
        if (ADD) dx2[row * nvec + i] = out;
      }
    }
  }

  const long part_row = (long)blockIdx.x * nvec * 8;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * kBlock;
    if (i < nvec) {
      float4* pw = reinterpret_cast<float4*>(dw_part + part_row + (long)i * 8);
      float4* pb = reinterpret_cast<float4*>(db_part + part_row + (long)i * 8);
      pw[0] = make_float4(dw_acc[k][0], dw_acc[k][1], dw_acc[k][2],
                          dw_acc[k][3]);
      pw[1] = make_float4(dw_acc[k][4], dw_acc[k][5], dw_acc[k][6],
                          dw_acc[k][7]);
      pb[0] = make_float4(db_acc[k][0], db_acc[k][1], db_acc[k][2],
                          db_acc[k][3]);
      pb[1] = make_float4(db_acc[k][4], db_acc[k][5], db_acc[k][6],
                          db_acc[k][7]);
    }
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports the real configs
// (VPT = 3 is D = 5120, VPT = 4 the widest fused row)
#define VITFSDP_INSTANTIATE_LN(VPT_, ADD_)                                   \
  template __global__ void ln_bwd_fused_kernel<VPT_, ADD_>(                  \
      const ushort8_t*, const ushort8_t*, const ushort8_t*,                  \
      const ushort8_t*, const float*, const float*, ushort8_t*, ushort8_t*,  \
      float*, float*, int, long, float);
VITFSDP_INSTANTIATE_LN(1, false)
VITFSDP_INSTANTIATE_LN(3, false)
VITFSDP_INSTANTIATE_LN(3, true)
VITFSDP_INSTANTIATE_LN(4, false)
VITFSDP_INSTANTIATE_LN(4, true)
#undef VITFSDP_INSTANTIATE_LN
#endif


// Fused residual-add + LayerNorm (SURVEY.md K2 fused epilogue): the
// pre-LN block computes norm2(x + attn_out) — fusing the add into the
// LN's statistics pass removes one full read+write of the [N, D] tensor
// per call, and the backward folds the residual gradient add into the
// dx pass (no separate elementwise add kernels).
__global__ void ln_add_fwd_kernel(const ushort8_t* __restrict__ x,
                                  const ushort8_t* __restrict__ res,
                                  const ushort8_t* __restrict__ w,
                                  const ushort8_t* __restrict__ b,
                                  ushort8_t* __restrict__ sum_out,
                                  ushort8_t* __restrict__ y,
                                  float* __restrict__ mean_out,
                                  float* __restrict__ rstd_out, int nvec,
                                  float inv_d, float eps) {
  __shared__ float scratch[kWaves];
  const long row = blockIdx.x;
  const ushort8_t* xr = x + row * nvec;
  const ushort8_t* rr = res + row * nvec;
  ushort8_t* sr = sum_out + row * nvec;
  ushort8_t* yr = y + row * nvec;

  float s = 0.f, ss = 0.f;
  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t xv = xr[i], rv = rr[i], sv;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf16_to_f32(xv[j]) + bf16_to_f32(rv[j]);
      sv[j] = f32_to_bf16(f);
      // statistics on the bf16-rounded sum, so pass 2 normalizes the
      // exact values it re-reads
      f = bf16_to_f32(sv[j]);
      s += f;
      ss += f * f;
    }
    sr[i] = sv;
  }
  s = block_sum<kWaves>(s, scratch);
  ss = block_sum<kWaves>(ss, scratch);
  const float mean = s * inv_d;
  const float var = fmaxf(ss * inv_d - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  if (threadIdx.x == 0) {
    mean_out[row] = mean;
    rstd_out[row] = rstd;
  }

  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t sv = sr[i], wv = w[i], bv = b[i], out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float xh = (bf16_to_f32(sv[j]) - mean) * rstd;
      out[j] = f32_to_bf16(xh * bf16_to_f32(wv[j]) + bf16_to_f32(bv[j]));
    }
    yr[i] = out;
  }
}

// dx = rstd*(g - mean(g) - xhat*mean(g*xhat)) + dsum; written to TWO
// buffers (the gradients of x and res are identical but the autograd
// engine must receive distinct tensors it may mutate independently)
__global__ void ln_add_bwd_dx_kernel(const ushort8_t* __restrict__ dy,
                                     const ushort8_t* __restrict__ dsum,
                                     const ushort8_t* __restrict__ s_in,
                                     const ushort8_t* __restrict__ w,
                                     const float* __restrict__ mean_in,
                                     const float* __restrict__ rstd_in,
                                     ushort8_t* __restrict__ dx1,
                                     ushort8_t* __restrict__ dx2, int nvec,
                                     float inv_d) {
  __shared__ float scratch[kWaves];
  const long row = blockIdx.x;
  const ushort8_t* dyr = dy + row * nvec;
  const ushort8_t* dsr = dsum + row * nvec;
  const ushort8_t* sr = s_in + row * nvec;
  ushort8_t* d1 = dx1 + row * nvec;
  ushort8_t* d2 = dx2 + row * nvec;
  const float mean = mean_in[row];
  const float rstd = rstd_in[row];

  float sg = 0.f, sgx = 0.f;
  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t dv = dyr[i], sv = sr[i], wv = w[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = bf16_to_f32(dv[j]) * bf16_to_f32(wv[j]);
      float xh = (bf16_to_f32(sv[j]) - mean) * rstd;
      sg += g;
      sgx += g * xh;
    }
  }
  sg = block_sum<kWaves>(sg, scratch) * inv_d;
  sgx = block_sum<kWaves>(sgx, scratch) * inv_d;

  for (int i = threadIdx.x; i < nvec; i += kBlock) {
    ushort8_t dv = dyr[i], sv = sr[i], wv = w[i], av = dsr[i], out;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float g = bf16_to_f32(dv[j]) * bf16_to_f32(wv[j]);
      float xh = (bf16_to_f32(sv[j]) - mean) * rstd;
      out[j] = f32_to_bf16(rstd * (g - sg - xh * sgx) + bf16_to_f32(av[j]));
    }
    d1[i] = out;
    d2[i] = out;
  }
}

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

void launch_dwdb_final(const torch::Tensor& dw_part,
                       const torch::Tensor& db_part, torch::Tensor& dw,
                       torch::Tensor& db, int d, int n_chunks,
                       hipStream_t stream) {
  hipLaunchKernelGGL(ln_bwd_dwdb_final_kernel,
                     dim3((d + kFinalCols - 1) / kFinalCols), dim3(kBlock), 0,
                     stream, dw_part.data_ptr<float>(),
                     db_part.data_ptr<float>(),
                     (unsigned short*)dw.data_ptr(),
                     (unsigned short*)db.data_ptr(), d, n_chunks);
  HIP_CHECK_LAST();
}

// two-kernel dgamma/dbeta for rows wider than the fused kernel's largest
// instantiation: column partials over row chunks, then the final stage
void dwdb_two_stage(const torch::Tensor& dy, const torch::Tensor& x,
                    const torch::Tensor& mean, const torch::Tensor& rstd,
                    torch::Tensor& dw, torch::Tensor& db, int d, long n,
                    hipStream_t stream) {
  // pick row chunking so the partial grid fills the chip: target ~2048
  // blocks total (256 CUs x 8, guide G11)
  const int grid_x = (d + kBlock - 1) / kBlock;
  int n_chunks = std::max(1, 2048 / std::max(grid_x, 1));
  int rows_per_chunk = (int)((n + n_chunks - 1) / n_chunks);
  rows_per_chunk = std::max(rows_per_chunk, 16);
  n_chunks = (int)((n + rows_per_chunk - 1) / rows_per_chunk);
  auto opts = x.options().dtype(torch::kFloat32);
  auto dw_part = torch::empty({n_chunks, d}, opts);
  auto db_part = torch::empty({n_chunks, d}, opts);
  hipLaunchKernelGGL(ln_bwd_dwdb_partial_kernel, dim3(grid_x, n_chunks),
                     dim3(kBlock), 0, stream,
                     (const unsigned short*)dy.data_ptr(),
                     (const unsigned short*)x.data_ptr(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(),
                     dw_part.data_ptr<float>(), db_part.data_ptr<float>(), d, n,
                     rows_per_chunk);
  HIP_CHECK_LAST();
  launch_dwdb_final(dw_part, db_part, dw, db, d, n_chunks, stream);
}

// dx (+ the second copy and the residual gradient when ADD) and dw/db in
// one pass over dy and x; requires d/8 <= kMaxVpt * kBlock
template <bool ADD>
void launch_bwd_fused(const torch::Tensor& dy, const torch::Tensor* dsum,
                      const torch::Tensor& x, const torch::Tensor& w,
                      const torch::Tensor& mean, const torch::Tensor& rstd,
                      torch::Tensor& dx1, torch::Tensor* dx2,
                      torch::Tensor& dw, torch::Tensor& db, int d, long n,
                      hipStream_t stream) {
  const int nvec = d / 8;
  const int n_blocks = (int)std::min<long>(n, kFusedBlocks);
  auto opts = x.options().dtype(torch::kFloat32);
  auto dw_part = torch::empty({n_blocks, d}, opts);
  auto db_part = torch::empty({n_blocks, d}, opts);
  auto launch = [&](auto vpt) {
    hipLaunchKernelGGL(
        (ln_bwd_fused_kernel<decltype(vpt)::value, ADD>), dim3(n_blocks),
        dim3(kBlock), 0, stream, (const ushort8_t*)dy.data_ptr(),
        ADD ? (const ushort8_t*)dsum->data_ptr() : nullptr,
        (const ushort8_t*)x.data_ptr(), (const ushort8_t*)w.data_ptr(),
        mean.data_ptr<float>(), rstd.data_ptr<float>(),
        (ushort8_t*)dx1.data_ptr(),
        ADD ? (ushort8_t*)dx2->data_ptr() : nullptr,
        dw_part.data_ptr<float>(), db_part.data_ptr<float>(), nvec, n,
        1.f / d);
  };
  switch ((nvec + kBlock - 1) / kBlock) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    default: launch(std::integral_constant<int, 4>{}); break;
  }
  HIP_CHECK_LAST();
  launch_dwdb_final(dw_part, db_part, dw, db, d, n_blocks, stream);
}

inline bool fused_bwd_fits(int d) {
  return d % 8 == 0 && d / 8 <= kMaxVpt * kBlock;
}

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
  TORCH_CHECK(x.dim() >= 1 && x.size(-1) > 0 && x.size(-1) % 8 == 0, fn,
              ": ", name, " must have a last dimension D that is a positive "
              "multiple of 8, got shape ", x.sizes());
  TORCH_CHECK(x.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// another [rows, D] bf16 operand: dy, dsum, res
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

// gamma / beta: bf16 of D elements
void check_affine(const char* fn, const char* name, const torch::Tensor& t,
                  const torch::Tensor& x) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.numel() == x.size(-1), fn, ": ", name, " must have D = ",
              x.size(-1), " elements, got ", t.numel());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

// saved mean / rstd: fp32, one per row
void check_stat(const char* fn, const char* name, const torch::Tensor& t,
                const torch::Tensor& x, long rows) {
  TORCH_CHECK(t.is_cuda() && t.device() == x.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, fn, ": ", name,
              " must be fp32, got ", t.scalar_type());
  TORCH_CHECK(t.numel() == rows, fn, ": ", name, " must have one element per "
              "row (", rows, "), got ", t.numel());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

}  // namespace

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps) {
  check_rows_input("layernorm_fwd", "x", x);
  check_affine("layernorm_fwd", "weight", w, x);
  check_affine("layernorm_fwd", "bias", b, x);
  const int d = x.size(-1);
  const long n = x.numel() / d;
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({n}, opts);
  auto rstd = torch::empty({n}, opts);
  if (n == 0) return {y, mean, rstd};  // a zero-sized grid is a launch error
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)n), dim3(kBlock), 0, stream,
                     (const ushort8_t*)x.data_ptr(),
                     (const ushort8_t*)w.data_ptr(),
                     (const ushort8_t*)b.data_ptr(), (ushort8_t*)y.data_ptr(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), d / 8,
                     1.f / d, (float)eps);
  HIP_CHECK_LAST();
  return {y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd) {
  check_rows_input("layernorm_bwd", "x", x);
  check_rows_like("layernorm_bwd", "dy", dy, x);
  check_affine("layernorm_bwd", "weight", w, x);
  const int d = x.size(-1);
  const long n = x.numel() / d;
  check_stat("layernorm_bwd", "mean", mean, x, n);
  check_stat("layernorm_bwd", "rstd", rstd, x, n);
  auto dx = torch::empty_like(x);
  auto dw = torch::empty_like(w);
  auto db = torch::empty_like(w);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (n == 0) {
    dw.zero_();
    db.zero_();
    return {dx, dw, db};
  }
  if (fused_bwd_fits(d)) {
    launch_bwd_fused<false>(dy, nullptr, x, w, mean, rstd, dx, nullptr, dw, db,
                            d, n, stream);
    return {dx, dw, db};
  }
  hipLaunchKernelGGL(ln_bwd_dx_kernel, dim3((unsigned)n), dim3(kBlock), 0,
                     stream, (const ushort8_t*)dy.data_ptr(),
                     (const ushort8_t*)x.data_ptr(),
                     (const ushort8_t*)w.data_ptr(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), (ushort8_t*)dx.data_ptr(), d / 8,
                     1.f / d);
  HIP_CHECK_LAST();
  dwdb_two_stage(dy, x, mean, rstd, dw, db, d, n, stream);
  return {dx, dw, db};
}


std::vector<torch::Tensor> layernorm_add_fwd(torch::Tensor x,
                                             torch::Tensor res,
                                             torch::Tensor w, torch::Tensor b,
                                             double eps) {
  check_rows_input("layernorm_add_fwd", "x", x);
  check_rows_like("layernorm_add_fwd", "res", res, x);
  check_affine("layernorm_add_fwd", "weight", w, x);
  check_affine("layernorm_add_fwd", "bias", b, x);
  const int d = x.size(-1);
  const long n = x.numel() / d;
  auto sum = torch::empty_like(x);
  auto y = torch::empty_like(x);
  auto opts = x.options().dtype(torch::kFloat32);
  auto mean = torch::empty({n}, opts);
  auto rstd = torch::empty({n}, opts);
  if (n == 0) return {sum, y, mean, rstd};
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ln_add_fwd_kernel, dim3((unsigned)n), dim3(kBlock), 0,
                     stream, (const ushort8_t*)x.data_ptr(),
                     (const ushort8_t*)res.data_ptr(),
                     (const ushort8_t*)w.data_ptr(),
                     (const ushort8_t*)b.data_ptr(),
                     (ushort8_t*)sum.data_ptr(), (ushort8_t*)y.data_ptr(),
                     mean.data_ptr<float>(), rstd.data_ptr<float>(), d / 8,
                     1.f / d, (float)eps);
  HIP_CHECK_LAST();
  return {sum, y, mean, rstd};
}

std::vector<torch::Tensor> layernorm_add_bwd(torch::Tensor dy,
                                             torch::Tensor dsum,
                                             torch::Tensor sum,
                                             torch::Tensor w,
                                             torch::Tensor mean,
                                             torch::Tensor rstd) {
  check_rows_input("layernorm_add_bwd", "sum", sum);
  check_rows_like("layernorm_add_bwd", "dy", dy, sum);
  check_rows_like("layernorm_add_bwd", "dsum", dsum, sum);
  check_affine("layernorm_add_bwd", "weight", w, sum);
  const int d = sum.size(-1);
  const long n = sum.numel() / d;
  check_stat("layernorm_add_bwd", "mean", mean, sum, n);
  check_stat("layernorm_add_bwd", "rstd", rstd, sum, n);
  auto dx1 = torch::empty_like(sum);
  auto dx2 = torch::empty_like(sum);
  auto dw = torch::empty_like(w);
  auto db = torch::empty_like(w);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (n == 0) {
    dw.zero_();
    db.zero_();
    return {dx1, dx2, dw, db};
  }
  if (fused_bwd_fits(d)) {
    launch_bwd_fused<true>(dy, &dsum, sum, w, mean, rstd, dx1, &dx2, dw, db, d,
                           n, stream);
    return {dx1, dx2, dw, db};
  }
  hipLaunchKernelGGL(ln_add_bwd_dx_kernel, dim3((unsigned)n), dim3(kBlock), 0,
                     stream, (const ushort8_t*)dy.data_ptr(),
                     (const ushort8_t*)dsum.data_ptr(),
                     (const ushort8_t*)sum.data_ptr(),
                     (const ushort8_t*)w.data_ptr(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), (ushort8_t*)dx1.data_ptr(),
                     (ushort8_t*)dx2.data_ptr(), d / 8, 1.f / d);
  HIP_CHECK_LAST();
  // dgamma/dbeta: same two-stage column reduction as plain LN, with the
  // summed input playing the role of x
  dwdb_two_stage(dy, sum, mean, rstd, dw, db, d, n, stream);
  return {dx1, dx2, dw, db};
}

#endif  // VITFSDP_KERNELS_ONLY
