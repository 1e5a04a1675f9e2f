// SwiGLU between fc1 and fc2 (--mlp_type swiglu): from the packed
// pre-activation h [rows, 2H], gate half first,
//     a = silu(g) * u,   g = h[:, :H],  u = h[:, H:]
// forward in one pass, backward in one pass that also yields fc1's bias
// gradient (the column sums of dh), and the transposed variants the TN
// weight-gradient route wants: dh^T as a third output of the backward
// and a^T rebuilt from h for fc2.  The treatment gelu.hip gives the GELU.
//
// All kernels are memory-bound, bf16 in and out, fp32 arithmetic, 16-byte
// accesses: s = 1 / (1 + expf(-g)), a = g * s * u, every output rounded
// once.  The gate vector and its value twin sit H elements apart in one
// row, so each kernel reads two (backward: three) streams with the same
// row stride 2H.
//
//   swiglu_fwd_kernel         thread per 8-wide output column, walking
//                             the rows of its chunk: 2 loads, 1 store
//   swiglu_bwd_colsum_kernel  the same walk: 3 loads, 2 stores, and 16
//                             fp32 running sums (8 gate columns, their 8
//                             value twins) in registers; partials
//                             [n_chunks, 2H] finished by colsum_final.h
//   swiglu_bwd_colsum_t_kernel  64-row x (128 gate + 128 value) column
//                             tiles through 32 KB of LDS: (A) compute,
//                             store dh and the tile, (B) a thread per tile
//                             column adds its rows in row order, (C) 8
//                             lanes assemble a 128-byte segment of dh^T
//   swiglu_fwd_t_kernel       transpose.hip's 64 x 64 tiles and grid with
//                             the activation between the two loads and
//                             the LDS write
//
// Bit identities the callers rely on: both backward kernels evaluate
// dswiglu_pair and use one chunk plan, and both add a column's rounded
// values in row order, so dh and the sums are equal in bits; both forward
// kernels evaluate swiglu_one, so swiglu_fwd_t(h) is swiglu_fwd(h).t() in
// bits.
//
// DROP instantiations (hidden dropout behind the activation): element
// (row, col in [0, H)) is kept by hash_keep (stream_tiles.h).  The
// backward takes the plain da: the
// mask and the scale are applied here, to both halves.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "colsum_final.h"
#include "common.h"
#ifndef VITFSDP_KERNELS_ONLY
#include "transpose.h"  // transpose_plan: swiglu_fwd_t moves transpose.hip's tiles
#endif

// No packed fp32 VALU ops (v_pk_add/mul/fma_f32) in this file's kernels:
// the loops over 8-element vectors below are exactly what the compiler
// pairs into them.  (The host pass does not know the feature.)
#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

#include "stream_tiles.h"

namespace {

constexpr int kBlock = 256;

// expf(-g) overflows to +inf from g < -88.7: s is then +0 and every
// product below a signed zero, the limit.
__device__ __forceinline__ float sigmoid_f32(float g) {
  return 1.f / (1.f + expf(-g));
}

// THE forward expression: both forward kernels call it.
__device__ __forceinline__ float swiglu_one(float g, float u) {
  return g * sigmoid_f32(g) * u;
}

// THE backward expression: both backward kernels call it.  The fma is
// written out so that no kernel contracts it differently.
__device__ __forceinline__ void dswiglu_pair(float da, float g, float u,
                                             float& dg, float& du) {
  const float s = sigmoid_f32(g);
  dg = da * u * s * __builtin_fmaf(g, 1.f - s, 1.f);
  du = da * g * s;
}

template <bool DROP>
__device__ __forceinline__ unsigned short swiglu_elem(unsigned short g,
                                                      unsigned short u,
                                                      const DropArgs& d,
                                                      unsigned row,
                                                      unsigned col) {
  if constexpr (DROP) {
    const bool keep = hash_keep(d.seed, d.thresh, row, col);
    return keep ? f32_to_bf16(swiglu_one(widen(g), widen(u)) * d.rscale)
                : (unsigned short)0;
  } else {
    return f32_to_bf16(swiglu_one(widen(g), widen(u)));
  }
}

// A dropped element is SELECTED to +0 in both halves.
template <bool DROP>
__device__ __forceinline__ void dswiglu_elem(unsigned short da,
                                             unsigned short g,
                                             unsigned short u,
                                             const DropArgs& d, unsigned row,
                                             unsigned col, unsigned short& dg,
                                             unsigned short& du) {
  float fg, fu;
  if constexpr (DROP) {
    const bool keep = hash_keep(d.seed, d.thresh, row, col);
    dswiglu_pair(widen(da) * d.rscale, widen(g), widen(u), fg, fu);
    dg = keep ? f32_to_bf16(fg) : (unsigned short)0;
    du = keep ? f32_to_bf16(fu) : (unsigned short)0;
  } else {
    dswiglu_pair(widen(da), widen(g), widen(u), fg, fu);
    dg = f32_to_bf16(fg);
    du = f32_to_bf16(fu);
  }
}

// h: [n_rows, 2 * nvec] vectors, a: [n_rows, nvec] vectors
template <bool DROP>
__global__ __launch_bounds__(kBlock) void swiglu_fwd_kernel(
    const ushort8_t* __restrict__ h, ushort8_t* __restrict__ a, int nvec,
    long n_rows, int rows_per_chunk, DropArgs drop) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const unsigned c0 = (unsigned)vc * 8u;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long chunk_end = row_begin + rows_per_chunk;
  const long row_end = chunk_end < n_rows ? chunk_end : n_rows;
#pragma unroll 4
  for (long r = row_begin; r < row_end; ++r) {
    const ushort8_t gv = h[r * 2 * nvec + vc];
    const ushort8_t uv = h[r * 2 * nvec + nvec + vc];
    ushort8_t out;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      out[j] = swiglu_elem<DROP>(gv[j], uv[j], drop, (unsigned)r, c0 + j);
    a[r * nvec + vc] = out;
  }
}

// da: [n_rows, nvec] vectors; h, dh: [n_rows, 2 * nvec] vectors;
// part: fp32 [gridDim.y, 16 * nvec]
template <bool DROP>
__global__ __launch_bounds__(kBlock) void swiglu_bwd_colsum_kernel(
    const ushort8_t* __restrict__ da, const ushort8_t* __restrict__ h,
    ushort8_t* __restrict__ dh, float* __restrict__ part, int nvec,
    long n_rows, int rows_per_chunk, DropArgs drop) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const unsigned c0 = (unsigned)vc * 8u;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long chunk_end = row_begin + rows_per_chunk;
  const long row_end = chunk_end < n_rows ? chunk_end : n_rows;
  float acc_g[8], acc_u[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc_g[j] = acc_u[j] = 0.f;
#pragma unroll 2
  for (long r = row_begin; r < row_end; ++r) {
    const long ig = r * 2 * nvec + vc, iu = ig + nvec;
    const ushort8_t dv = da[r * nvec + vc], gv = h[ig], uv = h[iu];
    ushort8_t og, ou;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned short dg, du;
      dswiglu_elem<DROP>(dv[j], gv[j], uv[j], drop, (unsigned)r, c0 + j, dg,
                         du);
      og[j] = dg;
      ou[j] = du;
      // the sums are over the ROUNDED values: they equal dh.sum(0)
      acc_g[j] += widen(dg);
      acc_u[j] += widen(du);
    }
    dh[ig] = og;
    dh[iu] = ou;
  }
  float* pg = part + ((long)blockIdx.y * 2 * nvec + vc) * 8;
  store_partials8(pg, acc_g);
  store_partials8(pg + (long)nvec * 8, acc_u);
}

// The same, and dh^T [2H, rows] as a third output.  A block owns kTHalf
// gate columns from c0 and their value twins from H + c0; tile column tc
// holds dh column c0 + tc for tc < kTHalf and H + c0 + tc - kTHalf above.
// The tile is 64 rows x 256 columns of bf16 = 32 KB, a row 32 16-byte
// slots stored at slot ^ (row / 8 % 8): the XOR touches the low three
// bits only, so each half stays in its own 16 slots, and the 8 lanes that
// assemble a dh^T segment in (C) land in 8 different 4-bank groups.  The
// chunks and the order of every sum are the plain kernel's.  8-row groups
// that straddle a chunk edge, and all groups when rows % 8 != 0, are
// stored by element.
constexpr int kTRows = 64;
constexpr int kTHalf = 128;
constexpr int kTCols = 2 * kTHalf;
constexpr int kTSlots = kTCols / 8;
constexpr int kTHalfSlots = kTHalf / 8;

__global__ __launch_bounds__(kBlock) void swiglu_bwd_colsum_t_kernel(
    const unsigned short* __restrict__ da, const unsigned short* __restrict__ h,
    unsigned short* __restrict__ dh, unsigned short* __restrict__ dht,
    float* __restrict__ part, long H, long n_rows, int rows_per_chunk) {
  __shared__ ushort8_t tile[kTRows * kTSlots];
  const unsigned short* tile_s = reinterpret_cast<const unsigned short*>(tile);
  const DropArgs no_drop = {0u, 1.f, 0u};
  const int t = threadIdx.x;
  const long c0 = (long)blockIdx.x * kTHalf;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long chunk_end = row_begin + rows_per_chunk;
  const long row_end = chunk_end < n_rows ? chunk_end : n_rows;
  const bool vec_store = (n_rows & 7) == 0;  // dh^T rows 16-byte aligned
  // (A): gate slot a_slot and value slot a_slot + 16 of rows a_row + 16k
  const int a_slot = t & (kTHalfSlots - 1), a_row = t >> 4;
  const bool a_col_ok = c0 + a_slot * 8 < H;
  // (B): tile column t, that is dh column b_col
  const bool b_col_ok = c0 + (t & (kTHalf - 1)) < H;
  const long b_col = (t < kTHalf ? c0 : H + c0 - kTHalf) + t;
  // (C): tile column c_hi + 32k, rows 8 c_lo..
  const int c_hi = t >> 3, c_lo = t & 7;
  float acc = 0.f;

  for (long tr0 = row_begin & ~(long)(kTRows - 1); tr0 < row_end;
       tr0 += kTRows) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int r = a_row + 16 * k;
      const long gr = tr0 + r;
      if (a_col_ok && gr >= row_begin && gr < row_end) {
        const long ig = gr * 2 * H + c0 + a_slot * 8;
        const ushort8_t dv = *reinterpret_cast<const ushort8_t*>(
            da + gr * H + c0 + a_slot * 8);
        const ushort8_t gv = *reinterpret_cast<const ushort8_t*>(h + ig);
        const ushort8_t uv = *reinterpret_cast<const ushort8_t*>(h + ig + H);
        ushort8_t og, ou;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          unsigned short dg, du;
          dswiglu_elem<false>(dv[j], gv[j], uv[j], no_drop, 0u, 0u, dg, du);
          og[j] = dg;
          ou[j] = du;
        }
        *reinterpret_cast<ushort8_t*>(dh + ig) = og;
        *reinterpret_cast<ushort8_t*>(dh + ig + H) = ou;
        const int sw = (r >> 3) & 7;
        tile[r * kTSlots + (a_slot ^ sw)] = og;
        tile[r * kTSlots + ((a_slot + kTHalfSlots) ^ sw)] = ou;
      }
    }
    lds_barrier();
    // rows and columns outside the chunk or the tensor were not written
    // to the tile; (B) and (C) read none of them
    if (b_col_ok) {
      const long lo = row_begin - tr0, hi = row_end - tr0;
      const int rb = lo > 0 ? (int)lo : 0;
      const int re = hi < kTRows ? (int)hi : kTRows;
      const int slot = t >> 3, e = t & 7;
      for (int r = rb; r < re; ++r)
        acc += widen(tile_s[r * kTCols + ((slot ^ ((r >> 3) & 7)) << 3) + e]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c_hi + 32 * k;
      const long gr = tr0 + c_lo * 8;  // first row of this 8-row group
      if (c0 + (c & (kTHalf - 1)) < H && gr < row_end && gr + 8 > row_begin) {
        const unsigned short* src =
            tile_s + (c_lo * 8) * kTCols + (((c >> 3) ^ c_lo) << 3) + (c & 7);
        const long col = (c < kTHalf ? c0 : H + c0 - kTHalf) + c;
        unsigned short* dst = dht + col * n_rows + gr;
        if (vec_store && gr >= row_begin && gr + 8 <= row_end) {
          ushort8_t o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = src[j * kTCols];
          *reinterpret_cast<ushort8_t*>(dst) = o;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (gr + j >= row_begin && gr + j < row_end) dst[j] = src[j * kTCols];
        }
      }
    }
    lds_barrier();
  }
  if (b_col_ok) part[(long)blockIdx.y * 2 * H + b_col] = acc;
}

// a^T [H, R] from h [R, 2H]: gelu_fwd_t_kernel's tiles, swizzle, segments,
// grid and ragged-edge guards over the OUTPUT's [R, H], with two loads per
// tile vector.
constexpr int kFTile = 64;

__global__ __launch_bounds__(kBlock) void swiglu_fwd_t_kernel(
    const unsigned short* __restrict__ h, unsigned short* __restrict__ y,
    long R, long H, int tiles_per_block) {
  __shared__ SwizzledTile<kFTile> tile;
  const unsigned short* tile_s = reinterpret_cast<const unsigned short*>(tile);
  const DropArgs no_drop = {0u, 1.f, 0u};
  const int t = threadIdx.x;
  // load phase: lane -> row hi + 32k, 16-byte column slot lo;
  // store phase: lane -> column hi + 32k, 8-row group lo
  const int hi = t >> 3, lo = t & 7;
  const long c0 = (long)blockIdx.x * kFTile;
  const bool col_ok = c0 + lo * 8 < H;
  const bool vec_store = (R & 7) == 0;  // output rows 16-byte aligned

  const long tile_begin = (long)blockIdx.y * tiles_per_block;
  for (int it = 0; it < tiles_per_block; ++it) {
    const long r0 = (tile_begin + it) * kFTile;
    if (r0 >= R) break;  // block-uniform
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int r = hi + 32 * k;
      // rows and columns outside the tensor are not written to the tile;
      // the store phase reads none of them
      if (col_ok && r0 + r < R) {
        const unsigned short* src = h + (r0 + r) * 2 * H + c0 + lo * 8;
        const ushort8_t gv = *reinterpret_cast<const ushort8_t*>(src);
        const ushort8_t uv = *reinterpret_cast<const ushort8_t*>(src + H);
        ushort8_t o;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          o[j] = swiglu_elem<false>(gv[j], uv[j], no_drop, 0u, 0u);
        tile_write<kFTile>(tile, r, lo, o);
      }
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = hi + 32 * k;
      const long r = r0 + lo * 8;
      if (c0 + c < H && r < R) {
        const unsigned short* src =
            tile_s + (lo * 8) * kFTile + tile_slot(lo * 8, c >> 3) * 8 + (c & 7);
        unsigned short* dst = y + (c0 + c) * R + r;
        if (vec_store) {  // then r + 8 <= R
          ushort8_t o;
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] = src[j * kFTile];
          *reinterpret_cast<ushort8_t*>(dst) = o;
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (r + j < R) dst[j] = src[j * kFTile];
        }
      }
    }
    lds_barrier();
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every kernel
#define VITFSDP_INSTANTIATE_SWIGLU(DROP_)                                    \
  template __global__ void swiglu_fwd_kernel<DROP_>(                         \
      const ushort8_t*, ushort8_t*, int, long, int, DropArgs);               \
  template __global__ void swiglu_bwd_colsum_kernel<DROP_>(                  \
      const ushort8_t*, const ushort8_t*, ushort8_t*, float*, int, long,     \
      int, DropArgs);
VITFSDP_INSTANTIATE_SWIGLU(false)
VITFSDP_INSTANTIATE_SWIGLU(true)
#undef VITFSDP_INSTANTIATE_SWIGLU
#endif

}  // namespace

#ifdef __HIP_DEVICE_COMPILE__
#pragma clang attribute pop
#endif

#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"

namespace {

// What every entry point asks of h: bf16 [.., 2H] contiguous on the GPU,
// 16-byte aligned, H % 8 == 0.  Returns H.
long check_h(const char* op, const torch::Tensor& h) {
  check_bf16_operand(h, op, "h");
  TORCH_CHECK(h.dim() >= 1 && h.size(-1) > 0 && h.size(-1) % 2 == 0, op,
              ": h's last dim must be 2H (even), got ",
              h.dim() ? h.size(-1) : 0);
  const long H = h.size(-1) / 2;
  TORCH_CHECK(H % 8 == 0, op, ": H must be a multiple of 8, got ", H);
  TORCH_CHECK(H < (1L << 30), op, ": last dim too large");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(h.data_ptr()) % 16 == 0, op,
              ": h must be 16-byte aligned");
  return H;
}

// p == 0: no mask
DropArgs drop_args_or_none(const char* op, double p, long seed, long n) {
  return p != 0.0 ? drop_args(op, p, seed, n) : DropArgs{0u, 1.f, 0u};
}

// Row chunks of the walking kernels: ~2048 blocks in all (256 CUs x 8), at
// least 16 rows per chunk so the partials stay small against the tensor.
constexpr long kWalkBlocks = 2048, kWalkMinRows = 16;

std::vector<int64_t> with_last(const torch::Tensor& t, long last) {
  auto sizes = t.sizes().vec();
  sizes.back() = last;
  return sizes;
}

std::vector<torch::Tensor> swiglu_bwd_run(const char* op, torch::Tensor da,
                                          torch::Tensor h, bool with_t,
                                          double p, long seed) {
  const long H = check_h(op, h);
  check_bf16_operand(da, op, "da");
  TORCH_CHECK(da.device() == h.device(), op, ": da must be on h's device");
  TORCH_CHECK(da.dim() == h.dim() && da.sizes().vec() == with_last(h, H), op,
              ": da must be h's shape with H as the last dim");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(da.data_ptr()) % 16 == 0, op,
              ": da must be 16-byte aligned");
  const long n = da.numel() / H;
  const bool drop_on = p != 0.0;
  TORCH_CHECK(!(with_t && drop_on), op, ": dh^T is made with p == 0 only");
  const DropArgs drop = drop_args_or_none(op, p, seed, n);
  auto dh = torch::empty_like(h);
  auto colsum = torch::empty({2 * H}, h.options());
  torch::Tensor dht;
  if (with_t) dht = torch::empty({2 * H, n}, h.options());
  if (n == 0) {
    colsum.zero_();
    return with_t ? std::vector<torch::Tensor>{dh, colsum, dht}
                  : std::vector<torch::Tensor>{dh, colsum};
  }
  const int grid_x = (int)((H / 8 + kBlock - 1) / kBlock);
  const ChunkPlan cp = chunk_plan(n, grid_x, kWalkBlocks, kWalkMinRows);
  auto part = torch::empty({cp.n_chunks, 2 * H},
                           h.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  const int nvec = (int)(H / 8);
  if (with_t) {
    // the same chunks, so the same partials; only the block shape differs
    hipLaunchKernelGGL(
        swiglu_bwd_colsum_t_kernel,
        dim3((unsigned)((H + kTHalf - 1) / kTHalf), (unsigned)cp.n_chunks),
        dim3(kBlock), 0, stream, (const unsigned short*)da.data_ptr(),
        (const unsigned short*)h.data_ptr(), (unsigned short*)dh.data_ptr(),
        (unsigned short*)dht.data_ptr(), part.data_ptr<float>(), H, n,
        (int)cp.rows_per_chunk);
  } else if (drop_on) {
    hipLaunchKernelGGL(swiglu_bwd_colsum_kernel<true>,
                       dim3(grid_x, (unsigned)cp.n_chunks), dim3(kBlock), 0,
                       stream, (const ushort8_t*)da.data_ptr(),
                       (const ushort8_t*)h.data_ptr(),
                       (ushort8_t*)dh.data_ptr(), part.data_ptr<float>(), nvec,
                       n, (int)cp.rows_per_chunk, drop);
  } else {
    hipLaunchKernelGGL(swiglu_bwd_colsum_kernel<false>,
                       dim3(grid_x, (unsigned)cp.n_chunks), dim3(kBlock), 0,
                       stream, (const ushort8_t*)da.data_ptr(),
                       (const ushort8_t*)h.data_ptr(),
                       (ushort8_t*)dh.data_ptr(), part.data_ptr<float>(), nvec,
                       n, (int)cp.rows_per_chunk, drop);
  }
  HIP_CHECK_LAST();
  colsum_finish(part, colsum, 2 * H, cp.n_chunks, stream);
  if (with_t) return {dh, colsum, dht};
  return {dh, colsum};
}

}  // namespace

// h: bf16 [.., 2H].  Returns dropout(silu(h[.., :H]) * h[.., H:]) [.., H];
// p == 0 is no dropout, 0 < p < 1 the hash mask of seed.
torch::Tensor swiglu_fwd(torch::Tensor h, double p, long seed) {
  const char* op = "swiglu_fwd";
  const long H = check_h(op, h);
  const long n = h.numel() / (2 * H);
  const bool drop_on = p != 0.0;
  const DropArgs drop = drop_args_or_none(op, p, seed, n);
  auto a = torch::empty(with_last(h, H), h.options());
  if (n == 0) return a;
  const int grid_x = (int)((H / 8 + kBlock - 1) / kBlock);
  const ChunkPlan cp = chunk_plan(n, grid_x, kWalkBlocks, kWalkMinRows);
  const dim3 grid(grid_x, (unsigned)cp.n_chunks);
  auto stream = at::cuda::getCurrentCUDAStream();
  if (drop_on) {
    hipLaunchKernelGGL(swiglu_fwd_kernel<true>, grid, dim3(kBlock), 0, stream,
                       (const ushort8_t*)h.data_ptr(),
                       (ushort8_t*)a.data_ptr(), (int)(H / 8), n,
                       (int)cp.rows_per_chunk, drop);
  } else {
    hipLaunchKernelGGL(swiglu_fwd_kernel<false>, grid, dim3(kBlock), 0, stream,
                       (const ushort8_t*)h.data_ptr(),
                       (ushort8_t*)a.data_ptr(), (int)(H / 8), n,
                       (int)cp.rows_per_chunk, drop);
  }
  HIP_CHECK_LAST();
  return a;
}

// (dh like h, colsum bf16 [2H]) from da [.., H] (the gradient of
// swiglu_fwd's result, NOT yet masked) and h
std::vector<torch::Tensor> swiglu_bwd_colsum(torch::Tensor da, torch::Tensor h,
                                             double p, long seed) {
  return swiglu_bwd_run("swiglu_bwd_colsum", da, h, false, p, seed);
}

// (dh, colsum, dh^T [2H, rows]); dh and colsum bit-identical to the plain
// variant's at p == 0
std::vector<torch::Tensor> swiglu_bwd_colsum_t(torch::Tensor da,
                                               torch::Tensor h) {
  return swiglu_bwd_run("swiglu_bwd_colsum_t", da, h, true, 0.0, 0);
}

// h: bf16 [R, 2H] contiguous.  Returns swiglu_fwd(h, 0, 0)^T [H, R]
// contiguous, equal in bits.
torch::Tensor swiglu_fwd_t(torch::Tensor h) {
  const char* op = "swiglu_fwd_t";
  TORCH_CHECK(h.dim() == 2, op, ": 2-D GPU tensor expected");
  const long H = check_h(op, h);
  const long R = h.size(0);
  auto y = torch::empty({H, R}, h.options());
  if (R == 0) return y;
  const TransposePlan p = transpose_plan(R, H, op);
  hipLaunchKernelGGL(swiglu_fwd_t_kernel, p.grid, dim3(kBlock), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const unsigned short*)h.data_ptr(),
                     (unsigned short*)y.data_ptr(), R, H, p.tpb);
  HIP_CHECK_LAST();
  return y;
}
#endif  // VITFSDP_KERNELS_ONLY
