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
//
// With hidden dropout behind the GELU (--mlp_dropout > 0) the same two
// kernels run as their DROP instantiations: dx is the backward of
// dropout(gelu(x)), bit for bit what gelu_dropout_bwd (dropout.hip)
// writes, the mask regenerated from (seed, flattened row, column), and
// the sums run over that dx, dropped zeros included.  Only the element
// formula differs (dgelu_elem below); chunks, tiles and the order of
// every sum are those of the plain instantiations.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "colsum_final.h"
#include "common.h"
#include "gelu_math.h"  // gelu_bwd_one, gelu_erf_f32: shared with dropout.hip
#include "stream_tiles.h"
#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"
#include "transpose.h"  // transpose_plan: gelu_fwd_t moves transpose.hip's tiles
#endif

namespace {

constexpr int kBlock = 256;

// One element of dx.  DROP: the expression of
// hidden_dropout_kernel<kGeluDropBwd>, a dropped element SELECTED to +0.
template <bool DROP>
__device__ __forceinline__ unsigned short dgelu_elem(unsigned short dy,
                                                     unsigned short x,
                                                     const DropArgs& d,
                                                     unsigned row,
                                                     unsigned col) {
  if constexpr (DROP) {
    const bool keep = hash_keep(d.seed, d.thresh, row, col);
    return keep ? f32_to_bf16(
                      gelu_bwd_one(bf16_to_f32(dy) * d.rscale, bf16_to_f32(x)))
                : (unsigned short)0;
  } else {
    return f32_to_bf16(gelu_bwd_one(bf16_to_f32(dy), bf16_to_f32(x)));
  }
}

template <bool DROP>
__global__ __launch_bounds__(kBlock) void gelu_bwd_colsum_kernel(
    const ushort8_t* __restrict__ dy, const ushort8_t* __restrict__ x,
    ushort8_t* __restrict__ dx, float* __restrict__ part, int nvec,
    long n_rows, int rows_per_chunk, DropArgs drop) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  // the column half of the hash does not change along the row walk
  const unsigned c0 = (unsigned)vc * 8u;
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
      out[j] = dgelu_elem<DROP>(dv[j], xv[j], drop, (unsigned)r, c0 + j);
      // the sum is over the ROUNDED values: it equals dx.sum(0)
      acc[j] += bf16_to_f32(out[j]);
    }
    dx[i] = out;
  }
  store_partials8(part + ((long)blockIdx.y * nvec + vc) * 8, acc);
}

// The same, and dx^T [hid, rows] as a third output for the TN weight
// gradient of fc1 (ops/linear.py), so that dx is not read back for a
// transpose.  dx, the partials and hence the column sums are bit-identical
// to gelu_bwd_colsum_kernel's: the chunks are the same, and every
// column's fp32 sum still takes its rows one by one in row order.
//
// The thread-per-vector-column walk above cannot write dx^T in useful
// pieces (16 bytes per thread per row), so a block moves 64-row x
// 256-column tiles, aligned to multiples of 64 rows, through 32 KB of LDS
// in three phases: (A) each thread computes eight 16-byte vectors, writes
// them to dx and to the tile; (B) thread t walks column t down the tile's
// rows of this chunk, adding to its running sum; (C) as in transpose.hip,
// 8 lanes assemble one 128-byte segment of a dx^T row from 16-bit column
// reads.  The tile row holds 32 16-byte slots at slot ^ (row / 8 % 8), so
// the 8 lanes of (C) land in 8 different 4-bank groups.  A chunk is not a
// multiple of 8 rows in general (161 at 32768 x 20480): the 8-row groups
// that straddle a chunk boundary, and every group when rows % 8 != 0, are
// stored by element.
constexpr int kTRows = 64;
constexpr int kTCols = 256;

template <bool DROP>
__global__ __launch_bounds__(kBlock) void gelu_bwd_colsum_t_kernel(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    unsigned short* __restrict__ dx, unsigned short* __restrict__ dxt,
    float* __restrict__ part, long hid, long n_rows, int rows_per_chunk,
    DropArgs drop) {
  __shared__ SwizzledTile<kTCols> tile;
  const unsigned short* tile_s = reinterpret_cast<const unsigned short*>(tile);
  const int t = threadIdx.x;
  const long c0 = (long)blockIdx.x * kTCols;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long row_end = min(row_begin + rows_per_chunk, n_rows);
  const bool vec_store = (n_rows & 7) == 0;  // dx^T rows 16-byte aligned
  const int a_slot = t & 31, a_row = t >> 5;  // (A): rows a_row + 8k
  const bool a_col_ok = c0 + a_slot * 8 < hid;
  const unsigned a_c0 = (unsigned)(c0 + a_slot * 8);  // (A): first column
  const int c_hi = t >> 3, c_lo = t & 7;  // (C): column c_hi + 32k, rows 8 c_lo..
  float acc = 0.f;

  for (long tr0 = row_begin & ~(long)(kTRows - 1); tr0 < row_end;
       tr0 += kTRows) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = a_row + 8 * k;
      const long gr = tr0 + r;
      if (a_col_ok && gr >= row_begin && gr < row_end) {
        const long i = gr * hid + c0 + a_slot * 8;
        const ushort8_t dv = *reinterpret_cast<const ushort8_t*>(dy + i);
        const ushort8_t xv = *reinterpret_cast<const ushort8_t*>(x + i);
        ushort8_t out;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          out[j] =
              dgelu_elem<DROP>(dv[j], xv[j], drop, (unsigned)gr, a_c0 + j);
        *reinterpret_cast<ushort8_t*>(dx + i) = out;
        tile_write<kTCols>(tile, r, a_slot, out);
      }
    }
    __syncthreads();
    // rows and columns outside the chunk or the tensor were not written
    // to the tile; (B) and (C) read none of them
    if (c0 + t < hid) {
      const int rb = (int)max(row_begin - tr0, 0L);
      const int re = (int)min(row_end - tr0, (long)kTRows);
      const int slot = t >> 3, e = t & 7;
      for (int r = rb; r < re; ++r)
        acc += bf16_to_f32(
            tile_s[r * kTCols + (tile_slot(r, slot) << 3) + e]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c_hi + 32 * k;
      const long gr = tr0 + c_lo * 8;  // first row of this 8-row group
      if (c0 + c < hid && gr < row_end && gr + 8 > row_begin) {
        // rows 8 c_lo .. 8 c_lo + 7: tile_slot's XOR is c_lo for all of them
        const unsigned short* src =
            tile_s + (c_lo * 8) * kTCols + (((c >> 3) ^ c_lo) << 3) + (c & 7);
        unsigned short* dst = dxt + (c0 + c) * n_rows + gr;
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
    __syncthreads();
  }
  if (c0 + t < hid) part[(long)blockIdx.y * hid + c0 + t] = acc;
}

// gelu(x)^T [cols, rows] from x [rows, cols]: the act^T operand of fc2's TN
// weight gradient rebuilt from the saved pre-activation, so that the
// forward's gelu(x) need not be kept for the backward (ops/linear.py,
// mlp_fc2_recompute_act).  transpose.hip's plain kernel with the GELU
// applied between the 16-byte load and the LDS write: same 64 x 64 tiles,
// slot swizzle, 128-byte output segments, grid and ragged-edge guards.
// Each element is torch's F.gelu in bits: the exact-erf form in fp32,
// rounded once to bf16.
//
// Compiled without packed fp32 VALU ops (v_pk_mul/add/fma_f32), which the
// compiler may pair the eight elements of a vector into; hence
// lds_barrier (stream_tiles.h).
constexpr int kFTile = 64;

#ifdef __HIP_DEVICE_COMPILE__
__attribute__((target("no-packed-fp32-ops")))
#endif
__global__ __launch_bounds__(kBlock) void gelu_fwd_t_kernel(
    const unsigned short* __restrict__ x, unsigned short* __restrict__ y,
    long R, long C, int tiles_per_block) {
  __shared__ SwizzledTile<kFTile> tile;
  const unsigned short* tile_s = reinterpret_cast<const unsigned short*>(tile);
  const int t = threadIdx.x;
  // load phase: lane -> input row hi + 32k, 16-byte column slot lo;
  // store phase: lane -> input column hi + 32k, 8-row group lo
  const int hi = t >> 3, lo = t & 7;
  const long c0 = (long)blockIdx.x * kFTile;
  const bool col_ok = c0 + lo * 8 < C;
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
        const ushort8_t v =
            *reinterpret_cast<const ushort8_t*>(x + (r0 + r) * C + c0 + lo * 8);
        ushort8_t g;
#pragma unroll
        for (int j = 0; j < 8; ++j)
          g[j] = f32_to_bf16(gelu_erf_f32(bf16_to_f32(v[j])));
        tile_write<kFTile>(tile, r, lo, g);
      }
    }
    lds_barrier();
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int c = hi + 32 * k;
      const long r = r0 + lo * 8;
      if (c0 + c < C && r < R) {
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
#define VITFSDP_INSTANTIATE_DGELU(DROP_)                                     \
  template __global__ void gelu_bwd_colsum_kernel<DROP_>(                    \
      const ushort8_t*, const ushort8_t*, ushort8_t*, float*, int, long,     \
      int, DropArgs);                                                        \
  template __global__ void gelu_bwd_colsum_t_kernel<DROP_>(                  \
      const unsigned short*, const unsigned short*, unsigned short*,         \
      unsigned short*, float*, long, long, int, DropArgs);
VITFSDP_INSTANTIATE_DGELU(false)
VITFSDP_INSTANTIATE_DGELU(true)
#undef VITFSDP_INSTANTIATE_DGELU
#endif

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

// dy, x: bf16 [rows, hid] contiguous (any leading dims), hid % 8 == 0.
// Returns (dx like dy, colsum bf16 [hid]) and, with_t, dx^T [hid, rows].
// DROP: 0 < p < 1 and the seed of the forward's mask; unused otherwise.
template <bool DROP>
std::vector<torch::Tensor> gelu_bwd_colsum_run(const char* op,
                                               torch::Tensor dy,
                                               torch::Tensor x, bool with_t,
                                               double p, long seed) {
  check_bf16_operand(dy, op, "dy");
  check_bf16_operand(x, op, "x");
  TORCH_CHECK(dy.dim() >= 1 && dy.sizes() == x.sizes() &&
                  dy.device() == x.device(),
              op, ": dy and x must have one shape");
  const long hid = dy.size(-1);
  TORCH_CHECK(hid > 0 && hid % 8 == 0, op,
              ": last dim must be a multiple of 8, got ", hid);
  TORCH_CHECK(hid < (1L << 31), op, ": last dim too large");
  const long n = dy.numel() / hid;
  const DropArgs drop =
      DROP ? drop_args(op, p, seed, n) : DropArgs{0u, 1.f, 0u};
  auto dx = torch::empty_like(dy);
  auto colsum = torch::empty({hid}, dy.options());
  torch::Tensor dxt;
  if (with_t) dxt = torch::empty({hid, n}, dy.options());
  if (n == 0) {
    colsum.zero_();
    return with_t ? std::vector<torch::Tensor>{dx, colsum, dxt}
                  : std::vector<torch::Tensor>{dx, colsum};
  }
  const int nvec = (int)(hid / 8);
  // row chunking: ~2048 blocks in all (256 CUs x 8), at least 16 rows
  // per chunk so the partials stay small against the tensor itself
  const int grid_x = (nvec + kBlock - 1) / kBlock;
  const auto [n_chunks, rows_per_chunk] = chunk_plan(n, grid_x, 2048, 16);
  auto part = torch::empty({n_chunks, hid},
                           dy.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (with_t) {
    // the same chunks, so the same partials; only the block shape differs
    hipLaunchKernelGGL(
        gelu_bwd_colsum_t_kernel<DROP>,
        dim3((unsigned)((hid + kTCols - 1) / kTCols), (unsigned)n_chunks),
        dim3(kBlock), 0, stream, (const unsigned short*)dy.data_ptr(),
        (const unsigned short*)x.data_ptr(), (unsigned short*)dx.data_ptr(),
        (unsigned short*)dxt.data_ptr(), part.data_ptr<float>(), hid, n,
        (int)rows_per_chunk, drop);
  } else {
    hipLaunchKernelGGL(gelu_bwd_colsum_kernel<DROP>,
                       dim3(grid_x, (unsigned)n_chunks), dim3(kBlock), 0,
                       stream, (const ushort8_t*)dy.data_ptr(),
                       (const ushort8_t*)x.data_ptr(),
                       (ushort8_t*)dx.data_ptr(), part.data_ptr<float>(), nvec,
                       n, (int)rows_per_chunk, drop);
  }
  HIP_CHECK_LAST();
  colsum_finish(part, colsum, hid, n_chunks, stream);
  if (with_t) return {dx, colsum, dxt};
  return {dx, colsum};
}

}  // namespace

std::vector<torch::Tensor> gelu_bwd_colsum(torch::Tensor dy, torch::Tensor x) {
  return gelu_bwd_colsum_run<false>("gelu_bwd_colsum", dy, x, false, 0.0, 0);
}

std::vector<torch::Tensor> gelu_bwd_colsum_t(torch::Tensor dy,
                                             torch::Tensor x) {
  return gelu_bwd_colsum_run<false>("gelu_bwd_colsum", dy, x, true, 0.0, 0);
}

// (dx, colsum) with dx bit-identical to gelu_dropout_bwd(dy, x, p, seed)
std::vector<torch::Tensor> gelu_dropout_bwd_colsum(torch::Tensor dy,
                                                   torch::Tensor x, double p,
                                                   long seed) {
  return gelu_bwd_colsum_run<true>("gelu_dropout_bwd_colsum", dy, x, false, p,
                                   seed);
}

// (dx, colsum, dx^T); dx and colsum bit-identical to the plain variant's
std::vector<torch::Tensor> gelu_dropout_bwd_colsum_t(torch::Tensor dy,
                                                     torch::Tensor x, double p,
                                                     long seed) {
  return gelu_bwd_colsum_run<true>("gelu_dropout_bwd_colsum", dy, x, true, p,
                                   seed);
}

// x: bf16 [rows, cols] contiguous, cols % 8 == 0.  Returns gelu(x)^T
// [cols, rows] contiguous, each element F.gelu's (exact erf) in bits.
torch::Tensor gelu_fwd_t(torch::Tensor x) {
  const char* op = "gelu_fwd_t";
  check_bf16_operand(x, op, "input");
  TORCH_CHECK(x.dim() == 2, op, ": 2-D tensor expected");
  const long R = x.size(0), C = x.size(1);
  TORCH_CHECK(C > 0 && C % 8 == 0, op,
              ": columns must be a multiple of 8, got ", C);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(x.data_ptr()) % 16 == 0, op,
              ": input must be 16-byte aligned");
  auto y = torch::empty({C, R}, x.options());
  if (R == 0) return y;
  const TransposePlan p = transpose_plan(R, C, op);
  hipLaunchKernelGGL(gelu_fwd_t_kernel, p.grid, dim3(kBlock), 0,
                     at::cuda::getCurrentCUDAStream(),
                     (const unsigned short*)x.data_ptr(),
                     (unsigned short*)y.data_ptr(), R, C, p.tpb);
  HIP_CHECK_LAST();
  return y;
}
#endif  // VITFSDP_KERNELS_ONLY

