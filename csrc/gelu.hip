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

#include "colsum_final.h"  // partials -> bf16 sums, shared with transpose.hip
#include "common.h"
#include "gelu_math.h"  // gelu_bwd_one, shared with dropout.hip

namespace {

constexpr int kBlock = 256;

// The mask of the DROP instantiations: element (row, col) is kept iff
// dropout_hash(seed, row, col) >= thresh, and a kept dy is scaled by
// rscale (thresh and rscale as launch<> in dropout.hip computes them).
struct DropArgs {
  unsigned thresh;
  float rscale;
  unsigned seed;
};

// One element of dx.  DROP: the expression of
// hidden_dropout_kernel<kGeluDropBwd>, a dropped element SELECTED to +0.
template <bool DROP>
__device__ __forceinline__ unsigned short dgelu_elem(unsigned short dy,
                                                     unsigned short x,
                                                     const DropArgs& d,
                                                     unsigned row,
                                                     unsigned col) {
  if constexpr (DROP) {
    const bool keep = dropout_hash(d.seed, row, col) >= d.thresh;
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
  float4* p = reinterpret_cast<float4*>(part + ((long)blockIdx.y * nvec + vc) * 8);
  p[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
  p[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
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
constexpr int kTSlots = kTCols / 8;

template <bool DROP>
__global__ __launch_bounds__(kBlock) void gelu_bwd_colsum_t_kernel(
    const unsigned short* __restrict__ dy, const unsigned short* __restrict__ x,
    unsigned short* __restrict__ dx, unsigned short* __restrict__ dxt,
    float* __restrict__ part, long hid, long n_rows, int rows_per_chunk,
    DropArgs drop) {
  __shared__ ushort8_t tile[kTRows * kTSlots];
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
        tile[r * kTSlots + (a_slot ^ ((r >> 3) & 7))] = out;
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
            tile_s[r * kTCols + ((slot ^ ((r >> 3) & 7)) << 3) + e]);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int c = c_hi + 32 * k;
      const long gr = tr0 + c_lo * 8;  // first row of this 8-row group
      if (c0 + c < hid && gr < row_end && gr + 8 > row_begin) {
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
  TORCH_CHECK(dy.is_cuda() && x.is_cuda() && dy.is_contiguous() &&
                  x.is_contiguous(),
              op, ": contiguous GPU tensors");
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
                  x.scalar_type() == torch::kBFloat16,
              op, ": bf16 only");
  TORCH_CHECK(dy.dim() >= 1 && dy.sizes() == x.sizes() &&
                  dy.device() == x.device(),
              op, ": dy and x must have one shape");
  const long hid = dy.size(-1);
  TORCH_CHECK(hid > 0 && hid % 8 == 0, op,
              ": last dim must be a multiple of 8, got ", hid);
  TORCH_CHECK(hid < (1L << 31), op, ": last dim too large");
  const long n = dy.numel() / hid;
  DropArgs drop = {0u, 1.f, 0u};
  if (DROP) {
    TORCH_CHECK(p > 0.0 && p < 1.0, op, ": p must be in (0, 1), got ", p);
    // the hash takes the flattened row as 32 bits
    TORCH_CHECK(n < (1L << 32), op, ": rows must be below 2^32");
    // in double, exactly as launch<> in dropout.hip
    const uint64_t t64 = (uint64_t)(p * 4294967296.0);
    drop.thresh = t64 > 4294967295ull ? 4294967295u : (unsigned)t64;
    drop.rscale = (float)(1.0 / (1.0 - p));
    drop.seed = (unsigned)seed;
  }
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
  long n_chunks = std::max(1, 2048 / grid_x);
  long rows_per_chunk = std::max<long>((n + n_chunks - 1) / n_chunks, 16);
  n_chunks = (n + rows_per_chunk - 1) / rows_per_chunk;
  TORCH_CHECK(n_chunks <= 65535, op, ": too many rows");
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
  hipLaunchKernelGGL(colsum_final_kernel, colsum_final_grid(hid),
                     dim3(kColsumFinalBlock), 0, stream, part.data_ptr<float>(),
                     (unsigned short*)colsum.data_ptr(), (int)hid,
                     (int)n_chunks);
  HIP_CHECK_LAST();
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
#endif  // VITFSDP_KERNELS_ONLY

