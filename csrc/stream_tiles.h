// Device building blocks of the memory-bound streaming kernels: the
// counterpart of mfma_tiles.h for dropout.hip, drop_path.hip,
// layer_scale.hip, gelu.hip, swiglu.hip and transpose.hip (qk_norm.hip
// takes widen, qk_rmsnorm.hip widen and lds_barrier).
//
// All __forceinline__ and written with builtins only.  From a kernel
// compiled without packed fp32 ops by a target attribute, a plain-inline
// HIP header function (__uint_as_float, make_float4, __syncthreads, ...),
// which has the default target features, is CALLED, per element, instead
// of inlined.  A file that pushes that attribute with `#pragma clang
// attribute` includes this header inside the pushed region.
#pragma once

#include "common.h"

// Unnamed, as the namespace of the kernels: a kernel's symbol, which
// profiles and traces key on, spells the namespace of its DropArgs argument.
namespace {

typedef float float4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float widen(unsigned short u) {
  return __builtin_bit_cast(float, (unsigned)u << 16);
}

// __syncthreads by builtin
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// THE keep test of the hash masks: element (row, col) of a [rows, C]
// tensor, row the flattened row, or sample (b, 0) of stochastic depth, is
// kept iff the hash reaches thresh = hash_thresh(p) (stream_host.h).
__device__ __forceinline__ bool hash_keep(unsigned seed, unsigned thresh,
                                          unsigned row, unsigned col) {
  return dropout_hash(seed, row, col) >= thresh;
}

// An element mask as one kernel argument (drop_args, stream_host.h); a
// kept value is scaled by rscale = 1 / (1 - p).
struct DropArgs {
  unsigned thresh;
  float rscale;
  unsigned seed;
};

// A thread's eight fp32 column sums as one 32-byte segment of a partials
// row (32-byte aligned: the columns are a multiple of 8).
__device__ __forceinline__ void store_partials8(float* p,
                                                const float (&acc)[8]) {
  float4_t* q = reinterpret_cast<float4_t*>(p);
  q[0] = float4_t{acc[0], acc[1], acc[2], acc[3]};
  q[1] = float4_t{acc[4], acc[5], acc[6], acc[7]};
}

// The swizzled transpose tile: 64 rows x COLS bf16 columns in LDS, a row
// COLS / 8 16-byte slots, slot s of row r stored at s ^ (r / 8 % 8).  The
// load phase writes whole 16-byte vectors; in the store phase the 8 lanes
// that assemble one 128-byte segment of an output row (one column of tile
// rows 8 lo .. 8 lo + 7, lo = 0..7) land in 8 different 4-bank groups, so
// the 16-bit column reads are free of bank conflicts without padding.  The
// XOR touches the low three slot bits only: at COLS = 256 each half of a
// row stays in its own 16 slots.
template <int COLS>
using SwizzledTile = ushort8_t[64 * COLS / 8];

__device__ __forceinline__ int tile_slot(int row, int slot) {
  return slot ^ ((row >> 3) & 7);
}

template <int COLS>
__device__ __forceinline__ void tile_write(SwizzledTile<COLS>& tile, int row,
                                           int slot, ushort8_t v) {
  // the row first, then the slot: the order the compiler gives tile[i]
  ushort8_t* row_p = tile + row * (COLS / 8);
  row_p[tile_slot(row, slot)] = v;
}

}  // namespace
