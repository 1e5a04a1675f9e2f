// Shared MFMA / LDS building blocks for the hand-written CDNA4 kernels
// (fmha.hip, wgemm.hip, fgemm.hip, probes.hip).  Device-only, no torch
// headers, everything __device__ __forceinline__: each hardware
// convention lives here once, next to the name of the GPU test that
// pins it (tests/test_gpu_kernels.py, probe kernels in probes.hip).
//
// These kernels sit on register-count occupancy steps: a helper's shape
// changes the allocation, so check every new use against
// tools/check_resources.sh (profiles/raw/kernel_resources.txt).
#pragma once

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

// MFMA fragment layouts, lane l of the wave:
//   mfma_f32_16x16x32_bf16 (test_mfma_probe_layout), col = l&15, seg = l>>4
//     A[i][k]: a[j] = A[col][seg*8 + j]
//     B[k][j]: b[j] = B[seg*8 + j][col]
//     C[i][j]: c[r] = C[seg*4 + r][col]
//   mfma_f32_32x32x16_bf16 (test_mfma32_probe_layout)
//     A: a[j] = A[l&31][(l>>5)*8 + j], B: b[j] = B[(l>>5)*8 + j][l&31]
//     C: c[g*4 + r] = C[(l>>5)*4 + g*8 + r][l&31]
//
// ds_read_b64_tr_b16 (test_tr16_probe_semantics): per 16-lane group,
// lane i reads 4 contiguous u16 at its own 8-byte-aligned address; the
// 64 gathered elements form a stream ordered (lane, elem) and lane l
// receives stream[(l&15) + 16*j], j = 0..3.  Reading a [4 row][16 col]
// sub-tile of a row-major LDS tile with lane addresses
// row = base + (i>>2), col = colbase + (i&3)*4 therefore delivers column
// (l&15) of the sub-tile to lane l — a free transpose.  Two such reads
// (rows seg*8 + 4*h, h = 0,1) make one 16x16x32 B (or A^T) fragment.

// one hardware transpose read at an LDS byte address (not yet waited)
__device__ __forceinline__ u32x2 tr16_read(unsigned lds_byte_addr) {
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:0"
               : "=v"(v)
               : "v"(lds_byte_addr));
  return v;
}

// same, at lds_byte_addr + OFF with OFF (< 64 KB) in the instruction's
// immediate: reads that differ by a constant share one address VGPR
template <int OFF>
__device__ __forceinline__ u32x2 tr16_read_at(unsigned lds_byte_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field is 16 bits");
  u32x2 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2"
               : "=v"(v)
               : "v"(lds_byte_addr), "n"(OFF));
  return v;
}

// counted LDS wait: at most N LDS reads still in flight.  The fragment
// halves about to be consumed ride along as "+v" operands so their
// MFMAs cannot be scheduled above the wait (guide rule 18) without
// fencing the whole scheduler.
template <int N>
__device__ __forceinline__ void lds_wait(u32x2& lo, u32x2& hi) {
  asm volatile("s_waitcnt lgkmcnt(%[cnt])"
               : "+v"(lo), "+v"(hi)
               : [cnt] "i"(N)
               : "memory");
}

// the two transpose-read halves (k = seg*8 + 0..3, + 4..7) as one fragment
__device__ __forceinline__ bf16x8 frag_from(u32x2 lo, u32x2 hi) {
  union {
    u32x2 uu[2];
    bf16x8 v;
  } cv;
  cv.uu[0] = lo;
  cv.uu[1] = hi;
  return cv.v;
}

__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  return (unsigned)f32_to_bf16(lo) | ((unsigned)f32_to_bf16(hi) << 16);
}

// acc[c] += A · B_c for NC 16-column chunks, B_c = columns c*16..+16 of
// the 32 rows of a ROW-major LDS tile (row stride STRIDE elements) at
// byte address lds_base, gathered by transpose reads through a 2-deep
// ring with counted waits.  The lane-dependent address is computed once;
// every read is that plus a compile-time offset (recomputing the full
// expression per read costs ~10 VGPRs and spills the attention forward).
template <int NC, int STRIDE>
__device__ __forceinline__ void mfma_tr_ring(bf16x8 a, unsigned lds_base,
                                             int seg, int col,
                                             f32x4 (&acc)[NC]) {
  const unsigned lane_base =
      lds_base +
      2u * (unsigned)((seg * 8 + (col >> 2)) * STRIDE + (col & 3) * 4);
  u32x2 bf[2][2];
#pragma unroll
  for (int h = 0; h < 2; ++h)
    bf[0][h] = tr16_read(lane_base + 2u * (4 * h * STRIDE));
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const int cur = c & 1;
    if (c + 1 < NC) {
#pragma unroll
      for (int h = 0; h < 2; ++h)
        bf[cur ^ 1][h] =
            tr16_read(lane_base + 2u * (4 * h * STRIDE + (c + 1) * 16));
      lds_wait<2>(bf[cur][0], bf[cur][1]);
    } else {
      lds_wait<0>(bf[cur][0], bf[cur][1]);
    }
    acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
        a, frag_from(bf[cur][0], bf[cur][1]), acc[c], 0, 0, 0);
  }
}

// C layout -> A layout without an LDS round-trip.  pk[kk][rr] holds the
// bf16 pair (k = 16*kk + seg*4 + 2*rr, +1) of a [32 k][16 q] C-layout
// tile for q = col.  Target elem pair j2 wants k = seg*8 + 2*j2 of its
// own q = col, which lives in lane col + 16*((seg&1)*2 + (j2>>1)), slot
// (kk = seg>>1, rr = j2&1).  A source lane serves targets from BOTH kk
// halves, so shuffle both kk slots and let each target select by its seg.
__device__ __forceinline__ bf16x8 c_to_a_layout(const unsigned (&pk)[2][2],
                                                int seg, int col) {
  union {
    unsigned u[4];
    bf16x8 v;
  } cvt;
#pragma unroll
  for (int j2 = 0; j2 < 4; ++j2) {
    const int src = col + 16 * ((seg & 1) * 2 + (j2 >> 1));
    const unsigned lo = (unsigned)__shfl((int)pk[0][j2 & 1], src);
    const unsigned hi = (unsigned)__shfl((int)pk[1][j2 & 1], src);
    cvt.u[j2] = (seg >> 1) ? hi : lo;
  }
  return cvt.v;
}

// A/B-layout register fragments of one [.][D] row starting at p (valid =
// row in range): frag[kc][j] = p[kc*32 + seg*8 + j], zero beyond D and
// for invalid rows.  One 16-B load per chunk, scalar tail where a padded
// D cuts the chunk.
template <int NKC, int D>
__device__ __forceinline__ void load_row_frags(const short* __restrict__ p,
                                               bool valid, int seg,
                                               bf16x8 (&frag)[NKC]) {
#pragma unroll
  for (int kc = 0; kc < NKC; ++kc) {
    const int d0 = kc * 32 + seg * 8;
    if (valid && d0 + 8 <= D) {
      frag[kc] = *reinterpret_cast<const bf16x8*>(&p[d0]);
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        frag[kc][j] = (valid && d0 + j < D) ? p[d0 + j] : (short)0;
    }
  }
}

// Register staging of a [ROWS][COLS] bf16 LDS tile (COLS = D padded up,
// columns >= D zero) by a THREADS-thread block, one 16-B vector per
// thread per step: hoisted per-thread (row, column) coordinates, the
// global -> register load and the register -> LDS store.  The callers
// issue the two halves at different points (T14 split staging: next
// tile's loads fly under this tile's MFMAs) and own the registers.
template <int ROWS, int COLS, int D, int THREADS>
struct TileStage {
  static constexpr int VPR = COLS / 8;  // vectors per row
  static constexpr int N = (ROWS * VPR + THREADS - 1) / THREADS;
  int r[N], c[N];
  __device__ __forceinline__ TileStage() {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const int idx = (int)threadIdx.x + i * THREADS;
      r[i] = idx / VPR;
      c[i] = (idx % VPR) * 8;
    }
  }
  // rows row0..row0+ROWS of the T-row tensor p (zero for rows >= T)
  template <int M>
  __device__ __forceinline__ void load(const short* __restrict__ p,
                                       long row_stride, int row0, int T,
                                       bf16x8 (&st)[M]) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      bf16x8 val = {0, 0, 0, 0, 0, 0, 0, 0};
      const int row = row0 + r[i];
      if (r[i] < ROWS && row < T && (COLS <= D || c[i] < D)) {
        val = *reinterpret_cast<const bf16x8*>(
            &p[(long)row * row_stride + c[i]]);
      }
      st[i] = val;
    }
  }
  template <int STRIDE, int M>
  __device__ __forceinline__ void store(short (*tile)[STRIDE],
                                        const bf16x8 (&st)[M]) const {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (r[i] < ROWS) {
        *reinterpret_cast<bf16x8*>(&tile[r[i]][c[i]]) = st[i];
      }
    }
  }
};

// M-major XCD swizzle (guide T1) for a grid of nwg workgroups, nwg % 8
// == 0: the dispatcher places linear block id bid on XCD bid % 8; the
// remap gives each XCD one contiguous run of nwg/8 tiles, so its
// co-resident blocks share operand panels in its private L2.
__device__ __forceinline__ int xcd_swizzle_m_major(int bid, int nwg) {
  return (bid & 7) * (nwg >> 3) + (bid >> 3);
}

// XCD-aware 2D tile clustering for a gridDim.x x gridDim.y grid of
// output tiles (wgemm.hip, fgemm.hip): the dispatcher places block bid
// on XCD bid%8, so each XCD's co-resident ~32 workgroups are
// cid = bid>>3 consecutive.  Give each XCD a contiguous 2D
// sub-rectangle of the tile grid and walk it in GROUP_M-wide bands:
// the resident set then covers a GM x (32/GM) RECTANGLE, reusing x
// panels GM-fold and y panels (32/GM)-fold in the XCD's private L2.
// (An M-major run reuses only one operand; at 1 workgroup/CU the other
// operand's streams alone exceed the per-CU HBM budget — MfmaUtil
// measured 44% on fgemm.)  Grids the 8 sub-rectangles do not divide
// fall back to the M-major run, tile counts that are no multiple of 8
// keep the identity mapping.
__device__ __forceinline__ void xcd_cluster_tile(int& bx, int& by) {
  bx = blockIdx.x;
  by = blockIdx.y;
  const int gx = gridDim.x, gy = gridDim.y;
  const int nwg = gx * gy;
  const int bid = (int)(blockIdx.x + blockIdx.y * gx);
  int sx = 2, sy = 4;  // 8 XCD sub-rectangles
  if (gy % 4 != 0) {
    if (gy % 2 == 0) { sx = 4; sy = 2; }
    else { sx = 8; sy = 1; }
  }
  if ((nwg & 7) == 0 && gx % sx == 0 && gy % sy == 0) {
    const int xcd = bid & 7, cid = bid >> 3;
    const int lw = gx / sx, lh = gy / sy;
    const int gm = (lw % 4 == 0) ? 4 : ((lw % 2 == 0) ? 2 : 1);
    const int per_band = gm * lh;
    const int band = cid / per_band, r = cid % per_band;
    bx = (xcd % sx) * lw + band * gm + (r % gm);
    by = (xcd / sx) * lh + r / gm;
  } else if ((nwg & 7) == 0) {
    const int swz = xcd_swizzle_m_major(bid, nwg);
    bx = swz % gx;
    by = swz / gx;
  }
}
