// Flash-style fused multi-head attention for CDNA4 (kernel K4,
// SURVEY.md §2D): per-head softmax(Q K^T * scale) V with online softmax,
// O(T) memory, for the ViT-10B head_dim of 160 (= 5120/32, reference
// run_vit_training.py:341-342) — off the usual 64/128 fast paths, so the
// tiling is D-generic over 32-wide MFMA K-chunks (160 = 5 x 32).
//
// head_dim is a TEMPLATE parameter: every fragment/accumulator loop is
// compile-time bounded so the f32x4 MFMA accumulators stay in VGPRs — a
// runtime-indexed ext_vector array silently spills to scratch, which
// measured ~300x slower (guide §5.4 rule 20; seen in the first profile,
// profiles/).
//
// Structure (forward):
//   grid = (B*H, ceil(T/QTile)); block = 256 threads = 4 waves; K/V
//   tiles double-buffered in LDS with T14 split staging (next tile's
//   HBM loads issue before this tile's MFMA phases), one barrier/tile.
//   Per 32-key tile:
//     - SWAPPED S^T = K Q^T via __builtin_amdgcn_mfma_f32_16x16x32_bf16
//       (C-layout rows = k, cols = q: each lane owns ONE q row),
//     - fully in-register online softmax (7 fmax + 2 cross-seg shuffles
//       per row; state = two scalars per lane),
//     - P re-enters the MFMA A layout via 4 packed bf16-pair shuffles
//       (no LDS round-trip, no lgkmcnt drain),
//     - O += P V with B fragments gathered from the ROW-major V tile
//       by ds_read_b64_tr_b16 hardware transpose reads (2-deep ring).
//   Epilogue: O /= rowsum, store bf16, write LSE (fp32) for backward.
//
// Backward: fully fused (FlashAttention-2 style), two MFMA kernels —
// fmha_bwd_dq (q-tile ownership) and fmha_bwd_dkv (k-tile ownership),
// both recompute P from the forward LSE; Delta = rowsum(dO*O) is its
// own reduction kernel.  No batched GEMM library calls (the hipBLASLt
// composition survives as a debug path, VITFSDP_FMHA_BWD=compose).
//
// MFMA fragment layouts, transpose-read semantics and the shared
// ring / pack / reshuffle / fragment-load helpers: mfma_tiles.h.

// Compile with -DVITFSDP_KERNELS_ONLY to build just the device kernels
// (no torch headers) — used by csrc/tools/check_resources.sh for
// -Rpass-analysis=kernel-resource-usage without the extension build.
#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <cstdlib>
#include <cstring>
#include <type_traits>
#endif

#include "mfma_tiles.h"

namespace {

constexpr int kBlockThreads = 256;
constexpr int kKTile = 32;  // k rows per inner iteration
constexpr int kMaxD = 192;  // supports head_dim up to 192 (10B uses 160)

template <int D>
struct FmhaShapes {
  // 16-row q sub-tiles per wave: 2 where the register budget allows >=2
  // waves/SIMD occupancy; 1 for large head_dim (at D=160, QSub=2 costs
  // 228 VGPR + 80 AGPR -> 1 wave/SIMD, measured slower than QSub=1)
  static constexpr int QSub = (D <= 96) ? 2 : 1;
  static constexpr int QTile = 64 * QSub;  // q rows per workgroup
  static constexpr int DP = ((D + 31) / 32) * 32;  // zero-padded for QK
  static constexpr int NKC = DP / 32;              // QK^T K-chunks
  static constexpr int NC = D / 16;                // PV / O column chunks
  // LDS row strides in elements, padded so the 16-lane ds_read_b128
  // column groups land on distinct banks (stride*2B stays 16B-aligned)
  static constexpr int KStride = DP + 8;
  static constexpr int PStride = kKTile + 8;  // 40
  static constexpr int VRow = D + 16;  // row-major V: 8B-aligned tr
                                       // lanes, conflict-free groups
  struct Shared {
    short k_tile[2][kKTile][KStride];  // double-buffered
    short v_tile[2][kKTile][VRow];     // ROW-major [k][d], dbuf: PV reads
                                       // it via ds_read_b64_tr_b16
  };
  // The backward kernels keep ONLY row-major tiles: the operands that
  // need K-contiguous fragments (dQ's K, dKV's Q/dO) are read with
  // ds_read_b64_tr_b16 hardware transpose reads, so the element-wise
  // transposed copies (and their bank-conflict swizzles) are gone.
  struct SharedDQ {
    short k_tile[kKTile][KStride];  // row-major (S^T + dQ operands)
    short v_tile[kKTile][KStride];  // row-major (dP^T operand)
  };
  struct SharedDKV {
    short q_tile[32][KStride];    // row-major (S^T + dK operands)
    short do_tile[32][KStride];   // row-major (dP^T + dV operands)
    short pt_tile[4][16][PStride];   // P^T re-layout per wave
    short dst_tile[4][16][PStride];  // dS^T re-layout per wave
  };
};


// grid = (B*H, ceil(T/kQTile)): bh on x so a head's q-tiles share the
// XCD whose L2 already holds its K/V (blockIdx linearization round-
// robins x across XCDs; y strides keep bh%8 constant -> same XCD)
// Strides (in elements, d innermost contiguous): the q/k/v pointers
// share one stride set (they are views of the fused qkv projection
// [B,T,3,H,D]); o has its own (it is written [B,T,H,D] = [B,T,E], so the
// attention module needs no permute/contiguous copies on either side).
struct QkvStrides {
  long qb, qh, qt;  // q/k/v batch, head, token strides
  long ob, oh, ot;  // o (and dO) strides
};

// Attention-dropout mask: dropout_hash (common.h) of (seed, global q row
// incl. bh, k column), so forward and both backward kernels regenerate
// the identical mask with no stored bits.

template <int D, bool DROP = false>
// min 3 waves/SIMD: the double-buffered staging otherwise lands at
// 182 regs -> 2 waves; forcing 3 costs a few prologue spills at most
__global__ __launch_bounds__(kBlockThreads, 3) void fmha_fwd_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, short* __restrict__ o,
    float* __restrict__ lse_out, int T, int H, QkvStrides st, float scale,
    unsigned drop_thresh = 0, float drop_rscale = 1.f, unsigned seed = 0) {
  using S = FmhaShapes<D>;
  constexpr int DP = S::DP, NKC = S::NKC, NC = S::NC;
  constexpr int kQSub = S::QSub;
  constexpr int kQTile = S::QTile;
  HIP_DYNAMIC_SHARED(char, smem_raw)
  typename S::Shared& sm = *reinterpret_cast<typename S::Shared*>(smem_raw);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;  // fragment column group
  const int seg = lane >> 4;  // fragment k/row segment (0..3)
  const long bh = blockIdx.x;
  const int q_base = blockIdx.y * kQTile;
  // this wave's first q row, per sub-tile qs: q_row0 + 16*qs
  const int q_row0 = q_base + wave * (16 * kQSub);

  const int b_idx = (int)(bh / H), h_idx = (int)(bh % H);
  const long qkv_off = (long)b_idx * st.qb + (long)h_idx * st.qh;
  const long o_off = (long)b_idx * st.ob + (long)h_idx * st.oh;

  // ---- hoisted staging coordinates (reused every K/V tile): the K
  // tile is zero-padded to DP columns for QK^T, the V tile is D wide ----
  using KStage = TileStage<kKTile, DP, D, kBlockThreads>;
  using VStage = TileStage<kKTile, D, D, kBlockThreads>;
  const KStage k_stg;
  const VStage v_stg;

  // ---- load Q fragments to registers: sub-tile qs, chunk kc, elem j ->
  // Q[q_row0 + 16*qs + col][seg*8 + j + 32*kc] (zero-padded beyond D/T) --
  bf16x8 q_frag[kQSub][NKC];
#pragma unroll
  for (int qs = 0; qs < kQSub; ++qs) {
    const int q_row = q_row0 + 16 * qs + col;
    load_row_frags<NKC, D>(q + qkv_off + (long)q_row * st.qt, q_row < T, seg,
                           q_frag[qs]);
  }

  // ---- online softmax state: ONE q row per lane (q = col) ----
  float m_run[kQSub], l_run[kQSub];
  f32x4 o_acc[kQSub][NC];
#pragma unroll
  for (int qs = 0; qs < kQSub; ++qs) {
    m_run[qs] = -INFINITY;
    l_run[qs] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) o_acc[qs][c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging helpers (double-buffered K/V, T14 split: the NEXT
  // tile's global loads are issued before this tile's compute so HBM
  // latency hides under the MFMA phases; the LDS writes land after) ----
  // K and V staging share one register block: their live ranges are
  // disjoint (K: issue -> write before PV; V: issue -> write after PV)
  bf16x8 stage[KStage::N > VStage::N ? KStage::N : VStage::N];
  auto issue_k_loads = [&](int k_base) {
    k_stg.load(k + qkv_off, st.qt, k_base, T, stage);
  };
  auto write_k_tile = [&](int buf) { k_stg.store(sm.k_tile[buf], stage); };
  auto issue_v_loads = [&](int k_base) {
    v_stg.load(v + qkv_off, st.qt, k_base, T, stage);
  };
  auto write_v_tile = [&](int buf) { v_stg.store(sm.v_tile[buf], stage); };

  const int n_ktiles = (T + kKTile - 1) / kKTile;
  // prologue: stage tile 0 into buffer 0
  issue_k_loads(0);
  write_k_tile(0);
  issue_v_loads(0);
  write_v_tile(0);
  __syncthreads();

  int cur = 0;
  for (int kt = 0; kt < n_ktiles; ++kt) {
    const int k_base = kt * kKTile;
    const bool has_next = kt + 1 < n_ktiles;

    // issue next K loads; their latency hides under this tile's QK^T
    if (has_next) issue_k_loads(k_base + kKTile);

    // ---- per q sub-tile: S^T = scale*(K Q^T), in-register softmax ----
    // Swapped operands (guide §B attn): mfma(A=K, B=Q) puts the scores
    // in C layout rows = k, cols = q — each lane holds the 8 scores of
    // ONE q row (q = col), so the row reduce is 7 in-register ops plus
    // two cross-seg shuffles, the softmax state is two scalars per
    // lane, and P returns to the MFMA A layout with four packed
    // shuffles instead of an LDS round-trip + lgkmcnt(0) drain.
    // Q's register fragments serve both orders: its A-layout fragment
    // (lane: Q[col][seg*8+j]) IS its B-layout fragment for the swap.
#pragma unroll
    for (int qs = 0; qs < kQSub; ++qs) {
      f32x4 st_frag[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
          // A fragment: A[col][seg*8+j] = K[kk*16+col][kc*32+seg*8+j]
          bf16x8 a_frag = *reinterpret_cast<const bf16x8*>(
              &sm.k_tile[cur][kk * 16 + col][kc * 32 + seg * 8]);
          st_frag[kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag, q_frag[qs][kc], st_frag[kk], 0, 0, 0);
        }
      }

      // lane's 8 scores: q = col, k = k_base + 16*kk + seg*4 + r
      float sc[2][4];
      float my_max = -INFINITY;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float sv = st_frag[kk][r] * scale;
          if (k_base + 16 * kk + seg * 4 + r >= T) sv = -INFINITY;
          sc[kk][r] = sv;
          my_max = fmaxf(my_max, sv);
        }
      }
      my_max = fmaxf(my_max, __shfl_xor(my_max, 16));
      my_max = fmaxf(my_max, __shfl_xor(my_max, 32));
      const float m_new = fmaxf(m_run[qs], my_max);
      const float alpha = __expf(m_run[qs] - m_new);
      m_run[qs] = m_new;

      float p[2][4];
      float row_sum = 0.f;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float pv =
              (sc[kk][r] == -INFINITY) ? 0.f : __expf(sc[kk][r] - m_new);
          p[kk][r] = pv;
          row_sum += pv;
        }
      }
      row_sum += __shfl_xor(row_sum, 16);
      row_sum += __shfl_xor(row_sum, 32);
      l_run[qs] = l_run[qs] * alpha + row_sum;

      if (DROP) {
        // dropout on P (post-softmax, reference nn.Dropout semantics):
        // the row sum above stays UNMASKED (it is the softmax
        // normalizer); the PV path gets the masked, 1/(1-p)-scaled P
        const unsigned qg = (unsigned)(bh * T + q_row0 + 16 * qs + col);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const unsigned kg = (unsigned)(k_base + 16 * kk + seg * 4 + r);
            p[kk][r] = dropout_hash(seed, qg, kg) >= drop_thresh
                           ? p[kk][r] * drop_rscale
                           : 0.f;
          }
        }
      }

      // pack P to bf16 pairs (consecutive k): pk[kk][rr] holds
      // (k = 16*kk + seg*4 + 2*rr, +1) for q = col
      unsigned pk[2][2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int rr = 0; rr < 2; ++rr)
          pk[kk][rr] = pack_bf16x2(p[kk][2 * rr], p[kk][2 * rr + 1]);
      }
      const bf16x8 pa = c_to_a_layout(pk, seg, col);

      // rescale O: its C-layout rows are q = seg*4 + r, whose alpha
      // lives in lane (seg*4 + r) of the column group
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float alpha_o = __shfl(alpha, seg * 4 + r);
#pragma unroll
        for (int c = 0; c < NC; ++c) o_acc[qs][c][r] *= alpha_o;
      }

      // K(t+1) in flight and QK^T(t) done for the LAST sub-tile: write
      // it, then issue V(t+1) loads to hide under PV
      if (qs == kQSub - 1 && has_next) {
        write_k_tile(cur ^ 1);
        issue_v_loads(k_base + kKTile);
      }

      // ---- O += P V : NC chunks of 16 output columns ----
      // B fragments come from the ROW-major V tile via
      // transpose reads (mfma_tr_ring): the element-wise transposed
      // store and its bank-conflict swizzle are gone entirely.
      const unsigned v_lds_base =
          (unsigned)__builtin_amdgcn_groupstaticsize() +
          (unsigned)(offsetof(typename S::Shared, v_tile)) +
          (unsigned)cur * (unsigned)sizeof(sm.v_tile[0]);
      mfma_tr_ring<NC, S::VRow>(pa, v_lds_base, seg, col, o_acc[qs]);
    }

    if (has_next) write_v_tile(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }

  // ---- epilogue: normalize, store O and LSE ----
#pragma unroll
  for (int qs = 0; qs < kQSub; ++qs) {
    // this lane's own row stats (q = col) feed the LSE store; the O
    // rows it holds (q = seg*4 + r) read their l from the owning lane
    if (seg == 0) {
      const int q_row = q_row0 + 16 * qs + col;
      if (q_row < T) {
        lse_out[bh * T + q_row] = m_run[qs] + __logf(l_run[qs]);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float l_row = __shfl(l_run[qs], seg * 4 + r);
      const int q_row = q_row0 + 16 * qs + seg * 4 + r;
      if (q_row >= T) continue;
      const float inv_l = (l_row > 0.f) ? 1.f / l_row : 0.f;
      const long out_base = o_off + (long)q_row * st.ot;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        o[out_base + c * 16 + col] =
            (short)f32_to_bf16(o_acc[qs][c][r] * inv_l);
      }
    }
  }
}

template <int D, bool DROP = false>
__global__ __launch_bounds__(kBlockThreads, 3) void fmha_bwd_dq_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dq, int T, int H, QkvStrides st, float scale,
    unsigned drop_thresh = 0, float drop_rscale = 1.f, unsigned seed = 0) {
  using S = FmhaShapes<D>;
  constexpr int DP = S::DP, NKC = S::NKC, NC = S::NC;
  constexpr int kQSub = S::QSub;
  constexpr int kQTile = S::QTile;
  HIP_DYNAMIC_SHARED(char, smem_raw)
  typename S::SharedDQ& sm =
      *reinterpret_cast<typename S::SharedDQ*>(smem_raw);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int seg = lane >> 4;
  const long bh = blockIdx.x;
  const int q_base = blockIdx.y * kQTile;
  const int q_row0 = q_base + wave * (16 * kQSub);
  const int b_idx = (int)(bh / H), h_idx = (int)(bh % H);
  const long qkv_off = (long)b_idx * st.qb + (long)h_idx * st.qh;
  const long o_off = (long)b_idx * st.ob + (long)h_idx * st.oh;

  // Q and dO register fragments: the same registers serve as the B
  // operands of the swapped S^T / dP^T products (see the forward)
  bf16x8 q_frag[kQSub][NKC], do_frag[kQSub][NKC];
  float lse_q[kQSub], delta_q[kQSub];
#pragma unroll
  for (int qs = 0; qs < kQSub; ++qs) {
    const int q_row = q_row0 + 16 * qs + col;
    const bool valid = q_row < T;
    load_row_frags<NKC, D>(q + qkv_off + (long)q_row * st.qt, valid, seg,
                           q_frag[qs]);
    load_row_frags<NKC, D>(dout + o_off + (long)q_row * st.ot, valid, seg,
                           do_frag[qs]);
    // per-lane row stats: this lane's q row is q = col (swapped layout)
    lse_q[qs] = valid ? lse[bh * T + q_row] : 0.f;
    delta_q[qs] = valid ? delta[bh * T + q_row] : 0.f;
  }

  f32x4 dq_acc[kQSub][NC];
#pragma unroll
  for (int qs = 0; qs < kQSub; ++qs)
#pragma unroll
    for (int c = 0; c < NC; ++c) dq_acc[qs][c] = f32x4{0.f, 0.f, 0.f, 0.f};

  // register staging for the K/V tiles (one coordinate set serves both)
  using Stage = TileStage<kKTile, DP, D, kBlockThreads>;
  const Stage stg;
  bf16x8 kst[Stage::N], vst[Stage::N];
  auto issue_kv_loads = [&](int k_base) {
    stg.load(k + qkv_off, st.qt, k_base, T, kst);
    stg.load(v + qkv_off, st.qt, k_base, T, vst);
  };
  auto write_kv_tiles = [&]() {
    stg.store(sm.k_tile, kst);
    stg.store(sm.v_tile, vst);
  };

  const int n_ktiles = (T + kKTile - 1) / kKTile;
  issue_kv_loads(0);
  write_kv_tiles();
  __syncthreads();
  for (int kt = 0; kt < n_ktiles; ++kt) {
    const int k_base = kt * kKTile;
    const bool has_next = kt + 1 < n_ktiles;
    // next tile's HBM loads fly under this tile's MFMA phases (T14)
    if (has_next) issue_kv_loads(k_base + kKTile);

#pragma unroll
    for (int qs = 0; qs < kQSub; ++qs) {
      // swapped: S^T = K Q^T, dP^T = V dO^T — C rows = k, cols = q, so
      // each lane owns one q row (q = col) like the forward
      f32x4 st_frag[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
      f32x4 dpt_frag[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int kc = 0; kc < NKC; ++kc) {
          bf16x8 kb = *reinterpret_cast<const bf16x8*>(
              &sm.k_tile[kk * 16 + col][kc * 32 + seg * 8]);
          bf16x8 vb = *reinterpret_cast<const bf16x8*>(
              &sm.v_tile[kk * 16 + col][kc * 32 + seg * 8]);
          st_frag[kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              kb, q_frag[qs][kc], st_frag[kk], 0, 0, 0);
          dpt_frag[kk] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              vb, do_frag[qs][kc], dpt_frag[kk], 0, 0, 0);
        }
      }

      // dS = scale * exp(scale*S - lse) * (dP - Delta), packed to bf16
      // pairs along k (k = k_base + 16*kk + seg*4 + r for q = col)
      unsigned pk[2][2];
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
          float ds[2] = {0.f, 0.f};
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            const int r = 2 * rr + h;
            const int k_idx = k_base + 16 * kk + seg * 4 + r;
            if (k_idx < T) {
              const float pv =
                  __expf(st_frag[kk][r] * scale - lse_q[qs]);
              float dp = dpt_frag[kk][r];
              if (DROP) {
                // dP = dPD * D (gradient through the dropout mask)
                const unsigned qg = (unsigned)(bh * T + q_row0 + 16 * qs + col);
                dp = dropout_hash(seed, qg, (unsigned)k_idx) >= drop_thresh
                         ? dp * drop_rscale
                         : 0.f;
              }
              ds[h] = scale * pv * (dp - delta_q[qs]);
            }
          }
          pk[kk][rr] = pack_bf16x2(ds[0], ds[1]);
        }
      }
      const bf16x8 ds_frag = c_to_a_layout(pk, seg, col);

      // dQ += dS K: B fragments from the row-major K tile via hardware
      // transpose reads
      const unsigned k_lds_base =
          (unsigned)__builtin_amdgcn_groupstaticsize() +
          (unsigned)offsetof(typename S::SharedDQ, k_tile);
      mfma_tr_ring<NC, S::KStride>(ds_frag, k_lds_base, seg, col,
                                   dq_acc[qs]);
    }

    if (has_next) {
      __syncthreads();  // all reads of tile kt done
      write_kv_tiles();
      __syncthreads();  // tile kt+1 staged
    }
  }

#pragma unroll
  for (int qs = 0; qs < kQSub; ++qs) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q_row = q_row0 + 16 * qs + seg * 4 + r;
      if (q_row >= T) continue;
      const long out_base = qkv_off + (long)q_row * st.qt;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        dq[out_base + c * 16 + col] = (short)f32_to_bf16(dq_acc[qs][c][r]);
      }
    }
  }
}

template <int D, bool DROP = false>
__global__ __launch_bounds__(kBlockThreads, 2) void fmha_bwd_dkv_kernel(
    const short* __restrict__ q, const short* __restrict__ k,
    const short* __restrict__ v, const short* __restrict__ dout,
    const float* __restrict__ lse, const float* __restrict__ delta,
    short* __restrict__ dk, short* __restrict__ dv, int T, int H,
    QkvStrides st, float scale,
    unsigned drop_thresh = 0, float drop_rscale = 1.f, unsigned seed = 0) {
  using S = FmhaShapes<D>;
  constexpr int DP = S::DP, NKC = S::NKC, NC = S::NC;
  constexpr int kQStream = 32;  // q rows streamed per iteration
  HIP_DYNAMIC_SHARED(char, smem_raw)
  typename S::SharedDKV& sm =
      *reinterpret_cast<typename S::SharedDKV*>(smem_raw);

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int col = lane & 15;
  const int seg = lane >> 4;
  const long bh = blockIdx.x;
  const int k_base = blockIdx.y * 64;     // workgroup's 64 k rows
  const int k_row0 = k_base + wave * 16;  // this wave's 16 k rows
  const int b_idx = (int)(bh / H), h_idx = (int)(bh % H);
  const long qkv_off = (long)b_idx * st.qb + (long)h_idx * st.qh;
  const long o_off = (long)b_idx * st.ob + (long)h_idx * st.oh;

  // K and V fragments in registers (A operands of S^T and dP^T)
  bf16x8 k_frag[NKC], v_frag[NKC];
  {
    const int k_row = k_row0 + col;
    const long base = qkv_off + (long)k_row * st.qt;
    load_row_frags<NKC, D>(k + base, k_row < T, seg, k_frag);
    load_row_frags<NKC, D>(v + base, k_row < T, seg, v_frag);
  }

  f32x4 dk_acc[NC], dv_acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    dk_acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    dv_acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // register staging for the q/dO tiles (one coordinate set serves both)
  using Stage = TileStage<kQStream, DP, D, kBlockThreads>;
  const Stage stg;
  bf16x8 q_st[Stage::N], do_st[Stage::N];
  auto issue_qdo_loads = [&](int q_base) {
    stg.load(q + qkv_off, st.qt, q_base, T, q_st);
    stg.load(dout + o_off, st.ot, q_base, T, do_st);
  };
  auto write_qdo_tiles = [&]() {
    stg.store(sm.q_tile, q_st);
    stg.store(sm.do_tile, do_st);
  };

  const int n_qtiles = (T + kQStream - 1) / kQStream;
  issue_qdo_loads(0);
  write_qdo_tiles();
  __syncthreads();
  for (int qt = 0; qt < n_qtiles; ++qt) {
    const int q_base = qt * kQStream;
    const bool has_next = qt + 1 < n_qtiles;
    // next tile's HBM loads fly under this tile's MFMA phases (T14)
    if (has_next) issue_qdo_loads(q_base + kQStream);

    // S^T and dP^T: [16 k][32 q]
    f32x4 st_frag[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    f32x4 dpt_frag[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
#pragma unroll
      for (int kc = 0; kc < NKC; ++kc) {
        bf16x8 qb = *reinterpret_cast<const bf16x8*>(
            &sm.q_tile[qq * 16 + col][kc * 32 + seg * 8]);
        bf16x8 dob = *reinterpret_cast<const bf16x8*>(
            &sm.do_tile[qq * 16 + col][kc * 32 + seg * 8]);
        st_frag[qq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            k_frag[kc], qb, st_frag[qq], 0, 0, 0);
        dpt_frag[qq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            v_frag[kc], dob, dpt_frag[qq], 0, 0, 0);
      }
    }

    // P^T = exp(scale*S^T - lse[q]); dS^T = scale*P^T*(dP^T - Delta[q])
#pragma unroll
    for (int qq = 0; qq < 2; ++qq) {
      const int q_idx = q_base + qq * 16 + col;
      const bool q_ok = q_idx < T;
      const float l = q_ok ? lse[bh * T + q_idx] : 0.f;
      const float dlt = q_ok ? delta[bh * T + q_idx] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pt = 0.f, dst = 0.f;
        if (q_ok) {
          pt = __expf(st_frag[qq][r] * scale - l);
          float dp = dpt_frag[qq][r];
          if (DROP) {
            const unsigned qg = (unsigned)(bh * T + q_idx);
            const unsigned kg = (unsigned)(k_row0 + seg * 4 + r);
            const bool keep = dropout_hash(seed, qg, kg) >= drop_thresh;
            dp = keep ? dp * drop_rscale : 0.f;
            dst = scale * pt * (dp - dlt);
            // dV uses the MASKED P (the forward multiplied PD into V)
            pt = keep ? pt * drop_rscale : 0.f;
          } else {
            dst = scale * pt * (dp - dlt);
          }
        }
        sm.pt_tile[wave][seg * 4 + r][qq * 16 + col] =
            (short)f32_to_bf16(pt);
        sm.dst_tile[wave][seg * 4 + r][qq * 16 + col] =
            (short)f32_to_bf16(dst);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    bf16x8 pt_frag = *reinterpret_cast<const bf16x8*>(
        &sm.pt_tile[wave][col][seg * 8]);
    bf16x8 dst_frag = *reinterpret_cast<const bf16x8*>(
        &sm.dst_tile[wave][col][seg * 8]);
    // dV += P^T dO, dK += dS^T Q: B fragments from the row-major tiles
    // via hardware transpose reads.  TWO sequential passes (dV then dK),
    // each with a single-operand 2-deep ring: the combined dual ring
    // costed 8 more live registers and pushed the kernel to 266 regs /
    // 1 wave/SIMD.
    const unsigned base0 = (unsigned)__builtin_amdgcn_groupstaticsize();
    const unsigned q_lds_base =
        base0 + (unsigned)offsetof(typename S::SharedDKV, q_tile);
    const unsigned do_lds_base =
        base0 + (unsigned)offsetof(typename S::SharedDKV, do_tile);
    mfma_tr_ring<NC, S::KStride>(pt_frag, do_lds_base, seg, col, dv_acc);
    mfma_tr_ring<NC, S::KStride>(dst_frag, q_lds_base, seg, col, dk_acc);
    if (has_next) {
      __syncthreads();  // everyone is done reading tile qt
      write_qdo_tiles();
      __syncthreads();  // tile qt+1 fully staged
    }
  }

#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k_row = k_row0 + seg * 4 + r;
    if (k_row >= T) continue;
    const long out_base = qkv_off + (long)k_row * st.qt;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      dk[out_base + c * 16 + col] = (short)f32_to_bf16(dk_acc[c][r]);
      dv[out_base + c * 16 + col] = (short)f32_to_bf16(dv_acc[c][r]);
    }
  }
}

// Delta = rowsum(dO * O), bandwidth-bound: it streams dO and O once
// (671 MB at the ViT-10B shape) for 4 MB of output.  o/dO are strided
// [B,T,H,D]- or [B,H,T,D]-layout tensors, delta is contiguous [B,H,T].
//
// Deliberately NOT fused into fmha_bwd_dq_kernel, which loads the same
// dO rows: that kernel sits exactly on an occupancy step (168 VGPRs,
// 3 waves/SIMD, profiles/raw/kernel_resources.txt) and has no registers
// left for the O fragments.
//
// 256-thread blocks, 8 lanes per row (32 rows per block iteration,
// grid-stride), 16-byte loads: lane g of a row's group loads vectors
// g, g+8, g+16 (D <= 192 is at most 24 vectors).  Rows are walked in
// MEMORY order (h fastest when the head stride is the smaller one, as in
// the [B,T,H,D] training layout), so a wave reads 8 adjacent rows as
// one contiguous span instead of 8 pieces a token stride apart.
//
// Summation order: element e of a row lands in accumulator j = e % 8 of
// lane g = (e / 8) % 8, i.e. "virtual lane" 8g + j = e % 64 — the lane
// the one-wave-per-row kernel below gives it — and the reduction
// replays that kernel's xor butterfly (32, 16, 8 across the 8 lanes,
// then 4, 2, 1 across the accumulators).  fp32 addition is commutative,
// so delta, and with it dq/dk/dv, is bit-identical to the scalar path.
constexpr int kRowdotLanes = 8;
constexpr int kRowdotRows = kBlockThreads / kRowdotLanes;  // per iteration
constexpr int kRowdotMaxLoads = kMaxD / 8 / kRowdotLanes;  // 3

__global__ __launch_bounds__(kBlockThreads) void fmha_rowdot_kernel(
    const ushort8_t* __restrict__ dout, const ushort8_t* __restrict__ o,
    float* __restrict__ delta, int n_rows, int T, int H, int nvec,
    long sob, long soh, long sot /* strides in 8-element vectors */,
    int h_fast) {
  const int g = threadIdx.x % kRowdotLanes;
  const int slot = threadIdx.x / kRowdotLanes;
  for (long r0 = (long)blockIdx.x * kRowdotRows; r0 < n_rows;
       r0 += (long)gridDim.x * kRowdotRows) {
    const bool ok = r0 + slot < n_rows;
    // every lane stays in the loop for the shuffles; rows past the end
    // load nothing and store nothing
    const unsigned r = ok ? (unsigned)(r0 + slot) : 0u;
    unsigned b, h, t;
    if (h_fast) {
      h = r % (unsigned)H;
      t = (r / (unsigned)H) % (unsigned)T;
    } else {
      t = r % (unsigned)T;
      h = (r / (unsigned)T) % (unsigned)H;
    }
    b = r / ((unsigned)T * (unsigned)H);
    const long base = (long)b * sob + (long)h * soh + (long)t * sot;

    ushort8_t dv[kRowdotMaxLoads], ov[kRowdotMaxLoads];
#pragma unroll
    for (int k = 0; k < kRowdotMaxLoads; ++k) {
      const int v = g + k * kRowdotLanes;
      if (ok && v < nvec) {
        dv[k] = dout[base + v];
        ov[k] = o[base + v];
      }
    }
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
    for (int k = 0; k < kRowdotMaxLoads; ++k) {
      const int v = g + k * kRowdotLanes;
      if (ok && v < nvec) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          acc[j] += bf16_to_f32(dv[k][j]) * bf16_to_f32(ov[k][j]);
      }
    }
    // virtual-lane offsets 32, 16, 8 = lane-group offsets 4, 2, 1
#pragma unroll
    for (int off = kRowdotLanes / 2; off > 0; off >>= 1) {
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], off);
    }
    // virtual-lane offsets 4, 2, 1 stay inside the lane
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += acc[j + 4];
    acc[0] += acc[2];
    acc[1] += acc[3];
    acc[0] += acc[1];
    if (ok && g == 0) delta[((long)b * H + h) * T + t] = acc[0];
  }
}

// Scalar path for operands whose base address is not 16-byte aligned:
// one wave per (b,h,t) row, 2-byte loads.
__global__ __launch_bounds__(64) void fmha_rowdot_scalar_kernel(
    const unsigned short* __restrict__ dout,
    const unsigned short* __restrict__ o, float* __restrict__ delta, int T,
    int H, int D, long sob, long soh, long sot) {
  const long row = blockIdx.x;  // linear over [B,H,T]
  const int t = (int)(row % T);
  const int h = (int)((row / T) % H);
  const long b = row / ((long)T * H);
  const long base = b * sob + (long)h * soh + (long)t * sot;
  float acc = 0.f;
  for (int i = threadIdx.x; i < D; i += 64)
    acc += bf16_to_f32(dout[base + i]) * bf16_to_f32(o[base + i]);
  acc = wave_all_sum(acc);
  if (threadIdx.x == 0) delta[row] = acc;
}

// P = exp(scale*S - lse); dS = scale * P * (dP - Delta)
// fused, bf16 io, 8-wide vectorized (rows are T elements, T % 8 == 0 on
// every ViT config; scalar fallback otherwise)
__global__ __launch_bounds__(256) void fmha_dsoftmax_kernel(
    const unsigned short* __restrict__ s_raw,
    const unsigned short* __restrict__ dp, const float* __restrict__ lse,
    const float* __restrict__ delta, unsigned short* __restrict__ p_out,
    unsigned short* __restrict__ ds_out, int T, float scale) {
  const long row = blockIdx.x;  // over B*H*T rows
  const float row_lse = lse[row];
  const float row_delta = delta[row];
  const long base = row * T;
  if ((T & 7) == 0) {
    const int nvec = T / 8;
    const ushort8_t* sv = (const ushort8_t*)(s_raw + base);
    const ushort8_t* dpv = (const ushort8_t*)(dp + base);
    ushort8_t* pv = (ushort8_t*)(p_out + base);
    ushort8_t* dsv = (ushort8_t*)(ds_out + base);
    for (int i = threadIdx.x; i < nvec; i += 256) {
      ushort8_t s8 = sv[i], d8 = dpv[i], p8, ds8;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __expf(bf16_to_f32(s8[j]) * scale - row_lse);
        p8[j] = f32_to_bf16(p);
        ds8[j] = f32_to_bf16(scale * p * (bf16_to_f32(d8[j]) - row_delta));
      }
      pv[i] = p8;
      dsv[i] = ds8;
    }
  } else {
    for (int i = threadIdx.x; i < T; i += 256) {
      const float p = __expf(bf16_to_f32(s_raw[base + i]) * scale - row_lse);
      p_out[base + i] = f32_to_bf16(p);
      ds_out[base + i] =
          f32_to_bf16(scale * p * (bf16_to_f32(dp[base + i]) - row_delta));
    }
  }
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports the real configs
template __global__ void fmha_fwd_kernel<160, false>(
    const short*, const short*, const short*, short*, float*, int, int,
    QkvStrides, float, unsigned, float, unsigned);
template __global__ void fmha_fwd_kernel<160, true>(
    const short*, const short*, const short*, short*, float*, int, int,
    QkvStrides, float, unsigned, float, unsigned);
template __global__ void fmha_fwd_kernel<64, false>(
    const short*, const short*, const short*, short*, float*, int, int,
    QkvStrides, float, unsigned, float, unsigned);
#define VITFSDP_INSTANTIATE_BWD(D_, DROP_)                                  \
  template __global__ void fmha_bwd_dq_kernel<D_, DROP_>(                    \
      const short*, const short*, const short*, const short*, const float*,  \
      const float*, short*, int, int, QkvStrides, float, unsigned, float,    \
      unsigned);                                                             \
  template __global__ void fmha_bwd_dkv_kernel<D_, DROP_>(                   \
      const short*, const short*, const short*, const short*, const float*,  \
      const float*, short*, short*, int, int, QkvStrides, float, unsigned,   \
      float, unsigned);
VITFSDP_INSTANTIATE_BWD(160, false)
VITFSDP_INSTANTIATE_BWD(160, true)  // the dropout backward training uses
VITFSDP_INSTANTIATE_BWD(64, false)  // QSub = 2
#undef VITFSDP_INSTANTIATE_BWD
#else
struct FmhaArgs {
  const short *q, *k, *v;
  short* o;        // or dO for backward
  int B, H, T;
  QkvStrides st;
  float scale;
  float p_drop = 0.f;   // attention dropout probability
  unsigned seed = 0;    // dropout mask seed
};

inline unsigned drop_threshold(float p) {
  if (p <= 0.f) return 0u;
  double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (unsigned)t;
}

// one launch per kernel: f(std::bool_constant<DROP>, thresh, rscale, seed)
template <typename F>
void with_dropout(const FmhaArgs& a, F&& f) {
  if (a.p_drop > 0.f) {
    f(std::true_type{}, drop_threshold(a.p_drop), 1.f / (1.f - a.p_drop),
      a.seed);
  } else {
    f(std::false_type{}, 0u, 1.f, 0u);
  }
}

template <int D>
void launch_fmha_fwd(const FmhaArgs& a, torch::Tensor& lse) {
  dim3 grid((unsigned)((long)a.B * a.H),
            (a.T + FmhaShapes<D>::QTile - 1) / FmhaShapes<D>::QTile);
  auto stream = at::cuda::getCurrentCUDAStream();
  with_dropout(a, [&](auto drop, unsigned thr, float rs, unsigned seed) {
    hipLaunchKernelGGL((fmha_fwd_kernel<D, decltype(drop)::value>), grid,
                       dim3(kBlockThreads),
                       sizeof(typename FmhaShapes<D>::Shared), stream, a.q,
                       a.k, a.v, a.o, lse.data_ptr<float>(), a.T, a.H, a.st,
                       a.scale, thr, rs, seed);
  });
  HIP_CHECK_LAST();
}

template <int D>
void launch_fmha_bwd(const FmhaArgs& a, const torch::Tensor& lse,
                     const torch::Tensor& delta, short* dq, short* dk,
                     short* dv) {
  using S = FmhaShapes<D>;
  auto stream = at::cuda::getCurrentCUDAStream();
  const unsigned BH = (unsigned)((long)a.B * a.H);
  dim3 grid_dq(BH, (a.T + S::QTile - 1) / S::QTile);
  dim3 grid_dkv(BH, (a.T + 63) / 64);
  with_dropout(a, [&](auto drop, unsigned thr, float rs, unsigned seed) {
    constexpr bool kDrop = decltype(drop)::value;
    hipLaunchKernelGGL((fmha_bwd_dq_kernel<D, kDrop>), grid_dq,
                       dim3(kBlockThreads), sizeof(typename S::SharedDQ),
                       stream, a.q, a.k, a.v, a.o /*dO*/,
                       lse.data_ptr<float>(), delta.data_ptr<float>(), dq,
                       a.T, a.H, a.st, a.scale, thr, rs, seed);
    HIP_CHECK_LAST();
    hipLaunchKernelGGL((fmha_bwd_dkv_kernel<D, kDrop>), grid_dkv,
                       dim3(kBlockThreads), sizeof(typename S::SharedDKV),
                       stream, a.q, a.k, a.v, a.o /*dO*/,
                       lse.data_ptr<float>(), delta.data_ptr<float>(), dk, dv,
                       a.T, a.H, a.st, a.scale, thr, rs, seed);
    HIP_CHECK_LAST();
  });
}

#define VITFSDP_FMHA_DISPATCH(D_, expr)                               \
  switch (D_) {                                                       \
    case 16: { constexpr int kD = 16; expr; break; }                  \
    case 32: { constexpr int kD = 32; expr; break; }                  \
    case 48: { constexpr int kD = 48; expr; break; }                  \
    case 64: { constexpr int kD = 64; expr; break; }                  \
    case 80: { constexpr int kD = 80; expr; break; }                  \
    case 96: { constexpr int kD = 96; expr; break; }                  \
    case 112: { constexpr int kD = 112; expr; break; }                \
    case 128: { constexpr int kD = 128; expr; break; }                \
    case 144: { constexpr int kD = 144; expr; break; }                \
    case 160: { constexpr int kD = 160; expr; break; }                \
    case 176: { constexpr int kD = 176; expr; break; }                \
    case 192: { constexpr int kD = 192; expr; break; }                \
    default: TORCH_CHECK(false, "fmha: unsupported head_dim ", D_);   \
  }

#endif  // VITFSDP_KERNELS_ONLY

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

QkvStrides contiguous_strides(int H, int T, int D) {
  QkvStrides st;
  st.qh = (long)T * D;
  st.qb = (long)H * st.qh;
  st.qt = D;
  st.ob = st.qb;
  st.oh = st.qh;
  st.ot = st.qt;
  return st;
}

// qkv: [B, T, 3, H, D] contiguous; o / dO: [B, T, H, D]
QkvStrides fused_qkv_strides(int T, int H, int D) {
  QkvStrides st;
  st.qt = 3L * H * D;
  st.qb = (long)T * st.qt;
  st.qh = D;
  st.ot = (long)H * D;
  st.ob = (long)T * st.ot;
  st.oh = D;
  return st;
}

torch::Tensor run_rowdot(const torch::Tensor& dout, const torch::Tensor& o,
                         int B, int H, int T, int D, const QkvStrides& st) {
  auto delta = torch::empty({B, H, T}, dout.options().dtype(torch::kFloat32));
  auto stream = at::cuda::getCurrentCUDAStream();
  const long n_rows = (long)B * H * T;
  if (n_rows == 0) return delta;
  // 16-byte loads need 16-byte-aligned bases (D % 16 == 0 makes every
  // stride a multiple of 8 elements already); the row index is split
  // with 32-bit divides
  const bool aligned =
      ((reinterpret_cast<uintptr_t>(dout.data_ptr()) |
        reinterpret_cast<uintptr_t>(o.data_ptr())) & 15) == 0 &&
      D % 8 == 0 && D <= kMaxD && st.ob % 8 == 0 && st.oh % 8 == 0 &&
      st.ot % 8 == 0;
  if (aligned && n_rows < (1L << 31)) {
    // 2048 blocks = 256 CUs x 8: one block per SIMD slot at full
    // occupancy (the kernel needs well under 64 VGPRs)
    const long n_blocks =
        std::min<long>((n_rows + kRowdotRows - 1) / kRowdotRows, 2048);
    hipLaunchKernelGGL(fmha_rowdot_kernel, dim3((unsigned)n_blocks),
                       dim3(kBlockThreads), 0, stream,
                       (const ushort8_t*)dout.data_ptr(),
                       (const ushort8_t*)o.data_ptr(), delta.data_ptr<float>(),
                       (int)n_rows, T, H, D / 8, st.ob / 8, st.oh / 8,
                       st.ot / 8, st.oh < st.ot ? 1 : 0);
  } else {
    hipLaunchKernelGGL(fmha_rowdot_scalar_kernel, dim3(n_rows), dim3(64), 0,
                       stream, (const unsigned short*)dout.data_ptr(),
                       (const unsigned short*)o.data_ptr(),
                       delta.data_ptr<float>(), T, H, D, st.ob, st.oh, st.ot);
  }
  HIP_CHECK_LAST();
  return delta;
}

bool supported_head_dim(long D) { return D >= 16 && D <= kMaxD && D % 16 == 0; }

// The backward kernels read every operand through raw pointers with
// strides derived from q's (or qkv's) shape alone, so each one has to be
// exactly the tensor the strides describe: a view with other strides
// gives wrong gradients, a smaller one an out-of-bounds read.
void check_bwd_operand(const char* fn, const char* name,
                       const torch::Tensor& t, const torch::Tensor& like,
                       at::IntArrayRef shape) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), fn, ": ", name,
              " must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, fn, ": ", name,
              " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.sizes() == shape, fn, ": ", name, " must have shape ", shape,
              ", got ", t.sizes());
  TORCH_CHECK(t.is_contiguous(), fn, ": ", name, " must be contiguous");
}

void check_bwd_lse(const char* fn, const torch::Tensor& lse,
                   const torch::Tensor& like, long B, long H, long T) {
  TORCH_CHECK(lse.is_cuda() && lse.device() == like.device(), fn,
              ": lse must be a GPU tensor on the device of the other operands");
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32, fn,
              ": lse must be fp32, got ", lse.scalar_type());
  TORCH_CHECK(lse.dim() == 3 && lse.size(0) == B && lse.size(1) == H &&
                  lse.size(2) == T,
              fn, ": lse must have shape [B, H, T] = [", B, ", ", H, ", ", T,
              "], got ", lse.sizes());
  TORCH_CHECK(lse.is_contiguous(), fn, ": lse must be contiguous");
}

}  // namespace

// ---- [B,H,T,D] contiguous API (kernel unit tests, generic use) ----

std::vector<torch::Tensor> fmha_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, double scale,
                                    double p_drop, long seed) {
  TORCH_CHECK(q.is_cuda() && q.is_contiguous() && k.is_contiguous() &&
              v.is_contiguous());
  TORCH_CHECK(q.scalar_type() == torch::kBFloat16, "fmha_fwd: bf16 only");
  TORCH_CHECK(q.dim() == 4, "fmha_fwd: [B, H, T, D]");
  const int B = q.size(0), H = q.size(1), T = q.size(2), D = q.size(3);
  TORCH_CHECK(D % 16 == 0 && D <= kMaxD,
              "fmha_fwd: head_dim must be a multiple of 16 and <= ", kMaxD);

  auto o = torch::empty_like(q);
  auto lse = torch::empty({B, H, T}, q.options().dtype(torch::kFloat32));
  FmhaArgs a{(const short*)q.data_ptr(), (const short*)k.data_ptr(),
             (const short*)v.data_ptr(), (short*)o.data_ptr(),
             B, H, T, contiguous_strides(H, T, D), (float)scale,
             (float)p_drop, (unsigned)seed};
  VITFSDP_FMHA_DISPATCH(D, launch_fmha_fwd<kD>(a, lse));
  return {o, lse};
}

std::vector<torch::Tensor> fmha_bwd(torch::Tensor dout, torch::Tensor q,
                                    torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse,
                                    double scale, double p_drop, long seed) {
  TORCH_CHECK(q.is_cuda() && q.dim() == 4,
              "fmha_bwd: q must be a GPU tensor [B, H, T, D]");
  TORCH_CHECK(supported_head_dim(q.size(3)),
              "fmha_bwd: head_dim must be a multiple of 16 and <= ", kMaxD,
              ", got ", q.size(3));
  check_bwd_operand("fmha_bwd", "q", q, q, q.sizes());
  check_bwd_operand("fmha_bwd", "k", k, q, q.sizes());
  check_bwd_operand("fmha_bwd", "v", v, q, q.sizes());
  check_bwd_operand("fmha_bwd", "o", o, q, q.sizes());
  check_bwd_operand("fmha_bwd", "dout", dout, q, q.sizes());
  check_bwd_lse("fmha_bwd", lse, q, q.size(0), q.size(1), q.size(2));
  const int B = q.size(0), H = q.size(1), T = q.size(2), D = q.size(3);
  const QkvStrides st = contiguous_strides(H, T, D);
  auto delta = run_rowdot(dout, o, B, H, T, D, st);
  auto stream = at::cuda::getCurrentCUDAStream();

  static const bool use_compose = [] {
    const char* e = getenv("VITFSDP_FMHA_BWD");
    return e != nullptr && strcmp(e, "compose") == 0;
  }();
  if (use_compose) {
    // fallback/debug path: batched hipBLASLt GEMMs + fused softmax-grad
    // kernel (measured ~5x slower than the fused kernels at the 10B
    // shape — the tiny per-head batched GEMMs run at 26-50 TF/s)
    auto s_raw = at::matmul(q, k.transpose(-2, -1));
    auto dp = at::matmul(dout, v.transpose(-2, -1));
    auto p = torch::empty_like(s_raw);
    auto ds = torch::empty_like(s_raw);
    hipLaunchKernelGGL(fmha_dsoftmax_kernel, dim3((long)B * H * T), dim3(256),
                       0, stream, (const unsigned short*)s_raw.data_ptr(),
                       (const unsigned short*)dp.data_ptr(),
                       lse.data_ptr<float>(), delta.data_ptr<float>(),
                       (unsigned short*)p.data_ptr(),
                       (unsigned short*)ds.data_ptr(), T, (float)scale);
    HIP_CHECK_LAST();
    auto dv = at::matmul(p.transpose(-2, -1), dout);
    auto dq = at::matmul(ds, k);
    auto dk = at::matmul(ds.transpose(-2, -1), q);
    return {dq, dk, dv};
  }

  auto dq = torch::empty_like(q);
  auto dk = torch::empty_like(k);
  auto dv = torch::empty_like(v);
  FmhaArgs a{(const short*)q.data_ptr(), (const short*)k.data_ptr(),
             (const short*)v.data_ptr(), (short*)dout.data_ptr(),
             B, H, T, st, (float)scale, (float)p_drop, (unsigned)seed};
  VITFSDP_FMHA_DISPATCH(
      D, launch_fmha_bwd<kD>(a, lse, delta, (short*)dq.data_ptr(),
                             (short*)dk.data_ptr(), (short*)dv.data_ptr()));
  return {dq, dk, dv};
}

// Delta alone, for contiguous [B,H,T,D] operands (direct kernel tests)
torch::Tensor fmha_rowdot(torch::Tensor dout, torch::Tensor o) {
  TORCH_CHECK(dout.is_cuda() && o.is_cuda() && dout.is_contiguous() &&
                  o.is_contiguous(),
              "fmha_rowdot: contiguous GPU tensors");
  TORCH_CHECK(dout.scalar_type() == torch::kBFloat16 &&
                  o.scalar_type() == torch::kBFloat16,
              "fmha_rowdot: bf16 only");
  TORCH_CHECK(dout.dim() == 4 && dout.sizes() == o.sizes(),
              "fmha_rowdot: two [B, H, T, D] tensors of one shape");
  const int B = dout.size(0), H = dout.size(1), T = dout.size(2),
            D = dout.size(3);
  TORCH_CHECK(D % 16 == 0 && D <= kMaxD,
              "fmha_rowdot: head_dim must be a multiple of 16 and <= ", kMaxD);
  return run_rowdot(dout, o, B, H, T, D, contiguous_strides(H, T, D));
}

// ---- fused-qkv API: zero-copy path used by the Attention module ----
// qkv: [B, T, 3, H, D] contiguous (the fused projection output reshaped);
// o comes back [B, T, H, D] (== [B, T, E]); dO arrives the same way.

std::vector<torch::Tensor> fmha_fwd_qkv(torch::Tensor qkv, long num_heads,
                                        double scale, double p_drop,
                                        long seed) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 5 &&
                  qkv.size(2) == 3 && qkv.size(3) == num_heads,
              "fmha_fwd_qkv: expected contiguous [B, T, 3, H, D]");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16, "fmha: bf16 only");
  const int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3),
            D = qkv.size(4);
  TORCH_CHECK(D % 16 == 0 && D <= kMaxD,
              "fmha: head_dim must be a multiple of 16 and <= ", kMaxD);
  const QkvStrides st = fused_qkv_strides(T, H, D);

  auto o = torch::empty({B, T, (long)H * D}, qkv.options());
  auto lse = torch::empty({B, H, T}, qkv.options().dtype(torch::kFloat32));
  const short* base = (const short*)qkv.data_ptr();
  FmhaArgs a{base, base + (long)H * D, base + 2L * H * D,
             (short*)o.data_ptr(), B, H, T, st, (float)scale,
             (float)p_drop, (unsigned)seed};
  VITFSDP_FMHA_DISPATCH(D, launch_fmha_fwd<kD>(a, lse));
  return {o, lse};
}

torch::Tensor fmha_bwd_qkv(torch::Tensor dout, torch::Tensor qkv,
                           torch::Tensor o, torch::Tensor lse,
                           long num_heads, double scale, double p_drop,
                           long seed) {
  TORCH_CHECK(qkv.is_cuda() && qkv.is_contiguous() && qkv.dim() == 5 &&
                  qkv.size(2) == 3 && qkv.size(3) == num_heads,
              "fmha_bwd_qkv: expected contiguous GPU qkv [B, T, 3, H, D]");
  TORCH_CHECK(qkv.scalar_type() == torch::kBFloat16,
              "fmha_bwd_qkv: qkv must be bf16, got ", qkv.scalar_type());
  TORCH_CHECK(supported_head_dim(qkv.size(4)),
              "fmha_bwd_qkv: head_dim must be a multiple of 16 and <= ", kMaxD,
              ", got ", qkv.size(4));
  {
    // o and dO are [B, T, H*D]; the equivalent [B, T, H, D] view is
    // accepted too (same memory)
    const long b = qkv.size(0), t = qkv.size(1), h = qkv.size(3),
               d = qkv.size(4);
    const std::vector<long> flat{b, t, h * d}, split{b, t, h, d};
    check_bwd_operand("fmha_bwd_qkv", "o", o, qkv,
                      o.dim() == 4 ? split : flat);
    check_bwd_operand("fmha_bwd_qkv", "dout", dout, qkv,
                      dout.dim() == 4 ? split : flat);
    check_bwd_lse("fmha_bwd_qkv", lse, qkv, b, h, t);
  }
  const int B = qkv.size(0), T = qkv.size(1), H = qkv.size(3),
            D = qkv.size(4);
  const QkvStrides st = fused_qkv_strides(T, H, D);
  auto delta = run_rowdot(dout, o, B, H, T, D, st);

  auto dqkv = torch::empty_like(qkv);
  const short* base = (const short*)qkv.data_ptr();
  short* dbase = (short*)dqkv.data_ptr();
  FmhaArgs a{base, base + (long)H * D, base + 2L * H * D,
             (short*)dout.data_ptr(), B, H, T, st, (float)scale,
             (float)p_drop, (unsigned)seed};
  VITFSDP_FMHA_DISPATCH(
      D, launch_fmha_bwd<kD>(a, lse, delta, dbase, dbase + (long)H * D,
                             dbase + 2L * H * D));
  return dqkv;
}
#endif  // VITFSDP_KERNELS_ONLY
