// Weight-gradient GEMM for CDNA4: C[M,N] = A^T B with A = dY [K, M] and
// B = X [K, N] both row-major bf16 (the Linear-backward wgrad shape,
// K = batch*tokens = 32768 for the ViT-10B config).
//
// hipBLASLt runs these transposed-A shapes at ~1.0-1.1 PF/s vs ~1.5 for
// the forward TN GEMMs.  The hard part of a hand-written version is that
// the contraction dim K is the non-contiguous axis of both operands; the
// usual fix (transpose during LDS staging) costs 64 scalar LDS writes
// per thread per K-step.  gfx950's ds_read_b64_tr_b16 removes that
// entirely: tiles stay row-major [k][m] in LDS and the MFMA fragments
// are gathered along K by the hardware transpose read (semantics:
// mfma_tiles.h).
//
// Tiling: 256x256 C tile per 512-thread block (8 waves as 2m x 4n, each
// wave 128x64), BK = 64, two LDS buffers of 2 x 32 KB = 128 KB, so ONE
// workgroup per CU.  Structure (the fgemm.hip ladder, profiles/
// PROFILES.md "wgemm NT ladder"):
//  * XCD-clustered 2-D tile mapping (xcd_cluster_tile, mfma_tiles.h);
//  * direct-to-LDS staging: the next K-step's global_load_lds (16 B)
//    are issued at the top of this step and fly under its MFMAs — no
//    staging registers, no LDS write pass;
//  * fragment reads as before (B up front, A through a 2-deep ring of
//    counted waits), now one address register per fragment plus
//    immediate offsets.
// The fragment-to-k mapping and the order of the k-chunk accumulation
// are those of the register-staged first version: outputs are
// bit-identical to it.
//
// LDS image.  One wave-wide global_load_lds deposits 1 KB contiguously
// = two packed 512-byte k-rows, so rows cannot be padded; bank spread
// comes from an XOR applied to the global SOURCE column and to the read
// address alike.  A 32-lane half of a transpose read (the unit that
// conflicts) takes 8 k-rows, r..r+3 and r+8..r+11 (r % 16 in {0, 4}),
// 32 bytes each at ONE 32-byte column chunk; with a 512-byte stride all
// 8 would sit on the same 32-byte slot of the 256-byte bank row (8-way).
// Storing chunk c of k-row k at chunk c ^ x(k),
//     x(k) = (k & 3) | (((k >> 3) & 1) << 2),
// gives the 8 rows the 8 distinct values of x, hence 8 distinct slots:
// conflict-free.  The XOR moves whole 32-byte chunks, so every lane's
// 8-byte address stays aligned and the two 16-byte halves of a chunk
// keep their order.  For the reading lane x is a lane constant
// ((col >> 2) | ((seg & 1) << 2)): all reads of a K-step are one
// address register per 16-column fragment plus an immediate offset.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "mfma_tiles.h"

namespace {

constexpr int kBM = 256;
constexpr int kBN = 256;
constexpr int kBK = 64;
constexpr int kThreads = 512;  // 8 waves: 2 (m) x 4 (n)
static_assert(kBM == kBN, "one staging/read scheme serves both tiles");
constexpr int kRowBytes = kBM * 2;  // packed k-row: 512 B = 16 chunks

struct WgemmShared {
  short a_tile[2][kBK][kBM];  // dY tile, [k][m ^ swizzle], double-buffered
  short b_tile[2][kBK][kBN];  // X  tile, [k][n ^ swizzle], double-buffered
};

// 32-byte chunk XOR of k-row k (header comment)
__device__ __forceinline__ int chunk_xor(int k) {
  return (k & 3) | (((k >> 3) & 1) << 2);
}

__device__ __forceinline__ void glds16(const short* gsrc, short* lds_dst) {
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*)gsrc,
      (__attribute__((address_space(3))) void*)lds_dst, 16, 0, 0);
}

template <bool WITH_BIAS>
__global__ __launch_bounds__(kThreads, 1) void wgemm_atb_kernel(
    const short* __restrict__ a,  // [K, M]
    const short* __restrict__ b,  // [K, N]
    short* __restrict__ c,        // [M, N]
    float* __restrict__ dbias,    // optional [M] fp32 (atomic), may be null
    int K, int M, int N) {
  HIP_DYNAMIC_SHARED(char, smem_raw)
  WgemmShared& sm = *reinterpret_cast<WgemmShared*>(smem_raw);
  const unsigned a_base0 = (unsigned)__builtin_amdgcn_groupstaticsize();
  const unsigned b_base0 = a_base0 + sizeof(sm.a_tile);
  constexpr unsigned kABufBytes = sizeof(sm.a_tile[0]);
  constexpr unsigned kBBufBytes = sizeof(sm.b_tile[0]);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int col = lane & 15;
  const int seg = lane >> 4;
  const int wm = wave >> 2;  // 0..1: wave's 128-row m strip
  const int wn = wave & 3;   // 0..3: wave's 64-col n strip

  // XCD-aware 2D tile clustering (mfma_tiles.h).  The operand panels
  // of a 10B shape are re-fetched 20-60x across the grid (~40 GB per
  // call, above HBM peak at the kernel's speed), so the kernel lives on
  // L2 reuse; the clustered rectangle gives it on BOTH operands where
  // the earlier M-major run reused one.
  int bx, by;
  xcd_cluster_tile(bx, by);
  const long m0 = (long)bx * kBM;
  const long n0 = (long)by * kBN;

  // DirectToLds staging: one global_load_lds(16 B) call deposits the
  // wave's 64 lanes contiguously = k-rows R, R+1 of a tile, so lane l
  // fills 16-B granule l&31 of row R + (l>>5) and fetches the source
  // granule whose 32-byte chunk is XORed with chunk_xor(row).  4 calls
  // per wave and operand cover the 64 rows.  No staging registers, no
  // LDS write pass; synced by vmcnt + barrier.
  constexpr int kCalls = kBK / 2 / (kThreads / 64);  // 4
  auto issue_dtl = [&](int buf, long k_base) {
    const int rsub = lane >> 5;
    const int gl = lane & 31;
#pragma unroll
    for (int i = 0; i < kCalls; ++i) {
      const int R = (wave * kCalls + i) * 2;
      const int k = R + rsub;
      const int g = (((gl >> 1) ^ chunk_xor(k)) << 1) | (gl & 1);
      glds16(&a[(k_base + k) * M + m0 + g * 8], &sm.a_tile[buf][R][0]);
      glds16(&b[(k_base + k) * N + n0 + g * 8], &sm.b_tile[buf][R][0]);
    }
  };

  // fragment-read addresses: lane (seg, col) reads k-row
  // kc*32 + seg*8 + 4h + (col>>2), 8 bytes at (col&3)*8 of the 32-byte
  // chunk of its 16-column fragment; that row's chunk XOR is the lane
  // constant xr, and (kc, h) move the address by a compile-time offset
  const int xr = (col >> 2) | ((seg & 1) << 2);
  const unsigned lane_off =
      (unsigned)((seg * 8 + (col >> 2)) * kRowBytes + (col & 3) * 8);
  unsigned a_off[8], b_off[4];
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
    a_off[mi] = lane_off + ((unsigned)((wm * 8 + mi) ^ xr) << 5);
#pragma unroll
  for (int ni = 0; ni < 4; ++ni)
    b_off[ni] = lane_off + ((unsigned)((wn * 4 + ni) ^ xr) << 5);

  f32x4 acc[8][4];
#pragma unroll
  for (int mi = 0; mi < 8; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  float bias_acc[WITH_BIAS ? 8 : 1];
#pragma unroll
  for (int mi = 0; mi < (WITH_BIAS ? 8 : 1); ++mi) bias_acc[mi] = 0.f;

  const int n_ksteps = K / kBK;
  issue_dtl(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  for (int ks = 0; ks < n_ksteps; ++ks) {
    const int buf = ks & 1;
    const unsigned a_base = a_base0 + (unsigned)buf * kABufBytes;
    const unsigned b_base = b_base0 + (unsigned)buf * kBBufBytes;
    // next K-step's tiles go to the OTHER buffer, whose last fragment
    // reads retired (the mi = 7 lgkmcnt(0)) before the previous barrier
    if (ks + 1 < n_ksteps) issue_dtl(buf ^ 1, (long)(ks + 1) * kBK);
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      // one fragment = two transpose reads (the lane's k-row and the
      // one 4 below) of chunk kc, at compile-time offsets from addr
      auto rd = [&](unsigned addr, u32x2 (&f)[2]) {
        if (kc == 0) {
          f[0] = tr16_read_at<0>(addr);
          f[1] = tr16_read_at<4 * kRowBytes>(addr);
        } else {
          f[0] = tr16_read_at<32 * kRowBytes>(addr);
          f[1] = tr16_read_at<36 * kRowBytes>(addr);
        }
      };
      // B fragments for this 32-k chunk (8 tr reads, reused across mi)
      u32x2 bf[4][2];
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) rd(b_base + b_off[ni], bf[ni]);
      // A fragments stream through a 2-deep ring: af[mi+1] is issued
      // before the MFMAs of af[mi], with counted lgkmcnt waits.  The
      // waits carry the about-to-be-consumed fragments as "+v" operands
      // so the MFMAs cannot be scheduled above them (guide rule 18)
      // without fencing the whole scheduler.  (All 24 reads up front
      // under one wait, fgemm's v7 rung, measured 2% SLOWER here: the
      // ring starts the MFMAs after 10 reads instead of 24.)
      u32x2 af[2][2];
      rd(a_base + a_off[0], af[0]);
#pragma unroll
      for (int mi = 0; mi < 8; ++mi) {
        const int cur = mi & 1;
        if (mi < 7) rd(a_base + a_off[mi + 1], af[cur ^ 1]);
        if (mi == 0) {
          // first wait also guards the B fragments (issued earlier,
          // retired in order before af[0]), which lds_wait's
          // two-operand signature does not cover
          asm volatile("s_waitcnt lgkmcnt(%[cnt])"
                       : "+v"(af[cur][0]), "+v"(af[cur][1]),
                         "+v"(bf[0][0]), "+v"(bf[0][1]), "+v"(bf[1][0]),
                         "+v"(bf[1][1]), "+v"(bf[2][0]), "+v"(bf[2][1])
                       : [cnt] "i"(2)
                       : "memory");
          asm volatile("" : "+v"(bf[3][0]), "+v"(bf[3][1]));
        } else if (mi < 7) {
          lds_wait<2>(af[cur][0], af[cur][1]);
        } else {
          lds_wait<0>(af[cur][0], af[cur][1]);
        }
        const bf16x8 a_frag = frag_from(af[cur][0], af[cur][1]);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) {
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a_frag, frag_from(bf[ni][0], bf[ni][1]), acc[mi][ni], 0, 0, 0);
        }
        __builtin_amdgcn_s_setprio(0);
        if (WITH_BIAS && wn == 0) {
          // dbias[m] = sum_k dY[k][m]: this lane's A fragment holds 8
          // consecutive k for column m = wm*128 + mi*16 + col
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            bias_acc[mi] +=
                bf16_to_f32((unsigned short)(af[cur][h][0] & 0xffff)) +
                bf16_to_f32((unsigned short)(af[cur][h][0] >> 16)) +
                bf16_to_f32((unsigned short)(af[cur][h][1] & 0xffff)) +
                bf16_to_f32((unsigned short)(af[cur][h][1] >> 16));
          }
        }
      }
    }

    // single barrier per K-step: the next step's tiles (in flight
    // since the top of this step) have landed and are visible
    if (ks + 1 < n_ksteps) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // epilogue: C[m][n], C-layout rows m = seg*4+r
#pragma unroll
  for (int mi = 0; mi < 8; ++mi) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long m = m0 + wm * 128 + mi * 16 + seg * 4 + r;
#pragma unroll
      for (int ni = 0; ni < 4; ++ni) {
        const long n = n0 + wn * 64 + ni * 16 + col;
        c[m * N + n] = (short)f32_to_bf16(acc[mi][ni][r]);
      }
    }
    if (WITH_BIAS && wn == 0) {
      // one lane per (m-column, seg-k-range): sum the 4 seg partials
      float v = bias_acc[mi];
      v += __shfl_xor(v, 16);
      v += __shfl_xor(v, 32);
      if (seg == 0) {
        atomicAdd(&dbias[m0 + wm * 128 + mi * 16 + col], v);
      }
    }
  }
}

#ifdef VITFSDP_KERNELS_ONLY
template __global__ void wgemm_atb_kernel<false>(const short*, const short*,
                                                 short*, float*, int, int,
                                                 int);
#endif

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
std::vector<torch::Tensor> wgrad_gemm(torch::Tensor a, torch::Tensor b,
                                      bool with_bias) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && b.is_contiguous());
  TORCH_CHECK(a.scalar_type() == torch::kBFloat16 &&
              b.scalar_type() == torch::kBFloat16);
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(0) == b.size(0));
  const long K = a.size(0), M = a.size(1), N = b.size(1);
  TORCH_CHECK(K % kBK == 0 && M % kBM == 0 && N % kBN == 0,
              "wgrad_gemm: needs K%64==0, M%256==0, N%256==0 (got ", K, ",",
              M, ",", N, ")");
  auto c = torch::empty({M, N}, a.options());
  torch::Tensor dbias;
  float* dbias_ptr = nullptr;
  if (with_bias) {
    dbias = torch::zeros({M}, a.options().dtype(torch::kFloat32));
    dbias_ptr = dbias.data_ptr<float>();
  }
  static bool attr_set = [] {
    hipFuncSetAttribute(
        reinterpret_cast<const void*>(&wgemm_atb_kernel<false>),
        hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(WgemmShared));
    hipFuncSetAttribute(
        reinterpret_cast<const void*>(&wgemm_atb_kernel<true>),
        hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(WgemmShared));
    return true;
  }();
  (void)attr_set;
  dim3 grid((unsigned)(M / kBM), (unsigned)(N / kBN));
  auto stream = at::cuda::getCurrentCUDAStream();
  if (with_bias) {
    hipLaunchKernelGGL(wgemm_atb_kernel<true>, grid, dim3(kThreads),
                       sizeof(WgemmShared), stream,
                       (const short*)a.data_ptr(), (const short*)b.data_ptr(),
                       (short*)c.data_ptr(), dbias_ptr, (int)K, (int)M,
                       (int)N);
  } else {
    hipLaunchKernelGGL(wgemm_atb_kernel<false>, grid, dim3(kThreads),
                       sizeof(WgemmShared), stream,
                       (const short*)a.data_ptr(), (const short*)b.data_ptr(),
                       (short*)c.data_ptr(), nullptr, (int)K, (int)M,
                       (int)N);
  }
  HIP_CHECK_LAST();
  if (with_bias) return {c, dbias};
  return {c};
}
#endif  // VITFSDP_KERNELS_ONLY
