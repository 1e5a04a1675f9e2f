// Patch dropout (--patch_drop_rate): each sample keeps a uniformly random
// K of its T patch tokens in training (timm's PatchDropout, ordered), and
// the front of the model runs on the kept tokens only:
//
//   tokens[b, j, :] = dropout(proj[b, j, :] + pos[idx[b, j], :])
//
//   patch_drop_plan       (seed, B, T, K) -> idx [B, K], inv [B, T]
//   patch_drop_embed_fwd  the line above, one pass
//   patch_drop_embed_bwd  (dproj, dpos) from one read of dy
//
// The subset is a pure function of one integer: token t of sample b gets
// the key dropout_hash(seed, b, t) (common.h, row = sample, column =
// token) and the K tokens with the smallest (key, t) pairs are kept.  T
// independent keys ranked this way make every K-subset equally likely,
// and the tie-break on t makes the rank a permutation, so exactly K are
// kept.  idx lists them ascending in t; inv is its inverse, inv[b, t] = j
// with idx[b, j] = t, or -1 for a dropped token.
//
// The plan is one workgroup per sample with the T <= 1024 keys in LDS.
// Each thread owns up to four CONSECUTIVE tokens and ranks them against
// all T keys (every lane reads the same LDS word: a broadcast), so the
// keep flags of a thread are one small count and the output slot of a
// kept token is a workgroup exclusive prefix sum of those counts: a wave
// scan, four wave totals through LDS.  No atomics, no sort.
//
// The forward is dropout.hip's layout: a thread owns ONE 8-wide vector
// column and walks the rows of its chunk, grid = (E/8/256, row chunks).
// The row b*K + j is the same for the whole block, so idx[b, j] is a
// scalar load and the pos row a wave-uniform base.  The sum is formed in
// fp32 and rounded to bf16 once (torch's add, bit for bit); the element
// mask, where p > 0, is dropout_fwd's on that bf16 sum: hash_keep at the
// flattened output row, one more multiply and rounding on a kept value.
//
// The backward turns the scatter-add of dpos inside out: grid =
// (E/8/256, T), a workgroup owns token t and walks b = 0 .. B-1 in order.
// j = inv[b, t] is a scalar load; a dropped token costs that load and
// nothing else.  For a kept one the thread loads its 16 bytes of
// dy[b, j, :], applies the forward's element mask, writes dproj and adds
// the fp32 value into eight registers; after the walk dpos[t, :] is
// rounded once to bf16.  Every row of dy belongs to exactly one t, so dy
// is read once, dproj written once, the order of every sum is fixed and
// nothing is atomic.  At p == 0 dproj is dy and is not written.
//
// idx and inv are trusted as far as values go, but never as addresses: an
// idx outside [0, T) is clamped into it and an inv outside [0, K) counts
// as dropped, so a foreign tensor can give wrong numbers and no stray
// access.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "common.h"
#include "stream_tiles.h"
#ifndef VITFSDP_KERNELS_ONLY
#include "stream_host.h"
#endif

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / WAVE_SIZE;
constexpr int kMaxTokens = 1024;
// consecutive tokens of one thread in the plan
constexpr int kPerThread = kMaxTokens / kBlock;
// samples per round of the backward's walk: that many loads in flight
constexpr int kWalk = 4;

// ---- 1. the plan ----------------------------------------------------------

__global__ __launch_bounds__(kBlock) void patch_drop_plan_kernel(
    int* __restrict__ idx, int* __restrict__ inv, int T, int K,
    unsigned seed) {
  __shared__ unsigned keys[kMaxTokens];
  __shared__ int wave_total[kWaves];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  for (int t = tid; t < T; t += kBlock)
    keys[t] = dropout_hash(seed, (unsigned)b, (unsigned)t);
  lds_barrier();

  // tokens [t0, t0 + per) of this thread, cut at T
  const int per = (T + kBlock - 1) / kBlock;
  const int t0 = tid * per;
  unsigned key[kPerThread];
  int rank[kPerThread];
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int t = t0 + i;
    key[i] = (i < per && t < T) ? keys[t] : 0u;
    rank[i] = 0;
  }
  // rank = number of tokens with a smaller (key, token) pair; a thread
  // past T has nothing to rank
  for (int u = 0; u < (t0 < T ? T : 0); ++u) {
    const unsigned ku = keys[u];
#pragma unroll
    for (int i = 0; i < kPerThread; ++i)
      rank[i] += (ku < key[i]) || (ku == key[i] && u < t0 + i);
  }
  bool keep[kPerThread];
  int count = 0;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    keep[i] = i < per && t0 + i < T && rank[i] < K;
    count += keep[i];
  }

  // exclusive prefix sum of count over the workgroup, in thread order
  const int lane = tid & (WAVE_SIZE - 1);
  const int wave = tid / WAVE_SIZE;
  int incl = count;
#pragma unroll
  for (int off = 1; off < WAVE_SIZE; off <<= 1) {
    const int up = __shfl_up(incl, off);
    if (lane >= off) incl += up;
  }
  if (lane == WAVE_SIZE - 1) wave_total[wave] = incl;
  lds_barrier();
  int slot = incl - count;
#pragma unroll
  for (int w = 0; w < kWaves; ++w)
    if (w < wave) slot += wave_total[w];

  int* idx_b = idx + (long)b * K;
  int* inv_b = inv + (long)b * T;
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int t = t0 + i;
    if (i < per && t < T) {
      // exactly K ranks are below K; the slot test keeps the store inside
      // the row whatever the arithmetic above did
      const bool kept = keep[i] && slot < K;
      inv_b[t] = kept ? slot : -1;
      if (kept) idx_b[slot++] = t;
    }
  }
}

// ---- 2. proj + pos[idx], dropout ------------------------------------------

template <bool DROP>
__global__ __launch_bounds__(kBlock) void patch_drop_embed_fwd_kernel(
    const ushort8_t* __restrict__ proj, const ushort8_t* __restrict__ pos,
    const int* __restrict__ idx, ushort8_t* __restrict__ out, int nvec,
    long n_rows, long rows_per_chunk, int T, DropArgs drop) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const long row_begin = (long)blockIdx.y * rows_per_chunk;
  const long row_end = min(row_begin + rows_per_chunk, n_rows);
  const unsigned c0 = (unsigned)vc * 8u;
#pragma unroll 4
  for (long r = row_begin; r < row_end; ++r) {
    // the same for the whole block: a scalar load, a uniform base
    const int t = min(max(idx[r], 0), T - 1);
    const long i = r * nvec + vc;
    const ushort8_t xv = proj[i];
    const ushort8_t pv = pos[(long)t * nvec + vc];
    ushort8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      // torch's bf16 add: the fp32 sum, rounded once
      const unsigned short s = f32_to_bf16(widen(xv[j]) + widen(pv[j]));
      if (DROP) {
        // dropout_fwd on that bf16 value, bit for bit
        const bool keep = hash_keep(drop.seed, drop.thresh, (unsigned)r, c0 + j);
        o[j] = keep ? f32_to_bf16(widen(s) * drop.rscale) : (unsigned short)0;
      } else {
        o[j] = s;
      }
    }
    out[i] = o;
  }
}

// ---- 3. dproj and dpos ----------------------------------------------------

template <bool DROP>
__global__ __launch_bounds__(kBlock) void patch_drop_embed_bwd_kernel(
    const ushort8_t* __restrict__ dy, const int* __restrict__ inv,
    ushort8_t* __restrict__ dproj, ushort8_t* __restrict__ dpos, int nvec,
    int B, int T, int K, DropArgs drop) {
  const int vc = blockIdx.x * kBlock + threadIdx.x;
  if (vc >= nvec) return;
  const int t = blockIdx.y;
  const unsigned c0 = (unsigned)vc * 8u;
  float acc[8] = {};
  for (int b0 = 0; b0 < B; b0 += kWalk) {
    // the round's rows first, then its loads, then the arithmetic
    long row[kWalk];
    ushort8_t v[kWalk];
#pragma unroll
    for (int w = 0; w < kWalk; ++w) {
      const int b = b0 + w;
      // uniform over the workgroup; outside [0, K) is a dropped token
      const int j = b < B ? inv[(long)b * T + t] : -1;
      row[w] = (unsigned)j < (unsigned)K ? (long)b * K + j : -1;
    }
#pragma unroll
    for (int w = 0; w < kWalk; ++w) {
      v[w] = ushort8_t{};
      if (row[w] >= 0) v[w] = dy[row[w] * nvec + vc];
    }
#pragma unroll
    for (int w = 0; w < kWalk; ++w) {
      if (row[w] < 0) continue;
      ushort8_t o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float g = widen(v[w][j]);
        if (DROP) {
          const bool keep =
              hash_keep(drop.seed, drop.thresh, (unsigned)row[w], c0 + j);
          const float s = g * drop.rscale;
          o[j] = keep ? f32_to_bf16(s) : (unsigned short)0;
          acc[j] += keep ? s : 0.f;
        } else {
          acc[j] += g;
        }
      }
      if (DROP) dproj[row[w] * nvec + vc] = o;
    }
  }
  ushort8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f32_to_bf16(acc[j]);
  dpos[(long)t * nvec + vc] = o;
}

#ifdef VITFSDP_KERNELS_ONLY
// explicit instantiations so -Rpass-analysis reports every variant
#define VITFSDP_INSTANTIATE_PATCH_DROP(DROP_)                                \
  template __global__ void patch_drop_embed_fwd_kernel<DROP_>(               \
      const ushort8_t*, const ushort8_t*, const int*, ushort8_t*, int, long, \
      long, int, DropArgs);                                                  \
  template __global__ void patch_drop_embed_bwd_kernel<DROP_>(               \
      const ushort8_t*, const int*, ushort8_t*, ushort8_t*, int, int, int,   \
      int, DropArgs);
VITFSDP_INSTANTIATE_PATCH_DROP(false)
VITFSDP_INSTANTIATE_PATCH_DROP(true)
#undef VITFSDP_INSTANTIATE_PATCH_DROP
#endif

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

void check_counts(const char* op, long T, long K) {
  TORCH_CHECK(T >= 1 && T <= kMaxTokens, op, ": T must be in [1, ",
              kMaxTokens, "], got ", T);
  TORCH_CHECK(K >= 1 && K <= T, op, ": K must be in [1, T = ", T, "], got ",
              K);
}

void check_index(const torch::Tensor& t, const torch::Tensor& like,
                 const char* op, const char* name, long d0, long d1) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() && t.device() == like.device(),
              op, ": ", name,
              " must be a contiguous GPU tensor on the operand's device");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, op, ": ", name,
              " must be int32, is ", t.scalar_type());
  TORCH_CHECK(t.dim() == 2 && t.size(0) == d0 && t.size(1) == d1, op, ": ",
              name, " must be [", d0, ", ", d1, "], is ", t.sizes());
}

// x: proj or dy, [B, K, E]
void check_tokens(const torch::Tensor& x, const char* op, const char* name) {
  check_bf16_operand(x, op, name);
  TORCH_CHECK(x.dim() == 3, op, ": ", name, " must be [B, K, E], is ",
              x.sizes());
  TORCH_CHECK(x.size(2) > 0 && x.size(2) % 8 == 0, op,
              ": last dim must be a multiple of 8, got ", x.size(2));
  TORCH_CHECK(x.size(0) < (1L << 31) && x.size(2) / 8 < (1L << 31), op,
              ": B and E / 8 must each be below 2^31");
}

// p == 0 is no mask: the kernels are then compiled without it
DropArgs embed_drop_args(const char* op, double p, long seed, long rows) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, op, ": p must be in [0, 1), got ", p);
  return p > 0.0 ? drop_args(op, p, seed, rows) : DropArgs{0u, 1.f, 0u};
}

}  // namespace

// (idx int32 [B, K] ascending, inv int32 [B, T]) on the current device
std::vector<torch::Tensor> patch_drop_plan(long seed, long B, long T, long K) {
  const char* op = "patch_drop_plan";
  check_counts(op, T, K);
  TORCH_CHECK(B >= 0 && B < (1L << 31), op, ": B must be in [0, 2^31), got ",
              B);
  auto opts = torch::TensorOptions().dtype(torch::kInt32).device(torch::kCUDA);
  auto idx = torch::empty({B, K}, opts);
  auto inv = torch::empty({B, T}, opts);
  if (B == 0) return {idx, inv};
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(patch_drop_plan_kernel, dim3((unsigned)B), dim3(kBlock),
                     0, stream, idx.data_ptr<int>(), inv.data_ptr<int>(),
                     (int)T, (int)K, (unsigned)seed);
  HIP_CHECK_LAST();
  return {idx, inv};
}

// proj bf16 [B, K, E], pos bf16 [T, E], idx int32 [B, K]; E % 8 == 0,
// 1 <= K <= T <= 1024, 0 <= p < 1
torch::Tensor patch_drop_embed_fwd(torch::Tensor proj, torch::Tensor pos,
                                   torch::Tensor idx, double p, long seed) {
  const char* op = "patch_drop_embed_fwd";
  check_tokens(proj, op, "proj");
  check_bf16_operand(pos, op, "pos");
  const long B = proj.size(0), K = proj.size(1), E = proj.size(2);
  TORCH_CHECK(pos.dim() == 2 && pos.size(1) == E &&
                  pos.device() == proj.device(),
              op, ": pos must be [T, ", E, "] on proj's device, is ",
              pos.sizes());
  const long T = pos.size(0);
  check_counts(op, T, K);
  check_index(idx, proj, op, "idx", B, K);
  const long rows = B * K;
  const DropArgs drop = embed_drop_args(op, p, seed, rows);
  auto out = torch::empty_like(proj);
  if (rows == 0) return out;

  const int nvec = (int)(E / 8);
  // row chunking as in dropout.hip: ~8192 blocks in all
  const long grid_x = (nvec + kBlock - 1) / kBlock;
  const auto [n_chunks, rows_per_chunk] = chunk_plan(rows, grid_x, 8192, 1);
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kernel = p > 0.0 ? patch_drop_embed_fwd_kernel<true>
                        : patch_drop_embed_fwd_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid_x, (unsigned)n_chunks),
                     dim3(kBlock), 0, stream,
                     (const ushort8_t*)proj.data_ptr(),
                     (const ushort8_t*)pos.data_ptr(), idx.data_ptr<int>(),
                     (ushort8_t*)out.data_ptr(), nvec, rows, rows_per_chunk,
                     (int)T, drop);
  HIP_CHECK_LAST();
  return out;
}

// dy bf16 [B, K, E], inv int32 [B, T] -> (dproj [B, K, E], dpos [T, E]);
// at p == 0 dproj IS dy
std::vector<torch::Tensor> patch_drop_embed_bwd(torch::Tensor dy,
                                                torch::Tensor inv, long T,
                                                double p, long seed) {
  const char* op = "patch_drop_embed_bwd";
  check_tokens(dy, op, "dy");
  const long B = dy.size(0), K = dy.size(1), E = dy.size(2);
  check_counts(op, T, K);
  check_index(inv, dy, op, "inv", B, T);
  const DropArgs drop = embed_drop_args(op, p, seed, B * K);
  auto dpos = torch::empty({T, E}, dy.options());
  auto dproj = p > 0.0 ? torch::empty_like(dy) : dy;

  const int nvec = (int)(E / 8);
  const long grid_x = (nvec + kBlock - 1) / kBlock;
  auto stream = at::cuda::getCurrentCUDAStream();
  auto kernel = p > 0.0 ? patch_drop_embed_bwd_kernel<true>
                        : patch_drop_embed_bwd_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid_x, (unsigned)T), dim3(kBlock),
                     0, stream, (const ushort8_t*)dy.data_ptr(),
                     inv.data_ptr<int>(),
                     p > 0.0 ? (ushort8_t*)dproj.data_ptr() : nullptr,
                     (ushort8_t*)dpos.data_ptr(), nvec, (int)B, (int)T, (int)K,
                     drop);
  HIP_CHECK_LAST();
  return {dproj, dpos};
}
#endif  // VITFSDP_KERNELS_ONLY
