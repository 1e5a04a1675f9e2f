// Fused softmax cross-entropy (kernel K9): log-softmax +
// NLL in one pass over bf16 logits with fp32 accumulation, mean
// reduction (reference: torch.nn.CrossEntropyLoss at
// run_vit_training.py:229,262).  Shapes are small ([batch, 1000]); one
// 256-thread block per row, loss accumulated with one fp32 atomic.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include <climits>

#include "common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / WAVE_SIZE;

__global__ void ce_fwd_kernel(const unsigned short* __restrict__ logits,
                              const long* __restrict__ target,
                              float* __restrict__ loss_out,
                              float* __restrict__ lse_out, int c,
                              float inv_n) {
  __shared__ float scratch[kWaves];
  const long row = blockIdx.x;
  const unsigned short* lr = logits + row * c;

  float m = -INFINITY;
  for (int i = threadIdx.x; i < c; i += kBlock)
    m = fmaxf(m, bf16_to_f32(lr[i]));
  m = block_max<kWaves>(m, scratch);

  float s = 0.f;
  for (int i = threadIdx.x; i < c; i += kBlock)
    s += __expf(bf16_to_f32(lr[i]) - m);
  s = block_sum<kWaves>(s, scratch);

  const float lse = m + __logf(s);
  if (threadIdx.x == 0) {
    lse_out[row] = lse;
    const float tl = bf16_to_f32(lr[target[row]]);
    atomicAdd(loss_out, (lse - tl) * inv_n);
  }
}

__global__ void ce_bwd_kernel(const unsigned short* __restrict__ logits,
                              const long* __restrict__ target,
                              const float* __restrict__ lse,
                              const float* __restrict__ dloss,
                              unsigned short* __restrict__ dlogits, int c,
                              float inv_n) {
  const long row = blockIdx.x;
  const unsigned short* lr = logits + row * c;
  unsigned short* dr = dlogits + row * c;
  const float scale = (*dloss) * inv_n;
  const float row_lse = lse[row];
  const long tgt = target[row];
  for (int i = threadIdx.x; i < c; i += kBlock) {
    float p = __expf(bf16_to_f32(lr[i]) - row_lse);
    float d = (p - (i == tgt ? 1.f : 0.f)) * scale;
    dr[i] = f32_to_bf16(d);
  }
}

}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
namespace {

// The kernels index raw pointers by the shape of logits alone, so every
// operand is checked against it before a launch.  An empty batch is
// refused: its mean loss is 0/0 and there is no row to launch a block for.
void check_logits_target(const char* fn, const torch::Tensor& logits,
                         const torch::Tensor& target) {
  TORCH_CHECK(logits.is_cuda(), fn, ": logits must be a GPU tensor");
  TORCH_CHECK(logits.scalar_type() == torch::kBFloat16, fn,
              ": logits must be bf16, got ", logits.scalar_type());
  TORCH_CHECK(logits.dim() == 2 && logits.size(0) > 0 && logits.size(1) > 0 &&
                  logits.size(1) <= INT_MAX,
              fn, ": logits must be a non-empty [N, C], got ", logits.sizes());
  TORCH_CHECK(logits.is_contiguous(), fn, ": logits must be contiguous");
  TORCH_CHECK(target.is_cuda() && target.device() == logits.device(), fn,
              ": target must be a GPU tensor on the device of logits");
  TORCH_CHECK(target.scalar_type() == torch::kLong, fn,
              ": target must be int64, got ", target.scalar_type());
  TORCH_CHECK(target.dim() == 1 && target.size(0) == logits.size(0), fn,
              ": target must have shape [N] = [", logits.size(0), "], got ",
              target.sizes());
  TORCH_CHECK(target.is_contiguous(), fn, ": target must be contiguous");
}

}  // namespace

std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits,
                                             torch::Tensor target) {
  check_logits_target("cross_entropy_fwd", logits, target);
  const long n = logits.size(0);
  const int c = (int)logits.size(1);
  auto opts = logits.options().dtype(torch::kFloat32);
  auto loss = torch::zeros({}, opts);
  auto lse = torch::empty({n}, opts);
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ce_fwd_kernel, dim3((unsigned)n), dim3(kBlock), 0, stream,
                     (const unsigned short*)logits.data_ptr(),
                     target.data_ptr<long>(), loss.data_ptr<float>(),
                     lse.data_ptr<float>(), c, 1.f / n);
  HIP_CHECK_LAST();
  return {loss, lse};
}

torch::Tensor cross_entropy_bwd(torch::Tensor dloss, torch::Tensor logits,
                                torch::Tensor target, torch::Tensor lse) {
  const char* fn = "cross_entropy_bwd";
  check_logits_target(fn, logits, target);
  const long n = logits.size(0);
  const int c = (int)logits.size(1);
  TORCH_CHECK(lse.is_cuda() && lse.device() == logits.device(), fn,
              ": lse must be a GPU tensor on the device of logits");
  TORCH_CHECK(lse.scalar_type() == torch::kFloat32, fn,
              ": lse must be fp32, got ", lse.scalar_type());
  TORCH_CHECK(lse.dim() == 1 && lse.size(0) == n, fn,
              ": lse must have shape [N] = [", n, "], got ", lse.sizes());
  TORCH_CHECK(lse.is_contiguous(), fn, ": lse must be contiguous");
  TORCH_CHECK(dloss.is_cuda() && dloss.device() == logits.device(), fn,
              ": dloss must be a GPU tensor on the device of logits");
  TORCH_CHECK(dloss.scalar_type() == torch::kFloat32, fn,
              ": dloss must be fp32 like the loss, got ", dloss.scalar_type());
  TORCH_CHECK(dloss.numel() == 1, fn, ": dloss must hold one element, got ",
              dloss.sizes());
  auto dlogits = torch::empty_like(logits);
  // one element, but possibly a view with a storage offset or stride
  auto dloss_f = dloss.contiguous();
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(ce_bwd_kernel, dim3((unsigned)n), dim3(kBlock), 0, stream,
                     (const unsigned short*)logits.data_ptr(),
                     target.data_ptr<long>(), lse.data_ptr<float>(),
                     dloss_f.data_ptr<float>(),
                     (unsigned short*)dlogits.data_ptr(), c, 1.f / n);
  HIP_CHECK_LAST();
  return dlogits;
}

#endif  // VITFSDP_KERNELS_ONLY
