// On-device probes that pin the hardware conventions the MFMA kernels
// (fmha.hip, wgemm.hip, fgemm.hip) rely on; the conventions themselves
// are written down in mfma_tiles.h.  Each probe runs one wave and is
// checked by a GPU test in tests/test_gpu_kernels.py.

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>
#endif

#include "mfma_tiles.h"

namespace {

// ds_read_b64_tr_b16 semantics probe: fill LDS with the identity
// pattern lds[i] = i (as raw u16), issue one transpose-read per lane at
// a caller-chosen per-lane base expression, return each lane's 4
// elements.  test_tr16_probe_semantics checks the (lane, elem) -> lds
// index map that tr16_read's callers rely on.
__global__ __launch_bounds__(64) void tr16_probe_kernel(
    unsigned short* __restrict__ out, int mode) {
  HIP_DYNAMIC_SHARED(char, smem_raw)
  unsigned short* lds = reinterpret_cast<unsigned short*>(smem_raw);
  for (int i = threadIdx.x; i < 1024; i += 64) lds[i] = (unsigned short)i;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  unsigned addr_elems;
  switch (mode) {
    case 0: addr_elems = 0; break;                                // uniform
    case 1: addr_elems = (lane & 15) + (lane >> 4) * 64; break;   // guide map
    case 2: addr_elems = (lane & 15) * 4; break;                  // 4/lane
    default: addr_elems = lane * 4; break;
  }
  // byte address into LDS (dynamic region starts at 0: no static smem)
  unsigned addr = addr_elems * 2 + (unsigned)__builtin_amdgcn_groupstaticsize();
  u32x2 v = tr16_read(addr);
  asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v) : : "memory");
  out[lane * 4 + 0] = (unsigned short)(v[0] & 0xffff);
  out[lane * 4 + 1] = (unsigned short)(v[0] >> 16);
  out[lane * 4 + 2] = (unsigned short)(v[1] & 0xffff);
  out[lane * 4 + 3] = (unsigned short)(v[1] >> 16);
}

// Layout probe for the WIDE MFMA (mfma_f32_32x32x16_bf16): one wave,
// row-major fp32 A[32][16] / B[16][32], using the assumed gfx9-family
// fragment maps (A: lane l row l&31, k (l>>5)*8+j; C: lane l col l&31,
// row (l>>5)*4 + g*8 + r at acc[g*4+r]).  The GPU test compares against
// torch.matmul to pin the layout before csrc/fgemm.hip relies on it.
__global__ __launch_bounds__(64) void mfma32_probe_kernel(
    const float* __restrict__ a, const float* __restrict__ b,
    float* __restrict__ c) {
  const int l = threadIdx.x;
  union { unsigned short u[8]; bf16x8 v; } av, bv;
  for (int j = 0; j < 8; ++j) {
    av.u[j] = f32_to_bf16(a[(l & 31) * 16 + (l >> 5) * 8 + j]);
    bv.u[j] = f32_to_bf16(b[((l >> 5) * 8 + j) * 32 + (l & 31)]);
  }
  f32x16 acc = {};
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av.v, bv.v, acc, 0, 0, 0);
  for (int g = 0; g < 4; ++g)
    for (int r = 0; r < 4; ++r)
      c[((l >> 5) * 4 + g * 8 + r) * 32 + (l & 31)] = acc[g * 4 + r];
}

// Layout probe: one wave computes a single 16x16x32 MFMA from row-major
// fp32 A[16][32], B[32][16] using the documented fragment maps; the GPU
// test compares against torch.matmul to pin the layout assumptions.
__global__ __launch_bounds__(64) void mfma_probe_kernel(
    const float* __restrict__ a, const float* __restrict__ b,
    float* __restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int col = lane & 15, seg = lane >> 4;
  bf16x8 af, bf;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    af[j] = (short)f32_to_bf16(a[col * 32 + seg * 8 + j]);
    bf[j] = (short)f32_to_bf16(b[(seg * 8 + j) * 16 + col]);
  }
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
#pragma unroll
  for (int r = 0; r < 4; ++r) c[(seg * 4 + r) * 16 + col] = acc[r];
}
}  // namespace

#ifndef VITFSDP_KERNELS_ONLY
torch::Tensor tr16_probe(long mode) {
  auto out = torch::zeros({64, 4}, torch::TensorOptions()
                                       .dtype(torch::kInt16)
                                       .device(torch::kCUDA));
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(tr16_probe_kernel, dim3(1), dim3(64), 2048, stream,
                     (unsigned short*)out.data_ptr(), (int)mode);
  HIP_CHECK_LAST();
  return out;
}

torch::Tensor mfma32_probe(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.is_cuda() && a.is_contiguous() && a.dim() == 2 &&
              a.size(0) == 32 && a.size(1) == 16);
  TORCH_CHECK(b.is_cuda() && b.is_contiguous() && b.dim() == 2 &&
              b.size(0) == 16 && b.size(1) == 32);
  TORCH_CHECK(a.scalar_type() == torch::kFloat32 &&
              b.scalar_type() == torch::kFloat32);
  auto c = torch::zeros({32, 32}, a.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(mfma32_probe_kernel, dim3(1), dim3(64), 0, stream,
                     a.data_ptr<float>(), b.data_ptr<float>(),
                     c.data_ptr<float>());
  HIP_CHECK_LAST();
  return c;
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b) {
  TORCH_CHECK(a.is_cuda() && a.sizes() == torch::IntArrayRef({16, 32}));
  TORCH_CHECK(b.is_cuda() && b.sizes() == torch::IntArrayRef({32, 16}));
  auto a32 = a.to(torch::kFloat32).contiguous();
  auto b32 = b.to(torch::kFloat32).contiguous();
  auto c = torch::empty({16, 16}, a32.options());
  auto stream = at::cuda::getCurrentCUDAStream();
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, stream,
                     a32.data_ptr<float>(), b32.data_ptr<float>(),
                     c.data_ptr<float>());
  HIP_CHECK_LAST();
  return c;
}
#endif  // VITFSDP_KERNELS_ONLY
