// Exact-erf GELU in fp32, forward and backward, shared by gelu.hip and
// dropout.hip so the two evaluate one formula with one set of constants.
#pragma once

#include <hip/hip_runtime.h>

// gelu(x) = x * Phi(x): torch's F.gelu with approximate='none'
__device__ __forceinline__ float gelu_erf_f32(float x) {
  constexpr float kAlpha = 0.70710678118654752440f;     // 1/sqrt(2)
  return 0.5f * x * (1.f + erff(x * kAlpha));
}

// d/dx gelu(x) * dy with gelu(x) = x * Phi(x): the formula (and fp32
// evaluation) of torch's GeluBackward with approximate='none'
__device__ __forceinline__ float gelu_bwd_one(float dy, float x) {
  constexpr float kAlpha = 0.70710678118654752440f;     // 1/sqrt(2)
  constexpr float kBeta = 0.39894228040143267794f;      // 1/sqrt(2*pi)
  const float cdf = 0.5f * (1.f + erff(x * kAlpha));
  const float pdf = expf(-0.5f * x * x) * kBeta;
  return dy * (cdf + x * pdf);
}
