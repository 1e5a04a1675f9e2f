// hipBLASLt invocations with explicit algorithm indices and fused
// epilogues (ROADMAP items 5/6).
//
// PyTorch's TunableOp crashes this ROCm 7.2 stack, so algorithm
// selection is done offline by csrc/tools/hipblaslt_search.cpp; the
// entries here apply a chosen index from Python:
//
//   d        = _C.lt_gemm(a, b, algo_index, bias)        # d = a @ b (+bias)
//   d, aux   = _C.lt_gemm_gelu(a, b, bias, algo_index)   # d = gelu(a@b+bias)
//   dx, dbia = _C.lt_gemm_dgelu_bgrad(dy, w, aux, algo_index)
//   dx       = _C.dgrad_tn(dy, w, algo_index)            # dx = dy @ w, TN
//
// algo_index < 0 uses the library heuristic (same pick as torch's
// matmul).  a/b may be row-contiguous tensors OR transposed views of
// row-contiguous tensors — both map onto hipBLASLt op flags with zero
// copies, which is what lets the dispatch-mode router (ops/linear.py)
// reroute the training GEMMs (forward x@W^T, dgrad dy@W, wgrad dy^T@x)
// without materializing any transpose.
//
// Layout math: row-major C[M,N] = A @ B is computed as the column-major
// dual D[N,M] = opA(B_mem) @ opB(A_mem): a row-contiguous operand is
// its own transpose in column-major interpretation (op=N), a transposed
// view needs op=T; leading dims are the underlying row lengths.  This
// reproduces exactly the Tensile kernel families the trace shows
// (Cijk_Alik TN fwd, Cijk_Ailk NN dgrad, Cijk_Ailk_Bjlk NT wgrad).

#ifndef VITFSDP_KERNELS_ONLY
#include <ATen/cuda/CUDAContext.h>
#include <torch/extension.h>

#include <hipblaslt/hipblaslt-ext.hpp>
#include <hipblaslt/hipblaslt.h>

#include "transpose.h"

#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace {

hipblasLtHandle_t lt_handle() {
  static hipblasLtHandle_t handle = [] {
    hipblasLtHandle_t h;
    if (hipblasLtCreate(&h) != HIPBLAS_STATUS_SUCCESS)
      throw std::runtime_error("hipblasLtCreate failed");
    return h;
  }();
  return handle;
}

void* lt_workspace(size_t bytes) {
  static void* ws = nullptr;
  static size_t ws_bytes = 0;
  static std::mutex mu;
  std::lock_guard<std::mutex> lock(mu);
  if (bytes > ws_bytes) {
    if (ws) (void)hipFree(ws);
    if (hipMalloc(&ws, bytes) != hipSuccess)
      throw std::runtime_error("lt_gemm workspace alloc failed");
    ws_bytes = bytes;
  }
  return ws;
}

constexpr size_t kMaxWorkspace = 128u << 20;

// dgrad_tn's W^T: one grow-only buffer per device, never returned, like
// the workspace above (at ViT-10B at most 210 MB, the fc1/fc2 weight).
// It is taken outside the caching allocator on purpose: the step's
// memory peak lies in the backward, a few GiB under the card's size, and
// a transient of this size per dgrad should not pass through the
// allocator's pools there.  Consecutive users are ordered by their
// stream alone, so the buffer belongs to the first stream that asks;
// nullptr sends a caller on another stream to the allocator for that
// call.  Growing frees the old buffer, and hipFree waits for the device.
constexpr int kMaxDevices = 16;

void* wt_scratch(int device, size_t bytes, hipStream_t stream) {
  struct Slot {
    void* ptr = nullptr;
    size_t bytes = 0;
    hipStream_t owner = nullptr;
    bool owned = false;
  };
  static Slot slots[kMaxDevices];
  static std::mutex mu;
  if (device < 0 || device >= kMaxDevices) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  Slot& s = slots[device];
  if (s.owned && s.owner != stream) return nullptr;
  if (bytes > s.bytes) {
    if (s.ptr) (void)hipFree(s.ptr);
    s.ptr = nullptr;
    s.bytes = 0;
    if (hipMalloc(&s.ptr, bytes) != hipSuccess) {
      (void)hipGetLastError();
      s.ptr = nullptr;
      return nullptr;  // the caching allocator may still have room
    }
    s.bytes = bytes;
  }
  s.owner = stream;
  s.owned = true;
  return s.ptr;
}

// 2-D operand layout: row-contiguous (op N in the column-major dual) or
// a transposed view of a row-contiguous base (op T).  Returns false if
// neither (caller must materialize).
struct Operand {
  hipblasOperation_t op;
  int64_t ld;
  const void* ptr;
};

bool classify(const torch::Tensor& t, Operand& out) {
  const int64_t r = t.size(0), c = t.size(1);
  const int64_t s0 = t.stride(0), s1 = t.stride(1);
  out.ptr = t.data_ptr();
  // row-contiguous [r, c]: column-major read gives the transpose we
  // need directly
  if (s1 == 1 && (s0 == c || r == 1)) {
    out.op = HIPBLAS_OP_N;
    out.ld = c;  // underlying row length
    return true;
  }
  // transposed view of a row-contiguous [c, r] base
  if (s0 == 1 && (s1 == r || c == 1)) {
    out.op = HIPBLAS_OP_T;
    out.ld = r;
    return true;
  }
  return false;
}

hipblasLtMatmulAlgo_t pick_algo(hipblaslt_ext::Gemm& gemm, long algo_index,
                                const char* what) {
  hipblasLtMatmulAlgo_t algo;
  if (algo_index >= 0) {
    std::vector<hipblasLtMatmulHeuristicResult_t> found;
    std::vector<int> idx{static_cast<int>(algo_index)};
    if (hipblaslt_ext::getAlgosFromIndex(lt_handle(), idx, found) ==
            HIPBLAS_STATUS_SUCCESS &&
        !found.empty()) {
      size_t need = 0;
      if (gemm.isAlgoSupported(found[0].algo, need) ==
              HIPBLAS_STATUS_SUCCESS &&
          need <= kMaxWorkspace) {
        return found[0].algo;
      }
    }
    // a tuned index that does not validate for THIS problem variant
    // (e.g. searched without the bias epilogue) falls back to the
    // heuristic: a worse kernel pick must never become a crash
  }
  hipblaslt_ext::GemmPreference pref;
  pref.setMaxWorkspaceBytes(kMaxWorkspace);
  std::vector<hipblasLtMatmulHeuristicResult_t> heur;
  TORCH_CHECK(
      gemm.algoGetHeuristic(1, pref, heur) == HIPBLAS_STATUS_SUCCESS &&
          !heur.empty(),
      what, ": no heuristic algorithm found");
  return heur[0].algo;
}

// Shared driver: row-major d[M,N] = a[M,K] @ b[K,N] with an optional
// fused epilogue.  bias: input vector length N (BIAS-family modes) or
// OUTPUT vector length N (BGRAD-family modes).  aux: [M,N] bf16, input
// for DGELU*, output for *_AUX_* modes.
torch::Tensor lt_run(const torch::Tensor& a, const torch::Tensor& b,
                     long algo_index, hipblasLtEpilogue_t mode,
                     void* bias_ptr, void* aux_ptr, const char* what) {
  TORCH_CHECK(a.is_cuda() && b.is_cuda(), what, ": CUDA tensors required");
  TORCH_CHECK(a.dtype() == torch::kBFloat16 && b.dtype() == torch::kBFloat16,
              what, ": bf16 only");
  TORCH_CHECK(a.dim() == 2 && b.dim() == 2 && a.size(1) == b.size(0), what,
              ": a[M,K] @ b[K,N] expected");
  const int64_t M = a.size(0), K = a.size(1), N = b.size(1);

  Operand opa, opb;
  torch::Tensor a_hold = a, b_hold = b;
  if (!classify(a_hold, opa)) {
    a_hold = a.contiguous();
    classify(a_hold, opa);
  }
  if (!classify(b_hold, opb)) {
    b_hold = b.contiguous();
    classify(b_hold, opb);
  }
  auto d = torch::empty({M, N}, a_hold.options());

  auto handle = lt_handle();
  hipStream_t stream = at::cuda::getCurrentCUDAStream();

  // column-major dual: A-slot <- b memory, B-slot <- a memory
  hipblaslt_ext::Gemm gemm(handle, opb.op, opa.op, HIP_R_16BF, HIP_R_16BF,
                           HIP_R_16BF, HIP_R_16BF, HIPBLAS_COMPUTE_32F);
  float alpha = 1.0f, beta = 0.0f;
  hipblaslt_ext::GemmEpilogue epilogue;
  hipblaslt_ext::GemmInputs inputs;
  if (mode != HIPBLASLT_EPILOGUE_DEFAULT) {
    epilogue.setMode(mode);
    if (bias_ptr != nullptr) epilogue.setBiasDataType(HIP_R_16BF);
    if (aux_ptr != nullptr) {
      epilogue.setAuxDataType(HIP_R_16BF);
      epilogue.setAuxLeadingDimension((int)N);
      epilogue.setAuxBatchStride((int)(M * N));
    }
  }
  if (bias_ptr != nullptr) inputs.setBias(bias_ptr);
  if (aux_ptr != nullptr) inputs.setAux(aux_ptr);
  inputs.setA(const_cast<void*>(opb.ptr));
  inputs.setB(const_cast<void*>(opa.ptr));
  inputs.setC(d.data_ptr());
  inputs.setD(d.data_ptr());
  inputs.setAlpha(&alpha);
  inputs.setBeta(&beta);

  hipblaslt_ext::GemmProblemType ptype(opb.op, opa.op, HIP_R_16BF, HIP_R_16BF,
                                       HIP_R_16BF, HIP_R_16BF,
                                       HIPBLAS_COMPUTE_32F);
  // (m, n, k) = (N, M, K); lda/ldb are the operands' underlying row
  // lengths, ldc/ldd = N
  TORCH_CHECK(gemm.setProblem(N, M, K, 1, opb.ld, opa.ld, N, N, 0, 0, 0, 0,
                              epilogue, inputs,
                              ptype) == HIPBLAS_STATUS_SUCCESS,
              what, ": setProblem failed");

  auto algo = pick_algo(gemm, algo_index, what);
  TORCH_CHECK(gemm.initialize(algo, lt_workspace(kMaxWorkspace), false,
                              stream) == HIPBLAS_STATUS_SUCCESS,
              what, ": initialize failed");
  TORCH_CHECK(gemm.run(stream) == HIPBLAS_STATUS_SUCCESS, what,
              ": run failed");
  return d;
}

}  // namespace

torch::Tensor lt_gemm(torch::Tensor a, torch::Tensor b, long algo_index,
                      c10::optional<torch::Tensor> bias) {
  void* bias_ptr = nullptr;
  torch::Tensor bias_c;
  hipblasLtEpilogue_t mode = HIPBLASLT_EPILOGUE_DEFAULT;
  if (bias.has_value()) {
    bias_c = bias->contiguous();
    TORCH_CHECK(bias_c.is_cuda() && bias_c.dtype() == torch::kBFloat16 &&
                    bias_c.numel() == b.size(1),
                "lt_gemm: bias must be bf16 CUDA of length N");
    bias_ptr = bias_c.data_ptr();
    mode = HIPBLASLT_EPILOGUE_BIAS;
  }
  return lt_run(a, b, algo_index, mode, bias_ptr, nullptr, "lt_gemm");
}

// dx[tok, in] = dy[tok, out] @ w[out, in], the input gradient of a
// linear, as the library's TN form: w is transposed into W^T [in, out]
// (csrc/transpose.hip, one read and one write of the weight) and the
// GEMM sees it as the op-T operand, the layout of a forward x @ W^T, so
// the tuned dual key is ("T","N", in, tok, out).  W^T is rebuilt on
// every call: weights change every step and FSDP storage resizing makes
// addresses recur, so nothing keyed by address would be safe to keep.
torch::Tensor dgrad_tn(torch::Tensor dy, torch::Tensor w, long algo_index) {
  const char* what = "dgrad_tn";
  TORCH_CHECK(dy.is_cuda() && w.is_cuda() && dy.device() == w.device(), what,
              ": dy and w must be on the same GPU");
  TORCH_CHECK(dy.scalar_type() == torch::kBFloat16 &&
                  w.scalar_type() == torch::kBFloat16,
              what, ": bf16 only");
  TORCH_CHECK(dy.dim() == 2 && w.dim() == 2 && dy.size(1) == w.size(0), what,
              ": dy[tok, out] @ w[out, in] expected");
  const int64_t tok = dy.size(0), out = w.size(0), in = w.size(1);
  TORCH_CHECK(tok > 0 && out > 0 && in > 0, what, ": empty operand");
  TORCH_CHECK(dy.stride(1) == 1 && dy.stride(0) == out && w.stride(1) == 1 &&
                  w.stride(0) == in,
              what, ": operands must be row-contiguous (no silent copy)");
  TORCH_CHECK(in % 8 == 0 && out % 8 == 0, what,
              ": in and out must be a multiple of 8, got in = ", in,
              ", out = ", out);
  TORCH_CHECK(reinterpret_cast<uintptr_t>(w.data_ptr()) % 16 == 0, what,
              ": w must be 16-byte aligned");
  const int device = w.get_device();
  TORCH_CHECK(device == at::cuda::current_device(), what,
              ": operands must be on the current device");

  hipStream_t stream = at::cuda::getCurrentCUDAStream();
  const size_t bytes = (size_t)in * (size_t)out * sizeof(uint16_t);
  torch::Tensor hold;
  void* wt = wt_scratch(device, bytes, stream);
  if (wt == nullptr) {
    hold = torch::empty({in, out}, w.options());
    wt = hold.data_ptr();
  }
  transpose2d_launch(w.data_ptr(), wt, out, in, stream, what);
  // W^T [in, out] contiguous, seen as its transposed view [out, in]
  auto wt_view = torch::from_blob(wt, {out, in}, {1, out}, w.options());
  return lt_run(dy, wt_view, algo_index, HIPBLASLT_EPILOGUE_DEFAULT, nullptr,
                nullptr, what);
}

// d = gelu(a @ b + bias), aux = a @ b + bias (the pre-activation, saved
// for the backward's DGELU epilogue).  NOTE: hipBLASLt's GELU is the
// tanh approximation; numerics policy handled by the Python caller.
std::vector<torch::Tensor> lt_gemm_gelu(torch::Tensor a, torch::Tensor b,
                                        c10::optional<torch::Tensor> bias,
                                        long algo_index) {
  const int64_t M = a.size(0), N = b.size(1);
  auto aux = torch::empty({M, N}, a.options().dtype(torch::kBFloat16));
  void* bias_ptr = nullptr;
  torch::Tensor bias_c;
  hipblasLtEpilogue_t mode = HIPBLASLT_EPILOGUE_GELU_AUX;
  if (bias.has_value()) {
    bias_c = bias->contiguous();
    TORCH_CHECK(bias_c.is_cuda() && bias_c.dtype() == torch::kBFloat16 &&
                    bias_c.numel() == N,
                "lt_gemm_gelu: bias must be bf16 CUDA of length N");
    bias_ptr = bias_c.data_ptr();
    mode = HIPBLASLT_EPILOGUE_GELU_AUX_BIAS;
  }
  auto d = lt_run(a, b, algo_index, mode, bias_ptr, aux.data_ptr(),
                  "lt_gemm_gelu");
  return {d, aux};
}

// dx = dgelu(dy @ w, aux) with dbias = column-sums of dx fused
// (DGELU_BGRAD): the backward of h = gelu(pre) where pre = x@W1^T+b1 —
// dy@w is d(gelu_out), aux is pre, dx is d(pre), dbias is db1.
std::vector<torch::Tensor> lt_gemm_dgelu_bgrad(torch::Tensor dy,
                                               torch::Tensor w,
                                               torch::Tensor aux,
                                               long algo_index) {
  const int64_t M = dy.size(0), N = w.size(1);
  TORCH_CHECK(aux.is_cuda() && aux.dtype() == torch::kBFloat16 &&
                  aux.dim() == 2 && aux.size(0) == M && aux.size(1) == N &&
                  aux.is_contiguous(),
              "lt_gemm_dgelu_bgrad: aux must be contiguous bf16 [M,N]");
  auto dbias = torch::empty({N}, dy.options().dtype(torch::kBFloat16));
  auto d = lt_run(dy, w, algo_index, HIPBLASLT_EPILOGUE_DGELU_BGRAD,
                  dbias.data_ptr(), aux.data_ptr(), "lt_gemm_dgelu_bgrad");
  return {d, dbias};
}

#endif  // VITFSDP_KERNELS_ONLY
