// Python bindings for the in-tree CDNA4 (gfx950) kernels.
// Built ahead of time via `python setup.py build_ext --inplace`
// (PYTORCH_ROCM_ARCH=gfx950); the resulting _C.so lives inside the
// package so it travels with repo snapshots to GPU boxes.

#include <torch/extension.h>

std::vector<torch::Tensor> layernorm_fwd(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor b, double eps);
std::vector<torch::Tensor> layernorm_bwd(torch::Tensor dy, torch::Tensor x,
                                         torch::Tensor w, torch::Tensor mean,
                                         torch::Tensor rstd);
std::vector<torch::Tensor> layernorm_add_fwd(torch::Tensor x,
                                             torch::Tensor res,
                                             torch::Tensor w, torch::Tensor b,
                                             double eps);
std::vector<torch::Tensor> layernorm_add_bwd(torch::Tensor dy,
                                             torch::Tensor dsum,
                                             torch::Tensor sum,
                                             torch::Tensor w,
                                             torch::Tensor mean,
                                             torch::Tensor rstd);

void fused_adamw(std::vector<torch::Tensor> params,
                 std::vector<torch::Tensor> grads,
                 std::vector<torch::Tensor> exp_avgs,
                 std::vector<torch::Tensor> exp_avg_sqs,
                 std::vector<c10::optional<torch::Tensor>> mirrors,
                 double lr,
                 double beta1, double beta2, double eps, double weight_decay,
                 double bias_c1, double bias_c2,
                 c10::optional<torch::Tensor> grad_scale,
                 double grad_prescale);
torch::Tensor multi_tensor_sqnorm(std::vector<torch::Tensor> tensors);
void multi_tensor_scale(std::vector<torch::Tensor> tensors, double factor);
void multi_tensor_scale_tensor(std::vector<torch::Tensor> tensors,
                               torch::Tensor factor);

std::vector<torch::Tensor> cross_entropy_fwd(torch::Tensor logits,
                                             torch::Tensor target);
torch::Tensor cross_entropy_bwd(torch::Tensor dloss, torch::Tensor logits,
                                torch::Tensor target, torch::Tensor lse);

std::vector<torch::Tensor> fmha_fwd(torch::Tensor q, torch::Tensor k,
                                    torch::Tensor v, double scale,
                                    double p_drop, long seed);
std::vector<torch::Tensor> fmha_bwd(torch::Tensor dout, torch::Tensor q,
                                    torch::Tensor k, torch::Tensor v,
                                    torch::Tensor o, torch::Tensor lse,
                                    double scale, double p_drop, long seed);
std::vector<torch::Tensor> fmha_fwd_qkv(torch::Tensor qkv, long num_heads,
                                        double scale, double p_drop,
                                        long seed);
torch::Tensor fmha_bwd_qkv(torch::Tensor dout, torch::Tensor qkv,
                           torch::Tensor o, torch::Tensor lse,
                           long num_heads, double scale, double p_drop,
                           long seed);
torch::Tensor fmha_rowdot(torch::Tensor dout, torch::Tensor o);
std::vector<torch::Tensor> gelu_bwd_colsum(torch::Tensor dy, torch::Tensor x);
std::vector<torch::Tensor> gelu_bwd_colsum_t(torch::Tensor dy,
                                             torch::Tensor x);
std::vector<torch::Tensor> gelu_dropout_bwd_colsum(torch::Tensor dy,
                                                   torch::Tensor x, double p,
                                                   long seed);
std::vector<torch::Tensor> gelu_dropout_bwd_colsum_t(torch::Tensor dy,
                                                     torch::Tensor x, double p,
                                                     long seed);
torch::Tensor transpose2d(torch::Tensor x);
std::vector<torch::Tensor> transpose_colsum(torch::Tensor x);
torch::Tensor dropout_fwd(torch::Tensor x, double p, long seed);
torch::Tensor dropout_add_fwd(torch::Tensor x, torch::Tensor res, double p,
                              long seed);
torch::Tensor gelu_dropout_fwd(torch::Tensor x, double p, long seed);
torch::Tensor gelu_dropout_bwd(torch::Tensor dy, torch::Tensor x, double p,
                               long seed);
torch::Tensor drop_path_fwd(torch::Tensor x, long n_samples, double p_path,
                            long seed_path, double p_elem, long seed_elem);
torch::Tensor drop_path_add_fwd(torch::Tensor x, torch::Tensor res,
                                long n_samples, double p_path, long seed_path,
                                double p_elem, long seed_elem);
torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b);
torch::Tensor mfma32_probe(torch::Tensor a, torch::Tensor b);
torch::Tensor tr16_probe(long mode);
std::vector<torch::Tensor> wgrad_gemm(torch::Tensor a, torch::Tensor b,
                                      bool with_bias);
torch::Tensor fwd_gemm(torch::Tensor x, torch::Tensor w,
                       c10::optional<torch::Tensor> bias);
std::vector<torch::Tensor> fwd_gemm_gelu(torch::Tensor x, torch::Tensor w,
                                         torch::Tensor bias);
torch::Tensor lt_gemm(torch::Tensor a, torch::Tensor b, long algo_index,
                      c10::optional<torch::Tensor> bias);
std::vector<torch::Tensor> lt_gemm_gelu(torch::Tensor a, torch::Tensor b,
                                        c10::optional<torch::Tensor> bias,
                                        long algo_index);
std::vector<torch::Tensor> lt_gemm_dgelu_bgrad(torch::Tensor dy,
                                               torch::Tensor w,
                                               torch::Tensor aux,
                                               long algo_index);
torch::Tensor dgrad_tn(torch::Tensor dy, torch::Tensor w, long algo_index);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "MI355X-native CDNA4 kernels for the FSDP ViT framework";
  m.def("layernorm_fwd", &layernorm_fwd, "LayerNorm forward (bf16, fp32 stats)");
  m.def("layernorm_bwd", &layernorm_bwd, "LayerNorm backward");
  m.def("layernorm_add_fwd", &layernorm_add_fwd,
        "fused residual-add + LayerNorm forward");
  m.def("layernorm_add_bwd", &layernorm_add_bwd,
        "fused residual-add + LayerNorm backward");
  m.def("fused_adamw", &fused_adamw,
        "multi-tensor AdamW step (fp32 master, fp32/bf16 grads with "
        "folded prescale + deferred clip)",
        py::arg("params"), py::arg("grads"), py::arg("exp_avgs"),
        py::arg("exp_avg_sqs"), py::arg("mirrors"), py::arg("lr"),
        py::arg("beta1"), py::arg("beta2"), py::arg("eps"),
        py::arg("weight_decay"), py::arg("bias_c1"), py::arg("bias_c2"),
        py::arg("grad_scale") = py::none(), py::arg("grad_prescale") = 1.0);
  m.def("multi_tensor_sqnorm", &multi_tensor_sqnorm,
        "sum of squares over tensor list");
  m.def("multi_tensor_scale", &multi_tensor_scale, "in-place scalar scale");
  m.def("multi_tensor_scale_tensor", &multi_tensor_scale_tensor,
        "in-place scale by device scalar");
  m.def("cross_entropy_fwd", &cross_entropy_fwd, "fused softmax CE forward");
  m.def("cross_entropy_bwd", &cross_entropy_bwd, "fused softmax CE backward");
  m.def("fmha_fwd", &fmha_fwd,
        "flash attention forward (bf16, head_dim<=192; in-kernel "
        "attention dropout via a counter-hash mask)",
        py::arg("q"), py::arg("k"), py::arg("v"), py::arg("scale"),
        py::arg("p_drop") = 0.0, py::arg("seed") = 0);
  m.def("fmha_bwd", &fmha_bwd,
        "flash attention backward (fused FA2-style; regenerates the "
        "dropout mask from the seed)",
        py::arg("dout"), py::arg("q"), py::arg("k"), py::arg("v"),
        py::arg("o"), py::arg("lse"), py::arg("scale"),
        py::arg("p_drop") = 0.0, py::arg("seed") = 0);
  m.def("fmha_fwd_qkv", &fmha_fwd_qkv,
        "flash attention forward on the fused [B,T,3,H,D] qkv projection "
        "(zero-copy strided IO, O returned as [B,T,E])",
        py::arg("qkv"), py::arg("num_heads"), py::arg("scale"),
        py::arg("p_drop") = 0.0, py::arg("seed") = 0);
  m.def("fmha_bwd_qkv", &fmha_bwd_qkv,
        "flash attention backward producing the fused dqkv [B,T,3,H,D]",
        py::arg("dout"), py::arg("qkv"), py::arg("o"), py::arg("lse"),
        py::arg("num_heads"), py::arg("scale"), py::arg("p_drop") = 0.0,
        py::arg("seed") = 0);
  m.def("fmha_rowdot", &fmha_rowdot,
        "Delta = rowsum(dO * O) of the attention backward, fp32 [B,H,T], "
        "for contiguous [B,H,T,D] operands",
        py::arg("dout"), py::arg("o"));
  m.def("gelu_bwd_colsum", &gelu_bwd_colsum,
        "(dx, colsum): exact-erf GELU backward and the bf16 column sums "
        "of dx over all rows (fc1 bias gradient) in one pass",
        py::arg("dy"), py::arg("x"));
  m.def("gelu_bwd_colsum_t", &gelu_bwd_colsum_t,
        "(dx, colsum, dx^T): gelu_bwd_colsum with dx^T [hid, rows] as a "
        "third output; dx and colsum are bit-identical to gelu_bwd_colsum's",
        py::arg("dy"), py::arg("x"));
  m.def("transpose2d", &transpose2d,
        "bf16 [R, C] contiguous -> [C, R] contiguous (C % 8 == 0)",
        py::arg("x"));
  m.def("transpose_colsum", &transpose_colsum,
        "(x^T, colsum): transpose2d plus the bf16 column sums of x over "
        "all rows (a linear's bias gradient) from the same read; fp32 "
        "accumulation in a fixed order",
        py::arg("x"));
  m.def("dropout_fwd", &dropout_fwd,
        "hidden dropout with the in-kernel (seed, row, col) hash mask: "
        "keep ? x / (1 - p) : 0; the same call on dy is its backward",
        py::arg("x"), py::arg("p"), py::arg("seed"));
  m.def("dropout_add_fwd", &dropout_add_fwd,
        "x + dropout(res) in one pass (residual add with the branch's "
        "dropout folded in), rounded once",
        py::arg("x"), py::arg("res"), py::arg("p"), py::arg("seed"));
  m.def("gelu_dropout_fwd", &gelu_dropout_fwd,
        "dropout(gelu(x)) in one pass, exact-erf GELU, rounded once",
        py::arg("x"), py::arg("p"), py::arg("seed"));
  m.def("gelu_dropout_bwd", &gelu_dropout_bwd,
        "backward of gelu_dropout_fwd from dy and the pre-activation x; "
        "regenerates the mask from the seed",
        py::arg("dy"), py::arg("x"), py::arg("p"), py::arg("seed"));
  m.def("gelu_dropout_bwd_colsum", &gelu_dropout_bwd_colsum,
        "(dx, colsum): gelu_dropout_bwd and the bf16 column sums of dx "
        "over all rows (fc1 bias gradient) in one pass; dx is "
        "bit-identical to gelu_dropout_bwd's",
        py::arg("dy"), py::arg("x"), py::arg("p"), py::arg("seed"));
  m.def("gelu_dropout_bwd_colsum_t", &gelu_dropout_bwd_colsum_t,
        "(dx, colsum, dx^T): gelu_dropout_bwd_colsum with dx^T [hid, rows] "
        "as a third output; dx and colsum are bit-identical to "
        "gelu_dropout_bwd_colsum's",
        py::arg("dy"), py::arg("x"), py::arg("p"), py::arg("seed"));
  m.def("drop_path_fwd", &drop_path_fwd,
        "stochastic depth with the branch's element dropout folded in: "
        "sample b = row / (rows / n_samples) is kept iff "
        "dropout_hash(seed_path, b, 0) passes p_path; a dropped sample's "
        "rows are written as zeros without being read; the same call on "
        "dy is its backward",
        py::arg("x"), py::arg("n_samples"), py::arg("p_path"),
        py::arg("seed_path"), py::arg("p_elem"), py::arg("seed_elem"));
  m.def("drop_path_add_fwd", &drop_path_add_fwd,
        "x + drop_path(res) in one pass, rounded once; a dropped sample's "
        "rows of res are not read and x passes through bit for bit",
        py::arg("x"), py::arg("res"), py::arg("n_samples"),
        py::arg("p_path"), py::arg("seed_path"), py::arg("p_elem"),
        py::arg("seed_elem"));
  m.def("mfma_probe", &mfma_probe, "16x16x32 bf16 MFMA layout probe");
  m.def("mfma32_probe", &mfma32_probe, "32x32x16 bf16 MFMA layout probe");
  m.def("tr16_probe", &tr16_probe, "ds_read_b64_tr_b16 semantics probe");
  m.def("wgrad_gemm", &wgrad_gemm,
        "C = A^T B weight-gradient GEMM (bf16, tr16 transpose reads)");
  m.def("fwd_gemm", &fwd_gemm,
        "C = X W^T forward Linear GEMM (+fused bias), hand-written CDNA4 "
        "MFMA (csrc/fgemm.hip)",
        py::arg("x"), py::arg("w"), py::arg("bias") = py::none());
  m.def("fwd_gemm_gelu", &fwd_gemm_gelu,
        "(gelu(X W^T + bias), pre-activation) with the EXACT erf GELU "
        "fused into the hand-written forward GEMM epilogue",
        py::arg("x"), py::arg("w"), py::arg("bias"));
  m.def("lt_gemm", &lt_gemm,
        "row-major bf16 GEMM (+optional fused bias epilogue) via "
        "hipblaslt-ext with an explicit algorithm index (-1 = library "
        "heuristic); offline-search apply path, see "
        "csrc/tools/hipblaslt_search.cpp",
        py::arg("a"), py::arg("b"), py::arg("algo_index") = -1,
        py::arg("bias") = py::none());
  m.def("lt_gemm_gelu", &lt_gemm_gelu,
        "(gelu(a@b+bias), pre-activation aux) in one hipblaslt-ext GEMM "
        "(GELU_AUX epilogue; tanh-approx GELU)",
        py::arg("a"), py::arg("b"), py::arg("bias") = py::none(),
        py::arg("algo_index") = -1);
  m.def("lt_gemm_dgelu_bgrad", &lt_gemm_dgelu_bgrad,
        "(dgelu(dy@w, aux), column-sum bias grad) in one hipblaslt-ext "
        "GEMM (DGELU_BGRAD epilogue)",
        py::arg("dy"), py::arg("w"), py::arg("aux"),
        py::arg("algo_index") = -1);
  m.def("dgrad_tn", &dgrad_tn,
        "dx [tok, in] = dy [tok, out] @ w [out, in] as the library's TN "
        "GEMM on w^T, which csrc/transpose.hip writes into a scratch "
        "buffer on every call; row-contiguous bf16 operands, in and out "
        "multiples of 8, w 16-byte aligned",
        py::arg("dy"), py::arg("w"), py::arg("algo_index") = -1);
}
