// Operand checks of the decode-step launch wrappers (decode_linear.hip, skinny_gemm.hip,
// decode_gemv_q8.hip, decode_attn.hip, sampling.hip, logit_penalty.hip, logit_bias.hip, token_logprobs.hip, stop_check.hip, spec_decode.hip), written once. Each checks one operand and
// returns its typed pointer; `who` is the entry point's name for the message. Where the entry
// points differ, the difference is a parameter. Also the wrappers' dtype -> element type dispatch
// and their read of an integer environment switch. Host only.
#pragma once
#include "common.h"
#include "host_plan.h"
#include <cstdlib>
#include <initializer_list>
#include <torch/extension.h>

namespace penroz {

using OptTensor = c10::optional<torch::Tensor>;

inline bool la_defined(const OptTensor& t) { return t.has_value() && t->defined(); }
inline bool la_aligned(const torch::Tensor& t, int bytes) { return reinterpret_cast<uintptr_t>(t.data_ptr()) % bytes == 0; }

inline int la_env_int(const char* name, int unset) {
  const char* e = std::getenv(name);
  return e ? std::atoi(e) : unset;
}

// f(T{}) with T = bf16 / float / __half for the dtype; elem_of<T>() names T for host_plan.h
template <class T>
constexpr Elem elem_of() {
  return std::is_same<T, bf16>::value ? Elem::BF16 : std::is_same<T, float>::value ? Elem::F32 : Elem::F16;
}
template <class F>
void la_by_elem(const char* who, at::ScalarType dtype, F&& f) {
  if (dtype == torch::kBFloat16) f(bf16{});
  else if (dtype == torch::kFloat32) f(float{});
  else if (dtype == torch::kFloat16) f(__half{});
  else TORCH_CHECK(false, who, ": bf16, fp32 or fp16 expected, got ", dtype);
}

// `first` is on the GPU and every other operand given is on its device: no host pointer reaches a kernel
inline void la_one_device(const char* who, const torch::Tensor& first, std::initializer_list<OptTensor> rest) {
  for (const OptTensor& t : rest)
    TORCH_CHECK(first.is_cuda() && (!la_defined(t) || t->device() == first.device()), who,
                ": every operand must be on one GPU, the first operand's");
}

// int64 [1] scalar the kernel reads or bumps (cache position / length, step, seed)
inline int64_t* la_i64_scalar(const char* who, const char* what, const torch::Tensor& t) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == torch::kInt64 && t.numel() == 1, who, ": ", what,
              " must be a device int64 [1]");
  return t.data_ptr<int64_t>();
}

// int64 [1] or contiguous [rows]: one value for every row, or each row's own (a ragged decode step's
// positions and cache lengths). The kernel reads entry row · stride; the stride is 0 or 1.
struct I64Rows {
  int64_t* p = nullptr;
  int stride = 0;
};

inline I64Rows la_i64_rows(const char* who, const char* what, const torch::Tensor& t, int64_t rows) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == torch::kInt64 && t.is_contiguous() &&
                  (t.numel() == 1 || (t.dim() == 1 && t.numel() == rows)),
              who, ": ", what, " must be a device int64 [1] or contiguous [rows = ", rows, "]");
  return {t.data_ptr<int64_t>(), t.dim() == 1 && t.numel() == rows && rows > 1 ? 1 : 0};
}

// int32 contiguous tensor of exactly this shape (the stop check's sequences and per-row state)
inline int* la_i32_shape(const char* who, const char* what, const torch::Tensor& t, at::IntArrayRef shape) {
  TORCH_CHECK(t.defined() && t.is_cuda() && t.scalar_type() == torch::kInt32 && t.is_contiguous() && t.sizes() == shape,
              who, ": int32 contiguous ", what, " ", shape);
  return t.data_ptr<int>();
}

// fp32 contiguous tensor of exactly this shape (the int8 cache's per-token scales)
inline float* la_f32_shape(const char* who, const char* what, const OptTensor& t, at::IntArrayRef shape) {
  TORCH_CHECK(la_defined(t) && t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() &&
                  t->sizes() == shape, who, ": fp32 contiguous ", what, " ", shape);
  return t->data_ptr<float>();
}

// bf16 activation rows x [M, K]: unit column stride, rows 16-B aligned (16-B vector loads)
inline const bf16* la_rows(const char* who, const torch::Tensor& x, int K) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16 && x.dim() == 2 && x.size(1) == K &&
                  x.stride(1) == 1 && x.stride(0) % 8 == 0 && la_aligned(x, 16),
              who, ": bf16 x [M, K = ", K, "], unit column stride, rows 16-B aligned");
  return reinterpret_cast<const bf16*>(x.data_ptr());
}

// bf16 weight [N, K], contiguous and 16-B aligned; N a multiple of n_mult (16 for the MFMA tiles
// of decode_linear.hip, 2 for the packed [gate; up] and paired-row forms)
inline const bf16* la_weight(const char* who, const torch::Tensor& w, int n_mult = 1) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == torch::kBFloat16 && w.dim() == 2 && w.is_contiguous() &&
                  la_aligned(w, 16) && w.size(0) % n_mult == 0,
              who, ": bf16 contiguous 16-B aligned W [N, K], N % ", n_mult, " == 0");
  return reinterpret_cast<const bf16*>(w.data_ptr());
}

// int8 weight rows [N, K] + one fp32 scale per row [N] (weight-only quantisation, decode_gemv_q8.hip):
// contiguous, rows 16-B aligned (K % 16 == 0: a 16-B chunk is 16 weights), N a multiple of n_mult
struct Q8Weight {
  const int8_t* q = nullptr;
  const float* scale = nullptr;
  int N = 0, K = 0;
};

inline Q8Weight la_weight_q8(const char* who, const torch::Tensor& q, const torch::Tensor& scale, int n_mult = 1) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kInt8 && q.dim() == 2 && q.is_contiguous() && la_aligned(q, 16) &&
                  q.size(0) >= 1 && q.size(1) >= 16 && q.size(1) % 16 == 0 && q.size(0) % n_mult == 0,
              who, ": int8 contiguous 16-B aligned W [N, K], K % 16 == 0, N % ", n_mult, " == 0");
  TORCH_CHECK(scale.is_cuda() && scale.device() == q.device() && scale.scalar_type() == torch::kFloat32 &&
                  scale.is_contiguous() && scale.numel() == q.size(0),
              who, ": fp32 contiguous row scales [N = ", q.size(0), "] on W's device");
  return {q.data_ptr<int8_t>(), scale.data_ptr<float>(), (int)q.size(0), (int)q.size(1)};
}

// optional bf16 bias [N] (nullptr when absent); decode_linear.hip's MFMA epilogues read it in 8-B pieces
inline const bf16* la_bias(const char* who, const OptTensor& bias, int N, int align = 2) {
  if (!la_defined(bias)) return nullptr;
  TORCH_CHECK(bias->is_cuda() && bias->scalar_type() == torch::kBFloat16 && bias->is_contiguous() &&
                  bias->numel() == N && la_aligned(*bias, align),
              who, ": bf16 contiguous bias [N = ", N, "], ", align, "-B aligned");
  return reinterpret_cast<const bf16*>(bias->data_ptr());
}

// fp32 contiguous vector of n entries (gamma, beta, dbias, cos, sin), or of at least n
inline const float* la_f32_vec(const char* who, const char* what, const OptTensor& t, int64_t n, bool at_least = false) {
  TORCH_CHECK(la_defined(t) && t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->is_contiguous() &&
                  (at_least ? t->numel() >= n : t->numel() == n),
              who, ": fp32 contiguous ", what, " [", n, "]");
  return t->data_ptr<float>();
}

// fp32 contiguous matrix [rows, cols] of the residual stream (rows < 0: any)
inline float* la_f32_mat(const char* who, const char* what, const OptTensor& t, int64_t rows, int64_t cols) {
  TORCH_CHECK(la_defined(t) && t->is_cuda() && t->scalar_type() == torch::kFloat32 && t->dim() == 2 &&
                  t->is_contiguous() && (rows < 0 || t->size(0) == rows) && t->size(1) == cols,
              who, ": fp32 contiguous ", what, " [M, ", cols, "]");
  return t->data_ptr<float>();
}

// bf16 output [M, N] with unit column stride; align 8: rows 8-B aligned as well (4-value stores)
inline bf16* la_out(const char* who, const torch::Tensor& out, int M, int N, int align = 2) {
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == torch::kBFloat16 && out.dim() == 2 && out.size(0) == M &&
                  out.size(1) == N && out.stride(1) == 1 && (align < 8 || out.stride(0) % 4 == 0) && la_aligned(out, align),
              who, ": bf16 out [", M, ", ", N, "], unit column stride, rows ", align, "-B aligned");
  return reinterpret_cast<bf16*>(out.data_ptr());
}

// The fused residual add in front of a LayerNorm: x = resid_in + delta + dbias, resid_out receives
// the sum. A delta needs a resid_out that does not alias resid_in; dbias comes only with a delta.
// lone_ignored (decode_gemv): without a delta, dbias and resid_out are not looked at. Otherwise
// (decode_ln_linear) a lone dbias is an error and a lone resid_out is checked and written.
struct ResidArgs {
  const float* rin = nullptr;
  const bf16* delta = nullptr;
  const float* dbias = nullptr;
  float* rout = nullptr;
  int M = 0;
};

inline ResidArgs la_resid(const char* who, const OptTensor& rin, const OptTensor& delta, const OptTensor& dbias,
                          const OptTensor& rout, int K, bool lone_ignored) {
  ResidArgs r;
  r.rin = la_f32_mat(who, "resid_in", rin, -1, K);
  r.M = rin->size(0);
  const bool add = la_defined(delta);
  if (add) {
    TORCH_CHECK(delta->is_cuda() && delta->scalar_type() == torch::kBFloat16 && delta->is_contiguous() &&
                    delta->numel() == (int64_t)r.M * K,
                who, ": bf16 contiguous delta [M, K]");
    r.delta = reinterpret_cast<const bf16*>(delta->data_ptr());
    TORCH_CHECK(la_defined(rout), who, ": a residual add (delta) needs resid_out");
  }
  if (!add && lone_ignored) return r;
  if (la_defined(dbias)) {
    TORCH_CHECK(add, who, ": dbias only with a delta");
    r.dbias = la_f32_vec(who, "dbias", dbias, K);
  }
  if (la_defined(rout)) {
    TORCH_CHECK(rout->is_cuda() && rout->scalar_type() == torch::kFloat32 && rout->is_contiguous() &&
                    rout->numel() == (int64_t)r.M * K && rout->data_ptr() != rin->data_ptr(),
                who, ": fp32 contiguous resid_out [M, K], not aliasing resid_in");
    r.rout = rout->data_ptr<float>();
  }
  return r;
}

}  // namespace penroz
