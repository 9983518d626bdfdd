// Global L2 norm of the flat gradient buffer and the clipping coefficient, on the device.
//
//   norm = sqrt(Σ g²),  coef = min(1, max_norm / (norm + 1e-6))
// (torch.nn.utils.clip_grad_norm_, norm_type 2, error_if_nonfinite False: a NaN gradient gives
// NaN, NaN; an infinite one inf, 0.)
//
// grad_sumsq: one 256-thread workgroup per chunk of 16 384 floats writes part[chunk], the chunk's
//       Σ g² in fp64. An fp32 × fp32 product is exact in fp64, so the squares of 1e-30 and of 3e19
//       both survive. Every thread issues its 16 float4 loads before the first use; they are
//       non-temporal (the buffer is streamed once and is far larger than the Infinity Cache).
// grad_clip_finish: one workgroup folds the partial sums and writes out = (norm, coef) in fp32,
//       each rounded once from fp64.
// Both reduce by the same fixed tree — a lane sums its own values in index order, an fp64
// butterfly runs across the wave, the four waves combine in wave order — with no atomics and no
// grid-stride loop: the chunk of a value, and so the whole summation order, depends on its index
// alone, and the result is bitwise reproducible. The Adam kernels read out[1] from the device
// (adamw.hip, ``scale_dev``); the host never learns it.
#include "common.h"
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

namespace penroz {
namespace {

constexpr int kNormThreads = 256;
constexpr int kNormVecs = 16;                                  // float4 loads per thread
constexpr int64_t kNormChunk4 = (int64_t)kNormThreads * kNormVecs;  // float4 per chunk
constexpr int64_t kNormChunk = 4 * kNormChunk4;                // 16 384 floats

// Σ over the workgroup, valid in thread 0: butterfly across each wave, then the waves in order
__device__ __forceinline__ double block_sum(double s, double* red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

__device__ __forceinline__ double sq_acc(float4_t x, double s) {
#pragma unroll
  for (int k = 0; k < 4; ++k) s = fma((double)x[k], (double)x[k], s);
  return s;
}

__global__ void __launch_bounds__(kNormThreads) grad_sumsq_kernel(const float* __restrict__ g, int64_t n,
                                                                  double* __restrict__ part) {
  __shared__ double red[kNormThreads / 64];
  const int64_t n4 = n / 4;
  const int64_t base = (int64_t)blockIdx.x * kNormChunk4 + threadIdx.x;  // this thread's first float4
  const float4_t* g4 = reinterpret_cast<const float4_t*>(g);
  float4_t x[kNormVecs];
  if (((int64_t)blockIdx.x + 1) * kNormChunk4 <= n4) {  // a whole chunk (uniform over the workgroup)
#pragma unroll
    for (int j = 0; j < kNormVecs; ++j) x[j] = __builtin_nontemporal_load(g4 + base + (int64_t)j * kNormThreads);
  } else {  // the ragged last chunk: a vector past the end counts as zeros (s + 0·0 = s exactly)
#pragma unroll
    for (int j = 0; j < kNormVecs; ++j) {
      const int64_t q = base + (int64_t)j * kNormThreads;
      x[j] = q < n4 ? __builtin_nontemporal_load(g4 + q) : float4_t{0.f, 0.f, 0.f, 0.f};
    }
  }
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kNormVecs; ++j) s = sq_acc(x[j], s);
  // the n % 4 elements after the last whole vector lie in the last chunk
  if (blockIdx.x == gridDim.x - 1) {
    const int64_t i = 4 * n4 + threadIdx.x;
    if (i < n) {
      const double t = (double)g[i];
      s = fma(t, t, s);
    }
  }
  s = block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kNormThreads) grad_clip_finish_kernel(const double* __restrict__ part,
                                                                        int64_t chunks, double max_norm,
                                                                        float* __restrict__ out) {
  __shared__ double red[kNormThreads / 64];
  double s = 0.0;
  for (int64_t c = threadIdx.x; c < chunks; c += kNormThreads) s += part[c];
  s = block_sum(s, red);
  if (threadIdx.x == 0) {
    const double norm = sqrt(s);
    const double c = max_norm / (norm + 1e-6);
    out[0] = (float)norm;
    out[1] = (float)(c > 1.0 ? 1.0 : c);  // (a NaN stays a NaN, as torch's clamp keeps it)
  }
}

}  // namespace
}  // namespace penroz

using namespace penroz;

int64_t grad_sumsq_chunks(int64_t n) { return (n + kNormChunk - 1) / kNormChunk; }

// part[c] = Σ g² over chunk c, c < grad_sumsq_chunks(n); returns the number of chunks
int64_t grad_sumsq(torch::Tensor g, torch::Tensor part) {
  TORCH_CHECK(g.is_cuda() && g.scalar_type() == torch::kFloat32 && g.dim() == 1 && g.is_contiguous(),
              "grad_sumsq: the gradient must be a contiguous 1-d fp32 GPU tensor, got ", g.scalar_type(), " ", g.sizes());
  const int64_t n = g.numel();
  // the kernel reads the base as float4
  TORCH_CHECK(n == 0 || reinterpret_cast<uintptr_t>(g.data_ptr()) % 16 == 0, "grad_sumsq: the gradient must be 16-B aligned");
  const int64_t chunks = grad_sumsq_chunks(n);
  TORCH_CHECK(part.is_cuda() && part.device() == g.device() && part.scalar_type() == torch::kFloat64 &&
                  part.is_contiguous() && part.numel() >= chunks,
              "grad_sumsq: the workspace must be fp64 on the gradient's device with one element per chunk of 16384");
  TORCH_CHECK(chunks < ((int64_t)1 << 31), "grad_sumsq: too many chunks for one grid");
  if (chunks == 0) return 0;
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)chunks), dim3(kNormThreads), 0, at::hip::getCurrentHIPStream(),
                     g.data_ptr<float>(), n, part.data_ptr<double>());
  return chunks;
}

// out = (sqrt(Σ part[0 … chunks)), min(1, max_norm / (norm + 1e-6))), fp32 [2]
void grad_clip_finish(torch::Tensor part, int64_t chunks, double max_norm, torch::Tensor out) {
  TORCH_CHECK(part.is_cuda() && part.scalar_type() == torch::kFloat64 && part.is_contiguous() && chunks >= 0 &&
                  part.numel() >= chunks,
              "grad_clip_finish: the workspace must be fp64 with at least `chunks` elements");
  TORCH_CHECK(out.is_cuda() && out.device() == part.device() && out.scalar_type() == torch::kFloat32 &&
                  out.is_contiguous() && out.numel() == 2,
              "grad_clip_finish: out must be fp32 [2] on the workspace's device");
  hipLaunchKernelGGL(grad_clip_finish_kernel, dim3(1), dim3(kNormThreads), 0, at::hip::getCurrentHIPStream(),
                     part.data_ptr<double>(), chunks, max_norm, out.data_ptr<float>());
}
