// Gradient clipping by global norm, on the device (torch.nn.utils.clip_grad_norm_ semantics, norm_type 2; the reference reads
// `clip_grad_norm` at trainer/trainer.py:99 and logs `grad_norm` at trainer.py:532, 552-553).
//
//   squared-norm partials : every workgroup owns a fixed contiguous range of the input (a function of the sizes only),
//                           accumulates x * x in fp64 and writes ONE fp64 partial - no atomics, so the result is a pure
//                           function of the input bits (deterministic mode, identical on every data-parallel replica);
//   coefficient           : one workgroup folds the partials in a fixed order and leaves {total_norm, pre_scale * coef} in
//                           device memory, where the Adam kernels (csrc/embedding.hip) read their gradient scale.
#include "mhr_common.h"

#define GN_BLOCK 256
#define GN_CHUNK 8192            // fp32 elements one workgroup owns: 8 x 16-byte loads per thread

static inline int64_t gn_rows_per_wg(int dim) { return dim >= GN_CHUNK ? 1 : GN_CHUNK / dim; }

static inline int64_t gn_partials(int64_t n, int dim) {
  const int64_t per = gn_rows_per_wg(dim);
  const int64_t p = (n + per - 1) / per;
  return p < 1 ? 1 : p;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// fixed-order sum of one value per thread over the workgroup: butterfly inside each wave, then wave 0..3 in index order
__device__ __forceinline__ double block_sum_f64(double v, double* lds) {
  v = wave_sum_f64(v);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < GN_BLOCK / 64; ++w) s += lds[w];
  return s;
}

__device__ __forceinline__ void sq_acc4(const f32x4 x, double& a0, double& a1) {
  a0 = fma((double)x[0], (double)x[0], a0);
  a1 = fma((double)x[1], (double)x[1], a1);
  a0 = fma((double)x[2], (double)x[2], a0);
  a1 = fma((double)x[3], (double)x[3], a1);
}

__global__ __launch_bounds__(GN_BLOCK) void sqnorm_flat_kernel(const float* __restrict__ g, int64_t n,
                                                               double* __restrict__ partials) {
  __shared__ double lds[GN_BLOCK / 64];
  const int64_t begin = (int64_t)blockIdx.x * GN_CHUNK;
  const int64_t end = begin + GN_CHUNK < n ? begin + GN_CHUNK : n;
  double a0 = 0.0, a1 = 0.0;
  if (end - begin == GN_CHUNK) {                       // a whole chunk: 8 independent 16-byte loads in flight
    f32x4 x[GN_CHUNK / (4 * GN_BLOCK)];
#pragma unroll
    for (int k = 0; k < GN_CHUNK / (4 * GN_BLOCK); ++k)
      x[k] = *reinterpret_cast<const f32x4*>(g + begin + ((int64_t)k * GN_BLOCK + threadIdx.x) * 4);
#pragma unroll
    for (int k = 0; k < GN_CHUNK / (4 * GN_BLOCK); ++k) sq_acc4(x[k], a0, a1);
  } else {                                             // the last chunk: whole vectors, then the tail element by element
    const int64_t n4 = begin < end ? (end - begin) / 4 : 0;
    for (int64_t i = threadIdx.x; i < n4; i += GN_BLOCK) sq_acc4(*reinterpret_cast<const f32x4*>(g + begin + i * 4), a0, a1);
    for (int64_t i = begin + n4 * 4 + threadIdx.x; i < end; i += GN_BLOCK) a0 = fma((double)g[i], (double)g[i], a0);
  }
  const double s = block_sum_f64(a0 + a1, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// rows [n_ids, dim] of a sparse row gradient: a row counts where sorted_ids[i] starts a segment and lies in [0, n_rows) -
// the rows mhr_adam_rows / mhr_adam_rows_lazy apply.  Whatever the other rows hold is never read.
__global__ __launch_bounds__(GN_BLOCK) void sqnorm_rows_kernel(const float* __restrict__ rows, const int64_t* __restrict__ sorted_ids,
                                                               int64_t n_ids, int dim, int64_t n_rows, int64_t rows_per_wg,
                                                               double* __restrict__ partials) {
  __shared__ double lds[GN_BLOCK / 64];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t begin = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t end = begin + rows_per_wg < n_ids ? begin + rows_per_wg : n_ids;
  double a0 = 0.0, a1 = 0.0;
  for (int64_t i = begin + wave; i < end; i += GN_BLOCK / 64) {
    const int64_t id = sorted_ids[i];
    if (id < 0 || id >= n_rows) continue;
    if (i > 0 && sorted_ids[i - 1] == id) continue;                     // not the head of its segment
    const float* r = rows + i * dim;
    for (int c = lane * 4; c < dim; c += 256) sq_acc4(*reinterpret_cast<const f32x4*>(r + c), a0, a1);
  }
  const double s = block_sum_f64(a0 + a1, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(GN_BLOCK) void clip_coef_kernel(const double* __restrict__ partials, int64_t n_partials,
                                                             float pre_scale, float max_norm, float* __restrict__ out2) {
  __shared__ double lds[GN_BLOCK / 64];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < n_partials; i += GN_BLOCK) a += partials[i];
  const double sum = block_sum_f64(a, lds);
  if (threadIdx.x == 0) {
    // torch: clip_coef = max_norm / (total_norm + 1e-6) clamped to 1 from above (a NaN stays a NaN); formed in fp64 here and
    // rounded to fp32 once
    const double total = sqrt(sum) * (double)pre_scale;
    double coef = (double)max_norm / (total + 1e-6);
    if (coef > 1.0) coef = 1.0;
    out2[0] = (float)total;
    out2[1] = (float)((double)pre_scale * coef);
  }
}

extern "C" int64_t mhr_grad_sqnorm_partials(int64_t n, int dim) {
  if (n < 0 || dim < 1) return -1;
  return gn_partials(n, dim);
}

extern "C" int mhr_grad_sqnorm_flat(const float* g, int64_t n, double* partials, int64_t partials_off, void* stream) {
  MHR_REQUIRE(partials && (g || n == 0), "grad_sqnorm_flat: null pointer");
  MHR_REQUIRE(n >= 0 && partials_off >= 0, "grad_sqnorm_flat: bad sizes (n=%lld off=%lld)", (long long)n, (long long)partials_off);
  MHR_REQUIRE((uintptr_t)g % 16 == 0 && (uintptr_t)partials % 8 == 0, "grad_sqnorm_flat: g must be 16-byte aligned");
  const int64_t grid = gn_partials(n, 1);
  MHR_REQUIRE(grid <= 0x7FFFFFFF, "grad_sqnorm_flat: n=%lld needs more workgroups than one launch has", (long long)n);
  hipLaunchKernelGGL(sqnorm_flat_kernel, dim3((unsigned)grid), dim3(GN_BLOCK), 0, (hipStream_t)stream, g, n,
                     partials + partials_off);
  MHR_CHECK_LAUNCH("grad_sqnorm_flat");
  return MHR_OK;
}

extern "C" int mhr_grad_sqnorm_rows(const float* rows, const int64_t* sorted_ids, int64_t n_ids, int dim, int64_t n_rows,
                                    double* partials, int64_t partials_off, void* stream) {
  MHR_REQUIRE(partials && ((rows && sorted_ids) || n_ids == 0), "grad_sqnorm_rows: null pointer");
  MHR_REQUIRE(dim > 0 && dim % 4 == 0, "grad_sqnorm_rows: dim=%d must be a positive multiple of 4", dim);
  MHR_REQUIRE(n_ids >= 0 && n_rows >= 0 && partials_off >= 0, "grad_sqnorm_rows: bad sizes (n_ids=%lld n_rows=%lld off=%lld)",
              (long long)n_ids, (long long)n_rows, (long long)partials_off);
  MHR_REQUIRE((uintptr_t)rows % 16 == 0 && (uintptr_t)partials % 8 == 0, "grad_sqnorm_rows: rows must be 16-byte aligned");
  const int64_t grid = gn_partials(n_ids, dim);
  MHR_REQUIRE(grid <= 0x7FFFFFFF, "grad_sqnorm_rows: n_ids=%lld needs more workgroups than one launch has", (long long)n_ids);
  hipLaunchKernelGGL(sqnorm_rows_kernel, dim3((unsigned)grid), dim3(GN_BLOCK), 0, (hipStream_t)stream, rows, sorted_ids, n_ids,
                     dim, n_rows, gn_rows_per_wg(dim), partials + partials_off);
  MHR_CHECK_LAUNCH("grad_sqnorm_rows");
  return MHR_OK;
}

extern "C" int mhr_grad_clip_coef(const double* partials, int64_t n_partials, float pre_scale, float max_norm, float* out2,
                                  void* stream) {
  MHR_REQUIRE(partials && out2, "grad_clip_coef: null pointer");
  MHR_REQUIRE(n_partials >= 0, "grad_clip_coef: bad sizes (n_partials=%lld)", (long long)n_partials);
  MHR_REQUIRE(max_norm > 0.0f && pre_scale > 0.0f, "grad_clip_coef: max_norm=%g and pre_scale=%g must be positive",
              (double)max_norm, (double)pre_scale);
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(GN_BLOCK), 0, (hipStream_t)stream, partials, n_partials, pre_scale,
                     max_norm, out2);
  MHR_CHECK_LAUNCH("grad_clip_coef");
  return MHR_OK;
}
