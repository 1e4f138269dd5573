// Catalog exposure from a device item histogram (reference evaluator/metrics.py: ItemCoverage 473-516, AveragePopularity 519-585,
// ShannonEntropy 588-640, GiniIndex 643-696, TailPercentage 699-780).  All five are functions of c_k[i] = how many users have
// item i among their first k merged recommendations, so the evaluation keeps one integer histogram instead of the reference's
// [users, max(topk)] item matrix.
//
//   accumulate      : one thread per (user, rank); the rank's BAND is the first cut-off above it, and the thread adds 1 to
//                     band_counts[band][item] with an integer atomic.  c at cut-off t is the sum of the bands <= t.  Integer adds
//                     commute: the histogram is bit-identical whatever the batch split or the launch order.
//   finalize partial: 1024 items per workgroup; per cut-off the workgroup reduces (R, sum c*phi, sum c*tail, S = sum c ln c) in
//                     a fixed order into ONE partial per cell and counts its items into the count-of-counts table m[t][c]
//                     (integer atomics: counts below 64 into a table in LDS that is flushed once, the rest straight to memory).
//   finalize fold   : one workgroup per cut-off adds the partials in workgroup order and scans m[t][.] for the Gini numerator
//                     G = sum_c c m_c (N - 2R + 2 s_c + m_c), s_c = items of non-zero count below c - an exact integer.
// No floating-point atomics: S is an fp64 sum in an order fixed by the item ids alone, the same histogram gives the same bits.
#include "mhr_common.h"

#define EX_MAX_CUTS 16
#define EX_THREADS 256
#define EX_ITEMS_PER_THREAD 4
#define EX_BLOCK_ITEMS (EX_THREADS * EX_ITEMS_PER_THREAD)
#define EX_WAVES (EX_THREADS / 64)
#define EX_CELLS 4                // R, sum c*phi, sum c*tail (int64) and S (double): 8-byte words per (workgroup, cut-off)
#define EX_SMALL 64               // counts below this are tallied per workgroup in LDS first: nearly every item has a small count,
                                  // and one global atomic per (item, cut-off) onto those few words took 2.7 ms at 454 k items

struct ExCuts {                   // the host's cut-offs, ascending, passed by value
  int cut[EX_MAX_CUTS];
};

__global__ __launch_bounds__(EX_THREADS) void exposure_accumulate_kernel(const int64_t* __restrict__ topk_idx, int64_t total,
                                                                         int K, ExCuts cuts, int n_cuts, int64_t n_items,
                                                                         int32_t* __restrict__ band_counts,
                                                                         int32_t* __restrict__ bad) {
  const int64_t e = (int64_t)blockIdx.x * EX_THREADS + threadIdx.x;          // element b * K + j of the [B, K] list matrix
  if (e >= total) return;
  const int j = (int)(e % K);
  if (j >= cuts.cut[n_cuts - 1]) return;                                     // ranks at or beyond the last cut-off
  int t = 0;
#pragma unroll
  for (int s = 0; s < EX_MAX_CUTS - 1; ++s) t += (s < n_cuts - 1 && j >= cuts.cut[s]) ? 1 : 0;   // ascending: first cut above j
  const int64_t id = topk_idx[e];
  if (id < 0 || id >= n_items) {
    atomicAdd(bad, 1);
    return;
  }
  atomicAdd(band_counts + (int64_t)t * n_items + id, 1);
}

// 64 lanes -> lane 0, the same tree on every call
__device__ __forceinline__ long long ex_wave_sum(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}
__device__ __forceinline__ double ex_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// partials [n_wg, n_cuts, EX_CELLS] 8-byte words; count_of_counts [n_cuts, max_count + 1] (zeroed by the caller)
__global__ __launch_bounds__(EX_THREADS) void exposure_partial_kernel(const int32_t* __restrict__ band_counts, int n_cuts,
                                                                      int64_t n_items, const int64_t* __restrict__ item_pop,
                                                                      const uint8_t* __restrict__ item_tail, int max_count,
                                                                      long long* __restrict__ partials,
                                                                      int32_t* __restrict__ count_of_counts,
                                                                      int32_t* __restrict__ bad) {
  __shared__ long long lds_i[EX_MAX_CUTS][3][EX_WAVES];
  __shared__ double lds_s[EX_MAX_CUTS][EX_WAVES];
  __shared__ int lds_m[EX_MAX_CUTS][EX_SMALL];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int q = tid; q < n_cuts * EX_SMALL; q += EX_THREADS) lds_m[q / EX_SMALL][q % EX_SMALL] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * EX_BLOCK_ITEMS;
  long long c[EX_ITEMS_PER_THREAD], pop[EX_ITEMS_PER_THREAD], tail[EX_ITEMS_PER_THREAD];
#pragma unroll
  for (int u = 0; u < EX_ITEMS_PER_THREAD; ++u) {
    const int64_t i = base + u * EX_THREADS + tid;
    c[u] = 0;
    pop[u] = (item_pop && i < n_items) ? (long long)item_pop[i] : 0;
    tail[u] = (item_tail && i < n_items) ? (item_tail[i] != 0) : 0;
  }
  for (int t = 0; t < n_cuts; ++t) {
    long long r = 0, sp = 0, st = 0;
    double s = 0.0;
#pragma unroll
    for (int u = 0; u < EX_ITEMS_PER_THREAD; ++u) {
      const int64_t i = base + u * EX_THREADS + tid;
      if (i < n_items) c[u] += band_counts[(int64_t)t * n_items + i];
      if (c[u] > 0) {
        r += 1;
        sp += c[u] * pop[u];
        st += c[u] * tail[u];
        s += (double)c[u] * log((double)c[u]);
        if (c[u] > max_count) atomicAdd(bad, 1);            // more occurrences than users: outside the table, never written
        else if (c[u] < EX_SMALL) atomicAdd(&lds_m[t][c[u]], 1);
        else atomicAdd(count_of_counts + (int64_t)t * ((int64_t)max_count + 1) + c[u], 1);
      }
    }
    r = ex_wave_sum(r);
    sp = ex_wave_sum(sp);
    st = ex_wave_sum(st);
    s = ex_wave_sum(s);
    if (lane == 0) {
      lds_i[t][0][wave] = r;
      lds_i[t][1][wave] = sp;
      lds_i[t][2][wave] = st;
      lds_s[t][wave] = s;
    }
  }
  __syncthreads();
  if (tid < n_cuts) {
    long long* out = partials + ((int64_t)blockIdx.x * n_cuts + tid) * EX_CELLS;
    double s = 0.0;
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      long long a = 0;
#pragma unroll
      for (int w = 0; w < EX_WAVES; ++w) a += lds_i[tid][v][w];
      out[v] = a;
    }
#pragma unroll
    for (int w = 0; w < EX_WAVES; ++w) s += lds_s[tid][w];
    reinterpret_cast<double*>(out)[3] = s;
  }
  for (int q = tid; q < n_cuts * EX_SMALL; q += EX_THREADS) {          // only counts <= max_count were tallied: inside the table
    const int t = q / EX_SMALL, cnt = q % EX_SMALL, n = lds_m[t][cnt];
    if (n > 0) atomicAdd(count_of_counts + (int64_t)t * ((int64_t)max_count + 1) + cnt, n);
  }
}

// One workgroup per cut-off.  Thread q scans counts [1 + q * chunk, 1 + (q + 1) * chunk): its items M, its count mass
// W = sum c m_c and its share A = sum c m_c (N - 2R + m_c + 2 (items below c inside the chunk)); thread 0 then walks the chunks
// in order, G = sum_q A_q + 2 W_q (items in the chunks before q).
__global__ __launch_bounds__(EX_THREADS) void exposure_fold_kernel(const long long* __restrict__ partials, int64_t n_wg,
                                                                   int n_cuts, int64_t n_items, int max_count,
                                                                   const int32_t* __restrict__ count_of_counts,
                                                                   long long* __restrict__ out_int, double* __restrict__ out_f64) {
  __shared__ long long cell[3];
  __shared__ long long ch_m[EX_THREADS], ch_w[EX_THREADS], ch_a[EX_THREADS];
  const int t = blockIdx.x, tid = threadIdx.x;
  if (tid < 3) {
    long long a = 0;
#pragma unroll 8
    for (int64_t w = 0; w < n_wg; ++w) a += partials[(w * n_cuts + t) * EX_CELLS + tid];
    cell[tid] = a;
  } else if (tid == 3) {
    double s = 0.0;
#pragma unroll 8
    for (int64_t w = 0; w < n_wg; ++w) s += reinterpret_cast<const double*>(partials)[(w * n_cuts + t) * EX_CELLS + 3];
    out_f64[t] = s;
  }
  __syncthreads();
  const long long R = cell[0];
  const int64_t chunk = ((int64_t)max_count + EX_THREADS - 1) / EX_THREADS;
  const int64_t lo = 1 + (int64_t)tid * chunk;
  const int64_t hi = lo + chunk < (int64_t)max_count + 1 ? lo + chunk : (int64_t)max_count + 1;
  const int32_t* m = count_of_counts + (int64_t)t * ((int64_t)max_count + 1);
  long long M = 0, W = 0, A = 0;
  for (int64_t cnt = lo; cnt < hi; ++cnt) {
    const long long mc = m[cnt];
    A += cnt * mc * ((long long)n_items - 2 * R + mc + 2 * M);
    W += cnt * mc;
    M += mc;
  }
  ch_m[tid] = M;
  ch_w[tid] = W;
  ch_a[tid] = A;
  __syncthreads();
  if (tid == 0) {
    long long G = 0, before = 0;
    for (int q = 0; q < EX_THREADS; ++q) {
      G += ch_a[q] + 2 * ch_w[q] * before;
      before += ch_m[q];
    }
    out_int[t * 4 + 0] = R;
    out_int[t * 4 + 1] = cell[1];
    out_int[t * 4 + 2] = cell[2];
    out_int[t * 4 + 3] = G;
  }
}

static inline int64_t ex_n_wg(int64_t n_items) { return (n_items + EX_BLOCK_ITEMS - 1) / EX_BLOCK_ITEMS; }

extern "C" int mhr_exposure_accumulate(const int64_t* topk_idx, int B, int K, const int32_t* cuts, int n_cuts, int64_t n_items,
                                       int32_t* band_counts, int32_t* bad, void* stream) {
  MHR_REQUIRE(topk_idx, "exposure_accumulate: topk_idx is null");
  MHR_REQUIRE(cuts, "exposure_accumulate: cuts (host array) is null");
  MHR_REQUIRE(band_counts && bad, "exposure_accumulate: band_counts / bad is null");
  MHR_REQUIRE(B >= 0, "exposure_accumulate: B=%d is negative", B);
  MHR_REQUIRE(K >= 1, "exposure_accumulate: K=%d is below 1", K);
  MHR_REQUIRE(n_cuts >= 1 && n_cuts <= EX_MAX_CUTS, "exposure_accumulate: n_cuts=%d outside [1, %d]", n_cuts, EX_MAX_CUTS);
  MHR_REQUIRE(n_items >= 1 && n_items < (1ll << 31), "exposure_accumulate: n_items=%lld outside [1, 2^31)", (long long)n_items);
  ExCuts c;
  for (int t = 0; t < EX_MAX_CUTS; ++t) c.cut[t] = 0;
  for (int t = 0; t < n_cuts; ++t) {
    MHR_REQUIRE(cuts[t] >= 1 && (t == 0 || cuts[t] > cuts[t - 1]), "exposure_accumulate: cuts[%d]=%d is not ascending from 1", t,
                cuts[t]);
    c.cut[t] = cuts[t];
  }
  MHR_REQUIRE(cuts[n_cuts - 1] <= K, "exposure_accumulate: cuts[%d]=%d exceeds K=%d", n_cuts - 1, cuts[n_cuts - 1], K);
  if (B == 0) return MHR_OK;
  const int64_t total = (int64_t)B * K;
  MHR_REQUIRE((total + EX_THREADS - 1) / EX_THREADS < (1ll << 31), "exposure_accumulate: B * K = %lld is too large for one launch",
              (long long)total);
  hipLaunchKernelGGL(exposure_accumulate_kernel, dim3((unsigned)((total + EX_THREADS - 1) / EX_THREADS)), dim3(EX_THREADS), 0,
                     (hipStream_t)stream, topk_idx, total, K, c, n_cuts, n_items, band_counts, bad);
  MHR_CHECK_LAUNCH("exposure_accumulate");
  return MHR_OK;
}

extern "C" int64_t mhr_exposure_finalize_workspace_bytes(int n_cuts, int64_t n_items, int64_t max_count) {
  if (n_cuts < 1 || n_cuts > EX_MAX_CUTS || n_items < 1 || n_items >= (1ll << 31) || max_count < 0 || max_count >= (1ll << 31))
    return -1;
  const int64_t table = ((int64_t)n_cuts * (max_count + 1) * 4 + 7) / 8 * 8;
  return ex_n_wg(n_items) * n_cuts * EX_CELLS * 8 + table;
}

extern "C" int mhr_exposure_finalize(const int32_t* band_counts, int n_cuts, int64_t n_items, const int64_t* item_pop,
                                     const uint8_t* item_tail, int64_t max_count, int k_max, int64_t* out_int, double* out_f64,
                                     int32_t* bad, void* workspace, void* stream) {
  MHR_REQUIRE(band_counts, "exposure_finalize: band_counts is null");
  MHR_REQUIRE(out_int && out_f64 && bad && workspace, "exposure_finalize: out_int / out_f64 / bad / workspace is null");
  MHR_REQUIRE(n_cuts >= 1 && n_cuts <= EX_MAX_CUTS, "exposure_finalize: n_cuts=%d outside [1, %d]", n_cuts, EX_MAX_CUTS);
  MHR_REQUIRE(n_items >= 1 && n_items < (1ll << 31), "exposure_finalize: n_items=%lld outside [1, 2^31)", (long long)n_items);
  MHR_REQUIRE(max_count >= 0 && max_count < (1ll << 31), "exposure_finalize: max_count=%lld (users) outside [0, 2^31)",
              (long long)max_count);
  MHR_REQUIRE(k_max >= 1, "exposure_finalize: k_max=%d is below 1", k_max);
  // |G| <= N * U * k and the scan forms 2 * (items) * (count mass) on the way: 2 N U k must fit
  MHR_REQUIRE((__int128)2 * n_items * max_count * k_max < ((__int128)1 << 63),
              "exposure_finalize: 2 * n_items * users * k_max = 2 * %lld * %lld * %d does not fit 63 bits (the Gini numerator)",
              (long long)n_items, (long long)max_count, k_max);
  MHR_REQUIRE((uintptr_t)out_int % 8 == 0 && (uintptr_t)out_f64 % 8 == 0 && (uintptr_t)workspace % 8 == 0 &&
                  (!item_pop || (uintptr_t)item_pop % 8 == 0),
              "exposure_finalize: out_int / out_f64 / workspace / item_pop must be 8-byte aligned");
  const int64_t n_wg = ex_n_wg(n_items);
  long long* partials = (long long*)workspace;
  int32_t* table = (int32_t*)(partials + n_wg * n_cuts * EX_CELLS);
  const hipError_t e = hipMemsetAsync(table, 0, (size_t)n_cuts * (size_t)(max_count + 1) * 4, (hipStream_t)stream);
  if (e != hipSuccess) {
    mhr_set_error("exposure_finalize: clearing the count-of-counts table failed: %s", hipGetErrorString(e));
    return MHR_ELAUNCH;
  }
  hipLaunchKernelGGL(exposure_partial_kernel, dim3((unsigned)n_wg), dim3(EX_THREADS), 0, (hipStream_t)stream, band_counts, n_cuts,
                     n_items, item_pop, item_tail, (int)max_count, partials, table, bad);
  MHR_CHECK_LAUNCH("exposure_finalize (partials)");
  hipLaunchKernelGGL(exposure_fold_kernel, dim3((unsigned)n_cuts), dim3(EX_THREADS), 0, (hipStream_t)stream,
                     (const long long*)partials, n_wg, n_cuts, n_items, (int)max_count, (const int32_t*)table,
                     (long long*)out_int, out_f64);
  MHR_CHECK_LAUNCH("exposure_finalize (fold)");
  return MHR_OK;
}
