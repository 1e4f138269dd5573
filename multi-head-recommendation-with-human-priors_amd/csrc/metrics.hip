// Streaming evaluation metrics: one launch per batch turns (merged top-k ids, positives, group bits, item tag bits) into running
// fp64 sums of the per-user metric curves at the configured cut-offs, so an evaluation holds nothing that grows with its users
// (reference evaluator/metrics.py: Recall 179-181, NDCG 221-238, Hit 67-69, MRR 93-101, MAP 131-142, Precision 262-263,
// Entropy 29-41; the trainer all-reduces exactly these sums, trainer.py:1109-1123).
//
//   partial kernel : one user per lane, one wave per workgroup, one workgroup per (64 users, pred_len).  A lane walks its user's
//                    list in rank order (running hit count, DCG, AP sum, first hit rank - the order np.cumsum adds in) and
//                    leaves its six values per cut-off in LDS; the wave then adds the 64 users of every (group, metric,
//                    cut-off) cell in user order and writes ONE partial per cell into the workspace.  Entropy has a workgroup
//                    of its own per 64 users: per-tag counts live in bit-sliced counters (12 planes of 32 tags), so no
//                    per-lane array is indexed dynamically.
//   fold kernel    : one thread per cell adds the partials in workgroup order and then onto the accumulator.
// No floating-point atomics anywhere: the same launch sequence on the same inputs gives bit-identical accumulators.
#include "mhr_common.h"

#define MS_WAVE 64
#define MS_MAX_K 2048
#define MS_MAX_PRED 16
#define MS_MAX_TOPK 16
#define MS_MAX_GROUPS 32
#define MS_MAX_TAGS 32
#define MS_COLS 6                 // recall, ndcg, hit, mrr, map, precision
#define MS_PLANES 12              // a per-tag count <= 2048 needs 12 bits
#define MS_CHUNK 8                // ranks a lane loads at once: eight independent loads in flight, not one per loop trip
#define MS_POS_REGS 8             // positives a lane keeps in registers (longer target lists read the rest from memory)

struct MsLists {                  // the host's pred_len values and cut-offs, passed by value
  int pred[MS_MAX_PRED];
  int topk[MS_MAX_TOPK];
};

__host__ __device__ static inline int64_t ms_cells(int n_pred, int n_groups, int n_topk) {     // 8-byte words one workgroup writes
  return (int64_t)n_pred * n_groups * MS_COLS * n_topk + n_topk + (int64_t)n_pred * n_groups;
}
__host__ __device__ static inline int ms_row_stride(int n_topk) { return (MS_COLS * n_topk) | 1; }   // odd: a lane's row starts on its own bank pair

// ranks [j0, j0 + MS_CHUNK) of a user's list (-1 past k_scan): independent loads, all in flight at once
__device__ __forceinline__ void ms_load_chunk(const int64_t* __restrict__ row, int j0, int k_scan, int64_t (&it)[MS_CHUNK]) {
#pragma unroll
  for (int u = 0; u < MS_CHUNK; ++u) it[u] = j0 + u < k_scan ? row[j0 + u] : -1;
}

// bit u = rank j0 + u is a cut-off (tk: the cut-offs in registers, 0 in unused slots).  Uniform: scalar work once per chunk, so
// the scan itself looks at the cut-off list only at the few ranks that are one.
__device__ __forceinline__ uint32_t ms_cut_mask(const int (&tk)[MS_MAX_TOPK], int j0) {
  uint32_t m = 0u;
#pragma unroll
  for (int t = 0; t < MS_MAX_TOPK; ++t) {
    const int d = tk[t] - 1 - j0;
    m |= (d >= 0 && d < MS_CHUNK) ? (1u << d) : 0u;
  }
  return m;
}

// One workgroup (one wave) per 64 users and per pred index; with tags, one more per 64 users for the entropy (blockIdx.y = n_pred).
__global__ __launch_bounds__(MS_WAVE) void metric_sums_partial_kernel(
    const int64_t* __restrict__ topk_idx, int B, int K, int k_scan, const int64_t* __restrict__ positives, int pos_stride,
    const int32_t* __restrict__ pos_len, int pos_len_stride, MsLists lists, int n_pred, int n_topk,
    const double* __restrict__ disc, const double* __restrict__ idcg, const uint32_t* __restrict__ group_bits, int n_groups,
    const uint32_t* __restrict__ item_tag_bits, int64_t n_items, int n_tags, double* __restrict__ workspace) {
  extern __shared__ double ms_lds[];                     // [64, stride] values, then 64 group words
  const int stride = ms_row_stride(n_topk);
  uint32_t* bits_lds = reinterpret_cast<uint32_t*>(ms_lds + MS_WAVE * stride);
  const int lane = threadIdx.x;
  const int64_t b = (int64_t)blockIdx.x * MS_WAVE + lane;
  const bool act = b < B;
  const int n_act = B - (int64_t)blockIdx.x * MS_WAVE < MS_WAVE ? (int)(B - (int64_t)blockIdx.x * MS_WAVE) : MS_WAVE;
  const int mt_cells = MS_COLS * n_topk;
  const int64_t n_sum = (int64_t)n_pred * n_groups * mt_cells;
  double* part = workspace + (int64_t)blockIdx.x * ms_cells(n_pred, n_groups, n_topk);
  const int64_t* row = topk_idx + (act ? b : 0) * K;
  double* mine = ms_lds + lane * stride;
  const int i = blockIdx.y;
  int tk[MS_MAX_TOPK];
#pragma unroll
  for (int t = 0; t < MS_MAX_TOPK; ++t) tk[t] = t < n_topk ? lists.topk[t] : 0;

  // ---- entropy of the recommended list (every user once, no groups) ----------------------------------------------------
  if (i == n_pred) {
    if (act) {
      uint32_t pl[MS_PLANES];
#pragma unroll
      for (int q = 0; q < MS_PLANES; ++q) pl[q] = 0u;
      const uint32_t tag_mask = n_tags >= 32 ? 0xFFFFFFFFu : ((1u << n_tags) - 1u);
      // three chunks in flight: the ids of chunk n + 2, the tag words of chunk n + 1 (gathered by ids that arrived a trip ago),
      // the counting of chunk n
      int64_t it_b[MS_CHUNK], it_c[MS_CHUNK];
      uint32_t tw_a[MS_CHUNK], tw_b[MS_CHUNK];
      ms_load_chunk(row, 0, k_scan, it_b);
#pragma unroll
      for (int u = 0; u < MS_CHUNK; ++u) tw_a[u] = (it_b[u] >= 0 && it_b[u] < n_items) ? (item_tag_bits[it_b[u]] & tag_mask) : 0u;
      ms_load_chunk(row, MS_CHUNK, k_scan, it_b);
      for (int j0 = 0; j0 < k_scan; j0 += MS_CHUNK) {
        ms_load_chunk(row, j0 + 2 * MS_CHUNK, k_scan, it_c);
#pragma unroll
        for (int u = 0; u < MS_CHUNK; ++u) tw_b[u] = (it_b[u] >= 0 && it_b[u] < n_items) ? (item_tag_bits[it_b[u]] & tag_mask) : 0u;
        const uint32_t cut = ms_cut_mask(tk, j0);
#pragma unroll
        for (int u = 0; u < MS_CHUNK; ++u) {
          uint32_t carry = tw_a[u];
#pragma unroll
          for (int q = 0; q < MS_PLANES; ++q) {          // add one to the counter of every tag in `carry`
            const uint32_t t = pl[q] & carry;
            pl[q] ^= carry;
            carry = t;
          }
          if (!((cut >> u) & 1u)) continue;
          int total = 0;
          for (int c = 0; c < n_tags; ++c) {
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < MS_PLANES; ++q) cnt |= (int)((pl[q] >> c) & 1u) << q;
            total += cnt;
          }
          double h = 0.0;
          for (int c = 0; c < n_tags; ++c) {
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < MS_PLANES; ++q) cnt |= (int)((pl[q] >> c) & 1u) << q;
            if (cnt > 0) {
              const double p = (double)cnt / (double)total;
              h += p * log2(p);
            }
          }
          for (int t = 0; t < n_topk; ++t)
            if (lists.topk[t] == j0 + u + 1) mine[t] = -h;
        }
#pragma unroll
        for (int u = 0; u < MS_CHUNK; ++u) {
          tw_a[u] = tw_b[u];
          it_b[u] = it_c[u];
        }
      }
    }
    __syncthreads();
    if (lane < n_topk) {
      double s = 0.0;
#pragma unroll 8
      for (int u = 0; u < n_act; ++u) s += ms_lds[u * stride + lane];
      part[n_sum + lane] = s;
    }
    return;
  }

  // ---- the six top-k columns of pred index i ---------------------------------------------------------------------------
  const int p = lists.pred[i];
  bits_lds[lane] = act ? group_bits[b * n_pred + i] : 0u;
  if (act) {
    const int64_t* pos = positives + b * pos_stride;
    int64_t cur[MS_CHUNK], nxt[MS_CHUNK];
    ms_load_chunk(row, 0, k_scan, cur);
    int64_t pr[MS_POS_REGS];                             // the first positives in registers (slots past p repeat positives[0])
#pragma unroll
    for (int q = 0; q < MS_POS_REGS; ++q) pr[q] = pos[q <= p ? q : 0];
    const int plen = pos_len[b * pos_len_stride + p];
    int ideal = plen < K ? plen : K;                     // min(pos_len, K); >= 1 for every real user
    if (ideal < 1) ideal = 1;
    int c = 0, first = 0;
    double dcg = 0.0, ap = 0.0;
    for (int j0 = 0; j0 < k_scan; j0 += MS_CHUNK) {
      ms_load_chunk(row, j0 + MS_CHUNK, k_scan, nxt);    // the next chunk's ids travel while this one is scanned
      const uint32_t cut = ms_cut_mask(tk, j0);
#pragma unroll
      for (int u = 0; u < MS_CHUNK; ++u) {
        const int j = j0 + u;
        bool hit = false;
#pragma unroll
        for (int q = 0; q < MS_POS_REGS; ++q) hit |= pr[q] == cur[u];
        for (int q = MS_POS_REGS; q <= p; ++q) hit |= pos[q] == cur[u];
        if (hit && j < k_scan) {
          c += 1;
          dcg += disc[j];
          ap += (double)c / (double)(j + 1);
          if (first == 0) first = j + 1;
        }
        if (!((cut >> u) & 1u)) continue;
        const int jj = j < ideal - 1 ? j : ideal - 1;
        const double v_recall = (double)c / (double)plen, v_ndcg = dcg / idcg[jj], v_hit = c > 0 ? 1.0 : 0.0;
        const double v_mrr = first > 0 ? 1.0 / (double)first : 0.0, v_map = ap / (double)(jj + 1);
        const double v_prec = (double)c / (double)(j + 1);
        for (int t = 0; t < n_topk; ++t) {
          if (lists.topk[t] != j + 1) continue;
          mine[0 * n_topk + t] = v_recall;
          mine[1 * n_topk + t] = v_ndcg;
          mine[2 * n_topk + t] = v_hit;
          mine[3 * n_topk + t] = v_mrr;
          mine[4 * n_topk + t] = v_map;
          mine[5 * n_topk + t] = v_prec;
        }
      }
#pragma unroll
      for (int u = 0; u < MS_CHUNK; ++u) cur[u] = nxt[u];
    }
  }
  __syncthreads();
  for (int cell = lane; cell < n_groups * mt_cells; cell += MS_WAVE) {
    const int g = cell / mt_cells, mt = cell - g * mt_cells;
    double s = 0.0;
#pragma unroll 8
    for (int u = 0; u < n_act; ++u)
      if ((bits_lds[u] >> g) & 1u) s += ms_lds[u * stride + mt];
    part[(int64_t)i * n_groups * mt_cells + cell] = s;
  }
  if (lane < n_groups) {
    long long* part_cnt = reinterpret_cast<long long*>(part + n_sum + n_topk);
    long long n = 0;
    for (int u = 0; u < n_act; ++u) n += (bits_lds[u] >> lane) & 1u;
    part_cnt[i * n_groups + lane] = n;
  }
}

__global__ __launch_bounds__(256) void metric_sums_fold_kernel(const double* __restrict__ workspace, int n_wg, int64_t cells,
                                                               int64_t n_sum, int n_topk, double* __restrict__ sums,
                                                               long long* __restrict__ counts, double* __restrict__ entropy) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  if (c >= n_sum && c < n_sum + n_topk && !entropy) return;      // no tags: nobody wrote those partials
  if (c < n_sum + n_topk) {
    double s = 0.0;
    for (int w = 0; w < n_wg; ++w) s += workspace[(int64_t)w * cells + c];
    if (c < n_sum) sums[c] += s;
    else entropy[c - n_sum] += s;
  } else {
    const long long* ws = reinterpret_cast<const long long*>(workspace);
    long long n = 0;
    for (int w = 0; w < n_wg; ++w) n += ws[(int64_t)w * cells + c];
    counts[c - n_sum - n_topk] += n;
  }
}

extern "C" int64_t mhr_eval_metric_sums_workspace_bytes(int B, int n_pred, int n_groups, int n_topk) {
  if (B < 0 || n_pred < 1 || n_pred > MS_MAX_PRED || n_groups < 1 || n_groups > MS_MAX_GROUPS || n_topk < 1 ||
      n_topk > MS_MAX_TOPK)
    return -1;
  return (int64_t)((B + MS_WAVE - 1) / MS_WAVE) * ms_cells(n_pred, n_groups, n_topk) * 8;
}

extern "C" int mhr_eval_metric_sums(const int64_t* topk_idx, int B, int K, const int64_t* positives, int pos_stride,
                                    const int32_t* pos_len, int pos_len_stride, const int32_t* pred, int n_pred,
                                    const int32_t* topk, int n_topk, const double* disc, const double* idcg,
                                    const uint32_t* group_bits, int n_groups, const uint32_t* item_tag_bits, int64_t n_items,
                                    int n_tags, double* sums, int64_t* counts, double* entropy, void* workspace, void* stream) {
  MHR_REQUIRE(topk_idx, "eval_metric_sums: topk_idx is null");
  MHR_REQUIRE(positives && pos_len, "eval_metric_sums: positives / pos_len is null");
  MHR_REQUIRE(pred && topk, "eval_metric_sums: pred / topk (host arrays) is null");
  MHR_REQUIRE(disc && idcg && group_bits, "eval_metric_sums: disc / idcg / group_bits is null");
  MHR_REQUIRE(sums && counts && workspace, "eval_metric_sums: sums / counts / workspace is null");
  MHR_REQUIRE((item_tag_bits != nullptr) == (entropy != nullptr),
              "eval_metric_sums: item_tag_bits and entropy are given together or not at all");
  MHR_REQUIRE(B >= 0, "eval_metric_sums: B=%d is negative", B);
  MHR_REQUIRE(K >= 1 && K <= MS_MAX_K, "eval_metric_sums: K=%d outside [1, %d]", K, MS_MAX_K);
  MHR_REQUIRE(n_pred >= 1 && n_pred <= MS_MAX_PRED, "eval_metric_sums: n_pred=%d outside [1, %d]", n_pred, MS_MAX_PRED);
  MHR_REQUIRE(n_topk >= 1 && n_topk <= MS_MAX_TOPK, "eval_metric_sums: n_topk=%d outside [1, %d]", n_topk, MS_MAX_TOPK);
  MHR_REQUIRE(n_groups >= 1 && n_groups <= MS_MAX_GROUPS, "eval_metric_sums: n_groups=%d outside [1, %d]", n_groups,
              MS_MAX_GROUPS);
  MHR_REQUIRE(n_tags >= 0 && n_tags <= MS_MAX_TAGS, "eval_metric_sums: n_tags=%d outside [0, %d]", n_tags, MS_MAX_TAGS);
  MHR_REQUIRE(!item_tag_bits || n_items >= 0, "eval_metric_sums: n_items=%lld is negative", (long long)n_items);
  MsLists lists;
  int k_scan = 0, max_pred = 0;
  for (int t = 0; t < MS_MAX_TOPK; ++t) lists.topk[t] = 0;
  for (int i = 0; i < MS_MAX_PRED; ++i) lists.pred[i] = 0;
  for (int t = 0; t < n_topk; ++t) {
    MHR_REQUIRE(topk[t] >= 1 && topk[t] <= K, "eval_metric_sums: topk[%d]=%d outside [1, K=%d]", t, topk[t], K);
    lists.topk[t] = topk[t];
    if (topk[t] > k_scan) k_scan = topk[t];
  }
  for (int i = 0; i < n_pred; ++i) {
    MHR_REQUIRE(pred[i] >= 0, "eval_metric_sums: pred[%d]=%d is negative", i, pred[i]);
    lists.pred[i] = pred[i];
    if (pred[i] > max_pred) max_pred = pred[i];
  }
  MHR_REQUIRE(pos_stride > max_pred && pos_len_stride > max_pred,
              "eval_metric_sums: pos_stride=%d / pos_len_stride=%d must exceed max(pred)=%d", pos_stride, pos_len_stride, max_pred);
  MHR_REQUIRE((uintptr_t)sums % 8 == 0 && (uintptr_t)counts % 8 == 0 && (uintptr_t)workspace % 8 == 0 &&
                  (!entropy || (uintptr_t)entropy % 8 == 0),
              "eval_metric_sums: sums / counts / entropy / workspace must be 8-byte aligned");
  if (B == 0) return MHR_OK;
  const int n_wg = (B + MS_WAVE - 1) / MS_WAVE;
  const int64_t cells = ms_cells(n_pred, n_groups, n_topk);
  const int64_t n_sum = (int64_t)n_pred * n_groups * MS_COLS * n_topk;
  const size_t lds = (size_t)MS_WAVE * ms_row_stride(n_topk) * sizeof(double) + MS_WAVE * sizeof(uint32_t);
  hipLaunchKernelGGL(metric_sums_partial_kernel, dim3((unsigned)n_wg, (unsigned)(n_pred + (item_tag_bits ? 1 : 0))),
                     dim3(MS_WAVE), lds, (hipStream_t)stream, topk_idx, B, K, k_scan, positives, pos_stride, pos_len,
                     pos_len_stride, lists, n_pred, n_topk, disc, idcg, group_bits, n_groups, item_tag_bits, n_items, n_tags,
                     (double*)workspace);
  MHR_CHECK_LAUNCH("eval_metric_sums (partials)");
  hipLaunchKernelGGL(metric_sums_fold_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (const double*)workspace, n_wg, cells, n_sum, n_topk, sums, (long long*)counts, entropy);
  MHR_CHECK_LAUNCH("eval_metric_sums (fold)");
  return MHR_OK;
}
