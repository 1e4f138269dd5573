// split_mode = average: the decode that ranks the MEAN of a user's finite head scores (reference file:line under code/REC/:
// evaluator/collector.py:227-230 - sum of the finite heads / (finite count + 1e-8), then torch.topk; the -inf masks come from
// model/IDNet/hstu.py:982-1015 (tags, given priors) and trainer/trainer.py:724-726 (pad id, history)).
//
// The scorers are not touched.  Head h is finite for item n iff n is not the pad id, not in the user's history and
// (row_bits[b,h] & tag_bits[n]) != 0, so the set of finite heads depends on the item only through its tag word w, and the dot
// product is linear:  mean(b, n) = < q[b,w], items[n] >,  q[b,w] = (sum of the heads live for w) / count.  A catalog holds few
// distinct tag words ("patterns", at most 32 here), so the mean decode is a single-head decode with P query rows per user, each
// restricted to the items of its own pattern (ops.catalog_topk_mean).  Three small kernels around the existing scorers:
//   head_mean_queries      : the P fp32 query rows of every user and their row bits (a row with no live head is dead: bits 0)
//   rescore_mean_f32       : the reference's own arithmetic on the candidates of row (b, p): H fp32 dots, finite ones summed in
//                            ascending h, divided by float(count) (count + 1e-8 rounds to count in fp32 for count >= 1)
//   catalog_mean_rows_dense: every item's mean for a FEW users, all masks applied - the repair of users whose candidate lists
//                            cannot be certified or whose k-th mean is not > 0: an item masked in EVERY head scores 0 / 1e-8 = 0
//                            in the reference, not -inf, and outranks negative means, so it is stored as 0.0f
#include "mhr_common.h"

namespace {

__global__ __launch_bounds__(64) void head_mean_queries_kernel(const float* __restrict__ heads, const uint32_t* __restrict__ row_bits,
                                                               const uint32_t* __restrict__ words, int H, int P, int dim, int has_tags,
                                                               float* __restrict__ q, uint32_t* __restrict__ q_bits) {
  const int64_t bp = blockIdx.x;
  const int64_t b = bp / P;
  const int p = (int)(bp - b * P);
  const uint32_t w = words[p];
  int count = 0;
  for (int h = 0; h < H; ++h) count += (row_bits[b * H + h] & w) != 0u ? 1 : 0;
  for (int c = threadIdx.x * 4; c < dim; c += 64 * 4) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int h = 0; h < H; ++h)                                     // ascending h, like the re-score
      if ((row_bits[b * H + h] & w) != 0u) acc += *reinterpret_cast<const f32x4*>(heads + (b * H + h) * dim + c);
    if (count > 0) {
      const float n = (float)count;
      acc[0] /= n; acc[1] /= n; acc[2] /= n; acc[3] /= n;
    }
    *reinterpret_cast<f32x4*>(q + bp * dim + c) = acc;              // count == 0: exactly 0
  }
  // the pattern word of row p: bit p of the one-hot pattern table; without a tag table the scorers give every item bit 31
  if (threadIdx.x == 0) q_bits[bp] = count > 0 ? (has_tags ? (1u << p) : 0x80000000u) : 0u;
}

// one wave per (row, candidate), 16 bytes per lane, wave-shuffle sum - the dot of rescore_f32_kernel, once per head
__global__ __launch_bounds__(256) void rescore_mean_f32_kernel(const float* __restrict__ heads, const float* __restrict__ items, int dim,
                                                               int64_t n_items, int H, int P, const uint32_t* __restrict__ tag_bits,
                                                               const uint32_t* __restrict__ row_bits, const int64_t* __restrict__ cand_idx,
                                                               int k2, const int32_t* __restrict__ cand_cnt, int64_t n_pairs,
                                                               float* __restrict__ out_val, int32_t* __restrict__ out_idx) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * (blockDim.x >> 6);
  for (int64_t pr = wave; pr < n_pairs; pr += n_waves) {
    const int64_t row = pr / k2;
    const int j = (int)(pr - row * k2);
    if (j >= cand_cnt[row]) continue;
    const int64_t n = cand_idx[pr];
    const int64_t b = row / P;
    float sum = 0.f;
    int count = 0;
    if (n >= 0 && n < n_items) {
      const uint32_t tb = tag_bits ? tag_bits[n] : 0x80000000u;
      const float* it = items + n * dim;
      for (int h = 0; h < H; ++h) {
        const float* u = heads + (b * H + h) * dim;
        float acc = 0.f;
        for (int c = lane * 4; c < dim; c += 256) {
          const f32x4 a = *reinterpret_cast<const f32x4*>(u + c), v = *reinterpret_cast<const f32x4*>(it + c);
          acc += a[0] * v[0] + a[1] * v[1] + a[2] * v[2] + a[3] * v[3];
        }
        acc = wave_sum(acc);
        if ((row_bits[b * H + h] & tb) != 0u) {                     // the REAL tag word decides which heads are finite
          sum += acc;
          ++count;
        }
      }
    }
    if (lane == 0) {
      out_val[pr] = count > 0 ? sum / (float)count : 0.f;
      out_idx[pr] = (int32_t)n;
    }
  }
}

// One user per blockIdx.y; his H head rows and their row bits sit in LDS, the dots are formed for G = min(H, 8) heads at a time.
// A wave takes 64 consecutive items: lane j owns item base + j (its tag word, pad / history test, running sum and count, and
// the coalesced store), the wave forms the dots of one item at a time and lane j folds those of its item.
template <int G>
__global__ __launch_bounds__(256) void mean_rows_dense_kernel(const float* __restrict__ heads, const float* __restrict__ items, int dim,
                                                              int64_t n_items, const int32_t* __restrict__ user_list, int H,
                                                              const uint32_t* __restrict__ tag_bits, const uint32_t* __restrict__ row_bits,
                                                              const int32_t* __restrict__ hist_ptr, const int64_t* __restrict__ hist_items,
                                                              float* __restrict__ out_val, int32_t* __restrict__ out_idx,
                                                              int32_t* __restrict__ out_cnt) {
  extern __shared__ __attribute__((aligned(16))) float u_lds[];          // [H][dim] fp32, then [H] row bits
  uint32_t* rb_lds = reinterpret_cast<uint32_t*>(u_lds + (int64_t)H * dim);
  const int j = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = user_list[j];
  for (int i = threadIdx.x * 4; i < H * dim; i += 256 * 4)
    *reinterpret_cast<f32x4*>(u_lds + i) = *reinterpret_cast<const f32x4*>(heads + b * H * dim + i);
  for (int h = threadIdx.x; h < H; h += 256) rb_lds[h] = row_bits[b * H + h];
  __syncthreads();
  int hp0 = 0, hp1 = 0;
  if (hist_ptr) {
    hp0 = hist_ptr[b];
    hp1 = hist_ptr[b + 1];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) out_cnt[j] = (int32_t)n_items;

  const int64_t n_chunks = (n_items + 63) / 64;
  for (int64_t ch = (int64_t)blockIdx.x * 4 + wave; ch < n_chunks; ch += (int64_t)gridDim.x * 4) {
    const int64_t base = ch * 64, n = base + lane;
    const int n_here = (int)min((int64_t)64, n_items - base);          // wave-uniform
    uint32_t tb = 0u;
    if (n < n_items) {
      bool ok = n != 0;                                                // n == 0: the pad id (trainer.py:724)
      if (ok && hist_items) {                                          // trainer.py:725-726: the user's own history
        int lo = hp0, hi = hp1;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (hist_items[mid] < n) lo = mid + 1;
          else hi = mid;
        }
        ok = !(lo < hp1 && hist_items[lo] == n);
      }
      if (ok) tb = tag_bits ? tag_bits[n] : 0x80000000u;               // masked for every head: no bit matches
    }
    float sum = 0.f;
    int count = 0;
    for (int i = 0; i < n_here; ++i) {
      const float* it = items + (base + i) * dim;
      for (int h0 = 0; h0 < H; h0 += G) {
        float acc[G];
#pragma unroll
        for (int r = 0; r < G; ++r) acc[r] = 0.f;
        for (int c = lane * 4; c < dim; c += 256) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(it + c);
#pragma unroll
          for (int r = 0; r < G; ++r) {
            if (h0 + r < H) {
              const f32x4 a = *reinterpret_cast<const f32x4*>(u_lds + (h0 + r) * dim + c);
              acc[r] += a[0] * v[0] + a[1] * v[1] + a[2] * v[2] + a[3] * v[3];
            }
          }
        }
#pragma unroll
        for (int r = 0; r < G; ++r) {
          if (h0 + r < H) {                                            // wave-uniform
            const float s = wave_sum(acc[r]);
            if (lane == i && (rb_lds[h0 + r] & tb) != 0u) {            // ascending h
              sum += s;
              ++count;
            }
          }
        }
      }
    }
    if (n < n_items) {
      // collector.py:228: an item with no finite head is 0 / 1e-8 = 0, not -inf
      out_val[(int64_t)j * n_items + n] = count > 0 ? sum / (float)count : 0.f;
      out_idx[(int64_t)j * n_items + n] = (int32_t)n;
    }
  }
}

}  // namespace

extern "C" int mhr_head_mean_queries(const float* heads, const uint32_t* row_bits, const uint32_t* words, int B, int H, int P,
                                     int dim, int has_tags, float* q, uint32_t* q_bits, void* stream) {
  MHR_REQUIRE(heads && row_bits && words && q && q_bits, "head_mean_queries: null pointer");
  MHR_REQUIRE(B >= 0 && H >= 1 && P >= 1 && P <= 32 && dim > 0 && dim % 4 == 0,
              "head_mean_queries: bad sizes (H=%d, P=%d must be in [1,32], dim=%d a multiple of 4)", H, P, dim);
  MHR_REQUIRE(has_tags || P == 1, "head_mean_queries: P=%d patterns need a tag table", P);
  if (B == 0) return MHR_OK;
  MHR_REQUIRE((int64_t)B * P < (1ll << 31), "head_mean_queries: B*P too large");
  hipLaunchKernelGGL(head_mean_queries_kernel, dim3((unsigned)(B * P)), dim3(64), 0, (hipStream_t)stream, heads, row_bits, words, H, P,
                     dim, has_tags, q, q_bits);
  MHR_CHECK_LAUNCH("head_mean_queries");
  return MHR_OK;
}

extern "C" int mhr_rescore_mean_f32(const float* heads, const float* items, int dim, int64_t n_items, int H, int P,
                                    const uint32_t* tag_bits, const uint32_t* row_bits, const int64_t* cand_idx, int n_rows, int k2,
                                    const int32_t* cand_cnt, float* out_val, int32_t* out_idx, void* stream) {
  MHR_REQUIRE(heads && items && row_bits && cand_idx && cand_cnt && out_val && out_idx, "rescore_mean_f32: null pointer");
  MHR_REQUIRE(dim > 0 && dim % 4 == 0 && n_rows >= 0 && k2 >= 1 && n_items > 0 && H >= 1 && P >= 1 && n_rows % P == 0,
              "rescore_mean_f32: bad sizes (dim=%d, n_rows=%d must be a multiple of P=%d)", dim, n_rows, P);
  if (n_rows == 0) return MHR_OK;
  const int64_t n_pairs = (int64_t)n_rows * k2;
  hipLaunchKernelGGL(rescore_mean_f32_kernel, dim3(mhr_grid_for(n_pairs, 4)), dim3(256), 0, (hipStream_t)stream, heads, items, dim,
                     n_items, H, P, tag_bits, row_bits, cand_idx, k2, cand_cnt, n_pairs, out_val, out_idx);
  MHR_CHECK_LAUNCH("rescore_mean_f32");
  return MHR_OK;
}

extern "C" int mhr_catalog_mean_rows_dense(const float* heads, const float* items, int dim, int64_t n_items, const int32_t* user_list,
                                           int n_list, int H, const uint32_t* tag_bits, const uint32_t* row_bits,
                                           const int32_t* hist_ptr, const int64_t* hist_items, float* out_val, int32_t* out_idx,
                                           int32_t* out_cnt, void* stream) {
  MHR_REQUIRE(heads && items && user_list && row_bits && out_val && out_idx && out_cnt, "catalog_mean_rows_dense: null pointer");
  MHR_REQUIRE(dim > 0 && dim % 4 == 0 && H >= 1 && H <= 64 && (int64_t)H * dim <= 16000,
              "catalog_mean_rows_dense: H=%d x dim=%d unsupported (dim a multiple of 4, H <= 64, H x dim <= 16000: the head rows sit in LDS)",
              H, dim);
  MHR_REQUIRE(n_items > 0 && n_items < (1ll << 31) && n_list >= 0 && n_list <= 65535, "catalog_mean_rows_dense: bad sizes");
  MHR_REQUIRE((hist_ptr == nullptr) == (hist_items == nullptr), "catalog_mean_rows_dense: hist_ptr/hist_items must both be set or null");
  if (n_list == 0) return MHR_OK;
  hipStream_t s = (hipStream_t)stream;
  int gx = (int)((n_items + 255) / 256);
  const int want = (2048 + n_list - 1) / n_list;                // ~8 workgroups per CU over all listed users
  if (gx > want) gx = want;
  if (gx < 1) gx = 1;
  const size_t lds = (size_t)H * dim * sizeof(float) + (size_t)H * sizeof(uint32_t);
#define L_(G_)                                                                                                               \
  hipLaunchKernelGGL((mean_rows_dense_kernel<G_>), dim3(gx, n_list), dim3(256), lds, s, heads, items, dim, n_items, user_list, H, \
                     tag_bits, row_bits, hist_ptr, hist_items, out_val, out_idx, out_cnt)
  if (H <= 2) L_(2);
  else if (H <= 4) L_(4);
  else L_(8);
#undef L_
  MHR_CHECK_LAUNCH("catalog_mean_rows_dense");
  return MHR_OK;
}

extern "C" int64_t mhr_catalog_mean_rows_dense_workspace_bytes(int n_list, int64_t n_items) {
  if (n_list <= 0 || n_items <= 0) return 0;
  return (int64_t)n_list * n_items * 8 + (int64_t)n_list * 4;   // out_val f32 + out_idx i32 per (user, item), out_cnt i32 per user
}
