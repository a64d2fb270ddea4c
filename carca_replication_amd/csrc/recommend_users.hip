// The k best USERS per listed item (include/carca_hip.h: carca_recommend_users / carca_audience_read):
// carca_recommend_among's question turned round, for a campaign that asks who should hear about each of Q items.
//
// carca_recommend_users runs carca_recommend_among's scoring and exclusion launches unchanged (rc::rc_score over
// rc::ListedItems, recommend_score.h: the same instantiation, so a pair's raw logit has recommend's bits), which leave
// the [B, Q] raw logits in stream scratch with the exclusion sentinel in place, and then one merge launch:
//   au_merge_kernel  a workgroup owns AU_COLS = 16 adjacent item columns and walks the B rows AU_ROWS = 64 at a time
//                    (16 consecutive lanes read one 64-byte row segment).  Per column it keeps an LDS list of 64-bit keys
//                    rc::order_key(order bits of the logit, user id) -- larger key = larger logit, ties to the smaller
//                    user id -- seeded with the column's k running keys, and a threshold, the column's current k-th key.
//                    A lane skips an excluded pair (order bits 0), a dropped user (negative id) and a key at or below the
//                    threshold; a survivor is appended through an integer LDS atomic on the column's counter.  Before a
//                    round could overflow a list the workgroup sorts every list (the bitonic pattern of group_select.h)
//                    and keeps the k largest; the last sort's first k keys go back to the running state, descending.
// Keys are distinct per (item, user), a key is dropped only below k larger ones, and the result is the sorted k largest
// of old and new keys together: it depends neither on the order of the appends nor on how the users were split into
// calls.  Integer LDS atomics only, no scratch beyond the logit buffer.
//
// carca_audience_read turns the keys into linked scores (rc::link on the device, recommend's bits) and user ids.
#include "recommend_score.h"

namespace {

constexpr int AU_THREADS = 256;
constexpr int AU_COLS = 16;                         // item columns per workgroup: a row segment of 64 bytes
constexpr int AU_ROWS = 64;                         // users per round: AU_THREADS / AU_COLS rows, four times
constexpr int AU_ROW_STEP = AU_THREADS / AU_COLS;   // rows one pass of the workgroup covers
constexpr long long AU_MAX_PAIRS = 1ll << 31;       // B * Q stays below it, as the list calls bound B * N

// The keys a column's list holds: k kept ones and a round's appends, or 2k, rounded up to a power of two for the sort
// (k <= 64: 128; beyond: 256, 16 x 257 x 8 B = 32.1 KB of LDS).
inline int au_capacity(int k) {
  int P = 2;
  while (P < std::max(2 * k, k + AU_ROWS)) P <<= 1;
  return P;
}

// Column c's list is list[c * (P + 1) .. + P): the stride is padded by one key, so that the 16 columns' entries at one
// position fall on 16 different pairs of the 32 write banks (a stride of P keys puts them all on one).
// cnt[c]: the keys in the list; thr[c]: the key a new one has to beat.  Sorts every list descending and keeps k: whole
// workgroup; the caller has synchronised since the last append; ends with a barrier.
__device__ __forceinline__ void au_compact(unsigned long long* list, int* cnt, unsigned long long* thr, int P, int k) {
  const int tid = threadIdx.x, stride_c = P + 1;
  for (int i = tid; i < AU_COLS * P; i += AU_THREADS) {  // what lies past a list's keys (an earlier sort's losers)
    const int c = i / P, j = i % P;
    if (j >= cnt[c]) list[c * stride_c + j] = 0ull;
  }
  __syncthreads();
  const int half = P >> 1;
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < AU_COLS * half; i += AU_THREADS) {
        const int c = i / half, j = i % half;
        const int a = ((j & ~(stride - 1)) << 1) | (j & (stride - 1)), b = a | stride;
        unsigned long long* col = list + c * stride_c;
        const unsigned long long ka = col[a], kb = col[b];
        const bool desc = (a & size) == 0;
        if (desc ? (ka < kb) : (ka > kb)) col[a] = kb, col[b] = ka;
      }
      __syncthreads();
    }
  }
  if (tid < AU_COLS) {
    cnt[tid] = k;  // (zeros stand in where a list holds fewer: any key beats them)
    thr[tid] = list[tid * stride_c + k - 1];
  }
  __syncthreads();
}

// logits [B, ld_s] raw logits with the sentinel in place, Q columns; keys [Q, ld_keys], the first k of a row read and
// written; user_ids [B] or null (then user_base + row).  P = au_capacity(k); dynamic LDS: AU_COLS * (P + 1) keys.
__global__ __launch_bounds__(AU_THREADS) void au_merge_kernel(const float* __restrict__ logits, int ld_s, int B, int Q, int k,
                                                              int P, unsigned long long* __restrict__ keys, int ld_keys,
                                                              const int32_t* __restrict__ user_ids, int user_base) {
  extern __shared__ unsigned long long au_list[];
  __shared__ int cnt[AU_COLS];
  __shared__ unsigned long long thr[AU_COLS];
  const int tid = threadIdx.x, c = tid & (AU_COLS - 1), r = tid / AU_COLS;
  const int col0 = blockIdx.x * AU_COLS, col = col0 + c, stride_c = P + 1;
  for (int i = tid; i < AU_COLS * k; i += AU_THREADS) {  // the running keys seed the lists
    const int cc = i / k, j = i % k;
    au_list[cc * stride_c + j] = col0 + cc < Q ? keys[(size_t)(col0 + cc) * ld_keys + j] : 0ull;
  }
  __syncthreads();
  if (tid < AU_COLS) {
    cnt[tid] = k;
    thr[tid] = au_list[tid * stride_c + k - 1];
  }
  __syncthreads();
  const unsigned* bits = reinterpret_cast<const unsigned*>(logits);
  for (int u0 = 0; u0 < B; u0 += AU_ROWS) {
    // every list has room for a round: cnt <= P - AU_ROWS here, and a column takes at most AU_ROWS appends per round
    const unsigned long long t = thr[c];
#pragma unroll
    for (int s = 0; s < AU_ROWS / AU_ROW_STEP; ++s) {
      const int u = u0 + s * AU_ROW_STEP + r;
      if (u < B && col < Q) {
        const unsigned o = rc::order_bits(bits[(size_t)u * ld_s + col]);
        const int uid = user_ids ? user_ids[u] : user_base + u;
        if (o != 0u && uid >= 0) {  // (order bits 0: the exclusion sentinel; a negative id: a dropped row)
          const unsigned long long key = rc::order_key(o, (unsigned)uid);
          if (key > t) {
            const int at = atomicAdd(&cnt[c], 1);
            if (at < P) au_list[c * stride_c + at] = key;
          }
        }
      }
    }
    __syncthreads();
    if (__syncthreads_or(cnt[c] > P - AU_ROWS)) au_compact(au_list, cnt, thr, P, k);
  }
  au_compact(au_list, cnt, thr, P, k);
  for (int i = tid; i < AU_COLS * k; i += AU_THREADS) {
    const int cc = i / k, j = i % k;
    if (col0 + cc < Q) keys[(size_t)(col0 + cc) * ld_keys + j] = au_list[cc * stride_c + j];
  }
}

__global__ __launch_bounds__(AU_THREADS) void au_read_kernel(const unsigned long long* __restrict__ keys, int ld_keys, int n,
                                                             int k, int decoder, float* __restrict__ scores,
                                                             int64_t* __restrict__ users) {
  const int i = blockIdx.x * AU_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[(size_t)(i / k) * ld_keys + i % k];
  scores[i] = key ? rc::link(rc::unorder_bits((unsigned)(key >> 32)), decoder) : 0.f;  // (fewer than k eligible users:
  users[i] = key ? (int64_t)rc::key_id(key) : (int64_t)-1;                                //  score 0, user -1)
}

}  // namespace

extern "C" int carca_recommend_users(const CarcaRecommendDesc* desc, const CarcaCandidates* items, const CarcaAudience* state,
                                     void* stream_) {
  CARCA_CHECK_ARG(desc, "recommend_users: null descriptor");
  const CarcaRecommendDesc& D = *desc;
  hipStream_t stream = (hipStream_t)stream_;
  // (rc_check's output fields -- scores, ids_out -- are not this call's: its outputs are the keys)
  if (int rc = rc::check_model(D, "recommend_users")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "recommend_users: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::RC_KMAX, "recommend_users: k = %d exceeds the largest k, 128", D.k);
  if (int rc = rc::check_candidates(items, "recommend_users")) return rc;
  CARCA_CHECK_ARG(state, "recommend_users: null audience state");
  const int Q = items->n;
  CARCA_CHECK_ARG(state->keys || Q == 0, "recommend_users: null key state");
  CARCA_CHECK_ARG(state->ld_keys >= D.k, "recommend_users: ld_keys = %d shorter than k = %d", state->ld_keys, D.k);
  CARCA_CHECK_ARG(state->user_ids || (state->user_base >= 0 && state->user_base <= 0x7FFFFFFF - D.B),
                  "recommend_users: user_base = %d: the row ids must stay below 2^31", state->user_base);
  CARCA_CHECK_SUPPORTED(D.B <= 0x7FFFFFFF - AU_ROWS, "recommend_users: B = %d: the row index would overflow", D.B);
  CARCA_CHECK_SUPPORTED((long long)D.B * Q < AU_MAX_PAIRS, "recommend_users: B * Q = %lld does not fit an int (split the users)",
                        (long long)D.B * Q);
  if (Q == 0) return CARCA_OK;  // no item, no state
  float* logits = nullptr;
  const rc::ListedItems map{items->ids, Q};
  if (int rc = rc::rc_score(D, map, map, Q, stream, &logits)) return rc;
  const int P = au_capacity(D.k);
  hipLaunchKernelGGL(au_merge_kernel, dim3((Q + AU_COLS - 1) / AU_COLS), dim3(AU_THREADS),
                     (size_t)AU_COLS * (P + 1) * sizeof(unsigned long long), stream, logits, Q, D.B, Q, D.k, P, state->keys,
                     state->ld_keys, state->user_ids, state->user_base);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_audience_read(const unsigned long long* keys, int ld_keys, int n_rows, int k, int decoder, float* scores,
                                   int64_t* users, void* stream) {
  CARCA_CHECK_ARG(n_rows >= 0, "audience_read: n_rows must not be negative");
  CARCA_CHECK_ARG(k >= 1, "audience_read: k must be positive");
  CARCA_CHECK_SUPPORTED(k <= rc::RC_KMAX, "audience_read: k = %d exceeds the largest k, 128", k);
  CARCA_CHECK_ARG(ld_keys >= k, "audience_read: ld_keys = %d shorter than k = %d", ld_keys, k);
  CARCA_CHECK_ARG(decoder >= 0 && decoder <= 2, "audience_read: decoder must be 0 (cross-attention), 1 (dot) or 2 (normalised dot)");
  CARCA_CHECK_SUPPORTED((long long)n_rows * k < AU_MAX_PAIRS, "audience_read: n_rows * k = %lld does not fit an int",
                        (long long)n_rows * k);
  if (n_rows == 0) return CARCA_OK;
  CARCA_CHECK_ARG(keys && scores && users, "audience_read: null pointer");
  const int n = n_rows * k;
  hipLaunchKernelGGL(au_read_kernel, dim3((n + AU_THREADS - 1) / AU_THREADS), dim3(AU_THREADS), 0, (hipStream_t)stream, keys,
                     ld_keys, n, k, decoder, scores, users);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
