// The exclusion and selection launches of a full-catalogue top-k over a [B, n_items] buffer of raw logits, shared by
// carca_recommend (recommend.hip), carca_knn_recommend (knn_catalogue.hip) and carca_similar_items (similar_items.hip).
// Desc is the caller's descriptor, or a view (SelectView) with these fields: n_items, k, decoder, exclude / n_exclude / ld_exclude, scores / ld_scores, ids_out / ld_ids_out.
// `decoder` picks the link applied to the k selected logits: an int (recommend_common.h: rc::link) or rc::IdentityLink
// (the raw logit, for models without a link).  Keys are built and taken apart by recommend_common.h's helpers
// (rc::order_key, rc::key_id); an item whose order bits are 0 holds the exclusion sentinel and is skipped.
// Map (recommend_common.h) says what a column of the buffer is: rc::AllItems, column = item id, or rc::ListedItems,
// column = position in an ascending candidate list ([B, C] buffer; keys carry the position, ids_out the id behind it), or
// rc::UserLists, a list of its own per user: each workgroup takes its user's row of the map (for_user).
#pragma once
#include "recommend_common.h"

namespace rc {

constexpr int RC_SEL_THREADS = 256;   // selection workgroup
constexpr int RC_KMAX = 128;          // largest k
constexpr unsigned RC_SENTINEL = 0xFFFFFFFFu;  // a negative NaN pattern no arithmetic here produces; order key 0

struct IdentityLink {};
__device__ __forceinline__ float link(float y, IdentityLink) { return y; }

// the view of a caller without a model descriptor (knn_catalogue.hip, similar_items.hip): no link; the exclusion fields
// stay zero where the caller has no exclusion launch
struct SelectView {
  int n_items, k;
  IdentityLink decoder;
  const int32_t* exclude;
  int n_exclude, ld_exclude;
  float* scores;
  int ld_scores;
  int64_t* ids_out;
  int ld_ids_out;
};

// ---- exclusion ----------------------------------------------------------------------------------------------
template <class Desc, class Map = AllItems>
__global__ __launch_bounds__(64) void rc_exclude_kernel(Desc D, float* __restrict__ logits, int ld_s, Map map) {
  const int u = blockIdx.x;
  const auto m = map.for_user(u);
  float* row = logits + (size_t)u * ld_s;
  const float sent = __uint_as_float(RC_SENTINEL);
  if (!Map::listed && threadIdx.x == 0) row[0] = sent;  // id 0 is the padding item (carca.py:73); no list holds it
  for (int e = threadIdx.x; e < D.n_exclude; e += 64) {
    const int id = D.exclude[(size_t)u * D.ld_exclude + e];
    if (id > 0 && id < D.n_items) {  // (0 = no entry; duplicates write the same word)
      const int at = m.find(id);
      if (at >= 0) row[at] = sent;
    }
  }
}

// ---- selection ----------------------------------------------------------------------------------------------
template <class Desc, class Map = AllItems>
__global__ __launch_bounds__(RC_SEL_THREADS) void rc_select_kernel(Desc D, const float* __restrict__ logits, int ld_s,
                                                                   Map map) {
  __shared__ int hist[256];
  __shared__ unsigned long long skey[RC_KMAX];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_pbits, s_need, s_done, s_keff, s_cnt;
  const int tid = threadIdx.x, u = blockIdx.x;
  const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
  const auto m = map.for_user(u);
  const int n = m.size(D.n_items);
  if (tid == 0) s_prefix = 0ull, s_pbits = 0, s_done = 0, s_cnt = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;  // (RC_SEL_THREADS == 256 bins)
    __syncthreads();
    const unsigned long long prefix = s_prefix;
    const int pbits = s_pbits;
    for (int i = tid; i < n; i += RC_SEL_THREADS) {
      const unsigned o = rc::order_bits(row[i]);
      if (o == 0u) continue;  // sentinel: excluded
      const unsigned long long key = rc::order_key(o, (unsigned)i);
      if (pbits > 0 && (key >> (64 - pbits)) != prefix) continue;
      atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int need;
      if (pbits == 0) {  // first pass: the histogram holds every eligible item
        int total = 0;
        for (int b = 0; b < 256; ++b) total += hist[b];
        need = min(D.k, total);
        s_keff = need;
      } else {
        need = s_need;
      }
      if (need == 0) {
        s_done = 1;
      } else {
        int above = 0, b = 255;
        for (; b > 0; --b) {
          if (above + hist[b] >= need) break;
          above += hist[b];
        }
        need -= above;
        s_prefix = (prefix << 8) | (unsigned long long)b;
        s_pbits = pbits + 8;
        s_need = need;
        s_done = hist[b] == need;  // every key under the new prefix is taken: no lower digit matters
      }
    }
    __syncthreads();
    if (s_done) break;
  }
  const int keff = s_keff;
  // collect the keff keys >= prefix (exactly keff of them: keys are unique), sort them descending
  if (tid < RC_KMAX) skey[tid] = 0ull;
  __syncthreads();
  if (keff > 0) {
    const unsigned long long prefix = s_prefix;
    const int pbits = s_pbits;
    for (int i = tid; i < n; i += RC_SEL_THREADS) {
      const unsigned o = rc::order_bits(row[i]);
      if (o == 0u) continue;
      const unsigned long long key = rc::order_key(o, (unsigned)i);
      if ((key >> (64 - pbits)) >= prefix) {
        const int at = atomicAdd(&s_cnt, 1);
        if (at < RC_KMAX) skey[at] = key;
      }
    }
  }
  __syncthreads();
  for (int size = 2; size <= RC_KMAX; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < RC_KMAX) {
        const int p = tid ^ stride;
        if (p > tid) {
          const unsigned long long a = skey[tid], b = skey[p];
          const bool desc = (tid & size) == 0;
          if (desc ? (a < b) : (a > b)) skey[tid] = b, skey[p] = a;
        }
      }
      __syncthreads();
    }
  }
  if (tid < D.k) {
    float score = 0.f;
    long long id = 0;
    if (tid < keff) {
      const unsigned long long key = skey[tid];
      id = (long long)m.item((int)rc::key_id(key));
      const float y = rc::unorder_bits((unsigned)(key >> 32));
      score = rc::link(y, D.decoder);
    }
    D.scores[(size_t)u * D.ld_scores + tid] = score;
    D.ids_out[(size_t)u * D.ld_ids_out + tid] = id;
  }
}

}  // namespace rc
