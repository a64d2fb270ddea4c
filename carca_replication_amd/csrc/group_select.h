// The selection launches of the item-group calls (include/carca_hip.h: carca_recommend_groups / carca_recommend_capped;
// DESIGN.md section 23), behind the sweep and the exclusion launch of recommend.hip.
//
// The catalogue is swept once in group-major order (rc::ListedItems over CarcaItemGroups::order), so a user's row of the
// [B, C] logit buffer holds every group's logits side by side: group g owns columns [offsets[g], offsets[g + 1]).
//   rg_select_kernel  grid (B, G): workgroup (u, g) takes the k best of its segment.  Keys are rc::order_key(order bits,
//                     position): `order` ascends in id inside a group, so a position tie is an id tie, as under
//                     rc::ListedItems.  It writes order[position] and the linked logit (carca_recommend_groups), or, RAW,
//                     the key built again on the item's id into a [B, G, k] key buffer (stage 1 of carca_recommend_capped:
//                     positions do not order as ids do ACROSS groups);
//   rg_merge_kernel   grid (B): the k largest of a user's G * m id keys (0 = hole), linked and written out (stage 2).
// Both run gs_topk: a segment of up to GS_SORT_MAX columns is read once and its keys are sorted in LDS (as
// recommend_lists.hip sorts a short list); a longer one runs rc_select_kernel's MSB-first radix select (catalogue_select.h)
// and sorts the survivors.  The two regimes give the same keys.  Integer LDS atomics only (histogram, slot counter); keys
// are distinct, so the result does not depend on scheduling.
#pragma once
#include "catalogue_select.h"

namespace rc {

constexpr int GS_THREADS = 256;    // selection workgroup (== the radix histogram's bins)
constexpr int GS_SORT_MAX = 1024;  // longest segment whose keys are sorted whole in LDS
static_assert(GS_SORT_MAX >= RC_KMAX, "the key block holds the radix select's survivors too");

struct GsLds {
  unsigned long long key[GS_SORT_MAX];
  int hist[256];
  unsigned long long prefix;
  int pbits, need, done, keff, cnt;
};

// bitonic sort of key[0 .. P) descending (zeros last); P a power of two >= 2, workgroup-uniform.  The caller has
// published key[]; ends with a barrier
__device__ __forceinline__ void gs_sort_desc(unsigned long long* key, int P) {
  const int tid = threadIdx.x;
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P / 2; i += GS_THREADS) {
        const int a = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), b = a | stride;
        const unsigned long long ka = key[a], kb = key[b];
        const bool desc = (a & size) == 0;
        if (desc ? (ka < kb) : (ka > kb)) key[a] = kb, key[b] = ka;
      }
      __syncthreads();
    }
  }
}

// Leaves the k largest of the keys key_at(0 .. n - 1) in Z.key[0 .. k), descending, followed by zeros where fewer than k
// are non-zero.  key_at(i) is column i's key, 0 where the column is not eligible; non-zero keys are distinct.  Whole
// workgroup of GS_THREADS threads; n and k (1 <= k <= RC_KMAX) are workgroup-uniform; Z is not in use.  Ends with a barrier.
template <class KeyAt>
__device__ __forceinline__ void gs_topk(KeyAt key_at, int n, int k, GsLds& Z) {
  const int tid = threadIdx.x;
  if (n <= GS_SORT_MAX) {  // one read of the segment, sorted whole
    int P = 2;
    while (P < n) P <<= 1;
    const int fill = max(P, k);
    for (int i = tid; i < fill; i += GS_THREADS) Z.key[i] = i < n ? key_at(i) : 0ull;
    __syncthreads();
    gs_sort_desc(Z.key, P);
    return;
  }
  // rc_select_kernel's radix select: a byte of the key per pass, from the top, until the k-th largest key's prefix is known
  if (tid == 0) Z.prefix = 0ull, Z.pbits = 0, Z.done = 0, Z.cnt = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    Z.hist[tid] = 0;  // (GS_THREADS == 256 bins)
    __syncthreads();
    const unsigned long long prefix = Z.prefix;
    const int pbits = Z.pbits;
    for (int i = tid; i < n; i += GS_THREADS) {
      const unsigned long long key = key_at(i);
      if (key == 0ull) continue;
      if (pbits > 0 && (key >> (64 - pbits)) != prefix) continue;
      atomicAdd(&Z.hist[(int)((key >> shift) & 255ull)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int need;
      if (pbits == 0) {  // first pass: the histogram holds every eligible column
        int total = 0;
        for (int b = 0; b < 256; ++b) total += Z.hist[b];
        need = min(k, total);
        Z.keff = need;
      } else {
        need = Z.need;
      }
      if (need == 0) {
        Z.done = 1;
      } else {
        int above = 0, b = 255;
        for (; b > 0; --b) {
          if (above + Z.hist[b] >= need) break;
          above += Z.hist[b];
        }
        need -= above;
        Z.prefix = (prefix << 8) | (unsigned long long)b;
        Z.pbits = pbits + 8;
        Z.need = need;
        Z.done = Z.hist[b] == need;  // every key under the new prefix is taken: no lower digit matters
      }
    }
    __syncthreads();
    if (Z.done) break;
  }
  // collect the keff keys >= prefix (exactly keff of them: keys are distinct), sort them
  const int keff = Z.keff;
  int P = 2;
  while (P < k) P <<= 1;
  if (tid < P) Z.key[tid] = 0ull;  // (P <= RC_KMAX <= GS_THREADS)
  __syncthreads();
  if (keff > 0) {
    const unsigned long long prefix = Z.prefix;
    const int pbits = Z.pbits;
    for (int i = tid; i < n; i += GS_THREADS) {
      const unsigned long long key = key_at(i);
      if (key != 0ull && (key >> (64 - pbits)) >= prefix) {
        const int at = atomicAdd(&Z.cnt, 1);
        if (at < P) Z.key[at] = key;
      }
    }
  }
  __syncthreads();
  gs_sort_desc(Z.key, P);
}

// ---- top-k per (user, group) -----------------------------------------------------------------------------------------
// k: the entries written per (user, group) -- D.k, or min(D.k, max_per_group) for RAW.  Outputs: row u of D.scores /
// D.ids_out holds G lists of k side by side (ld_* >= G * k); RAW, keys_out [B, G, k].  A group without columns writes its k
// padded entries like any other.  The segment bounds are clamped to [0, n]: a damaged offsets table cannot lead a read
// outside the logit row.
template <class Desc, bool RAW>
__global__ __launch_bounds__(GS_THREADS) void rg_select_kernel(Desc D, const float* __restrict__ logits, int ld_s,
                                                               GroupedItems map, const int32_t* __restrict__ offsets,
                                                               int k, unsigned long long* __restrict__ keys_out) {
  __shared__ GsLds Z;
  const int tid = threadIdx.x, u = blockIdx.x, g = blockIdx.y, G = gridDim.y;
  const int lo = min(max(offsets[g], 0), map.n), hi = min(max(offsets[g + 1], lo), map.n);
  const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
  gs_topk(
      [&](int i) -> unsigned long long {
        const unsigned o = rc::order_bits(row[lo + i]);
        return o ? rc::order_key(o, (unsigned)(lo + i)) : 0ull;  // (order bits 0: the exclusion sentinel)
      },
      hi - lo, k, Z);
  if (tid < k) {
    const unsigned long long key = Z.key[tid];
    const int id = key ? map.order[rc::key_id(key)] : 0;
    if constexpr (RAW) {
      keys_out[((size_t)u * G + g) * k + tid] = key ? rc::order_key((unsigned)(key >> 32), (unsigned)id) : 0ull;
    } else {
      const float score = key ? rc::link(rc::unorder_bits((unsigned)(key >> 32)), D.decoder) : 0.f;
      D.scores[(size_t)u * D.ld_scores + (size_t)g * k + tid] = score;
      D.ids_out[(size_t)u * D.ld_ids_out + (size_t)g * k + tid] = (int64_t)id;
    }
  }
}

// ---- the capped list: the D.k largest of a user's n id keys -----------------------------------------------------------
template <class Desc>
__global__ __launch_bounds__(GS_THREADS) void rg_merge_kernel(Desc D, const unsigned long long* __restrict__ keys, int n) {
  __shared__ GsLds Z;
  const int tid = threadIdx.x, u = blockIdx.x;
  const unsigned long long* row = keys + (size_t)u * n;
  gs_topk([&](int i) -> unsigned long long { return row[i]; }, n, D.k, Z);
  if (tid < D.k) {
    const unsigned long long key = Z.key[tid];
    D.scores[(size_t)u * D.ld_scores + tid] = key ? rc::link(rc::unorder_bits((unsigned)(key >> 32)), D.decoder) : 0.f;
    D.ids_out[(size_t)u * D.ld_ids_out + tid] = key ? (int64_t)rc::key_id(key) : 0;
  }
}

}  // namespace rc
