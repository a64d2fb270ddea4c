// The selection launches of the deep top-k calls (include/carca_hip.h: carca_retrieve / carca_retrieve_among /
// carca_knn_retrieve), behind the scoring and exclusion launches of carca_recommend /
// carca_knn_recommend: the k best columns of a user's row of the [B, n] raw-logit buffer for k up to DS_KMAX = 4096, in
// rc_select_kernel's order (keys rc::order_key(order bits, column): logit descending, ties to the smaller column).
//   ds_part_kernel   grid (B, S): part p of user u owns columns [p n / S, (p + 1) n / S) of the row and writes the keys of
//                    its kp = min(k, ceil(n / S)) best eligible columns to a [B, S, kp] key buffer, 0 for a hole (stage 1).
//                    A key carries the column of the WHOLE row, so keys are distinct across parts;
//   ds_merge_kernel  grid (B): the k largest of the user's S * kp keys -- or, S = 1 (no stage 1), of the keys of the row
//                    itself -- sorted, linked, mapped to ids and written with the padding (stage 2).
// The k largest keys of a row are among the union of every part's kp largest, and keys are distinct, so the result is
// the same set in the same order for every S: rc_select_kernel's for k <= 128.
// Both run ds_topk, group_select.h's gs_topk with a key block of DS_KMAX keys: up to DS_KMAX columns are read once and
// sorted in LDS; more run the MSB-first radix select and sort the survivors.  Integer LDS atomics only (histogram, slot
// counter); no float atomics; nothing depends on scheduling.
#pragma once
#include "group_select.h"

namespace rc {

constexpr int DS_THREADS = GS_THREADS;  // selection workgroup (== the radix histogram's bins; gs_sort_desc strides by it)
constexpr int DS_KMAX = 4096;           // largest k, and the key block (32 KiB of LDS)
constexpr int DS_PARTS_MAX = 64;        // most parts a row is split into
constexpr size_t DS_MAX_KEY_BYTES = (size_t)1 << 30;  // the [B, S, kp] key scratch; beyond it S is lowered
static_assert((DS_KMAX & (DS_KMAX - 1)) == 0 && DS_KMAX >= 2 * DS_THREADS, "gs_sort_desc sorts a power of two");

struct DsLds {
  unsigned long long key[DS_KMAX];
  int hist[256];
  unsigned long long prefix;
  int pbits, need, done, keff, cnt;
};

// gs_topk over the larger block: leaves the k largest of the keys key_at(0 .. n - 1) in Z.key[0 .. k), descending,
// followed by zeros where fewer than k are non-zero.  key_at(i) is column i's key, 0 where the column is not eligible;
// non-zero keys are distinct.  Whole workgroup of DS_THREADS threads; n >= 0 and k (1 <= k <= DS_KMAX) are
// workgroup-uniform; Z is not in use.  Ends with a barrier.
template <class KeyAt>
__device__ __forceinline__ void ds_topk(KeyAt key_at, int n, int k, DsLds& Z) {
  const int tid = threadIdx.x;
  if (n <= DS_KMAX) {  // one read of the columns, sorted whole
    int P = 2;
    while (P < n) P <<= 1;
    const int fill = max(P, k);  // (<= DS_KMAX: P <= DS_KMAX as n is, k by the caller's check)
    for (int i = tid; i < fill; i += DS_THREADS) Z.key[i] = i < n ? key_at(i) : 0ull;
    __syncthreads();
    gs_sort_desc(Z.key, P);
    return;
  }
  // rc_select_kernel's radix select: a byte of the key per pass, from the top, until the k-th largest key's prefix is known
  if (tid == 0) Z.prefix = 0ull, Z.pbits = 0, Z.done = 0, Z.cnt = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    Z.hist[tid] = 0;  // (DS_THREADS == 256 bins)
    __syncthreads();
    const unsigned long long prefix = Z.prefix;
    const int pbits = Z.pbits;
    for (int i = tid; i < n; i += DS_THREADS) {
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
  for (int i = tid; i < P; i += DS_THREADS) Z.key[i] = 0ull;  // (P <= DS_KMAX)
  __syncthreads();
  if (keff > 0) {
    const unsigned long long prefix = Z.prefix;
    const int pbits = Z.pbits;
    for (int i = tid; i < n; i += DS_THREADS) {
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

// column i's key of a raw-logit row (order bits 0: the exclusion sentinel)
__device__ __forceinline__ unsigned long long ds_row_key(const unsigned* row, int i) {
  const unsigned o = rc::order_bits(row[i]);
  return o ? rc::order_key(o, (unsigned)i) : 0ull;
}

// ---- stage 1: the kp best keys of every part of a row -----------------------------------------------------------------
// grid (B, S), S >= 2; kp = min(D.k, ceil(n / S)) >= the longest part's length capped at k; keys_out [B, S, kp]
template <class Desc, class Map>
__global__ __launch_bounds__(DS_THREADS) void ds_part_kernel(Desc D, const float* __restrict__ logits, int ld_s, Map map,
                                                             int kp, unsigned long long* __restrict__ keys_out) {
  __shared__ DsLds Z;
  const int tid = threadIdx.x, u = blockIdx.x, p = blockIdx.y, S = gridDim.y;
  const int n = map.for_user(u).size(D.n_items);
  const int lo = (int)((long long)p * n / S), hi = (int)((long long)(p + 1) * n / S);
  const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
  ds_topk([&](int i) -> unsigned long long { return ds_row_key(row, lo + i); }, hi - lo, kp, Z);
  unsigned long long* out = keys_out + ((size_t)u * S + p) * kp;
  for (int j = tid; j < kp; j += DS_THREADS) out[j] = Z.key[j];
}

// ---- stage 2: the D.k largest keys of a user, linked and written -------------------------------------------------------
// keys: the [B, n_keys] buffer of stage 1, or null: the keys of the logit row itself (S = 1)
template <class Desc, class Map>
__global__ __launch_bounds__(DS_THREADS) void ds_merge_kernel(Desc D, const float* __restrict__ logits, int ld_s, Map map,
                                                              const unsigned long long* __restrict__ keys, int n_keys) {
  __shared__ DsLds Z;
  const int tid = threadIdx.x, u = blockIdx.x;
  const auto m = map.for_user(u);
  if (keys) {
    const unsigned long long* krow = keys + (size_t)u * n_keys;
    ds_topk([&](int i) -> unsigned long long { return krow[i]; }, n_keys, D.k, Z);
  } else {
    const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
    ds_topk([&](int i) -> unsigned long long { return ds_row_key(row, i); }, m.size(D.n_items), D.k, Z);
  }
  for (int j = tid; j < D.k; j += DS_THREADS) {
    const unsigned long long key = Z.key[j];
    float score = 0.f;
    long long id = 0;
    if (key) {
      id = (long long)m.item((int)rc::key_id(key));
      score = rc::link(rc::unorder_bits((unsigned)(key >> 32)), D.decoder);
    }
    D.scores[(size_t)u * D.ld_scores + j] = score;
    D.ids_out[(size_t)u * D.ld_ids_out + j] = id;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// Parts per user for B rows of n_slots columns.  Tuning key 24 (CARCA_TUNE_RETRIEVE_PARTS) > 0 forces the count; 0 is the
// shipped choice: one part while a row is short or the users alone give every CU two workgroups, otherwise enough parts
// for eight workgroups per CU, none shorter than 16384 columns (TUNING.md round 33: at 1 M columns and 128 users 16 parts
// beat 4 and 64, at 12,102 columns every split loses to one part).  Clamped to [1, DS_PARTS_MAX] and to the row length,
// then lowered while the key scratch would pass DS_MAX_KEY_BYTES.
inline int ds_parts(int B, int n_slots, int k) {
  const int forced = carca_tuning(CARCA_TUNE_RETRIEVE_PARTS);
  const long long cus = carca_num_cus();
  long long S = 1;
  if (forced > 0) {
    S = forced;
  } else if (n_slots > 32768 && B < 2 * cus) {
    S = std::min<long long>((n_slots + 16383) / 16384, (8 * cus + B - 1) / B);
  }
  S = std::max<long long>(1, std::min<long long>(S, std::min(DS_PARTS_MAX, n_slots)));
  while (S > 1 && (size_t)B * (size_t)S * (size_t)std::min<long long>(k, (n_slots + S - 1) / S) * 8 > DS_MAX_KEY_BYTES) --S;
  return (int)S;
}

// The selection of a deep top-k over the [B, n_slots] raw logits (row stride ld_s) that the caller's scoring and exclusion
// launches have queued on `stream`.  D: the caller's descriptor or an rc::SelectView (which carries no B), 1 <= D.k <=
// DS_KMAX checked.
template <class Desc, class Map>
int ds_select(const Desc& D, int B, const float* logits, int ld_s, int n_slots, Map map, const char* what,
              hipStream_t stream) {
  const int S = ds_parts(B, n_slots, D.k);
  unsigned long long* keys = nullptr;
  int kp = 0;
  if (S > 1) {
    kp = std::min(D.k, (n_slots + S - 1) / S);
    const size_t bytes = (size_t)B * (size_t)S * (size_t)kp * sizeof(unsigned long long);
    keys = (unsigned long long*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                                : carca_stream_scratch(stream, CARCA_SCRATCH_RETRIEVE, bytes));
    CARCA_CHECK_ARG(keys, "%s: scratch allocation of %zu bytes failed", what, bytes);
    hipLaunchKernelGGL((ds_part_kernel<Desc, Map>), dim3(B, S), dim3(DS_THREADS), 0, stream, D, logits, ld_s, map, kp,
                       keys);
    CARCA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((ds_merge_kernel<Desc, Map>), dim3(B), dim3(DS_THREADS), 0, stream, D, logits, ld_s, map,
                     (const unsigned long long*)keys, S * kp);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace rc
