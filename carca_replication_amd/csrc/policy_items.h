// A sampling policy's log-probabilities for listed items (include/carca_hip.h: carca_log_prob_items /
// carca_knn_log_prob_items): log pi(item | user) under softmax(logit / tau) over the user's eligible
// items -- the numerator of an IPS / SNIPS estimator whose denominator carca_recommend_sampled logged -- with the per-user
// logsumexp and entropy of that softmax from the same pass.  Behind the scoring and exclusion launches of carca_recommend
// / carca_knn_recommend:
//   pl_reduce_kernel  grid (B, S): sp_perturb_kernel's read side and nothing else (sampled_select.h: sp_z,
//                     sp_chunk_sums -- the same code, so the same bits): streams a user's row of the [B, n] raw-logit
//                     buffer once and writes, per CHUNK of SP_CHUNK columns, (max z, sum exp(z - max), sum exp(z - max)
//                     (max - z)) to [B, n_chunks, 3] of stream scratch.  No hash, no logs, no second buffer;
//   pl_finish_kernel  grid (B): merges the (max, sum) partials with sp_merge in sp_finish_kernel's shape -- lse carries that
//                     kernel's bits -- and the entropy partial alongside, then looks every listed id up: raw / tau - lse
//                     where the id is eligible, -inf exactly elsewhere.
// Nothing depends on S, on a row's alignment, on which lane read which column, on the batch or on the list's order: the
// chunk sums run in 64-bit fixed point, the merge shape depends on n_chunks alone, a list entry is a lookup.  No atomics, no
// LDS in the reduce pass.
#pragma once
#include "sampled_select.h"

namespace rc {

constexpr int PL_PART = 3;  // floats per chunk partial: max z, sum exp(z - max), sum exp(z - max) (max - z)

// ---- 1. the reduce pass ----------------------------------------------------------------------------------------------
// grid (B, S): chunk ownership and the loads are sp_perturb_kernel's -- part p of user u owns chunks [p nc / S,
// (p + 1) nc / S), wave w every SP_WAVES-th of them, read as 16-byte vectors aligned in memory with dword accesses at the
// ends of a shifted chunk.  logits is 16-byte aligned (the host side checks).  Offsets are size_t.
template <class Map, class Keep>
__global__ __launch_bounds__(SP_THREADS) void pl_reduce_kernel(const float* __restrict__ logits, int ld_s, int n_items, Map map,
                                                               Keep keep, float tau, int n_chunks, float* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int u = blockIdx.x, p = blockIdx.y, S = gridDim.y;
  const auto m = map.for_user(u);
  const int n = m.size(n_items);
  const unsigned* src = reinterpret_cast<const unsigned*>(logits) + (size_t)u * (size_t)ld_s;
  const int c_lo = (int)((long long)p * n_chunks / S), c_hi = (int)((long long)(p + 1) * n_chunks / S);
  for (int c = c_lo + w; c < c_hi; c += SP_WAVES) {
    const int c0 = c * SP_CHUNK, c1 = min(n, c0 + SP_CHUNK);
    const int shift = (int)((reinterpret_cast<uintptr_t>(src + c0) >> 2) & 3);  // floats past a 16-byte boundary
    float z[SP_VECS + 1][4];
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r <= SP_VECS; ++r) {  // (round SP_VECS: the one vector a shifted chunk spills into, lane 0's)
      const int col0 = c0 - shift + 4 * (lane + 64 * r);
#pragma unroll
      for (int e = 0; e < 4; ++e) z[r][e] = -INFINITY;
      if (col0 >= c1) continue;
      unsigned raw[4];
      if (col0 >= c0 && col0 + 4 <= c1) {
        const uint4 v = *reinterpret_cast<const uint4*>(src + col0);
        raw[0] = v.x, raw[1] = v.y, raw[2] = v.z, raw[3] = v.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = col0 + e;
          raw[e] = (col >= c0 && col < c1) ? src[col] : RC_SENTINEL;
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (raw[e] == RC_SENTINEL) continue;  // excluded, or outside the chunk
        if (!keep(m.item(col0 + e))) continue;
        const float zz = sp_z(raw[e], tau);
        z[r][e] = zz;
        mx = fmaxf(mx, zz);
      }
    }
    mx = wave_max(mx);
    unsigned long long acc, ent;
    sp_chunk_sums<true>(z, mx, acc, ent);
    if (lane == 0) {
      float* q = part + ((size_t)u * (size_t)n_chunks + (size_t)c) * PL_PART;
      q[0] = mx, q[1] = (float)acc * 0x1p-32f, q[2] = (float)ent * 0x1p-32f;
    }
  }
}

// (m, s, w) += (pm, ps, pw): sp_merge with the entropy partial w = sum exp(. - maximum) (maximum - .) carried alongside.
// Moving a side's reference from its own maximum m to M multiplies every term by e^(m - M) and adds (M - m) to its second
// factor: w' = (w + s (M - m)) e^(m - M).  (m, s) go through sp_merge itself, after w has read them.
__device__ __forceinline__ void pl_merge(float& m, float& s, float& w, float pm, float ps, float pw) {
  if (ps != 0.f) {
    if (s == 0.f) {
      w = pw;
    } else {
      const float M = fmaxf(m, pm);
      w = (w + s * (M - m)) * expf(m - M) + (pw + ps * (M - pm)) * expf(pm - M);
    }
  }
  sp_merge(m, s, pm, ps);
}

struct PlOut {
  float tau;
  const int64_t* items;  // [B, ld_items]: n_list entries per user, any int64
  int n_list, ld_items;
  float* log_probs;      // [B, ld_log_probs]
  int ld_log_probs;
  float* lse;            // [B] or null
  float* entropy;        // [B] or null
};

// ---- 2. the finishing launch ------------------------------------------------------------------------------------------
// grid (B).  The merge is sp_finish_kernel's: thread t folds chunks t, t + 256, ... in index order, then a fixed tree over
// the 256 threads.  Thread t then takes list entries t, t + 256, ...: the range check on the int64 id (a large id never
// wraps into range), the id's column, keep, and the sentinel test on the raw buffer -- a caller's list may name an
// excluded item, which the selection's ids never did.  n_slots: the columns of a row that hold logits.  The kernel reads
// n_items of the caller's descriptor and nothing else, so it takes that int and not the descriptor.
template <class Map, class Keep>
__global__ __launch_bounds__(SP_THREADS) void pl_finish_kernel(int n_items, const float* __restrict__ logits, int ld_s,
                                                               int n_slots, Map map, Keep keep, const float* __restrict__ part,
                                                               int n_chunks, PlOut X) {
  __shared__ float sm[SP_THREADS], ss[SP_THREADS], sw[SP_THREADS];
  const int tid = threadIdx.x, u = blockIdx.x;
  float m = -INFINITY, s = 0.f, w = 0.f;
  for (int c = tid; c < n_chunks; c += SP_THREADS) {
    const float* q = part + ((size_t)u * (size_t)n_chunks + (size_t)c) * PL_PART;
    pl_merge(m, s, w, q[0], q[1], q[2]);
  }
  sm[tid] = m, ss[tid] = s, sw[tid] = w;
  __syncthreads();
  for (int stride = SP_THREADS / 2; stride > 0; stride >>= 1) {
    if (tid < stride) {
      pl_merge(m, s, w, sm[tid + stride], ss[tid + stride], sw[tid + stride]);
      sm[tid] = m, ss[tid] = s, sw[tid] = w;
    }
    __syncthreads();
  }
  const float lse = sm[0] + logf(ss[0]);  // (no eligible item: -inf + -inf)
  if (tid == 0) {
    if (X.lse) X.lse[u] = lse;
    // (never below 0: a chunk's largest term saturates one unit under 2^32, so one dominant item gives s = 1 - 2^-24 and
    // log s = -6e-8 where the entropy is 1e-8)
    if (X.entropy) X.entropy[u] = ss[0] > 0.f ? fmaxf(logf(ss[0]) + sw[0] / ss[0], 0.f) : 0.f;
  }
  const auto mp = map.for_user(u);
  const unsigned* row = reinterpret_cast<const unsigned*>(logits) + (size_t)u * (size_t)ld_s;
  for (int j = tid; j < X.n_list; j += SP_THREADS) {
    const long long id = X.items[(size_t)u * (size_t)X.ld_items + j];
    float lp = -INFINITY;
    if (id > 0 && id < n_items) {
      const int col = mp.find((int)id);
      if (col >= 0 && col < n_slots && keep((int)id)) {
        const unsigned raw = row[col];
        if (raw != RC_SENTINEL) lp = __uint_as_float(raw) / X.tau - lse;
      }
    }
    X.log_probs[(size_t)u * (size_t)X.ld_log_probs + j] = lp;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
inline int pl_check(const CarcaPolicyItems* X, const char* what) {
  CARCA_CHECK_ARG(X, "%s: null policy block", what);
  // (a denormal temperature would take z = logit / temperature to +-inf, and z - max to NaN)
  CARCA_CHECK_ARG(std::isfinite(X->temperature) && X->temperature >= FLT_MIN,
                  "%s: temperature must be finite and positive, a normal fp32 number", what);
  CARCA_CHECK_ARG(X->n_list >= 0, "%s: n_list must not be negative", what);
  CARCA_CHECK_ARG(X->n_list == 0 || (X->items && X->log_probs), "%s: null pointer", what);
  CARCA_CHECK_ARG(X->ld_items >= X->n_list && X->ld_log_probs >= X->n_list, "%s: row stride shorter than its row", what);
  return CARCA_OK;
}

// The two launches over the [B, n_slots] raw logits (row stride ld_s >= n_slots) that the caller's scoring and exclusion
// launches have queued on `stream`.  n_items: the catalogue's size; map: what a column holds; keep: a further filter on
// the item (SpKeepAll, or SpKeepListed over an AllItems buffer).  Scratch: 12 bytes per user and chunk.
template <class Map, class Keep>
int pl_run(int n_items, int B, const float* logits, int ld_s, int n_slots, Map map, Keep keep, const CarcaPolicyItems& X,
           const char* what, hipStream_t stream) {
  CARCA_CHECK_ARG(ld_s >= n_slots, "%s: logit row stride shorter than its row", what);
  const int n_chunks = (n_slots + SP_CHUNK - 1) / SP_CHUNK;
  const size_t part_bytes = std::max((size_t)B * (size_t)n_chunks, (size_t)1) * PL_PART * sizeof(float);
  float* part = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, part_bytes, false, nullptr)
                                                        : carca_stream_scratch(stream, CARCA_SCRATCH_POLICY, part_bytes));
  CARCA_CHECK_ARG(part, "%s: scratch allocation of %zu bytes failed", what, part_bytes);
  CARCA_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "%s: the logit buffer must be 16-byte aligned", what);
  if (n_chunks > 0) {
    hipLaunchKernelGGL((pl_reduce_kernel<Map, Keep>), dim3(B, sp_parts(B, n_chunks)), dim3(SP_THREADS), 0, stream, logits,
                       ld_s, n_items, map, keep, X.temperature, n_chunks, part);
    CARCA_LAUNCH_CHECK();
  }
  const PlOut O = {X.temperature, X.items, X.n_list, X.ld_items, X.log_probs, X.ld_log_probs, X.lse, X.entropy};
  hipLaunchKernelGGL((pl_finish_kernel<Map, Keep>), dim3(B), dim3(SP_THREADS), 0, stream, n_items, logits, ld_s, n_slots, map,
                     keep, (const float*)part, n_chunks, O);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace rc
