// Gumbel top-k sampling with logged propensities (include/carca_hip.h: carca_recommend_sampled /
// carca_knn_recommend_sampled), behind the scoring and exclusion launches of carca_recommend /
// carca_knn_recommend: k items drawn WITHOUT replacement from softmax(logit / tau) over a user's eligible items -- a
// Plackett-Luce list -- as the k largest of z + g, z = logit / tau and g iid standard Gumbel (the Gumbel-top-k identity).
//   sp_perturb_kernel  grid (B, S): streams a user's row of the [B, n] raw-logit buffer once, writes z + g into a second
//                      [B, n] buffer (the exclusion sentinel copied through as the sentinel) and one (max z, sum exp(z -
//                      max)) partial per CHUNK of SP_CHUNK columns to [B, n_chunks] of stream scratch.  The raw buffer is
//                      only read: the finishing launch needs its bits;
//   rc::ds_select      deep_select.h as it stands, over the perturbed buffer: ids, and scores the next launch overwrites;
//   sp_finish_kernel   grid (B): merges the user's partials into logsumexp(z), finds each selected id's column, reads its
//                      RAW logit and writes scores = link(raw), log_probs = raw / tau - lse, padding (0, -inf).
// The noise is a function of (seed, user key, ITEM ID) alone -- never of the column, the batch row or the launch shape --
// so a user's draw does not depend on the batch it sits in, and under a candidate list it is the unrestricted draw with
// the other items struck out.  The hash, exactly (every variable a 32-bit unsigned, arithmetic mod 2^32; mix32 is
// batch_build.hip's finaliser, restated below):
//   hu = mix32( seed_lo ^ (key_lo * 0x9E3779B1) )
//   hu = mix32( hu ^ seed_hi ^ (key_hi * 0x85EBCA77) )          seed, key: 64 bits, _lo = bits 0..31, _hi = bits 32..63
//   h  = mix32( hu ^ (item * 0xC2B2AE3D) )
//   U  = ((h >> 9) + 0.5) * 2^-23                               23 hash bits reach U; U is exact in fp32
//   g  = -log(-log(U))
// U lies in [2^-24, 1 - 2^-24], strictly inside (0, 1) for every h, so g is finite for every element:
// g_min = -log(24 log 2) = -2.8116, g_max = -log(-log(1 - 2^-24)) = 16.6355.  A perturbed key is clamped to the finite
// fp32 range, so it never carries the sentinel's bits (a NaN pattern) whatever the logit and the temperature.
// The logsumexp does not depend on S, on the row's alignment or on which lane read which column: chunks are fixed ranges
// of row columns, a chunk's maximum is exact in any order, and its sum runs in 64-bit fixed point (each exp(z - max) in
// units of 2^-32: integer addition is associative); sp_finish_kernel merges the chunk partials in a fixed shape.
// No atomics at all; nothing depends on scheduling.
#pragma once
#include <cfloat>
#include <cmath>

#include "deep_select.h"

namespace rc {

constexpr int SP_THREADS = 256;                 // both kernels' workgroup
constexpr int SP_WAVES = SP_THREADS / 64;
constexpr int SP_VECS = 4;                      // 16-byte vectors per lane and chunk
constexpr int SP_CHUNK = 64 * 4 * SP_VECS;      // columns per chunk: one wave, one partial
constexpr int SP_PARTS_MAX = 1024;              // most parts a row is split into

// ---- the noise -------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ unsigned sp_mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ unsigned sp_user_hash(unsigned long long seed, unsigned long long key) {
  const unsigned h = sp_mix32((unsigned)seed ^ ((unsigned)key * 0x9E3779B1u));
  return sp_mix32(h ^ (unsigned)(seed >> 32) ^ ((unsigned)(key >> 32) * 0x85EBCA77u));
}
__host__ __device__ __forceinline__ unsigned sp_item_hash(unsigned hu, unsigned item) {
  return sp_mix32(hu ^ (item * 0xC2B2AE3Du));
}
__host__ __device__ __forceinline__ float sp_uniform(unsigned h) { return ((float)(h >> 9) + 0.5f) * 0x1p-23f; }
// the inner log is the accurate one (U up to 1 - 2^-24: its relative error is g's absolute error); the outer argument
// lies in [6e-8, 16.7], where the fast log's error stays below 2e-6 absolute
__device__ __forceinline__ float sp_gumbel(unsigned h) { return -__logf(-logf(sp_uniform(h))); }

struct SpKeepAll {
  __device__ __forceinline__ bool operator()(int) const { return true; }
};
// a candidate list over a buffer whose columns are item ids (carca_knn_recommend_sampled): items outside it are struck out
struct SpKeepListed {
  ListedItems list;
  __device__ __forceinline__ bool operator()(int id) const { return list.find(id) >= 0; }
};

struct SpNoise {
  float tau;
  unsigned long long seed;
  const int64_t* user_keys;  // [B], or null: user u's key is u
};

__device__ __forceinline__ unsigned long long sp_wave_sum(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- one chunk of a user's row: what the perturb pass and the reduce pass of policy_items.h share ---------------------
// A chunk is read as 16-byte vectors aligned in MEMORY (row starts are u * ld_s floats: any residue mod 4), so a chunk that
// does not start on a 16-byte boundary has a partial vector at either end, handled by dword accesses.  The two passes
// share z's definition (sp_z) and the whole reduction (sp_chunk_sums), so their (max z, sum exp(z - max)) partials are
// the same code over the same values -- z is one correctly rounded division, a maximum is exact in any order -- and
// carry the same bits by construction.  The load loop with its two eligibility tests stands twice, here with the
// perturbed store in it and in pl_reduce_kernel without: one template over both took sp_perturb_kernel<AllItems,
// SpKeepAll> from 49 to 84 VGPRs, a shared per-column eligibility function still to 71 (DESIGN.md
// section 28).

// z of a column whose bits are `raw`: one fp32 division
__device__ __forceinline__ float sp_z(unsigned raw, float tau) { return __uint_as_float(raw) / tau; }

// The chunk's sums over the wave, in units of 2^-32 and 64-bit integers (integer addition is associative: no sum depends
// on which lane read which column).  acc: sum exp(z - mx), each term exp2((z - mx) log2(e) + 32), at most 2^32 (saturated
// one unit below).  ENTROPY: also ent = sum exp(z - mx) (mx - z), each term that same exp2 value times (mx - z) -- at
// most 2^32 / e, since x exp(-x) <= 1 / e -- truncated to an integer.
template <bool ENTROPY>
__device__ __forceinline__ void sp_chunk_sums(const float (&z)[SP_VECS + 1][4], float mx, unsigned long long& acc,
                                              unsigned long long& ent) {
  acc = 0ull, ent = 0ull;
  if (mx > -INFINITY) {
#pragma unroll
    for (int r = 0; r <= SP_VECS; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = fminf(exp2f(fmaf(z[r][e] - mx, 1.4426950408889634f, 32.f)), 4294967040.f);  // (z = -inf: 0)
        acc += (unsigned long long)(unsigned)t;
        if constexpr (ENTROPY) ent += (unsigned long long)(unsigned)(t > 0.f ? t * (mx - z[r][e]) : 0.f);
      }
  }
  acc = sp_wave_sum(acc);
  if constexpr (ENTROPY) ent = sp_wave_sum(ent);
}

// ---- 1. the perturb pass --------------------------------------------------------------------------------------------
// grid (B, S): part p of user u owns chunks [p nc / S, (p + 1) nc / S) of the row, wave w of the workgroup every
// SP_WAVES-th of them; logits and pert are 16-byte aligned and share ld_s (the host side checks).  Offsets are size_t.
template <class Map, class Keep>
__global__ __launch_bounds__(SP_THREADS) void sp_perturb_kernel(const float* __restrict__ logits, float* __restrict__ pert,
                                                                int ld_s, int n_items, Map map, Keep keep, SpNoise N,
                                                                int n_chunks, float2* __restrict__ part) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int u = blockIdx.x, p = blockIdx.y, S = gridDim.y;
  const auto m = map.for_user(u);
  const int n = m.size(n_items);
  const unsigned hu = sp_user_hash(N.seed, (unsigned long long)(N.user_keys ? N.user_keys[u] : (int64_t)u));
  const unsigned* src = reinterpret_cast<const unsigned*>(logits) + (size_t)u * (size_t)ld_s;
  unsigned* dst = reinterpret_cast<unsigned*>(pert) + (size_t)u * (size_t)ld_s;
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
      const bool full = col0 >= c0 && col0 + 4 <= c1;
      unsigned raw[4], out[4];
      if (full) {
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
        const int col = col0 + e;
        out[e] = RC_SENTINEL;
        if (raw[e] == RC_SENTINEL) continue;  // excluded, or outside the chunk
        const int item = m.item(col);
        if (!keep(item)) continue;
        const float zz = sp_z(raw[e], N.tau);
        z[r][e] = zz;
        const float key = fminf(fmaxf(zz + sp_gumbel(sp_item_hash(hu, (unsigned)item)), -3.402823466e38f), 3.402823466e38f);
        out[e] = __float_as_uint(key);
        mx = fmaxf(mx, zz);
      }
      if (full) {
        *reinterpret_cast<uint4*>(dst + col0) = make_uint4(out[0], out[1], out[2], out[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int col = col0 + e;
          if (col >= c0 && col < c1) dst[col] = out[e];
        }
      }
    }
    mx = wave_max(mx);
    unsigned long long acc, ent;
    sp_chunk_sums<false>(z, mx, acc, ent);
    if (lane == 0) part[(size_t)u * (size_t)n_chunks + c] = make_float2(mx, (float)acc * 0x1p-32f);
  }
}

// (m, s) += (pm, ps): the running maximum and the sum of exp(. - maximum); an empty side has s = 0
__device__ __forceinline__ void sp_merge(float& m, float& s, float pm, float ps) {
  if (ps == 0.f) return;
  if (s == 0.f) {
    m = pm, s = ps;
    return;
  }
  const float M = fmaxf(m, pm);
  s = s * expf(m - M) + ps * expf(pm - M);
  m = M;
}

// ---- 3. the finishing launch ------------------------------------------------------------------------------------------
// grid (B).  The partials merge in a shape that depends on n_chunks alone: thread t folds chunks t, t + 256, ... in index
// order, then a fixed tree over the 256 threads.  D.ids_out holds ds_select's ids: a nonzero id is an eligible item of
// the map, so find gives its column.
template <class Desc, class Map>
__global__ __launch_bounds__(SP_THREADS) void sp_finish_kernel(Desc D, const float* __restrict__ logits, int ld_s, Map map,
                                                               float tau, const float2* __restrict__ part, int n_chunks,
                                                               float* __restrict__ log_probs, int ld_log_probs) {
  __shared__ float sm[SP_THREADS], ss[SP_THREADS];
  const int tid = threadIdx.x, u = blockIdx.x;
  float m = -INFINITY, s = 0.f;
  for (int c = tid; c < n_chunks; c += SP_THREADS) {
    const float2 q = part[(size_t)u * (size_t)n_chunks + c];
    sp_merge(m, s, q.x, q.y);
  }
  sm[tid] = m, ss[tid] = s;
  __syncthreads();
  for (int stride = SP_THREADS / 2; stride > 0; stride >>= 1) {
    if (tid < stride) {
      sp_merge(m, s, sm[tid + stride], ss[tid + stride]);
      sm[tid] = m, ss[tid] = s;
    }
    __syncthreads();
  }
  const float lse = sm[0] + logf(ss[0]);  // (no eligible item: no id is nonzero either)
  const auto mp = map.for_user(u);
  const float* row = logits + (size_t)u * (size_t)ld_s;
  for (int j = tid; j < D.k; j += SP_THREADS) {
    const long long id = D.ids_out[(size_t)u * D.ld_ids_out + j];
    float score = 0.f, lp = -INFINITY;
    if (id > 0 && id < D.n_items) {
      const int col = mp.find((int)id);
      if (col >= 0 && col < ld_s) {
        const float raw = row[col];
        score = rc::link(raw, D.decoder);
        lp = raw / tau - lse;
      }
    }
    D.scores[(size_t)u * D.ld_scores + j] = score;
    log_probs[(size_t)u * (size_t)ld_log_probs + j] = lp;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
inline int sp_check(const CarcaSampling* X, int k, const char* what) {
  CARCA_CHECK_ARG(X, "%s: null sampling block", what);
  // (a denormal temperature would take z = logit / temperature to +-inf, and z - max to NaN)
  CARCA_CHECK_ARG(std::isfinite(X->temperature) && X->temperature >= FLT_MIN,
                  "%s: temperature must be finite and positive, a normal fp32 number", what);
  CARCA_CHECK_ARG(X->log_probs, "%s: null pointer", what);
  CARCA_CHECK_ARG(X->ld_log_probs >= k, "%s: row stride shorter than its row", what);
  return CARCA_OK;
}

// Parts per user of the perturb pass: about eight workgroups per CU, no part under one chunk per wave.  Tuning key 24
// (CARCA_TUNE_RETRIEVE_PARTS) > 0 forces this split as it forces the selection's; no choice changes a bit of the result.
inline int sp_parts(int B, int n_chunks) {
  const int forced = carca_tuning(CARCA_TUNE_RETRIEVE_PARTS);
  long long S = forced > 0 ? forced : (8ll * carca_num_cus() + B - 1) / B;
  S = std::min<long long>(S, (n_chunks + SP_WAVES - 1) / SP_WAVES);
  return (int)std::max<long long>(1, std::min<long long>(S, SP_PARTS_MAX));
}

// The three steps over the [B, n_slots] raw logits (row stride ld_s >= n_slots; the perturbed buffer takes the same
// stride, so a row's alignment is the same in both) that the caller's scoring and exclusion launches have queued on
// `stream`.  D: the caller's descriptor or an rc::SelectView, 1 <= D.k <= DS_KMAX checked; map:
// what a column holds; keep: a further filter on the item (SpKeepAll, or SpKeepListed over an AllItems buffer).
template <class Desc, class Map, class Keep>
int sp_run(const Desc& D, int B, const float* logits, int ld_s, int n_slots, Map map, Keep keep, const CarcaSampling& X,
           const char* what, hipStream_t stream) {
  CARCA_CHECK_ARG(ld_s >= n_slots, "%s: logit row stride shorter than its row", what);
  const int n_chunks = (n_slots + SP_CHUNK - 1) / SP_CHUNK;
  const size_t pert_bytes = (std::max((size_t)B * (size_t)ld_s, (size_t)1) * sizeof(float) + 255) / 256 * 256;
  const size_t part_bytes = std::max((size_t)B * (size_t)n_chunks, (size_t)1) * sizeof(float2);
  char* base = (char*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, pert_bytes + part_bytes, false, nullptr)
                                                      : carca_stream_scratch(stream, CARCA_SCRATCH_SAMPLED, pert_bytes + part_bytes));
  CARCA_CHECK_ARG(base, "%s: scratch allocation of %zu bytes failed", what, pert_bytes + part_bytes);
  float* pert = (float*)base;
  float2* part = (float2*)(base + pert_bytes);
  CARCA_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(pert) & 15) == 0,
                  "%s: logit buffers must be 16-byte aligned", what);
  const SpNoise N = {X.temperature, (unsigned long long)X.seed, X.user_keys};
  if (n_chunks > 0) {
    hipLaunchKernelGGL((sp_perturb_kernel<Map, Keep>), dim3(B, sp_parts(B, n_chunks)), dim3(SP_THREADS), 0, stream, logits,
                       pert, ld_s, D.n_items, map, keep, N, n_chunks, part);
    CARCA_LAUNCH_CHECK();
  }
  if (int rc = ds_select(D, B, pert, ld_s, n_slots, map, what, stream)) return rc;
  hipLaunchKernelGGL((sp_finish_kernel<Desc, Map>), dim3(B), dim3(SP_THREADS), 0, stream, D, logits, ld_s, map,
                     X.temperature, (const float2*)part, n_chunks, X.log_probs, X.ld_log_probs);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace rc
