// Full-catalogue top-k and exact ranks for the KNN baseline (include/carca_hip.h: carca_knn_recommend,
// carca_knn_rank_items).
//
// The reference's KNN scores a (user, item) pair as the dot product of the last profile slot's attribute row with the
// item's attribute row (knn.py:13-19), so scoring the whole catalogue for B users is one GEMM, S = Q A^T, with
// Q [B, F] the users' query rows and A [n_items, F] the attribute table.  At C2 that is 128 x 12,102 x 4,096: a real GEMM,
// where CARCA's catalogue kernels (recommend_common.h) keep an item row of at most 128 floats in registers.
// Launches, no host wait, nothing retained:
//   1. query: the [Bp, ldq] query rows (Bp = B rounded up to the 64-user block), zero-padded, into stream scratch:
//      table[p_ids[u][L-1]] (a zero row for an id outside [0, n_items)), or the caller's dense rows;
//   2. scoring: a users x items GEMM into a [B, n_items] logit buffer.  Each 64-lane wave owns 16 items x 64 users,
//      its operands read straight from global memory with buffer loads (16 bytes per lane per step, the wave-uniform
//      base carrying the 64-bit row offset).  Two variants:
//        fp32: v_mfma_f32_16x16x4_f32, exact fp32 products; each output sums chains of 256 k (fmaf chains)
//              in fp32;
//        i8:   v_mfma_i32_16x16x64_i8 over an int8 copy of the table, i32 accumulation, converted once.  The caller
//              takes it only for tables whose entries are integers with max|x| <= 127 and max|x|^2 F < 2^24: every
//              partial sum is then an integer below 2^24, so the fp32 sum is exact too and the two agree bit for bit;
//   3. recommend: the exclusion and selection launches of carca_recommend (catalogue_select.h) with no link;
//      rank_items: the listed items' keys are read from the logit buffer, the exclusion launch overwrites excluded ids
//      with its sentinel, and a counting sweep adds, per (user, target), the items whose key is larger (ballot +
//      popcount per wave, one 64-bit integer atomic per workgroup and target: rc::count_larger, catalogue_sweep.h).
// Both calls take every logit from the same scoring launch, so the item at position r of recommend(k = 128) has rank r
// and the same score bits.  Integer atomics only: results do not depend on scheduling.
#include "catalogue_select.h"
#include "catalogue_sweep.h"

#include <type_traits>

namespace {

constexpr int KC_THREADS = 256;
constexpr int KC_WAVES = KC_THREADS / 64;
constexpr int KC_MU = 4;                  // 16-user blocks per wave
constexpr int KC_UB = 16 * KC_MU;         // users per workgroup (and the row padding of the query buffer)
constexpr int KC_IB = 16 * KC_WAVES;      // items per workgroup: 16 per wave
constexpr int KC_UNROLL = 4;              // 64-byte row chunks in flight per operand
constexpr int KC_FOLD = 16;               // fp32: chunks per MFMA chain (a multiple of KC_UNROLL)
constexpr int KC_CNT_PER_THREAD = 8;      // items per lane in the counting sweep
static_assert(KC_THREADS == rc::TILE, "rc::count_larger counts over a workgroup of rc::TILE threads");

typedef int i32x4 __attribute__((ext_vector_type(4)));

// buffer resource over `bytes` bytes from `base`: loads past the end return 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t kc_rsrc(const void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}

// the fields the exclusion / selection launches read (catalogue_select.h), with no link
struct KcSelect {
  int n_items, k;
  rc::IdentityLink decoder;
  const int32_t* exclude;
  int n_exclude, ld_exclude;
  float* scores;
  int ld_scores;
  int64_t* ids_out;
  int ld_ids_out;
};

// ---- 1. query rows ---------------------------------------------------------------------------------------------
struct KcQuery {
  int B, L, n_items, F, ldq;
  const int32_t* p_ids;
  int ld_p_ids;
  const float* user_a;  // dense rows, or NULL
  int64_t ld_user_a;
  const void* table;  // fp32 table, or its int8 copy (I8)
  int64_t ld_table;
  void* q;  // [Bp, ldq] fp32 or int8
};

template <bool I8>
__global__ __launch_bounds__(KC_THREADS) void kc_query_kernel(KcQuery A) {
  typedef typename std::conditional<I8, int8_t, float>::type T;
  const int u = blockIdx.x;
  const T* src = nullptr;
  if (u < A.B) {
    if (A.user_a) {
      src = reinterpret_cast<const T*>(A.user_a + (size_t)u * A.ld_user_a);
    } else {
      const int id = A.p_ids[(size_t)u * A.ld_p_ids + A.L - 1];
      if (id >= 0 && id < A.n_items) src = reinterpret_cast<const T*>(A.table) + (size_t)id * A.ld_table;
    }
  }
  T* dst = reinterpret_cast<T*>(A.q) + (size_t)u * A.ldq;
  for (int k = threadIdx.x; k < A.ldq; k += KC_THREADS) dst[k] = (src && k < A.F) ? src[k] : T(0);
}

// ---- 2. scoring --------------------------------------------------------------------------------------------------
struct KcScore {
  const void* table;  // fp32 [n_items, ld] (elements) or int8 [n_items, ld] (bytes)
  int ld;
  const void* q;  // [Bp, ldq], zero past F
  int ldq;
  int B, n_items, F;
  int nchunks;  // 64-byte chunks of a query row
  int nub;      // user blocks
  float* logits;
  int64_t ld_s;
};

// Operand chunk c of a row is its bytes 64c .. 64c + 63: lane (r = l & 15, g = l >> 4) holds bytes 64c + 16g .. +15 of
// user row r (A operand) and item row r (B operand).
template <bool I8, bool VEC>
__global__ __launch_bounds__(KC_THREADS) void kc_score_kernel(KcScore P) {
  constexpr int ES = I8 ? 1 : 4;
  typedef typename std::conditional<I8, i32x4, f32x4>::type V;
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int ub = blockIdx.x % P.nub, it = blockIdx.x / P.nub;
  const int u0 = ub * KC_UB, i0 = it * KC_IB + wave * 16;
  const int rows = max(0, min(16, P.n_items - i0));  // live item rows of this wave
  // wave-uniform bases carry the 64-bit row offsets; lane offsets stay below 16 rows
  const auto tr = kc_rsrc((const char*)P.table + (size_t)i0 * P.ld * ES, (unsigned)rows * P.ld * ES);
  const auto qr = kc_rsrc((const char*)P.q + (size_t)u0 * P.ldq * ES, (unsigned)KC_UB * P.ldq * ES);
  const int t_off = r * P.ld * ES + g * 16;
  int q_off[KC_MU];
#pragma unroll
  for (int m = 0; m < KC_MU; ++m) q_off[m] = (16 * m + r) * P.ldq * ES + g * 16;
  V acc[KC_MU];
#pragma unroll
  for (int m = 0; m < KC_MU; ++m) acc[m] = (V){0, 0, 0, 0};

  auto load_t = [&](int c) -> V {
    if constexpr (I8) {
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(tr, t_off, c * 64, 0);
      return (V){(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
    } else if constexpr (VEC) {  // F % 4 == 0: a lane's four k are all inside the row or all past it
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(tr, t_off, c * 64, 0);
      const bool in = 16 * c + 4 * g < P.F;
      return (V){in ? __uint_as_float(v[0]) : 0.f, in ? __uint_as_float(v[1]) : 0.f, in ? __uint_as_float(v[2]) : 0.f,
                 in ? __uint_as_float(v[3]) : 0.f};
    } else {
      V out;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * c + 4 * g + j;
        const float x = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(tr, r * P.ld * 4 + k * 4, 0, 0));
        out[j] = k < P.F ? x : 0.f;
      }
      return out;
    }
  };
  auto load_q = [&](int m, int c) -> V {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(qr, q_off[m], c * 64, 0);
    if constexpr (I8) {
      return (V){(int)v[0], (int)v[1], (int)v[2], (int)v[3]};
    } else {
      return (V){__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3])};
    }
  };
  auto mma = [&](V a, V b, V c) -> V {
    if constexpr (I8) {
      return __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, c, 0, 0, 0);
    } else {
      return mfma16_group(a, b, c);  // k = 16c + 4g + s at step s, the same permutation for both operands
    }
  };

  // fp32: the MFMA chain restarts every KC_FOLD chunks (256 k) and is added into `tot`, so an output's rounding error
  // grows with two short sums rather than one F-long fmaf chain (a 4,096-long chain of positive terms: ~2e-6 relative)
  V tot[KC_MU];
#pragma unroll
  for (int m = 0; m < KC_MU; ++m) tot[m] = (V){0, 0, 0, 0};
  auto fold = [&]() {
    if constexpr (!I8) {
#pragma unroll
      for (int m = 0; m < KC_MU; ++m) tot[m] += acc[m], acc[m] = (V){0, 0, 0, 0};
    }
  };
  int c = 0;
  for (; c + KC_UNROLL <= P.nchunks; c += KC_UNROLL) {
    V t[KC_UNROLL], q[KC_UNROLL][KC_MU];
#pragma unroll
    for (int j = 0; j < KC_UNROLL; ++j) {
      t[j] = load_t(c + j);
#pragma unroll
      for (int m = 0; m < KC_MU; ++m) q[j][m] = load_q(m, c + j);
    }
#pragma unroll
    for (int j = 0; j < KC_UNROLL; ++j)
#pragma unroll
      for (int m = 0; m < KC_MU; ++m) acc[m] = mma(q[j][m], t[j], acc[m]);
    if ((c + KC_UNROLL) % KC_FOLD == 0) fold();
  }
  for (; c < P.nchunks; ++c) {
    const V t = load_t(c);
#pragma unroll
    for (int m = 0; m < KC_MU; ++m) acc[m] = mma(load_q(m, c), t, acc[m]);
  }
  fold();
  if constexpr (I8) {
#pragma unroll
    for (int m = 0; m < KC_MU; ++m) tot[m] = acc[m];
  }
  // D: column (item) r, rows (users) 4g .. 4g + 3 of each 16-user block
  const int item = i0 + r;
  if (item < P.n_items) {
#pragma unroll
    for (int m = 0; m < KC_MU; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = u0 + 16 * m + 4 * g + j;
        if (u < P.B) P.logits[(size_t)u * P.ld_s + item] = (float)tot[m][j];
      }
  }
}

// ---- 3b. ranks: list keys, then a counting sweep -----------------------------------------------------------------
__global__ __launch_bounds__(rc::LIST_MAX) void kc_list_kernel(CarcaKnnRankDesc D, const float* __restrict__ logits,
                                                          int64_t ld_s, unsigned long long* __restrict__ tkeys) {
  const int u = blockIdx.x, j = threadIdx.x;
  if (j >= D.n_list) return;
  const int id = D.items[(size_t)u * D.ld_items + j];
  const bool valid = id >= 1 && id < D.n_items;
  const float logit = valid ? logits[(size_t)u * ld_s + id] : 0.f;
  tkeys[(size_t)u * D.n_list + j] = valid ? rc::item_key(logit, id) : rc::KEY_NEVER;
  D.scores[(size_t)u * D.ld_scores + j] = logit;
  D.ranks[(size_t)u * D.ld_ranks + j] = valid ? 0 : -1;  // the sweep adds to the valid ones only
}

__global__ __launch_bounds__(KC_THREADS) void kc_count_kernel(CarcaKnnRankDesc D, const float* __restrict__ logits,
                                                              int64_t ld_s, const unsigned long long* __restrict__ tkeys) {
  __shared__ rc::CountLds C;
  const int tid = threadIdx.x, u = blockIdx.y;
  for (int t = tid; t < D.n_list; t += KC_THREADS) C.tkey[t] = tkeys[(size_t)u * D.n_list + t];
  const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
  const long long base = (long long)blockIdx.x * KC_THREADS * KC_CNT_PER_THREAD;
  unsigned long long key[KC_CNT_PER_THREAD];
#pragma unroll
  for (int j = 0; j < KC_CNT_PER_THREAD; ++j) {  // excluded ids and id 0 hold the sentinel, whose order bits are 0
    const long long i = base + (long long)j * KC_THREADS + tid;
    const unsigned o = i < D.n_items ? rc::order_bits(row[i]) : 0u;
    key[j] = o ? rc::order_key(o, (unsigned)i) : 0ull;
  }
  __syncthreads();
  rc::count_larger(key, D.n_list, D.ranks + (size_t)u * D.ld_ranks, C);
}

// ---- shared host side ----------------------------------------------------------------------------------------------
// the model-side fields of both descriptors (same names)
template <class Desc>
int kc_check(const Desc& D, const char* what) {
  CARCA_CHECK_ARG(D.B >= 1 && D.L >= 1 && D.n_items >= 1 && D.F >= 1, "%s: B, L, n_items and F must be positive", what);
  CARCA_CHECK_SUPPORTED(D.B <= 65535, "%s: B = %d users exceeds 65535", what, D.B);
  // (32-bit lane offsets: 64 query rows and 16 table rows stay below 2^30 bytes)
  CARCA_CHECK_SUPPORTED(D.F <= (1 << 22), "%s: F = %d features exceeds 2^22", what, D.F);
  CARCA_CHECK_ARG(D.table && D.ld_table >= D.F && D.ld_table <= (1 << 24), "%s: null table or ld_table outside F..2^24",
                  what);
  CARCA_CHECK_ARG(D.user_a ? D.ld_user_a >= D.F : (D.p_ids && D.ld_p_ids >= D.L),
                  "%s: dense mode needs ld_user_a >= F, table mode p_ids with ld_p_ids >= L", what);
  CARCA_CHECK_ARG(!D.table_i8 || (!D.user_a && D.ld_table_i8 >= D.F && D.ld_table_i8 % 64 == 0),
                  "%s: table_i8 needs table mode and ld_table_i8 >= F, a multiple of 64", what);
  return rc::check_exclusion(D, what);
}

// scratch: [B, n_items] logits, then the [Bp, ldq] query rows, then `extra` bytes; launches the query and scoring kernels
template <class Desc>
int kc_score(const Desc& D, const char* what, size_t extra, hipStream_t stream, float** logits, int64_t* ld_s,
             void** extra_ptr) {
  const bool i8 = D.table_i8 != nullptr;
  const int es = i8 ? 1 : 4;
  const int ldq = i8 ? D.ld_table_i8 : round_up(D.F, 16);  // a whole number of 64-byte chunks
  const int nub = (D.B + KC_UB - 1) / KC_UB, Bp = nub * KC_UB;
  const int64_t lds = D.n_items;
  const size_t logit_bytes = ((size_t)D.B * (size_t)lds * sizeof(float) + 255) / 256 * 256;
  const size_t q_bytes = ((size_t)Bp * ldq * es + 255) / 256 * 256;
  const size_t bytes = logit_bytes + q_bytes + extra;
  char* base = (char*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                      : carca_stream_scratch(stream, CARCA_SCRATCH_KNN, bytes));
  CARCA_CHECK_ARG(base, "%s: scratch allocation of %zu bytes failed", what, bytes);
  *logits = (float*)base;
  *ld_s = lds;
  *extra_ptr = base + logit_bytes + q_bytes;
  KcQuery Q;
  Q.B = D.B, Q.L = D.L, Q.n_items = D.n_items, Q.F = D.F, Q.ldq = ldq;
  Q.p_ids = D.p_ids, Q.ld_p_ids = D.ld_p_ids, Q.user_a = D.user_a, Q.ld_user_a = D.ld_user_a;
  Q.table = i8 ? (const void*)D.table_i8 : (const void*)D.table;
  Q.ld_table = i8 ? D.ld_table_i8 : D.ld_table;
  Q.q = base + logit_bytes;
  if (i8)
    hipLaunchKernelGGL(kc_query_kernel<true>, dim3(Bp), dim3(KC_THREADS), 0, stream, Q);
  else
    hipLaunchKernelGGL(kc_query_kernel<false>, dim3(Bp), dim3(KC_THREADS), 0, stream, Q);
  CARCA_LAUNCH_CHECK();
  KcScore P;
  P.table = Q.table, P.ld = (int)Q.ld_table, P.q = Q.q, P.ldq = ldq;
  P.B = D.B, P.n_items = D.n_items, P.F = D.F, P.nchunks = ldq * es / 64, P.nub = nub;
  P.logits = *logits, P.ld_s = lds;
  const long long blocks = (long long)nub * ((D.n_items + KC_IB - 1) / KC_IB);
  CARCA_CHECK_SUPPORTED(blocks < (1ll << 31), "%s: %lld scoring workgroups", what, blocks);
  const bool vec = D.F % 4 == 0 && D.ld_table % 4 == 0 && ((uintptr_t)D.table & 15) == 0;
  if (i8)
    hipLaunchKernelGGL((kc_score_kernel<true, true>), dim3((unsigned)blocks), dim3(KC_THREADS), 0, stream, P);
  else if (vec)
    hipLaunchKernelGGL((kc_score_kernel<false, true>), dim3((unsigned)blocks), dim3(KC_THREADS), 0, stream, P);
  else
    hipLaunchKernelGGL((kc_score_kernel<false, false>), dim3((unsigned)blocks), dim3(KC_THREADS), 0, stream, P);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_knn_recommend(const CarcaKnnRecommendDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "knn_recommend: null descriptor");
  const CarcaKnnRecommendDesc& D = *desc;
  int rc = kc_check(D, "knn_recommend");
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_SUPPORTED(D.k >= 1 && D.k <= rc::RC_KMAX, "knn_recommend: k = %d outside 1..128", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out && D.ld_scores >= D.k && D.ld_ids_out >= D.k,
                  "knn_recommend: null output or row stride shorter than k");
  float* logits = nullptr;
  int64_t ld_s = 0;
  void* unused = nullptr;
  rc = kc_score(D, "knn_recommend", 0, stream, &logits, &ld_s, &unused);
  if (rc != CARCA_OK) return rc;
  KcSelect S;
  S.n_items = D.n_items, S.k = D.k, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  S.scores = D.scores, S.ld_scores = D.ld_scores, S.ids_out = D.ids_out, S.ld_ids_out = D.ld_ids_out;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<KcSelect>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(rc::rc_select_kernel<KcSelect>, dim3(D.B), dim3(rc::RC_SEL_THREADS), 0, stream, S, logits,
                     (int)ld_s, rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_knn_rank_items(const CarcaKnnRankDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "knn_rank_items: null descriptor");
  const CarcaKnnRankDesc& D = *desc;
  int rc = kc_check(D, "knn_rank_items");
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_SUPPORTED(D.n_list >= 1 && D.n_list <= rc::LIST_MAX, "knn_rank_items: n_list = %d outside 1..128", D.n_list);
  CARCA_CHECK_ARG(D.items && D.scores && D.ranks && D.ld_items >= D.n_list && D.ld_scores >= D.n_list &&
                      D.ld_ranks >= D.n_list,
                  "knn_rank_items: null list / output or row stride shorter than n_list");
  float* logits = nullptr;
  int64_t ld_s = 0;
  void* kp = nullptr;
  rc = kc_score(D, "knn_rank_items", (size_t)D.B * D.n_list * sizeof(unsigned long long), stream, &logits, &ld_s, &kp);
  if (rc != CARCA_OK) return rc;
  unsigned long long* tkeys = (unsigned long long*)kp;
  // the targets' keys before the exclusion overwrites any of them: an excluded target keeps its position
  hipLaunchKernelGGL(kc_list_kernel, dim3(D.B), dim3(rc::LIST_MAX), 0, stream, D, logits, ld_s, tkeys);
  CARCA_LAUNCH_CHECK();
  KcSelect S = {};
  S.n_items = D.n_items, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<KcSelect>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  const int per_block = KC_THREADS * KC_CNT_PER_THREAD;
  const dim3 grid((D.n_items + per_block - 1) / per_block, D.B);
  hipLaunchKernelGGL(kc_count_kernel, grid, dim3(KC_THREADS), 0, stream, D, logits, ld_s, tkeys);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
