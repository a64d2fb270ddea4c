// Full-catalogue top-k and exact ranks for the KNN baseline (include/carca_hip.h: carca_knn_recommend,
// carca_knn_rank_items).
//
// The reference's KNN scores a (user, item) pair as the dot product of the last profile slot's attribute row with the
// item's attribute row (knn.py:13-19), so scoring the whole catalogue for B users is one GEMM, S = Q A^T, with
// Q [B, F] the users' query rows and A [n_items, F] the attribute table.  At C2 that is 128 x 12,102 x 4,096: a real GEMM,
// where CARCA's catalogue kernels (recommend_common.h) keep an item row of at most 128 floats in registers.
// Launches, no host wait, nothing retained:
//   1. query (rs::gather_kernel, row_stream.h): the [Bp, ldq] query rows (Bp = B rounded up to the 64-user block),
//      zero-padded, into stream scratch: table[p_ids[u][L-1]] (a zero row for an id outside [0, n_items)), or the
//      caller's dense rows;
//   2. scoring (rs::score_kernel, the streaming loop shared with similar_items.hip): a users x items GEMM into a
//      [B, n_items] logit buffer, stored by this file's epilogue.  Two element types:
//        fp32: v_mfma_f32_16x16x4_f32, exact fp32 products; each output sums chains of 256 k (fmaf chains)
//              in fp32.  b128 loads of the table where F, ld_table and the table's address allow, b32 loads otherwise;
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
#include "deep_select.h"
#include "policy_items.h"
#include "row_stream.h"
#include "sampled_select.h"

namespace {

constexpr int KC_CNT_PER_THREAD = 8;      // items per lane in the counting sweep
static_assert(rs::THREADS == rc::TILE, "rc::count_larger counts over a workgroup of rc::TILE threads");

// ---- 1. query rows: the row source of rs::gather_kernel ----------------------------------------------------------
template <class T>
struct KcQueryRow {
  int B, L, n_items;
  const int32_t* p_ids;
  int ld_p_ids;
  const T* user_a;  // dense rows, or NULL
  int64_t ld_user_a;
  const T* table;  // fp32 table, or its int8 copy
  int64_t ld_table;
  __device__ const T* operator()(int u) const {
    if (u >= B) return nullptr;
    if (user_a) return user_a + (size_t)u * ld_user_a;
    const int id = p_ids[(size_t)u * ld_p_ids + L - 1];
    return id >= 0 && id < n_items ? table + (size_t)id * ld_table : nullptr;
  }
};

// ---- 2. scoring: the epilogue of rs::score_kernel ----------------------------------------------------------------
struct KcStore {
  float* logits;
  int64_t ld_s;
  int B, n_items;
  struct Shared {};
  __device__ void stage(int, Shared&) const {}
  __device__ void store(const f32x4 (&tile)[rs::MQ], int u0, int item, int g, const Shared&) const {
    if (item >= n_items) return;
#pragma unroll
    for (int m = 0; m < rs::MQ; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int u = u0 + 16 * m + 4 * g + j;
        if (u < B) logits[(size_t)u * ld_s + item] = tile[m][j];
      }
  }
};

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

__global__ __launch_bounds__(rs::THREADS) void kc_count_kernel(CarcaKnnRankDesc D, const float* __restrict__ logits,
                                                              int64_t ld_s, const unsigned long long* __restrict__ tkeys) {
  __shared__ rc::CountLds C;
  const int tid = threadIdx.x, u = blockIdx.y;
  for (int t = tid; t < D.n_list; t += rs::THREADS) C.tkey[t] = tkeys[(size_t)u * D.n_list + t];
  const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
  const long long base = (long long)blockIdx.x * rs::THREADS * KC_CNT_PER_THREAD;
  unsigned long long key[KC_CNT_PER_THREAD];
#pragma unroll
  for (int j = 0; j < KC_CNT_PER_THREAD; ++j) {  // excluded ids and id 0 hold the sentinel, whose order bits are 0
    const long long i = base + (long long)j * rs::THREADS + tid;
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
  const int nub = (D.B + rs::QB - 1) / rs::QB, Bp = nub * rs::QB;
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
  void* q = base + logit_bytes;
  if (i8) {
    const KcQueryRow<int8_t> src = {D.B, D.L, D.n_items, D.p_ids, D.ld_p_ids, nullptr, 0, D.table_i8, D.ld_table_i8};
    hipLaunchKernelGGL((rs::gather_kernel<int8_t, KcQueryRow<int8_t>>), dim3(Bp), dim3(rs::THREADS), 0, stream, src, D.F,
                       (int8_t*)q, ldq);
  } else {
    const KcQueryRow<float> src = {D.B, D.L, D.n_items, D.p_ids, D.ld_p_ids, D.user_a, D.ld_user_a, D.table, D.ld_table};
    hipLaunchKernelGGL((rs::gather_kernel<float, KcQueryRow<float>>), dim3(Bp), dim3(rs::THREADS), 0, stream, src, D.F,
                       (float*)q, ldq);
  }
  CARCA_LAUNCH_CHECK();
  rs::Operands P;
  P.table = i8 ? (const void*)D.table_i8 : (const void*)D.table, P.ld = i8 ? D.ld_table_i8 : D.ld_table;
  P.q = q, P.ldq = ldq, P.rows = D.n_items, P.cols = D.F, P.nchunks = ldq * es / 64, P.nqb = nub;
  const KcStore epi = {*logits, lds, D.B, D.n_items};
  const bool vec = D.F % 4 == 0 && D.ld_table % 4 == 0 && ((uintptr_t)D.table & 15) == 0;
  return i8    ? rs::launch_score<rs::I8>(P, epi, what, stream)
         : vec ? rs::launch_score<rs::F32Aligned>(P, epi, what, stream)
               : rs::launch_score<rs::F32Unaligned>(P, epi, what, stream);
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
  rc::SelectView S;
  S.n_items = D.n_items, S.k = D.k, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  S.scores = D.scores, S.ld_scores = D.ld_scores, S.ids_out = D.ids_out, S.ld_ids_out = D.ld_ids_out;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<rc::SelectView>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(rc::rc_select_kernel<rc::SelectView>, dim3(D.B), dim3(rc::RC_SEL_THREADS), 0, stream, S, logits,
                     (int)ld_s, rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// carca_knn_recommend in depth: the same query, scoring and exclusion launches, so the same logit
// bits, then the deep selection of deep_select.h in place of rc_select_kernel
extern "C" int carca_knn_retrieve(const CarcaKnnRecommendDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "knn_retrieve: null descriptor");
  const CarcaKnnRecommendDesc& D = *desc;
  int rc = kc_check(D, "knn_retrieve");
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_SUPPORTED(D.k >= 1 && D.k <= rc::DS_KMAX, "knn_retrieve: k = %d outside 1..4096", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out && D.ld_scores >= D.k && D.ld_ids_out >= D.k,
                  "knn_retrieve: null output or row stride shorter than k");
  float* logits = nullptr;
  int64_t ld_s = 0;
  void* unused = nullptr;
  rc = kc_score(D, "knn_retrieve", 0, stream, &logits, &ld_s, &unused);
  if (rc != CARCA_OK) return rc;
  rc::SelectView S;
  S.n_items = D.n_items, S.k = D.k, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  S.scores = D.scores, S.ld_scores = D.ld_scores, S.ids_out = D.ids_out, S.ld_ids_out = D.ld_ids_out;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<rc::SelectView>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  return rc::ds_select(S, D.B, logits, (int)ld_s, D.n_items, rc::AllItems{}, "knn_retrieve", stream);
}

// carca_knn_recommend drawn instead of sorted: the same query, scoring and exclusion launches, so
// the same logit bits, then sampled_select.h's perturb pass, deep selection and finishing launch with no link.  The
// buffer's columns are item ids; a candidate list strikes the items outside it out in the perturb pass.
extern "C" int carca_knn_recommend_sampled(const CarcaKnnRecommendDesc* desc, const CarcaCandidates* cand,
                                           const CarcaSampling* sampling, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "knn_recommend_sampled: null descriptor");
  const CarcaKnnRecommendDesc& D = *desc;
  int rc = kc_check(D, "knn_recommend_sampled");
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_SUPPORTED(D.k >= 1 && D.k <= rc::DS_KMAX, "knn_recommend_sampled: k = %d outside 1..4096", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out && D.ld_scores >= D.k && D.ld_ids_out >= D.k,
                  "knn_recommend_sampled: null output or row stride shorter than k");
  if ((rc = rc::sp_check(sampling, D.k, "knn_recommend_sampled")) != CARCA_OK) return rc;
  if (cand && (rc = rc::check_candidates(cand, "knn_recommend_sampled")) != CARCA_OK) return rc;
  float* logits = nullptr;
  int64_t ld_s = 0;
  void* unused = nullptr;
  rc = kc_score(D, "knn_recommend_sampled", 0, stream, &logits, &ld_s, &unused);
  if (rc != CARCA_OK) return rc;
  rc::SelectView S;
  S.n_items = D.n_items, S.k = D.k, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  S.scores = D.scores, S.ld_scores = D.ld_scores, S.ids_out = D.ids_out, S.ld_ids_out = D.ld_ids_out;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<rc::SelectView>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  if (cand)
    return rc::sp_run(S, D.B, logits, (int)ld_s, D.n_items, rc::AllItems{}, rc::SpKeepListed{rc::ListedItems{cand->ids, cand->n}},
                      *sampling, "knn_recommend_sampled", stream);
  return rc::sp_run(S, D.B, logits, (int)ld_s, D.n_items, rc::AllItems{}, rc::SpKeepAll{}, *sampling, "knn_recommend_sampled", stream);
}

// carca_log_prob_items over the KNN descriptor: carca_knn_recommend_sampled's query, scoring and
// exclusion launches, so the same logit bits and eligibility, then policy_items.h's reduce pass and finishing launch.  The
// buffer's columns are item ids; a candidate list strikes the items outside it out in both launches.
extern "C" int carca_knn_log_prob_items(const CarcaKnnRecommendDesc* desc, const CarcaCandidates* cand,
                                        const CarcaPolicyItems* policy, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "knn_log_prob_items: null descriptor");
  const CarcaKnnRecommendDesc& D = *desc;
  int rc = kc_check(D, "knn_log_prob_items");
  if (rc != CARCA_OK) return rc;
  if ((rc = rc::pl_check(policy, "knn_log_prob_items")) != CARCA_OK) return rc;
  if (cand && (rc = rc::check_candidates(cand, "knn_log_prob_items")) != CARCA_OK) return rc;
  float* logits = nullptr;
  int64_t ld_s = 0;
  void* unused = nullptr;
  rc = kc_score(D, "knn_log_prob_items", 0, stream, &logits, &ld_s, &unused);
  if (rc != CARCA_OK) return rc;
  rc::SelectView S = {};
  S.n_items = D.n_items, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<rc::SelectView>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  if (cand)
    return rc::pl_run(D.n_items, D.B, logits, (int)ld_s, D.n_items, rc::AllItems{},
                      rc::SpKeepListed{rc::ListedItems{cand->ids, cand->n}}, *policy, "knn_log_prob_items", stream);
  return rc::pl_run(D.n_items, D.B, logits, (int)ld_s, D.n_items, rc::AllItems{}, rc::SpKeepAll{}, *policy,
                    "knn_log_prob_items", stream);
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
  rc::SelectView S = {};
  S.n_items = D.n_items, S.exclude = D.exclude, S.n_exclude = D.n_exclude, S.ld_exclude = D.ld_exclude;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<rc::SelectView>, dim3(D.B), dim3(64), 0, stream, S, logits, (int)ld_s,
                     rc::AllItems{});
  CARCA_LAUNCH_CHECK();
  const int per_block = rs::THREADS * KC_CNT_PER_THREAD;
  const dim3 grid((D.n_items + per_block - 1) / per_block, D.B);
  hipLaunchKernelGGL(kc_count_kernel, grid, dim3(rs::THREADS), 0, stream, D, logits, ld_s, tkeys);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
