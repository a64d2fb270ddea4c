// Full-catalogue top-k recommendation (include/carca_hip.h: carca_recommend).
//
// The reference scores only the candidates a caller lists (carca.py:338-349, 352-399 over the 1 + 100 candidates of
// data.py:180-185).  In eval mode the candidates do not interact (carca.py:339: causal=None) and every embedding class is
// affine in the context, e(i, c) = T[i] + M c, so scoring EVERY item for a user needs per item only
// a row of a table built once per weight version, and per (user, item) pair:
//   cross-attention  sum_h softmax_l((QT[i]_h . K_hl + beta_hl) / sqrt(dh)) . u_hl  (+ wT[i]) + off_u
//   dot decoders     p_u . (T[i] + m_u), divided by ||T[i] + m_u|| for the normalised WeightedDotProduct
// Three launches, no host wait, nothing retained:
//   1. scoring, the sweep of catalogue_sweep.h with the sink below: workgroups own 256-item tiles (one item per lane, its
//      row in registers) and walk a chunk of users, each user's keys / folded values / score biases staged in LDS
//      (recommend_common.h); raw logits go to a [B, n_items] stream-scratch buffer;
//   2. exclusion: id 0 and the caller's [B, E] list are overwritten with a sentinel that selection never picks;
//   3. selection: one workgroup per user, an MSB-first radix select over 64-bit keys (order-preserving logit bits,
//      then the complemented item id, so ties go to the smaller id), a bitonic sort of the k survivors, and the link
//      (sigmoid, or (y + 1) / 2) applied to the k selected logits only.
// Launches 2 and 3 live in catalogue_select.h, shared with carca_knn_recommend (knn_catalogue.hip).
// Integer LDS atomics only (histograms, slot counters); the result does not depend on scheduling.
#include "catalogue_select.h"
#include "catalogue_sweep.h"

namespace {

// the sweep's sink: the raw logit into the [B, n_items] buffer
struct RcStoreSink {
  using Desc = CarcaRecommendDesc;
  struct Lds {};
  float* logits;
  int ld_s;
  __device__ __forceinline__ void begin_user(const Desc&, int, Lds&) const {}
  __device__ __forceinline__ void put(const Desc&, int u, int item, bool live, float logit, Lds&) const {
    if (live) logits[(size_t)u * ld_s + item] = logit;
  }
};

}  // namespace

extern "C" int carca_recommend(const CarcaRecommendDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "recommend: null descriptor");
  const CarcaRecommendDesc& D = *desc;
  if (int rc = rc::check_model(D, "recommend")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "recommend: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::RC_KMAX, "recommend: k = %d exceeds the largest k, 128", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "recommend: null pointer");
  CARCA_CHECK_ARG(D.ld_scores >= D.k && D.ld_ids_out >= D.k, "recommend: row stride shorter than its row");
  // raw logits [B, n_items]: stream scratch (or the capture's memory), consumed by the two launches behind the scoring one
  const int ld_s = D.n_items;
  const size_t bytes = (size_t)D.B * (size_t)ld_s * sizeof(float);
  float* logits = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                          : carca_stream_scratch(stream, CARCA_SCRATCH_RECOMMEND, bytes));
  CARCA_CHECK_ARG(logits, "recommend: scratch allocation of %zu bytes failed", bytes);
  const rc::SweepGrid G = rc::sweep_grid(D.n_items, D.B);
  const int rc = rc::dispatch_scorer(D, "recommend", [&](auto scorer) -> int {
    using Scorer = typename decltype(scorer)::type;
    hipLaunchKernelGGL((rc::sweep_kernel<Scorer, RcStoreSink>), G.grid, dim3(rc::TILE), 0, stream, D,
                       RcStoreSink{logits, ld_s}, G.users_per_block);
    CARCA_LAUNCH_CHECK();
    return CARCA_OK;
  });
  if (rc != CARCA_OK) return rc;
  hipLaunchKernelGGL(rc::rc_exclude_kernel<CarcaRecommendDesc>, dim3(D.B), dim3(64), 0, stream, D, logits, ld_s);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(rc::rc_select_kernel<CarcaRecommendDesc>, dim3(D.B), dim3(rc::RC_SEL_THREADS), 0, stream, D, logits,
                     ld_s);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
