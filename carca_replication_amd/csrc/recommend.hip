// Full-catalogue top-k recommendation (include/carca_hip.h: carca_recommend).
//
// The reference scores only the candidates a caller lists (carca.py:338-349, 352-399 over the 1 + 100 candidates of
// data.py:180-185).  In eval mode the candidates do not interact (carca.py:339: causal=None) and every embedding class is
// affine in the context, e(i, c) = T[i] + M c, so scoring EVERY item for a user needs per item only
// a row of a table built once per weight version, and per (user, item) pair:
//   cross-attention  sum_h softmax_l((QT[i]_h . K_hl + beta_hl) / sqrt(dh)) . u_hl  (+ wT[i]) + off_u
//   dot decoders     p_u . (T[i] + m_u), divided by ||T[i] + m_u|| for the normalised WeightedDotProduct
// Three launches, no host wait, nothing retained:
//   1. scoring, the sweep of catalogue_sweep.h with rc::RcStoreSink: workgroups own 256-item tiles (one item per lane, its
//      row in registers) and walk a chunk of users, each user's keys / folded values / score biases staged in LDS
//      (recommend_common.h) -- whole for a profile of up to CARCA_MAX_L slots, in chunks of CARCA_MAX_L valid slots
//      beyond (rc::CaLongScorer under rc::sweep_long_kernel; the dot decoders read no L); raw logits go to a
//      [B, n_items] stream-scratch buffer;
//   2. exclusion: id 0 and the caller's [B, E] list are overwritten with a sentinel that selection never picks;
//   3. selection: one workgroup per user, an MSB-first radix select over 64-bit keys (order-preserving logit bits,
//      then the complemented item id, so ties go to the smaller id), a bitonic sort of the k survivors, and the link
//      (sigmoid, or (y + 1) / 2) applied to the k selected logits only.
// Launches 2 and 3 live in catalogue_select.h, shared with carca_knn_recommend (knn_catalogue.hip); the sink and the host
// side of launches 1 and 2 (rc::rc_score) in recommend_score.h, shared with carca_recommend_users (recommend_users.hip).
// Integer LDS atomics only (histograms, slot counters); the result does not depend on scheduling.
//
// carca_recommend_among runs the same three launches over a candidate list S (ascending, distinct ids) in place of the
// catalogue, through the item map rc::ListedItems: the sweep's lane at position p owns item ids[p] (the same row gather,
// so the same logit bits), the buffer is [B, |S|] indexed by position, exclusion finds an id's position by binary search,
// and selection keys on the position (S ascending: ties still go to the smaller id) and writes ids[p].
//
// carca_recommend_groups / carca_recommend_capped sweep the catalogue once in group-major order --
// CarcaItemGroups::order through rc::ListedItems, carca_recommend_among's scoring launch and so its logit bits -- exclude
// through rc::GroupedItems (pos_of[id]: the order ascends only inside a group), and select per (user, group) segment with
// the kernels of group_select.h.
#include "group_select.h"
#include "recommend_score.h"

namespace {

// the checks of a top-k call; out_cols: the columns a user's row of the two outputs holds
int rc_check(const CarcaRecommendDesc& D, long long out_cols) {
  if (int rc = rc::check_model(D, "recommend")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "recommend: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::RC_KMAX, "recommend: k = %d exceeds the largest k, 128", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "recommend: null pointer");
  CARCA_CHECK_ARG(D.ld_scores >= out_cols && D.ld_ids_out >= out_cols, "recommend: row stride shorter than its row");
  return CARCA_OK;
}

template <class Map>
int rc_run(const CarcaRecommendDesc& D, Map map, int n_slots, hipStream_t stream) {
  if (int rc = rc_check(D, D.k)) return rc;
  float* logits = nullptr;
  if (int rc = rc::rc_score(D, map, map, n_slots, stream, &logits)) return rc;
  hipLaunchKernelGGL((rc::rc_select_kernel<CarcaRecommendDesc, Map>), dim3(D.B), dim3(rc::RC_SEL_THREADS), 0, stream, D,
                     logits, n_slots, map);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// ---- item groups --------------------------------------------------------------------------------
constexpr int RG_MAX_GROUPS = 65535;                // a grid dimension
constexpr size_t RG_MAX_KEY_BYTES = (size_t)1 << 30;  // the capped call's [B, G, m] key scratch

int rg_check(const CarcaRecommendDesc& D, const CarcaItemGroups* g, const char* what) {
  CARCA_CHECK_ARG(g, "%s: null item groups", what);
  CARCA_CHECK_ARG(g->n_groups >= 1, "%s: n_groups must be positive", what);
  CARCA_CHECK_SUPPORTED(g->n_groups <= RG_MAX_GROUPS, "%s: %d groups exceed %d (a grid dimension)", what, g->n_groups,
                        RG_MAX_GROUPS);
  CARCA_CHECK_ARG(g->n >= 0 && g->n < D.n_items, "%s: %d grouped items, the catalogue has %d", what, g->n, D.n_items - 1);
  CARCA_CHECK_ARG(g->offsets && g->pos_of && (g->n == 0 || g->order), "%s: null pointer in the item groups", what);
  return CARCA_OK;
}

// the sweep over the grouped order through rc::ListedItems -- carca_recommend_among's instantiation, so a pair's logit
// bits are carca_recommend's -- and the exclusion through rc::GroupedItems
int rg_score(const CarcaRecommendDesc& D, const CarcaItemGroups& g, hipStream_t stream, float** logits) {
  return rc::rc_score(D, rc::ListedItems{g.order, g.n}, rc::GroupedItems{g.order, g.pos_of, g.n}, g.n, stream, logits);
}

}  // namespace

extern "C" int carca_recommend(const CarcaRecommendDesc* desc, void* stream) {
  CARCA_CHECK_ARG(desc, "recommend: null descriptor");
  return rc_run(*desc, rc::AllItems{}, desc->n_items, (hipStream_t)stream);
}

extern "C" int carca_recommend_among(const CarcaRecommendDesc* desc, const CarcaCandidates* cand, void* stream) {
  CARCA_CHECK_ARG(desc, "recommend: null descriptor");
  if (int rc = rc::check_candidates(cand, "recommend")) return rc;
  return rc_run(*desc, rc::ListedItems{cand->ids, cand->n}, cand->n, (hipStream_t)stream);
}

extern "C" int carca_recommend_groups(const CarcaRecommendDesc* desc, const CarcaItemGroups* groups, void* stream_) {
  CARCA_CHECK_ARG(desc, "recommend_groups: null descriptor");
  const CarcaRecommendDesc& D = *desc;
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = rg_check(D, groups, "recommend_groups")) return rc;
  if (int rc = rc_check(D, (long long)groups->n_groups * D.k)) return rc;
  float* logits = nullptr;
  if (int rc = rg_score(D, *groups, stream, &logits)) return rc;
  hipLaunchKernelGGL((rc::rg_select_kernel<CarcaRecommendDesc, false>), dim3(D.B, groups->n_groups), dim3(rc::GS_THREADS), 0,
                     stream, D, logits, groups->n, rc::GroupedItems{groups->order, groups->pos_of, groups->n},
                     groups->offsets, D.k, nullptr);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_recommend_capped(const CarcaRecommendDesc* desc, const CarcaItemGroups* groups, int max_per_group,
                                      void* stream_) {
  CARCA_CHECK_ARG(desc, "recommend_capped: null descriptor");
  const CarcaRecommendDesc& D = *desc;
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = rg_check(D, groups, "recommend_capped")) return rc;
  if (int rc = rc_check(D, D.k)) return rc;
  CARCA_CHECK_ARG(max_per_group >= 1, "recommend_capped: max_per_group must be positive");
  // the capped list is the first k of the union of every group's best m = min(k, max_per_group)
  const int G = groups->n_groups, m = std::min(D.k, max_per_group);
  const size_t bytes = (size_t)D.B * (size_t)G * (size_t)m * sizeof(unsigned long long);
  CARCA_CHECK_SUPPORTED(bytes <= RG_MAX_KEY_BYTES,
                        "recommend_capped: B = %d users x %d groups x %d per group: the key scratch exceeds 1 GiB", D.B, G, m);
  float* logits = nullptr;
  if (int rc = rg_score(D, *groups, stream, &logits)) return rc;
  unsigned long long* keys =
      (unsigned long long*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                           : carca_stream_scratch(stream, CARCA_SCRATCH_GROUPS, bytes));
  CARCA_CHECK_ARG(keys, "recommend_capped: scratch allocation of %zu bytes failed", bytes);
  hipLaunchKernelGGL((rc::rg_select_kernel<CarcaRecommendDesc, true>), dim3(D.B, G), dim3(rc::GS_THREADS), 0, stream, D,
                     logits, groups->n, rc::GroupedItems{groups->order, groups->pos_of, groups->n}, groups->offsets, m, keys);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL((rc::rg_merge_kernel<CarcaRecommendDesc>), dim3(D.B), dim3(rc::GS_THREADS), 0, stream, D, keys, G * m);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
