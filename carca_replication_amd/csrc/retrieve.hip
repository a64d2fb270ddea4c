// Deep full-catalogue top-k (include/carca_hip.h: carca_retrieve / carca_retrieve_among): the first
// stage in front of a re-ranker, a business-rule filter or carca_recommend_lists -- the k best items per user for k up to
// 4096, where carca_recommend stops at 128.
//
// Scoring and exclusion are carca_recommend's own launches (rc::rc_score, recommend_score.h: the sweep of
// catalogue_sweep.h into a [B, n_slots] raw-logit buffer, then the sentinel over id 0 and the excluded ids), so a
// (user, item) pair's logit has carca_recommend's bits by construction.  Selection is deep_select.h's: a user's row is
// split into S parts whose best keys go to stream scratch (ds_part_kernel, grid (B, S)) and are merged per user
// (ds_merge_kernel), or, S = 1, the merge launch reads the row itself.  The keys are carca_recommend's
// (rc::order_key(order bits, column)), so the order is too: logit descending, ties to the smaller id; under a candidate
// list the column is the position in the ascending list and the id written is ids[position].
#include "deep_select.h"
#include "recommend_score.h"

namespace {

int rt_check(const CarcaRecommendDesc& D) {
  if (int rc = rc::check_model(D, "retrieve")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "retrieve: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::DS_KMAX, "retrieve: k = %d exceeds the largest k, 4096", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "retrieve: null pointer");
  CARCA_CHECK_ARG(D.ld_scores >= D.k && D.ld_ids_out >= D.k, "retrieve: row stride shorter than its row");
  return CARCA_OK;
}

template <class Map>
int rt_run(const CarcaRecommendDesc& D, Map map, int n_slots, hipStream_t stream) {
  if (int rc = rt_check(D)) return rc;
  float* logits = nullptr;
  if (int rc = rc::rc_score(D, map, map, n_slots, stream, &logits)) return rc;
  return rc::ds_select(D, D.B, logits, n_slots, n_slots, map, "retrieve", stream);
}

}  // namespace

extern "C" int carca_retrieve(const CarcaRecommendDesc* desc, void* stream) {
  CARCA_CHECK_ARG(desc, "retrieve: null descriptor");
  return rt_run(*desc, rc::AllItems{}, desc->n_items, (hipStream_t)stream);
}

extern "C" int carca_retrieve_among(const CarcaRecommendDesc* desc, const CarcaCandidates* cand, void* stream) {
  CARCA_CHECK_ARG(desc, "retrieve: null descriptor");
  if (int rc = rc::check_candidates(cand, "retrieve")) return rc;
  return rt_run(*desc, rc::ListedItems{cand->ids, cand->n}, cand->n, (hipStream_t)stream);
}
