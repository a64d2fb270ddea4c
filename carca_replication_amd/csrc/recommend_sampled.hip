// Gumbel top-k sampling with logged propensities (include/carca_hip.h: carca_recommend_sampled):
// k items per user drawn without replacement from softmax(logit / temperature) over the eligible items, reproducible
// from a seed, with each drawn item's log-probability under that softmax -- the pi(a | x) an off-policy estimator
// divides by.
//
// Scoring and exclusion are carca_recommend's own launches (rc::rc_score, recommend_score.h), so a (user, item) pair's
// raw logit has carca_recommend's bits and eligibility is carca_recommend's: id != 0, not excluded, inside the candidate
// list when one is given.  Behind them run sampled_select.h's three steps: the perturb pass (z + g into a second [B,
// n_slots] buffer, logsumexp partials), deep_select.h's selection over the perturbed buffer, and the finishing launch
// (scores = link(raw logit), log_probs = raw / temperature - logsumexp).  Under a candidate list a column is a position
// of the ascending list; the noise is hashed from the item id behind it.
#include "recommend_score.h"
#include "sampled_select.h"

namespace {

int rs_check(const CarcaRecommendDesc& D, const CarcaSampling* X) {
  if (int rc = rc::check_model(D, "recommend_sampled")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "recommend_sampled: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::DS_KMAX, "recommend_sampled: k = %d exceeds the largest k, 4096", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "recommend_sampled: null pointer");
  CARCA_CHECK_ARG(D.ld_scores >= D.k && D.ld_ids_out >= D.k, "recommend_sampled: row stride shorter than its row");
  return rc::sp_check(X, D.k, "recommend_sampled");
}

template <class Map>
int rs_run(const CarcaRecommendDesc& D, Map map, int n_slots, const CarcaSampling* X, hipStream_t stream) {
  if (int rc = rs_check(D, X)) return rc;
  float* logits = nullptr;
  if (int rc = rc::rc_score(D, map, map, n_slots, stream, &logits)) return rc;
  return rc::sp_run(D, D.B, logits, n_slots, n_slots, map, rc::SpKeepAll{}, *X, "recommend_sampled", stream);
}

}  // namespace

extern "C" int carca_recommend_sampled(const CarcaRecommendDesc* desc, const CarcaCandidates* cand,
                                       const CarcaSampling* sampling, void* stream) {
  CARCA_CHECK_ARG(desc, "recommend_sampled: null descriptor");
  if (!cand) return rs_run(*desc, rc::AllItems{}, desc->n_items, sampling, (hipStream_t)stream);
  if (int rc = rc::check_candidates(cand, "recommend_sampled")) return rc;
  return rs_run(*desc, rc::ListedItems{cand->ids, cand->n}, cand->n, sampling, (hipStream_t)stream);
}

// The perturb pass alone over caller-held buffers, columns = item ids (rc::AllItems, no filter): what tools/bench_sampled.py
// times against the bytes the pass moves.  logits and perturbed [B, n_slots] fp32, 16-byte aligned, row stride n_slots;
// partials [B, ceil(n_slots / 1024), 2] fp32.  Reads temperature, seed and user_keys of the sampling block.
extern "C" int carca_sampled_perturb(const float* logits, float* perturbed, float* partials, int B, int n_slots,
                                     const CarcaSampling* sampling, void* stream) {
  CARCA_CHECK_ARG(logits && perturbed && partials && sampling, "sampled_perturb: null pointer");
  CARCA_CHECK_ARG(B >= 1 && n_slots >= 1, "sampled_perturb: B and n_slots must be positive");
  CARCA_CHECK_ARG(std::isfinite(sampling->temperature) && sampling->temperature >= FLT_MIN,
                  "sampled_perturb: temperature must be finite and positive, a normal fp32 number");
  CARCA_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(perturbed) & 15) == 0,
                  "sampled_perturb: logit buffers must be 16-byte aligned");
  const int n_chunks = (n_slots + rc::SP_CHUNK - 1) / rc::SP_CHUNK;
  const rc::SpNoise N = {sampling->temperature, (unsigned long long)sampling->seed, sampling->user_keys};
  hipLaunchKernelGGL((rc::sp_perturb_kernel<rc::AllItems, rc::SpKeepAll>), dim3(B, rc::sp_parts(B, n_chunks)),
                     dim3(rc::SP_THREADS), 0, (hipStream_t)stream, logits, perturbed, n_slots, n_slots, rc::AllItems{},
                     rc::SpKeepAll{}, N, n_chunks, reinterpret_cast<float2*>(partials));
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
