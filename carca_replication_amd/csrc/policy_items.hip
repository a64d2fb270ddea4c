// A sampling policy's log-probabilities for listed items (include/carca_hip.h: carca_log_prob_items; DESIGN.md section
// 28): log pi(item | user) under softmax(logit / temperature) over the user's eligible items for every entry of a list per
// user, with the per-user logsumexp and entropy -- what an off-policy estimator puts over the propensities
// carca_recommend_sampled logged.
//
// Scoring and exclusion are carca_recommend's own launches (rc::rc_score, recommend_score.h), exactly as
// carca_recommend_sampled queues them, so a pair's raw logit and eligibility are that call's.  Behind them run
// policy_items.h's two launches: the reduce pass (the perturb pass's read side: chunk partials of the logsumexp and the
// entropy) and the finishing launch (the merge, then raw / temperature - logsumexp for every listed id that is eligible,
// -inf for every other).  The descriptor's k, scores and ids_out are not read.
#include "policy_items.h"
#include "recommend_score.h"

namespace {

template <class Map>
int lp_run(const CarcaRecommendDesc& D, Map map, int n_slots, const CarcaPolicyItems* X, hipStream_t stream) {
  if (int rc = rc::check_model(D, "log_prob_items")) return rc;
  if (int rc = rc::pl_check(X, "log_prob_items")) return rc;
  float* logits = nullptr;
  if (int rc = rc::rc_score(D, map, map, n_slots, stream, &logits)) return rc;
  return rc::pl_run(D.n_items, D.B, logits, n_slots, n_slots, map, rc::SpKeepAll{}, *X, "log_prob_items", stream);
}

}  // namespace

extern "C" int carca_log_prob_items(const CarcaRecommendDesc* desc, const CarcaCandidates* cand,
                                    const CarcaPolicyItems* policy, void* stream) {
  CARCA_CHECK_ARG(desc, "log_prob_items: null descriptor");
  if (!cand) return lp_run(*desc, rc::AllItems{}, desc->n_items, policy, (hipStream_t)stream);
  if (int rc = rc::check_candidates(cand, "log_prob_items")) return rc;
  return lp_run(*desc, rc::ListedItems{cand->ids, cand->n}, cand->n, policy, (hipStream_t)stream);
}

// The reduce pass alone over a caller-held buffer, columns = item ids (rc::AllItems, no filter): what tools/bench_policy.py
// times against the bytes the pass reads, beside carca_sampled_perturb on the same buffer.  logits [B, n_slots] fp32,
// 16-byte aligned, row stride n_slots; partials [B, ceil(n_slots / 1024), 3] fp32.
extern "C" int carca_policy_reduce(const float* logits, float* partials, int B, int n_slots, float temperature,
                                   void* stream) {
  CARCA_CHECK_ARG(logits && partials, "policy_reduce: null pointer");
  CARCA_CHECK_ARG(B >= 1 && n_slots >= 1, "policy_reduce: B and n_slots must be positive");
  CARCA_CHECK_ARG(std::isfinite(temperature) && temperature >= FLT_MIN,
                  "policy_reduce: temperature must be finite and positive, a normal fp32 number");
  CARCA_CHECK_ARG((reinterpret_cast<uintptr_t>(logits) & 15) == 0, "policy_reduce: the logit buffer must be 16-byte aligned");
  const int n_chunks = (n_slots + rc::SP_CHUNK - 1) / rc::SP_CHUNK;
  hipLaunchKernelGGL((rc::pl_reduce_kernel<rc::AllItems, rc::SpKeepAll>), dim3(B, rc::sp_parts(B, n_chunks)),
                     dim3(rc::SP_THREADS), 0, (hipStream_t)stream, logits, n_slots, n_slots, rc::AllItems{}, rc::SpKeepAll{},
                     temperature, n_chunks, partials);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
