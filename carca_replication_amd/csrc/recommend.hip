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
//      (recommend_common.h) -- whole for a profile of up to CARCA_MAX_L slots, in chunks of CARCA_MAX_L valid slots
//      beyond (rc::CaLongScorer under rc::sweep_long_kernel; the dot decoders read no L); raw logits go to a
//      [B, n_items] stream-scratch buffer;
//   2. exclusion: id 0 and the caller's [B, E] list are overwritten with a sentinel that selection never picks;
//   3. selection: one workgroup per user, an MSB-first radix select over 64-bit keys (order-preserving logit bits,
//      then the complemented item id, so ties go to the smaller id), a bitonic sort of the k survivors, and the link
//      (sigmoid, or (y + 1) / 2) applied to the k selected logits only.
// Launches 2 and 3 live in catalogue_select.h, shared with carca_knn_recommend (knn_catalogue.hip).
// Integer LDS atomics only (histograms, slot counters); the result does not depend on scheduling.
//
// carca_recommend_among runs the same three launches over a candidate list S (ascending, distinct ids) in place of the
// catalogue, through the item map rc::ListedItems: the sweep's lane at position p owns item ids[p] (the same row gather,
// so the same logit bits), the buffer is [B, |S|] indexed by position, exclusion finds an id's position by binary search,
// and selection keys on the position (S ascending: ties still go to the smaller id) and writes ids[p].
#include "catalogue_select.h"
#include "catalogue_sweep.h"

namespace {

// the sweep's sink: the raw logit into the [B, n_items] buffer -- or, under a candidate list, into the [B, C] buffer at
// the item's position, a listed id outside the catalogue as the exclusion sentinel
template <class Map>
struct RcStoreSink {
  using Desc = CarcaRecommendDesc;
  struct Lds {};
  float* logits;
  int ld_s;
  __device__ __forceinline__ void begin_user(const Desc&, int, Lds&) const {}
  __device__ __forceinline__ void put(const Desc&, int u, int pos, int, bool live, float logit, Lds&) const {
    if constexpr (Map::listed) {
      if (pos < ld_s) logits[(size_t)u * ld_s + pos] = live ? logit : __uint_as_float(rc::RC_SENTINEL);
    } else {
      if (live) logits[(size_t)u * ld_s + pos] = logit;
    }
  }
};

// n_slots: the columns of the logit buffer, n_items or the candidate count
template <class Map>
int rc_run(const CarcaRecommendDesc& D, Map map, int n_slots, hipStream_t stream) {
  if (int rc = rc::check_model(D, "recommend")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "recommend: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::RC_KMAX, "recommend: k = %d exceeds the largest k, 128", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "recommend: null pointer");
  CARCA_CHECK_ARG(D.ld_scores >= D.k && D.ld_ids_out >= D.k, "recommend: row stride shorter than its row");
  // raw logits [B, n_slots]: stream scratch (or the capture's memory), consumed by the two launches behind the scoring one
  const int ld_s = n_slots;
  const size_t bytes = std::max((size_t)D.B * (size_t)ld_s, (size_t)1) * sizeof(float);
  float* logits = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                          : carca_stream_scratch(stream, CARCA_SCRATCH_RECOMMEND, bytes));
  CARCA_CHECK_ARG(logits, "recommend: scratch allocation of %zu bytes failed", bytes);
  if (n_slots > 0) {  // (an empty candidate list: no tile to sweep, selection finds no eligible item)
    const rc::SweepGrid G = rc::sweep_grid(n_slots, D.B);
    const int rc = rc::dispatch_scorer(D, "recommend", [&](auto scorer) -> int {
      using Scorer = typename decltype(scorer)::type;
      if constexpr (Scorer::chunked) {  // cross-attention over a profile of more than CARCA_MAX_L slots
        hipLaunchKernelGGL((rc::sweep_long_kernel<Scorer, RcStoreSink<Map>, Map>), G.grid, dim3(rc::TILE), 0, stream, D,
                           RcStoreSink<Map>{logits, ld_s}, G.users_per_block, map);
      } else {
        hipLaunchKernelGGL((rc::sweep_kernel<Scorer, RcStoreSink<Map>, Map>), G.grid, dim3(rc::TILE), 0, stream, D,
                           RcStoreSink<Map>{logits, ld_s}, G.users_per_block, map);
      }
      CARCA_LAUNCH_CHECK();
      return CARCA_OK;
    });
    if (rc != CARCA_OK) return rc;
    hipLaunchKernelGGL((rc::rc_exclude_kernel<CarcaRecommendDesc, Map>), dim3(D.B), dim3(64), 0, stream, D, logits, ld_s,
                       map);
    CARCA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((rc::rc_select_kernel<CarcaRecommendDesc, Map>), dim3(D.B), dim3(rc::RC_SEL_THREADS), 0, stream, D,
                     logits, ld_s, map);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
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
