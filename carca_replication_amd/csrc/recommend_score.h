// The scoring and exclusion launches of a top-k call, shared by the calls that pick items per user (recommend.hip:
// carca_recommend, carca_recommend_among, carca_recommend_groups, carca_recommend_capped) and the call that picks users
// per item (recommend_users.hip: carca_recommend_users).  One copy of the sink and of the two launches, so a (user, item)
// pair's raw logit in the [B, n_slots] buffer has the same bits whichever call asked for it.
#pragma once
#include "catalogue_select.h"
#include "catalogue_sweep.h"

namespace rc {

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

// The scoring and exclusion launches.  n_slots: the columns of the logit buffer, n_items or the listed count; map: which
// item a column holds (the sweep asks it only for item(pos)); finder: where the exclusion launch finds an id's column --
// the map itself, or rc::GroupedItems over a grouped order, which is not ascending.  *out: the [B, n_slots] raw logits.
template <class Map, class Finder>
int rc_score(const CarcaRecommendDesc& D, Map map, Finder finder, int n_slots, hipStream_t stream, float** out) {
  // raw logits [B, n_slots]: stream scratch (or the capture's memory), consumed by the launches behind the scoring one
  const int ld_s = n_slots;
  const size_t bytes = std::max((size_t)D.B * (size_t)ld_s, (size_t)1) * sizeof(float);
  float* logits = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                          : carca_stream_scratch(stream, CARCA_SCRATCH_RECOMMEND, bytes));
  CARCA_CHECK_ARG(logits, "recommend: scratch allocation of %zu bytes failed", bytes);
  *out = logits;
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
    hipLaunchKernelGGL((rc::rc_exclude_kernel<CarcaRecommendDesc, Finder>), dim3(D.B), dim3(64), 0, stream, D, logits, ld_s,
                       finder);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}

}  // namespace rc
