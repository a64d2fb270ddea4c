// Several request contexts per user (include/carca_hip.h: carca_score_lists_at / carca_recommend_at /
// carca_recommend_among_at).
//
// The candidate's context enters a logit only through M c (recommend_common.h): K, u, the scored profile row and the
// head dot products QT[i]_h . K_hl are the same under every context of a user.  The scorers here (rc::CaContextScorer,
// rc::DotContextScorer) stage the context-free share of a user once, the context rows of CarcaContexts up to NC at a
// time, and compute each (head, slot) dot product once per item; every piece of arithmetic is the single-context
// scorers' own (ca_slot_dot, ca_slot_bias, ca_online_update, ca_slot_beta, ca_logit_offsets; dot_row, dot_finish,
// dot_stage_am), so the logit of (user u under context c, item i) has the bits carca_recommend / carca_score_lists give
// that pair from a descriptor holding row u * C + c.  Two kernels:
//   cx_list_kernel    ls_score_kernel's grid (recommend_lists.hip): workgroup (u, y) stages user u once and walks its
//                     rounds of the list, one entry per lane; per entry the C linked scores, or (BEST) the arg-max over
//                     the contexts by (rc::order_bits(logit), smaller c) and its linked score -- no [B, C, N] buffer;
//   cx_sweep_kernel   rc::sweep_kernel's shape: a 256-item tile in registers walks a chunk of users; raw logits of row
//                     u * C + c go through rc::RcStoreSink into the [B * C, n_slots] scratch, and carca_recommend's
//                     exclusion and selection launches (catalogue_select.h) run over the B * C rows through a descriptor
//                     copy whose B is B * C (the caller has repeated a user's exclusion row for each of its contexts).
// More than NC contexts run in passes of NC; the user's K / u stay staged across the passes.  No atomics at all in the two
// kernels; the selection's integer LDS atomics are scheduling-independent.
#include "catalogue_select.h"
#include "catalogue_sweep.h"
#include "recommend_score.h"

namespace {

constexpr int CX_TILE = rc::TILE;

// Contexts a lane serves at a time: its item row (up to 128 floats) stays in registers beside 3 * NC softmax states of
// the head in flight and NC logits.  Eight for every geometry: none of the instantiations spills (DESIGN.md section 25
// has the compiler's resource table); a geometry that did would get a smaller NC here.
template <int DPI, int DHP, int H>
struct CxNc {
  static constexpr int value = 8;
};
constexpr int CX_NC_DOT = 8;

__device__ __forceinline__ bool cx_valid(int id, int n_items) { return id >= 1 && id < n_items; }

// ---- 1. list scoring under C contexts, user-stationary -------------------------------------------------------------
// Workgroup (u, y) stages user u's context-free share once and walks rounds [r0, r1) of the list, CX_TILE entries each.
// With one pass (C <= NC) the contexts are staged once in front of the rounds and a lane past the end of the list skips
// its round; with more, every (round, pass) stages its NC contexts again and every lane takes part, a lane past the end
// (or at an id that is no item) carrying a dead item.  Barriers: stage_user's; with one pass stage_contexts' one; with
// more, per (round, pass) one in front of stage_contexts but the very first (the contexts staged before are read out)
// and stage_contexts' own.  Every trip count in front of a barrier is workgroup-uniform: r0, r1 and passes come from
// launch parameters (rounds_per_wg, D.n_list, X.n_contexts), stage_user's nv from an LDS word read after a barrier.
template <class Scorer, bool BEST>
__global__ __launch_bounds__(CX_TILE) void cx_list_kernel(CarcaListsDesc D, CarcaContexts X, int64_t* __restrict__ best,
                                                          int ld_best, int rounds_per_wg) {
  static_assert(sizeof(typename Scorer::User) <= 64 * 1024, "the list kernel's LDS exceeds the static limit");
  constexpr int NC = Scorer::NC;
  __shared__ typename Scorer::User S;
  const int u = blockIdx.x, tid = threadIdx.x;
  const int C = X.n_contexts, passes = (C + NC - 1) / NC;
  const int rounds = (D.n_list - 1) / CX_TILE + 1;
  const int r0 = blockIdx.y * rounds_per_wg, r1 = min(rounds, r0 + rounds_per_wg);
  const int32_t* row = D.items + (size_t)u * D.ld_items;
  Scorer scorer(D);
  scorer.stage_user(D, u, S);
  if (passes == 1) scorer.stage_contexts(D, X, u, 0, C, S);
  for (int r = r0; r < r1; ++r) {
    const long long idx = (long long)r * CX_TILE + tid;
    const bool in_list = idx < D.n_list;
    if (passes == 1 && !in_list) continue;  // (no barrier behind this point in a one-pass launch)
    const int id = in_list ? row[idx] : 0;
    const bool live = in_list && cx_valid(id, D.n_items);
    typename Scorer::Item I;
    scorer.load_item(D, id, live, I);
    unsigned best_o = 0u;
    int best_c = -1;
    for (int p = 0; p < passes; ++p) {
      const int c0 = p * NC, ncx = min(NC, C - c0);
      if (passes > 1) {
        if (r > r0 || p) __syncthreads();  // the contexts staged before these are read out
        scorer.stage_contexts(D, X, u, c0, ncx, S);
      }
      float y[NC];
      if (live) scorer.logits(D, X, u, c0, ncx, I, S, y);
      if (!in_list) continue;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c >= ncx) continue;
        if constexpr (BEST) {
          const unsigned o = rc::order_bits(__float_as_uint(y[c]));
          if (live && (best_c < 0 || o > best_o)) best_o = o, best_c = c0 + c;  // (a tie keeps the smaller context)
        } else {
          D.scores[(size_t)u * D.ld_scores + (size_t)(c0 + c) * D.n_list + idx] = live ? rc::link(y[c], D.decoder) : 0.f;
        }
      }
    }
    if constexpr (BEST) {
      if (in_list) {
        D.scores[(size_t)u * D.ld_scores + idx] = best_c >= 0 ? rc::link(rc::unorder_bits(best_o), D.decoder) : 0.f;
        best[(size_t)u * ld_best + idx] = (int64_t)best_c;
      }
    }
  }
}

// ---- 2. the catalogue sweep under C contexts --------------------------------------------------------------------------
// rc::sweep_kernel with the users' contexts inside: the lane's item row stays in registers while the users of its chunk
// walk by; per user the context-free share is staged once and the contexts in passes of NC.  Row u * C + c of the
// [B * C, ld_s] buffer takes (user u, context c) through rc::RcStoreSink (the exclusion sentinel where it puts it).
// Barriers per user: the loop's own (the previous user's LDS is read out); stage_user's; per pass one in front of every
// pass but the first (the previous pass's contexts are read out) and stage_contexts' own.  u0, u1 and passes come from
// launch parameters (users_per_block, D.B, X.n_contexts): workgroup-uniform.
template <class Scorer, class Map>
__global__ __launch_bounds__(CX_TILE) void cx_sweep_kernel(CarcaRecommendDesc D, CarcaContexts X, rc::RcStoreSink<Map> sink,
                                                           int users_per_block, Map map) {
  static_assert(sizeof(typename Scorer::User) <= 64 * 1024, "the sweep's LDS exceeds the static limit");
  constexpr int NC = Scorer::NC;
  __shared__ typename Scorer::User S;
  typename rc::RcStoreSink<Map>::Lds none;
  Scorer scorer(D);
  const int pos = blockIdx.x * CX_TILE + threadIdx.x;
  const int item = map.item(pos);
  const bool live = item >= 1 && item < D.n_items;
  typename Scorer::Item I;
  scorer.load_item(D, item, live, I);
  const int C = X.n_contexts, passes = (C + NC - 1) / NC;
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous user's LDS is read out
    scorer.stage_user(D, u, S);
    for (int p = 0; p < passes; ++p) {
      const int c0 = p * NC, ncx = min(NC, C - c0);
      if (p) __syncthreads();  // the previous pass's contexts are read out
      scorer.stage_contexts(D, X, u, c0, ncx, S);
      float y[NC];
      scorer.logits(D, X, u, c0, ncx, I, S, y);
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < ncx) sink.put(D, u * C + c0 + c, pos, item, live, y[c], none);
    }
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
template <class Desc>
int cx_check(const Desc& D, const CarcaContexts* ctx, const char* what) {
  if (int rc = rc::check_model(D, what)) return rc;
  CARCA_CHECK_ARG(ctx, "%s: null contexts", what);
  const CarcaContexts& X = *ctx;
  CARCA_CHECK_ARG(X.n_contexts >= 1, "%s: n_contexts must be positive", what);
  CARCA_CHECK_SUPPORTED((long long)D.B * X.n_contexts < (1ll << 31), "%s: B * n_contexts = %lld does not fit an int", what,
                        (long long)D.B * X.n_contexts);
  if (D.decoder == 0) {
    CARCA_CHECK_SUPPORTED(D.L <= CARCA_MAX_L,
                          "%s: profile length L = %d exceeds CARCA_MAX_L = %d: the chunked scorer of longer profiles is "
                          "not served under several contexts (call the single-context entry point per context)",
                          what, D.L, CARCA_MAX_L);
    CARCA_CHECK_ARG(!X.user_q || (X.ld_user_q >= D.d && X.ld_user_q % 4 == 0), "%s: bad contexts ld_user_q", what);
    CARCA_CHECK_ARG(!X.user_off || X.ld_user_off >= 1, "%s: bad contexts ld_user_off", what);
  } else {
    CARCA_CHECK_ARG(!X.user_m || (X.ld_user_m >= D.d && X.ld_user_m % 4 == 0), "%s: bad contexts ld_user_m", what);
  }
  return CARCA_OK;
}

// launch(ScorerOf<Scorer>{}) for the descriptor's multi-context scorer (rc::dispatch_scorer's table; L <= CARCA_MAX_L)
template <int DPI, int DHP, int H, class Launch>
int cx_launch_ca(Launch& launch) {
  return launch(rc::ScorerOf<rc::CaContextScorer<DHP, H, CxNc<DPI, DHP, H>::value>>{});
}
template <class Desc, class Launch>
int cx_dispatch(const Desc& D, const char* what, Launch launch) {
  int dpi = 0, dhp = 0, dpo = 0;
  carca_padded_dims(D.d, D.H, &dpi, &dhp, &dpo);
  const int H = D.H;
  if (D.decoder == 0) {
    CARCA_ATT_DISPATCH(cx_launch_ca, launch);
    carca_set_error("%s: no cross-attention kernel for (dpi %d, dhp %d, H %d)", what, dpi, dhp, H);
    return CARCA_ERR_UNSUPPORTED;
  }
  if (dpi == 64) return launch(rc::ScorerOf<rc::DotContextScorer<64, CX_NC_DOT>>{});
  if (dpi == 96) return launch(rc::ScorerOf<rc::DotContextScorer<96, CX_NC_DOT>>{});
  return launch(rc::ScorerOf<rc::DotContextScorer<128, CX_NC_DOT>>{});
}

template <class Map>
int cx_recommend(const CarcaRecommendDesc& D, const CarcaContexts* ctx, Map map, int n_slots, hipStream_t stream) {
  const char* what = "recommend_at";
  if (int rc = cx_check(D, ctx, what)) return rc;
  const CarcaContexts& X = *ctx;
  const int C = X.n_contexts;
  CARCA_CHECK_ARG(D.k >= 1, "%s: k must be positive", what);
  CARCA_CHECK_SUPPORTED(D.k <= rc::RC_KMAX, "%s: k = %d exceeds the largest k, 128", what, D.k);
  CARCA_CHECK_SUPPORTED((long long)C * D.k < (1ll << 31), "%s: n_contexts * k does not fit an int", what);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "%s: null pointer", what);
  CARCA_CHECK_ARG(D.ld_scores == C * D.k && D.ld_ids_out == C * D.k,
                  "%s: the outputs are dense, ld_scores and ld_ids_out must be n_contexts * k = %d", what, C * D.k);
  // raw logits [B * C, n_slots]: stream scratch (or the capture's memory), consumed by the launches behind the sweep
  const size_t bytes = std::max((size_t)D.B * (size_t)C * (size_t)n_slots, (size_t)1) * sizeof(float);
  float* logits = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                          : carca_stream_scratch(stream, CARCA_SCRATCH_RECOMMEND, bytes));
  CARCA_CHECK_ARG(logits, "%s: scratch allocation of %zu bytes failed", what, bytes);
  // the B * C rows as users of carca_recommend's own exclusion and selection launches: row u * C + c of the buffer, of
  // the exclusion list (repeated per context by the caller) and of the dense [B, C * k] outputs
  CarcaRecommendDesc R = D;
  R.B = D.B * C;
  R.ld_scores = D.k;
  R.ld_ids_out = D.k;
  if (n_slots > 0) {  // (an empty candidate list: no tile to sweep, selection finds no eligible item)
    const rc::SweepGrid G = rc::sweep_grid(n_slots, D.B);
    const int rc = cx_dispatch(D, what, [&](auto scorer) -> int {
      using Scorer = typename decltype(scorer)::type;
      hipLaunchKernelGGL((cx_sweep_kernel<Scorer, Map>), G.grid, dim3(CX_TILE), 0, stream, D, X,
                         rc::RcStoreSink<Map>{logits, n_slots}, G.users_per_block, map);
      CARCA_LAUNCH_CHECK();
      return CARCA_OK;
    });
    if (rc != CARCA_OK) return rc;
    hipLaunchKernelGGL((rc::rc_exclude_kernel<CarcaRecommendDesc, Map>), dim3(R.B), dim3(64), 0, stream, R, logits, n_slots,
                       map);
    CARCA_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL((rc::rc_select_kernel<CarcaRecommendDesc, Map>), dim3(R.B), dim3(rc::RC_SEL_THREADS), 0, stream, R,
                     logits, n_slots, map);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_score_lists_at(const CarcaListsDesc* desc, const CarcaContexts* contexts, int64_t* best_context,
                                    int ld_best_context, void* stream_) {
  const char* what = "score_lists_at";
  CARCA_CHECK_ARG(desc, "%s: null descriptor", what);
  const CarcaListsDesc& D = *desc;
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = cx_check(D, contexts, what)) return rc;
  const CarcaContexts& X = *contexts;
  CARCA_CHECK_ARG(D.n_list >= 1, "%s: n_list must be positive", what);
  CARCA_CHECK_ARG(D.items && D.ld_items >= D.n_list, "%s: null list or a row stride shorter than its row", what);
  const long long cols = best_context ? (long long)D.n_list : (long long)X.n_contexts * D.n_list;
  CARCA_CHECK_SUPPORTED(cols < (1ll << 31), "%s: n_contexts * n_list = %lld does not fit an int", what, cols);
  CARCA_CHECK_ARG(D.scores && D.ld_scores >= cols, "%s: null scores or a row stride shorter than its row", what);
  CARCA_CHECK_ARG(!best_context || ld_best_context >= D.n_list, "%s: ld_best_context shorter than its row", what);
  const rc::ListGrid G = rc::list_grid(D.n_list, D.B);
  return cx_dispatch(D, what, [&](auto scorer) -> int {
    using Scorer = typename decltype(scorer)::type;
    if (best_context) {
      hipLaunchKernelGGL((cx_list_kernel<Scorer, true>), G.grid, dim3(CX_TILE), 0, stream, D, X, best_context,
                         ld_best_context, G.rounds_per_wg);
    } else {
      hipLaunchKernelGGL((cx_list_kernel<Scorer, false>), G.grid, dim3(CX_TILE), 0, stream, D, X, (int64_t*)nullptr, 0,
                         G.rounds_per_wg);
    }
    CARCA_LAUNCH_CHECK();
    return CARCA_OK;
  });
}

extern "C" int carca_recommend_at(const CarcaRecommendDesc* desc, const CarcaContexts* contexts, void* stream) {
  CARCA_CHECK_ARG(desc, "recommend_at: null descriptor");
  return cx_recommend(*desc, contexts, rc::AllItems{}, desc->n_items, (hipStream_t)stream);
}

extern "C" int carca_recommend_among_at(const CarcaRecommendDesc* desc, const CarcaContexts* contexts,
                                        const CarcaCandidates* cand, void* stream) {
  CARCA_CHECK_ARG(desc, "recommend_at: null descriptor");
  if (int rc = rc::check_candidates(cand, "recommend_at")) return rc;
  return cx_recommend(*desc, contexts, rc::ListedItems{cand->ids, cand->n}, cand->n, (hipStream_t)stream);
}
