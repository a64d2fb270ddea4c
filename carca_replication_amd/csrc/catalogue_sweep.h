// What carca_recommend (recommend.hip) and carca_rank_items (rank.hip) share around the per-pair arithmetic of
// recommend_common.h, and the counting step they share with carca_knn_rank_items (knn_catalogue.hip):
//   sweep_kernel   a 256-item tile in registers walks a chunk of users, stages each user in LDS and scores the pair.  The
//                  scorer (rc::CaScorer / rc::DotScorer; rc::CaLongScorer under sweep_long_kernel, which stages a long
//                  profile in chunks) says how, the sink what becomes of the logit: recommend stores
//                  it, rank_items compares its key with the user's target keys; the item map (recommend_common.h:
//                  rc::AllItems / rc::ListedItems) says which item a lane owns: the catalogue's, or a candidate list's;
//   count_larger   per target, the keys of the workgroup that are larger, one integer atomic per target;
//   host side      the model-side descriptor checks, the exclusion-list check, the sweep grid and the dispatch from a
//                  descriptor's (decoder, d, H) to a scorer type.
// A sink has: Desc, Lds (its own LDS block), begin_user (before the user's staging, whose barriers publish what it
// writes) and put (every thread of the workgroup, live or not; pos is the lane's position under the map, item its id).
#pragma once
#include "recommend_common.h"

namespace rc {

// ---- the sweep ---------------------------------------------------------------------------------------------------
template <class Scorer, class Sink, class Map = AllItems>
__global__ __launch_bounds__(TILE) void sweep_kernel(typename Sink::Desc D, Sink sink, int users_per_block, Map map) {
  __shared__ typename Scorer::User S;
  __shared__ typename Sink::Lds C;
  Scorer scorer(D);
  const int pos = blockIdx.x * TILE + threadIdx.x;
  const int item = map.item(pos);
  const bool live = item >= 1 && item < D.n_items;
  typename Scorer::Item I;
  scorer.load_item(D, item, live, I);
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous user's LDS is read out
    sink.begin_user(D, u, C);
    scorer.stage_user(D, u, S);
    sink.put(D, u, pos, item, live, scorer.logit(D, u, I, S), C);
  }
}

// sweep_kernel for a chunked scorer (rc::CaLongScorer: a profile of more than CARCA_MAX_L slots), same sinks and maps.
// Barriers per user: the loop's own (the previous user's LDS is read out); begin_user's two (the compacted slot list and
// the sink's LDS are published); per chunk, one in front of every chunk but the first (the previous chunk is read out)
// and stage_chunk's two (K / u, then beta).  Every trip count in front of a barrier is workgroup-uniform: u0, u1 come from
// launch parameters, n_chunks() from LDS words every thread reads after begin_user's barrier.
template <class Scorer, class Sink, class Map = AllItems>
__global__ __launch_bounds__(TILE) void sweep_long_kernel(typename Sink::Desc D, Sink sink, int users_per_block, Map map) {
  __shared__ typename Scorer::User S;
  __shared__ typename Sink::Lds C;
  Scorer scorer(D);
  const int pos = blockIdx.x * TILE + threadIdx.x;
  const int item = map.item(pos);
  const bool live = item >= 1 && item < D.n_items;
  typename Scorer::Item I;
  scorer.load_item(D, item, live, I);
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous user's LDS is read out
    sink.begin_user(D, u, C);
    scorer.begin_user(D, u, S);
    typename Scorer::Acc A;
    scorer.reset(A);
    const int nc = scorer.n_chunks();
    for (int c = 0; c < nc; ++c) {
      if (c) __syncthreads();  // the previous chunk is read out
      scorer.stage_chunk(D, u, c, S);
      scorer.accumulate(I, S, c, A);
    }
    sink.put(D, u, pos, item, live, scorer.finish(D, u, I, A), C);
  }
}

// ---- counting ----------------------------------------------------------------------------------------------------
struct CountLds {
  unsigned long long tkey[LIST_MAX];  // the user's target keys (the caller fills and publishes them)
  int wcnt[TILE / 64][LIST_MAX];
};

__device__ __forceinline__ void add_count(int* p, int s) { atomicAdd(p, s); }
__device__ __forceinline__ void add_count(int64_t* p, int s) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)s);
}

// Counts, per target t < n_list, the keys of the workgroup (TILE threads, NK keys each) that are larger than C.tkey[t]
// and adds every non-zero sum to counts[t]: ballot + popcount per wave, the waves summed in LDS, one atomic per target.
template <int NK, class Count>
__device__ __forceinline__ void count_larger(const unsigned long long (&key)[NK], int n_list, Count* counts, CountLds& C) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int c0 = 0, c1 = 0;  // lane l keeps the wave's count for targets l and l + 64
  for (int t = 0; t < n_list; ++t) {
    const unsigned long long tk = C.tkey[t];
    int pc = 0;
#pragma unroll
    for (int j = 0; j < NK; ++j) pc += __popcll(__ballot(key[j] > tk));
    if (t < 64) {
      c0 = lane == t ? pc : c0;
    } else {
      c1 = lane == t - 64 ? pc : c1;
    }
  }
  C.wcnt[w][lane] = c0;
  C.wcnt[w][lane + 64] = c1;
  __syncthreads();
  if (tid < n_list) {
    int s = 0;
#pragma unroll
    for (int v = 0; v < TILE / 64; ++v) s += C.wcnt[v][tid];
    if (s) add_count(&counts[tid], s);
  }
}

// ---- host side ---------------------------------------------------------------------------------------------------
template <class Desc>
int check_exclusion(const Desc& D, const char* what) {
  CARCA_CHECK_ARG(D.n_exclude >= 0 && (D.n_exclude == 0 || (D.exclude && D.ld_exclude >= D.n_exclude)),
                  "%s: bad exclusion list", what);
  return CARCA_OK;
}

// the model-side fields of CarcaRecommendDesc / CarcaRankDesc (same names)
template <class Desc>
int check_model(const Desc& D, const char* what) {
  CARCA_CHECK_ARG(D.B >= 1 && D.L >= 1 && D.n_items >= 1 && D.d >= 1 && D.H >= 1,
                  "%s: B, L, n_items, d and H must be positive", what);
  CARCA_CHECK_SUPPORTED(D.L <= CARCA_MAX_PROFILE_L, "%s: profile length L = %d exceeds CARCA_MAX_PROFILE_L = %d", what, D.L,
                        CARCA_MAX_PROFILE_L);
  CARCA_CHECK_ARG(D.decoder >= 0 && D.decoder <= 2, "%s: decoder must be 0 (cross-attention), 1 (dot) or 2 (normalised dot)",
                  what);
  CARCA_CHECK_ARG(D.p_ids && D.item_q, "%s: null pointer", what);
  CARCA_CHECK_ARG(D.ld_p_ids >= D.L && D.ld_item_q >= D.d, "%s: row stride shorter than its row", what);
  CARCA_CHECK_ARG(D.ld_item_q % 4 == 0, "%s: ld_item_q must be a multiple of 4", what);
  if (int rc = check_exclusion(D, what)) return rc;
  CARCA_CHECK_SUPPORTED(D.d % D.H == 0 && D.d <= 128, "%s: d = %d, H = %d: no kernel (d %% H != 0 or d > 128)", what, D.d,
                        D.H);
  if (D.decoder == 0) {
    CARCA_CHECK_ARG(D.user_k && D.user_u && D.ld_user_k >= D.d && D.ld_user_u >= D.H && D.ld_user_k % 4 == 0,
                    "%s: cross-attention needs user_k / user_u", what);
    CARCA_CHECK_ARG(!D.user_q || (D.ld_user_q >= D.d && D.ld_user_q % 4 == 0), "%s: bad ld_user_q", what);
    CARCA_CHECK_ARG(!D.item_w || D.ld_item_w >= 1, "%s: bad ld_item_w", what);
    CARCA_CHECK_ARG(!D.user_off || D.ld_user_off >= 1, "%s: bad ld_user_off", what);
    CARCA_CHECK_SUPPORTED(carca_attn_geometry_built(D.d, D.H),
                          "%s: no cross-attention kernel built for d = %d, H = %d (see CARCA_ATT_GEOMETRIES)", what, D.d,
                          D.H);
  } else {
    CARCA_CHECK_ARG(D.user_q && D.ld_user_q >= D.d && D.ld_user_q % 4 == 0, "%s: dot decoders need user_q", what);
    CARCA_CHECK_ARG(!D.user_m || (D.ld_user_m >= D.d && D.ld_user_m % 4 == 0), "%s: bad ld_user_m", what);
  }
  return CARCA_OK;
}

// item tiles x user chunks, about two workgroups per CU; each workgroup keeps its tile's rows in registers.  n_slots is
// the map's size (n_items, or the candidate count: at least 1, an empty list launches no sweep)
struct SweepGrid {
  dim3 grid;
  int users_per_block;
};
inline SweepGrid sweep_grid(int n_slots, int B) {
  const int tiles = (n_slots + TILE - 1) / TILE;
  const int chunks = max(1, min(B, (2 * carca_num_cus() + tiles - 1) / tiles));
  const int upb = (B + chunks - 1) / chunks;
  return {dim3(tiles, (B + upb - 1) / upb), upb};
}

// The user-stationary list kernels (recommend_lists.hip, explain_lists.hip): users on the grid's x, list chunks on y.
// Workgroups per user: one for a list of up to two rounds of TILE entries; beyond, as many as bring the grid to about two
// workgroups per CU, each keeping at least two rounds so that a user's staging is shared.  Never more than 2 * CUs in y,
// whatever n_list.
struct ListGrid {
  dim3 grid;
  int rounds_per_wg;
};
inline ListGrid list_grid(int n_list, int B) {
  const int rounds = (n_list - 1) / TILE + 1;
  const int want = std::max(1, (2 * carca_num_cus() + B - 1) / B);
  const int chunks = std::max(1, std::min(want, rounds / 2));
  const int rpw = (rounds + chunks - 1) / chunks;
  return {dim3(B, (rounds + rpw - 1) / rpw), rpw};
}

// the candidate list of carca_recommend_among / carca_rank_items_among
inline int check_candidates(const CarcaCandidates* cand, const char* what) {
  CARCA_CHECK_ARG(cand, "%s: null candidate list", what);
  CARCA_CHECK_ARG(cand->n >= 0 && (cand->n == 0 || cand->ids), "%s: bad candidate list", what);
  return CARCA_OK;
}

// launch(ScorerOf<Scorer>{}) for the descriptor's scorer: one of CARCA_ATT_GEOMETRIES (CaScorer up to CARCA_MAX_L slots,
// CaLongScorer beyond), or one of the three dot widths (DotScorer reads no L)
template <class Scorer>
struct ScorerOf {
  using type = Scorer;
};
template <int DPI, int DHP, int H, class Launch>
int launch_ca(Launch& launch) {
  return launch(ScorerOf<CaScorer<DHP, H>>{});
}
template <int DPI, int DHP, int H, class Launch>
int launch_ca_long(Launch& launch) {
  return launch(ScorerOf<CaLongScorer<DHP, H>>{});
}
template <class Desc, class Launch>
int dispatch_scorer(const Desc& D, const char* what, Launch launch) {
  int dpi = 0, dhp = 0, dpo = 0;
  carca_padded_dims(D.d, D.H, &dpi, &dhp, &dpo);
  const int H = D.H;
  if (D.decoder == 0) {
    if (D.L <= CARCA_MAX_L) {  // the whole user in LDS
      CARCA_ATT_DISPATCH(launch_ca, launch);
    } else {  // the profile staged CARCA_MAX_L valid slots at a time
      CARCA_ATT_DISPATCH(launch_ca_long, launch);
    }
    carca_set_error("%s: no cross-attention kernel for (dpi %d, dhp %d, H %d)", what, dpi, dhp, H);
    return CARCA_ERR_UNSUPPORTED;
  }
  if (dpi == 64) return launch(ScorerOf<DotScorer<64>>{});
  if (dpi == 96) return launch(ScorerOf<DotScorer<96>>{});
  return launch(ScorerOf<DotScorer<128>>{});
}

}  // namespace rc
