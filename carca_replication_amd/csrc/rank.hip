// Exact full-catalogue ranks of listed items (include/carca_hip.h: carca_rank_items).
//
// The full-ranking protocol asks where the held-out item lands among all items; carca_recommend answers a different
// question (the k best) and cannot place an item beyond k = 128.  Here the rank of a target is a count: the eligible items
// whose key (recommend_common.h: logit bits, then the complemented id) is larger than the target's.  Every logit comes from
// the same helpers as carca_recommend's, so the two calls agree bit for bit.  Three launches, no host wait, nothing
// retained:
//   1. list scoring, one workgroup per user: the n_list targets and the n_exclude excluded entries are scored with the
//      user staged in LDS by the sweep's scorer (a cross-attention profile of more than CARCA_MAX_L slots: in chunks,
//      rk_list_long_kernel); their keys go to stream scratch, the targets' linked scores to `scores`, and the user's
//      [n_list] counter is zeroed;
//   2. counting sweep, recommend's sweep kernel (catalogue_sweep.h: a 256-item tile in registers walking a chunk of
//      users) with the sink below: each lane compares its item's key with the user's target keys (LDS), a wave counts
//      with ballot + popcount, the four waves sum in LDS and one integer atomic per (workgroup, user, target) with a
//      non-zero count goes to the counter (rc::count_larger).  No exclusion test (id 0 is never live) and no
//      [B, n_items] buffer;
//   3. correction, one workgroup per user: the distinct excluded ids (not 0, inside [0, n_items)) whose key is larger than
//      the target's are subtracted; an excluded target has its own key, which is not larger than itself.
// Integer atomics only: the counts do not depend on scheduling.
//
// carca_rank_items_among counts among a candidate list S (ascending, distinct ids) through the item map rc::ListedItems:
// launch 1 is unchanged (targets and excluded entries are scored by id, in S or not), the counting sweep runs over S
// (a lane at position p owns item ids[p]; keys carry the real id), and the correction subtracts only excluded ids that S
// holds (binary search): the others were never counted.
#include "catalogue_sweep.h"

namespace {

constexpr int RK_TILE = rc::TILE;
constexpr int RK_EX_CHUNK = 1024;  // exclusion keys the correction holds in LDS at a time

// scratch row per user: the n_list target keys, then the n_exclude exclusion keys (0 = no entry / invalid)
struct RkScratch {
  unsigned long long* keys;
  int ldk;
  int* counts;  // [B, n_list]
};

__device__ __forceinline__ bool rk_valid(int id, int n_items) { return id >= 1 && id < n_items; }

__device__ __forceinline__ int rk_list_id(const CarcaRankDesc& D, int u, int idx) {
  return idx < D.n_list ? D.items[(size_t)u * D.ld_items + idx] : D.exclude[(size_t)u * D.ld_exclude + idx - D.n_list];
}

__device__ __forceinline__ void rk_store_list(const CarcaRankDesc& D, RkScratch W, int u, int idx, int id, bool valid,
                                              float logit) {
  const bool target = idx < D.n_list;
  W.keys[(size_t)u * W.ldk + idx] = valid ? rc::item_key(logit, id) : (target ? rc::KEY_NEVER : 0ull);
  if (target) D.scores[(size_t)u * D.ld_scores + idx] = valid ? rc::link(logit, D.decoder) : 0.f;
}

// ---- 1. list scoring ---------------------------------------------------------------------------------------------
template <class Scorer>
__global__ __launch_bounds__(RK_TILE) void rk_list_kernel(CarcaRankDesc D, RkScratch W) {
  __shared__ typename Scorer::User S;
  const int u = blockIdx.x, tid = threadIdx.x;
  Scorer scorer(D);
  for (int t = tid; t < D.n_list; t += RK_TILE) W.counts[(size_t)u * D.n_list + t] = 0;
  scorer.stage_user(D, u, S);
  for (int idx = tid; idx < D.n_list + D.n_exclude; idx += RK_TILE) {
    const int id = rk_list_id(D, u, idx);
    const bool valid = rk_valid(id, D.n_items);
    typename Scorer::Item I;
    scorer.load_item(D, id, valid, I);
    rk_store_list(D, W, u, idx, id, valid, scorer.logit(D, u, I, S));
  }
}

// rk_list_kernel for a chunked scorer (rc::CaLongScorer).  The list is walked in rounds of RK_TILE entries with a
// trip count that is the same for the whole workgroup (n_list + n_exclude is a launch parameter), and a thread past
// the end of the list carries a dead item through the round, so every thread reaches every barrier.  The chunks are
// staged again in each round: a lane's (m, den, num) must see the user's slots in order.  Barriers: begin_user's two
// (the slot list is published); in front of every stage_chunk but the very first, one (the chunk staged before it is
// read out); stage_chunk's two (K / u, then beta).  n_chunks() is workgroup-uniform (LDS words read after a barrier).
template <class Scorer>
__global__ __launch_bounds__(RK_TILE) void rk_list_long_kernel(CarcaRankDesc D, RkScratch W) {
  __shared__ typename Scorer::User S;
  const int u = blockIdx.x, tid = threadIdx.x;
  Scorer scorer(D);
  for (int t = tid; t < D.n_list; t += RK_TILE) W.counts[(size_t)u * D.n_list + t] = 0;
  scorer.begin_user(D, u, S);
  const int n = D.n_list + D.n_exclude, nc = scorer.n_chunks();
  for (int base = 0; base < n; base += RK_TILE) {
    const int idx = base + tid;
    const bool listed = idx < n;
    const int id = listed ? rk_list_id(D, u, idx) : 0;
    const bool valid = listed && rk_valid(id, D.n_items);
    typename Scorer::Item I;
    scorer.load_item(D, id, valid, I);
    typename Scorer::Acc A;
    scorer.reset(A);
    for (int c = 0; c < nc; ++c) {
      if (base || c) __syncthreads();  // the chunk staged before this one is read out
      scorer.stage_chunk(D, u, c, S);
      scorer.accumulate(I, S, c, A);
    }
    if (listed) rk_store_list(D, W, u, idx, id, valid, scorer.finish(D, u, I, A));
  }
}

// ---- 2. the counting sweep's sink ----------------------------------------------------------------------------------
struct RkCountSink {
  using Desc = CarcaRankDesc;
  using Lds = rc::CountLds;
  RkScratch W;
  // the user's target keys into LDS (before the user's staging, whose barriers publish them)
  __device__ __forceinline__ void begin_user(const Desc& D, int u, Lds& C) const {
    for (int t = threadIdx.x; t < D.n_list; t += RK_TILE) C.tkey[t] = W.keys[(size_t)u * W.ldk + t];
  }
  __device__ __forceinline__ void put(const Desc& D, int u, int, int item, bool live, float logit, Lds& C) const {
    const unsigned long long key[1] = {live ? rc::item_key(logit, item) : 0ull};
    rc::count_larger(key, D.n_list, W.counts + (size_t)u * D.n_list, C);
  }
};

// ---- 3. correction -------------------------------------------------------------------------------------------------
template <class Map>
__global__ __launch_bounds__(RK_TILE) void rk_correct_kernel(CarcaRankDesc D, RkScratch W, Map map) {
  __shared__ unsigned long long ekey[RK_EX_CHUNK];
  const int u = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* row = W.keys + (size_t)u * W.ldk;
  const int32_t* ex = D.exclude + (size_t)u * D.ld_exclude;
  const unsigned long long tk = tid < D.n_list ? row[tid] : rc::KEY_NEVER;
  int corr = 0;
  for (int base = 0; base < D.n_exclude; base += RK_EX_CHUNK) {
    const int n = min(RK_EX_CHUNK, D.n_exclude - base);
    __syncthreads();  // the previous chunk is read out
    for (int j = tid; j < n; j += RK_TILE) {  // keep an entry's key only at the first occurrence of its id
      const int e = base + j, id = ex[e];
      bool first = rk_valid(id, D.n_items) && map.find(id) >= 0;  // (an id the sweep did not count is not subtracted)
      for (int e2 = 0; first && e2 < e; ++e2) first = ex[e2] != id;
      ekey[j] = first ? row[D.n_list + e] : 0ull;
    }
    __syncthreads();
    if (tid < D.n_list)
      for (int j = 0; j < n; ++j) corr += ekey[j] > tk;
  }
  if (tid < D.n_list) {
    const int id = D.items[(size_t)u * D.ld_items + tid];
    D.ranks[(size_t)u * D.ld_ranks + tid] =
        rk_valid(id, D.n_items) ? (int64_t)(W.counts[(size_t)u * D.n_list + tid] - corr) : (int64_t)-1;
  }
}

// n_slots: the positions the counting sweep covers, n_items or the candidate count
template <class Map>
int rk_run(const CarcaRankDesc& D, Map map, int n_slots, hipStream_t stream) {
  if (int rc = rc::check_model(D, "rank_items")) return rc;
  CARCA_CHECK_SUPPORTED(D.n_list >= 1 && D.n_list <= rc::LIST_MAX, "rank_items: n_list = %d outside 1..128", D.n_list);
  CARCA_CHECK_ARG(D.items && D.scores && D.ranks, "rank_items: null pointer");
  CARCA_CHECK_ARG(D.ld_items >= D.n_list && D.ld_scores >= D.n_list && D.ld_ranks >= D.n_list,
                  "rank_items: row stride shorter than its row");
  // scratch: the [B, n_list] counters, then the [B, n_list + n_exclude] keys
  RkScratch W;
  W.ldk = D.n_list + D.n_exclude;
  const size_t count_bytes = ((size_t)D.B * D.n_list * sizeof(int) + 255) / 256 * 256;
  const size_t bytes = count_bytes + (size_t)D.B * (size_t)W.ldk * sizeof(unsigned long long);
  char* base = (char*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                      : carca_stream_scratch(stream, CARCA_SCRATCH_RANK, bytes));
  CARCA_CHECK_ARG(base, "rank_items: scratch allocation of %zu bytes failed", bytes);
  W.counts = (int*)base;
  W.keys = (unsigned long long*)(base + count_bytes);
  const rc::SweepGrid G = rc::sweep_grid(std::max(n_slots, 1), D.B);
  const int rc = rc::dispatch_scorer(D, "rank_items", [&](auto scorer) -> int {
    using Scorer = typename decltype(scorer)::type;
    if constexpr (Scorer::chunked) {  // cross-attention over a profile of more than CARCA_MAX_L slots
      hipLaunchKernelGGL(rk_list_long_kernel<Scorer>, dim3(D.B), dim3(RK_TILE), 0, stream, D, W);
    } else {
      hipLaunchKernelGGL(rk_list_kernel<Scorer>, dim3(D.B), dim3(RK_TILE), 0, stream, D, W);
    }
    CARCA_LAUNCH_CHECK();
    if (n_slots == 0) return CARCA_OK;  // (an empty candidate list: no tile to sweep, every count stays 0)
    if constexpr (Scorer::chunked) {
      hipLaunchKernelGGL((rc::sweep_long_kernel<Scorer, RkCountSink, Map>), G.grid, dim3(RK_TILE), 0, stream, D,
                         RkCountSink{W}, G.users_per_block, map);
    } else {
      hipLaunchKernelGGL((rc::sweep_kernel<Scorer, RkCountSink, Map>), G.grid, dim3(RK_TILE), 0, stream, D, RkCountSink{W},
                         G.users_per_block, map);
    }
    CARCA_LAUNCH_CHECK();
    return CARCA_OK;
  });
  if (rc != CARCA_OK) return rc;
  hipLaunchKernelGGL(rk_correct_kernel<Map>, dim3(D.B), dim3(RK_TILE), 0, stream, D, W, map);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_rank_items(const CarcaRankDesc* desc, void* stream) {
  CARCA_CHECK_ARG(desc, "rank_items: null descriptor");
  return rk_run(*desc, rc::AllItems{}, desc->n_items, (hipStream_t)stream);
}

extern "C" int carca_rank_items_among(const CarcaRankDesc* desc, const CarcaCandidates* cand, void* stream) {
  CARCA_CHECK_ARG(desc, "rank_items: null descriptor");
  if (int rc = rc::check_candidates(cand, "rank_items")) return rc;
  return rk_run(*desc, rc::ListedItems{cand->ids, cand->n}, cand->n, (hipStream_t)stream);
}
