// Per-user candidate lists (include/carca_hip.h: carca_score_lists / carca_recommend_lists).
//
// A second-stage ranker gets a list of its own per user: items [B, n_list].  carca_recommend_among shares one list among
// the batch and keeps an item tile in registers while the users walk by; here the USER is stationary -- staged in LDS once
// by the sweep's scorer (recommend_common.h) -- and the user's list streams through the lanes, one entry per lane and
// round of 256.  Every logit comes from the scorers' load_item / stage_user + logit (rc::CaScorer, rc::DotScorer) or the
// chunk protocol (rc::CaLongScorer, a profile of more than CARCA_MAX_L slots), so a (user, item) pair has the bits
// carca_recommend and carca_rank_items give it.  Three kernels, no host wait, nothing retained:
//   ls_score_kernel   grid (B, list chunks): a workgroup stages user u and walks rounds_per_wg rounds of its list.  Linked
//                     scores in caller order (carca_score_lists), or raw logits by position into the [B, n_list] stream
//                     scratch of the split path below;
//   ls_fused_kernel   carca_recommend_lists for n_list <= 1024, one workgroup per user and ONE launch: eligibility (the id
//                     is an item and not in the user's exclusion row, staged in LDS by pieces), the scoring rounds, the
//                     entries' 64-bit keys (rc::item_key; 0 = not eligible) into LDS, a bitonic sort descending, and a
//                     ballot + prefix compaction of the first k keys that differ from their predecessor: a repeated id
//                     has the same logit bits and so the same key, which the sort puts side by side.  rc::link on those k
//                     only.  No atomics, no scratch;
//   the split path    carca_recommend_lists over rows the caller has sorted (sorted_rows; any n_list): ls_score_kernel
//                     writes raw logits by position (the exclusion sentinel where the position is not live), then the
//                     exclusion and selection launches of catalogue_select.h run over the per-user map rc::UserLists: a
//                     row's live positions are ascending and distinct, which is what the radix select needs of
//                     rc::ListedItems.
// Integer LDS atomics only (the selection's histogram): results do not depend on scheduling.
#include "catalogue_select.h"
#include "catalogue_sweep.h"

namespace {

constexpr int LS_TILE = rc::TILE;
constexpr int LS_WAVES = LS_TILE / 64;
constexpr int LS_FUSED_MAX = 1024;  // longest list of the fused kernel (catalogue.LIST_FUSED_MAX)
constexpr int LS_EX_PIECE = 1024;   // exclusion ids the fused kernel holds in LDS at a time
static_assert(LS_FUSED_MAX % LS_TILE == 0 && LS_FUSED_MAX / LS_TILE <= 32, "a lane keeps one eligibility bit per round");
static_assert(LS_EX_PIECE % 4 == 0, "the exclusion piece is read as int4");

__device__ __forceinline__ bool ls_valid(int id, int n_items) { return id >= 1 && id < n_items; }

// entry idx of user u's list -> its id, and whether it is scored.  RAW (the split path): the rows are sorted and a
// position is live as rc::ListedRow says, a repeat of its predecessor being dead.
template <bool RAW>
__device__ __forceinline__ int ls_entry(const CarcaListsDesc& D, int u, long long idx, bool& live) {
  const int32_t* row = D.items + (size_t)u * D.ld_items;
  const bool in_list = idx < D.n_list;
  int id = 0;
  if (in_list) id = RAW ? rc::ListedRow{row, D.n_list}.item((int)idx) : row[idx];
  live = in_list && ls_valid(id, D.n_items);
  return id;
}

template <bool RAW>
__device__ __forceinline__ void ls_store(const CarcaListsDesc& D, float* out, int ld_out, int u, long long idx, bool live,
                                         float logit) {
  out[(size_t)u * ld_out + idx] = RAW ? (live ? logit : __uint_as_float(rc::RC_SENTINEL))
                                      : (live ? rc::link(logit, D.decoder) : 0.f);
}

// ---- 1. list scoring, user-stationary ------------------------------------------------------------------------------
// Workgroup (u, y) stages user u once and walks rounds [r0, r1) of the list, LS_TILE entries each; r0, r1 come from launch
// parameters and are workgroup-uniform.
// The chunked scorer (rc::CaLongScorer) follows rk_list_long_kernel's protocol: a lane past the end of the list, or at a
// dead entry, carries a dead item through the round, so every thread reaches every barrier, and the chunks are staged
// again in each round: a lane's (m, den, num) must see the user's slots in order.  Barriers: begin_user's two (the slot
// list is published); in front of every stage_chunk but the workgroup's very first, one (the chunk staged before it is
// read out); stage_chunk's two (K / u, then beta).  n_chunks() is workgroup-uniform (LDS words read after a barrier).
// The other scorers have no barrier behind stage_user: a lane past the end of the list skips the round.
template <class Scorer, bool RAW>
__global__ __launch_bounds__(LS_TILE) void ls_score_kernel(CarcaListsDesc D, float* __restrict__ out, int ld_out,
                                                           int rounds_per_wg) {
  __shared__ typename Scorer::User S;
  const int u = blockIdx.x, tid = threadIdx.x;
  const int rounds = (D.n_list - 1) / LS_TILE + 1;
  const int r0 = blockIdx.y * rounds_per_wg, r1 = min(rounds, r0 + rounds_per_wg);
  Scorer scorer(D);
  if constexpr (Scorer::chunked) {
    scorer.begin_user(D, u, S);
    const int nc = scorer.n_chunks();
    for (int r = r0; r < r1; ++r) {
      const long long idx = (long long)r * LS_TILE + tid;
      bool live;
      const int id = ls_entry<RAW>(D, u, idx, live);
      typename Scorer::Item I;
      scorer.load_item(D, id, live, I);
      typename Scorer::Acc A;
      scorer.reset(A);
      for (int c = 0; c < nc; ++c) {
        if (r > r0 || c) __syncthreads();  // the chunk staged before this one is read out
        scorer.stage_chunk(D, u, c, S);
        scorer.accumulate(I, S, c, A);
      }
      if (idx < D.n_list) ls_store<RAW>(D, out, ld_out, u, idx, live, scorer.finish(D, u, I, A));
    }
  } else {
    scorer.stage_user(D, u, S);
    for (int r = r0; r < r1; ++r) {
      const long long idx = (long long)r * LS_TILE + tid;
      if (idx >= D.n_list) continue;
      bool live;
      const int id = ls_entry<RAW>(D, u, idx, live);
      typename Scorer::Item I;
      scorer.load_item(D, id, live, I);
      ls_store<RAW>(D, out, ld_out, u, idx, live, live ? scorer.logit(D, u, I, S) : 0.f);
    }
  }
}

// ---- 2. fused small-list top-k -------------------------------------------------------------------------------------
template <class Scorer>
struct LsFusedLds {
  typename Scorer::User S;
  unsigned long long key[LS_FUSED_MAX];  // a thread owns the entries idx = tid (mod LS_TILE) until the sort
  int4 ex4[LS_EX_PIECE / 4];
  int wcnt[LS_WAVES];
};

// an eligible entry's key; order bits 0 are the exclusion sentinel's, which selection never picks (catalogue_select.h)
__device__ __forceinline__ unsigned long long ls_key(float logit, int id) {
  const unsigned o = rc::order_bits(__float_as_uint(logit));
  return o ? rc::order_key(o, (unsigned)id) : 0ull;
}

// One workgroup per user, n_list <= LS_FUSED_MAX.  `rounds`, P (the sorted length: the power of two >= n_list) and every
// loop bound in front of a barrier come from launch parameters; the chunked scorer's rounds follow ls_score_kernel's
// barrier accounting with r0 = 0.
template <class Scorer>
__global__ __launch_bounds__(LS_TILE) void ls_fused_kernel(CarcaListsDesc D) {
  static_assert(sizeof(LsFusedLds<Scorer>) <= 64 * 1024, "the fused kernel's LDS exceeds the static limit");
  __shared__ LsFusedLds<Scorer> Z;
  const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = D.n_list;
  if (n > LS_FUSED_MAX) return;  // (the host has checked it: Z.key holds no more)
  const int rounds = (n - 1) / LS_TILE + 1;
  const int32_t* row = D.items + (size_t)u * D.ld_items;
  int P = 2;
  while (P < n) P <<= 1;

  // eligibility: bit r of `dead` is set where the lane's entry of round r is past the end, no item, or excluded
  unsigned dead = 0u;
  for (int r = 0; r < rounds; ++r) {
    const int idx = r * LS_TILE + tid;
    Z.key[idx] = 0ull;
    if (idx >= n || !ls_valid(row[idx], D.n_items)) dead |= 1u << r;
  }
  for (int idx = rounds * LS_TILE + tid; idx < P; idx += LS_TILE) Z.key[idx] = 0ull;
  for (int base = 0; base < D.n_exclude; base += LS_EX_PIECE) {
    const int np = min(LS_EX_PIECE, D.n_exclude - base), np4 = (np + 3) / 4;
    if (base) __syncthreads();  // the previous piece is read out
    int* ex = reinterpret_cast<int*>(Z.ex4);
    for (int j = tid; j < 4 * np4; j += LS_TILE)  // (padded with 0, which no live entry equals)
      ex[j] = j < np ? D.exclude[(size_t)u * D.ld_exclude + base + j] : 0;
    __syncthreads();
    for (int r = 0; r < rounds; ++r) {
      if ((dead >> r) & 1u) continue;
      const int id = row[r * LS_TILE + tid];
      bool hit = false;
      for (int j = 0; j < np4; ++j) {
        const int4 e = Z.ex4[j];
        hit |= e.x == id || e.y == id || e.z == id || e.w == id;
      }
      if (hit) dead |= 1u << r;
    }
  }

  // scoring: the key of every eligible entry
  Scorer scorer(D);
  if constexpr (Scorer::chunked) {
    scorer.begin_user(D, u, Z.S);
    const int nc = scorer.n_chunks();
    for (int r = 0; r < rounds; ++r) {
      const int idx = r * LS_TILE + tid;
      const bool live = !((dead >> r) & 1u);
      const int id = live ? row[idx] : 0;
      typename Scorer::Item I;
      scorer.load_item(D, id, live, I);
      typename Scorer::Acc A;
      scorer.reset(A);
      for (int c = 0; c < nc; ++c) {
        if (r || c) __syncthreads();  // the chunk staged before this one is read out
        scorer.stage_chunk(D, u, c, Z.S);
        scorer.accumulate(I, Z.S, c, A);
      }
      const float logit = scorer.finish(D, u, I, A);
      if (live) Z.key[idx] = ls_key(logit, id);
    }
  } else {
    scorer.stage_user(D, u, Z.S);
    for (int r = 0; r < rounds; ++r) {
      if ((dead >> r) & 1u) continue;
      const int idx = r * LS_TILE + tid, id = row[idx];
      typename Scorer::Item I;
      scorer.load_item(D, id, true, I);
      Z.key[idx] = ls_key(scorer.logit(D, u, I, Z.S), id);
    }
  }
  __syncthreads();  // the keys are published

  // bitonic sort of key[0 .. P), descending; the zeros (not eligible, padding) end up last
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < P / 2; i += LS_TILE) {
        const int a = ((i & ~(stride - 1)) << 1) | (i & (stride - 1)), b = a | stride;
        const unsigned long long ka = Z.key[a], kb = Z.key[b];
        const bool desc = (a & size) == 0;
        if (desc ? (ka < kb) : (ka > kb)) Z.key[a] = kb, Z.key[b] = ka;
      }
      __syncthreads();
    }
  }

  // the first k keys that are non-zero and differ from their predecessor (a repeated id: the same key), in order
  int taken = 0;  // kept keys ahead of this round: summed by every thread from the same LDS words, workgroup-uniform
  for (int p0 = 0; p0 < P && taken < D.k; p0 += LS_TILE) {
    const int i = p0 + tid;
    const unsigned long long key = i < P ? Z.key[i] : 0ull;
    const bool keep = key != 0ull && (i == 0 || Z.key[i - 1] != key);
    const unsigned long long m = __ballot(keep);
    if (lane == 0) Z.wcnt[w] = __popcll(m);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int v = 0; v < LS_WAVES; ++v) {
      if (v == w) before = total;
      total += Z.wcnt[v];
    }
    const int at = taken + before + __popcll(m & ((1ull << lane) - 1ull));
    if (keep && at < D.k) {
      D.scores[(size_t)u * D.ld_scores + at] = rc::link(rc::unorder_bits((unsigned)(key >> 32)), D.decoder);
      D.ids_out[(size_t)u * D.ld_ids_out + at] = (int64_t)rc::key_id(key);
    }
    taken += total;
    __syncthreads();  // wcnt is read out
  }
  for (int t = taken + tid; t < D.k; t += LS_TILE) {  // fewer than k eligible items: padding
    D.scores[(size_t)u * D.ld_scores + t] = 0.f;
    D.ids_out[(size_t)u * D.ld_ids_out + t] = 0;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------
int ls_check(const CarcaListsDesc& D, const char* what) {
  if (int rc = rc::check_model(D, what)) return rc;
  CARCA_CHECK_ARG(D.n_list >= 1, "%s: n_list must be positive", what);
  CARCA_CHECK_ARG(D.items && D.ld_items >= D.n_list, "%s: null list or a row stride shorter than its row", what);
  return CARCA_OK;
}

template <bool RAW>
int ls_score(const CarcaListsDesc& D, const char* what, float* out, int ld_out, hipStream_t stream) {
  const rc::ListGrid G = rc::list_grid(D.n_list, D.B);  // (the rounds per workgroup: catalogue_sweep.h)
  return rc::dispatch_scorer(D, what, [&](auto scorer) -> int {
    using Scorer = typename decltype(scorer)::type;
    hipLaunchKernelGGL((ls_score_kernel<Scorer, RAW>), G.grid, dim3(LS_TILE), 0, stream, D, out, ld_out, G.rounds_per_wg);
    CARCA_LAUNCH_CHECK();
    return CARCA_OK;
  });
}

}  // namespace

extern "C" int carca_score_lists(const CarcaListsDesc* desc, void* stream) {
  CARCA_CHECK_ARG(desc, "score_lists: null descriptor");
  const CarcaListsDesc& D = *desc;
  if (int rc = ls_check(D, "score_lists")) return rc;
  CARCA_CHECK_ARG(D.scores && D.ld_scores >= D.n_list, "score_lists: null scores or a row stride shorter than its row");
  return ls_score<false>(D, "score_lists", D.scores, D.ld_scores, (hipStream_t)stream);
}

extern "C" int carca_recommend_lists(const CarcaListsDesc* desc, void* stream_) {
  CARCA_CHECK_ARG(desc, "recommend_lists: null descriptor");
  const CarcaListsDesc& D = *desc;
  hipStream_t stream = (hipStream_t)stream_;
  if (int rc = ls_check(D, "recommend_lists")) return rc;
  CARCA_CHECK_ARG(D.k >= 1, "recommend_lists: k must be positive");
  CARCA_CHECK_SUPPORTED(D.k <= rc::RC_KMAX, "recommend_lists: k = %d exceeds the largest k, 128", D.k);
  CARCA_CHECK_ARG(D.scores && D.ids_out, "recommend_lists: null pointer");
  CARCA_CHECK_ARG(D.ld_scores >= D.k && D.ld_ids_out >= D.k, "recommend_lists: row stride shorter than its row");
  if (!D.sorted_rows) {
    CARCA_CHECK_SUPPORTED(D.n_list <= LS_FUSED_MAX,
                          "recommend_lists: n_list = %d exceeds %d: sort the rows and set sorted_rows", D.n_list,
                          LS_FUSED_MAX);
    return rc::dispatch_scorer(D, "recommend_lists", [&](auto scorer) -> int {
      using Scorer = typename decltype(scorer)::type;
      hipLaunchKernelGGL(ls_fused_kernel<Scorer>, dim3(D.B), dim3(LS_TILE), 0, stream, D);
      CARCA_LAUNCH_CHECK();
      return CARCA_OK;
    });
  }
  // raw logits [B, n_list] by position: stream scratch (or the capture's memory), consumed by the two launches behind
  const size_t bytes = (size_t)D.B * (size_t)D.n_list * sizeof(float);
  float* logits = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                          : carca_stream_scratch(stream, CARCA_SCRATCH_LISTS, bytes));
  CARCA_CHECK_ARG(logits, "recommend_lists: scratch allocation of %zu bytes failed", bytes);
  if (int rc = ls_score<true>(D, "recommend_lists", logits, D.n_list, stream)) return rc;
  const rc::UserLists map{D.items, D.n_list, D.ld_items};
  hipLaunchKernelGGL((rc::rc_exclude_kernel<CarcaListsDesc, rc::UserLists>), dim3(D.B), dim3(64), 0, stream, D, logits,
                     D.n_list, map);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL((rc::rc_select_kernel<CarcaListsDesc, rc::UserLists>), dim3(D.B), dim3(rc::RC_SEL_THREADS), 0, stream,
                     D, logits, D.n_list, map);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
