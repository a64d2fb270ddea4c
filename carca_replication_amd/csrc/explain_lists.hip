// Which profile slots drive a cross-attention score (include/carca_hip.h: carca_explain_lists).
//
// In eval mode the decoder's logit is additive over the user's valid profile slots (carca.py:253-263, 338-347):
//   logit(u, i) = base(u, i) + sum_t c(u, i, t),   c(u, i, t) = sum_h w_h(u, i, t) U[u, t, h],
// with w_h head h's softmax weight of slot t (the reference's return_w), U the folded value the scorers stage (user_u) and
// base what rc::ca_logit_offsets adds.  The kernel has ls_score_kernel's shape (recommend_lists.hip): the user is stationary
// in LDS, staged by the sweep's scorer (rc::CaScorer, or rc::CaLongScorer's chunk protocol past CARCA_MAX_L slots), and the
// user's list streams through the lanes, one entry per lane and round of rc::TILE.  A lane makes two passes over the staged
// slots:
//   pass one   the scorer's own logit (logit_stats / accumulate + finish: score_items' bits), which leaves each head's
//              final (m, den) in registers;
//   pass two   rc::ca_slot_score again per slot -- the expression pass one ran -- and w = exp2(s - m) / den: the weights,
//              their sum over the heads against U, and either the dense rows or an 8-entry insertion list in registers.
// The file holds no copy of the slot arithmetic.  Dense rows go through an LDS tile per wave, EX_SUB slots of the wave's 64
// entries at a time, so that consecutive lanes store consecutive positions of a row; every position of a row is written
// (padding slots, invalid ids and empty profiles as 0), so the host needs no memset.  No atomics, no scratch buffer,
// results do not depend on scheduling.
//
// Barriers.  Every trip count in front of a barrier is workgroup-uniform: the rounds [r0, r1) come from launch parameters,
// the chunk count and the chunk sizes from LDS words every thread reads behind a barrier (nv), and a lane past the end of
// the list or at an id that is no item carries a dead item through the whole round, with either scorer: no thread leaves
// a round early.  In order: stage_user's barriers (rc::CaScorer) or begin_user's two (rc::CaLongScorer: the slot list is
// published); dense only, two for the position -> slot map; then per round and pass the chunk walk -- chunk c is staged
// unless it is the chunk in LDS already (`staged`, workgroup-uniform: a profile of one chunk is staged once per workgroup),
// behind one barrier (the chunk staged before it is read out) unless it is the workgroup's first, and stage_chunk's own
// two (K / u, then beta); dense only, two per tile: one behind the lanes' writes, one behind the wave's reads.
#include <type_traits>

#include "catalogue_sweep.h"

namespace {

constexpr int EX_TILE = rc::TILE;
constexpr int EX_WAVES = EX_TILE / 64;
constexpr int EX_TOP_MAX = 8;  // largest top_m (catalogue.EXPLAIN_TOP_MAX): the insertion list a lane keeps in registers

template <class T, class = void>
struct ex_is_ca : std::false_type {};
template <class T>
struct ex_is_ca<T, std::void_t<decltype(T::HEADS)>> : std::true_type {};

template <class Scorer>
constexpr int ex_inv_len() {
  return Scorer::chunked ? CARCA_MAX_PROFILE_L : CARCA_MAX_L;
}
// slots per tile: 32 where the scorer's block leaves the room, else 16
template <class Scorer>
constexpr int ex_sub() {
  return sizeof(typename Scorer::User) + ex_inv_len<Scorer>() * 4 + EX_WAVES * 64 * 33 * 4 + 64 <= 64 * 1024 ? 32 : 16;
}

template <class Scorer, bool DENSE>
struct ExLds {
  typename Scorer::User S;
};
template <class Scorer>
struct ExLds<Scorer, true> {
  typename Scorer::User S;
  int inv[ex_inv_len<Scorer>()];                   // profile position -> compacted slot, -1 at a padding slot
  float tile[EX_WAVES][64][ex_sub<Scorer>() + 1];  // [wave][entry][slot of the tile], rows padded to an odd stride
};

template <class Scorer>
__device__ __forceinline__ float ex_scale(const Scorer& scorer) {
  if constexpr (Scorer::chunked) {
    return scorer.base.sc;
  } else {
    return scorer.sc;
  }
}

// head h's softmax weight of staged slot j, from the head's final (m, den)
template <class Scorer>
__device__ __forceinline__ float ex_weight(const typename Scorer::Item& I, const typename Scorer::User& S, int h, int j,
                                           float sc, float m, float den) {
  return exp2f(rc::ca_slot_score<Scorer::HEAD_PAD, Scorer::HEADS>(I.q[h], S, h, j, sc) - m) / den;
}

// staged slot j's contribution to the logit: sum_h w_h U[j][h], heads in ascending order
template <class Scorer>
__device__ __forceinline__ float ex_contrib(const typename Scorer::Item& I, const typename Scorer::User& S, int j, float sc,
                                            const float (&m)[Scorer::HEADS], const float (&den)[Scorer::HEADS]) {
  float c = 0.f;
#pragma unroll
  for (int h = 0; h < Scorer::HEADS; ++h) c = fmaf(ex_weight<Scorer>(I, S, h, j, sc, m[h], den[h]), S.Us[j][h], c);
  return c;
}

// The wave stores positions [p0, p1) of its 64 entries' rows (rows + e * ld: entry e's row): the tile's value where the
// position is a valid slot (inv: compacted slots jfirst .. of the tile) and the entry is live, else 0.  Consecutive
// lanes take consecutive positions of a row.  inv == nullptr: zeros.
template <int TS1>
__device__ __forceinline__ void ex_store_rows(float* __restrict__ rows, int ld, const float (*tile)[TS1], const int* inv,
                                              int jfirst, int p0, int p1, unsigned long long livem,
                                              unsigned long long inm, int lane) {
  const int len = p1 - p0, total = 64 * len;
#pragma nounroll
  for (int i = lane; i < total; i += 64) {
    const int e = i / len, p = p0 + (i - e * len);
    if (!((inm >> e) & 1ull)) continue;  // past the end of the list
    const int j = inv ? inv[p] : -1;
    float v = 0.f;
    if (j >= 0 && ((livem >> e) & 1ull)) v = tile[e][j - jfirst];
    rows[(size_t)e * ld + p] = v;
  }
}

// Workgroup (u, y) stages user u and walks rounds [r0, r1) of its list, EX_TILE entries each.  DENSE: scores, base and
// the rows contrib [L], weights [H][L] of every entry; else scores, base and the top_m slots of every entry.
template <class Scorer, bool DENSE>
__global__ __launch_bounds__(EX_TILE) void ex_kernel(CarcaExplainDesc D, int rounds_per_wg) {
  constexpr int H = Scorer::HEADS;
  static_assert(sizeof(ExLds<Scorer, DENSE>) <= 64 * 1024, "the explain kernel's LDS exceeds the static limit");
  __shared__ ExLds<Scorer, DENSE> Z;
  typename Scorer::User& S = Z.S;
  const int u = blockIdx.x, tid = threadIdx.x;
  const int rounds = (D.n_list - 1) / EX_TILE + 1;
  const int r0 = blockIdx.y * rounds_per_wg, r1 = min(rounds, r0 + rounds_per_wg);
  Scorer scorer(D);
  int nc;      // chunks of the user's valid slots (CaScorer: one, or none for an empty profile)
  int staged;  // the chunk in LDS, -1 before the first
  if constexpr (Scorer::chunked) {
    scorer.begin_user(D, u, S);
    nc = scorer.n_chunks();
    staged = -1;
  } else {
    scorer.stage_user(D, u, S);
    nc = scorer.nv > 0;
    staged = 0;
  }
  const int nv = scorer.nv;
  const float sc = ex_scale(scorer);
  auto stage = [&](int c) {
    if constexpr (Scorer::chunked) {
      if (staged != c) {
        if (staged >= 0) __syncthreads();  // the chunk staged before this one is read out
        scorer.stage_chunk(D, u, c, S);
        staged = c;
      }
    }
  };
  auto chunk_size = [&](int c) {
    if constexpr (Scorer::chunked) {
      return scorer.chunk_size(c);
    } else {
      return nv;
    }
  };
  if constexpr (DENSE) {
    for (int p = tid; p < D.L; p += EX_TILE) Z.inv[p] = -1;
    __syncthreads();
    for (int j = tid; j < nv; j += EX_TILE) Z.inv[S.slot[j]] = j;
    __syncthreads();
  }

  for (int r = r0; r < r1; ++r) {
    const long long idx = (long long)r * EX_TILE + tid;
    const bool in_list = idx < D.n_list;
    int id = 0;
    if (in_list) id = D.items[(size_t)u * D.ld_items + idx];
    const bool live = in_list && id >= 1 && id < D.n_items;
    typename Scorer::Item I;
    scorer.load_item(D, id, live, I);

    // pass one: the scorer's logit and each head's final (m, den)
    float m[H], den[H], logit;
    if constexpr (Scorer::chunked) {
      typename Scorer::Acc A;
      scorer.reset(A);
      for (int c = 0; c < nc; ++c) {
        stage(c);
        scorer.accumulate(I, S, c, A);
      }
      logit = scorer.finish(D, u, I, A);
#pragma unroll
      for (int h = 0; h < H; ++h) m[h] = A.m[h], den[h] = A.den[h];
    } else {
      typename Scorer::Stats T;
#pragma unroll
      for (int h = 0; h < H; ++h) T.m[h] = 0.f, T.den[h] = 1.f;
      logit = scorer.logit_stats(D, u, I, S, T);
#pragma unroll
      for (int h = 0; h < H; ++h) m[h] = T.m[h], den[h] = T.den[h];
    }
    if (in_list) {
      D.scores[(size_t)u * D.ld_scores + idx] = live ? rc::link(logit, D.decoder) : 0.f;
      D.base[(size_t)u * D.ld_base + idx] = live ? rc::ca_logit_offsets(D, u, I.off) : 0.f;
    }

    // pass two
    if constexpr (DENSE) {
      constexpr int TS = ex_sub<Scorer>();
      const int lane = tid & 63, w = tid >> 6;
      const unsigned long long livem = __ballot(live), inm = __ballot(in_list);
      const size_t e0 = (size_t)r * EX_TILE + w * 64;  // the wave's first entry
      float* crow = D.contrib + ((size_t)u * D.n_list + e0) * D.ld_contrib;
      float* wrow = D.weights + ((size_t)u * H * D.n_list + e0) * D.ld_weights;  // head h: + h * n_list rows
      const size_t whead = (size_t)D.n_list * D.ld_weights;
      for (int c = 0; c < nc; ++c) {
        stage(c);
        const int n = chunk_size(c), jg = c * CARCA_MAX_L;
        for (int j0 = 0; j0 < n; j0 += TS) {
          const int cnt = min(TS, n - j0), jf = jg + j0;
          // the positions this tile's rows cover: from behind the previous tile's last slot to its own last slot, and
          // the profile's two ends
          const int p0 = jf == 0 ? 0 : S.slot[jf - 1] + 1;
          const int p1 = jf + cnt >= nv ? D.L : S.slot[jf + cnt - 1] + 1;
          // one stream at a time through the tile: 0 the contributions, 1 + h head h's weights.  The loop stays rolled
          // (one copy of the store), and the head a stream reads is picked by constants: q is never indexed at run time
#pragma nounroll
          for (int s = 0; s <= H; ++s) {
            if (s == 0) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
              for (int t = 0; t < cnt; ++t) Z.tile[w][lane][t] = ex_contrib<Scorer>(I, S, j0 + t, sc, m, den);
            }
#pragma unroll
            for (int h = 0; h < H; ++h) {
              if (s == h + 1) {
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
                for (int t = 0; t < cnt; ++t) Z.tile[w][lane][t] = ex_weight<Scorer>(I, S, h, j0 + t, sc, m[h], den[h]);
              }
            }
            __syncthreads();  // the tile is written
            ex_store_rows(s == 0 ? crow : wrow + (size_t)(s - 1) * whead, s == 0 ? D.ld_contrib : D.ld_weights, Z.tile[w],
                          Z.inv, jf, p0, p1, livem, inm, lane);
            __syncthreads();  // the tile is read out
          }
        }
      }
      if (nc == 0) {  // an empty profile: rows of zeros (carca.py:256)
#pragma nounroll
        for (int s = 0; s <= H; ++s)
          ex_store_rows(s == 0 ? crow : wrow + (size_t)(s - 1) * whead, s == 0 ? D.ld_contrib : D.ld_weights, Z.tile[w],
                        nullptr, 0, 0, D.L, livem, inm, lane);
      }
    } else {
      // the EX_TOP_MAX largest contributions so far, descending; the slots come by in ascending position, and a slot
      // that equals an entry goes in front of it: ties to the later slot.  Indexed by constants only.
      float tc[EX_TOP_MAX];
      int tp[EX_TOP_MAX];
#pragma unroll
      for (int i = 0; i < EX_TOP_MAX; ++i) tc[i] = -INFINITY, tp[i] = -1;
      for (int c = 0; c < nc; ++c) {
        stage(c);
        const int n = chunk_size(c), jg = c * CARCA_MAX_L;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
        for (int j = 0; j < n; ++j) {
          float cv = ex_contrib<Scorer>(I, S, j, sc, m, den);
          int cp = S.slot[jg + j];
#pragma unroll
          for (int i = 0; i < EX_TOP_MAX; ++i) {
            const bool up = cv >= tc[i];
            const float oc = tc[i];
            const int op = tp[i];
            tc[i] = up ? cv : oc, tp[i] = up ? cp : op;
            cv = up ? oc : cv, cp = up ? op : cp;
          }
        }
      }
      if (in_list) {
        const size_t row = (size_t)u * D.n_list + idx;
#pragma unroll
        for (int i = 0; i < EX_TOP_MAX; ++i) {
          if (i < D.top_m) {
            const bool has = live && tp[i] >= 0;
            D.slots[row * D.ld_slots + i] = has ? (int64_t)tp[i] : (int64_t)-1;
            D.slot_items[row * D.ld_slot_items + i] = has ? (int64_t)D.p_ids[(size_t)u * D.ld_p_ids + tp[i]] : (int64_t)0;
            D.contrib[row * D.ld_contrib + i] = has ? tc[i] : 0.f;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int carca_explain_lists(const CarcaExplainDesc* desc, void* stream) {
  CARCA_CHECK_ARG(desc, "explain_lists: null descriptor");
  const CarcaExplainDesc& D = *desc;
  const char* what = "explain_lists";
  if (int rc = rc::check_model(D, what)) return rc;
  CARCA_CHECK_SUPPORTED(D.decoder == 0,
                        "%s: decoder %d is a dot decoder: its score reads the last profile slot only (carca.py:362), "
                        "there is nothing to decompose", what, D.decoder);
  CARCA_CHECK_ARG(D.n_list >= 1, "%s: n_list must be positive", what);
  CARCA_CHECK_ARG(D.items && D.ld_items >= D.n_list, "%s: null list or a row stride shorter than its row", what);
  CARCA_CHECK_ARG(D.scores && D.base && D.ld_scores >= D.n_list && D.ld_base >= D.n_list,
                  "%s: null scores / base or a row stride shorter than its row", what);
  const bool dense = D.weights != nullptr, top = D.slots != nullptr || D.slot_items != nullptr;
  CARCA_CHECK_ARG(dense != top, "%s: give either weights (the dense rows) or slots and slot_items (the top_m slots)", what);
  CARCA_CHECK_ARG(D.contrib, "%s: null contrib", what);
  if (dense) {
    CARCA_CHECK_ARG(D.ld_contrib >= D.L && D.ld_weights >= D.L, "%s: row stride shorter than L", what);
  } else {
    CARCA_CHECK_SUPPORTED(D.top_m >= 1 && D.top_m <= EX_TOP_MAX, "%s: top_m = %d outside 1..%d", what, D.top_m, EX_TOP_MAX);
    CARCA_CHECK_ARG(D.slots && D.slot_items, "%s: null slots / slot_items", what);
    CARCA_CHECK_ARG(D.ld_contrib >= D.top_m && D.ld_slots >= D.top_m && D.ld_slot_items >= D.top_m,
                    "%s: row stride shorter than top_m", what);
  }
  const rc::ListGrid G = rc::list_grid(D.n_list, D.B);
  return rc::dispatch_scorer(D, what, [&](auto scorer) -> int {
    using Scorer = typename decltype(scorer)::type;
    if constexpr (ex_is_ca<Scorer>::value) {
      if (dense) {
        hipLaunchKernelGGL((ex_kernel<Scorer, true>), G.grid, dim3(EX_TILE), 0, (hipStream_t)stream, D, G.rounds_per_wg);
      } else {
        hipLaunchKernelGGL((ex_kernel<Scorer, false>), G.grid, dim3(EX_TILE), 0, (hipStream_t)stream, D, G.rounds_per_wg);
      }
      CARCA_LAUNCH_CHECK();
      return CARCA_OK;
    } else {
      return CARCA_ERR_UNSUPPORTED;  // (not reached: the decoder was checked above)
    }
  });
}
