// Per-(user, item) logit arithmetic and the item order shared by the full-catalogue kernels: the top-k sweep of
// recommend.hip and the list scoring / counting sweep of rank.hip (both through catalogue_sweep.h), and the per-user list
// kernels of recommend_lists.hip, explain_lists.hip and recommend_contexts.hip.  The calls order items
// by the same 64-bit key (order-preserving logit bits, then the complemented id), so they must produce the same logit bits
// for the same (user, item): every kernel stages a user and scores an item through one of the scorers below
// (CaScorer, DotScorer: the same five members; CaLongScorer, CaScorer's arithmetic over a profile staged in chunks;
// CaContextScorer, DotContextScorer: the same pieces of arithmetic under several request contexts of one user),
// never through a copy of their arithmetic.  Desc is CarcaRecommendDesc or CarcaRankDesc (the model-side fields carry
// the same names and meanings, include/carca_hip.h).
#pragma once
#include "attn_common.h"

namespace rc {

constexpr int TILE = 256;       // items per sweep workgroup (one per lane)
constexpr int LIST_MAX = 128;   // largest list of rank_items
constexpr unsigned long long KEY_NEVER = ~0ull;  // key of an invalid target: no item orders before it

__device__ __forceinline__ unsigned order_bits(unsigned bits) {  // float bits -> unsigned with the same order
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float unorder_bits(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
// (order bits, id) -> key: larger key = earlier in recommend's order (logit descending, ties to the smaller id).  Order
// bits 0 are the exclusion sentinel's (catalogue_select.h): the callers that can meet it skip the item or use key 0.
__device__ __forceinline__ unsigned long long order_key(unsigned o, unsigned id) {
  return ((unsigned long long)o << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)id);
}
__device__ __forceinline__ unsigned long long item_key(float logit, int id) {
  return order_key(order_bits(__float_as_uint(logit)), (unsigned)id);
}
__device__ __forceinline__ unsigned key_id(unsigned long long key) {
  return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
}
// the model's link: sigmoid, or (y + 1) / 2 for the normalised dot decoder (carca.py:346, 367, 395-399)
__device__ __forceinline__ float link(float y, int decoder) {
  return decoder == 2 ? (y + 1.f) * 0.5f : 1.f / (1.f + expf(-y));
}

// ---- the item maps ---------------------------------------------------------------------------------------------------
// Which items a catalogue launch covers: positions 0 .. size - 1, each holding one item id.  AllItems is the catalogue
// itself (position = id); ListedItems a candidate list (CarcaCandidates: ascending, distinct, so positions order as ids
// do and a tie between two positions goes the way the tie between their ids goes).  An item's logit does not depend on
// the position that holds it (load_item gathers its row by id).
struct AllItems {
  static constexpr bool listed = false;
  __device__ __forceinline__ int size(int n_items) const { return n_items; }
  __device__ __forceinline__ int item(int pos) const { return pos; }
  __device__ __forceinline__ int find(int id) const { return id; }  // (the caller has checked 1 <= id < n_items)
  __device__ __forceinline__ AllItems for_user(int) const { return *this; }
};
struct ListedItems {
  static constexpr bool listed = true;
  const int32_t* ids;
  int n;
  __device__ __forceinline__ ListedItems for_user(int) const { return *this; }
  __device__ __forceinline__ int size(int) const { return n; }
  __device__ __forceinline__ int item(int pos) const { return pos < n ? ids[pos] : 0; }  // (0 is never live)
  __device__ __forceinline__ int find(int id) const {  // the position of id, -1 when the list does not hold it
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ids[mid] < id) {
        lo = mid + 1;
      } else {
        hi = mid;
      }
    }
    return (lo < n && ids[lo] == id) ? lo : -1;
  }
};
// A list of its own per user (recommend_lists.hip): row u of ids [B, ld], n entries in NONDECREASING order.  A position is
// live where its id is an item and differs from its predecessor's, so a row's live positions are ascending and distinct
// -- ListedItems' argument, per row -- and an id's first occurrence, which find returns, is its live one.  Ids outside
// [1, n_items) sort to the two ends and are never live (item gives 0 for a repeat; the caller tests the range).  A
// launch with one workgroup per user takes its row through for_user(u); the two maps above are their own rows.
struct ListedRow {
  static constexpr bool listed = true;
  const int32_t* ids;
  int n;
  __device__ __forceinline__ int size(int) const { return n; }
  __device__ __forceinline__ int item(int pos) const {
    return (pos < n && (pos == 0 || ids[pos - 1] != ids[pos])) ? ids[pos] : 0;
  }
  __device__ __forceinline__ int find(int id) const {  // the live position of id, -1 when the row does not hold it
    int lo = 0, hi = n;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (ids[mid] < id) {
        lo = mid + 1;
      } else {
        hi = mid;
      }
    }
    return (lo < n && ids[lo] == id) ? lo : -1;
  }
};
struct UserLists {
  static constexpr bool listed = true;
  const int32_t* ids;
  int n, ld;
  __device__ __forceinline__ ListedRow for_user(int u) const { return ListedRow{ids + (size_t)u * ld, n}; }
};

// The grouped order of CarcaItemGroups (group_select.h): positions 0 .. n - 1 of `order`, sorted by (group, id).  The
// sweep reads such an order through ListedItems (it asks only for item(pos)); this map is for the launches that look an id
// up.  find(id) = pos_of[id]: `order` is not ascending across groups, so ListedItems' binary search does not apply (the
// caller has checked 1 <= id < n_items = the entries of pos_of; an entry outside [0, n) counts as "not grouped" and is
// never used as an index).
struct GroupedItems {
  static constexpr bool listed = true;
  const int32_t* order;
  const int32_t* pos_of;
  int n;
  __device__ __forceinline__ GroupedItems for_user(int) const { return *this; }
  __device__ __forceinline__ int size(int) const { return n; }
  __device__ __forceinline__ int item(int pos) const { return pos < n ? order[pos] : 0; }
  __device__ __forceinline__ int find(int id) const {
    const int p = pos_of[id];
    return (p >= 0 && p < n) ? p : -1;
  }
};

// ---- the scorers ---------------------------------------------------------------------------------------------------
// A scorer is built per thread from the descriptor and has: User (one user's share, in LDS), Item (one item's share, in
// registers), load_item (zeros where !live), stage_user (whole workgroup of TILE threads; the caller has synchronised
// since the previous user's LDS was last read; ends with a barrier) and logit.  `chunked` says which protocol a kernel
// runs: false = stage_user + logit, true = CaLongScorer's chunk loop.

// ---- what the cross-attention scorers share ----------------------------------------------------------------------
// beta_hl = (M c W_Q^T)_h . K_hl, pre-scaled: the score bias of staged slot j (row j of Ks, head-padded) and head h under
// the context whose row of (M c) W_Q^T is dq (null: no context term).  ca_stage_slots runs it over the descriptor's
// row of user u, CaContextScorer over each of the user's context rows.
template <int DHP, int H>
__device__ __forceinline__ float ca_slot_beta(const float* dq, const float* Ks, int j, int h, int dh, float sc) {
  float b = 0.f;
  if (dq) {
    const float* r = dq + h * dh;
    for (int c = 0; c < dh; ++c) b = fmaf(r[c], Ks[j * DHP * H + h * DHP + c], b);
  }
  return b * sc;
}

// The context-free share of ca_stage_slots: the K rows of slot[0 .. n), head-padded, and their folded values into S (any
// User with Ks4 / Us).  Whole workgroup of TILE threads; n is workgroup-uniform; the caller has synchronised since S was
// last read and has published slot[].  One barrier: Ks / Us are published.
template <int DHP, int H, class Desc, class User>
__device__ __forceinline__ void ca_stage_rows(const Desc& D, int u, const int* slot, int n, User& S) {
  constexpr int DPO = DHP * H;
  const int tid = threadIdx.x, nthr = TILE;
  const int dh = D.d / H;
  float* Ks = reinterpret_cast<float*>(S.Ks4);
  for (int idx = tid; idx < n * DPO; idx += nthr) {
    const int j = idx / DPO, col = idx % DPO, h = col / DHP, c = col % DHP;
    Ks[idx] = c < dh ? D.user_k[((size_t)u * D.L + slot[j]) * D.ld_user_k + h * dh + c] : 0.f;
  }
  for (int idx = tid; idx < n * H; idx += nthr) {
    const int j = idx / H, h = idx % H;
    S.Us[j][h] = D.user_u[((size_t)u * D.L + slot[j]) * D.ld_user_u + h];
  }
  __syncthreads();
}

// Stages n <= CARCA_MAX_L profile slots of user u, slot[0 .. n), into S (any User with Ks4 / Us / Bs): their K rows
// head-padded, their folded values and the pre-scaled score biases.  Whole workgroup of TILE threads; n is
// workgroup-uniform; the caller has synchronised since S was last read and has published slot[].  Two barriers: the
// first publishes Ks / Us (beta reads Ks), the second Bs.
template <int DHP, int H, class Desc, class User>
__device__ __forceinline__ void ca_stage_slots(const Desc& D, int u, const int* slot, int n, float sc, User& S) {
  const int tid = threadIdx.x, nthr = TILE;
  const int dh = D.d / H;
  ca_stage_rows<DHP, H>(D, u, slot, n, S);
  const float* Ks = reinterpret_cast<const float*>(S.Ks4);
  const float* dq = D.user_q ? D.user_q + (size_t)u * D.ld_user_q : nullptr;
  for (int idx = tid; idx < n * H; idx += nthr) {
    const int j = idx / H, h = idx % H;
    S.Bs[h][j] = ca_slot_beta<DHP, H>(dq, Ks, j, h, dh, sc);
  }
  __syncthreads();
}

// The head dot product of a pair: QT[i]_h . K_hl over staged slot j.  It reads no context, so a scorer that serves several
// contexts of one user (CaContextScorer) computes it once per (head, slot) and runs ca_slot_bias per context.
template <int DHP, int H, class User>
__device__ __forceinline__ float ca_slot_dot(const float (&q)[DHP], const User& S, int h, int j) {
  const float4* kr = S.Ks4 + (j * DHP * H + h * DHP) / 4;
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int c4 = 0; c4 < DHP / 4; ++c4) {
    const float4 k4 = kr[c4];
    s0 = fmaf(q[4 * c4], k4.x, s0);
    s1 = fmaf(q[4 * c4 + 1], k4.y, s1);
    s0 = fmaf(q[4 * c4 + 2], k4.z, s0);
    s1 = fmaf(q[4 * c4 + 3], k4.w, s1);
  }
  return s0 + s1;
}
// the head dot product scaled into the exp2 domain, the context's pre-scaled bias (Bs) added
__device__ __forceinline__ float ca_slot_bias(float dot, float sc, float bias) { return fmaf(dot, sc, bias); }

// Staged slot j's pre-softmax score of head h, in the exp2 domain (scaled by log2(e) / sqrt(dh), the bias added): the
// two pieces above in sequence.  The only copy of this arithmetic: the scorers reach it through ca_slot_step (or through
// its two pieces), and explain_lists.hip evaluates it a second time per slot to turn a head's final (m, den) into that
// slot's softmax weight.
template <int DHP, int H, class User>
__device__ __forceinline__ float ca_slot_score(const float (&q)[DHP], const User& S, int h, int j, float sc) {
  return ca_slot_bias(ca_slot_dot<DHP, H>(q, S, h, j), sc, S.Bs[h][j]);
}

// staged slot j of head h, of score s, joins the head's running (m, den, num)
template <class User>
__device__ __forceinline__ void ca_online_update(float s, const User& S, int h, int j, float& m, float& den, float& num) {
  const float mn = fmaxf(m, s);
  const float a = exp2f(m - mn), e = exp2f(s - mn);
  den = fmaf(den, a, e);
  num = fmaf(num, a, e * S.Us[j][h]);
  m = mn;
}

// One step of a head's online exp2 softmax: staged slot j of head h joins the running (m, den, num).  CaScorer walks all
// of a user's slots with it, CaLongScorer the same slots 64 at a time.
template <int DHP, int H, class User>
__device__ __forceinline__ void ca_slot_step(const float (&q)[DHP], const User& S, int h, int j, float sc, float& m,
                                             float& den, float& num) {
  ca_online_update(ca_slot_score<DHP, H>(q, S, h, j, sc), S, h, j, m, den, num);
}

// the terms of a cross-attention logit that no profile slot enters; user_off: the (user, context) pair's w . M c, or null
__device__ __forceinline__ float ca_logit_offsets(const float* user_off, const float* ffn_b, float item_off) {
  float logit = item_off;
  if (user_off) logit += user_off[0];
  if (ffn_b) logit += ffn_b[0];
  return logit;
}
template <class Desc>
__device__ __forceinline__ float ca_logit_offsets(const Desc& D, int u, float item_off) {
  return ca_logit_offsets(D.user_off ? D.user_off + (size_t)u * D.ld_user_off : nullptr, D.ffn_b, item_off);
}

// Compacts the valid slots of user u's profile of D.L <= CARCA_MAX_L positions into S.slot / S.nvalid (leading pad slots
// and any interior id 0 are skipped).  Whole workgroup; one barrier: slot[] and nvalid are published.
template <class Desc, class User>
__device__ __forceinline__ void ca_compact_slots(const Desc& D, int u, User& S) {
  const int tid = threadIdx.x;
  if (tid < 64) {
    const bool v = tid < D.L && D.p_ids[(size_t)u * D.ld_p_ids + tid] != 0;
    const unsigned long long m = __ballot(v);
    if (v) S.slot[__popcll(m & ((1ull << tid) - 1ull))] = tid;
    if (tid == 0) S.nvalid = __popcll(m);
  }
  __syncthreads();
}

// cross-attention decoder, profiles of up to CARCA_MAX_L slots: the whole user in LDS
template <int DHP, int H>
struct CaScorer {
  static constexpr bool chunked = false;
  static constexpr int DPO = DHP * H, HEADS = H, HEAD_PAD = DHP;
  struct Stats {
    float m[H], den[H];  // a head's final running maximum and denominator
  };
  struct User {
    float4 Ks4[CARCA_MAX_L * DHP * H / 4];  // compacted valid profile slots, head-padded
    float Us[CARCA_MAX_L][H];
    float Bs[H][CARCA_MAX_L];
    int slot[CARCA_MAX_L];
    int nvalid;
  };
  struct Item {
    float q[H][DHP];  // QT row, head-padded
    float off;        // residual term
  };
  float sc;  // log2(e) / sqrt(dh): the softmax runs on exp2
  int nv;    // valid profile slots of the staged user

  template <class Desc>
  __device__ __forceinline__ explicit CaScorer(const Desc& D) : sc(1.4426950408889634f / sqrtf((float)(D.d / H))), nv(0) {}

  template <class Desc>
  __device__ __forceinline__ void load_item(const Desc& D, int item, bool live, Item& I) const {
    const int dh = D.d / H;
#pragma unroll
    for (int h = 0; h < H; ++h)
#pragma unroll
      for (int c = 0; c < DHP; ++c)
        I.q[h][c] = (live && c < dh) ? D.item_q[(size_t)item * D.ld_item_q + h * dh + c] : 0.f;
    I.off = 0.f;
    if (live && D.item_w) I.off = D.item_w[(size_t)item * D.ld_item_w];
  }

  template <class Desc>
  __device__ __forceinline__ void stage_user(const Desc& D, int u, User& S) {
    ca_compact_slots(D, u, S);
    nv = S.nvalid;
    ca_stage_slots<DHP, H>(D, u, S.slot, nv, sc, S);
  }

  template <class Desc>
  __device__ __forceinline__ float logit(const Desc& D, int u, const Item& I, const User& S) const {
    float logit = ca_logit_offsets(D, u, I.off);
    if (nv > 0) {  // (a fully masked profile: attention term 0, carca.py:256)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float m = -INFINITY, den = 0.f, num = 0.f;
        for (int j = 0; j < nv; ++j) ca_slot_step<DHP, H>(I.q[h], S, h, j, sc, m, den, num);
        logit += num / den;
      }
    }
    return logit;
  }

  // logit, leaving each head's final softmax statistics in T (untouched for a fully masked profile): slot j's weight
  // in head h is exp2(ca_slot_score(j) - T.m[h]) / T.den[h]
  template <class Desc>
  __device__ __forceinline__ float logit_stats(const Desc& D, int u, const Item& I, const User& S, Stats& T) const {
    float logit = ca_logit_offsets(D, u, I.off);
    if (nv > 0) {  // (a fully masked profile: attention term 0, carca.py:256)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float m = -INFINITY, den = 0.f, num = 0.f;
        for (int j = 0; j < nv; ++j) ca_slot_step<DHP, H>(I.q[h], S, h, j, sc, m, den, num);
        logit += num / den;
        T.m[h] = m, T.den[h] = den;
      }
    }
    return logit;
  }
};

// Cross-attention decoder, profiles of up to CARCA_MAX_PROFILE_L slots: the valid slots' positions in LDS, their rows
// staged CARCA_MAX_L at a time.  A lane keeps (m, den, num) per head across the chunks and walks the slots in ascending
// compacted order through ca_slot_step, so each head sees the sequence of steps CaScorer::logit would run over the
// same valid slots, and finish adds the same terms in the same order: the same logit bits.  In place of stage_user /
// logit a kernel runs
//   begin_user; for (c = 0; c < n_chunks(); ++c) { if (c) __syncthreads(); stage_chunk(c); accumulate(c); }  finish
// (sweep_long_kernel in catalogue_sweep.h, rk_list_long_kernel in rank.hip).  n_chunks() is workgroup-uniform: every
// thread computes it from the same LDS words after begin_user's barrier.
template <int DHP, int H>
struct CaLongScorer {
  static constexpr bool chunked = true;
  using Short = CaScorer<DHP, H>;
  using Item = typename Short::Item;
  static constexpr int ROUNDS = CARCA_MAX_PROFILE_L / TILE, WAVES = TILE / 64, HEADS = H, HEAD_PAD = DHP;
  static_assert(ROUNDS * TILE == CARCA_MAX_PROFILE_L, "the compaction covers the profile in whole rounds");
  struct User {
    float4 Ks4[CARCA_MAX_L * DHP * H / 4];  // the staged chunk: K rows of CARCA_MAX_L compacted slots, head-padded
    float Us[CARCA_MAX_L][H];
    float Bs[H][CARCA_MAX_L];
    int slot[CARCA_MAX_PROFILE_L];  // positions of the valid slots, ascending
    int wcnt[ROUNDS * WAVES];       // valid slots per (round, wave) of the compaction
  };
  struct Acc {
    float m[H], den[H], num[H];  // after the last chunk, (m, den) are what CaScorer::logit_stats leaves in its Stats
  };
  Short base;
  int nv;  // valid profile slots of the user begun

  template <class Desc>
  __device__ __forceinline__ explicit CaLongScorer(const Desc& D) : base(D), nv(0) {}

  template <class Desc>
  __device__ __forceinline__ void load_item(const Desc& D, int item, bool live, Item& I) const {
    base.load_item(D, item, live, I);
  }

  // Compacts the valid slots of all D.L positions into S.slot, ROUNDS rounds of TILE positions (a constant trip count):
  // a ballot per wave, the wave bases summed through LDS.  Whole workgroup; the caller has synchronised since the
  // previous user's LDS was last read.  The first barrier publishes wcnt, the second slot[].
  template <class Desc>
  __device__ __forceinline__ void begin_user(const Desc& D, int u, User& S) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    unsigned long long mask[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
      const int pos = r * TILE + tid;
      const bool v = pos < D.L && D.p_ids[(size_t)u * D.ld_p_ids + pos] != 0;
      mask[r] = __ballot(v);
      if (lane == 0) S.wcnt[r * WAVES + w] = __popcll(mask[r]);
    }
    __syncthreads();
    // before: the valid slots ahead of this wave's share of round r; total: all of them, summed by every thread from the
    // same LDS words, so nv is workgroup-uniform
    int before = 0, total = 0;
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r) {
#pragma unroll
      for (int v = 0; v < WAVES; ++v) {
        if (v == w) before = total;
        total += S.wcnt[r * WAVES + v];
      }
      if ((mask[r] >> lane) & 1ull) S.slot[before + __popcll(mask[r] & ((1ull << lane) - 1ull))] = r * TILE + tid;
    }
    nv = total;
    __syncthreads();
  }

  __device__ __forceinline__ int n_chunks() const { return (nv + CARCA_MAX_L - 1) / CARCA_MAX_L; }
  __device__ __forceinline__ int chunk_size(int c) const { return min(CARCA_MAX_L, nv - c * CARCA_MAX_L); }

  // Chunk c's rows into S.  Whole workgroup; the caller has synchronised since the previous chunk was last read; ends
  // with the barrier that publishes Bs (ca_stage_slots).
  template <class Desc>
  __device__ __forceinline__ void stage_chunk(const Desc& D, int u, int c, User& S) const {
    ca_stage_slots<DHP, H>(D, u, S.slot + c * CARCA_MAX_L, chunk_size(c), base.sc, S);
  }

  __device__ __forceinline__ void reset(Acc& A) const {
#pragma unroll
    for (int h = 0; h < H; ++h) A.m[h] = -INFINITY, A.den[h] = 0.f, A.num[h] = 0.f;
  }

  __device__ __forceinline__ void accumulate(const Item& I, const User& S, int c, Acc& A) const {
    const int n = chunk_size(c);
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float m = A.m[h], den = A.den[h], num = A.num[h];
      for (int j = 0; j < n; ++j) ca_slot_step<DHP, H>(I.q[h], S, h, j, base.sc, m, den, num);
      A.m[h] = m, A.den[h] = den, A.num[h] = num;
    }
  }

  template <class Desc>
  __device__ __forceinline__ float finish(const Desc& D, int u, const Item& I, const Acc& A) const {
    float logit = ca_logit_offsets(D, u, I.off);
    if (nv > 0) {  // (a fully masked profile: attention term 0, carca.py:256)
#pragma unroll
      for (int h = 0; h < H; ++h) logit += A.num[h] / A.den[h];
    }
    return logit;
  }
};

// Cross-attention decoder under several request contexts of one user (recommend_contexts.hip), profiles of up to
// CARCA_MAX_L slots.  K, u and the slot list do not depend on the context and are staged once (stage_user); the score
// biases of up to NC contexts at a time -- rows u * n_contexts + c0 .. of X.user_q, X a CarcaContexts -- go to
// Bs4[h][j][c], each through ca_slot_beta as ca_stage_slots computes CaScorer's Bs from the descriptor's row
// (stage_contexts).  logits walks (head, slot) once: ca_slot_dot once per pair, then per context ca_slot_bias and
// ca_online_update on that context's (m, den, num), and adds the heads to ca_logit_offsets' sum in CaScorer::logit's
// order -- per context the sequence of operations CaScorer::logit runs under that context, so the same logit bits.
// A kernel runs: stage_user; for each pass of NC contexts { if (pass) __syncthreads(); stage_contexts; logits }.
template <int DHP, int H, int NC_>
struct CaContextScorer {
  static constexpr int NC = NC_, HEADS = H, HEAD_PAD = DHP;
  static_assert(NC % 4 == 0 && (NC & (NC - 1)) == 0, "a slot's biases are read as float4; heads_upto halves NC");
  using Short = CaScorer<DHP, H>;
  using Item = typename Short::Item;
  struct User {
    float4 Ks4[CARCA_MAX_L * DHP * H / 4];  // compacted valid profile slots, head-padded
    float Us[CARCA_MAX_L][H];
    float4 Bs4[H][CARCA_MAX_L][NC / 4];  // the staged contexts' pre-scaled score biases
    int slot[CARCA_MAX_L];
    int nvalid;
  };
  Short base;
  int nv;  // valid profile slots of the staged user

  template <class Desc>
  __device__ __forceinline__ explicit CaContextScorer(const Desc& D) : base(D), nv(0) {}

  template <class Desc>
  __device__ __forceinline__ void load_item(const Desc& D, int item, bool live, Item& I) const {
    base.load_item(D, item, live, I);
  }

  // Two barriers: ca_compact_slots' (the slot list), ca_stage_rows' (Ks / Us).  nv is workgroup-uniform (an LDS word
  // every thread reads after the first).
  template <class Desc>
  __device__ __forceinline__ void stage_user(const Desc& D, int u, User& S) {
    ca_compact_slots(D, u, S);
    nv = S.nvalid;
    ca_stage_rows<DHP, H>(D, u, S.slot, nv, S);
  }

  // The biases of contexts c0 .. c0 + ncx of user u (ncx <= NC, workgroup-uniform).  The caller has synchronised since
  // Bs4 was last read; one barrier: Bs4 is published.
  template <class Desc, class Ctx>
  __device__ __forceinline__ void stage_contexts(const Desc& D, const Ctx& X, int u, int c0, int ncx, User& S) const {
    const int dh = D.d / H;
    const float* Ks = reinterpret_cast<const float*>(S.Ks4);
    float* Bs = reinterpret_cast<float*>(S.Bs4);
    for (int idx = threadIdx.x; idx < ncx * nv * H; idx += TILE) {
      const int c = idx / (nv * H), r = idx % (nv * H), j = r / H, h = r % H;
      const float* dq = X.user_q ? X.user_q + ((size_t)u * X.n_contexts + c0 + c) * X.ld_user_q : nullptr;
      Bs[(h * CARCA_MAX_L + j) * NC + c] = ca_slot_beta<DHP, H>(dq, Ks, j, h, dh, base.sc);
    }
    __syncthreads();
  }

  // y[c], c < ncx: the logit of (user u under context c0 + c, item I); y[c] means nothing for c >= ncx
  template <class Desc, class Ctx>
  __device__ __forceinline__ void logits(const Desc& D, const Ctx& X, int u, int c0, int ncx, const Item& I, const User& S,
                                         float (&y)[NC]) const {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      y[c] = 0.f;
      if (c < ncx)
        y[c] = ca_logit_offsets(X.user_off ? X.user_off + ((size_t)u * X.n_contexts + c0 + c) * X.ld_user_off : nullptr,
                                D.ffn_b, I.off);
    }
    if (nv > 0) heads_upto<NC>(ncx, I, S, y);  // (a fully masked profile: attention term 0, carca.py:256)
  }

 private:
  // The heads' attention terms of the first N staged contexts, added to y[0 .. N): N is a compile-time count, so the
  // slot loop carries no test per context.  Called with N >= ncx: a context past ncx runs over whatever Bs4 holds for
  // it and lands in a y the caller never reads.
  template <int N>
  __device__ __forceinline__ void heads(const Item& I, const User& S, float (&y)[NC]) const {
#pragma unroll
    for (int h = 0; h < H; ++h) {
      float m[N], den[N], num[N];
#pragma unroll
      for (int c = 0; c < N; ++c) m[c] = -INFINITY, den[c] = 0.f, num[c] = 0.f;
      for (int j = 0; j < nv; ++j) {
        const float dot = ca_slot_dot<DHP, H>(I.q[h], S, h, j);
        float bias[N];
        if constexpr (N % 4 == 0) {
#pragma unroll
          for (int c4 = 0; c4 < N / 4; ++c4) {
            const float4 b4 = S.Bs4[h][j][c4];
            bias[4 * c4] = b4.x, bias[4 * c4 + 1] = b4.y, bias[4 * c4 + 2] = b4.z, bias[4 * c4 + 3] = b4.w;
          }
        } else {
          const float* b = reinterpret_cast<const float*>(S.Bs4[h][j]);
#pragma unroll
          for (int c = 0; c < N; ++c) bias[c] = b[c];
        }
#pragma unroll
        for (int c = 0; c < N; ++c) ca_online_update(ca_slot_bias(dot, base.sc, bias[c]), S, h, j, m[c], den[c], num[c]);
      }
#pragma unroll
      for (int c = 0; c < N; ++c) y[c] += num[c] / den[c];
    }
  }
  // heads<N'> for the smallest N' = NC, NC / 2, ..., 1 that holds ncx contexts (ncx is workgroup-uniform)
  template <int N>
  __device__ __forceinline__ void heads_upto(int ncx, const Item& I, const User& S, float (&y)[NC]) const {
    if constexpr (N > 1) {
      if (2 * ncx <= N) {
        heads_upto<N / 2>(ncx, I, S, y);
        return;
      }
    }
    heads<N>(I, S, y);
  }
};

// ---- what the dot scorers share --------------------------------------------------------------------------------------
// t . r over a staged row (As4 or Ms4), as two interleaved chains
template <int DPI>
__device__ __forceinline__ float dot_row(const float (&t)[DPI], const float4* r4) {
  float d0 = 0.f, d1 = 0.f;
#pragma unroll
  for (int c4 = 0; c4 < DPI / 4; ++c4) {
    const float4 a4 = r4[c4];
    d0 = fmaf(t[4 * c4], a4.x, d0);
    d1 = fmaf(t[4 * c4 + 1], a4.y, d1);
    d0 = fmaf(t[4 * c4 + 2], a4.z, d0);
    d1 = fmaf(t[4 * c4 + 3], a4.w, d1);
  }
  return d0 + d1;
}
// a dot logit from its sums: ta = t . a, tm = t . m (0 without a context term), tn = t . t, am = a . m, mm = m . m
__device__ __forceinline__ float dot_finish(float ta, float tm, float tn, float am, float mm, bool norm) {
  float y = ta + am;
  if (norm) {
    const float n2 = fmaxf(tn + 2.f * tm + mm, 0.f);
    y = y / fmaxf(sqrtf(n2), 1e-12f);  // F.normalize(o): o / max(||o||, eps) (carca.py:388-389)
  }
  return y;
}
// a . m and m . m of a scored row a and a context row m (null: zeros) into am_mm[0 .. 2): one whole wave
__device__ __forceinline__ void dot_stage_am(const float* a_row, const float* m_row, int d, float* am_mm) {
  const int lane = threadIdx.x & 63;
  float a0 = 0.f, m0 = 0.f;
  for (int c = lane; c < d; c += 64) {
    const float a = a_row[c];
    const float mv = m_row ? m_row[c] : 0.f;
    a0 = fmaf(a, mv, a0);
    m0 = fmaf(mv, mv, m0);
  }
  a0 = wave_sum(a0);
  m0 = wave_sum(m0);
  if (lane == 0) am_mm[0] = a0, am_mm[1] = m0;
}

// dot decoders
template <int DPI>
struct DotScorer {
  static constexpr bool chunked = false;
  struct User {
    float4 As4[DPI / 4], Ms4[DPI / 4];
    float am_mm[2];
  };
  struct Item {
    float t[DPI];  // T row
    float tn;      // its squared norm
  };

  template <class Desc>
  __device__ __forceinline__ explicit DotScorer(const Desc&) {}

  template <class Desc>
  __device__ __forceinline__ void load_item(const Desc& D, int item, bool live, Item& I) const {
    I.tn = 0.f;
#pragma unroll
    for (int c = 0; c < DPI; ++c) {
      I.t[c] = (live && c < D.d) ? D.item_q[(size_t)item * D.ld_item_q + c] : 0.f;
      I.tn = fmaf(I.t[c], I.t[c], I.tn);
    }
  }

  template <class Desc>
  __device__ __forceinline__ void stage_user(const Desc& D, int u, User& S) {
    const int tid = threadIdx.x;
    const bool has_m = D.user_m != nullptr;
    float* As = reinterpret_cast<float*>(S.As4);
    float* Ms = reinterpret_cast<float*>(S.Ms4);
    if (tid < DPI) {
      As[tid] = tid < D.d ? D.user_q[(size_t)u * D.ld_user_q + tid] : 0.f;
      Ms[tid] = (has_m && tid < D.d) ? D.user_m[(size_t)u * D.ld_user_m + tid] : 0.f;
    }
    if (tid < 64)  // a_u . m_u and m_u . m_u, once per user
      dot_stage_am(D.user_q + (size_t)u * D.ld_user_q, has_m ? D.user_m + (size_t)u * D.ld_user_m : nullptr, D.d, S.am_mm);
    __syncthreads();
  }

  template <class Desc>
  __device__ __forceinline__ float logit(const Desc& D, int, const Item& I, const User& S) const {
    const bool norm = D.decoder == 2, has_m = D.user_m != nullptr;
    const float ta = dot_row<DPI>(I.t, S.As4);
    const float tm = (norm && has_m) ? dot_row<DPI>(I.t, S.Ms4) : 0.f;
    return dot_finish(ta, tm, I.tn, S.am_mm[0], S.am_mm[1], norm);
  }
};

// Dot decoders under several request contexts of one user (recommend_contexts.hip): the scored row a_u is staged once
// (stage_user), the rows m_c = M c of up to NC contexts at a time with their a . m and m . m (stage_contexts: rows
// u * n_contexts + c0 .. of X.user_m, X a CarcaContexts).  logits computes t . a once per item and per context t . m_c
// (normalised decoder) and dot_finish -- DotScorer::logit's pieces, so its bits under that context.  The kernels'
// protocol is CaContextScorer's.
template <int DPI, int NC_>
struct DotContextScorer {
  static constexpr int NC = NC_;
  using Short = DotScorer<DPI>;
  using Item = typename Short::Item;
  struct User {
    float4 As4[DPI / 4], Ms4[NC][DPI / 4];
    float am_mm[NC][2];
  };
  Short base;

  template <class Desc>
  __device__ __forceinline__ explicit DotContextScorer(const Desc& D) : base(D) {}

  template <class Desc>
  __device__ __forceinline__ void load_item(const Desc& D, int item, bool live, Item& I) const {
    base.load_item(D, item, live, I);
  }

  // one barrier: As4 is published
  template <class Desc>
  __device__ __forceinline__ void stage_user(const Desc& D, int u, User& S) {
    const int tid = threadIdx.x;
    float* As = reinterpret_cast<float*>(S.As4);
    if (tid < DPI) As[tid] = tid < D.d ? D.user_q[(size_t)u * D.ld_user_q + tid] : 0.f;
    __syncthreads();
  }

  // Contexts c0 .. c0 + ncx of user u (ncx <= NC, workgroup-uniform): wave w stages contexts w, w + TILE / 64, ... (a
  // wave-uniform trip count, no barrier inside).  The caller has synchronised since Ms4 / am_mm were last read; one
  // barrier: they are published.
  template <class Desc, class Ctx>
  __device__ __forceinline__ void stage_contexts(const Desc& D, const Ctx& X, int u, int c0, int ncx, User& S) const {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = w; c < ncx; c += TILE / 64) {
      const float* m_row = X.user_m ? X.user_m + ((size_t)u * X.n_contexts + c0 + c) * X.ld_user_m : nullptr;
      float* Ms = reinterpret_cast<float*>(S.Ms4[c]);
      for (int i = lane; i < DPI; i += 64) Ms[i] = (m_row && i < D.d) ? m_row[i] : 0.f;
      dot_stage_am(D.user_q + (size_t)u * D.ld_user_q, m_row, D.d, S.am_mm[c]);
    }
    __syncthreads();
  }

  template <class Desc, class Ctx>
  __device__ __forceinline__ void logits(const Desc& D, const Ctx& X, int, int, int ncx, const Item& I, const User& S,
                                         float (&y)[NC]) const {
    const bool norm = D.decoder == 2, has_m = X.user_m != nullptr;
    const float ta = dot_row<DPI>(I.t, S.As4);
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c < ncx) {
        const float tm = (norm && has_m) ? dot_row<DPI>(I.t, S.Ms4[c]) : 0.f;
        y[c] = dot_finish(ta, tm, I.tn, S.am_mm[c][0], S.am_mm[c][1], norm);
      }
  }
};

}  // namespace rc
