// Per-(user, item) logit arithmetic and the item order shared by the full-catalogue kernels: the top-k sweep of
// recommend.hip and the list scoring / counting sweep of rank.hip (both through catalogue_sweep.h).  Both calls order items
// by the same 64-bit key (order-preserving logit bits, then the complemented id), so they must produce the same logit bits
// for the same (user, item): every kernel stages a user and scores an item through one of the two scorers below
// (CaScorer, DotScorer: the same five members), never through a copy of their arithmetic.  Desc is CarcaRecommendDesc or
// CarcaRankDesc (the model-side fields carry the same names and meanings, include/carca_hip.h).
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
};
struct ListedItems {
  static constexpr bool listed = true;
  const int32_t* ids;
  int n;
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

// ---- the two scorers -----------------------------------------------------------------------------------------------
// A scorer is built per thread from the descriptor and has: User (one user's share, in LDS), Item (one item's share, in
// registers), load_item (zeros where !live), stage_user (whole workgroup of TILE threads; the caller has synchronised
// since the previous user's LDS was last read; ends with a barrier) and logit.

// cross-attention decoder
template <int DHP, int H>
struct CaScorer {
  static constexpr int DPO = DHP * H;
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
    const int tid = threadIdx.x, nthr = TILE;
    const int dh = D.d / H;
    float* Ks = reinterpret_cast<float*>(S.Ks4);
    if (tid < 64) {  // compact the valid slots (leading pad slots and any interior id 0 are skipped)
      const bool v = tid < D.L && D.p_ids[(size_t)u * D.ld_p_ids + tid] != 0;
      const unsigned long long m = __ballot(v);
      if (v) S.slot[__popcll(m & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) S.nvalid = __popcll(m);
    }
    __syncthreads();
    nv = S.nvalid;
    for (int idx = tid; idx < nv * DPO; idx += nthr) {
      const int j = idx / DPO, col = idx % DPO, h = col / DHP, c = col % DHP;
      Ks[idx] = c < dh ? D.user_k[((size_t)u * D.L + S.slot[j]) * D.ld_user_k + h * dh + c] : 0.f;
    }
    for (int idx = tid; idx < nv * H; idx += nthr) {
      const int j = idx / H, h = idx % H;
      S.Us[j][h] = D.user_u[((size_t)u * D.L + S.slot[j]) * D.ld_user_u + h];
    }
    __syncthreads();
    for (int idx = tid; idx < nv * H; idx += nthr) {  // beta_hl = (M c_u W_Q^T)_h . K_hl, pre-scaled
      const int j = idx / H, h = idx % H;
      float b = 0.f;
      if (D.user_q) {
        const float* dq = D.user_q + (size_t)u * D.ld_user_q + h * dh;
        for (int c = 0; c < dh; ++c) b = fmaf(dq[c], Ks[j * DPO + h * DHP + c], b);
      }
      S.Bs[h][j] = b * sc;
    }
    __syncthreads();
  }

  template <class Desc>
  __device__ __forceinline__ float logit(const Desc& D, int u, const Item& I, const User& S) const {
    float logit = I.off;
    if (D.user_off) logit += D.user_off[(size_t)u * D.ld_user_off];
    if (D.ffn_b) logit += D.ffn_b[0];
    if (nv > 0) {  // (a fully masked profile: attention term 0, carca.py:256)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float m = -INFINITY, den = 0.f, num = 0.f;
        for (int j = 0; j < nv; ++j) {
          const float4* kr = S.Ks4 + (j * DPO + h * DHP) / 4;
          float s0 = 0.f, s1 = 0.f;
#pragma unroll
          for (int c4 = 0; c4 < DHP / 4; ++c4) {
            const float4 k4 = kr[c4];
            s0 = fmaf(I.q[h][4 * c4], k4.x, s0);
            s1 = fmaf(I.q[h][4 * c4 + 1], k4.y, s1);
            s0 = fmaf(I.q[h][4 * c4 + 2], k4.z, s0);
            s1 = fmaf(I.q[h][4 * c4 + 3], k4.w, s1);
          }
          const float s = fmaf(s0 + s1, sc, S.Bs[h][j]);
          const float mn = fmaxf(m, s);
          const float a = exp2f(m - mn), e = exp2f(s - mn);
          den = fmaf(den, a, e);
          num = fmaf(num, a, e * S.Us[j][h]);
          m = mn;
        }
        logit += num / den;
      }
    }
    return logit;
  }
};

// dot decoders
template <int DPI>
struct DotScorer {
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
    if (tid < 64) {  // a_u . m_u and m_u . m_u, once per user
      float a0 = 0.f, m0 = 0.f;
      for (int c = tid; c < D.d; c += 64) {
        const float a = D.user_q[(size_t)u * D.ld_user_q + c];
        const float mv = has_m ? D.user_m[(size_t)u * D.ld_user_m + c] : 0.f;
        a0 = fmaf(a, mv, a0);
        m0 = fmaf(mv, mv, m0);
      }
      a0 = wave_sum(a0);
      m0 = wave_sum(m0);
      if (tid == 0) S.am_mm[0] = a0, S.am_mm[1] = m0;
    }
    __syncthreads();
  }

  template <class Desc>
  __device__ __forceinline__ float logit(const Desc& D, int, const Item& I, const User& S) const {
    const bool norm = D.decoder == 2, has_m = D.user_m != nullptr;
    float dot0 = 0.f, dot1 = 0.f, tm0 = 0.f, tm1 = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < DPI / 4; ++c4) {
      const float4 a4 = S.As4[c4];
      dot0 = fmaf(I.t[4 * c4], a4.x, dot0);
      dot1 = fmaf(I.t[4 * c4 + 1], a4.y, dot1);
      dot0 = fmaf(I.t[4 * c4 + 2], a4.z, dot0);
      dot1 = fmaf(I.t[4 * c4 + 3], a4.w, dot1);
    }
    float y = dot0 + dot1 + S.am_mm[0];
    if (norm) {
      if (has_m) {
#pragma unroll
        for (int c4 = 0; c4 < DPI / 4; ++c4) {
          const float4 m4 = S.Ms4[c4];
          tm0 = fmaf(I.t[4 * c4], m4.x, tm0);
          tm1 = fmaf(I.t[4 * c4 + 1], m4.y, tm1);
          tm0 = fmaf(I.t[4 * c4 + 2], m4.z, tm0);
          tm1 = fmaf(I.t[4 * c4 + 3], m4.w, tm1);
        }
      }
      const float n2 = fmaxf(I.tn + 2.f * (tm0 + tm1) + S.am_mm[1], 0.f);
      y = y / fmaxf(sqrtf(n2), 1e-12f);  // F.normalize(o): o / max(||o||, eps) (carca.py:388-389)
    }
    return y;
  }
};

}  // namespace rc
