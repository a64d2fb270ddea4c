// Full-catalogue top-k recommendation (include/carca_hip.h: carca_recommend).
//
// The reference scores only the candidates a caller lists (carca.py:338-349, 352-399 over the 1 + 100 candidates of
// data.py:180-185).  In eval mode the candidates do not interact (carca.py:339: causal=None) and every embedding class is
// affine in the context, e(i, c) = T[i] + M c, so scoring EVERY item for a user needs per item only
// a row of a table built once per weight version, and per (user, item) pair:
//   cross-attention  sum_h softmax_l((QT[i]_h . K_hl + beta_hl) / sqrt(dh)) . u_hl  (+ wT[i]) + off_u
//   dot decoders     p_u . (T[i] + m_u), divided by ||T[i] + m_u|| for the normalised WeightedDotProduct
// Three launches, no host wait, nothing retained:
//   1. scoring: workgroups own 256-item tiles (one item per lane, its row in registers) and walk a chunk of users, each
//      user's keys / folded values / score biases staged in LDS; raw logits go to a [B, n_items] stream-scratch buffer;
//   2. exclusion: id 0 and the caller's [B, E] list are overwritten with a sentinel that selection never picks;
//   3. selection: one workgroup per user, an MSB-first radix select over 64-bit keys (order-preserving logit bits,
//      then the complemented item id, so ties go to the smaller id), a bitonic sort of the k survivors, and the link
//      (sigmoid, or (y + 1) / 2) applied to the k selected logits only.
// Integer LDS atomics only (histograms, slot counters); the result does not depend on scheduling.
#include "attn_common.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int RC_TILE = 256;          // items per scoring workgroup (one per lane)
constexpr int RC_SEL_THREADS = 256;   // selection workgroup
constexpr int RC_KMAX = 128;          // largest k
constexpr unsigned RC_SENTINEL = 0xFFFFFFFFu;  // a negative NaN pattern no arithmetic here produces; order key 0

// ---- 1a. cross-attention scoring ----------------------------------------------------------------------------
template <int DPI, int DHP, int H>
__global__ __launch_bounds__(RC_TILE) void rc_score_ca_kernel(CarcaRecommendDesc D, float* __restrict__ logits, int ld_s,
                                                              int users_per_block) {
  constexpr int DPO = DHP * H;
  __shared__ float4 Ks4[CARCA_MAX_L * DPO / 4];  // compacted valid profile slots, head-padded
  __shared__ float Us[CARCA_MAX_L][H];
  __shared__ float Bs[H][CARCA_MAX_L];
  __shared__ int slot[CARCA_MAX_L];
  __shared__ int nvalid;
  float* Ks = reinterpret_cast<float*>(Ks4);
  const int tid = threadIdx.x;
  const int dh = D.d / H;
  const float sc = 1.4426950408889634f / sqrtf((float)dh);  // log2(e) / sqrt(dh): the softmax runs on exp2
  const int item = blockIdx.x * RC_TILE + tid;
  const bool live = item >= 1 && item < D.n_items;
  float q[H][DHP];
#pragma unroll
  for (int h = 0; h < H; ++h)
#pragma unroll
    for (int c = 0; c < DHP; ++c) q[h][c] = (live && c < dh) ? D.item_q[(size_t)item * D.ld_item_q + h * dh + c] : 0.f;
  float item_off = 0.f;
  if (live && D.item_w) item_off = D.item_w[(size_t)item * D.ld_item_w];
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous user's LDS is read out
    if (tid < 64) {  // compact the valid slots (leading pad slots and any interior id 0 are skipped)
      const bool v = tid < D.L && D.p_ids[(size_t)u * D.ld_p_ids + tid] != 0;
      const unsigned long long m = __ballot(v);
      if (v) slot[__popcll(m & ((1ull << tid) - 1ull))] = tid;
      if (tid == 0) nvalid = __popcll(m);
    }
    __syncthreads();
    const int nv = nvalid;
    for (int idx = tid; idx < nv * DPO; idx += RC_TILE) {
      const int j = idx / DPO, col = idx % DPO, h = col / DHP, c = col % DHP;
      Ks[idx] = c < dh ? D.user_k[((size_t)u * D.L + slot[j]) * D.ld_user_k + h * dh + c] : 0.f;
    }
    for (int idx = tid; idx < nv * H; idx += RC_TILE) {
      const int j = idx / H, h = idx % H;
      Us[j][h] = D.user_u[((size_t)u * D.L + slot[j]) * D.ld_user_u + h];
    }
    __syncthreads();
    for (int idx = tid; idx < nv * H; idx += RC_TILE) {  // beta_hl = (M c_u W_Q^T)_h . K_hl, pre-scaled
      const int j = idx / H, h = idx % H;
      float b = 0.f;
      if (D.user_q) {
        const float* dq = D.user_q + (size_t)u * D.ld_user_q + h * dh;
        for (int c = 0; c < dh; ++c) b = fmaf(dq[c], Ks[j * DPO + h * DHP + c], b);
      }
      Bs[h][j] = b * sc;
    }
    __syncthreads();
    float logit = item_off;
    if (D.user_off) logit += D.user_off[(size_t)u * D.ld_user_off];
    if (D.ffn_b) logit += D.ffn_b[0];
    if (nv > 0) {  // (a fully masked profile: attention term 0, carca.py:256)
#pragma unroll
      for (int h = 0; h < H; ++h) {
        float m = -INFINITY, den = 0.f, num = 0.f;
        for (int j = 0; j < nv; ++j) {
          const float4* kr = Ks4 + (j * DPO + h * DHP) / 4;
          float s0 = 0.f, s1 = 0.f;
#pragma unroll
          for (int c4 = 0; c4 < DHP / 4; ++c4) {
            const float4 k4 = kr[c4];
            s0 = fmaf(q[h][4 * c4], k4.x, s0);
            s1 = fmaf(q[h][4 * c4 + 1], k4.y, s1);
            s0 = fmaf(q[h][4 * c4 + 2], k4.z, s0);
            s1 = fmaf(q[h][4 * c4 + 3], k4.w, s1);
          }
          const float s = fmaf(s0 + s1, sc, Bs[h][j]);
          const float mn = fmaxf(m, s);
          const float a = exp2f(m - mn), e = exp2f(s - mn);
          den = fmaf(den, a, e);
          num = fmaf(num, a, e * Us[j][h]);
          m = mn;
        }
        logit += num / den;
      }
    }
    if (live) logits[(size_t)u * ld_s + item] = logit;
  }
}

template <int DPI, int DHP, int H>
int rc_launch_ca(const CarcaRecommendDesc& D, float* logits, int ld_s, dim3 grid, int upb, hipStream_t stream) {
  hipLaunchKernelGGL((rc_score_ca_kernel<DPI, DHP, H>), grid, dim3(RC_TILE), 0, stream, D, logits, ld_s, upb);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// ---- 1b. dot-decoder scoring ---------------------------------------------------------------------------------
template <int DPI>
__global__ __launch_bounds__(RC_TILE) void rc_score_dot_kernel(CarcaRecommendDesc D, float* __restrict__ logits, int ld_s,
                                                               int users_per_block) {
  __shared__ float4 As4[DPI / 4], Ms4[DPI / 4];
  __shared__ float am_mm[2];
  const int tid = threadIdx.x;
  const int item = blockIdx.x * RC_TILE + tid;
  const bool live = item >= 1 && item < D.n_items;
  const bool norm = D.decoder == 2, has_m = D.user_m != nullptr;
  float t[DPI];
  float tn = 0.f;
#pragma unroll
  for (int c = 0; c < DPI; ++c) {
    t[c] = (live && c < D.d) ? D.item_q[(size_t)item * D.ld_item_q + c] : 0.f;
    tn = fmaf(t[c], t[c], tn);
  }
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  float* As = reinterpret_cast<float*>(As4);
  float* Ms = reinterpret_cast<float*>(Ms4);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();
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
      if (tid == 0) am_mm[0] = a0, am_mm[1] = m0;
    }
    __syncthreads();
    float dot0 = 0.f, dot1 = 0.f, tm0 = 0.f, tm1 = 0.f;
#pragma unroll
    for (int c4 = 0; c4 < DPI / 4; ++c4) {
      const float4 a4 = As4[c4];
      dot0 = fmaf(t[4 * c4], a4.x, dot0);
      dot1 = fmaf(t[4 * c4 + 1], a4.y, dot1);
      dot0 = fmaf(t[4 * c4 + 2], a4.z, dot0);
      dot1 = fmaf(t[4 * c4 + 3], a4.w, dot1);
    }
    float y = dot0 + dot1 + am_mm[0];
    if (norm) {
      if (has_m) {
#pragma unroll
        for (int c4 = 0; c4 < DPI / 4; ++c4) {
          const float4 m4 = Ms4[c4];
          tm0 = fmaf(t[4 * c4], m4.x, tm0);
          tm1 = fmaf(t[4 * c4 + 1], m4.y, tm1);
          tm0 = fmaf(t[4 * c4 + 2], m4.z, tm0);
          tm1 = fmaf(t[4 * c4 + 3], m4.w, tm1);
        }
      }
      const float n2 = fmaxf(tn + 2.f * (tm0 + tm1) + am_mm[1], 0.f);
      y = y / fmaxf(sqrtf(n2), 1e-12f);  // F.normalize(o): o / max(||o||, eps) (carca.py:388-389)
    }
    if (live) logits[(size_t)u * ld_s + item] = y;
  }
}

template <int DPI>
int rc_launch_dot(const CarcaRecommendDesc& D, float* logits, int ld_s, dim3 grid, int upb, hipStream_t stream) {
  hipLaunchKernelGGL((rc_score_dot_kernel<DPI>), grid, dim3(RC_TILE), 0, stream, D, logits, ld_s, upb);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// ---- 2. exclusion ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rc_exclude_kernel(CarcaRecommendDesc D, float* __restrict__ logits, int ld_s) {
  const int u = blockIdx.x;
  float* row = logits + (size_t)u * ld_s;
  const float sent = __uint_as_float(RC_SENTINEL);
  if (threadIdx.x == 0) row[0] = sent;  // id 0 is the padding item (carca.py:73)
  for (int e = threadIdx.x; e < D.n_exclude; e += 64) {
    const int id = D.exclude[(size_t)u * D.ld_exclude + e];
    if (id > 0 && id < D.n_items) row[id] = sent;  // (0 = no entry; duplicates write the same word)
  }
}

// ---- 3. selection ----------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned rc_order(unsigned bits) {  // float bits -> unsigned with the same order
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ float rc_unorder(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

__global__ __launch_bounds__(RC_SEL_THREADS) void rc_select_kernel(CarcaRecommendDesc D, const float* __restrict__ logits,
                                                                   int ld_s) {
  __shared__ int hist[256];
  __shared__ unsigned long long skey[RC_KMAX];
  __shared__ unsigned long long s_prefix;
  __shared__ int s_pbits, s_need, s_done, s_keff, s_cnt;
  const int tid = threadIdx.x, u = blockIdx.x;
  const unsigned* row = reinterpret_cast<const unsigned*>(logits + (size_t)u * ld_s);
  const int n = D.n_items;
  if (tid == 0) s_prefix = 0ull, s_pbits = 0, s_done = 0, s_cnt = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    hist[tid] = 0;  // (RC_SEL_THREADS == 256 bins)
    __syncthreads();
    const unsigned long long prefix = s_prefix;
    const int pbits = s_pbits;
    for (int i = tid; i < n; i += RC_SEL_THREADS) {
      const unsigned o = rc_order(row[i]);
      if (o == 0u) continue;  // sentinel: excluded
      const unsigned long long key = ((unsigned long long)o << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
      if (pbits > 0 && (key >> (64 - pbits)) != prefix) continue;
      atomicAdd(&hist[(int)((key >> shift) & 255ull)], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int need;
      if (pbits == 0) {  // first pass: the histogram holds every eligible item
        int total = 0;
        for (int b = 0; b < 256; ++b) total += hist[b];
        need = min(D.k, total);
        s_keff = need;
      } else {
        need = s_need;
      }
      if (need == 0) {
        s_done = 1;
      } else {
        int above = 0, b = 255;
        for (; b > 0; --b) {
          if (above + hist[b] >= need) break;
          above += hist[b];
        }
        need -= above;
        s_prefix = (prefix << 8) | (unsigned long long)b;
        s_pbits = pbits + 8;
        s_need = need;
        s_done = hist[b] == need;  // every key under the new prefix is taken: no lower digit matters
      }
    }
    __syncthreads();
    if (s_done) break;
  }
  const int keff = s_keff;
  // collect the keff keys >= prefix (exactly keff of them: keys are unique), sort them descending
  if (tid < RC_KMAX) skey[tid] = 0ull;
  __syncthreads();
  if (keff > 0) {
    const unsigned long long prefix = s_prefix;
    const int pbits = s_pbits;
    for (int i = tid; i < n; i += RC_SEL_THREADS) {
      const unsigned o = rc_order(row[i]);
      if (o == 0u) continue;
      const unsigned long long key = ((unsigned long long)o << 32) | (unsigned)(0xFFFFFFFFu - (unsigned)i);
      if ((key >> (64 - pbits)) >= prefix) {
        const int at = atomicAdd(&s_cnt, 1);
        if (at < RC_KMAX) skey[at] = key;
      }
    }
  }
  __syncthreads();
  for (int size = 2; size <= RC_KMAX; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      if (tid < RC_KMAX) {
        const int p = tid ^ stride;
        if (p > tid) {
          const unsigned long long a = skey[tid], b = skey[p];
          const bool desc = (tid & size) == 0;
          if (desc ? (a < b) : (a > b)) skey[tid] = b, skey[p] = a;
        }
      }
      __syncthreads();
    }
  }
  if (tid < D.k) {
    float score = 0.f;
    long long id = 0;
    if (tid < keff) {
      const unsigned long long key = skey[tid];
      id = (long long)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
      const float y = rc_unorder((unsigned)(key >> 32));
      score = D.decoder == 2 ? (y + 1.f) * 0.5f : 1.f / (1.f + expf(-y));  // carca.py:346, 367, 395-399
    }
    D.scores[(size_t)u * D.ld_scores + tid] = score;
    D.ids_out[(size_t)u * D.ld_ids_out + tid] = id;
  }
}

}  // namespace

extern "C" int carca_recommend(const CarcaRecommendDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "recommend: null descriptor");
  const CarcaRecommendDesc& D = *desc;
  CARCA_CHECK_ARG(D.B >= 1 && D.L >= 1 && D.n_items >= 1 && D.d >= 1 && D.H >= 1 && D.k >= 1,
                  "recommend: B, L, n_items, d, H and k must be positive");
  CARCA_CHECK_SUPPORTED(D.L <= CARCA_MAX_L, "recommend: profile length L = %d exceeds CARCA_MAX_L = %d", D.L, CARCA_MAX_L);
  CARCA_CHECK_SUPPORTED(D.k <= RC_KMAX, "recommend: k = %d exceeds the largest k, 128", D.k);
  CARCA_CHECK_ARG(D.decoder >= 0 && D.decoder <= 2, "recommend: decoder must be 0 (cross-attention), 1 (dot) or 2 (normalised dot)");
  CARCA_CHECK_ARG(D.p_ids && D.item_q && D.scores && D.ids_out, "recommend: null pointer");
  CARCA_CHECK_ARG(D.ld_p_ids >= D.L && D.ld_item_q >= D.d && D.ld_scores >= D.k && D.ld_ids_out >= D.k,
                  "recommend: row stride shorter than its row");
  CARCA_CHECK_ARG(D.ld_item_q % 4 == 0, "recommend: ld_item_q must be a multiple of 4");
  CARCA_CHECK_ARG(D.n_exclude >= 0 && (D.n_exclude == 0 || (D.exclude && D.ld_exclude >= D.n_exclude)),
                  "recommend: bad exclusion list");
  CARCA_CHECK_SUPPORTED(D.d % D.H == 0 && D.d <= 128, "recommend: d = %d, H = %d: no kernel (d %% H != 0 or d > 128)", D.d,
                        D.H);
  int dpi = 0, dhp = 0, dpo = 0;
  carca_padded_dims(D.d, D.H, &dpi, &dhp, &dpo);
  const int H = D.H;
  if (D.decoder == 0) {
    CARCA_CHECK_ARG(D.user_k && D.user_u && D.ld_user_k >= D.d && D.ld_user_u >= D.H && D.ld_user_k % 4 == 0,
                    "recommend: cross-attention needs user_k / user_u");
    CARCA_CHECK_ARG(!D.user_q || (D.ld_user_q >= D.d && D.ld_user_q % 4 == 0), "recommend: bad ld_user_q");
    CARCA_CHECK_ARG(!D.item_w || D.ld_item_w >= 1, "recommend: bad ld_item_w");
    CARCA_CHECK_ARG(!D.user_off || D.ld_user_off >= 1, "recommend: bad ld_user_off");
    CARCA_CHECK_SUPPORTED(carca_attn_geometry_built(D.d, D.H),
                          "recommend: no cross-attention kernel built for d = %d, H = %d (see CARCA_ATT_GEOMETRIES)", D.d,
                          D.H);
  } else {
    CARCA_CHECK_ARG(D.user_q && D.ld_user_q >= D.d && D.ld_user_q % 4 == 0, "recommend: dot decoders need user_q");
    CARCA_CHECK_ARG(!D.user_m || (D.ld_user_m >= D.d && D.ld_user_m % 4 == 0), "recommend: bad ld_user_m");
  }
  // raw logits [B, n_items]: stream scratch (or the capture's memory), consumed by the two launches behind the scoring one
  const int ld_s = D.n_items;
  const size_t bytes = (size_t)D.B * (size_t)ld_s * sizeof(float);
  float* logits = (float*)(carca_stream_capturing(stream) ? carca_capture_alloc(stream, bytes, false, nullptr)
                                                          : carca_stream_scratch(stream, CARCA_SCRATCH_RECOMMEND, bytes));
  CARCA_CHECK_ARG(logits, "recommend: scratch allocation of %zu bytes failed", bytes);
  // grid: item tiles x user chunks, about two workgroups per CU; each workgroup keeps its tile's rows in registers
  const int tiles = (D.n_items + RC_TILE - 1) / RC_TILE;
  const int chunks = max(1, min(D.B, (2 * carca_num_cus() + tiles - 1) / tiles));
  const int upb = (D.B + chunks - 1) / chunks;
  const dim3 grid(tiles, (D.B + upb - 1) / upb);
  int rc = CARCA_ERR_UNSUPPORTED;
  if (D.decoder == 0) {
    rc = [&]() -> int {
      CARCA_ATT_DISPATCH(rc_launch_ca, D, logits, ld_s, grid, upb, stream);
      carca_set_error("recommend: no cross-attention kernel for (dpi %d, dhp %d, H %d)", dpi, dhp, H);
      return CARCA_ERR_UNSUPPORTED;
    }();
  } else if (dpi == 64) {
    rc = rc_launch_dot<64>(D, logits, ld_s, grid, upb, stream);
  } else if (dpi == 96) {
    rc = rc_launch_dot<96>(D, logits, ld_s, grid, upb, stream);
  } else {
    rc = rc_launch_dot<128>(D, logits, ld_s, grid, upb, stream);
  }
  if (rc != CARCA_OK) return rc;
  hipLaunchKernelGGL(rc_exclude_kernel, dim3(D.B), dim3(64), 0, stream, D, logits, ld_s);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(rc_select_kernel, dim3(D.B), dim3(RC_SEL_THREADS), 0, stream, D, logits, ld_s);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
