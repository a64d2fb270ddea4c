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
// Launches 2 and 3 live in catalogue_select.h, shared with carca_knn_recommend (knn_catalogue.hip).
// Integer LDS atomics only (histograms, slot counters); the result does not depend on scheduling.
#include "catalogue_select.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int RC_TILE = rc::TILE;     // items per scoring workgroup (one per lane)
using rc::RC_KMAX;
using rc::RC_SEL_THREADS;

// ---- 1a. cross-attention scoring (per-(user, item) arithmetic: recommend_common.h) -------------------------------
template <int DPI, int DHP, int H>
__global__ __launch_bounds__(RC_TILE) void rc_score_ca_kernel(CarcaRecommendDesc D, float* __restrict__ logits, int ld_s,
                                                              int users_per_block) {
  __shared__ rc::CaUser<DHP, H> S;
  const float sc = rc::ca_scale<H>(D);
  const int item = blockIdx.x * RC_TILE + threadIdx.x;
  const bool live = item >= 1 && item < D.n_items;
  float q[H][DHP];
  float item_off;
  rc::ca_load_item(D, item, live, q, item_off);
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous user's LDS is read out
    const int nv = rc::ca_stage_user(D, u, sc, S);
    const float logit = rc::ca_logit(D, u, q, item_off, nv, sc, S);
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
  __shared__ rc::DotUser<DPI> S;
  const int item = blockIdx.x * RC_TILE + threadIdx.x;
  const bool live = item >= 1 && item < D.n_items;
  float t[DPI];
  float tn;
  rc::dot_load_item(D, item, live, t, tn);
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();
    rc::dot_stage_user(D, u, S);
    const float y = rc::dot_logit(D, t, tn, S);
    if (live) logits[(size_t)u * ld_s + item] = y;
  }
}

template <int DPI>
int rc_launch_dot(const CarcaRecommendDesc& D, float* logits, int ld_s, dim3 grid, int upb, hipStream_t stream) {
  hipLaunchKernelGGL((rc_score_dot_kernel<DPI>), grid, dim3(RC_TILE), 0, stream, D, logits, ld_s, upb);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
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
  hipLaunchKernelGGL(rc::rc_exclude_kernel<CarcaRecommendDesc>, dim3(D.B), dim3(64), 0, stream, D, logits, ld_s);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(rc::rc_select_kernel<CarcaRecommendDesc>, dim3(D.B), dim3(RC_SEL_THREADS), 0, stream, D, logits, ld_s);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
