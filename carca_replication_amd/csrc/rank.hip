// Exact full-catalogue ranks of listed items (include/carca_hip.h: carca_rank_items).
//
// The full-ranking protocol asks where the held-out item lands among all items; carca_recommend answers a different
// question (the k best) and cannot place an item beyond k = 128.  Here the rank of a target is a count: the eligible items
// whose key (recommend_common.h: logit bits, then the complemented id) is larger than the target's.  Every logit comes from
// the same helpers as carca_recommend's, so the two calls agree bit for bit.  Three launches, no host wait, nothing
// retained:
//   1. list scoring, one workgroup per user: the n_list targets and the n_exclude excluded entries are scored with the
//      user staged in LDS as the sweep stages it; their keys go to stream scratch, the targets' linked scores to `scores`,
//      and the user's [n_list] counter is zeroed;
//   2. counting sweep, the tiling of recommend's scoring kernel (a 256-item tile in registers walking a chunk of users):
//      each lane compares its item's key with the user's target keys (LDS), a wave counts with ballot + popcount, the
//      four waves sum in LDS and one integer atomic per (workgroup, user, target) with a non-zero count goes to the
//      counter.  No exclusion test (id 0 is never live) and no [B, n_items] buffer;
//   3. correction, one workgroup per user: the distinct excluded ids (not 0, inside [0, n_items)) whose key is larger than
//      the target's are subtracted; an excluded target has its own key, which is not larger than itself.
// Integer atomics only: the counts do not depend on scheduling.
#include "recommend_common.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int RK_TILE = rc::TILE;
constexpr int RK_NMAX = 128;    // largest list
constexpr int RK_WAVES = RK_TILE / 64;
constexpr int RK_EX_CHUNK = 1024;  // exclusion keys the correction holds in LDS at a time
constexpr unsigned long long RK_NEVER = ~0ull;  // key of an invalid target: no item orders before it

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
  W.keys[(size_t)u * W.ldk + idx] = valid ? rc::item_key(logit, id) : (target ? RK_NEVER : 0ull);
  if (target) D.scores[(size_t)u * D.ld_scores + idx] = valid ? rc::link(logit, D.decoder) : 0.f;
}

// ---- 1. list scoring ---------------------------------------------------------------------------------------------
template <int DPI, int DHP, int H>
__global__ __launch_bounds__(RK_TILE) void rk_list_ca_kernel(CarcaRankDesc D, RkScratch W) {
  __shared__ rc::CaUser<DHP, H> S;
  const int u = blockIdx.x, tid = threadIdx.x;
  const float sc = rc::ca_scale<H>(D);
  for (int t = tid; t < D.n_list; t += RK_TILE) W.counts[(size_t)u * D.n_list + t] = 0;
  const int nv = rc::ca_stage_user(D, u, sc, S);
  for (int idx = tid; idx < D.n_list + D.n_exclude; idx += RK_TILE) {
    const int id = rk_list_id(D, u, idx);
    const bool valid = rk_valid(id, D.n_items);
    float q[H][DHP];
    float item_off;
    rc::ca_load_item(D, id, valid, q, item_off);
    rk_store_list(D, W, u, idx, id, valid, rc::ca_logit(D, u, q, item_off, nv, sc, S));
  }
}

template <int DPI>
__global__ __launch_bounds__(RK_TILE) void rk_list_dot_kernel(CarcaRankDesc D, RkScratch W) {
  __shared__ rc::DotUser<DPI> S;
  const int u = blockIdx.x, tid = threadIdx.x;
  for (int t = tid; t < D.n_list; t += RK_TILE) W.counts[(size_t)u * D.n_list + t] = 0;
  rc::dot_stage_user(D, u, S);
  for (int idx = tid; idx < D.n_list + D.n_exclude; idx += RK_TILE) {
    const int id = rk_list_id(D, u, idx);
    const bool valid = rk_valid(id, D.n_items);
    float t[DPI];
    float tn;
    rc::dot_load_item(D, id, valid, t, tn);
    rk_store_list(D, W, u, idx, id, valid, rc::dot_logit(D, t, tn, S));
  }
}

// ---- 2. counting sweep ---------------------------------------------------------------------------------------------
struct RkCountLds {
  unsigned long long tkey[RK_NMAX];
  int wcnt[RK_WAVES][RK_NMAX];
};

// the user's target keys into LDS (before the user's staging, whose barriers publish them)
__device__ __forceinline__ void rk_stage_targets(const CarcaRankDesc& D, RkScratch W, int u, RkCountLds& C) {
  for (int t = threadIdx.x; t < D.n_list; t += RK_TILE) C.tkey[t] = W.keys[(size_t)u * W.ldk + t];
}

// counts, per target, the lanes whose key is larger; one atomic per target with a non-zero count
__device__ __forceinline__ void rk_count(const CarcaRankDesc& D, RkScratch W, int u, unsigned long long key,
                                         RkCountLds& C) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int c0 = 0, c1 = 0;  // lane l keeps the wave's count for targets l and l + 64
  for (int t = 0; t < D.n_list; ++t) {
    const int pc = __popcll(__ballot(key > C.tkey[t]));
    if (t < 64) {
      c0 = lane == t ? pc : c0;
    } else {
      c1 = lane == t - 64 ? pc : c1;
    }
  }
  C.wcnt[w][lane] = c0;
  C.wcnt[w][lane + 64] = c1;
  __syncthreads();
  if (tid < D.n_list) {
    int s = 0;
#pragma unroll
    for (int v = 0; v < RK_WAVES; ++v) s += C.wcnt[v][tid];
    if (s) atomicAdd(&W.counts[(size_t)u * D.n_list + tid], s);
  }
}

template <int DPI, int DHP, int H>
__global__ __launch_bounds__(RK_TILE) void rk_count_ca_kernel(CarcaRankDesc D, RkScratch W, int users_per_block) {
  __shared__ rc::CaUser<DHP, H> S;
  __shared__ RkCountLds C;
  const float sc = rc::ca_scale<H>(D);
  const int item = blockIdx.x * RK_TILE + threadIdx.x;
  const bool live = item >= 1 && item < D.n_items;
  float q[H][DHP];
  float item_off;
  rc::ca_load_item(D, item, live, q, item_off);
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();  // the previous user's LDS is read out
    rk_stage_targets(D, W, u, C);
    const int nv = rc::ca_stage_user(D, u, sc, S);
    const float logit = rc::ca_logit(D, u, q, item_off, nv, sc, S);
    rk_count(D, W, u, live ? rc::item_key(logit, item) : 0ull, C);
  }
}

template <int DPI>
__global__ __launch_bounds__(RK_TILE) void rk_count_dot_kernel(CarcaRankDesc D, RkScratch W, int users_per_block) {
  __shared__ rc::DotUser<DPI> S;
  __shared__ RkCountLds C;
  const int item = blockIdx.x * RK_TILE + threadIdx.x;
  const bool live = item >= 1 && item < D.n_items;
  float t[DPI];
  float tn;
  rc::dot_load_item(D, item, live, t, tn);
  const int u0 = blockIdx.y * users_per_block, u1 = min(D.B, u0 + users_per_block);
  for (int u = u0; u < u1; ++u) {
    __syncthreads();
    rk_stage_targets(D, W, u, C);
    rc::dot_stage_user(D, u, S);
    const float y = rc::dot_logit(D, t, tn, S);
    rk_count(D, W, u, live ? rc::item_key(y, item) : 0ull, C);
  }
}

template <int DPI, int DHP, int H>
int rk_launch_ca(const CarcaRankDesc& D, RkScratch W, dim3 grid, int upb, hipStream_t stream) {
  hipLaunchKernelGGL((rk_list_ca_kernel<DPI, DHP, H>), dim3(D.B), dim3(RK_TILE), 0, stream, D, W);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL((rk_count_ca_kernel<DPI, DHP, H>), grid, dim3(RK_TILE), 0, stream, D, W, upb);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

template <int DPI>
int rk_launch_dot(const CarcaRankDesc& D, RkScratch W, dim3 grid, int upb, hipStream_t stream) {
  hipLaunchKernelGGL((rk_list_dot_kernel<DPI>), dim3(D.B), dim3(RK_TILE), 0, stream, D, W);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL((rk_count_dot_kernel<DPI>), grid, dim3(RK_TILE), 0, stream, D, W, upb);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// ---- 3. correction -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RK_TILE) void rk_correct_kernel(CarcaRankDesc D, RkScratch W) {
  __shared__ unsigned long long ekey[RK_EX_CHUNK];
  const int u = blockIdx.x, tid = threadIdx.x;
  const unsigned long long* row = W.keys + (size_t)u * W.ldk;
  const int32_t* ex = D.exclude + (size_t)u * D.ld_exclude;
  const unsigned long long tk = tid < D.n_list ? row[tid] : RK_NEVER;
  int corr = 0;
  for (int base = 0; base < D.n_exclude; base += RK_EX_CHUNK) {
    const int n = min(RK_EX_CHUNK, D.n_exclude - base);
    __syncthreads();  // the previous chunk is read out
    for (int j = tid; j < n; j += RK_TILE) {  // keep an entry's key only at the first occurrence of its id
      const int e = base + j, id = ex[e];
      bool first = rk_valid(id, D.n_items);
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

}  // namespace

extern "C" int carca_rank_items(const CarcaRankDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "rank_items: null descriptor");
  const CarcaRankDesc& D = *desc;
  CARCA_CHECK_ARG(D.B >= 1 && D.L >= 1 && D.n_items >= 1 && D.d >= 1 && D.H >= 1,
                  "rank_items: B, L, n_items, d and H must be positive");
  CARCA_CHECK_SUPPORTED(D.L <= CARCA_MAX_L, "rank_items: profile length L = %d exceeds CARCA_MAX_L = %d", D.L,
                        CARCA_MAX_L);
  CARCA_CHECK_SUPPORTED(D.n_list >= 1 && D.n_list <= RK_NMAX, "rank_items: n_list = %d outside 1..128", D.n_list);
  CARCA_CHECK_ARG(D.decoder >= 0 && D.decoder <= 2,
                  "rank_items: decoder must be 0 (cross-attention), 1 (dot) or 2 (normalised dot)");
  CARCA_CHECK_ARG(D.p_ids && D.item_q && D.items && D.scores && D.ranks, "rank_items: null pointer");
  CARCA_CHECK_ARG(D.ld_p_ids >= D.L && D.ld_item_q >= D.d && D.ld_items >= D.n_list && D.ld_scores >= D.n_list &&
                      D.ld_ranks >= D.n_list,
                  "rank_items: row stride shorter than its row");
  CARCA_CHECK_ARG(D.ld_item_q % 4 == 0, "rank_items: ld_item_q must be a multiple of 4");
  CARCA_CHECK_ARG(D.n_exclude >= 0 && (D.n_exclude == 0 || (D.exclude && D.ld_exclude >= D.n_exclude)),
                  "rank_items: bad exclusion list");
  CARCA_CHECK_SUPPORTED(D.d % D.H == 0 && D.d <= 128, "rank_items: d = %d, H = %d: no kernel (d %% H != 0 or d > 128)",
                        D.d, D.H);
  int dpi = 0, dhp = 0, dpo = 0;
  carca_padded_dims(D.d, D.H, &dpi, &dhp, &dpo);
  const int H = D.H;
  if (D.decoder == 0) {
    CARCA_CHECK_ARG(D.user_k && D.user_u && D.ld_user_k >= D.d && D.ld_user_u >= D.H && D.ld_user_k % 4 == 0,
                    "rank_items: cross-attention needs user_k / user_u");
    CARCA_CHECK_ARG(!D.user_q || (D.ld_user_q >= D.d && D.ld_user_q % 4 == 0), "rank_items: bad ld_user_q");
    CARCA_CHECK_ARG(!D.item_w || D.ld_item_w >= 1, "rank_items: bad ld_item_w");
    CARCA_CHECK_ARG(!D.user_off || D.ld_user_off >= 1, "rank_items: bad ld_user_off");
    CARCA_CHECK_SUPPORTED(carca_attn_geometry_built(D.d, D.H),
                          "rank_items: no cross-attention kernel built for d = %d, H = %d (see CARCA_ATT_GEOMETRIES)",
                          D.d, D.H);
  } else {
    CARCA_CHECK_ARG(D.user_q && D.ld_user_q >= D.d && D.ld_user_q % 4 == 0, "rank_items: dot decoders need user_q");
    CARCA_CHECK_ARG(!D.user_m || (D.ld_user_m >= D.d && D.ld_user_m % 4 == 0), "rank_items: bad ld_user_m");
  }
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
  // sweep grid: recommend's (item tiles x user chunks, about two workgroups per CU)
  const int tiles = (D.n_items + RK_TILE - 1) / RK_TILE;
  const int chunks = max(1, min(D.B, (2 * carca_num_cus() + tiles - 1) / tiles));
  const int upb = (D.B + chunks - 1) / chunks;
  const dim3 grid(tiles, (D.B + upb - 1) / upb);
  int rc = CARCA_ERR_UNSUPPORTED;
  if (D.decoder == 0) {
    rc = [&]() -> int {
      CARCA_ATT_DISPATCH(rk_launch_ca, D, W, grid, upb, stream);
      carca_set_error("rank_items: no cross-attention kernel for (dpi %d, dhp %d, H %d)", dpi, dhp, H);
      return CARCA_ERR_UNSUPPORTED;
    }();
  } else if (dpi == 64) {
    rc = rk_launch_dot<64>(D, W, grid, upb, stream);
  } else if (dpi == 96) {
    rc = rk_launch_dot<96>(D, W, grid, upb, stream);
  } else {
    rc = rk_launch_dot<128>(D, W, grid, upb, stream);
  }
  if (rc != CARCA_OK) return rc;
  hipLaunchKernelGGL(rk_correct_kernel, dim3(D.B), dim3(RK_TILE), 0, stream, D, W);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}
