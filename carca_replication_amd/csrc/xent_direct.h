// The direct-staged tile kernel of the two losses whose classes are the catalogue's items themselves: catalogue_xent.hip
//  and policy_xent.hip (a temperature, per-row exclusion lists, per-row coefficients, the entropy;
// section 29).  What lives here, once: xd_tile_kernel<RULE, MODE, NCB>: the LDS carve-up, both tiles staged straight into
// LDS behind the barrier (xt_stage_direct), the bounds tests of a stream entry (item ids 1 .. s_end-1, or the valid rows
// of the split), the 64-bit mask word of a step shifted once to the lane's first entry, and xent_tile.h's two products
// and epilogue around them.  A loss supplies a rule struct (CatalogueRule, PolicyRule<ENT, LISTS>) for what differs:
// the lane's state beyond (lse, pos, max, sum-exp), what a stream row carries in DT, the mask word, the logit's
// transform, G of an eligible entry, and the forward's tile step and partial store.  Each file keeps its rule, its merge
// kernel and its entry points.
#pragma once
#include "xent_tile.h"

#include <type_traits>

namespace {

// RULE: all members static and __forceinline__
//   Args                                   what the kernel takes by value after XentTile (X below; may be empty)
//   ROW_WORDS                              DT: 4-byte words of LDS per stream row (s_row: ROW_WORDS arrays of XT_TILE)
//   SCALED                                 whether xt_epilogue scales the final class gradient by grad / n_valid
//   LISTS                                  whether an own entry has a sorted list of stream entries that are masked for it
//   Lane                                   the lane's state beside the kernel's own (o_lse, o_pos, run_m, run_s), default-
//                                          initialised; may be empty
//   own<MODE>(A, X, nv, o_idx, s_begin, o_lse, x)   fills it (not called for an empty Lane): o_idx is a valid-row index
//                                          (FWD / DP) or an item (DT)
//   stage_row(A, X, s_row, v, in, tid)     DT, threads 0..63: the words of stream row v (in: v lies in the split)
//   step_mask(x, s0)                       LISTS: bit b set iff stream entry s0 + b is masked for the own entry
//   logit(X, z)                            the logit of a product (zt below)
//   g_own(z, n, j, zt, si, o_lse, o_pos, x)   DP: G of eligible item si for the own row, from the product z[n][j] or zt
//   g_stream(z, n, j, zt, s_row, sl, o_idx)   DT: G of own item o_idx for stream row sl
//   fwd_logit(z, n, j, zt, ok)             FWD: z[n][j] becomes the logit, or -inf where not ok
//   fwd_tile(z, run_m, run_s, x)           FWD: after a tile's 16 logits
//   fwd_store(A, X, run_m, run_s, x, split, o_idx, q, nv)   FWD: the four-lane merge and the partial's store
// The shape of these hooks is what keeps both clients' code: the catalogue's lane state stays in plain locals here, own()
// is skipped for an empty Lane, and a hook gets the product both in place (z, n, j: what the catalogue reads, inside its
// branch) and as the logit computed in front of the branch (zt: what the policy reads).  Each simpler form changed the
// instruction stream of some catalogue instantiation ("One tile kernel").
// NCB: 16-column blocks the kernel is built for (d <= 16 NCB)
template <class RULE, int MODE, int NCB>
__global__ __launch_bounds__(XT_THREADS) void xd_tile_kernel(XentTile A, typename RULE::Args X) {
  extern __shared__ float xd_lds[];
  float* own = xd_lds;
  float* str = xd_lds + XT_TILE * A.pitch;
  float* s_row = str + XT_TILE * A.pitch;  // DT: RULE::stage_row's words of the stream rows
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16);
  const int own0 = blockIdx.x * XT_TILE, split = blockIdx.y;
  int s_begin, s_end;
  if (MODE != XT_DT && own0 >= nv) return;  // (grid sized for R; rows past n_valid have nothing to do)
  xt_split_range<MODE>(A, nv, split, s_begin, s_end);
  constexpr bool OWN_ROWS = MODE != XT_DT;
  xt_stage_direct(A, own, own0, OWN_ROWS ? nv : A.n, OWN_ROWS, kpad, tid);

  // this lane's own entry (column r16 of the wave's Z^T tiles)
  const int o_idx = own0 + 16 * w + r16;
  float o_lse = 0.f;
  int o_pos = -1;
  if constexpr (MODE == XT_DP) {
    if (o_idx < nv) {
      const int r = A.ridx[o_idx];
      o_lse = A.lse[r];
      o_pos = A.pos[r];
    }
  }
  typename RULE::Lane x;  // what the rule keeps per lane beside these
  if constexpr (!std::is_empty_v<typename RULE::Lane>) RULE::template own<MODE>(A, X, nv, o_idx, s_begin, o_lse, x);
  float run_m = -INFINITY, run_s = 0.f;  // FWD
  f32x4 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += XT_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    xt_stage_direct(A, str, s0, s_end, !OWN_ROWS, kpad, tid);
    if constexpr (MODE == XT_DT) {
      if (tid < XT_TILE) RULE::stage_row(A, X, s_row, s0 + tid, s0 + tid < s_end, tid);
    }
    // (shifted once to the lane's first stream entry 4q: the 16 tests below then read bits at compile-time offsets)
    unsigned long long mask = 0ull;
    if constexpr (RULE::LISTS) mask = RULE::step_mask(x, s0) >> (4 * q);
    __syncthreads();
    f32x4 z[4];
    xt_logits<NCB>(A, own_row, str, r16, q, z);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sl = 16 * n + 4 * q + j, si = s0 + sl;
        const bool listed = RULE::LISTS && ((mask >> (16 * n + j)) & 1ull);
        const float zt = RULE::logit(X, z[n][j]);
        if constexpr (MODE == XT_FWD) {
          // items s0 + 16n + 4q + j of own row r16: id 0, ids past the split and listed ids are not classes (-inf)
          RULE::fwd_logit(z, n, j, zt, si >= 1 && si < s_end && !listed);
        } else {
          // G[own r16][stream 16n + 4q + j] (0 outside the valid rows and the eligible classes)
          float g = 0.f;
          if constexpr (MODE == XT_DP) {
            if (o_idx < nv && si >= 1 && si < s_end && !listed) g = RULE::g_own(z, n, j, zt, si, o_lse, o_pos, x);
          } else {
            if (si < s_end && o_idx >= 1 && o_idx < A.n && !listed) g = RULE::g_stream(z, n, j, zt, s_row, sl, o_idx);
          }
          z[n][j] = g;
        }
      }
    if constexpr (MODE == XT_FWD) RULE::fwd_tile(z, run_m, run_s, x);
    else xt_accumulate<NCB>(A, z, str, r16, q, acc);
  }

  if constexpr (MODE == XT_FWD) RULE::fwd_store(A, X, run_m, run_s, x, split, o_idx, q, nv);
  else xt_epilogue<MODE, NCB, RULE::SCALED>(A, acc, nv, own0, split, w, lane);
}

// the tile kernels of one rule and mode, with the rule's LDS words per stream row
template <class RULE, int MODE>
XentKernelsT<typename RULE::Args> xd_kernels() {
  return {xd_tile_kernel<RULE, MODE, 4>, xd_tile_kernel<RULE, MODE, 8>, xd_tile_kernel<RULE, MODE, 16>, RULE::ROW_WORDS};
}

}  // namespace
