// Full-catalogue softmax cross-entropy for the dot decoders (include/carca_hip.h: carca_catalogue_xent_fwd / _bwd;
// DESIGN.md section 13).
//
//   CE = sum over valid rows r of ( logsumexp_{i = 1 .. n_items-1} P[r] . T[i]  -  P[r] . T[pos_r] ) / n_valid
//
// with no [R, n_items] buffer: the forward keeps a running (max, sum-exp) per row over the item tiles, the backward
// recomputes every logit tile and multiplies G = softmax - onehot into dP = G T and dT = G^T P straight away.
// Launches, no host wait:
//   1. compact: one workgroup lists the valid rows (pos in [1, n_items)) in row order: ridx[v] = r, rpos[r] = v or -1,
//      nv = n_valid (device-side; every later launch reads it);
//   2. tile: a workgroup owns 64 rows of one operand (the "own" tile, staged once in LDS) and streams 64-row tiles of the
//      other through LDS.  Each of its four waves owns 16 own rows and computes the 64 x 16 logit tile Z^T = S O^T with
//      v_mfma_f32_16x16x4_f32 (exact fp32 products), the K loop over round_up(d, 16) columns, zero-filled past d when the
//      tiles are staged.  The D layout (column = own row l & 15, row = stream row 4 (l >> 4) + reg) is exactly the A
//      operand of the second product (k = stream row), so G never leaves the registers:
//        FWD  own = rows, stream = the items of one split: lane-local running (max, sum-exp) of own row l & 15, merged
//             over the four lanes of that row at the end, one (max, sum) partial per (split, row);
//        DP   own = rows, stream = items: partial dP[split][v] = sum over the split's items of G T;
//        DT   own = items, stream = the valid rows of one split: dT[i] (or its partial) = sum over rows of G^T P;
//   3. FWD: merge the split partials per row in split order, lse = M + log(sum), row loss = lse - P[r] . T[pos_r]; one
//      workgroup sums the row losses in a fixed order (fp64) into the mean;
//      BWD: the split partials of dP (and of dT, when the rows are split) are summed in split order and scaled by
//      grad / n_valid; padding rows get dP = 0, item 0 and the columns past d get 0.
// No float atomics: every sum has one fixed order, so two calls give the same bits.
// The tile skeleton (split range, both MFMA products, the running (max, sum-exp), the lane merge, the epilogue, the
// helper kernels, the launch sequences) is xent_tile.h's and the tile kernel xent_direct.h's, shared with policy_xent.hip;
// this file keeps its rule (the own row's lse and pos, G = softmax - onehot), its merge kernel and its entry points.
#include "xent_direct.h"

namespace {

// ---- 2. logit tiles: the rule for xd_tile_kernel ---------------------------------------------------------------------
struct CatalogueRule {
  struct Args {};
  static constexpr int ROW_WORDS = 2;  // DT: lse and pos of each stream row
  static constexpr bool SCALED = true, LISTS = false;

  struct Lane {};  // (no lane state beside the kernel's own lse and pos: own() is not called)
  static __device__ __forceinline__ void stage_row(const XentTile& A, const Args&, float* s_row, int v, bool in, int tid) {
    const int r = in ? A.ridx[v] : 0;
    s_row[tid] = in ? A.lse[r] : 0.f;
    reinterpret_cast<int*>(s_row + XT_TILE)[tid] = in ? A.pos[r] : -1;
  }

  static __device__ __forceinline__ float logit(const Args&, float z) { return z; }

  // G = softmax - onehot
  static __device__ __forceinline__ float g_own(const f32x4 (&z)[4], int n, int j, float, int si, float o_lse,
                                               int o_pos, const Lane&) {
    return __expf(z[n][j] - o_lse) - (si == o_pos ? 1.f : 0.f);
  }
  static __device__ __forceinline__ float g_stream(const f32x4 (&z)[4], int n, int j, float, const float* s_row,
                                                  int sl, int o_idx) {
    return __expf(z[n][j] - s_row[sl]) - (reinterpret_cast<const int*>(s_row + XT_TILE)[sl] == o_idx ? 1.f : 0.f);
  }

  // FWD: -inf where masked; the lane's running (max, sum-exp)
  static __device__ __forceinline__ void fwd_logit(f32x4 (&z)[4], int n, int j, float, bool ok) {
    if (!ok) z[n][j] = -INFINITY;
  }
  static __device__ __forceinline__ void fwd_tile(const f32x4 (&z)[4], float& m, float& s, Lane&) {
    xt_running_update(z, m, s);
  }
  static __device__ __forceinline__ void fwd_store(const XentTile& A, const Args&, float m, float s, const Lane&, int split,
                                                   int o_idx, int q, int nv) {
    xt_store_partial(A, m, s, split, o_idx, q, nv);
  }
};

// ---- 3. merges (cx_mean_kernel and cx_reduce_kernel: xent_tile.h) ----------------------------------------------------

__global__ __launch_bounds__(256) void cx_merge_kernel(CarcaCatalogueXentDesc D, const int32_t* __restrict__ rpos,
                                                       const float* __restrict__ part_m, const float* __restrict__ part_s) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= D.R) return;
  const int v = rpos[r];
  if (v < 0) {
    D.lse[r] = 0.f;
    D.row_loss[r] = 0.f;
    return;
  }
  float M = -INFINITY;
  for (int s = 0; s < D.splits_items; ++s) M = fmaxf(M, part_m[(size_t)s * D.R + v]);
  float sum = 0.f;
  for (int s = 0; s < D.splits_items; ++s) {
    const float m = part_m[(size_t)s * D.R + v];
    if (m > -INFINITY) sum += part_s[(size_t)s * D.R + v] * expf(m - M);
  }
  const float lse = M + logf(sum);
  const float* p = D.P + (size_t)r * D.ld_p;
  const float* t = D.T + (size_t)D.pos[r] * D.ld_t;
  float zp = 0.f;
  for (int k = 0; k < D.d; ++k) zp = fmaf(p[k], t[k], zp);
  D.lse[r] = lse;
  D.row_loss[r] = lse - zp;
}

// ---- host side -----------------------------------------------------------------------------------------------------
XentCall cx_call(const CarcaCatalogueXentDesc& D) {
  XentCall C = {};
  XentTile& A = C.A;
  A.R = D.R, A.n = D.n_items, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_t;
  A.P = D.P, A.T = D.T, A.pos = D.pos;
  A.lse = D.lse, A.grad = D.grad;
  A.per_split = D.items_per_split;
  C.op = "catalogue_xent", C.classes = "items";
  C.scratch = D.scratch, C.scratch_floats = D.scratch_floats;
  C.splits_n = D.splits_items, C.splits_rows = D.splits_rows;
  C.row_loss = D.row_loss, C.loss = D.loss, C.dP = D.dP, C.dT = D.dT;
  return C;
}

}  // namespace

extern "C" int carca_catalogue_xent_fwd(const CarcaCatalogueXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "catalogue_xent_fwd: null descriptor");
  const CarcaCatalogueXentDesc& D = *desc;
  XentCall C = cx_call(D);
  return xt_forward(
      C, xd_kernels<CatalogueRule, XT_FWD>(), stream,
      [&](const int32_t* rpos, const float* part_m, const float* part_s) {
        hipLaunchKernelGGL(cx_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D, rpos, part_m, part_s);
      },
      CatalogueRule::Args{});
}

extern "C" int carca_catalogue_xent_bwd(const CarcaCatalogueXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "catalogue_xent_bwd: null descriptor");
  XentCall C = cx_call(*desc);
  return xt_backward(C, xd_kernels<CatalogueRule, XT_DP>(), xd_kernels<CatalogueRule, XT_DT>(), stream,
                     [](const int32_t*, const int32_t*, float*, int) {}, CatalogueRule::Args{});
}
