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
// launch sequences) is xent_tile.h's, shared with sampled_xent.hip; this file keeps its staging (straight into LDS behind
// the barrier), its mask / G rule and its merge kernel.
#include "xent_tile.h"

namespace {

// ---- 2. logit tiles ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void cx_stage(const XentTile& A, float* dst, int first, int end, bool rows, int kpad, int tid) {
  // rows: entries first .. end-1 are valid-row indices (P[ridx[v]]); else item ids (T[i]).  Zero past `end` and past d.
  const int nc4 = kpad / 4;
  for (int idx = tid; idx < XT_TILE * nc4; idx += XT_THREADS) {
    const int row = idx / nc4, c = 4 * (idx - row * nc4);
    const int e = first + row;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (e < end && c < A.d) {
      const float* src = rows ? A.P + (size_t)A.ridx[e] * A.ld_p : A.T + (size_t)e * A.ld_t;
      v = *reinterpret_cast<const f32x4*>(src + c);  // (ld % 4 == 0 and c < d <= ld: the 16 bytes lie in the row)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (c + j >= A.d) v[j] = 0.f;
    }
    *reinterpret_cast<f32x4*>(dst + row * A.pitch + c) = v;
  }
}

// NCB: 16-column blocks the kernel is built for (d <= 16 NCB)
template <int MODE, int NCB>
__global__ __launch_bounds__(XT_THREADS) void cx_tile_kernel(XentTile A) {
  extern __shared__ float cx_lds[];
  float* own = cx_lds;
  float* str = cx_lds + XT_TILE * A.pitch;
  float* s_lse = str + XT_TILE * A.pitch;                       // DT: lse of the stream rows
  int* s_pos = reinterpret_cast<int*>(s_lse + XT_TILE);         // DT: pos of the stream rows
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16);
  const int own0 = blockIdx.x * XT_TILE, split = blockIdx.y;
  int s_begin, s_end;
  if (MODE != XT_DT && own0 >= nv) return;  // (grid sized for R; rows past n_valid have nothing to do)
  xt_split_range<MODE>(A, nv, split, s_begin, s_end);
  constexpr bool OWN_ROWS = MODE != XT_DT;
  cx_stage(A, own, own0, OWN_ROWS ? nv : A.n, OWN_ROWS, kpad, tid);

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
  float run_m = -INFINITY, run_s = 0.f;  // FWD
  f32x4 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += XT_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    cx_stage(A, str, s0, s_end, !OWN_ROWS, kpad, tid);
    if constexpr (MODE == XT_DT) {
      if (tid < XT_TILE) {
        const int v = s0 + tid;
        const int r = v < s_end ? A.ridx[v] : 0;
        s_lse[tid] = v < s_end ? A.lse[r] : 0.f;
        s_pos[tid] = v < s_end ? A.pos[r] : -1;
      }
    }
    __syncthreads();
    f32x4 z[4];
    xt_logits<NCB>(A, own_row, str, r16, q, z);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sl = 16 * n + 4 * q + j, si = s0 + sl;
        if constexpr (MODE == XT_FWD) {
          // items s0 + 16n + 4q + j of own row r16: id 0 and ids past the split are not classes (-inf)
          if (!(si >= 1 && si < s_end)) z[n][j] = -INFINITY;
        } else {
          // G[own r16][stream 16n + 4q + j] = softmax - onehot (0 outside the valid rows / classes)
          float g = 0.f;
          if constexpr (MODE == XT_DP) {
            if (o_idx < nv && si >= 1 && si < s_end) g = __expf(z[n][j] - o_lse) - (si == o_pos ? 1.f : 0.f);
          } else {
            if (si < s_end && o_idx >= 1 && o_idx < A.n)
              g = __expf(z[n][j] - s_lse[sl]) - (s_pos[sl] == o_idx ? 1.f : 0.f);
          }
          z[n][j] = g;
        }
      }
    if constexpr (MODE == XT_FWD) xt_running_update(z, run_m, run_s);
    else xt_accumulate<NCB>(A, z, str, r16, q, acc);
  }

  if constexpr (MODE == XT_FWD) xt_store_partial(A, run_m, run_s, split, o_idx, q, nv);
  else xt_epilogue<MODE, NCB>(A, acc, nv, own0, split, w, lane);
}

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
  return xt_forward(C, XT_KERNELS(cx_tile_kernel, XT_FWD), stream,
                    [&](const int32_t* rpos, const float* part_m, const float* part_s) {
                      hipLaunchKernelGGL(cx_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D, rpos, part_m,
                                         part_s);
                    });
}

extern "C" int carca_catalogue_xent_bwd(const CarcaCatalogueXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "catalogue_xent_bwd: null descriptor");
  XentCall C = cx_call(*desc);
  return xt_backward(C, XT_KERNELS(cx_tile_kernel, XT_DP), XT_KERNELS(cx_tile_kernel, XT_DT), stream,
                     [](const int32_t*, const int32_t*, float*, int) {});
}
