// Sampled softmax cross-entropy with the logQ correction for the dot decoders (include/carca_hip.h:
// carca_sampled_xent_fwd / _bwd).
//
//   z'(r, k) = P[r] . S[k] + bs[k],   z'(r, +) = P[r] . Tp[r] + bp[r]      (bs, bp = -log(K Q(id)): the logQ correction)
//   CE = sum over valid rows r of ( logsumexp( {z'(r, +)} U {z'(r, k) : k in N_r} ) - z'(r, +) ) / n_valid
//   N_r = { k : s_ids[k] in [1, n_items) and s_ids[k] != pos[r] }   (accidental hits and invalid ids removed)
//
// with no [R, K] buffer.  The structure is catalogue_xent.hip's, with the K samples in place of the catalogue:
//   1. compact (cx_compact_kernel, xent_tile.h): the valid rows (pos in [1, n_items)) in row order;
//   2. tile: a workgroup owns 64 rows of one operand (staged once in LDS) and streams 64-row tiles of the other.  Each
//      of its four waves computes the 64 x 16 logit tile Z^T = S O^T on v_mfma_f32_16x16x4_f32 (exact fp32 products);
//      its D layout is the A operand of the second product, so G never leaves the registers.  The next stream tile's
//      loads are issued before the current one's products and read back only when it is written to LDS after the next
//      barrier (masked there); DS, whose stream rows are gathered through ridx, loads those indices one tile ahead:
//        FWD  own = valid rows, stream = the samples of one split: running (max, sum-exp) per (split, row);
//        DP   own = valid rows, stream = samples: partial dP[split][v] = sum over the split's samples of G S;
//        DS   (xent_tile.h: XT_DT) own = samples, stream = the valid rows of one split: dS[k] (or its partial) = sum over rows of G^T P;
//      G = exp(z' - lse), 0 where masked (accidental hits, invalid ids, padding);
//   3. FWD: the split partials merged in split order, then the positive term; lse, row loss; the fp64 mean
//      (cx_mean_kernel).  BWD: the positive term (p_pos - 1) Tp[r] is written as one more dP partial after the splits,
//      and dTp[r] = grad / n_valid (p_pos - 1) P[r]; cx_reduce_kernel sums the partials in split order.
// No float atomics: every sum has one fixed order, so two calls give the same bits.
// The tile skeleton (split range, both MFMA products, the running (max, sum-exp), the lane merge, the epilogue, the
// launch sequences) is xent_tile.h's, shared with catalogue_xent.hip; the staging (the next stream tile in registers) is
// xent_stage.h's, shared with sampled_bce.hip; this file keeps its mask / G rule and its two merge kernels.
#include "xent_stage.h"

namespace {

// ---- 2. logit tiles ------------------------------------------------------------------------------------------------
// (the staging of a 64-row tile through registers -- sx_issue, sx_rows, sx_store -- is xent_stage.h's, shared with
// sampled_bce.hip)
// the per-entry values of a stream tile (threads 0..63), masked when stored: FWD / DP: bs and id of the samples; DS: lse
// and pos of the valid rows, read through mrow = ridx[entry] (loaded one tile ahead)
template <int MODE>
__device__ __forceinline__ void sx_meta(const XentTile& A, int s0, int s_end, int mrow, int tid, float& f, int& id) {
  if (tid < XT_TILE) {
    if constexpr (MODE == XT_DT) {
      f = A.lse[mrow];
      id = A.pos[mrow];
    } else {
      const int e = min(s0 + tid, s_end - 1);
      f = A.bias[e];
      id = A.ids[e];
    }
  }
}

// NCB: 16-column blocks the kernel is built for (d <= 16 NCB)
template <int MODE, int NCB>
__global__ __launch_bounds__(XT_THREADS) void sx_tile_kernel(XentTile A) {
  extern __shared__ float sx_lds[];
  float* own = sx_lds;
  float* str = sx_lds + XT_TILE * A.pitch;
  float* s_f = str + XT_TILE * A.pitch;                // FWD / DP: bs of the stream samples; DS: lse of the stream rows
  int* s_id = reinterpret_cast<int*>(s_f + XT_TILE);   // FWD / DP: ids of the stream samples; DS: pos of the stream rows
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16), nc4 = kpad / 4;
  const int own0 = blockIdx.x * XT_TILE, split = blockIdx.y;
  int s_begin, s_end;
  if (MODE != XT_DT && own0 >= nv) return;  // (grid sized for R; rows past n_valid have nothing to do)
  xt_split_range<MODE>(A, nv, split, s_begin, s_end);
  constexpr bool OWN_ROWS = MODE != XT_DT;
  const int d4 = (A.d + 3) / 4 * 4;
  const float* sbase = OWN_ROWS ? A.T : A.P;  // the streamed operand
  const int sld = OWN_ROWS ? A.ld_t : A.ld_p;
  f32x4 pre[NCB];  // the stream tile in flight
  int src[NCB];    // its pieces' operand rows
  {
    const int own_end = OWN_ROWS ? nv : A.n;
    sx_rows<NCB>(A, src, own0, own_end, OWN_ROWS, nc4, tid);
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);  // (the row indices, once: then the pieces' loads go out back to back)
    sx_issue<NCB>(OWN_ROWS ? A.P : A.T, OWN_ROWS ? A.ld_p : A.ld_t, src, pre, nc4, d4, tid);
    sx_store<NCB>(A, pre, own, own0, own_end, nc4, tid);
  }
  float pre_f = 0.f;
  int pre_id = 0, mrow = 0;
  if (s_begin < s_end) {
    sx_rows<NCB>(A, src, s_begin, s_end, !OWN_ROWS, nc4, tid);
    if constexpr (MODE == XT_DT) mrow = tid < XT_TILE ? A.ridx[min(s_begin + tid, s_end - 1)] : 0;
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);
    sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
    sx_meta<MODE>(A, s_begin, s_end, mrow, tid, pre_f, pre_id);
    if constexpr (MODE == XT_DT) {  // the row indices one tile ahead
      if (s_begin + XT_TILE < s_end) {
        sx_rows<NCB>(A, src, s_begin + XT_TILE, s_end, true, nc4, tid);
        mrow = tid < XT_TILE ? A.ridx[min(s_begin + XT_TILE + tid, s_end - 1)] : 0;
      }
    }
  }

  // this lane's own entry (column r16 of the wave's Z^T tiles)
  const int o_idx = own0 + 16 * w + r16;
  float o_f = 0.f;  // DP: lse of the own row; DS: bs of the own sample
  int o_id = -1;    // FWD / DP: pos of the own row; DS: id of the own sample
  bool o_ok = false;
  if constexpr (MODE != XT_DT) {
    if (o_idx < nv) {
      const int r = A.ridx[o_idx];
      o_id = A.pos[r];
      if constexpr (MODE == XT_DP) o_f = A.lse[r];
      o_ok = true;
    }
  } else {
    if (o_idx < A.n) {
      o_id = A.ids[o_idx];
      o_f = A.bias[o_idx];
      o_ok = o_id >= 1 && o_id < A.n_items;
    }
  }
  float run_m = -INFINITY, run_s = 0.f;  // FWD
  f32x4 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += XT_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    // Every load in flight lands here, on every path: without this wait the compiler, which sees the pieces' loads and
    // stores under branches, assumes some may still be pending and waits for them again between the next tile's loads.
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);
    sx_store<NCB>(A, pre, str, s0, s_end, nc4, tid);
    if (tid < XT_TILE) {
      const bool live = s0 + tid < s_end;
      s_f[tid] = live ? pre_f : 0.f;
      s_id[tid] = live ? pre_id : (MODE == XT_DT ? -1 : 0);  // (id 0: never a class)
    }
    __syncthreads();
    if (s0 + XT_TILE < s_end) {  // the next tile's loads: in flight while this tile multiplies
      if constexpr (MODE != XT_DT) sx_rows<NCB>(A, src, s0 + XT_TILE, s_end, false, nc4, tid);
      sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
      sx_meta<MODE>(A, s0 + XT_TILE, s_end, mrow, tid, pre_f, pre_id);
      if constexpr (MODE == XT_DT) {  // the row indices of the tile after it
        if (s0 + 2 * XT_TILE < s_end) {
          sx_rows<NCB>(A, src, s0 + 2 * XT_TILE, s_end, true, nc4, tid);
          mrow = tid < XT_TILE ? A.ridx[min(s0 + 2 * XT_TILE + tid, s_end - 1)] : 0;
        }
      }
    }
    f32x4 z[4];
    xt_logits<NCB>(A, own_row, str, r16, q, z);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sl = 16 * n + 4 * q + j;
        if constexpr (MODE == XT_FWD) {
          // the corrected logits of own row r16 against samples s0 + 16n + 4q + j; -inf where masked
          const int sid = s_id[sl];
          const bool ok = sid >= 1 && sid < A.n_items && sid != o_id;
          z[n][j] = ok ? z[n][j] + s_f[sl] : -INFINITY;
        } else {
          // G[own r16][stream 16n + 4q + j] = exp(z' - lse), 0 where masked
          float g = 0.f;
          if constexpr (MODE == XT_DP) {
            const int sid = s_id[sl];
            if (o_ok && sid >= 1 && sid < A.n_items && sid != o_id) g = __expf(z[n][j] + s_f[sl] - o_f);
          } else {
            if (o_ok && s0 + sl < s_end && s_id[sl] != o_id) g = __expf(z[n][j] + o_f - s_f[sl]);
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

// ---- 3. merges -----------------------------------------------------------------------------------------------------
// per row: the split partials in split order, then the positive term z'(r, +) = P[r] . Tp[r] + bp[r]
__global__ __launch_bounds__(256) void sx_merge_kernel(CarcaSampledXentDesc D, const int32_t* __restrict__ rpos,
                                                       const float* __restrict__ part_m, const float* __restrict__ part_s) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= D.R) return;
  const int v = rpos[r];
  if (v < 0) {
    D.lse[r] = 0.f;
    D.row_loss[r] = 0.f;
    return;
  }
  const float* p = D.P + (size_t)r * D.ld_p;
  const float* t = D.Tp + (size_t)r * D.ld_tp;
  float zp = 0.f;
  for (int k = 0; k < D.d; ++k) zp = fmaf(p[k], t[k], zp);
  zp += D.bp[r];
  float M = -INFINITY;
  for (int s = 0; s < D.splits_samples; ++s) M = fmaxf(M, part_m[(size_t)s * D.R + v]);
  M = fmaxf(M, zp);
  float sum = 0.f;
  for (int s = 0; s < D.splits_samples; ++s) {
    const float m = part_m[(size_t)s * D.R + v];
    if (m > -INFINITY) sum += part_s[(size_t)s * D.R + v] * expf(m - M);
  }
  sum += expf(zp - M);
  const float lse = M + logf(sum);
  D.lse[r] = lse;
  D.row_loss[r] = lse - zp;
}

// the positive term of the backward, p_pos = exp(z'(r, +) - lse) = exp(-row_loss):
//   part[v][col] = (p_pos - 1) Tp[r][col]          (col < ldo: dP's last partial, unscaled, by valid-row index)
//   dTp[r][col]  = grad / n_valid (p_pos - 1) P[r][col]    (0 for padding rows and past d)
__global__ __launch_bounds__(256) void sx_positive_kernel(CarcaSampledXentDesc D, const int32_t* __restrict__ rpos,
                                                          const int32_t* __restrict__ nv, float* __restrict__ part, int ldo) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)D.R * D.ld_tp) return;
  const int r = (int)(idx / D.ld_tp), col = (int)(idx - (int64_t)r * D.ld_tp);
  const int v = rpos[r];
  float dt = 0.f;
  if (v >= 0) {
    const float gp = expf(-D.row_loss[r]) - 1.f;
    if (col < ldo) part[(size_t)v * ldo + col] = col < D.d ? gp * D.Tp[(size_t)r * D.ld_tp + col] : 0.f;
    if (col < D.d) {
      const int n = nv[0];
      dt = gp * D.P[(size_t)r * D.ld_p + col] * (n > 0 ? D.grad[0] / (float)n : 0.f);
    }
  }
  D.dTp[(size_t)r * D.ld_tp + col] = dt;
}

// ---- host side -----------------------------------------------------------------------------------------------------
// the descriptor under xent_tile.h's names, after the checks of what only this loss has (the positives, the corrections)
int sx_call(const CarcaSampledXentDesc& D, const char* what, XentCall& C) {
  CARCA_CHECK_ARG(D.Tp && D.bp && D.s_ids && D.bs && D.row_loss, "%s: null Tp, bp, s_ids, bs or row_loss", what);
  CARCA_CHECK_ARG(D.ld_tp >= D.d && D.ld_tp % 4 == 0, "%s: ld_tp must be a multiple of 4, at least d", what);
  CARCA_CHECK_SUPPORTED((int64_t)D.R * D.ld_tp < (1ll << 40), "%s: operands too large", what);
  C = {};
  XentTile& A = C.A;
  A.R = D.R, A.n = D.K, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_s;
  A.P = D.P, A.T = D.S, A.pos = D.pos, A.ids = D.s_ids, A.bias = D.bs;
  A.lse = D.lse, A.grad = D.grad;
  A.per_split = D.samples_per_split;
  C.op = "sampled_xent", C.classes = "samples";
  C.scratch = D.scratch, C.scratch_floats = D.scratch_floats;
  C.splits_n = D.splits_samples, C.splits_rows = D.splits_rows, C.extra_dp = 1;  // (the positive term)
  C.row_loss = D.row_loss, C.loss = D.loss, C.dP = D.dP, C.dT = D.dS;
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_sampled_xent_fwd(const CarcaSampledXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "sampled_xent_fwd: null descriptor");
  const CarcaSampledXentDesc& D = *desc;
  XentCall C;
  const int rc = sx_call(D, "sampled_xent_fwd", C);
  if (rc != CARCA_OK) return rc;
  return xt_forward(C, XT_KERNELS(sx_tile_kernel, XT_FWD), stream,
                    [&](const int32_t* rpos, const float* part_m, const float* part_s) {
                      hipLaunchKernelGGL(sx_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D, rpos, part_m,
                                         part_s);
                    });
}

extern "C" int carca_sampled_xent_bwd(const CarcaSampledXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "sampled_xent_bwd: null descriptor");
  const CarcaSampledXentDesc& D = *desc;
  XentCall C;
  const int rc = sx_call(D, "sampled_xent_bwd", C);
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_ARG(D.dTp, "sampled_xent_bwd: null dTp");
  // the positive term: dP's last partial, after the sample splits'; dTp
  return xt_backward(C, XT_KERNELS(sx_tile_kernel, XT_DP), XT_KERNELS(sx_tile_kernel, XT_DT), stream,
                     [&](const int32_t* rpos, const int32_t* nv, float* part, int ldo) {
                       const int64_t ntp = (int64_t)D.R * D.ld_tp;
                       hipLaunchKernelGGL(sx_positive_kernel, dim3((unsigned)((ntp + 255) / 256)), dim3(256), 0, stream, D,
                                          rpos, nv, part, ldo);
                     });
}
