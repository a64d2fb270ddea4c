// Sampled softmax cross-entropy with the logQ correction for the dot decoders (include/carca_hip.h:
// carca_sampled_xent_fwd / _bwd).
//
//   z'(r, k) = P[r] . S[k] + bs[k],   z'(r, +) = P[r] . Tp[r] + bp[r]      (bs, bp = -log(K Q(id)): the logQ correction)
//   CE = sum over valid rows r of ( logsumexp( {z'(r, +)} U {z'(r, k) : k in N_r} ) - z'(r, +) ) / n_valid
//   N_r = { k : s_ids[k] in [1, n_items) and s_ids[k] != pos[r] }   (accidental hits and invalid ids removed)
//
// with no [R, K] buffer.  The structure is catalogue_xent.hip's, with the K samples in place of the catalogue:
//   1. compact (cx_compact_kernel, xent_tile.h): the valid rows (pos in [1, n_items)) in row order;
//   2. tile (xs_tile_kernel under SxRule): a workgroup owns 64 rows of one operand (staged once in LDS) and streams 64-row tiles of the other.  Each
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
// The tile kernel is xent_stage.h's xs_tile_kernel (the staging one tile ahead in registers, the mask tests), shared with
// sampled_bce.hip, around xent_tile.h's skeleton (split range, both MFMA products, the running (max, sum-exp), the lane
// merge, the epilogue, the launch sequences), shared with catalogue_xent.hip; this file keeps its rule (SxRule: what a
// stream entry and the own entry carry, the forward's steps, G) and its two merge kernels.
#include "xent_stage.h"

namespace {

// ---- 2. logit tiles: the softmax's rule for xs_tile_kernel ---------------------------------------------------------------
struct SxRule {
  static constexpr bool keep_f(int) { return true; }

  // the per-entry values of a stream tile (threads 0..63), masked when stored: FWD / DP: bs and id of the samples; DS: lse
  // and pos of the valid rows, read through mrow = ridx[entry] (loaded one tile ahead)
  template <int MODE>
  static __device__ __forceinline__ void meta(const XentTile& A, int s0, int s_end, int mrow, int tid, float& f, int& id) {
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

  // the lane's own entry: DP: lse of the own row; DS: bs of the own sample
  template <int MODE>
  static __device__ __forceinline__ float own_f(const XentTile& A, int e) {
    if constexpr (MODE == XT_DP) return A.lse[e];
    else if constexpr (MODE == XT_DT) return A.bias[e];
    else return 0.f;
  }

  // FWD: the lane's running (max, sum-exp); a logit is corrected, or -inf where masked
  struct Fwd {
    float m = -INFINITY, s = 0.f;
  };
  static __device__ __forceinline__ float fwd_logit(bool ok, float z, const float* s_f, int sl, float, Fwd&) {
    return ok ? z + s_f[sl] : -INFINITY;
  }
  static __device__ __forceinline__ void fwd_tile(const f32x4 (&z)[4], Fwd& run) { xt_running_update(z, run.m, run.s); }
  static __device__ __forceinline__ void fwd_store(const XentTile& A, const Fwd& run, int split, int o_idx, int q, int nv) {
    xt_store_partial(A, run.m, run.s, split, o_idx, q, nv);
  }

  // G = exp(z' - lse)
  template <int MODE>
  static __device__ __forceinline__ float g(float z, const float* s_f, int sl, float o_f) {
    if constexpr (MODE == XT_DP) return __expf(z + s_f[sl] - o_f);
    else return __expf(z + o_f - s_f[sl]);
  }
};

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
  return xt_forward(C, XS_KERNELS(SxRule, XT_FWD), stream,
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
  return xt_backward(C, XS_KERNELS(SxRule, XT_DP), XS_KERNELS(SxRule, XT_DT), stream,
                     [&](const int32_t* rpos, const int32_t* nv, float* part, int ldo) {
                       const int64_t ntp = (int64_t)D.R * D.ld_tp;
                       hipLaunchKernelGGL(sx_positive_kernel, dim3((unsigned)((ntp + 255) / 256)), dim3(256), 0, stream, D,
                                          rpos, nv, part, ldo);
                     });
}
