// Binary cross-entropy against K shared negatives (gBCE) for the dot decoders (include/carca_hip.h:
// carca_sampled_bce_fwd / _bwd).
//
//   z(r, +) = P[r] . Tp[r]                          (Tp: the positive's row, its context included)
//   z(r, k) = P[r] . S[k] + br[r],  br[r] = P[r] . C[r]   (C[r] = M c_r: the row's context share; 0 without C)
//   loss = sum over valid rows r of ( beta sp(-z(r, +)) + sum_{k in N_r} sp(z(r, k)) ) / n_valid,  sp = softplus
//   N_r = { k : s_ids[k] in [1, n_items) and s_ids[k] != pos[r] }   (accidental hits and invalid ids removed)
//
// with no [R, K] buffer.  The structure is sampled_xent.hip's, with a sigmoid in place of the softmax:
//   1. compact (cx_compact_kernel, xent_tile.h): the valid rows (pos in [1, n_items)) in row order;
//   2. row pre-pass (forward): zpos[r] = z(r, +) and br[r] per original row, both kept for the backward;
//   3. tile: xent_stage.h's xs_tile_kernel (the next stream tile in registers, the mask tests, xent_tile.h's products and
//      epilogue), the kernel sampled_xent.hip runs, under this file's rule (SbRule).  br travels where the softmax
//      backward carries lse (XentTile::lse): the own row's value in FWD and DP, the stream rows' metadata in DS:
//        FWD  own = valid rows, stream = the samples of one split: (sum sp(z), sum sigmoid(z)) per (split, row);
//        DP   own = valid rows, stream = samples: partial dP[split][v] = sum over the split's samples of G S;
//        DS   (xent_tile.h: XT_DT) own = samples, stream = the valid rows of one split: dS[k] (or its partial) = G^T P;
//      G = sigmoid(z), 0 where masked (accidental hits, invalid ids, padding);
//   4. FWD: the split partials summed in split order, then beta sp(-zpos): row_loss, gsum[r] = G_r = sum_k G (kept for
//      the backward); the fp64 mean (cx_mean_kernel).  BWD: with gp = -beta sigmoid(-zpos), gp Tp[r] + G_r C[r] is
//      written as one more dP partial after the splits; dTp[r] = grad / n_valid gp P[r], dC[r] = grad / n_valid G_r P[r];
//      cx_reduce_kernel sums the partials in split order.
// No float atomics: every sum has one fixed order, so two calls give the same bits.
#include "xent_stage.h"

namespace {

// softplus(x) and sigmoid(x) from one exp of -|x| (never overflows): sp = max(x, 0) + log(1 + e), sigmoid = 1 / (1 + e)
// for x >= 0 and e / (1 + e) below.  Where 1 + e would round e away, log(1 + e) is its series e - e^2 / 2.
__device__ __forceinline__ float sb_sigmoid(float x) {
  const float e = __expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  return x >= 0.f ? r : e * r;
}
__device__ __forceinline__ void sb_softplus_sigmoid(float x, float& sp, float& sg) {
  const float e = __expf(-fabsf(x));
  const float r = __builtin_amdgcn_rcpf(1.f + e);
  sg = x >= 0.f ? r : e * r;
  const float l = e < 0x1p-12f ? e - 0.5f * e * e : __logf(1.f + e);
  sp = fmaxf(x, 0.f) + l;
}

// ---- 2. row pre-pass -------------------------------------------------------------------------------------------------
// zpos[r] = P[r] . Tp[r], br[r] = P[r] . C[r] (0 without C; both 0 for a row that is not valid): eight lanes per row, lane l
// columns l, l + 8, ..., merged with xor shuffles (one fixed order)
__global__ __launch_bounds__(256) void sb_rows_kernel(CarcaSampledBceDesc D) {
  const int r = blockIdx.x * 32 + (threadIdx.x >> 3), l = threadIdx.x & 7;
  float zp = 0.f, b = 0.f;
  if (r < D.R) {
    const int id = D.pos[r];
    if (id >= 1 && id < D.n_items) {
      const float* p = D.P + (size_t)r * D.ld_p;
      const float* t = D.Tp + (size_t)r * D.ld_tp;
      for (int k = l; k < D.d; k += 8) zp = fmaf(p[k], t[k], zp);
      if (D.C) {
        const float* c = D.C + (size_t)r * D.ld_c;
        for (int k = l; k < D.d; k += 8) b = fmaf(p[k], c[k], b);
      }
    }
  }
#pragma unroll
  for (int x = 4; x >= 1; x >>= 1) {
    zp += __shfl_xor(zp, x);
    b += __shfl_xor(b, x);
  }
  if (r < D.R && l == 0) {
    D.zpos[r] = zp;
    D.br[r] = b;
  }
}

// ---- 3. logit tiles: the sigmoid's rule for xs_tile_kernel --------------------------------------------------------------
struct SbRule {
  // (FWD / DP: the samples carry no float, and s_f is not written)
  static constexpr bool keep_f(int mode) { return mode == XT_DT; }

  // the per-entry values of a stream tile (threads 0..63), masked when stored: FWD / DP: id of the samples; DS: br and pos
  // of the valid rows, read through mrow = ridx[entry] (loaded one tile ahead)
  template <int MODE>
  static __device__ __forceinline__ void meta(const XentTile& A, int s0, int s_end, int mrow, int tid, float& f, int& id) {
    if (tid < XT_TILE) {
      if constexpr (MODE == XT_DT) {
        f = A.lse[mrow];
        id = A.pos[mrow];
      } else {
        id = A.ids[min(s0 + tid, s_end - 1)];
      }
    }
  }

  // the lane's own entry: FWD / DP: br of the own row (in the lse slot)
  template <int MODE>
  static __device__ __forceinline__ float own_f(const XentTile& A, int e) {
    if constexpr (MODE != XT_DT) return A.lse[e];
    else return 0.f;
  }

  // FWD: sum of softplus(z), sum of sigmoid(z) over the lane's unmasked logits
  struct Fwd {
    float sp = 0.f, sg = 0.f;
  };
  static __device__ __forceinline__ float fwd_logit(bool ok, float z, const float*, int, float o_f, Fwd& run) {
    if (ok) {
      float sp, sg;
      sb_softplus_sigmoid(z + o_f, sp, sg);
      run.sp += sp;
      run.sg += sg;
    }
    return z;
  }
  static __device__ __forceinline__ void fwd_tile(const f32x4 (&)[4], Fwd&) {}
  // merge the four lanes of own row r16 (lanes r16 + 16q; + is commutative, so every lane gets the same bits) and store
  // the (sum softplus, sum sigmoid) partial of (split, valid row o_idx) in the part_m / part_s slots
  static __device__ __forceinline__ void fwd_store(const XentTile& A, Fwd run, int split, int o_idx, int q, int nv) {
#pragma unroll
    for (int x = 16; x <= 32; x *= 2) {
      run.sp += __shfl_xor(run.sp, x);
      run.sg += __shfl_xor(run.sg, x);
    }
    if (q == 0 && o_idx < nv) {
      A.part_m[(size_t)split * A.R + o_idx] = run.sp;
      A.part_s[(size_t)split * A.R + o_idx] = run.sg;
    }
  }

  // G = sigmoid(z): DP: z = P[r] . S[k] + br of the own row; DS: + br of the stream row
  template <int MODE>
  static __device__ __forceinline__ float g(float z, const float* s_f, int sl, float o_f) {
    if constexpr (MODE == XT_DP) return sb_sigmoid(z + o_f);
    else return sb_sigmoid(z + s_f[sl]);
  }
};

// ---- 4. merges -----------------------------------------------------------------------------------------------------
// per row: the split partials in split order, then the positive term beta sp(-zpos)
__global__ __launch_bounds__(256) void sb_merge_kernel(CarcaSampledBceDesc D, const int32_t* __restrict__ rpos,
                                                       const float* __restrict__ part_sp, const float* __restrict__ part_sg) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= D.R) return;
  const int v = rpos[r];
  if (v < 0) {
    D.row_loss[r] = 0.f;
    D.gsum[r] = 0.f;
    return;
  }
  float sp = 0.f, sg = 0.f;
  for (int s = 0; s < D.splits_samples; ++s) {
    sp += part_sp[(size_t)s * D.R + v];
    sg += part_sg[(size_t)s * D.R + v];
  }
  const float zp = D.zpos[r];
  D.row_loss[r] = D.beta * (fmaxf(-zp, 0.f) + log1pf(expf(-fabsf(zp)))) + sp;
  D.gsum[r] = sg;
}

// the row terms of the backward, gp = -beta sigmoid(-zpos[r]) and G_r = gsum[r]:
//   part[v][col] = gp Tp[r][col] + G_r C[r][col]          (col < ldo: dP's last partial, unscaled, by valid-row index)
//   dTp[r][col]  = grad / n_valid gp P[r][col]             (col < ld_tp; 0 for padding rows and past d)
//   dC[r][col]   = grad / n_valid G_r P[r][col]            (col < ld_c; with C only)
__global__ __launch_bounds__(256) void sb_positive_kernel(CarcaSampledBceDesc D, const int32_t* __restrict__ rpos,
                                                          const int32_t* __restrict__ nv, float* __restrict__ part, int ldo,
                                                          int ldm) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)D.R * ldm) return;
  const int r = (int)(idx / ldm), col = (int)(idx - (int64_t)r * ldm);
  const int v = rpos[r];
  float dt = 0.f, dc = 0.f;
  if (v >= 0) {
    const float zp = D.zpos[r];
    const float e = expf(-fabsf(zp)), s = 1.f / (1.f + e);
    const float gp = -D.beta * (zp >= 0.f ? e * s : s);
    const float G = D.gsum[r];
    if (col < ldo) {
      float x = 0.f;
      if (col < D.d) {
        x = gp * D.Tp[(size_t)r * D.ld_tp + col];
        if (D.C) x = fmaf(G, D.C[(size_t)r * D.ld_c + col], x);
      }
      part[(size_t)v * ldo + col] = x;
    }
    if (col < D.d) {
      const int n = nv[0];
      const float p = D.P[(size_t)r * D.ld_p + col] * (n > 0 ? D.grad[0] / (float)n : 0.f);
      dt = gp * p;
      dc = G * p;
    }
  }
  if (col < D.ld_tp) D.dTp[(size_t)r * D.ld_tp + col] = dt;
  if (D.C && col < D.ld_c) D.dC[(size_t)r * D.ld_c + col] = dc;
}

// ---- host side -----------------------------------------------------------------------------------------------------
// the descriptor under xent_tile.h's names, after the checks of what only this loss has (the positives, the context rows,
// the per-row values the forward keeps for the backward)
int sb_call(const CarcaSampledBceDesc& D, const char* what, XentCall& C) {
  CARCA_CHECK_ARG(D.Tp && D.s_ids && D.zpos && D.br && D.gsum && D.row_loss, "%s: null Tp, s_ids, zpos, br, gsum or row_loss",
                  what);
  CARCA_CHECK_ARG(D.ld_tp >= D.d && D.ld_tp % 4 == 0, "%s: ld_tp must be a multiple of 4, at least d", what);
  CARCA_CHECK_ARG(!D.C || D.ld_c >= D.d, "%s: ld_c must be at least d", what);
  CARCA_CHECK_ARG(D.beta >= 0.f && D.beta <= 1.f, "%s: beta = %g outside [0, 1]", what, (double)D.beta);
  CARCA_CHECK_SUPPORTED((int64_t)D.R * D.ld_tp < (1ll << 40) && (!D.C || (int64_t)D.R * D.ld_c < (1ll << 40)),
                        "%s: operands too large", what);
  C = {};
  XentTile& A = C.A;
  A.R = D.R, A.n = D.K, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_s;
  A.P = D.P, A.T = D.S, A.pos = D.pos, A.ids = D.s_ids, A.bias = nullptr;
  A.lse = D.br, A.grad = D.grad;  // (br rides in the slot of the softmax's lse)
  A.per_split = D.samples_per_split;
  C.op = "sampled_bce", C.classes = "samples";
  C.scratch = D.scratch, C.scratch_floats = D.scratch_floats;
  C.splits_n = D.splits_samples, C.splits_rows = D.splits_rows, C.extra_dp = 1;  // (the row terms)
  C.share_partials = 1;  // (dS's partials in the words of dP's: the backward's scratch is the larger set, not both)
  C.row_loss = D.row_loss, C.loss = D.loss, C.dP = D.dP, C.dT = D.dS;
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_sampled_bce_fwd(const CarcaSampledBceDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "sampled_bce_fwd: null descriptor");
  const CarcaSampledBceDesc& D = *desc;
  XentCall C;
  int rc = sb_call(D, "sampled_bce_fwd", C);
  if (rc != CARCA_OK) return rc;
  if ((rc = xt_check(C, "fwd", false)) != CARCA_OK) return rc;  // (before the pre-pass reads the operands)
  hipLaunchKernelGGL(sb_rows_kernel, dim3((D.R + 31) / 32), dim3(256), 0, stream, D);
  CARCA_LAUNCH_CHECK();
  return xt_forward(C, XS_KERNELS(SbRule, XT_FWD), stream,
                    [&](const int32_t* rpos, const float* part_sp, const float* part_sg) {
                      hipLaunchKernelGGL(sb_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D, rpos, part_sp,
                                         part_sg);
                    });
}

extern "C" int carca_sampled_bce_bwd(const CarcaSampledBceDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "sampled_bce_bwd: null descriptor");
  const CarcaSampledBceDesc& D = *desc;
  XentCall C;
  const int rc = sb_call(D, "sampled_bce_bwd", C);
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_ARG(D.dTp && (!D.C || D.dC), "sampled_bce_bwd: null dTp, or C without dC");
  // the row terms: dP's last partial, after the sample splits'; dTp and dC
  return xt_backward(C, XS_KERNELS(SbRule, XT_DP), XS_KERNELS(SbRule, XT_DT), stream,
                     [&](const int32_t* rpos, const int32_t* nv, float* part, int ldo) {
                       const int ldm = D.C && D.ld_c > D.ld_tp ? D.ld_c : D.ld_tp;
                       const int64_t n = (int64_t)D.R * ldm;
                       hipLaunchKernelGGL(sb_positive_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, D, rpos,
                                          nv, part, ldo, ldm);
                     });
}
