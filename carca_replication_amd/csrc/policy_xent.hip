// Row log-softmax with a temperature and a per-row exclusion list, forward and backward (include/carca_hip.h:
// carca_policy_xent_fwd / _bwd): the differentiable log-probability of a served policy.
//
//   z[r, i] = P[r] . T[i] / tau;  class i of row r is eligible iff 1 <= i < n_items and i is not in excl[r];
//   row r is valid iff items[r] is an eligible class of r;
//   log_prob[r] = z[r, items[r]] - logsumexp over the eligible i of z[r, i],  entropy[r] = -sum p log p  (0 when not valid);
//   dz[r, i] = (c[r] (1[i = items[r]] - p[r, i]) - h[r] p[r, i] (log p[r, i] + H[r])) / tau on the eligible (r, i) of
//   valid rows, 0 elsewhere;  dP = dz T,  dT = dz^T P.
//
// The third client of xent_tile.h's skeleton and host path, and the second of xent_direct.h's tile kernel.  What is its
// own, in PolicyRule:
//   the mask: the 64 stream entries of a step are consecutive (FWD / DP: item ids; DT: valid-row indices), so what is
//     excluded for a lane's own entry in one step is one 64-bit word.  The lists arrive sorted (FWD / DP: each row's ids;
//     DT: per item, the valid-row indices that exclude it, in CSR form), a lane starts a cursor at the lower bound of its
//     workgroup's split and walks it forward once, so a step costs the list entries that fall into it and nothing more;
//   the row coefficients: c, h, H and lse are read with the own entry (DP) or staged with the stream rows (DT); there is
//     no n_valid and no scalar grad, so the epilogue and the split reduce are the unscaled instantiations;
//   the entropy (only when asked for): a third running value w = sum e^(z - m) (m - z) beside (m, s), merged like them:
//     entropy = max(log s + w / s, 0).
// and px_merge_kernel, px_check and the two entry points.
// No [R, n_items] buffer, no float atomics, every sum in one fixed order.
#include "xent_direct.h"

namespace {

// what a policy tile kernel reads beside XentTile (A.pos: items; A.lse: per original row; A.grad: unused)
struct PolicyTile {
  float inv_tau;
  const int32_t* excl;    // [R][E] by original row, ascending; null: no list
  int E;
  const int32_t* t_off;   // DT: [n_items + 1] offsets into t_rows; null: no list
  const int32_t* t_rows;  // DT: per item, ascending valid-row indices of the rows that exclude it
  const float* c;         // backward: dL/dlog_prob per original row
  const float* h;         // backward, entropy: dL/dentropy per original row
  const float* ent;       // backward, entropy: H per original row
  float* part_w;          // forward, entropy: [splits][R]
};

// xt_running_update with the entropy's third value: w = sum e^(z - m) (m - z) over the logits seen
__device__ __forceinline__ void px_running_update(const f32x4 (&z)[4], float& run_m, float& run_s, float& run_w) {
  float cm = -INFINITY;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int j = 0; j < 4; ++j) cm = fmaxf(cm, z[n][j]);
  if (cm > -INFINITY) {
    const float mn = fmaxf(run_m, cm);
    float s = 0.f, w = 0.f;
    if (run_m > -INFINITY) {
      const float sc = __expf(run_m - mn);
      w = sc * (run_w + (mn - run_m) * run_s);
      s = run_s * sc;
    }
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (z[n][j] > -INFINITY) {
          const float e = __expf(z[n][j] - mn);
          s += e;
          w += e * (mn - z[n][j]);
        }
    run_m = mn;
    run_s = s;
    run_w = w;
  }
}

// xt_store_partial with the third value (every term of the merge is symmetric in the two lanes: the same bits in each)
__device__ __forceinline__ void px_store_partial(const XentTile& A, const PolicyTile& X, float run_m, float run_s,
                                                 float run_w, int split, int o_idx, int q, int nv) {
#pragma unroll
  for (int x = 16; x <= 32; x *= 2) {
    const float om = __shfl_xor(run_m, x), os = __shfl_xor(run_s, x), ow = __shfl_xor(run_w, x);
    const float mn = fmaxf(run_m, om);
    float a = 0.f, aw = 0.f, b = 0.f, bw = 0.f;
    if (run_m > -INFINITY) {
      const float sc = __expf(run_m - mn);
      a = run_s * sc;
      aw = sc * (run_w + (mn - run_m) * run_s);
    }
    if (om > -INFINITY) {
      const float sc = __expf(om - mn);
      b = os * sc;
      bw = sc * (ow + (mn - om) * os);
    }
    run_m = mn;
    run_s = a + b;
    run_w = aw + bw;
  }
  if (q == 0 && o_idx < nv) {
    A.part_m[(size_t)split * A.R + o_idx] = run_m;
    A.part_s[(size_t)split * A.R + o_idx] = run_s;
    X.part_w[(size_t)split * A.R + o_idx] = run_w;
  }
}

// ---- the rule for xd_tile_kernel ----------------------------------------------------------------------------------------
// ENT: the entropy is computed (FWD) or has an upstream gradient (DP / DT); LISTS_: the call has exclusion lists (without
// them the cursor, the word and its 16 tests per step are not compiled in)
template <bool ENT, bool LISTS_>
struct PolicyRule {
  using Args = PolicyTile;
  static constexpr int ROW_WORDS = 5;  // DT: lse, c / tau, h / tau, H - lse and the item of each stream row
  static constexpr bool SCALED = false, LISTS = LISTS_;

  // the own entry's coefficients (DP), its list with the cursor, and the forward's third running value
  struct Lane {
    float c = 0.f, h = 0.f, k = 0.f, w = 0.f;
    const int32_t* list = nullptr;
    int cur = 0, cur_end = 0;
  };
  template <int MODE>
  static __device__ __forceinline__ void own(const XentTile& A, const Args& X, int nv, int o_idx, int s_begin, float o_lse,
                                             Lane& x) {
    if constexpr (MODE != XT_DT) {
      if (o_idx < nv) {
        const int r = A.ridx[o_idx];
        if constexpr (MODE == XT_DP) {
          x.c = X.c[r] * X.inv_tau;
          if constexpr (ENT) {
            x.h = X.h[r] * X.inv_tau;
            x.k = X.ent[r] - o_lse;
          }
        }
        if constexpr (LISTS) {
          x.list = X.excl + (size_t)r * X.E;
          x.cur_end = X.E;
        }
      }
    } else {
      if constexpr (LISTS) {
        if (o_idx >= 1 && o_idx < A.n) {
          x.list = X.t_rows;
          x.cur = X.t_off[o_idx];
          x.cur_end = X.t_off[o_idx + 1];
        }
      }
    }
    if constexpr (LISTS) {
      if (x.cur < x.cur_end) x.cur = xt_lower_bound(x.list, x.cur, x.cur_end, s_begin);
    }
  }
  static __device__ __forceinline__ void stage_row(const XentTile& A, const Args& X, float* s_row, int v, bool in, int tid) {
    const int r = in ? A.ridx[v] : 0;
    const float lse = in ? A.lse[r] : 0.f;
    s_row[tid] = lse;
    reinterpret_cast<int*>(s_row + 4 * XT_TILE)[tid] = in ? A.pos[r] : -1;
    s_row[XT_TILE + tid] = in ? X.c[r] * X.inv_tau : 0.f;
    if constexpr (ENT) {
      s_row[2 * XT_TILE + tid] = in ? X.h[r] * X.inv_tau : 0.f;
      s_row[3 * XT_TILE + tid] = in ? X.ent[r] - lse : 0.f;
    }
  }

  // bit b set iff s0 + b is listed; the cursor moves past the entries below s0 + 64 (entries at cur are >= s0: the cursor
  // started at the lower bound of the split's first entry and the steps are consecutive)
  static __device__ __forceinline__ unsigned long long step_mask(Lane& x, int s0) {
    unsigned long long m = 0ull;
    while (x.cur < x.cur_end) {
      const int v = x.list[x.cur];
      if (v >= s0 + XT_TILE) break;
      m |= 1ull << (v - s0);
      ++x.cur;
    }
    return m;
  }

  static __device__ __forceinline__ float logit(const Args& X, float z) { return z * X.inv_tau; }

  // dz = (c (onehot - p) - h p (log p + H)) / tau with log p = z / tau - lse
  static __device__ __forceinline__ float g_own(const f32x4 (&)[4], int, int, float zt, int si, float o_lse,
                                               int o_pos, const Lane& x) {
    const float p = __expf(zt - o_lse);
    float g = x.c * ((si == o_pos ? 1.f : 0.f) - p);
    if constexpr (ENT) g -= x.h * p * (zt + x.k);
    return g;
  }
  static __device__ __forceinline__ float g_stream(const f32x4 (&)[4], int, int, float zt, const float* s_row,
                                                  int sl, int o_idx) {
    const float p = __expf(zt - s_row[sl]);
    float g = s_row[XT_TILE + sl] * ((reinterpret_cast<const int*>(s_row + 4 * XT_TILE)[sl] == o_idx ? 1.f : 0.f) - p);
    if constexpr (ENT) g -= s_row[2 * XT_TILE + sl] * p * (zt + s_row[3 * XT_TILE + sl]);
    return g;
  }

  // FWD: z / tau, -inf where masked; the running (max, sum-exp), with the entropy (max, sum-exp, w)
  static __device__ __forceinline__ void fwd_logit(f32x4 (&z)[4], int n, int j, float zt, bool ok) {
    z[n][j] = ok ? zt : -INFINITY;
  }
  static __device__ __forceinline__ void fwd_tile(const f32x4 (&z)[4], float& m, float& s, Lane& x) {
    if constexpr (ENT) px_running_update(z, m, s, x.w);
    else xt_running_update(z, m, s);
  }
  static __device__ __forceinline__ void fwd_store(const XentTile& A, const Args& X, float m, float s, const Lane& x,
                                                   int split, int o_idx, int q, int nv) {
    if constexpr (ENT) px_store_partial(A, X, m, s, x.w, split, o_idx, q, nv);
    else xt_store_partial(A, m, s, split, o_idx, q, nv);
  }
};

// ---- forward merge: the split partials of a row in split order -> lse, log_prob, entropy, valid -------------------------
__global__ __launch_bounds__(256) void px_merge_kernel(CarcaPolicyXentDesc D, const int32_t* __restrict__ rpos,
                                                       const float* __restrict__ part_m, const float* __restrict__ part_s,
                                                       const float* __restrict__ part_w) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= D.R) return;
  const int v = rpos[r];
  D.valid[r] = v >= 0;
  if (v < 0) {
    D.lse[r] = 0.f;
    D.log_prob[r] = 0.f;
    if (D.entropy) D.entropy[r] = 0.f;
    return;
  }
  float M = -INFINITY;
  for (int s = 0; s < D.splits_items; ++s) M = fmaxf(M, part_m[(size_t)s * D.R + v]);
  float sum = 0.f, ws = 0.f;
  for (int s = 0; s < D.splits_items; ++s) {
    const float m = part_m[(size_t)s * D.R + v];
    if (m > -INFINITY) {
      const float sc = expf(m - M), ps = part_s[(size_t)s * D.R + v];
      sum += ps * sc;
      if (D.entropy) ws += sc * (part_w[(size_t)s * D.R + v] + (M - m) * ps);
    }
  }
  const float ls = logf(sum);
  const float lse = M + ls;
  const float* p = D.P + (size_t)r * D.ld_p;
  const float* t = D.T + (size_t)D.items[r] * D.ld_t;
  float zp = 0.f;
  for (int k = 0; k < D.d; ++k) zp = fmaf(p[k], t[k], zp);
  D.lse[r] = lse;
  D.log_prob[r] = zp * (1.f / D.temperature) - lse;
  if (D.entropy) D.entropy[r] = fmaxf(ls + ws / sum, 0.f);
}

// ---- host side -----------------------------------------------------------------------------------------------------
template <int MODE>
XentKernelsT<PolicyTile> px_kernels(bool ent, bool lists) {
  if (ent) return lists ? xd_kernels<PolicyRule<true, true>, MODE>() : xd_kernels<PolicyRule<true, false>, MODE>();
  return lists ? xd_kernels<PolicyRule<false, true>, MODE>() : xd_kernels<PolicyRule<false, false>, MODE>();
}

XentCall px_call(const CarcaPolicyXentDesc& D) {
  XentCall C = {};
  XentTile& A = C.A;
  A.R = D.R, A.n = D.n_items, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_t;
  A.P = D.P, A.T = D.T, A.pos = D.items;
  A.lse = D.lse;
  A.per_split = D.items_per_split;
  C.op = "policy_xent", C.classes = "items";
  C.scratch = D.scratch, C.scratch_floats = D.scratch_floats;
  C.splits_n = D.splits_items, C.splits_rows = D.splits_rows;
  C.dP = D.dP, C.dT = D.dT;
  C.excl = D.n_excl ? D.excl : nullptr, C.n_excl = D.n_excl;
  return C;
}

PolicyTile px_tile(const CarcaPolicyXentDesc& D) {
  PolicyTile X = {};
  X.inv_tau = 1.f / D.temperature;
  X.excl = D.n_excl ? D.excl : nullptr, X.E = D.n_excl;
  return X;
}

int px_check(const CarcaPolicyXentDesc& D, const char* pass) {
  CARCA_CHECK_ARG(D.temperature > 0.f && __builtin_isfinite(D.temperature) && __builtin_isfinite(1.f / D.temperature),
                  "policy_xent_%s: the temperature must be a finite number > 0", pass);
  CARCA_CHECK_ARG(D.n_excl >= 0 && (D.n_excl == 0 || D.excl), "policy_xent_%s: n_excl = %d with a null list", pass, D.n_excl);
  CARCA_CHECK_SUPPORTED((int64_t)D.R * D.n_excl < (1ll << 31), "policy_xent_%s: R n_excl must stay below 2^31", pass);
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_policy_xent_fwd(const CarcaPolicyXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "policy_xent_fwd: null descriptor");
  const CarcaPolicyXentDesc& D = *desc;
  int rc = px_check(D, "fwd");
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_ARG(D.items && D.log_prob && D.valid, "policy_xent_fwd: null items, log_prob or valid");
  XentCall C = px_call(D);
  C.fwd_parts = D.entropy ? 3 : 2;
  if ((rc = xt_check<false>(C, "fwd", false)) != CARCA_OK) return rc;  // (before the third partial is addressed)
  PolicyTile X = px_tile(D);
  X.part_w = C.scratch + xt_layout(C, false).part3;
  return xt_forward<false>(
      C, px_kernels<XT_FWD>(D.entropy != nullptr, X.excl != nullptr), stream,
      [&](const int32_t* rpos, const float* part_m, const float* part_s) {
        hipLaunchKernelGGL(px_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D, rpos, part_m, part_s,
                           X.part_w);
      },
      X);
}

extern "C" int carca_policy_xent_bwd(const CarcaPolicyXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "policy_xent_bwd: null descriptor");
  const CarcaPolicyXentDesc& D = *desc;
  int rc = px_check(D, "bwd");
  if (rc != CARCA_OK) return rc;
  CARCA_CHECK_ARG(D.items && D.c, "policy_xent_bwd: null items or c");
  CARCA_CHECK_ARG(!D.h || D.entropy, "policy_xent_bwd: h without the forward's entropy");
  CARCA_CHECK_ARG(D.n_excl == 0 || (D.t_off && D.t_rows), "policy_xent_bwd: an exclusion list without its transposed lists");
  const bool ent = D.h != nullptr;
  XentCall C = px_call(D);
  PolicyTile X = px_tile(D);
  X.t_off = D.n_excl ? D.t_off : nullptr, X.t_rows = D.t_rows;
  X.c = D.c, X.h = D.h, X.ent = D.entropy;
  return xt_backward<false>(C, px_kernels<XT_DP>(ent, X.excl != nullptr), px_kernels<XT_DT>(ent, X.t_off != nullptr), stream,
                            [](const int32_t*, const int32_t*, float*, int) {}, X);
}
