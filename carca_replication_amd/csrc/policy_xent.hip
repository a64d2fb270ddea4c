// Row log-softmax with a temperature and a per-row exclusion list, forward and backward (include/carca_hip.h:
// carca_policy_xent_fwd / _bwd): the differentiable log-probability of a served policy.
//
//   z[r, i] = P[r] . T[i] / tau;  class i of row r is eligible iff 1 <= i < n_items and i is not in excl[r];
//   row r is valid iff items[r] is an eligible class of r;
//   log_prob[r] = z[r, items[r]] - logsumexp over the eligible i of z[r, i],  entropy[r] = -sum p log p  (0 when not valid);
//   dz[r, i] = (c[r] (1[i = items[r]] - p[r, i]) - h[r] p[r, i] (log p[r, i] + H[r])) / tau on the eligible (r, i) of
//   valid rows, 0 elsewhere;  dP = dz T,  dT = dz^T P.
//
// The third client of xent_tile.h's skeleton, with catalogue_xent.hip's staging and launch sequences.  What is its own:
//   the mask: the 64 stream entries of a step are consecutive (FWD / DP: item ids; DT: valid-row indices), so what is
//     excluded for a lane's own entry in one step is one 64-bit word.  The lists arrive sorted (FWD / DP: each row's ids;
//     DT: per item, the valid-row indices that exclude it, in CSR form), a lane starts a cursor at the lower bound of its
//     workgroup's split and walks it forward once, so a step costs the list entries that fall into it and nothing more;
//   the row coefficients: c, h, H and lse are read with the own entry (DP) or staged with the stream rows (DT); there is
//     no n_valid and no scalar grad, so the epilogue and the split reduce scale by nothing;
//   the entropy (only when asked for): a third running value w = sum e^(z - m) (m - z) beside (m, s), merged like them:
//     entropy = max(log s + w / s, 0).
// No [R, n_items] buffer, no float atomics, every sum in one fixed order.
#include "xent_tile.h"

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

// first index in [lo, hi) whose entry is >= key
__device__ __forceinline__ int px_lower_bound(const int32_t* a, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// bit b set iff s0 + b is listed; the cursor moves past the entries below s0 + 64 (entries at cur are >= s0: the cursor
// started at the lower bound of the split's first entry and the steps are consecutive)
__device__ __forceinline__ unsigned long long px_step_mask(const int32_t* a, int& cur, int end, int s0) {
  unsigned long long m = 0ull;
  while (cur < end) {
    const int v = a[cur];
    if (v >= s0 + XT_TILE) break;
    m |= 1ull << (v - s0);
    ++cur;
  }
  return m;
}

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

// xt_epilogue without a scale: the row coefficients carry all of it.  final_out (DT with one row split): out is dT
// itself, zeros up to the row stride
template <int MODE, int NCB>
__device__ __forceinline__ void px_epilogue(const XentTile& A, const f32x4 (&acc)[NCB], int nv, int own0, int split, int w,
                                            int lane) {
  const int r16 = lane & 15, q = lane >> 4, ncb = (A.d + 15) / 16;
  float* out = A.out + (size_t)split * A.out_split_stride;
  const int own_end = MODE == XT_DP ? nv : A.n;
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    if (c < ncb) {
      const int col = 16 * c + r16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = own0 + 16 * w + 4 * q + j;
        if (e < own_end && col < A.ld_out) out[(size_t)e * A.ld_out + col] = col < A.d ? acc[c][j] : 0.f;
      }
    }
  }
  if (MODE == XT_DT && A.final_out) {
    for (int col = 16 * ncb + lane; col < A.ld_out; col += 64)
      for (int j = 0; j < 16; ++j) {
        const int e = own0 + 16 * w + j;
        if (e < A.n) out[(size_t)e * A.ld_out + col] = 0.f;
      }
  }
}

// catalogue_xent.hip's staging: entries first .. end-1 are valid-row indices (P[ridx[v]]) or item ids (T[i])
__device__ __forceinline__ void px_stage(const XentTile& A, float* dst, int first, int end, bool rows, int kpad, int tid) {
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

constexpr int PX_ROW_WORDS = 5;  // DT: lse, c / tau, h / tau, H - lse and the item of each stream row

// ENT: the entropy is computed (FWD) or has an upstream gradient (DP / DT); LISTS: the call has exclusion lists (without
// them the cursor, the word and its 16 tests per step are not compiled in)
template <int MODE, int NCB, bool ENT, bool LISTS>
__global__ __launch_bounds__(XT_THREADS) void px_tile_kernel(XentTile A, PolicyTile X) {
  extern __shared__ float px_lds[];
  float* own = px_lds;
  float* str = px_lds + XT_TILE * A.pitch;
  float* s_lse = str + XT_TILE * A.pitch;  // DT: per stream row
  float* s_c = s_lse + XT_TILE;
  float* s_h = s_c + XT_TILE;
  float* s_k = s_h + XT_TILE;
  int* s_pos = reinterpret_cast<int*>(s_k + XT_TILE);
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16);
  const int own0 = blockIdx.x * XT_TILE, split = blockIdx.y;
  int s_begin, s_end;
  if (MODE != XT_DT && own0 >= nv) return;
  xt_split_range<MODE>(A, nv, split, s_begin, s_end);
  constexpr bool OWN_ROWS = MODE != XT_DT;
  px_stage(A, own, own0, OWN_ROWS ? nv : A.n, OWN_ROWS, kpad, tid);

  // this lane's own entry (column r16 of the wave's Z^T tiles), its coefficients and its list
  const int o_idx = own0 + 16 * w + r16;
  float o_lse = 0.f, o_c = 0.f, o_h = 0.f, o_k = 0.f;
  int o_pos = -1;
  const int32_t* list = nullptr;
  int cur = 0, cur_end = 0;
  if constexpr (OWN_ROWS) {
    if (o_idx < nv) {
      const int r = A.ridx[o_idx];
      if constexpr (MODE == XT_DP) {
        o_lse = A.lse[r];
        o_pos = A.pos[r];
        o_c = X.c[r] * X.inv_tau;
        if constexpr (ENT) {
          o_h = X.h[r] * X.inv_tau;
          o_k = X.ent[r] - o_lse;
        }
      }
      if constexpr (LISTS) {
        list = X.excl + (size_t)r * X.E;
        cur_end = X.E;
      }
    }
  } else {
    if constexpr (LISTS) {
      if (o_idx >= 1 && o_idx < A.n) {
        list = X.t_rows;
        cur = X.t_off[o_idx];
        cur_end = X.t_off[o_idx + 1];
      }
    }
  }
  if constexpr (LISTS) {
    if (cur < cur_end) cur = px_lower_bound(list, cur, cur_end, s_begin);
  }

  float run_m = -INFINITY, run_s = 0.f, run_w = 0.f;  // FWD
  f32x4 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += XT_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    px_stage(A, str, s0, s_end, !OWN_ROWS, kpad, tid);
    if constexpr (MODE == XT_DT) {
      if (tid < XT_TILE) {
        const int v = s0 + tid;
        const bool in = v < s_end;
        const int r = in ? A.ridx[v] : 0;
        const float lse = in ? A.lse[r] : 0.f;
        s_lse[tid] = lse;
        s_pos[tid] = in ? A.pos[r] : -1;
        s_c[tid] = in ? X.c[r] * X.inv_tau : 0.f;
        if constexpr (ENT) {
          s_h[tid] = in ? X.h[r] * X.inv_tau : 0.f;
          s_k[tid] = in ? X.ent[r] - lse : 0.f;
        }
      }
    }
    // (shifted once to the lane's first stream entry 4q: the 16 tests below then read bits at compile-time offsets)
    unsigned long long mask = 0ull;
    if constexpr (LISTS) mask = px_step_mask(list, cur, cur_end, s0) >> (4 * q);
    __syncthreads();
    f32x4 z[4];
    xt_logits<NCB>(A, own_row, str, r16, q, z);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sl = 16 * n + 4 * q + j, si = s0 + sl;
        const bool listed = LISTS && ((mask >> (16 * n + j)) & 1ull);
        const float zt = z[n][j] * X.inv_tau;
        if constexpr (MODE == XT_FWD) {
          z[n][j] = (si >= 1 && si < s_end && !listed) ? zt : -INFINITY;
        } else {
          // dz[own r16][stream 16n + 4q + j] (0 outside the valid rows and the eligible classes)
          float g = 0.f;
          if constexpr (MODE == XT_DP) {
            if (o_idx < nv && si >= 1 && si < s_end && !listed) {
              const float p = __expf(zt - o_lse);
              g = o_c * ((si == o_pos ? 1.f : 0.f) - p);
              if constexpr (ENT) g -= o_h * p * (zt + o_k);
            }
          } else {
            if (si < s_end && o_idx >= 1 && o_idx < A.n && !listed) {
              const float p = __expf(zt - s_lse[sl]);
              g = s_c[sl] * ((s_pos[sl] == o_idx ? 1.f : 0.f) - p);
              if constexpr (ENT) g -= s_h[sl] * p * (zt + s_k[sl]);
            }
          }
          z[n][j] = g;
        }
      }
    if constexpr (MODE == XT_FWD) {
      if constexpr (ENT) px_running_update(z, run_m, run_s, run_w);
      else xt_running_update(z, run_m, run_s);
    } else {
      xt_accumulate<NCB>(A, z, str, r16, q, acc);
    }
  }

  if constexpr (MODE == XT_FWD) {
    if constexpr (ENT) px_store_partial(A, X, run_m, run_s, run_w, split, o_idx, q, nv);
    else xt_store_partial(A, run_m, run_s, split, o_idx, q, nv);
  } else {
    px_epilogue<MODE, NCB>(A, acc, nv, own0, split, w, lane);
  }
}

// ---- the valid rows, in row order: cx_compact_kernel with the row's own list consulted ----------------------------------
__global__ __launch_bounds__(CX_COMPACT_THREADS) void px_compact_kernel(const int32_t* __restrict__ pos,
                                                                         const int32_t* __restrict__ excl, int E, int R,
                                                                         int n_items, int32_t* __restrict__ ridx,
                                                                         int32_t* __restrict__ rpos, int32_t* __restrict__ nv) {
  __shared__ int wsum[CX_COMPACT_THREADS / 64];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < R; r0 += CX_COMPACT_THREADS) {
    const int r = r0 + tid;
    const int p = r < R ? pos[r] : 0;
    bool ok = r < R && p >= 1 && p < n_items;
    if (ok && excl) {
      const int32_t* l = excl + (size_t)r * E;
      const int at = px_lower_bound(l, 0, E, p);
      ok = !(at < E && l[at] == p);
    }
    const unsigned long long m = __ballot(ok);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int off = base_s;
    for (int j = 0; j < w; ++j) off += wsum[j];
    if (r < R) {
      const int v = off + before;
      rpos[r] = ok ? v : -1;
      if (ok) ridx[v] = r;
    }
    __syncthreads();
    if (tid == CX_COMPACT_THREADS - 1) {
      int tot = 0;
      for (int j = 0; j < CX_COMPACT_THREADS / 64; ++j) tot += wsum[j];
      base_s += tot;
    }
    __syncthreads();
  }
  if (tid == 0) nv[0] = base_s;
}

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

// dst[e][col] (col < ld_dst) = sum over splits of part[s][map(e)][col] for col < d, else 0: cx_reduce_kernel unscaled
__global__ __launch_bounds__(256) void px_reduce_kernel(const float* __restrict__ part, int64_t split_stride, int splits,
                                                        int ld_part, const int32_t* __restrict__ rpos, int rows, int d,
                                                        float* __restrict__ dst, int ld_dst) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * ld_dst) return;
  const int e = (int)(idx / ld_dst), col = (int)(idx - (int64_t)e * ld_dst);
  const int src = rpos ? rpos[e] : e;
  float v = 0.f;
  if (src >= 0 && col < d)
    for (int s = 0; s < splits; ++s) v += part[(size_t)s * split_stride + (size_t)src * ld_part + col];
  dst[(size_t)e * ld_dst + col] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------
using PolicyKernel = void (*)(XentTile, PolicyTile);
struct PolicyKernels {
  PolicyKernel k4, k8, k16;
};
#define PX_KERNELS(MODE, ENT, LISTS) \
  (PolicyKernels{px_tile_kernel<MODE, 4, ENT, LISTS>, px_tile_kernel<MODE, 8, ENT, LISTS>, px_tile_kernel<MODE, 16, ENT, LISTS>})
template <int MODE>
PolicyKernels px_kernels(bool ent, bool lists) {
  if (ent) return lists ? PX_KERNELS(MODE, true, true) : PX_KERNELS(MODE, true, false);
  return lists ? PX_KERNELS(MODE, false, true) : PX_KERNELS(MODE, false, false);
}

int px_launch_tile(const PolicyKernels& K, const XentTile& A, const PolicyTile& X, int own_entries, hipStream_t stream) {
  const size_t lds = (size_t)2 * XT_TILE * A.pitch * sizeof(float) + XT_TILE * PX_ROW_WORDS * sizeof(float);
  const PolicyKernel kern = A.d <= 64 ? K.k4 : A.d <= 128 ? K.k8 : K.k16;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    carca_set_error("policy_xent: cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3((own_entries + XT_TILE - 1) / XT_TILE, A.splits), dim3(XT_THREADS), lds, stream, A, X);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// (xt_check wants a row_loss / loss pair in the forward and a grad in the backward: log_prob and c stand in)
XentCall px_call(const CarcaPolicyXentDesc& D) {
  XentCall C = {};
  XentTile& A = C.A;
  A.R = D.R, A.n = D.n_items, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_t;
  A.P = D.P, A.T = D.T, A.pos = D.items;
  A.lse = D.lse, A.grad = D.c;
  A.per_split = D.items_per_split;
  C.op = "policy_xent", C.classes = "items";
  C.scratch = D.scratch, C.scratch_floats = D.scratch_floats;
  C.splits_n = D.splits_items, C.splits_rows = D.splits_rows;
  C.row_loss = D.log_prob, C.loss = D.log_prob, C.dP = D.dP, C.dT = D.dT;
  return C;
}

int px_check(const CarcaPolicyXentDesc& D, const char* pass) {
  CARCA_CHECK_ARG(D.temperature > 0.f && __builtin_isfinite(D.temperature) && __builtin_isfinite(1.f / D.temperature),
                  "policy_xent_%s: the temperature must be a finite number > 0", pass);
  CARCA_CHECK_ARG(D.n_excl >= 0 && (D.n_excl == 0 || D.excl), "policy_xent_%s: n_excl = %d with a null list", pass, D.n_excl);
  CARCA_CHECK_SUPPORTED((int64_t)D.R * D.n_excl < (1ll << 31), "policy_xent_%s: R n_excl must stay below 2^31", pass);
  return CARCA_OK;
}

// xt_begin with px_compact_kernel
int px_begin(XentCall& C, const CarcaPolicyXentDesc& D, const XentLayout& L, hipStream_t stream) {
  int32_t* base = reinterpret_cast<int32_t*>(C.scratch);
  C.A.ridx = base + L.ridx, C.A.nv = base + L.nv;
  C.A.pitch = round_up(C.A.d, 16) + 4;
  hipLaunchKernelGGL(px_compact_kernel, dim3(1), dim3(CX_COMPACT_THREADS), 0, stream, D.items, D.n_excl ? D.excl : nullptr,
                     D.n_excl, D.R, D.n_items, base + L.ridx, base + L.rpos, base + L.nv);
  CARCA_LAUNCH_CHECK();
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
  if ((rc = xt_check(C, "fwd", false)) != CARCA_OK) return rc;
  const XentLayout L = xt_layout(C, false);
  const int64_t part = cx_r64((int64_t)D.splits_items * D.R);
  CARCA_CHECK_ARG(!D.entropy || D.scratch_floats >= L.total + part, "policy_xent_fwd: scratch of %lld floats, %lld needed",
                  (long long)D.scratch_floats, (long long)(L.total + part));
  if ((rc = px_begin(C, D, L, stream)) != CARCA_OK) return rc;
  XentTile A = C.A;
  A.splits = C.splits_n;
  A.part_m = C.scratch + L.part;
  A.part_s = C.scratch + L.part2;
  PolicyTile X = {};
  X.inv_tau = 1.f / D.temperature;
  X.excl = D.n_excl ? D.excl : nullptr, X.E = D.n_excl;
  X.part_w = C.scratch + L.total;
  rc = px_launch_tile(px_kernels<XT_FWD>(D.entropy != nullptr, X.excl != nullptr), A, X, A.R, stream);
  if (rc != CARCA_OK) return rc;
  hipLaunchKernelGGL(px_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D,
                     reinterpret_cast<const int32_t*>(C.scratch) + L.rpos, A.part_m, A.part_s, X.part_w);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
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
  if ((rc = xt_check(C, "bwd", true)) != CARCA_OK) return rc;
  const XentLayout L = xt_layout(C, true);
  if ((rc = px_begin(C, D, L, stream)) != CARCA_OK) return rc;
  const int ldo = (C.A.d + 3) / 4 * 4;
  const int32_t* rpos = reinterpret_cast<const int32_t*>(C.scratch) + L.rpos;
  PolicyTile X = {};
  X.inv_tau = 1.f / D.temperature;
  X.excl = D.n_excl ? D.excl : nullptr, X.E = D.n_excl;
  X.t_off = D.n_excl ? D.t_off : nullptr, X.t_rows = D.t_rows;
  X.c = D.c, X.h = D.h, X.ent = D.entropy;
  // the dP tile, its partials summed per original row (rows that are not valid: 0)
  XentTile A = C.A;
  A.splits = C.splits_n;
  A.out = C.scratch + L.part, A.out_split_stride = (int64_t)A.R * ldo, A.ld_out = ldo;
  rc = px_launch_tile(px_kernels<XT_DP>(ent, X.excl != nullptr), A, X, A.R, stream);
  if (rc != CARCA_OK) return rc;
  {
    const int64_t n = (int64_t)A.R * A.ld_p;
    hipLaunchKernelGGL(px_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, A.out, A.out_split_stride,
                       A.splits, A.ld_out, rpos, A.R, A.d, D.dP, A.ld_p);
    CARCA_LAUNCH_CHECK();
  }
  // the dT tile: one row split writes dT itself, more write partials summed per item
  XentTile B = C.A;
  B.splits = C.splits_rows;
  if (C.splits_rows == 1) {
    B.out = D.dT, B.out_split_stride = 0, B.ld_out = B.ld_t, B.final_out = 1;
  } else {
    B.out = C.scratch + L.part2, B.out_split_stride = (int64_t)B.n * ldo, B.ld_out = ldo;
  }
  rc = px_launch_tile(px_kernels<XT_DT>(ent, X.t_off != nullptr), B, X, B.n, stream);
  if (rc != CARCA_OK) return rc;
  if (C.splits_rows > 1) {
    const int64_t n = (int64_t)B.n * B.ld_t;
    hipLaunchKernelGGL(px_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, B.out, B.out_split_stride,
                       B.splits, B.ld_out, nullptr, B.n, B.d, D.dT, B.ld_t);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}
