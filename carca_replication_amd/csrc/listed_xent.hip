// Softmax cross-entropy over per-list negatives for the dot decoders (include/carca_hip.h: carca_listed_xent_fwd / _bwd;
// DESIGN.md section 30).  Row r reads list g = r / rows_per_list of `lists` [G, N]; entry (g, j) is item lists[g][j], whose
// embedded row is S[index[g][j]] (index < 0: no class):
//
//   z(r, +) = P[r] . Tp[r] + pos_bias[r],   z(r, j) = P[r] . S[index[g][j]] + bias[g][j]
//   CE = sum over valid rows r of ( logsumexp( {z(r, +)} U {z(r, j) : j in N_r} ) - z(r, +) ) / n_valid
//   N_r = { j : index[g][j] >= 0, lists[g][j] in [1, n_items) and lists[g][j] != pos[r] }   (duplicates each count)
//
// with no [R, N] buffer.  The structure is sampled_xent.hip's, with a list per group of rows in place of the K shared
// samples:
//   1. compact (cx_compact_kernel, xent_tile.h): the valid rows (pos in [1, n_items)) in row order.  A group's rows are
//      consecutive, so its valid rows are the consecutive valid-row indices [goff[g], goff[g + 1]), each found by a
//      binary search in ridx (xl_groups_kernel);
//   2. tile (xl_tile_kernel): a workgroup owns 64 entries of one operand (staged once in LDS) and streams 64-entry tiles
//      of the other, with xent_stage.h's register staging (loads clamped and unmasked, masked at the LDS store) and
//      xent_tile.h's two exact-fp32 MFMA products:
//        FWD  own = up to 64 valid rows of one group, stream = the entries of one split of its list (S rows gathered
//             through index): running (max, sum-exp) per (split, row);
//        DP   the same tiles: partial dP[split][v] = sum over the split's entries of G S;
//        DS   own = 64 entries of one list (S rows gathered), stream = the group's valid rows: the entry partial
//             E[g][j] = sum over the group's rows of G P, written once to the [G N, ld] scratch;
//      G = exp(z - lse), 0 where masked;
//   3. FWD: the split partials merged in split order, then the positive term; lse, row loss; the fp64 mean
//      (cx_mean_kernel).  BWD: the positive term (p_pos - 1) Tp[r] is one more dP partial after the splits', and
//      dTp[r] = grad / n_valid (p_pos - 1) P[r]; cx_reduce_kernel sums the partials in split order.  dS[u] = grad /
//      n_valid times the sum of the entry partials of item u in the order of the by-item CSR (csr_ent ascending inside
//      an item): xl_gather_kernel, one wave per item.
// No float atomics: every sum has one fixed order, so two calls give the same bits.
#include "xent_stage.h"

namespace {

struct XlArgs {
  int G, rpl, N, U;      // lists, rows per list, entries per list, rows of S
  int blocks;            // FWD / DP: 64-row blocks per group; DS: 64-entry blocks per list
  const int32_t* lists;  // [G, N]
  const int32_t* index;  // [G, N]
  const float* bias;     // [G, N] or null
  const int32_t* goff;   // [G + 1]: the valid-row index of the first valid row at or after row g rpl (xl_groups_kernel)
};

// the operand row of each piece of the tile of entries first .. first+63 (entries past `end` clamped to end - 1; end >
// first): ROWS: the valid row ridx[entry]; else the row of S of list entry `entry`, clamped into [0, U) (an entry
// that is no class loads row 0 and is masked afterwards)
template <int NCB, bool ROWS>
__device__ __forceinline__ void xl_rows(const XentTile& A, const int32_t* index_g, int U, int (&src)[NCB], int first, int end,
                                        int nc4, int tid) {
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int idx = tid + XT_THREADS * i;
    const int e = min(first + idx / nc4, end - 1);
    int s = 0;
    if (idx < XT_TILE * nc4) s = ROWS ? A.ridx[e] : min(max(index_g[e], 0), U - 1);
    src[i] = s;
  }
}

// the float and id of stream entry s0 + tid (threads 0..63; clamped to s_end - 1, masked when stored).  FWD / DP: the
// entry's bias and its item id, 0 where the entry is no class; DS: lse and pos of the valid row
template <int MODE>
__device__ __forceinline__ void xl_meta(const XentTile& A, const XlArgs& X, size_t eb, int s0, int s_end, int tid, float& f,
                                        int& id) {
  if (tid < XT_TILE) {
    const int e = min(s0 + tid, s_end - 1);
    if constexpr (MODE == XT_DT) {
      const int r = A.ridx[e];
      f = A.lse[r];
      id = A.pos[r];
    } else {
      const int it = X.lists[eb + e];
      f = X.bias ? X.bias[eb + e] : 0.f;
      id = X.index[eb + e] >= 0 && it >= 1 && it < A.n_items ? it : 0;
    }
  }
}

// goff[g] = the number of valid rows in front of row g rpl, g = 0 .. G: ridx is ascending, so a lower bound in it
__global__ __launch_bounds__(256) void xl_groups_kernel(const int32_t* __restrict__ ridx, const int32_t* __restrict__ nv,
                                                        int G, int rpl, int32_t* __restrict__ goff) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g <= G) goff[g] = xt_lower_bound(ridx, 0, nv[0], g * rpl);
}

// NCB: 16-column blocks the kernel is built for (d <= 16 NCB).  Grid: (groups x blocks, splits).
template <int MODE, int NCB>
__global__ __launch_bounds__(XT_THREADS) void xl_tile_kernel(XentTile A, XlArgs X) {
  extern __shared__ float xl_lds[];
  float* own = xl_lds;
  float* str = xl_lds + XT_TILE * A.pitch;
  float* s_f = str + XT_TILE * A.pitch;               // FWD / DP: bias of the stream entries; DS: lse of the stream rows
  int* s_id = reinterpret_cast<int*>(s_f + XT_TILE);  // FWD / DP: item ids of the stream entries; DS: pos of the stream rows
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16), nc4 = kpad / 4;
  const int g = blockIdx.x / X.blocks, blk = blockIdx.x - g * X.blocks, split = blockIdx.y;
  const int v_begin = X.goff[g], v_end = X.goff[g + 1];  // the group's valid rows
  constexpr bool OWN_ROWS = MODE != XT_DT;
  const size_t eb = (size_t)g * X.N;  // the list's first entry
  const int32_t* index_g = X.index + eb;
  const int own0 = OWN_ROWS ? v_begin + blk * XT_TILE : blk * XT_TILE;
  const int own_end = OWN_ROWS ? v_end : X.N;
  if (own0 >= own_end) return;  // (FWD / DP: the grid is sized for rpl rows per group; DS: never)
  int s_begin, s_end;
  if constexpr (OWN_ROWS) {
    s_begin = split * A.per_split;
    s_end = min(s_begin + A.per_split, X.N);
  } else {
    s_begin = v_begin;
    s_end = v_end;
  }
  const int d4 = (A.d + 3) / 4 * 4;
  const float* sbase = OWN_ROWS ? A.T : A.P;  // the streamed operand
  const int sld = OWN_ROWS ? A.ld_t : A.ld_p;
  f32x4 pre[NCB];  // the stream tile in flight
  int src[NCB];    // its pieces' operand rows
  {
    xl_rows<NCB, OWN_ROWS>(A, index_g, X.U, src, own0, own_end, nc4, tid);
    sx_issue<NCB>(OWN_ROWS ? A.P : A.T, OWN_ROWS ? A.ld_p : A.ld_t, src, pre, nc4, d4, tid);
    sx_store<NCB>(A, pre, own, own0, own_end, nc4, tid);
  }
  float pre_f = 0.f;
  int pre_id = 0;
  if (s_begin < s_end) {
    xl_rows<NCB, !OWN_ROWS>(A, index_g, X.U, src, s_begin, s_end, nc4, tid);
    sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
    xl_meta<MODE>(A, X, eb, s_begin, s_end, tid, pre_f, pre_id);
  }

  // this lane's own entry (column r16 of the wave's Z^T tiles)
  const int o_idx = own0 + 16 * w + r16;
  float o_f = 0.f;  // DP: lse of the own row; DS: bias of the own entry
  int o_id = -1;    // FWD / DP: pos of the own row; DS: item id of the own entry
  bool o_ok = false;
  if (o_idx < own_end) {
    if constexpr (OWN_ROWS) {
      const int r = A.ridx[o_idx];
      o_id = A.pos[r];
      if constexpr (MODE == XT_DP) o_f = A.lse[r];
      o_ok = true;
    } else {
      o_id = X.lists[eb + o_idx];
      o_f = X.bias ? X.bias[eb + o_idx] : 0.f;
      o_ok = index_g[o_idx] >= 0 && o_id >= 1 && o_id < A.n_items;
    }
  }
  float run_m = -INFINITY, run_s = 0.f;  // FWD
  f32x4 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += XT_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);  // (every load in flight lands here, on every path: see xs_tile_kernel)
    sx_store<NCB>(A, pre, str, s0, s_end, nc4, tid);
    if (tid < XT_TILE) {
      const bool live = s0 + tid < s_end;
      s_f[tid] = live ? pre_f : 0.f;
      s_id[tid] = live ? pre_id : (MODE == XT_DT ? -1 : 0);  // (id 0: never a class)
    }
    __syncthreads();
    if (s0 + XT_TILE < s_end) {  // the next tile's loads: in flight while this tile multiplies
      xl_rows<NCB, !OWN_ROWS>(A, index_g, X.U, src, s0 + XT_TILE, s_end, nc4, tid);
      sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
      xl_meta<MODE>(A, X, eb, s0 + XT_TILE, s_end, tid, pre_f, pre_id);
    }
    f32x4 z[4];
    xt_logits<NCB>(A, own_row, str, r16, q, z);
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sl = 16 * n + 4 * q + j;
        if constexpr (MODE == XT_FWD) {
          // own row r16 against entries s0 + 16n + 4q + j; masked: hits of the row's positive, no-class entries (id 0)
          const int sid = s_id[sl];
          z[n][j] = sid != 0 && sid != o_id ? z[n][j] + s_f[sl] : -INFINITY;
        } else {
          float gg = 0.f;  // G[own r16][stream 16n + 4q + j], 0 where masked
          if constexpr (MODE == XT_DP) {
            const int sid = s_id[sl];
            if (o_ok && sid != 0 && sid != o_id) gg = __expf(z[n][j] + s_f[sl] - o_f);
          } else {
            if (o_ok && s0 + sl < s_end && s_id[sl] != o_id) gg = __expf(z[n][j] + o_f - s_f[sl]);
          }
          z[n][j] = gg;
        }
      }
    if constexpr (MODE == XT_FWD) xt_running_update(z, run_m, run_s);
    else xt_accumulate<NCB>(A, z, str, r16, q, acc);
  }

  if constexpr (MODE == XT_FWD) {
    xt_store_partial(A, run_m, run_s, split, o_idx, q, v_end);
  } else if constexpr (MODE == XT_DP) {
    xt_epilogue<MODE, NCB>(A, acc, v_end, own0, split, w, lane);
  } else {
    XentTile B = A;  // the list's rows of the entry partials: [N, ld_out] at entry g N, unscaled
    B.n = X.N;
    B.out = A.out + eb * A.ld_out;
    B.final_out = 0;
    xt_epilogue<MODE, NCB, false>(B, acc, nv, own0, 0, w, lane);
  }
}

#define XL_KERNELS(MODE) \
  (XentKernelsT<XlArgs>{xl_tile_kernel<MODE, 4>, xl_tile_kernel<MODE, 8>, xl_tile_kernel<MODE, 16>})

// ---- 3. merges -----------------------------------------------------------------------------------------------------
// per row: the split partials in split order, then the positive term z(r, +) = P[r] . Tp[r] + pos_bias[r]
__global__ __launch_bounds__(256) void xl_merge_kernel(CarcaListedXentDesc D, int splits, const int32_t* __restrict__ rpos,
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
  if (D.pos_bias) zp += D.pos_bias[r];
  float M = zp;
  for (int s = 0; s < splits; ++s) M = fmaxf(M, part_m[(size_t)s * D.R + v]);
  float sum = 0.f;
  for (int s = 0; s < splits; ++s) {
    const float m = part_m[(size_t)s * D.R + v];
    if (m > -INFINITY) sum += part_s[(size_t)s * D.R + v] * expf(m - M);
  }
  sum += expf(zp - M);
  const float lse = M + logf(sum);
  D.lse[r] = lse;
  D.row_loss[r] = lse - zp;
}

// the positive term of the backward, p_pos = exp(z(r, +) - lse) = exp(-row_loss):
//   part[v][col] = (p_pos - 1) Tp[r][col]          (col < ldo: dP's last partial, unscaled, by valid-row index)
//   dTp[r][col]  = grad / n_valid (p_pos - 1) P[r][col]    (0 for padding rows and past d)
__global__ __launch_bounds__(256) void xl_positive_kernel(CarcaListedXentDesc D, const int32_t* __restrict__ rpos,
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

// dS[u] = grad / n_valid (sum of the entry partials ent[csr_ent[k]], k = csr_off[u] .. csr_off[u + 1] - 1, in that
// order); zeros past d.  One wave per item, a lane per 16-byte column piece
__global__ __launch_bounds__(256) void xl_gather_kernel(CarcaListedXentDesc D, const float* __restrict__ ent, int ldo,
                                                        const int32_t* __restrict__ nv) {
  const int u = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (u >= D.U) return;
  const int64_t n_ent = (int64_t)D.G * D.N;
  const int k0 = max(D.csr_off[u], 0), k1 = (int)min((int64_t)D.csr_off[u + 1], n_ent);
  const int n = nv[0];
  const float coef = n > 0 ? D.grad[0] / (float)n : 0.f;
  for (int c = 4 * lane; c < D.ld_s; c += 256) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    if (c < ldo) {
      for (int k = k0; k < k1; ++k) {
        const int e = D.csr_ent[k];
        if (e >= 0 && e < n_ent) a += *reinterpret_cast<const f32x4*>(ent + (size_t)e * ldo + c);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = c + j < D.d ? a[j] * coef : 0.f;
    *reinterpret_cast<f32x4*>(D.dS + (size_t)u * D.ld_s + c) = a;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------
// scratch in 4-byte words (mirrored by ops.listed_xent_plan): the row lists, nv, the group offsets, then the forward's (max, sum-exp)
// partials [splits][R] each, or the backward's dP partials [splits + 1][R][ldo] and the entry partials [G N][ldo]
struct XlLayout {
  int64_t ridx, rpos, nv, goff, part, part2, ent, total;
};
XlLayout xl_layout(const CarcaListedXentDesc& D, bool bwd) {
  XlLayout L;
  const int64_t R = D.R, ldo = (D.d + 3) / 4 * 4;
  L.ridx = 0;
  L.rpos = cx_r64(R);
  L.nv = 2 * cx_r64(R);
  L.goff = L.nv + 64;
  L.part = L.goff + cx_r64((int64_t)D.G + 1);
  if (!bwd) {
    L.part2 = L.part + cx_r64((int64_t)D.splits * R);
    L.ent = 0;
    L.total = L.part2 + cx_r64((int64_t)D.splits * R);
  } else {
    L.part2 = 0;
    L.ent = L.part + cx_r64((int64_t)(D.splits + 1) * R * ldo);
    L.total = L.ent + cx_r64((int64_t)D.G * D.N * ldo);
  }
  return L;
}

// the checks of both passes, the tile arguments and the compact launch
int xl_begin(const CarcaListedXentDesc& D, const char* what, bool bwd, XentCall& C, XlArgs& X, XlLayout& L,
             hipStream_t stream) {
  CARCA_CHECK_ARG(D.R >= 1 && D.G >= 1 && D.N >= 1 && D.U >= 0 && D.n_items >= 1 && D.d >= 1,
                  "%s: the row, list, entry and item counts and d must be positive (U may be 0)", what);
  CARCA_CHECK_ARG(D.rows_per_list >= 1 && D.rows_per_list <= 1024 && (int64_t)D.G * D.rows_per_list == D.R,
                  "%s: rows_per_list must lie in 1..1024 with R = G rows_per_list", what);
  CARCA_CHECK_SUPPORTED(D.d <= XT_MAX_D, "%s: d = %d exceeds %d", what, D.d, XT_MAX_D);
  CARCA_CHECK_SUPPORTED((int64_t)D.G * D.N < (1ll << 31) && (int64_t)D.R + 64 < (1ll << 31) / 64,
                        "%s: G N must stay below 2^31 and R below 2^25", what);
  CARCA_CHECK_ARG(D.P && D.Tp && D.pos && D.lists && D.index && D.scratch && D.lse && D.row_loss && (D.S || D.U == 0),
                  "%s: null P, Tp, pos, S, lists, index, scratch, lse or row_loss", what);
  CARCA_CHECK_ARG(D.ld_p >= D.d && D.ld_p % 4 == 0 && D.ld_tp >= D.d && D.ld_tp % 4 == 0 &&
                      (D.U == 0 || (D.ld_s >= D.d && D.ld_s % 4 == 0)),
                  "%s: the row strides must be multiples of 4, at least d", what);
  CARCA_CHECK_ARG(((uintptr_t)D.P & 15) == 0 && ((uintptr_t)D.S & 15) == 0 && ((uintptr_t)D.scratch & 15) == 0,
                  "%s: P, S and scratch must be 16-byte aligned", what);
  CARCA_CHECK_ARG(D.splits >= 1 && D.splits <= XT_MAX_SPLITS && D.entries_per_split >= 1 &&
                      D.entries_per_split % XT_TILE == 0 && (int64_t)D.entries_per_split * D.splits >= D.N,
                  "%s: 1..%d splits of a multiple of %d entries covering the list", what, XT_MAX_SPLITS, XT_TILE);
  CARCA_CHECK_SUPPORTED((int64_t)D.R * D.ld_p < (1ll << 40) && (int64_t)D.R * D.ld_tp < (1ll << 40) &&
                            (int64_t)D.U * D.ld_s < (1ll << 40),
                        "%s: operands too large", what);
  L = xl_layout(D, bwd);
  CARCA_CHECK_ARG(D.scratch_floats >= L.total, "%s: scratch of %lld floats, %lld needed", what, (long long)D.scratch_floats,
                  (long long)L.total);
  if (!bwd) {
    CARCA_CHECK_ARG(D.loss, "%s: null loss", what);
  } else {
    CARCA_CHECK_ARG(D.grad && D.dP && D.dTp, "%s: null grad, dP or dTp", what);
    CARCA_CHECK_ARG(D.U == 0 || (D.dS && D.csr_off && D.csr_ent && ((uintptr_t)D.dS & 15) == 0),
                    "%s: null csr_off or csr_ent, or dS null or not 16-byte aligned", what);
  }
  C = {};
  C.op = "listed_xent";
  int32_t* base = reinterpret_cast<int32_t*>(D.scratch);
  XentTile& A = C.A;
  A.R = D.R, A.n = D.N, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_s;
  A.P = D.P, A.T = D.S, A.pos = D.pos;
  A.lse = D.lse, A.grad = D.grad;
  A.per_split = D.entries_per_split;
  A.ridx = base + L.ridx, A.nv = base + L.nv;
  A.pitch = round_up(D.d, 16) + 4;
  X = {};
  X.G = D.G, X.rpl = D.rows_per_list, X.N = D.N, X.U = D.U;
  X.lists = D.lists, X.index = D.index, X.bias = D.bias, X.goff = base + L.goff;
  hipLaunchKernelGGL(cx_compact_kernel<false>, dim3(1), dim3(CX_COMPACT_THREADS), 0, stream, D.pos, D.R, D.n_items,
                     base + L.ridx, base + L.rpos, base + L.nv, (const int32_t*)nullptr, 0);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(xl_groups_kernel, dim3(D.G / 256 + 1), dim3(256), 0, stream, base + L.ridx, base + L.nv, D.G,
                     D.rows_per_list, base + L.goff);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_listed_xent_fwd(const CarcaListedXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "listed_xent_fwd: null descriptor");
  const CarcaListedXentDesc& D = *desc;
  XentCall C;
  XlArgs X;
  XlLayout L;
  int rc = xl_begin(D, "listed_xent_fwd", false, C, X, L, stream);
  if (rc != CARCA_OK) return rc;
  XentTile A = C.A;
  A.splits = D.splits;
  A.part_m = D.scratch + L.part;
  A.part_s = D.scratch + L.part2;
  if (D.U > 0) {
    X.blocks = (D.rows_per_list + XT_TILE - 1) / XT_TILE;
    if ((rc = xt_launch_tile(C, XL_KERNELS(XT_FWD), A, D.G * X.blocks * XT_TILE, stream, X)) != CARCA_OK) return rc;
  }
  // (no row of S: every list is empty, and the merge reads no partial)
  hipLaunchKernelGGL(xl_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D, D.U > 0 ? D.splits : 0,
                     reinterpret_cast<const int32_t*>(D.scratch) + L.rpos, A.part_m, A.part_s);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(cx_mean_kernel, dim3(1), dim3(1024), 0, stream, D.row_loss, D.R, D.loss, A.nv);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_listed_xent_bwd(const CarcaListedXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "listed_xent_bwd: null descriptor");
  const CarcaListedXentDesc& D = *desc;
  XentCall C;
  XlArgs X;
  XlLayout L;
  int rc = xl_begin(D, "listed_xent_bwd", true, C, X, L, stream);
  if (rc != CARCA_OK) return rc;
  const int ldo = (D.d + 3) / 4 * 4;
  const int32_t* rpos = reinterpret_cast<const int32_t*>(D.scratch) + L.rpos;
  const int splits = D.U > 0 ? D.splits : 0;
  XentTile A = C.A;
  A.splits = D.splits;
  A.out = D.scratch + L.part, A.out_split_stride = (int64_t)D.R * ldo, A.ld_out = ldo;
  if (D.U > 0) {
    X.blocks = (D.rows_per_list + XT_TILE - 1) / XT_TILE;
    if ((rc = xt_launch_tile(C, XL_KERNELS(XT_DP), A, D.G * X.blocks * XT_TILE, stream, X)) != CARCA_OK) return rc;
  }
  // the positive term: dP's last partial, after the entry splits'; dTp
  const int64_t ntp = (int64_t)D.R * D.ld_tp;
  hipLaunchKernelGGL(xl_positive_kernel, dim3((unsigned)((ntp + 255) / 256)), dim3(256), 0, stream, D, rpos, A.nv,
                     A.out + (size_t)splits * A.out_split_stride, ldo);
  CARCA_LAUNCH_CHECK();
  A.splits = splits;
  xt_reduce<true>(A, 1, rpos, D.R, D.dP, D.ld_p, stream);
  CARCA_LAUNCH_CHECK();
  if (D.U > 0) {
    XentTile B = C.A;
    B.splits = 1;
    B.out = D.scratch + L.ent, B.out_split_stride = 0, B.ld_out = ldo, B.final_out = 0;
    X.blocks = (D.N + XT_TILE - 1) / XT_TILE;
    CARCA_CHECK_SUPPORTED((int64_t)D.G * X.blocks < (1ll << 31) / XT_TILE, "listed_xent_bwd: too many entry blocks");
    if ((rc = xt_launch_tile(C, XL_KERNELS(XT_DT), B, D.G * X.blocks * XT_TILE, stream, X)) != CARCA_OK) return rc;
    hipLaunchKernelGGL(xl_gather_kernel, dim3((D.U + 3) / 4), dim3(256), 0, stream, D, D.scratch + L.ent, ldo, B.nv);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}
