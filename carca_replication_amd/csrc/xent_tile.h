// The tile skeleton and host path of the softmax cross-entropy family.  Four ops run on it, through two tile kernels:
//   xd_tile_kernel (xent_direct.h: tiles staged straight into LDS)   catalogue_xent.hip (the classes are the whole
//       catalogue) and policy_xent.hip (the same classes under a temperature, per-row exclusion
//       lists and per-row coefficients, with the entropy; section 29);
//   xs_tile_kernel (xent_stage.h: tiles staged one step ahead in registers)   sampled_xent.hip (the classes are K shared
//       samples with the logQ correction, section 14) and sampled_bce.hip (a sigmoid loss over them, section 16).
//
// A workgroup of four waves owns 64 rows of one operand (the "own" tile, staged once in LDS) and streams 64-row tiles of
// the other through LDS.  Wave w owns own rows 16w .. 16w+15; lane l holds column r16 = l & 15 and the stream rows
// 16n + 4q + j (q = l >> 4) of the 64 x 16 logit tile Z^T = S O^T, which is exactly the A operand of the second product
// out += G * stream, so G never leaves the registers.  What lives here, once:
//   device: the split range of a workgroup, the direct staging of a tile, the Z^T product, the running (max, sum-exp)
//           update of masked logits, the G * stream accumulation, the four-lane merge with its partial store, the output
//           epilogue with its zero tail (scaled by grad / n_valid, or SCALED = false: by nothing);
//           cx_compact_kernel (the valid rows, pos in [1, n_items) and, LISTS, not in the row's own sorted list, in row
//           order), cx_mean_kernel (the fp64 mean of the row losses) and cx_reduce_kernel (split partials summed in split
//           order, scaled like the epilogue);
//   host:   the call description and scratch layout, the checks the descriptors share, the LDS-size / NCB dispatch, and
//           the launch sequences of the forward (compact, tile, merge, and MEAN: mean) and the backward (compact, dP
//           tile, reduce, dT tile, reduce), for a mean loss under a scalar grad (MEAN, the three losses) or per-row
//           values under per-row coefficients (policy_xent).
// What each tile kernel keeps: how it stages a tile and its mask tests around a rule struct's hooks.  What each client
// keeps: its rule (CatalogueRule, PolicyRule<ENT, LISTS>; SxRule, SbRule), its merge kernel, the checks of its own
// descriptor fields, and two short entry points; the sampled losses also their positive-term and pre-pass kernels, the
// policy its three-value running update and lane merge for the entropy.
#pragma once
#include "carca_common.h"
#include "../../include/carca_hip.h"

#include <math.h>

namespace {

constexpr int XT_THREADS = 256;
constexpr int XT_TILE = 64;  // own rows per workgroup (16 per wave) and stream rows per step
constexpr int XT_MAX_D = 256;
constexpr int XT_MAX_SPLITS = 256;
constexpr int CX_COMPACT_THREADS = 1024;
enum { XT_FWD = 0, XT_DP = 1, XT_DT = 2 };  // DT: the gradient of the class operand (dT, dS)

__host__ __device__ inline int64_t cx_r64(int64_t n) { return (n + 63) / 64 * 64; }

// ---- the arguments of a tile kernel ----------------------------------------------------------------------------------
struct XentTile {
  int R, n, n_items, d, ld_p, ld_t;  // n: classes (the catalogue's items, or the K samples); ids lie in [1, n_items)
  const float* P;
  const float* T;                    // the class operand [n, ld_t]
  const int32_t* pos;
  const int32_t* ids;                // sampled: item id of each class (catalogue: null, class i is item i)
  const float* bias;                 // sampled: logQ correction of each class (catalogue: null)
  const int32_t* ridx;
  const int32_t* nv;
  const float* lse;   // backward: per original row
  const float* grad;  // backward: upstream scale [1]
  int splits;         // FWD / DP: class splits; DT: row splits
  int per_split;      // FWD / DP: classes per split (a multiple of XT_TILE)
  int pitch;          // LDS row pitch in floats
  float* part_m;      // FWD: [splits][R]
  float* part_s;
  float* out;         // DP: [splits][R][ld_out] by valid-row index; DT: [splits][n][ld_out], or dT itself
  int64_t out_split_stride;
  int ld_out;
  int final_out;      // DT with one split: scale by grad / n_valid and write zeros past d (out = dT)
};

// ---- device helpers ---------------------------------------------------------------------------------------------------
// stream entries [s_begin, s_end) of the workgroup of split `split`: FWD / DP stream the classes of one split, DT the
// valid rows of one split.  (The early return of a FWD / DP row block past n_valid stays in the kernel, in front of this
// call: returned through here as a bool, it changed the sampled forward's prologue and cost it 2 % at K = 8192.)
template <int MODE>
__device__ __forceinline__ void xt_split_range(const XentTile& A, int nv, int split, int& s_begin, int& s_end) {
  if constexpr (MODE != XT_DT) {
    s_begin = split * A.per_split;
    s_end = min(s_begin + A.per_split, A.n);
  } else {
    const int nb = (nv + XT_TILE - 1) / XT_TILE;
    s_begin = (int)((long long)split * nb / A.splits) * XT_TILE;
    s_end = min((int)((long long)(split + 1) * nb / A.splits) * XT_TILE, nv);
  }
}

// A 64-row tile straight into LDS (the direct-staged kernel's staging; xs_tile_kernel has its own, through registers):
// entries first .. end-1 are valid-row indices (rows: P[ridx[v]]) or class indices (T[i]).  Zero past `end` and past d.
__device__ __forceinline__ void xt_stage_direct(const XentTile& A, float* dst, int first, int end, bool rows, int kpad,
                                                int tid) {
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

// first index in [lo, hi) of the ascending list a whose entry is >= key
__device__ __forceinline__ int xt_lower_bound(const int32_t* a, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Z^T[stream 16n + 4q + reg][own r16] for the four 16-row stream blocks n (own_row: the lane's own row, at column 4q).
// (The products accumulate in locals, copied to the caller's array at the end: accumulating through the reference costs
// every instantiation 12 more AGPRs, and two of them a wave of occupancy.)
template <int NCB>
__device__ __forceinline__ void xt_logits(const XentTile& A, const float* own_row, const float* str, int r16, int q,
                                          f32x4 (&z_out)[4]) {
  const int nkg = round_up(A.d, 16) / 16;
  f32x4 z[4];
#pragma unroll
  for (int n = 0; n < 4; ++n) z[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kg = 0; kg < NCB; ++kg) {
    if (kg < nkg) {
      const f32x4 b = *reinterpret_cast<const f32x4*>(own_row + 16 * kg);
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(str + (16 * n + r16) * A.pitch + 16 * kg + 4 * q);
        z[n] = mfma16_group(a, b, z[n]);
      }
    }
  }
#pragma unroll
  for (int n = 0; n < 4; ++n) z_out[n] = z[n];
}

// the lane's running (max, sum-exp) over one more tile of logits, -inf where masked
__device__ __forceinline__ void xt_running_update(const f32x4 (&z)[4], float& run_m, float& run_s) {
  float cm = -INFINITY;
#pragma unroll
  for (int n = 0; n < 4; ++n)
#pragma unroll
    for (int j = 0; j < 4; ++j) cm = fmaxf(cm, z[n][j]);
  if (cm > -INFINITY) {
    const float mn = fmaxf(run_m, cm);
    float s = run_m > -INFINITY ? run_s * __expf(run_m - mn) : 0.f;
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (z[n][j] > -INFINITY) s += __expf(z[n][j] - mn);
    run_m = mn;
    run_s = s;
  }
}

// out[own r16][col 16c + l&15] += sum over the 64 stream rows of G * stream  (k = stream 16n + 4q + j at step j)
template <int NCB>
__device__ __forceinline__ void xt_accumulate(const XentTile& A, const f32x4 (&g)[4], const float* str, int r16, int q,
                                              f32x4 (&acc)[NCB]) {
  const int ncb = (A.d + 15) / 16;
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    if (c < ncb) {
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[c] = mfma16(g[n][j], str[(16 * n + 4 * q + j) * A.pitch + 16 * c + r16], acc[c]);
    }
  }
}

// FWD: merge the four lanes of own row r16 (lanes r16 + 16q; max and + are commutative, so every lane gets the same
// bits) and store the (max, sum) partial of (split, valid row o_idx)
__device__ __forceinline__ void xt_store_partial(const XentTile& A, float run_m, float run_s, int split, int o_idx, int q,
                                                 int nv) {
#pragma unroll
  for (int x = 16; x <= 32; x *= 2) {
    const float om = __shfl_xor(run_m, x), os = __shfl_xor(run_s, x);
    const float mn = fmaxf(run_m, om);
    const float a = run_m > -INFINITY ? run_s * __expf(run_m - mn) : 0.f;
    const float b = om > -INFINITY ? os * __expf(om - mn) : 0.f;
    run_m = mn;
    run_s = a + b;
  }
  if (q == 0 && o_idx < nv) {
    A.part_m[(size_t)split * A.R + o_idx] = run_m;
    A.part_s[(size_t)split * A.R + o_idx] = run_s;
  }
}

// DP / DT: D of acc[c] is column 16c + r16 of own rows 16w + 4q + j.  final_out (DT with one row split): out is the class
// gradient itself, zeros up to the row stride and, SCALED, the grad / n_valid factor (not SCALED: no factor anywhere, and
// neither nv's nor grad's read nor a multiply in the code)
template <int MODE, int NCB, bool SCALED = true>
__device__ __forceinline__ void xt_epilogue(const XentTile& A, const f32x4 (&acc)[NCB], int nv, int own0, int split, int w,
                                            int lane) {
  const int r16 = lane & 15, q = lane >> 4, ncb = (A.d + 15) / 16;
  float* out = A.out + (size_t)split * A.out_split_stride;
  float coef = 1.f;
  if constexpr (SCALED && MODE == XT_DT) {
    if (A.final_out) coef = nv > 0 ? A.grad[0] / (float)nv : 0.f;
  }
  const int own_end = MODE == XT_DP ? nv : A.n;
#pragma unroll
  for (int c = 0; c < NCB; ++c) {
    if (c < ncb) {
      const int col = 16 * c + r16;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int e = own0 + 16 * w + 4 * q + j;
        if (e < own_end && col < A.ld_out) out[(size_t)e * A.ld_out + col] = col < A.d ? (SCALED ? acc[c][j] * coef : acc[c][j]) : 0.f;
      }
    }
  }
  if (MODE == XT_DT && A.final_out) {  // columns past the 16-column blocks, up to the row stride
    for (int col = 16 * ncb + lane; col < A.ld_out; col += 64)
      for (int j = 0; j < 16; ++j) {
        const int e = own0 + 16 * w + j;
        if (e < A.n) out[(size_t)e * A.ld_out + col] = 0.f;
      }
  }
}

// ---- valid rows, in row order -----------------------------------------------------------------------------------
// LISTS: a row whose pos is in its own ascending list excl[r][0 .. E) is not valid either (policy_xent.hip)
template <bool LISTS>
__global__ __launch_bounds__(CX_COMPACT_THREADS) void cx_compact_kernel(const int32_t* __restrict__ pos, int R, int n_items,
                                                                         int32_t* __restrict__ ridx,
                                                                         int32_t* __restrict__ rpos, int32_t* __restrict__ nv,
                                                                         const int32_t* __restrict__ excl, int E) {
  __shared__ int wsum[CX_COMPACT_THREADS / 64];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < R; r0 += CX_COMPACT_THREADS) {
    const int r = r0 + tid;
    const int p = r < R ? pos[r] : 0;
    bool ok = r < R && p >= 1 && p < n_items;
    if constexpr (LISTS) {
      if (ok) {
        const int32_t* l = excl + (size_t)r * E;
        const int at = xt_lower_bound(l, 0, E, p);
        ok = !(at < E && l[at] == p);
      }
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

__global__ __launch_bounds__(1024) void cx_mean_kernel(const float* __restrict__ row_loss, int R, float* __restrict__ loss,
                                                       const int32_t* __restrict__ nv) {
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int r = tid; r < R; r += 1024) s += (double)row_loss[r];
  red[tid] = s;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) loss[0] = nv[0] > 0 ? (float)(red[0] / (double)nv[0]) : 0.f;
}

// dst[e][col] (col < ld_dst) = coef * sum over splits of part[s][map(e)][col] for col < d, else 0; coef = grad / n_valid,
// or, not SCALED, no factor (nv and grad are not read)
template <bool SCALED>
__global__ __launch_bounds__(256) void cx_reduce_kernel(const float* __restrict__ part, int64_t split_stride, int splits,
                                                        int ld_part, const int32_t* __restrict__ rpos, int rows, int d,
                                                        float* __restrict__ dst, int ld_dst, const int32_t* __restrict__ nv,
                                                        const float* __restrict__ grad) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * ld_dst) return;
  const int e = (int)(idx / ld_dst), col = (int)(idx - (int64_t)e * ld_dst);
  const int src = rpos ? rpos[e] : e;
  float v = 0.f;
  if (src >= 0 && col < d) {
    for (int s = 0; s < splits; ++s) v += part[(size_t)s * split_stride + (size_t)src * ld_part + col];
    if constexpr (SCALED) {
      const int n = nv[0];
      v *= n > 0 ? grad[0] / (float)n : 0.f;
    }
  }
  dst[(size_t)e * ld_dst + col] = v;
}

// ---- host side -----------------------------------------------------------------------------------------------------
// One call under one set of names, filled from either descriptor.  A carries the operands (R, n, n_items, d, P, T, pos,
// ids, bias, lse, grad, per_split); the rest is what the launch sequences need beside them.
//
// MEAN, the host path's one compile-time switch (a template argument, so that an op's code object holds only the helper
// kernels it launches): true for the three mean losses, whose backward scales by the scalar grad / n_valid and whose
// forward ends with cx_mean_kernel over row_loss.  false for policy_xent: per-row outputs under per-row coefficients that
// its tile kernel reads itself, so nothing scales (no grad, no row_loss / loss, no mean launch), and a row may carry an
// exclusion list that the compact pass consults.
struct XentCall {
  XentTile A;
  const char* op;       // "catalogue_xent" / "sampled_xent" / "sampled_bce" / "policy_xent"
  const char* classes;  // what a class is called in messages
  float* scratch;
  int64_t scratch_floats;
  int splits_n, splits_rows;  // class splits (FWD / DP), row splits (DT)
  int extra_dp;               // dP partials written after the class splits' (sampled: the positive term)
  int share_partials;         // backward: the class operand's partials reuse the dP partials' words (see XentLayout)
  float* row_loss;
  float* loss;
  float* dP;  // [R, ld_p]
  float* dT;  // [n, ld_t]
  int fwd_parts = 2;    // forward partials per (split, valid row): (max, sum-exp), and with 3 the entropy's sum
  const int32_t* excl;  // not MEAN: [R][n_excl] by original row, each row ascending; null: no lists
  int n_excl;
};

// scratch layout in 4-byte words (mirrored by ops._xent_plan): the row lists, nv, then the forward's fwd_parts partials
// per split and valid row, or the backward's dP partials [splits_n + extra_dp][R][ldo] and, with more than one row split,
// the class operand's partials [splits_rows][n][ldo].  The dP partials are summed into dP before the class operand's tile
// launches (one stream), so with share_partials the second set starts where the first does and the scratch is the larger
// of the two, not their sum.
struct XentLayout {
  int64_t ridx, rpos, nv, part, part2, part3, total;  // part3: the forward's third partial (fwd_parts = 3)
};
inline XentLayout xt_layout(const XentCall& C, bool bwd) {
  XentLayout L;
  const int64_t R = C.A.R, ldo = (C.A.d + 3) / 4 * 4;
  L.ridx = 0;
  L.rpos = cx_r64(R);
  L.nv = 2 * cx_r64(R);
  L.part = L.nv + 64;
  L.part3 = 0;
  if (!bwd) {
    const int64_t one = cx_r64((int64_t)C.splits_n * R);
    L.part2 = L.part + one;
    L.part3 = L.part2 + one;
    L.total = L.part + C.fwd_parts * one;
  } else {
    const int64_t dp = cx_r64((int64_t)(C.splits_n + C.extra_dp) * R * ldo);
    const int64_t dt = C.splits_rows > 1 ? cx_r64((int64_t)C.splits_rows * C.A.n * ldo) : 0;
    L.part2 = C.share_partials ? L.part : L.part + dp;
    L.total = C.share_partials ? L.part + (dp > dt ? dp : dt) : L.part2 + dt;
  }
  return L;
}

// the checks the descriptors share (each entry point checks its own operands and outputs beside these)
template <bool MEAN = true>
int xt_check(const XentCall& C, const char* pass, bool bwd) {
  const XentTile& A = C.A;
  CARCA_CHECK_ARG(A.R >= 1 && A.n >= 1 && A.n_items >= 1 && A.d >= 1, "%s_%s: the row, %s and item counts and d must be positive",
                  C.op, pass, C.classes);
  CARCA_CHECK_SUPPORTED(A.d <= XT_MAX_D, "%s_%s: d = %d exceeds %d", C.op, pass, A.d, XT_MAX_D);
  CARCA_CHECK_ARG(A.P && A.T && A.pos && C.scratch, "%s_%s: null P, %s operand, pos or scratch", C.op, pass, C.classes);
  CARCA_CHECK_ARG(A.ld_p >= A.d && A.ld_p % 4 == 0 && A.ld_t >= A.d && A.ld_t % 4 == 0,
                  "%s_%s: the row strides must be multiples of 4, at least d", C.op, pass);
  CARCA_CHECK_ARG(((uintptr_t)A.P & 15) == 0 && ((uintptr_t)A.T & 15) == 0, "%s_%s: P and the %s operand must be 16-byte aligned",
                  C.op, pass, C.classes);
  CARCA_CHECK_ARG(C.splits_n >= 1 && C.splits_n <= XT_MAX_SPLITS && C.splits_rows >= 1 && C.splits_rows <= XT_MAX_SPLITS,
                  "%s_%s: split counts outside 1..%d", C.op, pass, XT_MAX_SPLITS);
  CARCA_CHECK_ARG(A.per_split >= 1 && A.per_split % XT_TILE == 0 && (int64_t)A.per_split * C.splits_n >= A.n,
                  "%s_%s: %s per split must be a multiple of %d covering all of them in the given splits", C.op, pass,
                  C.classes, XT_TILE);
  CARCA_CHECK_SUPPORTED((int64_t)A.n * A.ld_t < (1ll << 40) && (int64_t)A.R * A.ld_p < (1ll << 40),
                        "%s_%s: operands too large", C.op, pass);
  const XentLayout L = xt_layout(C, bwd);
  CARCA_CHECK_ARG(C.scratch_floats >= L.total, "%s_%s: scratch of %lld floats, %lld needed", C.op, pass,
                  (long long)C.scratch_floats, (long long)L.total);
  CARCA_CHECK_ARG(A.lse, "%s_%s: null lse", C.op, pass);
  if (!bwd) {
    CARCA_CHECK_ARG(!MEAN || (C.row_loss && C.loss), "%s_%s: null row_loss or loss", C.op, pass);
  } else {
    CARCA_CHECK_ARG((!MEAN || A.grad) && C.dP && C.dT, "%s_%s: null grad or gradient output", C.op, pass);
  }
  return CARCA_OK;
}

// the tile kernels of one mode, built for d <= 64, 128, 256 (NCB = 4, 8, 16).  X: what the kernel takes by value after
// XentTile (the sampled kernels: nothing; the direct-staged kernel: its rule's Args); row_words: the 4-byte words of LDS
// the kernel keeps per stream row beside the tile
template <class... X>
struct XentKernelsT {
  void (*k4)(XentTile, X...);
  void (*k8)(XentTile, X...);
  void (*k16)(XentTile, X...);
  int row_words = 2;
};
using XentKernels = XentKernelsT<>;

template <class... X>
int xt_launch_tile(const XentCall& C, const XentKernelsT<X...>& K, const XentTile& A, int own_entries, hipStream_t stream,
                   const X&... x) {
  const size_t lds = (size_t)2 * XT_TILE * A.pitch * sizeof(float) + XT_TILE * K.row_words * sizeof(float);
  const auto kern = A.d <= 64 ? K.k4 : A.d <= 128 ? K.k8 : K.k16;
  hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) {
    carca_set_error("%s: cannot reserve %zu B of LDS: %s", C.op, lds, hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(kern, dim3((own_entries + XT_TILE - 1) / XT_TILE, A.splits), dim3(XT_THREADS), lds, stream, A, x...);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// the scratch pointers of a call's tile arguments, the LDS pitch, and the compact launch every call starts with
template <bool MEAN>
int xt_begin(XentCall& C, const XentLayout& L, hipStream_t stream) {
  int32_t* base = reinterpret_cast<int32_t*>(C.scratch);
  C.A.ridx = base + L.ridx, C.A.nv = base + L.nv;
  C.A.pitch = round_up(C.A.d, 16) + 4;  // (+4 floats: the 16 rows of a 16-byte LDS read start 4 banks apart)
  auto compact = cx_compact_kernel<false>;
  if constexpr (!MEAN) {
    if (C.excl) compact = cx_compact_kernel<true>;
  }
  hipLaunchKernelGGL(compact, dim3(1), dim3(CX_COMPACT_THREADS), 0, stream, C.A.pos, C.A.R, C.A.n_items, base + L.ridx,
                     base + L.rpos, base + L.nv, C.excl, C.n_excl);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// forward: compact, FWD tile, merge(rpos, part_m, part_s) (the caller's launch: lse and the row's value), and, MEAN, the
// fp64 mean.  x: the tile kernel's arguments after XentTile
template <bool MEAN = true, class Merge, class... X>
int xt_forward(XentCall& C, const XentKernelsT<X...>& fwd, hipStream_t stream, Merge merge, const X&... x) {
  int rc = xt_check<MEAN>(C, "fwd", false);
  if (rc != CARCA_OK) return rc;
  const XentLayout L = xt_layout(C, false);
  if ((rc = xt_begin<MEAN>(C, L, stream)) != CARCA_OK) return rc;
  XentTile A = C.A;
  A.splits = C.splits_n;
  A.part_m = C.scratch + L.part;
  A.part_s = C.scratch + L.part2;
  if ((rc = xt_launch_tile(C, fwd, A, A.R, stream, x...)) != CARCA_OK) return rc;
  merge(reinterpret_cast<const int32_t*>(C.scratch) + L.rpos, A.part_m, A.part_s);
  CARCA_LAUNCH_CHECK();
  if constexpr (MEAN) {
    hipLaunchKernelGGL(cx_mean_kernel, dim3(1), dim3(1024), 0, stream, C.row_loss, A.R, C.loss, A.nv);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}

// a tile launch whose `splits` partials (A.out) cx_reduce_kernel then sums into dst [rows, ld_dst] with `extra` more
template <bool MEAN>
void xt_reduce(const XentTile& A, int extra, const int32_t* rpos, int rows, float* dst, int ld_dst, hipStream_t stream) {
  const int64_t n = (int64_t)rows * ld_dst;
  hipLaunchKernelGGL(cx_reduce_kernel<MEAN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, A.out,
                     A.out_split_stride, A.splits + extra, A.ld_out, rpos, rows, A.d, dst, ld_dst, A.nv, A.grad);
}

// backward: compact; the dP tile, extra(rpos, nv, part, ldo) (the caller's launch writing the extra_dp partials; unused
// with none), the partials summed per original row (padding rows: 0); the dT tile, where one row split writes dT itself
// and more write partials summed per class.  x: the tile kernels' arguments after XentTile
template <bool MEAN = true, class Extra, class... X>
int xt_backward(XentCall& C, const XentKernelsT<X...>& dp, const XentKernelsT<X...>& dt, hipStream_t stream, Extra extra,
                const X&... x) {
  int rc = xt_check<MEAN>(C, "bwd", true);
  if (rc != CARCA_OK) return rc;
  const XentLayout L = xt_layout(C, true);
  if ((rc = xt_begin<MEAN>(C, L, stream)) != CARCA_OK) return rc;
  const int ldo = (C.A.d + 3) / 4 * 4;
  const int32_t* rpos = reinterpret_cast<const int32_t*>(C.scratch) + L.rpos;
  XentTile A = C.A;
  A.splits = C.splits_n;
  A.out = C.scratch + L.part, A.out_split_stride = (int64_t)A.R * ldo, A.ld_out = ldo;
  if ((rc = xt_launch_tile(C, dp, A, A.R, stream, x...)) != CARCA_OK) return rc;
  if (C.extra_dp) {
    extra(rpos, A.nv, A.out + (size_t)C.splits_n * A.out_split_stride, ldo);
    CARCA_LAUNCH_CHECK();
  }
  xt_reduce<MEAN>(A, C.extra_dp, rpos, A.R, C.dP, A.ld_p, stream);
  CARCA_LAUNCH_CHECK();
  XentTile B = C.A;
  B.splits = C.splits_rows;
  if (C.splits_rows == 1) {
    B.out = C.dT, B.out_split_stride = 0, B.ld_out = B.ld_t, B.final_out = 1;
  } else {
    B.out = C.scratch + L.part2, B.out_split_stride = (int64_t)B.n * ldo, B.ld_out = ldo;
  }
  if ((rc = xt_launch_tile(C, dt, B, B.n, stream, x...)) != CARCA_OK) return rc;
  if (C.splits_rows > 1) {
    xt_reduce<MEAN>(B, 0, nullptr, B.n, C.dT, B.ld_t, stream);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}

}  // namespace
