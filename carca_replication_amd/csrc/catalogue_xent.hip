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
#include "catalogue_xent_common.h"

#include <math.h>

namespace {

constexpr int CX_THREADS = 256;
constexpr int CX_TILE = 64;  // own rows per workgroup (16 per wave) and stream rows per step
constexpr int CX_MAX_D = 256;
constexpr int CX_MAX_SPLITS = 256;
enum { CX_FWD = 0, CX_DP = 1, CX_DT = 2 };

// scratch layout in 4-byte words (mirrored by ops.catalogue_xent_plan)
struct CxLayout {
  int64_t ridx, rpos, nv, part, part2, total;
};
CxLayout cx_layout(const CarcaCatalogueXentDesc& D, bool bwd) {
  CxLayout L;
  const int64_t R = D.R, ldo = (D.d + 3) / 4 * 4;
  L.ridx = 0;
  L.rpos = cx_r64(R);
  L.nv = 2 * cx_r64(R);
  L.part = L.nv + 64;
  if (!bwd) {  // (max, sum-exp) per split and valid row
    L.part2 = L.part + cx_r64((int64_t)D.splits_items * R);
    L.total = L.part2 + cx_r64((int64_t)D.splits_items * R);
  } else {  // dP partials [splits_items][R][ldo], then dT partials [splits_rows][n_items][ldo] when splits_rows > 1
    L.part2 = L.part + cx_r64((int64_t)D.splits_items * R * ldo);
    L.total = L.part2 + (D.splits_rows > 1 ? cx_r64((int64_t)D.splits_rows * D.n_items * ldo) : 0);
  }
  return L;
}

// ---- 1. valid rows, in row order: cx_compact_kernel (catalogue_xent_common.h) ------------------------------------

// ---- 2. logit tiles ------------------------------------------------------------------------------------------------
struct CxTile {
  int R, n_items, d, ld_p, ld_t;
  const float* P;
  const float* T;
  const int32_t* pos;
  const int32_t* ridx;
  const int32_t* nv;
  const float* lse;   // backward: per original row
  const float* grad;  // backward: upstream scale [1]
  int splits;         // FWD / DP: item splits; DT: row splits
  int per_split;      // FWD / DP: items per split (a multiple of CX_TILE)
  int pitch;          // LDS row pitch in floats
  float* part_m;      // FWD: [splits][R]
  float* part_s;
  float* out;         // DP: [splits][R][ld_out] by valid-row index; DT: [splits][n_items][ld_out], or dT itself
  int64_t out_split_stride;
  int ld_out;
  int final_out;      // DT with one split: scale by grad / n_valid and write zeros past d (out = dT)
};

template <int MODE>
__device__ __forceinline__ void cx_stage(const CxTile& A, float* dst, int first, int end, bool rows, int kpad, int tid) {
  // rows: entries first .. end-1 are valid-row indices (P[ridx[v]]); else item ids (T[i]).  Zero past `end` and past d.
  const int nc4 = kpad / 4;
  for (int idx = tid; idx < CX_TILE * nc4; idx += CX_THREADS) {
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
__global__ __launch_bounds__(CX_THREADS) void cx_tile_kernel(CxTile A) {
  extern __shared__ float cx_lds[];
  float* own = cx_lds;
  float* str = cx_lds + CX_TILE * A.pitch;
  float* s_lse = str + CX_TILE * A.pitch;                       // DT: lse of the stream rows
  int* s_pos = reinterpret_cast<int*>(s_lse + CX_TILE);         // DT: pos of the stream rows
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16), nkg = kpad / 16;
  const int own0 = blockIdx.x * CX_TILE, split = blockIdx.y;
  int s_begin, s_end;
  if constexpr (MODE != CX_DT) {
    if (own0 >= nv) return;  // (grid sized for R; rows past n_valid have nothing to do)
    s_begin = split * A.per_split;
    s_end = min(s_begin + A.per_split, A.n_items);
  } else {
    const int nb = (nv + CX_TILE - 1) / CX_TILE;
    s_begin = (int)((long long)split * nb / A.splits) * CX_TILE;
    s_end = min((int)((long long)(split + 1) * nb / A.splits) * CX_TILE, nv);
  }
  constexpr bool OWN_ROWS = MODE != CX_DT;
  cx_stage<MODE>(A, own, own0, OWN_ROWS ? nv : A.n_items, OWN_ROWS, kpad, tid);

  // this lane's own entry (column r16 of the wave's Z^T tiles)
  const int o_idx = own0 + 16 * w + r16;
  float o_lse = 0.f;
  int o_pos = -1;
  if constexpr (MODE == CX_DP) {
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
  const int ncb = (A.d + 15) / 16;
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += CX_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    cx_stage<MODE>(A, str, s0, s_end, !OWN_ROWS, kpad, tid);
    if constexpr (MODE == CX_DT) {
      if (tid < CX_TILE) {
        const int v = s0 + tid;
        const int r = v < s_end ? A.ridx[v] : 0;
        s_lse[tid] = v < s_end ? A.lse[r] : 0.f;
        s_pos[tid] = v < s_end ? A.pos[r] : -1;
      }
    }
    __syncthreads();
    // Z^T[stream 16n + 4q + reg][own r16] for the four 16-row stream blocks n
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
    if constexpr (MODE == CX_FWD) {
      // items s0 + 16n + 4q + reg of own row r16: id 0 and ids past the split are not classes
      float cm = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int it = s0 + 16 * n + 4 * q + j;
          if (it >= 1 && it < s_end) cm = fmaxf(cm, z[n][j]);
        }
      if (cm > -INFINITY) {
        const float mn = fmaxf(run_m, cm);
        float s = run_m > -INFINITY ? run_s * __expf(run_m - mn) : 0.f;
#pragma unroll
        for (int n = 0; n < 4; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int it = s0 + 16 * n + 4 * q + j;
            if (it >= 1 && it < s_end) s += __expf(z[n][j] - mn);
          }
        run_m = mn;
        run_s = s;
      }
    } else {
      // G[own r16][stream 16n + 4q + j] = softmax - onehot (0 outside the valid rows / classes)
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int si = s0 + 16 * n + 4 * q + j;
          float g = 0.f;
          if constexpr (MODE == CX_DP) {
            if (o_idx < nv && si >= 1 && si < s_end) g = __expf(z[n][j] - o_lse) - (si == o_pos ? 1.f : 0.f);
          } else {
            const int sl = 16 * n + 4 * q + j;
            if (si < s_end && o_idx >= 1 && o_idx < A.n_items)
              g = __expf(z[n][j] - s_lse[sl]) - (s_pos[sl] == o_idx ? 1.f : 0.f);
          }
          z[n][j] = g;
        }
      // out[own r16][col 16c + l&15] += sum over the 64 stream rows of G * S  (k = stream 16n + 4q + j at step j)
#pragma unroll
      for (int c = 0; c < NCB; ++c) {
        if (c < ncb) {
#pragma unroll
          for (int n = 0; n < 4; ++n)
#pragma unroll
            for (int j = 0; j < 4; ++j)
              acc[c] = mfma16(z[n][j], str[(16 * n + 4 * q + j) * A.pitch + 16 * c + r16], acc[c]);
        }
      }
    }
  }

  if constexpr (MODE == CX_FWD) {
    // merge the four lanes of own row r16 (lanes r16 + 16q); max and + are commutative, so every lane gets the same bits
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
  } else {
    // D of acc[c]: column 16c + r16, own rows 16w + 4q + j
    float* out = A.out + (size_t)split * A.out_split_stride;
    float coef = 1.f;
    if constexpr (MODE == CX_DT) {
      if (A.final_out) coef = nv > 0 ? A.grad[0] / (float)nv : 0.f;
    }
    const int own_end = MODE == CX_DP ? nv : A.n_items;
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
      if (c < ncb) {
        const int col = 16 * c + r16;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int e = own0 + 16 * w + 4 * q + j;
          if (e < own_end && col < A.ld_out) out[(size_t)e * A.ld_out + col] = col < A.d ? acc[c][j] * coef : 0.f;
        }
      }
    }
    if (MODE == CX_DT && A.final_out) {  // columns past the 16-column blocks, up to the row stride
      for (int col = 16 * ncb + lane; col < A.ld_out; col += 64)
        for (int j = 0; j < 16; ++j) {
          const int e = own0 + 16 * w + j;
          if (e < A.n_items) out[(size_t)e * A.ld_out + col] = 0.f;
        }
    }
  }
}

// ---- 3. merges (cx_mean_kernel and cx_reduce_kernel: catalogue_xent_common.h) -------------------------------------------------------------------------------------------------
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
int cx_check(const CarcaCatalogueXentDesc& D, const char* what, bool bwd) {
  CARCA_CHECK_ARG(D.R >= 1 && D.n_items >= 1 && D.d >= 1, "%s: R, n_items and d must be positive", what);
  CARCA_CHECK_SUPPORTED(D.d <= CX_MAX_D, "%s: d = %d exceeds %d", what, D.d, CX_MAX_D);
  CARCA_CHECK_ARG(D.P && D.T && D.pos && D.scratch, "%s: null P, T, pos or scratch", what);
  CARCA_CHECK_ARG(D.ld_p >= D.d && D.ld_p % 4 == 0 && D.ld_t >= D.d && D.ld_t % 4 == 0,
                  "%s: ld_p and ld_t must be multiples of 4, at least d", what);
  CARCA_CHECK_ARG(((uintptr_t)D.P & 15) == 0 && ((uintptr_t)D.T & 15) == 0, "%s: P and T must be 16-byte aligned", what);
  CARCA_CHECK_ARG(D.splits_items >= 1 && D.splits_items <= CX_MAX_SPLITS && D.splits_rows >= 1 &&
                      D.splits_rows <= CX_MAX_SPLITS,
                  "%s: split counts outside 1..%d", what, CX_MAX_SPLITS);
  CARCA_CHECK_ARG(D.items_per_split >= 1 && D.items_per_split % CX_TILE == 0 &&
                      (int64_t)D.items_per_split * D.splits_items >= D.n_items,
                  "%s: items_per_split must be a multiple of %d covering n_items in splits_items splits", what, CX_TILE);
  CARCA_CHECK_SUPPORTED((int64_t)D.n_items * D.ld_t < (1ll << 40) && (int64_t)D.R * D.ld_p < (1ll << 40),
                        "%s: operands too large", what);
  const CxLayout L = cx_layout(D, bwd);
  CARCA_CHECK_ARG(D.scratch_floats >= L.total, "%s: scratch of %lld floats, %lld needed", what,
                  (long long)D.scratch_floats, (long long)L.total);
  CARCA_CHECK_ARG(D.lse, "%s: null lse", what);
  if (!bwd) {
    CARCA_CHECK_ARG(D.row_loss && D.loss, "%s: null row_loss or loss", what);
  } else {
    CARCA_CHECK_ARG(D.grad && D.dP && D.dT, "%s: null grad, dP or dT", what);
  }
  return CARCA_OK;
}

template <int MODE>
int cx_launch_tile(const CxTile& A, dim3 grid, hipStream_t stream) {
  const size_t lds = (size_t)2 * CX_TILE * A.pitch * sizeof(float) + CX_TILE * (sizeof(float) + sizeof(int));
  auto pick = [&](auto kern) -> int {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      carca_set_error("catalogue_xent: cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
      return (int)e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(CX_THREADS), lds, stream, A);
    CARCA_LAUNCH_CHECK();
    return CARCA_OK;
  };
  if (A.d <= 64) return pick(cx_tile_kernel<MODE, 4>);
  if (A.d <= 128) return pick(cx_tile_kernel<MODE, 8>);
  return pick(cx_tile_kernel<MODE, 16>);
}

CxTile cx_tile_args(const CarcaCatalogueXentDesc& D, const CxLayout& L) {
  CxTile A = {};
  A.R = D.R, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_t = D.ld_t;
  A.P = D.P, A.T = D.T, A.pos = D.pos;
  int32_t* base = reinterpret_cast<int32_t*>(D.scratch);
  A.ridx = base + L.ridx, A.nv = base + L.nv;
  A.lse = D.lse, A.grad = D.grad;
  A.per_split = D.items_per_split;
  A.pitch = round_up(D.d, 16) + 4;  // (+4 floats: the 16 rows of a 16-byte LDS read start 4 banks apart)
  return A;
}

int cx_compact(const CarcaCatalogueXentDesc& D, const CxLayout& L, hipStream_t stream) {
  int32_t* base = reinterpret_cast<int32_t*>(D.scratch);
  hipLaunchKernelGGL(cx_compact_kernel, dim3(1), dim3(CX_COMPACT_THREADS), 0, stream, D.pos, D.R, D.n_items,
                     base + L.ridx, base + L.rpos, base + L.nv);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_catalogue_xent_fwd(const CarcaCatalogueXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "catalogue_xent_fwd: null descriptor");
  const CarcaCatalogueXentDesc& D = *desc;
  int rc = cx_check(D, "catalogue_xent_fwd", false);
  if (rc != CARCA_OK) return rc;
  const CxLayout L = cx_layout(D, false);
  if ((rc = cx_compact(D, L, stream)) != CARCA_OK) return rc;
  CxTile A = cx_tile_args(D, L);
  A.splits = D.splits_items;
  A.part_m = D.scratch + L.part;
  A.part_s = D.scratch + L.part2;
  const dim3 grid((D.R + CX_TILE - 1) / CX_TILE, D.splits_items);
  if ((rc = cx_launch_tile<CX_FWD>(A, grid, stream)) != CARCA_OK) return rc;
  hipLaunchKernelGGL(cx_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D,
                     reinterpret_cast<const int32_t*>(D.scratch) + L.rpos, A.part_m, A.part_s);
  CARCA_LAUNCH_CHECK();
  hipLaunchKernelGGL(cx_mean_kernel, dim3(1), dim3(1024), 0, stream, D, A.nv);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_catalogue_xent_bwd(const CarcaCatalogueXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "catalogue_xent_bwd: null descriptor");
  const CarcaCatalogueXentDesc& D = *desc;
  int rc = cx_check(D, "catalogue_xent_bwd", true);
  if (rc != CARCA_OK) return rc;
  const CxLayout L = cx_layout(D, true);
  if ((rc = cx_compact(D, L, stream)) != CARCA_OK) return rc;
  const int ldo = (D.d + 3) / 4 * 4;
  const int32_t* rpos = reinterpret_cast<const int32_t*>(D.scratch) + L.rpos;
  // dP: partials per item split, summed per original row (padding rows: 0)
  CxTile A = cx_tile_args(D, L);
  A.splits = D.splits_items;
  A.out = D.scratch + L.part, A.out_split_stride = (int64_t)D.R * ldo, A.ld_out = ldo;
  if ((rc = cx_launch_tile<CX_DP>(A, dim3((D.R + CX_TILE - 1) / CX_TILE, D.splits_items), stream)) != CARCA_OK) return rc;
  const int64_t np = (int64_t)D.R * D.ld_p;
  hipLaunchKernelGGL(cx_reduce_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, A.out,
                     A.out_split_stride, D.splits_items, ldo, rpos, D.R, D.d, D.dP, D.ld_p, A.nv, D.grad);
  CARCA_LAUNCH_CHECK();
  // dT: one row split writes dT itself, more write partials summed per item
  CxTile B = cx_tile_args(D, L);
  B.splits = D.splits_rows;
  if (D.splits_rows == 1) {
    B.out = D.dT, B.out_split_stride = 0, B.ld_out = D.ld_t, B.final_out = 1;
  } else {
    B.out = D.scratch + L.part2, B.out_split_stride = (int64_t)D.n_items * ldo, B.ld_out = ldo;
  }
  if ((rc = cx_launch_tile<CX_DT>(B, dim3((D.n_items + CX_TILE - 1) / CX_TILE, D.splits_rows), stream)) != CARCA_OK)
    return rc;
  if (D.splits_rows > 1) {
    const int64_t nt = (int64_t)D.n_items * D.ld_t;
    hipLaunchKernelGGL(cx_reduce_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, stream, B.out,
                       B.out_split_stride, D.splits_rows, ldo, (const int32_t*)nullptr, D.n_items, D.d, D.dT, D.ld_t,
                       B.nv, D.grad);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}
