// Sampled softmax cross-entropy with the logQ correction for the dot decoders (include/carca_hip.h:
// carca_sampled_xent_fwd / _bwd).
//
//   z'(r, k) = P[r] . S[k] + bs[k],   z'(r, +) = P[r] . Tp[r] + bp[r]      (bs, bp = -log(K Q(id)): the logQ correction)
//   CE = sum over valid rows r of ( logsumexp( {z'(r, +)} U {z'(r, k) : k in N_r} ) - z'(r, +) ) / n_valid
//   N_r = { k : s_ids[k] in [1, n_items) and s_ids[k] != pos[r] }   (accidental hits and invalid ids removed)
//
// with no [R, K] buffer.  The structure is catalogue_xent.hip's, with the K samples in place of the catalogue:
//   1. compact (cx_compact_kernel, catalogue_xent_common.h): the valid rows (pos in [1, n_items)) in row order;
//   2. tile: a workgroup owns 64 rows of one operand (staged once in LDS) and streams 64-row tiles of the other.  Each
//      of its four waves computes the 64 x 16 logit tile Z^T = S O^T on v_mfma_f32_16x16x4_f32 (exact fp32 products);
//      its D layout is the A operand of the second product, so G never leaves the registers.  The next stream tile's
//      loads are issued before the current one's products and read back only when it is written to LDS after the next
//      barrier (masked there); DS, whose stream rows are gathered through ridx, loads those indices one tile ahead:
//        FWD  own = valid rows, stream = the samples of one split: running (max, sum-exp) per (split, row);
//        DP   own = valid rows, stream = samples: partial dP[split][v] = sum over the split's samples of G S;
//        DS   own = samples, stream = the valid rows of one split: dS[k] (or its partial) = sum over rows of G^T P;
//      G = exp(z' - lse), 0 where masked (accidental hits, invalid ids, padding);
//   3. FWD: the split partials merged in split order, then the positive term; lse, row loss; the fp64 mean
//      (cx_mean_kernel).  BWD: the positive term (p_pos - 1) Tp[r] is written as one more dP partial after the splits,
//      and dTp[r] = grad / n_valid (p_pos - 1) P[r]; cx_reduce_kernel sums the partials in split order.
// No float atomics: every sum has one fixed order, so two calls give the same bits.
#include "catalogue_xent_common.h"

#include <math.h>

namespace {

constexpr int SX_THREADS = 256;
constexpr int SX_TILE = 64;  // own rows per workgroup (16 per wave) and stream rows per step
constexpr int SX_MAX_D = 256;
constexpr int SX_MAX_SPLITS = 256;
enum { SX_FWD = 0, SX_DP = 1, SX_DS = 2 };
constexpr int SX_WAIT_VM0 = 0x0F70;  // s_waitcnt vmcnt(0) expcnt(7) lgkmcnt(15): wait for the vector memory loads only

// scratch layout in 4-byte words (mirrored by ops.sampled_xent_plan)
struct SxLayout {
  int64_t ridx, rpos, nv, part, part2, total;
};
SxLayout sx_layout(const CarcaSampledXentDesc& D, bool bwd) {
  SxLayout L;
  const int64_t R = D.R, ldo = (D.d + 3) / 4 * 4;
  L.ridx = 0;
  L.rpos = cx_r64(R);
  L.nv = 2 * cx_r64(R);
  L.part = L.nv + 64;
  if (!bwd) {  // (max, sum-exp) per split and valid row
    L.part2 = L.part + cx_r64((int64_t)D.splits_samples * R);
    L.total = L.part2 + cx_r64((int64_t)D.splits_samples * R);
  } else {  // dP partials [splits_samples + 1][R][ldo] (the last: the positive term), dS partials [splits_rows][K][ldo]
    L.part2 = L.part + cx_r64((int64_t)(D.splits_samples + 1) * R * ldo);
    L.total = L.part2 + (D.splits_rows > 1 ? cx_r64((int64_t)D.splits_rows * D.K * ldo) : 0);
  }
  return L;
}

// ---- 2. logit tiles ------------------------------------------------------------------------------------------------
struct SxTile {
  int R, K, n_items, d, ld_p, ld_s;
  const float* P;
  const float* S;
  const int32_t* pos;
  const int32_t* s_ids;
  const float* bs;
  const int32_t* ridx;
  const int32_t* nv;
  const float* lse;   // backward: per original row
  const float* grad;  // backward: upstream scale [1]
  int splits;         // FWD / DP: sample splits; DS: row splits
  int per_split;      // FWD / DP: samples per split (a multiple of SX_TILE)
  int pitch;          // LDS row pitch in floats
  float* part_m;      // FWD: [splits][R]
  float* part_s;
  float* out;         // DP: [splits][R][ld_out] by valid-row index; DS: [splits][K][ld_out], or dS itself
  int64_t out_split_stride;
  int ld_out;
  int final_out;      // DS with one split: scale by grad / n_valid and write zeros past d (out = dS)
};

// A 64-row tile in registers: this thread's NCB 16-byte pieces (64 rows x round_up(d, 16) columns over 256 threads is
// round_up(d, 16) / 16 <= NCB pieces); piece i is tile row (tid + 256 i) / nc4, columns 4 ((tid + 256 i) % nc4) + 0..3.
// The loads read nothing back: each piece's operand row comes from sx_rows (clamped to the tile's last entry) and its
// column is clamped to the row's last 16 bytes (ld % 4 == 0 and ld >= d), and sx_store zeroes the rows past the tile's
// end and the columns past d when it writes the tile to LDS.  So the next stream tile's loads stay in flight while the
// current tile multiplies.
template <int NCB>
__device__ __forceinline__ void sx_issue(const float* base, int ld, const int (&src)[NCB], f32x4 (&v)[NCB], int nc4, int d4,
                                         int tid) {
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int idx = tid + SX_THREADS * i;
    const int row = idx / nc4, c = min(4 * (idx - row * nc4), d4 - 4);
    // (idx < 64 nc4 iff i < nc4 / 4: a wave-uniform branch, no exec mask around the load)
    if (i < nc4 / 4) v[i] = *reinterpret_cast<const f32x4*>(base + (size_t)src[i] * ld + c);
  }
}

// the operand row of each piece of the tile of entries first .. first+63 (entries past `end` clamped to end - 1; end >
// first): the sample index itself, or, with rows, the valid row ridx[entry] (a global load)
template <int NCB>
__device__ __forceinline__ void sx_rows(const SxTile& A, int (&src)[NCB], int first, int end, bool rows, int nc4, int tid) {
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int idx = tid + SX_THREADS * i;
    const int e = min(first + idx / nc4, end - 1);
    src[i] = e;
    if (rows && idx < SX_TILE * nc4) src[i] = A.ridx[e];
  }
}

template <int NCB>
__device__ __forceinline__ void sx_store(const SxTile& A, const f32x4 (&v)[NCB], float* dst, int first, int end, int nc4,
                                         int tid) {
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int idx = tid + SX_THREADS * i;
    const int row = idx / nc4, c = 4 * (idx - row * nc4);
    if (idx < SX_TILE * nc4) {
      f32x4 x = v[i];
      const bool live = first + row < end;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!live || c + j >= A.d) x[j] = 0.f;
      *reinterpret_cast<f32x4*>(dst + row * A.pitch + c) = x;
    }
  }
}

// the per-entry values of a stream tile (threads 0..63), masked when stored: FWD / DP: bs and id of the samples; DS: lse
// and pos of the valid rows, read through mrow = ridx[entry] (loaded one tile ahead)
template <int MODE>
__device__ __forceinline__ void sx_meta(const SxTile& A, int s0, int s_end, int mrow, int tid, float& f, int& id) {
  if (tid < SX_TILE) {
    if constexpr (MODE == SX_DS) {
      f = A.lse[mrow];
      id = A.pos[mrow];
    } else {
      const int e = min(s0 + tid, s_end - 1);
      f = A.bs[e];
      id = A.s_ids[e];
    }
  }
}

// NCB: 16-column blocks the kernel is built for (d <= 16 NCB)
template <int MODE, int NCB>
__global__ __launch_bounds__(SX_THREADS) void sx_tile_kernel(SxTile A) {
  extern __shared__ float sx_lds[];
  float* own = sx_lds;
  float* str = sx_lds + SX_TILE * A.pitch;
  float* s_f = str + SX_TILE * A.pitch;                // FWD / DP: bs of the stream samples; DS: lse of the stream rows
  int* s_id = reinterpret_cast<int*>(s_f + SX_TILE);   // FWD / DP: ids of the stream samples; DS: pos of the stream rows
  const int tid = threadIdx.x, lane = tid & 63, r16 = lane & 15, q = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nv = A.nv[0];
  const int kpad = round_up(A.d, 16), nkg = kpad / 16, nc4 = kpad / 4;
  const int own0 = blockIdx.x * SX_TILE, split = blockIdx.y;
  int s_begin, s_end;
  if constexpr (MODE != SX_DS) {
    if (own0 >= nv) return;  // (grid sized for R; rows past n_valid have nothing to do)
    s_begin = split * A.per_split;
    s_end = min(s_begin + A.per_split, A.K);
  } else {
    const int nb = (nv + SX_TILE - 1) / SX_TILE;
    s_begin = (int)((long long)split * nb / A.splits) * SX_TILE;
    s_end = min((int)((long long)(split + 1) * nb / A.splits) * SX_TILE, nv);
  }
  constexpr bool OWN_ROWS = MODE != SX_DS;
  const int d4 = (A.d + 3) / 4 * 4;
  const float* sbase = OWN_ROWS ? A.S : A.P;  // the streamed operand
  const int sld = OWN_ROWS ? A.ld_s : A.ld_p;
  f32x4 pre[NCB];  // the stream tile in flight
  int src[NCB];    // its pieces' operand rows
  {
    const int own_end = OWN_ROWS ? nv : A.K;
    sx_rows<NCB>(A, src, own0, own_end, OWN_ROWS, nc4, tid);
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);  // (the row indices, once: then the pieces' loads go out back to back)
    sx_issue<NCB>(OWN_ROWS ? A.P : A.S, OWN_ROWS ? A.ld_p : A.ld_s, src, pre, nc4, d4, tid);
    sx_store<NCB>(A, pre, own, own0, own_end, nc4, tid);
  }
  float pre_f = 0.f;
  int pre_id = 0, mrow = 0;
  if (s_begin < s_end) {
    sx_rows<NCB>(A, src, s_begin, s_end, !OWN_ROWS, nc4, tid);
    if constexpr (MODE == SX_DS) mrow = tid < SX_TILE ? A.ridx[min(s_begin + tid, s_end - 1)] : 0;
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);
    sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
    sx_meta<MODE>(A, s_begin, s_end, mrow, tid, pre_f, pre_id);
    if constexpr (MODE == SX_DS) {  // the row indices one tile ahead
      if (s_begin + SX_TILE < s_end) {
        sx_rows<NCB>(A, src, s_begin + SX_TILE, s_end, true, nc4, tid);
        mrow = tid < SX_TILE ? A.ridx[min(s_begin + SX_TILE + tid, s_end - 1)] : 0;
      }
    }
  }

  // this lane's own entry (column r16 of the wave's Z^T tiles)
  const int o_idx = own0 + 16 * w + r16;
  float o_f = 0.f;  // DP: lse of the own row; DS: bs of the own sample
  int o_id = -1;    // FWD / DP: pos of the own row; DS: id of the own sample
  bool o_ok = false;
  if constexpr (MODE != SX_DS) {
    if (o_idx < nv) {
      const int r = A.ridx[o_idx];
      o_id = A.pos[r];
      if constexpr (MODE == SX_DP) o_f = A.lse[r];
      o_ok = true;
    }
  } else {
    if (o_idx < A.K) {
      o_id = A.s_ids[o_idx];
      o_f = A.bs[o_idx];
      o_ok = o_id >= 1 && o_id < A.n_items;
    }
  }
  float run_m = -INFINITY, run_s = 0.f;  // FWD
  f32x4 acc[NCB];
#pragma unroll
  for (int c = 0; c < NCB; ++c) acc[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int ncb = (A.d + 15) / 16;
  const float* own_row = own + (16 * w + r16) * A.pitch + 4 * q;

  for (int s0 = s_begin; s0 < s_end; s0 += SX_TILE) {
    __syncthreads();  // (the previous step's readers of `str` are done)
    // Every load in flight lands here, on every path: without this wait the compiler, which sees the pieces' loads and
    // stores under branches, assumes some may still be pending and waits for them again between the next tile's loads.
    __builtin_amdgcn_s_waitcnt(SX_WAIT_VM0);
    sx_store<NCB>(A, pre, str, s0, s_end, nc4, tid);
    if (tid < SX_TILE) {
      const bool live = s0 + tid < s_end;
      s_f[tid] = live ? pre_f : 0.f;
      s_id[tid] = live ? pre_id : (MODE == SX_DS ? -1 : 0);  // (id 0: never a class)
    }
    __syncthreads();
    if (s0 + SX_TILE < s_end) {  // the next tile's loads: in flight while this tile multiplies
      if constexpr (MODE != SX_DS) sx_rows<NCB>(A, src, s0 + SX_TILE, s_end, false, nc4, tid);
      sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
      sx_meta<MODE>(A, s0 + SX_TILE, s_end, mrow, tid, pre_f, pre_id);
      if constexpr (MODE == SX_DS) {  // the row indices of the tile after it
        if (s0 + 2 * SX_TILE < s_end) {
          sx_rows<NCB>(A, src, s0 + 2 * SX_TILE, s_end, true, nc4, tid);
          mrow = tid < SX_TILE ? A.ridx[min(s0 + 2 * SX_TILE + tid, s_end - 1)] : 0;
        }
      }
    }
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
    if constexpr (MODE == SX_FWD) {
      // the corrected logits of own row r16 against samples s0 + 16n + 4q + j; -inf where masked
      float cm = -INFINITY;
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int sl = 16 * n + 4 * q + j, sid = s_id[sl];
          const bool ok = sid >= 1 && sid < A.n_items && sid != o_id;
          z[n][j] = ok ? z[n][j] + s_f[sl] : -INFINITY;
          cm = fmaxf(cm, z[n][j]);
        }
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
    } else {
      // G[own r16][stream 16n + 4q + j] = exp(z' - lse), 0 where masked
#pragma unroll
      for (int n = 0; n < 4; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int sl = 16 * n + 4 * q + j;
          float g = 0.f;
          if constexpr (MODE == SX_DP) {
            const int sid = s_id[sl];
            if (o_ok && sid >= 1 && sid < A.n_items && sid != o_id) g = __expf(z[n][j] + s_f[sl] - o_f);
          } else {
            if (o_ok && s0 + sl < s_end && s_id[sl] != o_id) g = __expf(z[n][j] + o_f - s_f[sl]);
          }
          z[n][j] = g;
        }
      // out[own r16][col 16c + l&15] += sum over the 64 stream rows of G * stream  (k = stream 16n + 4q + j at step j)
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

  if constexpr (MODE == SX_FWD) {
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
    if constexpr (MODE == SX_DS) {
      if (A.final_out) coef = nv > 0 ? A.grad[0] / (float)nv : 0.f;
    }
    const int own_end = MODE == SX_DP ? nv : A.K;
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
    if (MODE == SX_DS && A.final_out) {  // columns past the 16-column blocks, up to the row stride
      for (int col = 16 * ncb + lane; col < A.ld_out; col += 64)
        for (int j = 0; j < 16; ++j) {
          const int e = own0 + 16 * w + j;
          if (e < A.K) out[(size_t)e * A.ld_out + col] = 0.f;
        }
    }
  }
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
int sx_check(const CarcaSampledXentDesc& D, const char* what, bool bwd) {
  CARCA_CHECK_ARG(D.R >= 1 && D.K >= 1 && D.n_items >= 1 && D.d >= 1, "%s: R, K, n_items and d must be positive", what);
  CARCA_CHECK_SUPPORTED(D.d <= SX_MAX_D, "%s: d = %d exceeds %d", what, D.d, SX_MAX_D);
  CARCA_CHECK_ARG(D.P && D.Tp && D.bp && D.pos && D.S && D.s_ids && D.bs && D.scratch,
                  "%s: null P, Tp, bp, pos, S, s_ids, bs or scratch", what);
  CARCA_CHECK_ARG(D.ld_p >= D.d && D.ld_p % 4 == 0 && D.ld_tp >= D.d && D.ld_tp % 4 == 0 && D.ld_s >= D.d &&
                      D.ld_s % 4 == 0,
                  "%s: ld_p, ld_tp and ld_s must be multiples of 4, at least d", what);
  CARCA_CHECK_ARG(((uintptr_t)D.P & 15) == 0 && ((uintptr_t)D.S & 15) == 0, "%s: P and S must be 16-byte aligned", what);
  CARCA_CHECK_ARG(D.splits_samples >= 1 && D.splits_samples <= SX_MAX_SPLITS && D.splits_rows >= 1 &&
                      D.splits_rows <= SX_MAX_SPLITS,
                  "%s: split counts outside 1..%d", what, SX_MAX_SPLITS);
  CARCA_CHECK_ARG(D.samples_per_split >= 1 && D.samples_per_split % SX_TILE == 0 &&
                      (int64_t)D.samples_per_split * D.splits_samples >= D.K,
                  "%s: samples_per_split must be a multiple of %d covering K in splits_samples splits", what, SX_TILE);
  CARCA_CHECK_SUPPORTED((int64_t)D.K * D.ld_s < (1ll << 40) && (int64_t)D.R * D.ld_p < (1ll << 40) &&
                            (int64_t)D.R * D.ld_tp < (1ll << 40),
                        "%s: operands too large", what);
  const SxLayout L = sx_layout(D, bwd);
  CARCA_CHECK_ARG(D.scratch_floats >= L.total, "%s: scratch of %lld floats, %lld needed", what,
                  (long long)D.scratch_floats, (long long)L.total);
  CARCA_CHECK_ARG(D.lse && D.row_loss, "%s: null lse or row_loss", what);
  if (!bwd) {
    CARCA_CHECK_ARG(D.loss, "%s: null loss", what);
  } else {
    CARCA_CHECK_ARG(D.grad && D.dP && D.dTp && D.dS, "%s: null grad, dP, dTp or dS", what);
  }
  return CARCA_OK;
}

template <int MODE>
int sx_launch_tile(const SxTile& A, dim3 grid, hipStream_t stream) {
  const size_t lds = (size_t)2 * SX_TILE * A.pitch * sizeof(float) + SX_TILE * (sizeof(float) + sizeof(int));
  auto pick = [&](auto kern) -> int {
    hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) {
      carca_set_error("sampled_xent: cannot reserve %zu B of LDS: %s", lds, hipGetErrorString(e));
      return (int)e;
    }
    hipLaunchKernelGGL(kern, grid, dim3(SX_THREADS), lds, stream, A);
    CARCA_LAUNCH_CHECK();
    return CARCA_OK;
  };
  if (A.d <= 64) return pick(sx_tile_kernel<MODE, 4>);
  if (A.d <= 128) return pick(sx_tile_kernel<MODE, 8>);
  return pick(sx_tile_kernel<MODE, 16>);
}

SxTile sx_tile_args(const CarcaSampledXentDesc& D, const SxLayout& L) {
  SxTile A = {};
  A.R = D.R, A.K = D.K, A.n_items = D.n_items, A.d = D.d, A.ld_p = D.ld_p, A.ld_s = D.ld_s;
  A.P = D.P, A.S = D.S, A.pos = D.pos, A.s_ids = D.s_ids, A.bs = D.bs;
  int32_t* base = reinterpret_cast<int32_t*>(D.scratch);
  A.ridx = base + L.ridx, A.nv = base + L.nv;
  A.lse = D.lse, A.grad = D.grad;
  A.per_split = D.samples_per_split;
  A.pitch = round_up(D.d, 16) + 4;  // (+4 floats: the 16 rows of a 16-byte LDS read start 4 banks apart)
  return A;
}

int sx_compact(const CarcaSampledXentDesc& D, const SxLayout& L, hipStream_t stream) {
  int32_t* base = reinterpret_cast<int32_t*>(D.scratch);
  hipLaunchKernelGGL(cx_compact_kernel, dim3(1), dim3(CX_COMPACT_THREADS), 0, stream, D.pos, D.R, D.n_items,
                     base + L.ridx, base + L.rpos, base + L.nv);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_sampled_xent_fwd(const CarcaSampledXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "sampled_xent_fwd: null descriptor");
  const CarcaSampledXentDesc& D = *desc;
  int rc = sx_check(D, "sampled_xent_fwd", false);
  if (rc != CARCA_OK) return rc;
  const SxLayout L = sx_layout(D, false);
  if ((rc = sx_compact(D, L, stream)) != CARCA_OK) return rc;
  SxTile A = sx_tile_args(D, L);
  A.splits = D.splits_samples;
  A.part_m = D.scratch + L.part;
  A.part_s = D.scratch + L.part2;
  const dim3 grid((D.R + SX_TILE - 1) / SX_TILE, D.splits_samples);
  if ((rc = sx_launch_tile<SX_FWD>(A, grid, stream)) != CARCA_OK) return rc;
  hipLaunchKernelGGL(sx_merge_kernel, dim3((D.R + 255) / 256), dim3(256), 0, stream, D,
                     reinterpret_cast<const int32_t*>(D.scratch) + L.rpos, A.part_m, A.part_s);
  CARCA_LAUNCH_CHECK();
  CarcaCatalogueXentDesc M = {};  // (the fields cx_mean_kernel reads: R, row_loss, loss)
  M.R = D.R, M.row_loss = D.row_loss, M.loss = D.loss;
  hipLaunchKernelGGL(cx_mean_kernel, dim3(1), dim3(1024), 0, stream, M, A.nv);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_sampled_xent_bwd(const CarcaSampledXentDesc* desc, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  CARCA_CHECK_ARG(desc, "sampled_xent_bwd: null descriptor");
  const CarcaSampledXentDesc& D = *desc;
  int rc = sx_check(D, "sampled_xent_bwd", true);
  if (rc != CARCA_OK) return rc;
  const SxLayout L = sx_layout(D, true);
  if ((rc = sx_compact(D, L, stream)) != CARCA_OK) return rc;
  const int ldo = (D.d + 3) / 4 * 4;
  const int32_t* rpos = reinterpret_cast<const int32_t*>(D.scratch) + L.rpos;
  // dP: partials per sample split, then the positive term, summed per original row (padding rows: 0); dTp
  SxTile A = sx_tile_args(D, L);
  A.splits = D.splits_samples;
  A.out = D.scratch + L.part, A.out_split_stride = (int64_t)D.R * ldo, A.ld_out = ldo;
  if ((rc = sx_launch_tile<SX_DP>(A, dim3((D.R + SX_TILE - 1) / SX_TILE, D.splits_samples), stream)) != CARCA_OK)
    return rc;
  const int64_t ntp = (int64_t)D.R * D.ld_tp;
  hipLaunchKernelGGL(sx_positive_kernel, dim3((unsigned)((ntp + 255) / 256)), dim3(256), 0, stream, D, rpos, A.nv,
                     A.out + (size_t)D.splits_samples * A.out_split_stride, ldo);
  CARCA_LAUNCH_CHECK();
  const int64_t np = (int64_t)D.R * D.ld_p;
  hipLaunchKernelGGL(cx_reduce_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, A.out,
                     A.out_split_stride, D.splits_samples + 1, ldo, rpos, D.R, D.d, D.dP, D.ld_p, A.nv, D.grad);
  CARCA_LAUNCH_CHECK();
  // dS: one row split writes dS itself, more write partials summed per sample
  SxTile B = sx_tile_args(D, L);
  B.splits = D.splits_rows;
  if (D.splits_rows == 1) {
    B.out = D.dS, B.out_split_stride = 0, B.ld_out = D.ld_s, B.final_out = 1;
  } else {
    B.out = D.scratch + L.part2, B.out_split_stride = (int64_t)D.K * ldo, B.ld_out = ldo;
  }
  if ((rc = sx_launch_tile<SX_DS>(B, dim3((D.K + SX_TILE - 1) / SX_TILE, D.splits_rows), stream)) != CARCA_OK) return rc;
  if (D.splits_rows > 1) {
    const int64_t ns = (int64_t)D.K * D.ld_s;
    hipLaunchKernelGGL(cx_reduce_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, stream, B.out,
                       B.out_split_stride, D.splits_rows, ldo, (const int32_t*)nullptr, D.K, D.d, D.dS, D.ld_s, B.nv,
                       D.grad);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}
