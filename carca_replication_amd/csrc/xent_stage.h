// The staged tile kernel of the two losses over K shared samples: sampled_xent.hip (softmax with the logQ correction,
// DESIGN.md section 14) and sampled_bce.hip (gBCE, section 16).  What lives here, once:
//   the register staging: a 64-row tile of an operand is loaded into registers one step ahead and written to LDS, masked,
//     after the next barrier (sx_issue, sx_rows, sx_store);
//   xs_tile_kernel<RULE, MODE, NCB>: the LDS carve-up, the own tile, the prefetch of the next stream tile with its waits,
//     the lane's own entry, the mask tests, and xent_tile.h's two products and epilogue around them.
// A loss supplies a stateless rule struct (SxRule, SbRule) for the four places where the two differ: the per-entry float
// and id a stream tile carries (and whether the float is kept in LDS), the float of the lane's own entry, the forward's
// state with its per-logit step, per-tile step and partial store, and the value of G for an unmasked entry.  Each file
// keeps its rule, its pre-pass / merge / positive kernels and its entry points.
#pragma once
#include "xent_tile.h"

namespace {

constexpr int SX_WAIT_VM0 = 0x0F70;  // s_waitcnt vmcnt(0) expcnt(7) lgkmcnt(15): wait for the vector memory loads only

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
    const int idx = tid + XT_THREADS * i;
    const int row = idx / nc4, c = min(4 * (idx - row * nc4), d4 - 4);
    // (idx < 64 nc4 iff i < nc4 / 4: a wave-uniform branch, no exec mask around the load)
    if (i < nc4 / 4) v[i] = *reinterpret_cast<const f32x4*>(base + (size_t)src[i] * ld + c);
  }
}

// the operand row of each piece of the tile of entries first .. first+63 (entries past `end` clamped to end - 1; end >
// first): the sample index itself, or, with rows, the valid row ridx[entry] (a global load)
template <int NCB>
__device__ __forceinline__ void sx_rows(const XentTile& A, int (&src)[NCB], int first, int end, bool rows, int nc4, int tid) {
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int idx = tid + XT_THREADS * i;
    const int e = min(first + idx / nc4, end - 1);
    src[i] = e;
    if (rows && idx < XT_TILE * nc4) src[i] = A.ridx[e];
  }
}

template <int NCB>
__device__ __forceinline__ void sx_store(const XentTile& A, const f32x4 (&v)[NCB], float* dst, int first, int end, int nc4,
                                         int tid) {
#pragma unroll
  for (int i = 0; i < NCB; ++i) {
    const int idx = tid + XT_THREADS * i;
    const int row = idx / nc4, c = 4 * (idx - row * nc4);
    if (idx < XT_TILE * nc4) {
      f32x4 x = v[i];
      const bool live = first + row < end;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!live || c + j >= A.d) x[j] = 0.f;
      *reinterpret_cast<f32x4*>(dst + row * A.pitch + c) = x;
    }
  }
}

// ---- the tile kernel -------------------------------------------------------------------------------------------------
// RULE: all members static and __forceinline__ (MODE as a template argument where it matters)
//   keep_f(MODE)                           constexpr: whether the stream entries' float is kept in LDS (s_f) in this mode
//   meta<MODE>(A, s0, s_end, mrow, tid, f, id)   threads 0..63: the float and id of stream entry s0 + tid (clamped to
//                                          s_end - 1), masked when stored; DS reads them through mrow = ridx[entry]
//   own_f<MODE>(A, e)                      the float of the lane's own entry: e is the original row in FWD / DP, the sample
//                                          index in DS
//   Fwd                                    the lane's forward state, default-initialised
//   fwd_logit(ok, z, s_f, sl, o_f, run)    FWD: one logit against stream entry sl, ok where unmasked; returns the new z
//   fwd_tile(z, run)                       FWD: after a tile's 16 logits
//   fwd_store(A, run, split, o_idx, q, nv) FWD: the four-lane merge and the partial of (split, valid row o_idx)
//   g<MODE>(z, s_f, sl, o_f)               DP / DS: G of an unmasked entry
// (z goes in by value and comes back as the result: an element of an f32x4 does not bind to a reference.)
// NCB: 16-column blocks the kernel is built for (d <= 16 NCB)
template <class RULE, int MODE, int NCB>
__global__ __launch_bounds__(XT_THREADS) void xs_tile_kernel(XentTile A) {
  extern __shared__ float xs_lds[];
  float* own = xs_lds;
  float* str = xs_lds + XT_TILE * A.pitch;
  float* s_f = str + XT_TILE * A.pitch;                // the stream entries' float (RULE::meta), where the rule keeps it
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
    RULE::template meta<MODE>(A, s_begin, s_end, mrow, tid, pre_f, pre_id);
    if constexpr (MODE == XT_DT) {  // the row indices one tile ahead
      if (s_begin + XT_TILE < s_end) {
        sx_rows<NCB>(A, src, s_begin + XT_TILE, s_end, true, nc4, tid);
        mrow = tid < XT_TILE ? A.ridx[min(s_begin + XT_TILE + tid, s_end - 1)] : 0;
      }
    }
  }

  // this lane's own entry (column r16 of the wave's Z^T tiles)
  const int o_idx = own0 + 16 * w + r16;
  float o_f = 0.f;  // RULE::own_f
  int o_id = -1;    // FWD / DP: pos of the own row; DS: id of the own sample
  bool o_ok = false;
  if constexpr (MODE != XT_DT) {
    if (o_idx < nv) {
      const int r = A.ridx[o_idx];
      o_id = A.pos[r];
      o_f = RULE::template own_f<MODE>(A, r);
      o_ok = true;
    }
  } else {
    if (o_idx < A.n) {
      o_id = A.ids[o_idx];
      o_f = RULE::template own_f<MODE>(A, o_idx);
      o_ok = o_id >= 1 && o_id < A.n_items;
    }
  }
  typename RULE::Fwd run;  // FWD
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
      if constexpr (RULE::keep_f(MODE)) s_f[tid] = live ? pre_f : 0.f;
      s_id[tid] = live ? pre_id : (MODE == XT_DT ? -1 : 0);  // (id 0: never a class)
    }
    __syncthreads();
    if (s0 + XT_TILE < s_end) {  // the next tile's loads: in flight while this tile multiplies
      if constexpr (MODE != XT_DT) sx_rows<NCB>(A, src, s0 + XT_TILE, s_end, false, nc4, tid);
      sx_issue<NCB>(sbase, sld, src, pre, nc4, d4, tid);
      RULE::template meta<MODE>(A, s0 + XT_TILE, s_end, mrow, tid, pre_f, pre_id);
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
          // own row r16 against samples s0 + 16n + 4q + j; masked: accidental hits and invalid ids (padding: id 0)
          const int sid = s_id[sl];
          const bool ok = sid >= 1 && sid < A.n_items && sid != o_id;
          z[n][j] = RULE::fwd_logit(ok, z[n][j], s_f, sl, o_f, run);
        } else {
          // G[own r16][stream 16n + 4q + j], 0 where masked
          float g = 0.f;
          if constexpr (MODE == XT_DP) {
            const int sid = s_id[sl];
            if (o_ok && sid >= 1 && sid < A.n_items && sid != o_id) g = RULE::template g<MODE>(z[n][j], s_f, sl, o_f);
          } else {
            if (o_ok && s0 + sl < s_end && s_id[sl] != o_id) g = RULE::template g<MODE>(z[n][j], s_f, sl, o_f);
          }
          z[n][j] = g;
        }
      }
    if constexpr (MODE == XT_FWD) RULE::fwd_tile(z, run);
    else xt_accumulate<NCB>(A, z, str, r16, q, acc);
  }

  if constexpr (MODE == XT_FWD) RULE::fwd_store(A, run, split, o_idx, q, nv);
  else xt_epilogue<MODE, NCB>(A, acc, nv, own0, split, w, lane);
}

// the tile kernels of one rule and mode, as xent_direct.h's xd_kernels
#define XS_KERNELS(RULE, MODE) \
  (XentKernels{xs_tile_kernel<RULE, MODE, 4>, xs_tile_kernel<RULE, MODE, 8>, xs_tile_kernel<RULE, MODE, 16>})

}  // namespace
