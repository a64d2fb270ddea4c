// The 384-row one-block-per-CU tile of the row GEMM, once: what gemm.hip's cu_tile (gemm_rows_cu_kernel, gemm_rows_sk_kernel,
// gemm_rows_skc_kernel) and gemm_stream.hip's stream_tiles (gemm_rows_cus_kernel) share.  Include inside the translation
// unit, after carca_common.h and include/carca_hip.h.
//
// The tile: 384 rows x (32 TN + XC) columns, twelve waves, wave w owns rows 32 w .. 32 w + 31 x all columns as TN 32x32
// accumulator tiles (v_mfma_f32_32x32x2_f32) + XC <= 2 VALU columns; K step 32 = four 8-k groups; operands staged global ->
// registers -> LDS with rows padded to 36 floats, LDS double-buffered (ONE barrier per K step).  With a single lock-stepped
// block per CU nothing else covers a wave's non-MFMA instructions, so the step is scheduled by hand: every LDS read, LDS
// write and global load sits in the gap behind one of the wave's own MFMAs (mfma_group pins them there), fragments are
// double-buffered in registers one 8-k group ahead.  The step SCHEDULES stay with their kernels (what a gap carries differs:
// cu_tile's items are K tiles of one tile, stream_tiles' items have compile-time kinds and cross tile boundaries).
#pragma once
namespace {
namespace tile384 {

constexpr int BM = 384, BK = 32, LS = BK + 4, NT = 768, NW = 12, C4 = BK / 4;
constexpr int A_PER = BM * C4 / NT;  // 4 staged float4 of A per thread and K tile
constexpr int A_BUF = BM * LS;       // floats per LDS buffer of A
constexpr int b_cols(int TN, int XC) { return 32 * TN + XC; }
constexpr int b_buf(int TN, int XC) { return b_cols(TN, XC) * LS; }                  // floats per LDS buffer of B
constexpr int b_per(int TN, int XC) { return (b_cols(TN, XC) * C4 + NT - 1) / NT; }  // staged float4 of B per thread: 1 (TN = 4: 2)
// LDS of a kernel: both A buffers; both B buffers + the dummy strip behind them, where the threads without a live B slot
// store theirs (the pipelined body stays branch-free): the dead staging slots of a K tile, at least 256 for the context group
constexpr int AS_FLOATS = 2 * A_BUF;  // 27,648
constexpr int bs_floats(int TN, int XC = 0) {
  const int dead = (b_per(TN, XC) * NT - b_cols(TN, XC) * C4) * 4;
  return 2 * b_buf(TN, XC) + (dead > 1024 ? dead : 1024);
}
constexpr int BS_FLOATS = bs_floats(3);  // the 96-column kernels (their narrow last column block is smaller)

#define CARCA_PIN() __builtin_amdgcn_sched_barrier(0)

// ids that are equal mod 8 land on one XCD under round-robin placement: renumber them contiguously per XCD (bijective for
// any `total`) so that the workgroups that share an A row block share an L2.  (gemm_rows_skc_kernel keeps its own copy
// beside the share of the numbers that its XCD gets: with this function its code comes out different)
__device__ __forceinline__ int xcd_swizzle(const int id, const int total) {
  const int xcd = id & 7, q8 = total >> 3, r8 = total & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (id >> 3);
}

// the segment of row block rb (rb_start: row blocks in front of each segment)
__device__ __forceinline__ int seg_of(const CarcaGemmDesc& D, const int* rb_start, const int rb) {
  int s = 0;
#pragma unroll
  for (int i = 1; i < CARCA_MAX_SEGS; ++i)
    if (i < D.nseg && rb >= rb_start[i]) s = i;
  return s;
}

// four floats of a ragged K tile: element-wise under kk + e < klen unless the whole tile lies inside klen
__device__ __forceinline__ f32x4 load4(const float* p, bool full, int kk, int klen) {
  if (full) return *reinterpret_cast<const f32x4_u*>(p);
  f32x4 v;
  v[0] = kk + 0 < klen ? p[0] : 0.f;
  v[1] = kk + 1 < klen ? p[1] : 0.f;
  v[2] = kk + 2 < klen ? p[2] : 0.f;
  v[3] = kk + 3 < klen ? p[3] : 0.f;
  return v;
}

// The context columns (k-source 1, 4 <= K1 <= 8) as ONE 8-k group: thread (row tid >> 1, half xh = tid & 1) requests the
// 16-byte group of its row that starts at column cs = min(4 xh, K1 - 4) -- the second half clamped to END at K1 -- and
// stores ctx_fix of it: the group moved up by sh = 4 xh - cs to its columns 4 xh .. 4 xh + 3, columns at or past K1 as zeros
// (stream_tiles keeps its own copy: called from there, this function costs gemm_rows_cus_kernel ~960 instructions)
__device__ __forceinline__ f32x4 ctx_fix(const f32x4 v, const int sh, const int xh, const int K1) {
  f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float x = sh == 0 ? v[e] : (sh == 1 ? v[(e + 1) & 3] : (sh == 2 ? v[(e + 2) & 3] : v[(e + 3) & 3]));
    o[e] = (4 * xh + e < K1) ? x : 0.f;
  }
  return o;
}

// Fragment addresses (a_frag, b_frag, x_frag below) of lane (lr = lane & 31, lh = lane >> 5) inside LDS buffer 0:
//   a_frag = &As[(wave * 32 + lr) * LS + 4 * lh]   row wave * 32 + lr of A
//   b_frag = &Bs[lr * LS + 4 * lh]                 row lr of B's first column tile
//   x_frag = &Bs[(32 * TN) * LS + 4 * lh]          the XC extra rows of the B tile: one k quad per half wave
// (written out in cu_tile and stream_tiles: behind a function here, the stream-K kernels' code comes out different)

// fragment read j of 8-k group kg from LDS buffer `buf` into set (fa, fb, fx): j = 0 is A, 1..TN the B tiles, then the XC columns
template <int TN, int XC>
__device__ __forceinline__ void read_frag(const float* a_frag, const float* b_frag, const float* x_frag, int j, int buf, int kg,
                                          f32x4& fa, f32x4 (&fb)[TN], f32x4 (&fx)[XC > 0 ? XC : 1]) {
  constexpr int NR = TN + 1, B_BUF = b_buf(TN, XC);
  if (j == 0)
    fa = *reinterpret_cast<const f32x4*>(a_frag + buf * A_BUF + kg * 8);
  else if (j < NR)
    fb[j - 1] = *reinterpret_cast<const f32x4*>(b_frag + buf * B_BUF + (j - 1) * 32 * LS + kg * 8);
  else
    fx[j - NR] = *reinterpret_cast<const f32x4*>(x_frag + buf * B_BUF + (j - NR) * LS + kg * 8);
}
// The 4 TN MFMAs of one 8-k group, each pinned; aux(i) is issued behind MFMA i and must be independent of it.  Behind the
// first XC MFMAs: the VALU columns' four k positions of the lane's quad (xacc[c], summed at the end: xcol_total)
template <int TN, int XC, class Aux>
__device__ __forceinline__ void mfma_group(f32x16 (&acc)[TN], f32x4 (&xacc)[XC > 0 ? XC : 1], const f32x4& fa,
                                           const f32x4 (&fb)[TN], const f32x4 (&fx)[XC > 0 ? XC : 1], Aux&& aux) {
#pragma unroll
  for (int i = 0; i < 4 * TN; ++i) {
    acc[i % TN] = mfma32(fa[i / TN], fb[i % TN][i / TN], acc[i % TN]);
    CARCA_PIN();
    if constexpr (XC > 0) {
      if (i < XC) {
        // two v_pk_fma_f32, written out: left to the compiler the same four FMAs cost 70 spilled VGPRs (it re-plans the
        // fragment registers of the whole pinned step around them)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        const int c = i < XC ? i : 0;
        f32x2 a0 = {fa[0], fa[1]}, a1 = {fa[2], fa[3]};
        f32x2 w0 = {fx[c][0], fx[c][1]}, w1 = {fx[c][2], fx[c][3]};
        f32x2 x0 = {xacc[c][0], xacc[c][1]}, x1 = {xacc[c][2], xacc[c][3]};
        asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(x0) : "v"(a0), "v"(w0));
        asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(x1) : "v"(a1), "v"(w1));
        xacc[c] = f32x4{x0[0], x0[1], x1[0], x1[1]};
      }
    }
    aux(i);
    CARCA_PIN();
  }
}
// A VALU column at the end: lane (lr, lh) holds row wave * 32 + lr's sum over the k quads of its half in xacc; the two
// halves meet (both lanes of a row get the total)
__device__ __forceinline__ float xcol_total(const f32x4& xacc) {
  const float mine = (xacc[0] + xacc[1]) + (xacc[2] + xacc[3]);
  auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(mine), __float_as_uint(mine), false, false);
  return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}

}  // namespace tile384
}  // namespace
