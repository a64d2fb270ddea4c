// The register staging of the sampled losses' tile kernels (sampled_xent.hip; sampled_bce.hip,
// section 16): a 64-row tile of an operand is loaded into registers one step ahead and written to LDS, masked, after the
// next barrier.  Both files include these helpers; each keeps its own tile kernel, mask / G rule and merge kernels.
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

}  // namespace
