// Launches shared by the softmax cross-entropy kernels: catalogue_xent.hip (the full catalogue) and
// sampled_xent.hip (K shared samples with the logQ correction).
//   cx_compact_kernel: the valid rows (pos in [1, n_items)) in row order;
//   cx_mean_kernel:    the fp64 mean of the row losses over the valid rows;
//   cx_reduce_kernel:  split partials summed in split order and scaled by grad / n_valid.
#pragma once
#include "carca_common.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int CX_COMPACT_THREADS = 1024;

__host__ __device__ inline int64_t cx_r64(int64_t n) { return (n + 63) / 64 * 64; }

// ---- valid rows, in row order -----------------------------------------------------------------------------------
__global__ __launch_bounds__(CX_COMPACT_THREADS) void cx_compact_kernel(const int32_t* __restrict__ pos, int R, int n_items,
                                                                         int32_t* __restrict__ ridx,
                                                                         int32_t* __restrict__ rpos, int32_t* __restrict__ nv) {
  __shared__ int wsum[CX_COMPACT_THREADS / 64];
  __shared__ int base_s;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) base_s = 0;
  __syncthreads();
  for (int r0 = 0; r0 < R; r0 += CX_COMPACT_THREADS) {
    const int r = r0 + tid;
    const int p = r < R ? pos[r] : 0;
    const bool ok = r < R && p >= 1 && p < n_items;
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

__global__ __launch_bounds__(1024) void cx_mean_kernel(CarcaCatalogueXentDesc D, const int32_t* __restrict__ nv) {
  __shared__ double red[1024];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int r = tid; r < D.R; r += 1024) s += (double)D.row_loss[r];
  red[tid] = s;
  __syncthreads();
  for (int h = 512; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) D.loss[0] = nv[0] > 0 ? (float)(red[0] / (double)nv[0]) : 0.f;
}

// dst[e][col] (col < ld_dst) = coef * sum over splits of part[s][map(e)][col] for col < d, else 0
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
    const int n = nv[0];
    v *= n > 0 ? grad[0] / (float)n : 0.f;
  }
  dst[(size_t)e * ld_dst + col] = v;
}

}  // namespace
