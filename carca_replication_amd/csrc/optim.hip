// f3: the optimizer step of the train driver as ONE launch.
// The reference trains with torch.optim.Adam(lr, betas=(0.9, 0.98), weight_decay) (scripts/training.py:174,
// src/train.py:96); its update for parameter p with gradient g at step t (no amsgrad, L2-style weight decay) is
//   g  = g + wd * p
//   m  = m + (1 - b1) (g - m)                  (torch writes it as lerp)
//   v  = b2 v + (1 - b2) g g
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// All of a model's tensors are walked by one grid: a table of (p, g, m, v, n) entries passed by value, blocks assigned
// to 1024-element chunks through a prefix of chunk counts.  HBM-bound: 7 floats moved per element (read p g m v, write
// p m v) = 28 B/element, 87 MB for the 3.09 M parameters of C2.
// Two options of the same launch: the gradient multiplied by a device scalar first (clipping by
// global norm: carca_grad_norm below computes that scalar), and decoupled weight decay (torch.optim.AdamW):
//   p  = p (1 - lr wd)        instead of        g = g + wd p
#include "carca_common.h"
#include "../../include/carca_hip.h"

namespace {

constexpr int ADAM_MAX = 48;     // tensors per launch (3.6 KB of kernel arguments)
constexpr int ADAM_CHUNK = 1024; // elements per block

struct AdamTable {
  CarcaAdamTensor t[ADAM_MAX];
  int chunk_start[ADAM_MAX + 1];
  int n;
};
struct AdamScalars {
  float lr_c1;      // lr / (1 - b1^t)
  float sqrt_c2;    // sqrt(1 - b2^t)
  float omb1, b2, omb2, eps, wd;  // 1 - b1 and 1 - b2 rounded from double like torch's python scalars
  float decay;      // decoupled decay: 1 - lr*wd, combined in double and rounded once
};

// A product rounded on its own: never one half of a contracted multiply-add (hipcc contracts across statements by
// default and honours this pragma; __fmul_rn is a plain `*` to it).
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// SCALE: g arrives multiplied by `gs` (the clip factor).  DECOUPLED: AdamW.  Both products are rounded on their own: the
// bits are those of scaling the gradient / decaying the parameter in a pass of its own and then taking the plain step.
// The plain step keeps the four lines it always had, and with them the multiply-adds the compiler contracts them into:
// g = fma(wd, p, g), m = fma(1-b1, g - m, m), and for v fma(g, (1-b2) g, b2 v) on the one-float paths but
// fma(b2, v, g ((1-b2) g)) on the four-float paths (VEC).  The other three instantiations spell exactly those out -- left
// to itself the compiler contracts g * gs or pairs it with wd * p instead -- so that all four round alike: a clip factor
// of 1.0f changes no bit (tests/test_hip_optim_clip.py holds this on every path).
template <bool SCALE, bool DECOUPLED, bool VEC>
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& s, float gs) {
  if (!SCALE && !DECOUPLED) {
    g = g + s.wd * p;
    m = m + s.omb1 * (g - m);
    v = s.b2 * v + s.omb2 * g * g;
    p = p - s.lr_c1 * m / (sqrtf(v) / s.sqrt_c2 + s.eps);
    return;
  }
  if (SCALE) g = mul_rounded(g, gs);
  if (DECOUPLED)
    p = mul_rounded(p, s.decay);
  else
    g = __fmaf_rn(s.wd, p, g);
  m = __fmaf_rn(s.omb1, g - m, m);
  const float og = mul_rounded(s.omb2, g);
  v = VEC ? __fmaf_rn(s.b2, v, mul_rounded(og, g)) : __fmaf_rn(g, og, mul_rounded(s.b2, v));
  p = p - mul_rounded(s.lr_c1, m) / (sqrtf(v) / s.sqrt_c2 + s.eps);
}

template <bool SCALE, bool DECOUPLED>
__global__ __launch_bounds__(256) void adam_kernel(const AdamTable tab, const AdamScalars s, const float* __restrict__ grad_scale) {
  const float gs = SCALE ? *grad_scale : 1.f;
  int ti = 0;
  for (int i = 1; i < tab.n; ++i)
    if ((int)blockIdx.x >= tab.chunk_start[i]) ti = i;
  const CarcaAdamTensor T = tab.t[ti];
  const int64_t base = (int64_t)((int)blockIdx.x - tab.chunk_start[ti]) * ADAM_CHUNK;
  const int64_t left = T.n - base;
  const bool aligned = (((uintptr_t)T.p | (uintptr_t)T.g | (uintptr_t)T.m | (uintptr_t)T.v) & 15) == 0;
  if (T.row_mask && !((T.row_len & 3) == 0 && aligned)) {  // rows or pointers off the 16-byte grid: one float per thread
    for (int64_t i = base + threadIdx.x; i < base + ADAM_CHUNK && i < T.n; i += 256) {
      if (!T.row_mask[i / T.row_len]) continue;
      float p = T.p[i], m = T.m[i], v = T.v[i];
      adam_one<SCALE, DECOUPLED, false>(p, T.g[i], m, v, s, gs);
      T.p[i] = p;
      T.m[i] = m;
      T.v[i] = v;
    }
    return;
  }
  if (T.row_mask) {  // embedding table with a row mask: untouched rows are skipped (see the header)
    for (int64_t i = base + threadIdx.x * 4; i < base + ADAM_CHUNK && i < T.n; i += 1024) {
      if (!T.row_mask[i / T.row_len]) continue;
      f32x4 p = *reinterpret_cast<const f32x4*>(T.p + i), m = *reinterpret_cast<const f32x4*>(T.m + i);
      f32x4 v = *reinterpret_cast<const f32x4*>(T.v + i);
      const f32x4 g = *reinterpret_cast<const f32x4*>(T.g + i);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float pr = p[r], mr = m[r], vr = v[r];
        adam_one<SCALE, DECOUPLED, true>(pr, g[r], mr, vr, s, gs);
        p[r] = pr;
        m[r] = mr;
        v[r] = vr;
      }
      *reinterpret_cast<f32x4*>(T.p + i) = p;
      *reinterpret_cast<f32x4*>(T.m + i) = m;
      *reinterpret_cast<f32x4*>(T.v + i) = v;
    }
    return;
  }
  const bool vec = left >= ADAM_CHUNK && aligned;
  if (vec) {  // one float4 per thread
    const int64_t i = base + threadIdx.x * 4;
    f32x4 p = *reinterpret_cast<const f32x4*>(T.p + i), m = *reinterpret_cast<const f32x4*>(T.m + i);
    f32x4 v = *reinterpret_cast<const f32x4*>(T.v + i);
    const f32x4 g = *reinterpret_cast<const f32x4*>(T.g + i);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float pr = p[r], mr = m[r], vr = v[r];
      adam_one<SCALE, DECOUPLED, true>(pr, g[r], mr, vr, s, gs);
      p[r] = pr;
      m[r] = mr;
      v[r] = vr;
    }
    *reinterpret_cast<f32x4*>(T.p + i) = p;
    *reinterpret_cast<f32x4*>(T.m + i) = m;
    *reinterpret_cast<f32x4*>(T.v + i) = v;
  } else {
    for (int64_t i = base + threadIdx.x; i < base + ADAM_CHUNK && i < T.n; i += 256) {
      float p = T.p[i], m = T.m[i], v = T.v[i];
      adam_one<SCALE, DECOUPLED, false>(p, T.g[i], m, v, s, gs);
      T.p[i] = p;
      T.m[i] = m;
      T.v[i] = v;
    }
  }
}

// ---- global gradient norm ---------------------------------------------------------------------
// Sum of squares of one 1024-element chunk per block, over the same table and chunk prefix as adam_kernel.  Which
// elements a thread owns depends on the chunk and on g's alignment ONLY (never on the row mask): 4 consecutive ones
// where the chunk is full and g is 16-byte aligned, elements t, t+256, t+512, t+768 otherwise.  A masked row's
// elements enter as 0 without being read -- their gradient IS 0 (CarcaAdamTensor.row_mask) and x + 0 = x, so the sum
// has the bits of the unmasked one.  Fixed order throughout: one product and three fused multiply-adds per thread, a
// 6-stage butterfly per wave, the four wave sums added in wave order: 13 roundings on the longest path.  No atomics.
__device__ __forceinline__ float sumsq4(float a, float b, float c, float d) {
  return __fmaf_rn(d, d, __fmaf_rn(c, c, __fmaf_rn(b, b, mul_rounded(a, a))));
}

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const AdamTable tab, float* __restrict__ partials) {
  __shared__ float wave_sum[4];
  // the last entry whose first chunk is <= this block's (entries without elements share their successor's start): a
  // binary search -- at most 6 dependent reads of the argument block where adam_kernel's scan makes tab.n
  int ti = 0, hi = tab.n;
  while (hi - ti > 1) {
    const int mid = (ti + hi) >> 1;
    if ((int)blockIdx.x >= tab.chunk_start[mid])
      ti = mid;
    else
      hi = mid;
  }
  const CarcaAdamTensor T = tab.t[ti];
  const int64_t base = (int64_t)((int)blockIdx.x - tab.chunk_start[ti]) * ADAM_CHUNK;
  const bool vec = T.n - base >= ADAM_CHUNK && (((uintptr_t)T.g) & 15) == 0;
  float e[4] = {0.f, 0.f, 0.f, 0.f};
  if (vec) {
    const int64_t i = base + threadIdx.x * 4;
    if (!T.row_mask) {
      const f32x4 g = *reinterpret_cast<const f32x4*>(T.g + i);
      e[0] = g[0], e[1] = g[1], e[2] = g[2], e[3] = g[3];
    } else if ((T.row_len & 3) == 0) {  // the four elements share a row
      if (T.row_mask[i / T.row_len]) {
        const f32x4 g = *reinterpret_cast<const f32x4*>(T.g + i);
        e[0] = g[0], e[1] = g[1], e[2] = g[2], e[3] = g[3];
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (T.row_mask[(i + r) / T.row_len]) e[r] = T.g[i + r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t i = base + threadIdx.x + r * 256;
      if (i < T.n && (!T.row_mask || T.row_mask[i / T.row_len])) e[r] = T.g[i];
    }
  }
  float s = sumsq4(e[0], e[1], e[2], e[3]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);  // (a + b = b + a: every lane holds the same bits)
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// One block: thread t adds partials[t], partials[t + 1024], ... in double, a fixed LDS tree adds the threads.
constexpr int NORM_FINISH_THREADS = 1024;
__global__ __launch_bounds__(NORM_FINISH_THREADS) void grad_norm_finish_kernel(const float* __restrict__ partials, int64_t n,
                                                                               float max_norm, float* __restrict__ out) {
  __shared__ double acc[NORM_FINISH_THREADS];
  double a = 0.;
#pragma unroll 8
  for (int64_t i = threadIdx.x; i < n; i += NORM_FINISH_THREADS) a += (double)partials[i];
  acc[threadIdx.x] = a;
  __syncthreads();
  for (int w = NORM_FINISH_THREADS / 2; w >= 1; w >>= 1) {
    if ((int)threadIdx.x < w) acc[threadIdx.x] += acc[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float norm = (float)sqrt(acc[0]);
    const float r = max_norm / (norm + 1e-6f);
    out[0] = norm;
    out[1] = r > 1.f ? 1.f : r;  // (a NaN norm stays a NaN scale: clip_grad_norm_ with error_if_nonfinite=False)
  }
}

__global__ void mark_rows_kernel(const int32_t* __restrict__ ids, int64_t n, uint8_t* __restrict__ mask, int64_t n_rows) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const int64_t r = ids[i];
    if (r >= 0 && r < n_rows) mask[r] = 1;
  }
}
struct IdLists {
  const int32_t* ids[CARCA_MAX_SEGS];
  long long start[CARCA_MAX_SEGS + 1];
  int n;
};
// one wave per id: its row is cleared with 16-byte stores (row_len % 4 == 0) or element stores
__global__ __launch_bounds__(256) void zero_rows_kernel(float* __restrict__ table, int64_t n_rows, int row_len, const IdLists L) {
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  if (i >= L.start[L.n]) return;
  int s = 0;
  for (int j = 1; j < L.n; ++j)
    if (i >= L.start[j]) s = j;
  const int64_t r = L.ids[s][i - L.start[s]];
  if (r < 0 || r >= n_rows) return;
  float* row = table + r * row_len;
  if ((row_len & 3) == 0 && (((uintptr_t)table) & 15) == 0) {
    for (int c = lane * 4; c < row_len; c += 256) *reinterpret_cast<f32x4*>(row + c) = f32x4{0.f, 0.f, 0.f, 0.f};
  } else {
    for (int c = lane; c < row_len; c += 64) row[c] = 0.f;
  }
}
__global__ void concat_ids_kernel(const IdLists L, int32_t* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.start[L.n]) return;
  int s = 0;
  for (int j = 1; j < L.n; ++j)
    if (i >= L.start[j]) s = j;
  out[i] = L.ids[s][i - L.start[s]];
}
static int make_lists(const int32_t* const* ids, const int64_t* counts, int nlists, IdLists* L, const char* who) {
  CARCA_CHECK_ARG(ids && counts && nlists >= 1 && nlists <= CARCA_MAX_SEGS, "%s: 1..%d id lists", who, CARCA_MAX_SEGS);
  long long t = 0;
  for (int i = 0; i < nlists; ++i) {
    CARCA_CHECK_ARG(ids[i] && counts[i] >= 0, "%s: list %d malformed", who, i);
    L->ids[i] = ids[i];
    L->start[i] = t;
    t += counts[i];
  }
  L->start[nlists] = t;
  L->n = nlists;
  return CARCA_OK;
}

}  // namespace

extern "C" int carca_mark_rows(const int32_t* ids, int64_t n, uint8_t* mask, int64_t n_rows, void* stream_) {
  CARCA_CHECK_ARG(ids && mask && n >= 0 && n_rows >= 1, "mark_rows: null pointer or bad sizes");
  if (n == 0) return CARCA_OK;
  hipLaunchKernelGGL(mark_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, ids, n, mask, n_rows);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_zero_rows(float* table, int64_t n_rows, int row_len, const int32_t* const* ids, const int64_t* counts,
                               int nlists, void* stream_) {
  CARCA_CHECK_ARG(table && n_rows >= 1 && row_len >= 1, "zero_rows: null table or bad sizes");
  IdLists L{};
  int rc = make_lists(ids, counts, nlists, &L, "zero_rows");
  if (rc != CARCA_OK) return rc;
  if (L.start[L.n] == 0) return CARCA_OK;
  const long long blocks = (L.start[L.n] + 3) / 4;  // one wave per id, four waves per block
  CARCA_CHECK_SUPPORTED(blocks < (1ll << 31), "zero_rows: too many ids");
  hipLaunchKernelGGL(zero_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, table, n_rows, row_len, L);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_concat_ids(const int32_t* const* ids, const int64_t* counts, int nlists, int32_t* out, void* stream_) {
  CARCA_CHECK_ARG(out, "concat_ids: null output");
  IdLists L{};
  int rc = make_lists(ids, counts, nlists, &L, "concat_ids");
  if (rc != CARCA_OK) return rc;
  if (L.start[L.n] == 0) return CARCA_OK;
  hipLaunchKernelGGL(concat_ids_kernel, dim3((unsigned)((L.start[L.n] + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, L, out);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

// Table `first / ADAM_MAX` of a host array of tensors: up to ADAM_MAX entries and the prefix of their chunk counts.
static int fill_table(const CarcaAdamTensor* tensors, int n, int first, AdamTable* tab, long long* chunks_out, const char* who) {
  tab->n = n - first < ADAM_MAX ? n - first : ADAM_MAX;
  long long chunks = 0;
  for (int i = 0; i < tab->n; ++i) {
    tab->t[i] = tensors[first + i];
    tab->chunk_start[i] = (int)chunks;
    chunks += (tensors[first + i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
    CARCA_CHECK_SUPPORTED(chunks < (1ll << 31), "%s: too many elements in one launch", who);
  }
  tab->chunk_start[tab->n] = (int)chunks;
  *chunks_out = chunks;
  return CARCA_OK;
}

extern "C" int carca_grad_norm(const CarcaAdamTensor* tensors, int n, double max_norm, float* partials, int64_t n_partials,
                               float* out, void* stream_) {
  CARCA_CHECK_ARG(tensors && n >= 1, "grad_norm: no tensors");
  CARCA_CHECK_ARG(partials && out, "grad_norm: null partials or out");
  CARCA_CHECK_ARG(max_norm > 0., "grad_norm: max_norm must be > 0 (got %g)", max_norm);
  long long total = 0;
  for (int i = 0; i < n; ++i) {
    CARCA_CHECK_ARG(tensors[i].g && tensors[i].n >= 0, "grad_norm: tensor %d malformed", i);
    CARCA_CHECK_ARG(!tensors[i].row_mask || (tensors[i].row_len >= 1 && tensors[i].n % tensors[i].row_len == 0),
                    "grad_norm: tensor %d: a row mask needs row_len >= 1 dividing n", i);
    total += (tensors[i].n + ADAM_CHUNK - 1) / ADAM_CHUNK;
  }
  CARCA_CHECK_ARG(n_partials >= total, "grad_norm: %lld partials for %lld chunks of %d elements", (long long)n_partials, total,
                  ADAM_CHUNK);
  long long done = 0;
  for (int first = 0; first < n; first += ADAM_MAX) {
    AdamTable tab{};
    long long chunks = 0;
    int rc = fill_table(tensors, n, first, &tab, &chunks, "grad_norm");
    if (rc != CARCA_OK) return rc;
    if (chunks == 0) continue;
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream_, tab, partials + done);
    CARCA_LAUNCH_CHECK();
    done += chunks;
  }
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(NORM_FINISH_THREADS), 0, (hipStream_t)stream_, partials,
                     (int64_t)total, (float)max_norm, out);
  CARCA_LAUNCH_CHECK();
  return CARCA_OK;
}

extern "C" int carca_adam_step_ex(const CarcaAdamTensor* tensors, int n, double lr, double beta1, double beta2, double eps,
                                  double weight_decay, int step, int decoupled, const float* grad_scale, void* stream_) {
  CARCA_CHECK_ARG(tensors && n >= 1, "adam_step: no tensors");
  CARCA_CHECK_ARG(step >= 1 && lr >= 0. && beta1 >= 0. && beta1 < 1. && beta2 >= 0. && beta2 < 1. && eps >= 0. &&
                      weight_decay >= 0.,
                  "adam_step: bad hyper-parameters (step=%d lr=%g betas=(%g, %g) eps=%g wd=%g)", step, lr, beta1, beta2,
                  eps, weight_decay);
  for (int i = 0; i < n; ++i) {
    CARCA_CHECK_ARG(tensors[i].p && tensors[i].g && tensors[i].m && tensors[i].v && tensors[i].n >= 0,
                    "adam_step: tensor %d malformed", i);
    CARCA_CHECK_ARG(!tensors[i].row_mask || (tensors[i].row_len >= 1 && weight_decay == 0.),
                    "adam_step: tensor %d: a row mask needs row_len >= 1 and weight_decay = 0 (decay moves untouched rows)", i);
  }
  AdamScalars s;
  s.lr_c1 = (float)(lr / (1.0 - pow(beta1, step)));  // the host arithmetic torch does in double, rounded once
  s.sqrt_c2 = (float)sqrt(1.0 - pow(beta2, step));
  s.omb1 = (float)(1.0 - beta1);
  s.b2 = (float)beta2;
  s.omb2 = (float)(1.0 - beta2);
  s.eps = (float)eps;
  s.wd = (float)weight_decay;
  s.decay = (float)(1.0 - lr * weight_decay);
  auto kernel = grad_scale ? (decoupled ? adam_kernel<true, true> : adam_kernel<true, false>)
                           : (decoupled ? adam_kernel<false, true> : adam_kernel<false, false>);
  for (int first = 0; first < n; first += ADAM_MAX) {
    AdamTable tab{};
    long long chunks = 0;
    int rc = fill_table(tensors, n, first, &tab, &chunks, "adam_step");
    if (rc != CARCA_OK) return rc;
    if (chunks == 0) continue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream_, tab, s, grad_scale);
    CARCA_LAUNCH_CHECK();
  }
  return CARCA_OK;
}

extern "C" int carca_adam_step(const CarcaAdamTensor* tensors, int n, double lr, double beta1, double beta2, double eps,
                               double weight_decay, int step, void* stream_) {
  return carca_adam_step_ex(tensors, n, lr, beta1, beta2, eps, weight_decay, step, 0, nullptr, stream_);
}
