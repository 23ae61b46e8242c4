// Optimiser kernels beyond the reference's Adam, over the model's flat fp32 parameter / gradient buffers: the L2 norm of the gradient (fixed-order fp64 reduction), the clip
// record it leaves in device memory (coefficient of torch.nn.utils.clip_grad_norm_, skip flag for a non-finite norm, running statistics), and the SGD (momentum, Nesterov)
// and Adam / AdamW updates that read the coefficient from that record.  The host reads nothing on the step path.
// All are HBM-bound streaming kernels: 16-byte loads and stores, a scalar tail, a grid-stride loop.  vsseg_adam (elementwise.hip) is untouched.
#include "common.h"
#include <math.h>

static_assert(sizeof(vsseg_clip_record) == 64, "the record layout is part of the ABI");

constexpr int GN_THREADS = 256;
constexpr int GN_SHARD = VSSEG_GRAD_NORM_SHARD;    // elements per partial: 8 float4 per thread
constexpr int GN_FINAL = VSSEG_GRAD_NORM_FINAL;    // partials consumed per pass of the finalising workgroup (thread = partial)
constexpr int GN_VEC = GN_SHARD / (4 * GN_THREADS);  // float4 per thread and shard
static_assert(GN_SHARD == GN_VEC * 4 * GN_THREADS && GN_FINAL == GN_THREADS, "shard = whole float4 rounds of the workgroup; finalise: thread = partial");

// sum over the 256 threads of a workgroup in a fixed order (butterfly inside a wave, then wave 0 + 1 + 2 + 3); valid in thread 0
__device__ __forceinline__ double gn_block_sum(double v, double* part) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((part[0] + part[1]) + part[2]) + part[3];
  __syncthreads();
  return r;
}

// partials[s] = sum of g[i]^2 over shard s = [s * GN_SHARD, (s + 1) * GN_SHARD) ∩ [0, n), every square and every addition in fp64.  Thread t owns the float4 groups
// t, t + 256, ... of the shard and adds their elements in index order; the vector path (whole shard, 16-byte aligned base) and the guarded scalar path add the same
// elements in the same order, so a partial does not depend on which of them ran, and nothing depends on the grid (shards are strided over the workgroups).
__global__ __launch_bounds__(GN_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n, int64_t nshards, double* __restrict__ partials, int aligned) {
  __shared__ double part[4];
  for (int64_t s = blockIdx.x; s < nshards; s += gridDim.x) {
    const int64_t base = s * GN_SHARD;
    double acc = 0.0;
    if (aligned && base + GN_SHARD <= n) {
      const float4* q = reinterpret_cast<const float4*>(g + base) + threadIdx.x;
      float4 x[GN_VEC];
#pragma unroll
      for (int j = 0; j < GN_VEC; ++j) x[j] = q[j * GN_THREADS];
#pragma unroll
      for (int j = 0; j < GN_VEC; ++j) {
        acc = __builtin_fma((double)x[j].x, (double)x[j].x, acc);
        acc = __builtin_fma((double)x[j].y, (double)x[j].y, acc);
        acc = __builtin_fma((double)x[j].z, (double)x[j].z, acc);
        acc = __builtin_fma((double)x[j].w, (double)x[j].w, acc);
      }
    } else {
#pragma unroll
      for (int j = 0; j < GN_VEC; ++j) {
        const int64_t i0 = base + 4 * (int64_t)(j * GN_THREADS + threadIdx.x);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double d = i0 + k < n ? (double)g[i0 + k] : 0.0;
          acc = __builtin_fma(d, d, acc);
        }
      }
    }
    const double r = gn_block_sum(acc, part);
    if (threadIdx.x == 0) partials[s] = r;
  }
}

// One workgroup: thread t adds the partials t, t + GN_FINAL, ... in that order, the 256 sums are combined in the fixed order of gn_block_sum; thread 0 writes the record.
__global__ __launch_bounds__(GN_THREADS) void grad_norm_finalize_kernel(const double* __restrict__ partials, int64_t nshards, double gscale_abs, double max_norm, vsseg_clip_record* __restrict__ rec) {
  __shared__ double part[4];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < nshards; i += GN_FINAL) acc += partials[i];
  const double total = gn_block_sum(acc, part);
  if (threadIdx.x != 0) return;
  const double norm = gscale_abs * sqrt(total);
  const bool finite = isfinite(norm);
  const float coef = finite ? (float)fmin(1.0, max_norm / (norm + 1e-6)) : 0.f;  // clip_grad_norm_'s coefficient, formed in fp64 and rounded once
  rec->norm = norm;
  rec->coef = coef;
  rec->skip = finite ? 0 : 1;
  rec->steps += 1;
  if (finite) {
    if (coef < 1.f) rec->clipped += 1;
    rec->norm_sum += norm;
    if (norm > rec->norm_max) rec->norm_max = norm;
  } else {
    rec->skipped += 1;
  }
}

static inline int64_t gn_shards(int64_t n) { return (n + GN_SHARD - 1) / GN_SHARD; }

extern "C" int64_t vsseg_grad_norm_scratch_bytes(int64_t n) {
  VSSEG_CHECK(n >= 0, "vsseg_grad_norm_scratch_bytes: n = %lld is negative", (long long)n);
  const int64_t shards = gn_shards(n);
  return 8 * (shards > 0 ? shards : 1);
}

extern "C" int vsseg_grad_norm(const float* g, int64_t n, float gscale, double max_norm, double* scratch, int64_t scratch_bytes, vsseg_clip_record* record, void* stream) {
  VSSEG_CHECK(n >= 0, "vsseg_grad_norm: n = %lld is negative", (long long)n);
  VSSEG_CHECK((g || n == 0) && scratch && record, "vsseg_grad_norm: null pointer");
  VSSEG_CHECK(((uintptr_t)g & 3) == 0 && ((uintptr_t)scratch & 7) == 0 && ((uintptr_t)record & 7) == 0, "vsseg_grad_norm: misaligned pointer (g 4, scratch 8, record 8 bytes)");
  VSSEG_CHECK(isfinite(max_norm) && max_norm > 0.0, "vsseg_grad_norm: max_norm = %g must be finite and > 0", max_norm);
  VSSEG_CHECK(isfinite(gscale), "vsseg_grad_norm: gscale = %g must be finite", (double)gscale);
  const int64_t shards = gn_shards(n);
  VSSEG_CHECK(scratch_bytes >= 8 * shards, "vsseg_grad_norm: %lld bytes of scratch, %lld needed (vsseg_grad_norm_scratch_bytes)", (long long)scratch_bytes, (long long)(8 * shards));
  if (shards > 0) {
    const int grid = (int)(shards < 1024 ? shards : 1024);
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3(grid), dim3(GN_THREADS), 0, as_stream(stream), g, n, shards, scratch, (int)(((uintptr_t)g & 15) == 0));
    VSSEG_LAUNCH_CHECK("vsseg_grad_norm");
  }
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(GN_THREADS), 0, as_stream(stream), (const double*)scratch, shards, fabs((double)gscale), max_norm, record);
  VSSEG_LAUNCH_CHECK("vsseg_grad_norm");
  return VSSEG_OK;
}

// ------------------------------------------------------------------------------------------------------------
// updates.  `rec` may be null (coefficient 1, never skipped).  A set skip flag leaves every buffer bitwise untouched: the kernel returns before its first store.
// ------------------------------------------------------------------------------------------------------------
struct ClipView {
  float coef;
  bool skip;
};
__device__ __forceinline__ ClipView clip_of(const vsseg_clip_record* rec) { return rec ? ClipView{rec->coef, rec->skip != 0} : ClipView{1.f, false}; }

// torch.optim.SGD(lr, momentum, dampening 0, weight_decay, nesterov): g' = coef * (gscale * g) + wd * p; buf = mu * buf + g'; d = nesterov ? g' + mu * buf : buf; p -= lr * d
// MOM 0: no buffer (d = g'), 1: momentum, 2: Nesterov
// No contraction into fused multiply-adds in the two element functions: every product and sum is rounded on its own, as written, so that the vector body, the scalar
// tail and the unaligned kernel give the same bits for the same element (hipcc contracts differently from one instantiation to the next).
template <int MOM> __device__ __forceinline__ void sgd_elem(float& p, float g, float& b, float lr, float mu, float wd, float gscale, float coef) {
#pragma clang fp contract(off)
  const float gg = g * gscale * coef + wd * p;
  float d = gg;
  if constexpr (MOM != 0) {
    b = mu * b + gg;
    d = MOM == 2 ? gg + mu * b : b;
  }
  p = p - lr * d;
}
template <int MOM, bool VEC>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n, float lr, float mu, float wd, float gscale, const vsseg_clip_record* __restrict__ rec) {
  const ClipView c = clip_of(rec);
  if (c.skip) return;
  const int64_t gt = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = VEC ? n >> 2 : 0;
  for (int64_t i = gt; i < n4; i += nthreads) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    float4 bb = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (MOM != 0) bb = reinterpret_cast<float4*>(buf)[i];
    sgd_elem<MOM>(pp.x, gg.x, bb.x, lr, mu, wd, gscale, c.coef);
    sgd_elem<MOM>(pp.y, gg.y, bb.y, lr, mu, wd, gscale, c.coef);
    sgd_elem<MOM>(pp.z, gg.z, bb.z, lr, mu, wd, gscale, c.coef);
    sgd_elem<MOM>(pp.w, gg.w, bb.w, lr, mu, wd, gscale, c.coef);
    if constexpr (MOM != 0) reinterpret_cast<float4*>(buf)[i] = bb;
    reinterpret_cast<float4*>(p)[i] = pp;
  }
  for (int64_t i = 4 * n4 + gt; i < n; i += nthreads) {  // the tail (everything when the buffers are not 16-byte aligned)
    float pp = p[i], bb = 0.f;
    if constexpr (MOM != 0) bb = buf[i];
    sgd_elem<MOM>(pp, g[i], bb, lr, mu, wd, gscale, c.coef);
    if constexpr (MOM != 0) buf[i] = bb;
    p[i] = pp;
  }
}

// torch.optim.Adam (DEC false: coupled decay, the arithmetic of adam_kernel with the clipped gradient) / torch.optim.AdamW (DEC true: p *= 1 - lr * wd first, no wd * p in
// the gradient)
template <bool DEC> __device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float b1, float b2, float eps, float wd, float decay, float step_size, float inv_sqrt_bc2, float gscale, float coef) {
#pragma clang fp contract(off)
  float pp = p, gg = g * gscale * coef;
  if constexpr (DEC) pp = pp * decay;
  else gg = gg + wd * pp;
  const float mm = b1 * m + (1.f - b1) * gg;
  const float vv = b2 * v + (1.f - b2) * gg * gg;
  m = mm;
  v = vv;
  p = pp - step_size * mm / (sqrtf(vv) * inv_sqrt_bc2 + eps);
}
template <bool DEC, bool VEC>
__global__ __launch_bounds__(256) void adam_clipped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n, float lr, float b1, float b2, float eps, float wd, float decay,
                                                           float bc1, float bc2, float gscale, const vsseg_clip_record* __restrict__ rec) {
  const ClipView c = clip_of(rec);
  if (c.skip) return;
  const float step_size = lr / bc1, inv_sqrt_bc2 = rsqrtf(bc2);
  const int64_t gt = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthreads = (int64_t)gridDim.x * blockDim.x;
  const int64_t n4 = VEC ? n >> 2 : 0;
  for (int64_t i = gt; i < n4; i += nthreads) {
    float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    adam_elem<DEC>(pp.x, gg.x, mm.x, vv.x, b1, b2, eps, wd, decay, step_size, inv_sqrt_bc2, gscale, c.coef);
    adam_elem<DEC>(pp.y, gg.y, mm.y, vv.y, b1, b2, eps, wd, decay, step_size, inv_sqrt_bc2, gscale, c.coef);
    adam_elem<DEC>(pp.z, gg.z, mm.z, vv.z, b1, b2, eps, wd, decay, step_size, inv_sqrt_bc2, gscale, c.coef);
    adam_elem<DEC>(pp.w, gg.w, mm.w, vv.w, b1, b2, eps, wd, decay, step_size, inv_sqrt_bc2, gscale, c.coef);
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(p)[i] = pp;
  }
  for (int64_t i = 4 * n4 + gt; i < n; i += nthreads) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam_elem<DEC>(pp, g[i], mm, vv, b1, b2, eps, wd, decay, step_size, inv_sqrt_bc2, gscale, c.coef);
    m[i] = mm;
    v[i] = vv;
    p[i] = pp;
  }
}

static inline bool aligned16(const void* a, const void* b, const void* c, const void* d) { return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 15) == 0; }
static inline bool aligned4(const void* a, const void* b, const void* c, const void* d) { return ((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c) | ((uintptr_t)d)) & 3) == 0; }
// one float4 per thread and round when the buffers allow it, else one element
static inline int update_grid(int64_t n, bool vec) { return grid_for(vec ? (n + 3) / 4 : n, 256, 2048); }

extern "C" int vsseg_sgd(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd, int32_t nesterov, float gscale, const vsseg_clip_record* record, void* stream) {
  VSSEG_CHECK(n >= 0, "vsseg_sgd: n = %lld is negative", (long long)n);
  VSSEG_CHECK(momentum >= 0.f && momentum < 1.f, "vsseg_sgd: momentum = %g must be in [0, 1)", (double)momentum);
  VSSEG_CHECK(!nesterov || momentum > 0.f, "vsseg_sgd: Nesterov momentum needs momentum > 0");
  VSSEG_CHECK(p && g && (buf || momentum == 0.f), "vsseg_sgd: null pointer (the momentum buffer may be null only with momentum 0)");
  VSSEG_CHECK(aligned4(p, g, buf, nullptr) && ((uintptr_t)record & 7) == 0, "vsseg_sgd: misaligned pointer");
  if (n == 0) return VSSEG_OK;
  const bool vec = aligned16(p, g, momentum > 0.f ? buf : nullptr, nullptr);
  const dim3 grid(update_grid(n, vec)), block(256);
  hipStream_t s = as_stream(stream);
#define SGD_LAUNCH(MOM)                                                                                                                     \
  do {                                                                                                                                      \
    if (vec) hipLaunchKernelGGL((sgd_kernel<MOM, true>), grid, block, 0, s, p, g, buf, n, lr, momentum, wd, gscale, record);                \
    else hipLaunchKernelGGL((sgd_kernel<MOM, false>), grid, block, 0, s, p, g, buf, n, lr, momentum, wd, gscale, record);                   \
  } while (0)
  if (momentum == 0.f) SGD_LAUNCH(0);
  else if (!nesterov) SGD_LAUNCH(1);
  else SGD_LAUNCH(2);
#undef SGD_LAUNCH
  VSSEG_LAUNCH_CHECK("vsseg_sgd");
  return VSSEG_OK;
}

extern "C" int vsseg_adam_clipped(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps, float wd, float bc1, float bc2, float gscale, int32_t decoupled,
                                  const vsseg_clip_record* record, void* stream) {
  VSSEG_CHECK(n >= 0, "vsseg_adam_clipped: n = %lld is negative", (long long)n);
  VSSEG_CHECK(p && g && m && v, "vsseg_adam_clipped: null pointer");
  VSSEG_CHECK(aligned4(p, g, m, v) && ((uintptr_t)record & 7) == 0, "vsseg_adam_clipped: misaligned pointer");
  if (n == 0) return VSSEG_OK;
  if (!record && !decoupled) return vsseg_adam(p, g, m, v, n, lr, beta1, beta2, eps, wd, bc1, bc2, gscale, stream);  // nothing to clip, coupled decay: the same launch, the same bits
  const bool vec = aligned16(p, g, m, v);
  const dim3 grid(update_grid(n, vec)), block(256);
  hipStream_t s = as_stream(stream);
  const float decay = (float)(1.0 - (double)lr * (double)wd);
#define ADAM_LAUNCH(DEC)                                                                                                                                              \
  do {                                                                                                                                                                \
    if (vec) hipLaunchKernelGGL((adam_clipped_kernel<DEC, true>), grid, block, 0, s, p, g, m, v, n, lr, beta1, beta2, eps, wd, decay, bc1, bc2, gscale, record);      \
    else hipLaunchKernelGGL((adam_clipped_kernel<DEC, false>), grid, block, 0, s, p, g, m, v, n, lr, beta1, beta2, eps, wd, decay, bc1, bc2, gscale, record);         \
  } while (0)
  if (decoupled) ADAM_LAUNCH(true);
  else ADAM_LAUNCH(false);
#undef ADAM_LAUNCH
  VSSEG_LAUNCH_CHECK("vsseg_adam_clipped");
  return VSSEG_OK;
}
