// Dice_spvPA loss (ref:params/losses/dice_spvPA.py:90-167, 238-297) as fused reductions + one elementwise backward,
// and the hard-Dice metric (ref:params/VSparams.py:393-408).  Everything here is HBM-bound: logits are read once
// forward and once backward; the ~25 ATen temporaries of the reference never exist.
#include "common.h"
#include "topk.h"
#include "volume.h"  // the mask rule

#define SMOOTH 1e-5

// label pyramid for the attention supervision: G_{l+1} = MaxPool3d(ratio)(G_l)   (ref :268-277)
__global__ void maxpool_label_kernel(const float* __restrict__ src, int n, int sx, int sy, int sz, int rx, int ry, int rz, float* __restrict__ dst) {
  const int dx = sx / rx, dy = sy / ry, dz = sz / rz;
  const int64_t total = (int64_t)n * dx * dy * dz;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    int z = (int)(r % dz); r /= dz;
    int y = (int)(r % dy); r /= dy;
    int x = (int)(r % dx);
    int64_t b = r / dx;
    float m = -INFINITY;
    for (int a = 0; a < rx; ++a)
      for (int c = 0; c < ry; ++c)
        for (int e = 0; e < rz; ++e) m = fmaxf(m, src[((b * sx + x * rx + a) * sy + y * ry + c) * (int64_t)sz + z * rz + e]);
    dst[i] = m;
  }
}
extern "C" int vsseg_maxpool_label(const float* src, int32_t n, const int32_t sdims[3], const int32_t ratio[3], float* dst, void* stream) {
  VSSEG_CHECK(src && dst && ratio[0] >= 1 && ratio[1] >= 1 && ratio[2] >= 1, "vsseg_maxpool_label: bad arguments");
  VSSEG_CHECK(sdims[0] % ratio[0] == 0 && sdims[1] % ratio[1] == 0 && sdims[2] % ratio[2] == 0, "vsseg_maxpool_label: attention pyramid shapes must divide (ref dice_spvPA.py:273)");
  int64_t total = (int64_t)n * (sdims[0] / ratio[0]) * (sdims[1] / ratio[1]) * (sdims[2] / ratio[2]);
  hipLaunchKernelGGL(maxpool_label_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), src, n, sdims[0], sdims[1], sdims[2], ratio[0], ratio[1], ratio[2], dst);
  VSSEG_LAUNCH_CHECK("vsseg_maxpool_label");
  return VSSEG_OK;
}

// `fx` > 0: the block's sums are added as fixed-point integers of that scale (vsseg_fx_add: order-independent); 0: fp64 atomics (the hard-Dice voxel
// counts: integers, exact in fp64 whatever the order)
constexpr double VSSEG_FX_DICE = 4294967296.0;  // 2^32: sums of at most 2^31 voxel weights in [0, 1], 2.3e-10 resolution
__device__ __forceinline__ void block_reduce_add(double* vals, int nvals, double* dst, double fx, unsigned* fxflag) {
  __shared__ double sh[16][12];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int k = 0; k < nvals; ++k) {
    double v = wave_sum_d(vals[k]);
    if (lane == 0) sh[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < nvals) {
    double t = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += sh[w][threadIdx.x];
    if (fx > 0.0) vsseg_fx_add(&dst[threadIdx.x], t, fx, fxflag);
    else atomicAdd(&dst[threadIdx.x], t);
  }
}

// Launch shape of the three reductions below: every workgroup ends with one fixed-point atomic per sum, all of a launch's sums share one or two cache lines, and the
// atomics of one LINE retire one after the other (~4 ns each: with the 1024 workgroups per sample of the first version — 12288 atomics into 96 bytes — the
// attention-map sums of the 96x32x128 level took 49 us for 6 MB, profiles/r06_kernel_stats.txt).  ~512 workgroups of 512 threads in total (2 per CU, 16 waves per CU),
// 16-byte loads.
constexpr int DICE_THREADS = 512;
static inline int dice_blocks(int64_t items, int n) {
  int64_t want = (items + DICE_THREADS * 2 - 1) / (DICE_THREADS * 2);
  const int cap = n >= 512 ? 1 : 512 / n;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

// the six terms of one voxel of the (optionally hardness-weighted) 2-class soft Dice (ref :279-283)
__device__ __forceinline__ void dice_pred_terms(float l0, float l1, float lab, int hardness, float* t) {
  const float m = fmaxf(l0, l1), e0 = __expf(l0 - m), e1 = __expf(l1 - m), inv = 1.f / (e0 + e1);
  const float p0 = e0 * inv, p1 = e1 * inv;
  const int cls = (int)(long long)lab;
  const float g1 = cls == 1 ? 1.f : 0.f, g0 = cls == 0 ? 1.f : 0.f;
  float w0 = 1.f, w1 = 1.f;
  if (hardness) { w0 = 0.6f * fabsf(p0 - g0) + 0.4f; w1 = 0.6f * fabsf(p1 - g1) + 0.4f; }
  t[0] += w0 * g0 * p0; t[1] += w0 * g0; t[2] += w0 * p0;
  t[3] += w1 * g1 * p1; t[4] += w1 * g1; t[5] += w1 * p1;
}

// sums[b][c][0..2] = (I, G, P) of the (optionally hardness-weighted) 2-class soft Dice.  A thread adds four voxels in fp32 and keeps its running sums in fp64.
__global__ __launch_bounds__(DICE_THREADS) void dice_pred_sums_kernel(const float* __restrict__ logits, int pitch, const float* __restrict__ label, int64_t nvox, int hardness, double* __restrict__ sums, unsigned* fxflag) {
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * nvox * pitch;
  const float* lb = label + (int64_t)b * nvox;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if (pitch == 2 && (nvox & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0) {
    const float4* lg4 = reinterpret_cast<const float4*>(lg);
    const float4* lb4 = reinterpret_cast<const float4*>(lb);
    for (int64_t i = tid; i < (nvox >> 2); i += nthr) {
      const float4 a = lg4[2 * i], c = lg4[2 * i + 1], g = lb4[i];
      float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      dice_pred_terms(a.x, a.y, g.x, hardness, t);
      dice_pred_terms(a.z, a.w, g.y, hardness, t);
      dice_pred_terms(c.x, c.y, g.z, hardness, t);
      dice_pred_terms(c.z, c.w, g.w, hardness, t);
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[k] += (double)t[k];
    }
  } else {
    for (int64_t v = tid; v < nvox; v += nthr) {
      const float2 l = *reinterpret_cast<const float2*>(lg + v * pitch);
      float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      dice_pred_terms(l.x, l.y, lb[v], hardness, t);
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[k] += (double)t[k];
    }
  }
  block_reduce_add(acc, 6, sums + (int64_t)b * 6, VSSEG_FX_DICE, fxflag);
}
extern "C" int vsseg_dice_pred_sums(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, double* sums, void* stream) {
  VSSEG_CHECK(logits && label && sums && pitch >= 2 && pitch % 2 == 0 && n >= 1 && nvox >= 1, "vsseg_dice_pred_sums: bad arguments");
  dim3 g(dice_blocks(nvox / 4, n), n);
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_pred_sums");
  hipLaunchKernelGGL(dice_pred_sums_kernel, g, dim3(DICE_THREADS), 0, as_stream(stream), logits, pitch, label, nvox, hardness, sums, fxflag);
  VSSEG_LAUNCH_CHECK("vsseg_dice_pred_sums");
  return VSSEG_OK;
}

// sums[b][0..2] = (I, G, P) of the single-channel Dice between an attention map and the pooled label
__global__ __launch_bounds__(DICE_THREADS) void dice_att_sums_kernel(const float* __restrict__ att, const float* __restrict__ label, int64_t nvox, double* __restrict__ sums, unsigned* fxflag) {
  const int b = blockIdx.y;
  const float* a = att + (int64_t)b * nvox;
  const float* lb = label + (int64_t)b * nvox;
  double acc[3] = {0, 0, 0};
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if ((nvox & 3) == 0 && (reinterpret_cast<uintptr_t>(att) & 15) == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0) {
    const float4* a4 = reinterpret_cast<const float4*>(a);
    const float4* l4 = reinterpret_cast<const float4*>(lb);
    for (int64_t i = tid; i < (nvox >> 2); i += nthr) {
      const float4 p = a4[i], g = l4[i];
      acc[0] += (double)((g.x * p.x + g.y * p.y) + (g.z * p.z + g.w * p.w));
      acc[1] += (double)((g.x + g.y) + (g.z + g.w));
      acc[2] += (double)((p.x + p.y) + (p.z + p.w));
    }
  } else {
    for (int64_t v = tid; v < nvox; v += nthr) {
      const float p = a[v], g = lb[v];
      acc[0] += (double)(g * p); acc[1] += (double)g; acc[2] += (double)p;
    }
  }
  block_reduce_add(acc, 3, sums + (int64_t)b * 3, VSSEG_FX_DICE, fxflag);
}
extern "C" int vsseg_dice_att_sums(const float* att, const float* label, int32_t n, int64_t nvox, double* sums, void* stream) {
  VSSEG_CHECK(att && label && sums && n >= 1 && nvox >= 1, "vsseg_dice_att_sums: bad arguments");
  dim3 g(dice_blocks(nvox / 4, n), n);
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_att_sums");
  hipLaunchKernelGGL(dice_att_sums_kernel, g, dim3(DICE_THREADS), 0, as_stream(stream), att, label, nvox, sums, fxflag);
  VSSEG_LAUNCH_CHECK("vsseg_dice_att_sums");
  return VSSEG_OK;
}

// One pass over one level of the supervision pyramid whose next level pools (2, 2, 1) (the two finest levels of the 2.5D network): the attention-map sums against the
// level's label, the next level's label G' = MaxPool3d((2,2,1))(G) (ref :268-277) and, at the finest level (PRED), the sums of the softmax Dice of the logits — what
// vsseg_dice_pred_sums + vsseg_dice_att_sums + vsseg_maxpool_label do in three passes that read the label three times (0.63 GB instead of 0.43 at 4 x 384x128x128).
// A thread owns a 2 x 2 x 4 block of voxels = four z-quads of one pooling window row: sixteen 16-byte loads in flight, one 16-byte store of pooled labels.
template <bool PRED>
__global__ __launch_bounds__(DICE_THREADS) void dice_level_kernel(const float* __restrict__ logits, const float* __restrict__ att, const float* __restrict__ label, int X, int Y, int Z, int hardness,
                                                                    double* __restrict__ pred_sums, double* __restrict__ att_sums, float* __restrict__ pooled, unsigned* fxflag) {
  const int b = blockIdx.y;
  const int64_t nvox = (int64_t)X * Y * Z;
  const int X2 = X >> 1, Y2 = Y >> 1, Zq = Z >> 2;
  const float4* lg4 = PRED ? reinterpret_cast<const float4*>(logits + (int64_t)b * nvox * 2) : nullptr;
  const float4* at4 = reinterpret_cast<const float4*>(att + (int64_t)b * nvox);
  const float4* lb4 = reinterpret_cast<const float4*>(label + (int64_t)b * nvox);
  float4* po4 = pooled ? reinterpret_cast<float4*>(pooled + (int64_t)b * (nvox >> 2)) : nullptr;
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int64_t items = (int64_t)X2 * Y2 * Zq, nthr = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < items; i += nthr) {
    const int zq = (int)(i % Zq);
    const int64_t r = i / Zq;
    const int y2 = (int)(r % Y2), x2 = (int)(r / Y2);
    float4 g[4], p[4], la[4], lc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t q = ((int64_t)(2 * x2 + (j >> 1)) * Y + 2 * y2 + (j & 1)) * Zq + zq;  // float4 index of the quad
      g[j] = lb4[q];
      p[j] = at4[q];
      if constexpr (PRED) { la[j] = lg4[2 * q]; lc[j] = lg4[2 * q + 1]; }
    }
    float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ai = 0.f, ag = 0.f, ap = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (PRED) {
        dice_pred_terms(la[j].x, la[j].y, g[j].x, hardness, t);
        dice_pred_terms(la[j].z, la[j].w, g[j].y, hardness, t);
        dice_pred_terms(lc[j].x, lc[j].y, g[j].z, hardness, t);
        dice_pred_terms(lc[j].z, lc[j].w, g[j].w, hardness, t);
      }
      ai += (g[j].x * p[j].x + g[j].y * p[j].y) + (g[j].z * p[j].z + g[j].w * p[j].w);
      ag += (g[j].x + g[j].y) + (g[j].z + g[j].w);
      ap += (p[j].x + p[j].y) + (p[j].z + p[j].w);
    }
    if constexpr (PRED) {
#pragma unroll
      for (int k = 0; k < 6; ++k) acc[k] += (double)t[k];
    }
    acc[6] += (double)ai; acc[7] += (double)ag; acc[8] += (double)ap;
    if (po4) {
      float4 m;
      m.x = fmaxf(fmaxf(g[0].x, g[1].x), fmaxf(g[2].x, g[3].x));
      m.y = fmaxf(fmaxf(g[0].y, g[1].y), fmaxf(g[2].y, g[3].y));
      m.z = fmaxf(fmaxf(g[0].z, g[1].z), fmaxf(g[2].z, g[3].z));
      m.w = fmaxf(fmaxf(g[0].w, g[1].w), fmaxf(g[2].w, g[3].w));
      po4[((int64_t)x2 * Y2 + y2) * Zq + zq] = m;
    }
  }
  // (block_reduce_add: threads 0..nvals-1 add one value each — the two groups go to their own buffers in two calls)
  if constexpr (PRED) block_reduce_add(acc, 6, pred_sums + (int64_t)b * 6, VSSEG_FX_DICE, fxflag);
  if constexpr (PRED) __syncthreads();
  block_reduce_add(acc + 6, 3, att_sums + (int64_t)b * 3, VSSEG_FX_DICE, fxflag);
}
extern "C" int vsseg_dice_level_sums(const float* logits, const float* att, const float* label, int32_t n, const int32_t dims[3], int32_t hardness, double* pred_sums, double* att_sums, float* pooled, void* stream) {
  VSSEG_CHECK(att && label && att_sums && n >= 1 && (!logits || pred_sums), "vsseg_dice_level_sums: bad arguments");
  VSSEG_CHECK(dims[0] >= 2 && dims[1] >= 2 && dims[2] >= 4 && dims[0] % 2 == 0 && dims[1] % 2 == 0 && dims[2] % 4 == 0, "vsseg_dice_level_sums: %d x %d x %d is not made of 2 x 2 x 4 blocks", dims[0], dims[1], dims[2]);
  VSSEG_CHECK(((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(att) | reinterpret_cast<uintptr_t>(label) | reinterpret_cast<uintptr_t>(pooled)) & 15) == 0, "vsseg_dice_level_sums: operands must be 16-byte aligned");
  const int64_t items = (int64_t)(dims[0] / 2) * (dims[1] / 2) * (dims[2] / 4);
  dim3 g(dice_blocks(items * 2, n), n);  // (an item is sixteen voxels: twice the loads of the other reductions' eight per thread and round)
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_level_sums");
  if (logits) hipLaunchKernelGGL(dice_level_kernel<true>, g, dim3(DICE_THREADS), 0, as_stream(stream), logits, att, label, dims[0], dims[1], dims[2], hardness, pred_sums, att_sums, pooled, fxflag);
  else hipLaunchKernelGGL(dice_level_kernel<false>, g, dim3(DICE_THREADS), 0, as_stream(stream), logits, att, label, dims[0], dims[1], dims[2], hardness, pred_sums, att_sums, pooled, fxflag);
  VSSEG_LAUNCH_CHECK("vsseg_dice_level_sums");
  return VSSEG_OK;
}

// The coarse levels of the supervision pyramid in ONE launch: level i's label = MaxPool3d(sdims / dims_i)(src) straight from the finest of them (a max-pool of a max-pool
// is the max-pool over the product window) and its attention-map sums.  Level by level this was two launches of a few thousand voxels each, ~6 us apiece whatever their size.
// 1024-thread workgroups: the sums of all levels and samples of this launch share three cache lines and the fixed-point atomics of one LINE retire one after the other:
// a quarter of the workgroups of a 256-thread launch, four times the threads (measured the same 32 us either way: the launch is bound by its dependent loads, not by these)
constexpr int DICE_TAIL_THREADS = 1024;
struct DiceTailK {
  vsseg_dice_tail_desc d;
  int first[VSSEG_DICE_MAX_LEVELS + 1];  // workgroup range of level i: [first[i], first[i+1])
};
__global__ __launch_bounds__(DICE_TAIL_THREADS) void dice_tail_kernel(const DiceTailK k, unsigned* fxflag) {
  const int b = blockIdx.y;
  int l = 0;
  while (l + 1 < k.d.nlevels && (int)blockIdx.x >= k.first[l + 1]) ++l;
  const int nb = k.first[l + 1] - k.first[l], lb = (int)blockIdx.x - k.first[l];
  const int dx = k.d.dims[l][0], dy = k.d.dims[l][1], dz = k.d.dims[l][2];
  const int sx = k.d.sdims[0], sy = k.d.sdims[1], sz = k.d.sdims[2];
  const int rx = sx / dx, ry = sy / dy, rz = sz / dz;
  const int nvox = dx * dy * dz;
  const float* __restrict__ src = k.d.src + (int64_t)b * sx * sy * sz;
  const float* __restrict__ att = k.d.att[l] + (int64_t)b * nvox;
  float* __restrict__ out = k.d.label[l] ? k.d.label[l] + (int64_t)b * nvox : nullptr;
  double acc[3] = {0, 0, 0};
  // T lanes (a power of two <= 64) share the pooling window of one voxel — the coarsest level of the benchmark network pools 8 x 8 x 8 = 512 values per voxel for 768 voxels:
  // one thread per voxel walked them one dependent load after the other (170 us for the launch) — and meet in a butterfly of lane exchanges (max: exact in any order)
  const int win = rx * ry * rz;
  int T = 1;
  while (T < 64 && T * 2 <= win) T *= 2;
  const int vpb = DICE_TAIL_THREADS / T, sub = (int)threadIdx.x % T, slot = (int)threadIdx.x / T;
  const float idz = 1.0f / (float)dz, idy = 1.0f / (float)dy, irz = 1.0f / (float)rz, iry = 1.0f / (float)ry;
  if (win == 1 && (nvox & 3) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(att) | reinterpret_cast<uintptr_t>(out)) & 15) == 0) {
    // the level IS the source level: dice_att_sums_kernel's loop (16-byte loads, no coordinates)
    for (int i = lb * DICE_TAIL_THREADS + (int)threadIdx.x; i < (nvox >> 2); i += nb * DICE_TAIL_THREADS) {
      const float4 g = reinterpret_cast<const float4*>(src)[i], p = reinterpret_cast<const float4*>(att)[i];
      if (out) reinterpret_cast<float4*>(out)[i] = g;
      acc[0] += (double)((g.x * p.x + g.y * p.y) + (g.z * p.z + g.w * p.w));
      acc[1] += (double)((g.x + g.y) + (g.z + g.w));
      acc[2] += (double)((p.x + p.y) + (p.z + p.w));
    }
  } else
  for (int base = lb * vpb * 4; base < nvox; base += nb * vpb * 4) {  // (block-uniform trip count: every lane takes part in the exchanges)
    // four voxels per lane group and round: their loads are issued together (one voxel per round was a chain of dependent ~1 us loads: 8 rounds, 30 us)
    int iv[4];
    float m[4], p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = base + u * vpb + slot;
      iv[u] = i < nvox ? i : -1;
      const int ic = i < nvox ? i : 0, r = vsseg_fdiv(ic, dz, idz), z = ic - r * dz, x = vsseg_fdiv(r, dy, idy), y = r - x * dy;  // (values < 2^22: common.h)
      m[u] = -INFINITY;
      for (int w = sub; w < win; w += T) {
        const int ac = vsseg_fdiv(w, rz, irz), e = w - ac * rz, a = vsseg_fdiv(ac, ry, iry), c = ac - a * ry;
        m[u] = fmaxf(m[u], src[((int64_t)(x * rx + a) * sy + y * ry + c) * sz + z * rz + e]);
      }
      p[u] = att[ic];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      for (int off = T >> 1; off > 0; off >>= 1) m[u] = fmaxf(m[u], __shfl_xor(m[u], off));
      if (iv[u] >= 0 && sub == 0) {
        if (out) out[iv[u]] = m[u];
        acc[0] += (double)(m[u] * p[u]); acc[1] += (double)m[u]; acc[2] += (double)p[u];
      }
    }
  }
  block_reduce_add(acc, 3, k.d.sums + ((int64_t)l * k.d.n + b) * 3, VSSEG_FX_DICE, fxflag);
}
extern "C" int vsseg_dice_tail_sums(const vsseg_dice_tail_desc* d, void* stream) {
  VSSEG_CHECK(d && d->src && d->sums && d->n >= 1 && d->nlevels >= 1 && d->nlevels <= VSSEG_DICE_MAX_LEVELS, "vsseg_dice_tail_sums: bad arguments");
  DiceTailK k;
  k.d = *d;
  int nb = 0;
  for (int l = 0; l < d->nlevels; ++l) {
    VSSEG_CHECK(d->att[l], "vsseg_dice_tail_sums: level %d has no attention map", l);
    bool same = true;
    for (int a = 0; a < 3; ++a) {
      VSSEG_CHECK(d->dims[l][a] >= 1 && d->sdims[a] % d->dims[l][a] == 0, "vsseg_dice_tail_sums: attention pyramid shapes must divide (ref dice_spvPA.py:273)");
      same = same && d->dims[l][a] == d->sdims[a];
    }
    VSSEG_CHECK(d->label[l] || same, "vsseg_dice_tail_sums: level %d pools but has no label buffer", l);
    const int64_t nvox = (int64_t)d->dims[l][0] * d->dims[l][1] * d->dims[l][2];
    VSSEG_CHECK(nvox < (1ll << 22), "vsseg_dice_tail_sums: level %d is too large for the tail launch (>= 2^22 voxels per sample)", l);
    k.first[l] = nb;
    int64_t win = 1, T = 1;
    for (int a = 0; a < 3; ++a) win *= d->sdims[a] / d->dims[l][a];
    while (T < 64 && T * 2 <= win) T *= 2;
    nb += (int)std::min<int64_t>(48, win == 1 ? (nvox + 8191) / 8192 : (nvox * T + 2047) / 2048);  // T lanes per voxel (dice_tail_kernel)
  }
  for (int l = d->nlevels; l <= VSSEG_DICE_MAX_LEVELS; ++l) k.first[l] = nb;
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_tail_sums");
  hipLaunchKernelGGL(dice_tail_kernel, dim3(nb, d->n), dim3(DICE_TAIL_THREADS), 0, as_stream(stream), k, fxflag);
  VSSEG_LAUNCH_CHECK("vsseg_dice_tail_sums");
  return VSSEG_OK;
}

// The voxel-wise cross-entropy term beside the Dice loss (Dice_spvPA(ce_weight=lambda, ce_foreground_weight=w_fg); include/vsseg_hip.h states the formulas):
//   CE = sum_{b,v} w[y] * softplus(x[1-y] - x[y]) / W,  y = ((int)label == 1),  w = (1, w_fg),  W = N_bg + w_fg * N_fg
// = torch's F.cross_entropy(logits, y, weight=[1, w_fg]).  softplus(z) = max(z, 0) + log1p(exp(-|z|)) is -log softmax(x)[y] without the overflow of -log(p_y) once p_y
// underflows.  sums[0..2] = (S_bg, S_fg, N_fg) of the whole batch: the CE sums over the background and the foreground voxels and the foreground count.
// Scale: VSSEG_FX_STAT (2^20), NOT VSSEG_FX_DICE — a voxel's value is |z|, not bounded by 1: at batch 4 of 384x128x128 with every |z| = 100 a workgroup (1/512 of the
// voxels) adds 4.9e6, beyond the 1.0e6 that 2^32 leaves room for and far inside the 4.3e9 of 2^20; the total (2.5e9) stays below 2^63 / 2^20 = 8.8e12.  The resolution,
// 2^-20 per workgroup (rounded to nearest) and 512 workgroups at most, is 2.4e-4 on a sum that is divided by W >= the number of voxels.
__device__ __forceinline__ void ce_terms(float l0, float l1, float lab, float* t) {
  const bool fg = (int)(long long)lab == 1;
  const float z = fg ? l0 - l1 : l1 - l0;
  // log1p(e), e = exp(-|z|) in (0, 1]: e - e^2 / 2 below 2^-12 (the next term, e^3 / 3, is below 2^-26 e), log(1 + e) above it, where rounding 1 + e costs at most
  // 2^-24 absolute — a library log1pf made the pass compute-bound (99 us against the 51 us of vsseg_dice_pred_sums over the same bytes).  A NaN logit: NaN through it.
  const float e = __expf(-fabsf(z));
  const float v = (z > 0.f ? z : 0.f) + (e < 0x1p-12f ? e * (1.f - 0.5f * e) : __logf(1.f + e));
  t[0] += fg ? 0.f : v; t[1] += fg ? v : 0.f; t[2] += fg ? 1.f : 0.f;
}
// The focal cross-entropy (vsseg_ce_focal_sums; include/vsseg_hip.h states the formulas): a voxel's value is w[y] * q^gamma * softplus(z), q = sigmoid(z) = 1 - p_y.
// The two parts that the sums pass and the backward share, from z and e = exp(-|z|): sp = softplus(z) as ce_terms forms it and qg = q^gamma = exp(-gamma * softplus(-z))
// with softplus(-z) = max(-z, 0) + log1p(e) — no log of a rounded probability: at z = -200 the exponent is -200 gamma and qg underflows to 0, at z = +200 it is
// -gamma e = 0 and qg is 1.  One logarithm and one exponential per voxel beyond the plain term's.  A NaN logit: NaN through both.
struct CeFocalParts { float sp, qg; };
__device__ __forceinline__ CeFocalParts ce_focal_parts(float z, float e, float gamma) {
  const float l1p = e < 0x1p-12f ? e * (1.f - 0.5f * e) : __logf(1.f + e);
  CeFocalParts r;
  r.sp = (z > 0.f ? z : 0.f) + l1p;
  r.qg = __expf(-gamma * ((z < 0.f ? -z : 0.f) + l1p));
  return r;
}
__device__ __forceinline__ void ce_focal_terms(float l0, float l1, float lab, float gamma, float* t) {
  const bool fg = (int)(long long)lab == 1;
  const float z = fg ? l0 - l1 : l1 - l0;
  const CeFocalParts f = ce_focal_parts(z, __expf(-fabsf(z)), gamma);
  const float v = f.qg * f.sp;
  t[0] += fg ? 0.f : v; t[1] += fg ? v : 0.f; t[2] += fg ? 1.f : 0.f;
}
// dice_pred_sums_kernel's launch shape and its two paths; a thread adds four voxels in fp32 and keeps its running sums in fp64.  FOCAL: the values of ce_focal_terms
template <bool FOCAL>
__global__ __launch_bounds__(DICE_THREADS) void ce_sums_kernel(const float* __restrict__ logits, int pitch, const float* __restrict__ label, int64_t nvox, double* __restrict__ sums, unsigned* fxflag, float gamma) {
  auto ce_terms = [gamma](float l0, float l1, float lab, float* t) {
    if constexpr (FOCAL) ce_focal_terms(l0, l1, lab, gamma, t);
    else ::ce_terms(l0, l1, lab, t);
  };
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * nvox * pitch;
  const float* lb = label + (int64_t)b * nvox;
  double acc[3] = {0, 0, 0};
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if (pitch == 2 && (nvox & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0) {
    const float4* lg4 = reinterpret_cast<const float4*>(lg);
    const float4* lb4 = reinterpret_cast<const float4*>(lb);
    for (int64_t i = tid; i < (nvox >> 2); i += nthr) {
      const float4 a = lg4[2 * i], c = lg4[2 * i + 1], g = lb4[i];
      float t[3] = {0.f, 0.f, 0.f};
      ce_terms(a.x, a.y, g.x, t);
      ce_terms(a.z, a.w, g.y, t);
      ce_terms(c.x, c.y, g.z, t);
      ce_terms(c.z, c.w, g.w, t);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += (double)t[k];
    }
  } else {
    for (int64_t v = tid; v < nvox; v += nthr) {
      const float2 l = *reinterpret_cast<const float2*>(lg + v * pitch);
      float t[3] = {0.f, 0.f, 0.f};
      ce_terms(l.x, l.y, lb[v], t);
#pragma unroll
      for (int k = 0; k < 3; ++k) acc[k] += (double)t[k];
    }
  }
  block_reduce_add(acc, 3, sums, VSSEG_FX_STAT, fxflag);  // (one mean over the batch: every sample adds to the same three slots)
}
extern "C" int vsseg_ce_sums(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, double* sums, void* stream) {
  VSSEG_CHECK(logits && label && sums && pitch >= 2 && pitch % 2 == 0 && n >= 1 && nvox >= 1, "vsseg_ce_sums: bad arguments");
  dim3 g(dice_blocks(nvox / 4, n), n);
  VSSEG_FX_FLAG(fxflag, "vsseg_ce_sums");
  hipLaunchKernelGGL(ce_sums_kernel<false>, g, dim3(DICE_THREADS), 0, as_stream(stream), logits, pitch, label, nvox, sums, fxflag, 0.f);
  VSSEG_LAUNCH_CHECK("vsseg_ce_sums");
  return VSSEG_OK;
}
static bool ce_focal_gamma_ok(double g) { return g >= 0.0 && g <= 5.0; }  // (a NaN fails both)
extern "C" int vsseg_ce_focal_sums(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, double ce_focal_gamma, double* sums, void* stream) {
  VSSEG_CHECK(logits && label && sums && pitch >= 2 && pitch % 2 == 0 && n >= 1 && nvox >= 1, "vsseg_ce_focal_sums: bad arguments");
  VSSEG_CHECK(ce_focal_gamma_ok(ce_focal_gamma), "vsseg_ce_focal_sums: ce_focal_gamma must be in [0, 5]");
  dim3 g(dice_blocks(nvox / 4, n), n);
  VSSEG_FX_FLAG(fxflag, "vsseg_ce_focal_sums");
  hipLaunchKernelGGL(ce_sums_kernel<true>, g, dim3(DICE_THREADS), 0, as_stream(stream), logits, pitch, label, nvox, sums, fxflag, (float)ce_focal_gamma);
  VSSEG_LAUNCH_CHECK("vsseg_ce_focal_sums");
  return VSSEG_OK;
}

// loss = mean_{b,c} f_pred + sum_l (1/L) mean_b f_att,  f = 1 - (2I+eps)/(G+P+eps).  coef holds d(loss)/dI and d(loss)/dG(=dP).
// With `ce_sums` (vsseg_dice_ce_finalize): + ce_weight * (S_bg + w_fg * S_fg) / W, added in fp64 before the one cast, and ce_coef = (ce_weight / W, ce_weight * w_fg / W),
// W = (voxels - N_fg) + w_fg * N_fg — the backward reads the two from device memory: no host read of N_fg.
// With `topk` (vsseg_dice_ce_topk_finalize; the record of vsseg_ce_topk_select, topk.h): + ce_weight * (S_gt + (K - n_gt) * t) / K, S_gt = s_above + s_tail, and
// topk_coef = (ce_weight / K, ce_weight * w_fg / K, the tie share (K - n_gt) / n_eq, the threshold's bits, w_fg as the select rounded it) — the division is by K, not by W.
// With `region` (vsseg_loss_finalize: the Tversky ratio, its focal exponent, pooling over the batch; include/vsseg_hip.h states the formulas) a logits ratio leaves THREE
// coefficients, coef[b][c][0..2] = d(loss)/d(I, G, P); an attention-map ratio keeps (d/dI, d/dP) — its G is the label.  A pooled ratio writes its coefficients once per sample.
struct DiceRegionK { int on, pool; double beta, gamma; };
// one ratio of weight `wgt` from its three sums: its term, and c[0..2] = d(wgt * term)/d(I, G, P)
__device__ __forceinline__ double region_ratio(double I, double G, double P, double aP, double aG, double gamma, double wgt, double poison, double* c) {
  const double D = 2.0 * aP * P + 2.0 * aG * G + SMOOTH + poison * 0.0, num = 2.0 * I + SMOOTH;  // (+ NaN when poisoned: the coefficients too)
  const double u = 1.0 - num / D;
  double term = u, d = wgt;
  if (gamma != 1.0) {  // max(u, 1e-7)^gamma: constant below the floor
    const bool floored = u < 1e-7;
    term = floored ? pow(1e-7, gamma) : pow(u, gamma);
    d = floored ? 0.0 : wgt * gamma * pow(u, gamma - 1.0);
  }
  c[0] = -2.0 / D * d;
  c[1] = num * 2.0 * aG / (D * D) * d;
  c[2] = num * 2.0 * aP / (D * D) * d;
  return wgt * term;
}
__global__ void dice_finalize_kernel(const double* pred_sums, const double* att_sums, int n, int nlevels, float* loss, float* coef, const unsigned* fxflag,
                                     const double* ce_sums, double voxels, double ce_weight, double ce_fg_weight, float* ce_coef, const TopkRec* topk, float* topk_coef, const DiceRegionK region) {
  if (blockIdx.x != 0) return;
  __shared__ double region_part[64];  // (every launch of this kernel has 64 threads)
  if (region.on) {
    // a ratio per thread — the fp64 powers of the focal exponent, one after the other in one thread, were 10 us of the loss phase — and their terms added in thread order below
    const double poison = vsseg_fx_poison(fxflag), alpha = 1.0 - region.beta;
    const int groups = region.pool ? 1 : n, per = region.pool ? n : 1;  // a ratio is formed over `per` samples
    double part = 0.0;
    for (int r = threadIdx.x; r < (2 + nlevels) * groups; r += 64) {
      const bool pred = r < 2 * groups;
      const int l = pred ? 0 : (r - 2 * groups) / groups, q = pred ? r / 2 : (r - 2 * groups) % groups, c = pred ? r % 2 : 1;  // (an attention map weighs like the foreground class)
      double s[3] = {0.0, 0.0, 0.0}, k[3];
      for (int b = q * per; b < (q + 1) * per; ++b)
        for (int j = 0; j < 3; ++j) s[j] += vsseg_fx_get((pred ? pred_sums + (b * 2 + c) * 3 : att_sums + (l * n + b) * 3) + j, VSSEG_FX_DICE);
      part += region_ratio(s[0], s[1], s[2], c == 1 ? alpha : region.beta, c == 1 ? region.beta : alpha, region.gamma, 1.0 / ((pred ? 2.0 : (double)nlevels) * groups), poison, k);
      for (int b = q * per; b < (q + 1) * per; ++b) {
        if (pred) {
          for (int j = 0; j < 3; ++j) coef[(b * 2 + c) * 3 + j] = (float)k[j];
        } else {
          coef[n * 6 + (l * n + b) * 2 + 0] = (float)k[0];
          coef[n * 6 + (l * n + b) * 2 + 1] = (float)k[2];
        }
      }
    }
    region_part[threadIdx.x] = part;
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double total = vsseg_fx_poison(fxflag);  // NaN while a partial sum of this process was non-finite / out of range (common.h)
  if (region.on) {
    for (int t = 0; t < 64; ++t) total += region_part[t];
  } else {
  for (int b = 0; b < n; ++b)
    for (int c = 0; c < 2; ++c) {
      const double* sp = pred_sums + (b * 2 + c) * 3;
      const double s[3] = {vsseg_fx_get(sp, VSSEG_FX_DICE), vsseg_fx_get(sp + 1, VSSEG_FX_DICE), vsseg_fx_get(sp + 2, VSSEG_FX_DICE)};
      double D = s[1] + s[2] + SMOOTH + total * 0.0, num = 2.0 * s[0] + SMOOTH, wgt = 1.0 / (2.0 * n);  // (+ NaN when poisoned: the coefficients too)
      total += wgt * (1.0 - num / D);
      coef[(b * 2 + c) * 2 + 0] = (float)(-2.0 / D * wgt);
      coef[(b * 2 + c) * 2 + 1] = (float)(num / (D * D) * wgt);
    }
  for (int l = 0; l < nlevels; ++l)
    for (int b = 0; b < n; ++b) {
      const double* sp = att_sums + (l * n + b) * 3;
      const double s[3] = {vsseg_fx_get(sp, VSSEG_FX_DICE), vsseg_fx_get(sp + 1, VSSEG_FX_DICE), vsseg_fx_get(sp + 2, VSSEG_FX_DICE)};
      double D = s[1] + s[2] + SMOOTH + total * 0.0, num = 2.0 * s[0] + SMOOTH, wgt = 1.0 / ((double)nlevels * n);
      total += wgt * (1.0 - num / D);
      coef[n * 4 + (l * n + b) * 2 + 0] = (float)(-2.0 / D * wgt);
      coef[n * 4 + (l * n + b) * 2 + 1] = (float)(num / (D * D) * wgt);
    }
  }
  if (ce_sums) {
    const double sbg = vsseg_fx_get(ce_sums, VSSEG_FX_STAT), sfg = vsseg_fx_get(ce_sums + 1, VSSEG_FX_STAT), nfg = vsseg_fx_get(ce_sums + 2, VSSEG_FX_STAT);
    const double W = (voxels - nfg) + ce_fg_weight * nfg + total * 0.0;  // (+ NaN when poisoned: the coefficients too)
    total += ce_weight * (sbg + ce_fg_weight * sfg) / W;
    ce_coef[0] = (float)(ce_weight / W);
    ce_coef[1] = (float)(ce_weight * ce_fg_weight / W);
  }
  if (topk) {
    const double K = (double)topk->k + total * 0.0, ngt = (double)topk->n_gt, neq = (double)topk->n_eq;  // (+ NaN when poisoned: the coefficients too)
    const double t = (double)__uint_as_float(topk->threshold_bits);
    const double rest = K - ngt;  // what the elements at the threshold share: 1 <= rest <= n_eq
    total += ce_weight * ((vsseg_fx_get(&topk->s_above, VSSEG_FX_STAT) + topk->s_tail) + rest * t) / K;
    topk_coef[0] = (float)(ce_weight / K);
    topk_coef[1] = (float)(ce_weight * ce_fg_weight / K);
    topk_coef[2] = (float)(rest / neq);
    const bool poisoned = *fxflag != 0u;  // (then the threshold and the weight are NaN patterns as well: every coefficient is)
    reinterpret_cast<unsigned*>(topk_coef)[3] = poisoned ? 0xFFFFFFFFu : topk->threshold_bits;
    topk_coef[4] = poisoned ? __uint_as_float(0x7FC00000u) : (float)ce_fg_weight;
    topk_coef[5] = topk_coef[6] = topk_coef[7] = 0.f;
  }
  *loss = (float)total;
}
extern "C" int vsseg_dice_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, float* loss, float* coef, void* stream) {
  VSSEG_CHECK(pred_sums && loss && coef && (nlevels == 0 || att_sums), "vsseg_dice_finalize: bad arguments");
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_finalize");
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), pred_sums, att_sums, n, nlevels, loss, coef, fxflag, (const double*)nullptr, 0.0, 0.0, 0.0, (float*)nullptr, (const TopkRec*)nullptr, (float*)nullptr, DiceRegionK{0, 0, 0.5, 1.0});
  VSSEG_LAUNCH_CHECK("vsseg_dice_finalize");
  return VSSEG_OK;
}
extern "C" int vsseg_dice_ce_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, const double* ce_sums, int64_t nvox, double ce_weight, double ce_foreground_weight, float* loss, float* coef,
                                      float* ce_coef, void* stream) {
  VSSEG_CHECK(pred_sums && loss && coef && (nlevels == 0 || att_sums) && ce_sums && ce_coef && n >= 1 && nvox >= 1, "vsseg_dice_ce_finalize: bad arguments");
  VSSEG_CHECK(ce_weight >= 0.0 && ce_weight < INFINITY && ce_foreground_weight > 0.0 && ce_foreground_weight < INFINITY, "vsseg_dice_ce_finalize: ce_weight must be finite and >= 0, ce_foreground_weight finite and > 0");
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_ce_finalize");
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), pred_sums, att_sums, n, nlevels, loss, coef, fxflag, ce_sums, (double)n * (double)nvox, ce_weight, ce_foreground_weight, ce_coef, (const TopkRec*)nullptr, (float*)nullptr, DiceRegionK{0, 0, 0.5, 1.0});
  VSSEG_LAUNCH_CHECK("vsseg_dice_ce_finalize");
  return VSSEG_OK;
}
extern "C" int vsseg_dice_ce_topk_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, const void* topk_scratch, double ce_weight, double ce_foreground_weight, float* loss, float* coef,
                                           float* topk_coef, void* stream) {
  VSSEG_CHECK(pred_sums && loss && coef && (nlevels == 0 || att_sums) && topk_scratch && topk_coef && n >= 1, "vsseg_dice_ce_topk_finalize: bad arguments");
  VSSEG_CHECK(ce_weight >= 0.0 && ce_weight < INFINITY && ce_foreground_weight > 0.0 && ce_foreground_weight < INFINITY, "vsseg_dice_ce_topk_finalize: ce_weight must be finite and >= 0, ce_foreground_weight finite and > 0");
  VSSEG_FX_FLAG(fxflag, "vsseg_dice_ce_topk_finalize");
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), pred_sums, att_sums, n, nlevels, loss, coef, fxflag, (const double*)nullptr, 0.0, ce_weight, ce_foreground_weight, (float*)nullptr,
                     reinterpret_cast<const TopkRec*>(topk_scratch), topk_coef, DiceRegionK{0, 0, 0.5, 1.0});
  VSSEG_LAUNCH_CHECK("vsseg_dice_ce_topk_finalize");
  return VSSEG_OK;
}
// the range checks of a vsseg_loss_opts record, before any launch (comparisons that a NaN fails)
static int loss_opts_check(const vsseg_loss_opts* o, const char* who) {
  VSSEG_CHECK(o, "%s: no options record", who);
  VSSEG_CHECK((o->region == 0 || o->region == 1) && (o->batch_dice == 0 || o->batch_dice == 1) && o->reserved == 0, "%s: region and batch_dice are 0 or 1, reserved is 0", who);
  VSSEG_CHECK(o->region || !o->batch_dice, "%s: batch_dice needs region = 1", who);
  if (o->region) {
    VSSEG_CHECK(o->tversky_beta > 0.0 && o->tversky_beta < 1.0, "%s: tversky_beta must be in (0, 1)", who);
    VSSEG_CHECK(o->focal_tversky_gamma >= 0.25 && o->focal_tversky_gamma <= 4.0, "%s: focal_tversky_gamma must be in [0.25, 4]", who);
  }
  VSSEG_CHECK(o->ce_mode >= VSSEG_CE_NONE && o->ce_mode <= VSSEG_CE_FOCAL, "%s: ce_mode %d is none of VSSEG_CE_*", who, o->ce_mode);
  if (o->ce_mode != VSSEG_CE_NONE)
    VSSEG_CHECK(o->ce_weight >= 0.0 && o->ce_weight < INFINITY && o->ce_foreground_weight > 0.0 && o->ce_foreground_weight < INFINITY, "%s: ce_weight must be finite and >= 0, ce_foreground_weight finite and > 0", who);
  if (o->ce_mode == VSSEG_CE_FOCAL) VSSEG_CHECK(ce_focal_gamma_ok(o->ce_focal_gamma), "%s: ce_focal_gamma must be in [0, 5]", who);
  return VSSEG_OK;
}
extern "C" int vsseg_loss_finalize(const double* pred_sums, const double* att_sums, int32_t n, int32_t nlevels, const void* ce_state, int64_t nvox, const vsseg_loss_opts* opts, float* loss, float* coef, float* ce_coef,
                                   void* stream) {
  VSSEG_CHECK(pred_sums && loss && coef && (nlevels == 0 || att_sums) && n >= 1 && nlevels >= 0 && nvox >= 1, "vsseg_loss_finalize: bad arguments");
  if (loss_opts_check(opts, "vsseg_loss_finalize") != VSSEG_OK) return VSSEG_EINVAL;
  VSSEG_CHECK(opts->ce_mode == VSSEG_CE_NONE || (ce_state && ce_coef), "vsseg_loss_finalize: the cross-entropy term needs its sums (or the select's record) and ce_coef");
  const bool topk = opts->ce_mode == VSSEG_CE_TOPK, sums = opts->ce_mode == VSSEG_CE_PLAIN || opts->ce_mode == VSSEG_CE_FOCAL;  // (the focal sums decode like the plain ones)
  VSSEG_FX_FLAG(fxflag, "vsseg_loss_finalize");
  hipLaunchKernelGGL(dice_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), pred_sums, att_sums, n, nlevels, loss, coef, fxflag, sums ? reinterpret_cast<const double*>(ce_state) : nullptr,
                     (double)n * (double)nvox, opts->ce_weight, opts->ce_foreground_weight, sums ? ce_coef : nullptr, topk ? reinterpret_cast<const TopkRec*>(ce_state) : nullptr, topk ? ce_coef : nullptr,
                     DiceRegionK{opts->region, opts->batch_dice, opts->tversky_beta, opts->focal_tversky_gamma});
  VSSEG_LAUNCH_CHECK("vsseg_loss_finalize");
  return VSSEG_OK;
}

// d(loss)/d(logits) of one voxel: through the Dice sums, the (non-detached) hardness weight (ref :279-283) and the softmax
// CE: + the gradient of the cross-entropy term of the voxel, k * w[y] * (softmax(x) - onehot(y)) with kbg = k * w[0], kfg = k * w[1] (vsseg_dice_ce_finalize's ce_coef),
// formed from the OTHER class's probability — (+kfg p0, -kfg p0) for y = 1, (-kbg p1, +kbg p1) for y = 0: p_y - 1 cancels once p_y rounds to 1 — and added in fp32
// SPLIT (the region options of vsseg_loss_finalize): G and P have coefficients of their own, (B, P) = d(loss)/d(G, P) — A g t + B g s + P t
// CE 3: the focal cross-entropy — dz = k w[y] q^gamma (gamma (1 - q) softplus(z) + q) to the other class's logit, -dz to the label's own (ce_focal_parts)
template <int CE, bool SPLIT = false> __device__ __forceinline__ float2 dice_pred_grad(float l0, float l1, float lab, int hardness, float A0, float B0, float A1, float B1, float kbg, float kfg, float P0 = 0.f, float P1 = 0.f,
                                                                                       float fgamma = 0.f) {
  const float m = fmaxf(l0, l1), e0 = __expf(l0 - m), e1 = __expf(l1 - m), inv = 1.f / (e0 + e1);
  const float p0 = e0 * inv, p1 = e1 * inv;
  const int cls = (int)(long long)lab;
  const float g1 = cls == 1 ? 1.f : 0.f, g0 = cls == 0 ? 1.f : 0.f;
  float w0 = 1.f, w1 = 1.f, s0 = 0.f, s1 = 0.f;
  if (hardness) {
    const float d0 = p0 - g0, d1 = p1 - g1;
    w0 = 0.6f * fabsf(d0) + 0.4f; w1 = 0.6f * fabsf(d1) + 0.4f;
    s0 = d0 > 0.f ? 0.6f : (d0 < 0.f ? -0.6f : 0.f);
    s1 = d1 > 0.f ? 0.6f : (d1 < 0.f ? -0.6f : 0.f);
  }
  const float t0 = w0 + p0 * s0, t1 = w1 + p1 * s1;  // d(w*p)/dp
  float dp0, dp1;
  if constexpr (SPLIT) {
    dp0 = A0 * g0 * t0 + B0 * g0 * s0 + P0 * t0;
    dp1 = A1 * g1 * t1 + B1 * g1 * s1 + P1 * t1;
  } else {
    dp0 = A0 * g0 * t0 + B0 * (g0 * s0 + t0);
    dp1 = A1 * g1 * t1 + B1 * (g1 * s1 + t1);
  }
  const float dot = dp0 * p0 + dp1 * p1;
  float2 r = make_float2(p0 * (dp0 - dot), p1 * (dp1 - dot));
  if constexpr (CE == 3) {
    // q = sigmoid(z) and 1 - q = p_y are the softmax probabilities above, and exp(-|z|) is the smaller of e0, e1 (the other is exp(0) = 1)
    const CeFocalParts f = ce_focal_parts(cls == 1 ? l0 - l1 : l1 - l0, fminf(e0, e1), fgamma);
    const float q = cls == 1 ? p0 : p1, py = cls == 1 ? p1 : p0;
    const float dz = f.qg * (fgamma * py * f.sp + q);
    const float c = cls == 1 ? kfg * dz : -(kbg * dz);
    r.x += c; r.y -= c;
  } else if constexpr (CE != 0) {
    const float c = cls == 1 ? kfg * p0 : -(kbg * p1);
    r.x += c; r.y -= c;
  }
  return r;
}
// OUT 0: fp32 [voxel][2];  1: bf16 [voxel][2] (the compact operand of the marching backward kernels);  2: bf16 rows of 8 channels, channels 2..7 written as zeros;
// 3: fp32, any pitch (channels >= 2 are not touched).  1-3 are the layouts the training plan stages the gradient in (vsseg_dice_pred_bwd_to): written here, the
// fp32 tensor and the cast pass over it (0.3 GB read + written per step at 4 x 384x128x128) do not exist.  Same values: the cast was the same round-to-nearest-even.
// CE: the cross-entropy gradient is formed here as well (vsseg_dice_ce_pred_bwd / _to) and the sum is stored once — a second pass would round the bf16 operand twice.
// CE 2 (the top-k term, vsseg_dice_ce_topk_pred_bwd / _to): the voxel's cross-entropy gradient times c = 1 above the threshold, the tie share at it, 0 below it — its value
// is recomputed by the one function of topk.h and its KEY is compared with the threshold's bits, as the select counted it.
// CE 3 (the focal term, vsseg_loss_pred_bwd / _to): fgamma is the exponent, a kernel argument.  SPLIT: coef holds three per ratio, (A, B, P) = d(loss)/d(I, G, P).
template <int CE, bool SPLIT> __device__ __forceinline__ float2 dice_pred_grad_of(float l0, float l1, float lab, int hardness, float A0, float B0, float A1, float B1, float kbg, float kfg, float share, unsigned tbits, float wfg,
                                                                                  float P0, float P1, float fgamma) {
  if constexpr (CE == 2) {
    const unsigned u = topk_key(ce_topk_value(l0, l1, lab, wfg));
    const float c = u > tbits ? 1.f : (u == tbits ? share : 0.f);
    return dice_pred_grad<1, SPLIT>(l0, l1, lab, hardness, A0, B0, A1, B1, kbg * c, kfg * c, P0, P1);
  } else {
    return dice_pred_grad<CE, SPLIT>(l0, l1, lab, hardness, A0, B0, A1, B1, kbg, kfg, P0, P1, fgamma);
  }
}
template <int OUT, int CE, bool SPLIT> __global__ __launch_bounds__(256) void dice_pred_bwd_kernel(const float* __restrict__ logits, int pitch, const float* __restrict__ label, int64_t nvox, int hardness, const float* __restrict__ coef,
                                                                                                      const float* __restrict__ gscale, void* __restrict__ dst, int dpitch, const float* __restrict__ ce_coef, float fgamma) {
  const int b = blockIdx.y;
  const float* lg = logits + (int64_t)b * nvox * pitch;
  const float* lb = label + (int64_t)b * nvox;
  const float gs = gscale ? *gscale : 1.f;
  constexpr int NC = SPLIT ? 3 : 2;  // coefficients per ratio
  const float A0 = coef[(b * 2 + 0) * NC] * gs, B0 = coef[(b * 2 + 0) * NC + 1] * gs, A1 = coef[(b * 2 + 1) * NC] * gs, B1 = coef[(b * 2 + 1) * NC + 1] * gs;
  float P0 = 0.f, P1 = 0.f;
  if constexpr (SPLIT) { P0 = coef[(b * 2 + 0) * 3 + 2] * gs; P1 = coef[(b * 2 + 1) * 3 + 2] * gs; }
  float kbg = 0.f, kfg = 0.f;
  float share = 0.f, wfg = 1.f;
  unsigned tbits = 0u;
  if constexpr (CE != 0) { kbg = ce_coef[0] * gs; kfg = ce_coef[1] * gs; }
  if constexpr (CE == 2) { share = ce_coef[2]; tbits = reinterpret_cast<const unsigned*>(ce_coef)[3]; wfg = ce_coef[4]; }  // (vsseg_dice_ce_topk_finalize's topk_coef)
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  auto store = [&](int64_t v, float2 g) {
    const int64_t e = ((int64_t)b * nvox + v) * dpitch;
    if constexpr (OUT == 1) *reinterpret_cast<unsigned*>(reinterpret_cast<bf16_t*>(dst) + e) = f2bf2(g.x, g.y);
    else if constexpr (OUT == 2) *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(dst) + e) = make_uint4(f2bf2(g.x, g.y), 0u, 0u, 0u);
    else *reinterpret_cast<float2*>(reinterpret_cast<float*>(dst) + e) = g;
  };
  if (pitch == 2 && (nvox & 3) == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const float4* lg4 = reinterpret_cast<const float4*>(lg);
    const float4* lb4 = reinterpret_cast<const float4*>(lb);
    for (int64_t i = tid; i < (nvox >> 2); i += nthr) {
      const float4 a = lg4[2 * i], c = lg4[2 * i + 1], g = lb4[i];
      const float2 r0 = dice_pred_grad_of<CE, SPLIT>(a.x, a.y, g.x, hardness, A0, B0, A1, B1, kbg, kfg, share, tbits, wfg, P0, P1, fgamma), r1 = dice_pred_grad_of<CE, SPLIT>(a.z, a.w, g.y, hardness, A0, B0, A1, B1, kbg, kfg, share, tbits, wfg, P0, P1, fgamma);
      const float2 r2 = dice_pred_grad_of<CE, SPLIT>(c.x, c.y, g.z, hardness, A0, B0, A1, B1, kbg, kfg, share, tbits, wfg, P0, P1, fgamma), r3 = dice_pred_grad_of<CE, SPLIT>(c.z, c.w, g.w, hardness, A0, B0, A1, B1, kbg, kfg, share, tbits, wfg, P0, P1, fgamma);
      if constexpr (OUT == 0) {
        float4* o = reinterpret_cast<float4*>(reinterpret_cast<float*>(dst) + ((int64_t)b * nvox + 4 * i) * 2);
        o[0] = make_float4(r0.x, r0.y, r1.x, r1.y);
        o[1] = make_float4(r2.x, r2.y, r3.x, r3.y);
      } else if constexpr (OUT == 1) {
        *reinterpret_cast<uint4*>(reinterpret_cast<bf16_t*>(dst) + ((int64_t)b * nvox + 4 * i) * 2) = make_uint4(f2bf2(r0.x, r0.y), f2bf2(r1.x, r1.y), f2bf2(r2.x, r2.y), f2bf2(r3.x, r3.y));
      } else {
        store(4 * i, r0); store(4 * i + 1, r1); store(4 * i + 2, r2); store(4 * i + 3, r3);
      }
    }
  } else {
    for (int64_t v = tid; v < nvox; v += nthr) {
      const float2 l = *reinterpret_cast<const float2*>(lg + v * pitch);
      store(v, dice_pred_grad_of<CE, SPLIT>(l.x, l.y, lb[v], hardness, A0, B0, A1, B1, kbg, kfg, share, tbits, wfg, P0, P1, fgamma));
    }
  }
}
template <int CE, bool SPLIT = false>
static int dice_pred_bwd_launch(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const float* gscale, void* dst, int out, int dpitch,
                                void* stream, const char* who, float fgamma = 0.f) {
  VSSEG_CHECK(logits && label && coef && dst && pitch >= 2 && pitch % 2 == 0 && n >= 1 && nvox >= 1 && (!CE || ce_coef), "%s: bad arguments", who);
  dim3 g(grid_for((nvox + 3) / 4, 256, 2048), n), t(256);
  hipStream_t s = as_stream(stream);
  if (out == 0) hipLaunchKernelGGL((dice_pred_bwd_kernel<0, CE, SPLIT>), g, t, 0, s, logits, pitch, label, nvox, hardness, coef, gscale, dst, 2, ce_coef, fgamma);
  else if (out == 1) hipLaunchKernelGGL((dice_pred_bwd_kernel<1, CE, SPLIT>), g, t, 0, s, logits, pitch, label, nvox, hardness, coef, gscale, dst, 2, ce_coef, fgamma);
  else if (out == 2) hipLaunchKernelGGL((dice_pred_bwd_kernel<2, CE, SPLIT>), g, t, 0, s, logits, pitch, label, nvox, hardness, coef, gscale, dst, 8, ce_coef, fgamma);
  else hipLaunchKernelGGL((dice_pred_bwd_kernel<3, CE, SPLIT>), g, t, 0, s, logits, pitch, label, nvox, hardness, coef, gscale, dst, dpitch, ce_coef, fgamma);
  VSSEG_LAUNCH_CHECK(who);
  return VSSEG_OK;
}
// the layout (OUT of dice_pred_bwd_kernel) a staged destination asks for, or -1 with the error set
static int dice_pred_bwd_layout(const vsseg_tensor& dst, int32_t n, int64_t nvox, const char* who) {
  if (!(dst.ptr && !dst.ptr2 && dst.c == 2 && dst.pitch >= 2 && tensor_voxels(dst) == (int64_t)n * nvox)) {
    vsseg_set_error("%s: destination is not a 2-channel tensor of %lld voxels", who, (long long)n * nvox);
    return -1;
  }
  if (dst.dtype == VSSEG_BF16 && dst.pitch == 2) return 1;
  if (dst.dtype == VSSEG_BF16 && dst.pitch == 8 && (reinterpret_cast<uintptr_t>(dst.ptr) & 15) == 0) return 2;
  if (dst.dtype == VSSEG_F32 && dst.pitch % 2 == 0) return dst.pitch == 2 ? 0 : 3;
  vsseg_set_error("%s: destination layout (dtype %d, pitch %d) is not one the training plan stages the gradient in", who, dst.dtype, dst.pitch);
  return -1;
}
extern "C" int vsseg_dice_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* gscale, float* dlogits, void* stream) {
  return dice_pred_bwd_launch<0>(logits, pitch, label, n, nvox, hardness, coef, nullptr, gscale, dlogits, 0, 2, stream, "vsseg_dice_pred_bwd");
}
extern "C" int vsseg_dice_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* gscale, vsseg_tensor dst, void* stream) {
  const int out = dice_pred_bwd_layout(dst, n, nvox, "vsseg_dice_pred_bwd_to");
  if (out < 0) return VSSEG_EINVAL;
  return dice_pred_bwd_launch<0>(logits, pitch, label, n, nvox, hardness, coef, nullptr, gscale, dst.ptr, out, dst.pitch, stream, "vsseg_dice_pred_bwd_to");
}
extern "C" int vsseg_dice_ce_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const float* gscale, float* dlogits,
                                      void* stream) {
  return dice_pred_bwd_launch<1>(logits, pitch, label, n, nvox, hardness, coef, ce_coef, gscale, dlogits, 0, 2, stream, "vsseg_dice_ce_pred_bwd");
}
extern "C" int vsseg_dice_ce_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const float* gscale, vsseg_tensor dst,
                                         void* stream) {
  const int out = dice_pred_bwd_layout(dst, n, nvox, "vsseg_dice_ce_pred_bwd_to");
  if (out < 0) return VSSEG_EINVAL;
  return dice_pred_bwd_launch<1>(logits, pitch, label, n, nvox, hardness, coef, ce_coef, gscale, dst.ptr, out, dst.pitch, stream, "vsseg_dice_ce_pred_bwd_to");
}
extern "C" int vsseg_dice_ce_topk_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* topk_coef, const float* gscale, float* dlogits,
                                           void* stream) {
  return dice_pred_bwd_launch<2>(logits, pitch, label, n, nvox, hardness, coef, topk_coef, gscale, dlogits, 0, 2, stream, "vsseg_dice_ce_topk_pred_bwd");
}
extern "C" int vsseg_dice_ce_topk_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* topk_coef, const float* gscale,
                                              vsseg_tensor dst, void* stream) {
  const int out = dice_pred_bwd_layout(dst, n, nvox, "vsseg_dice_ce_topk_pred_bwd_to");
  if (out < 0) return VSSEG_EINVAL;
  return dice_pred_bwd_launch<2>(logits, pitch, label, n, nvox, hardness, coef, topk_coef, gscale, dst.ptr, out, dst.pitch, stream, "vsseg_dice_ce_topk_pred_bwd_to");
}

// every combination of the region options and the cross-entropy modes (vsseg_loss_opts): the record picks the instantiation
static int loss_pred_bwd_dispatch(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const vsseg_loss_opts* o, const float* gscale, void* dst,
                                  int out, int dpitch, void* stream, const char* who) {
  const float fg = o->ce_mode == VSSEG_CE_FOCAL ? (float)o->ce_focal_gamma : 0.f;
#define VSSEG_LOSS_BWD(CE, SPLIT) return dice_pred_bwd_launch<CE, SPLIT>(logits, pitch, label, n, nvox, hardness, coef, ce_coef, gscale, dst, out, dpitch, stream, who, fg)
  if (o->region) {
    if (o->ce_mode == VSSEG_CE_NONE) VSSEG_LOSS_BWD(0, true);
    if (o->ce_mode == VSSEG_CE_PLAIN) VSSEG_LOSS_BWD(1, true);
    if (o->ce_mode == VSSEG_CE_TOPK) VSSEG_LOSS_BWD(2, true);
    VSSEG_LOSS_BWD(3, true);
  }
  if (o->ce_mode == VSSEG_CE_NONE) VSSEG_LOSS_BWD(0, false);
  if (o->ce_mode == VSSEG_CE_PLAIN) VSSEG_LOSS_BWD(1, false);
  if (o->ce_mode == VSSEG_CE_TOPK) VSSEG_LOSS_BWD(2, false);
  VSSEG_LOSS_BWD(3, false);
#undef VSSEG_LOSS_BWD
}
extern "C" int vsseg_loss_pred_bwd(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const vsseg_loss_opts* opts, const float* gscale,
                                   float* dlogits, void* stream) {
  if (loss_opts_check(opts, "vsseg_loss_pred_bwd") != VSSEG_OK) return VSSEG_EINVAL;
  return loss_pred_bwd_dispatch(logits, pitch, label, n, nvox, hardness, coef, ce_coef, opts, gscale, dlogits, 0, 2, stream, "vsseg_loss_pred_bwd");
}
extern "C" int vsseg_loss_pred_bwd_to(const float* logits, int32_t pitch, const float* label, int32_t n, int64_t nvox, int32_t hardness, const float* coef, const float* ce_coef, const vsseg_loss_opts* opts, const float* gscale,
                                      vsseg_tensor dst, void* stream) {
  if (loss_opts_check(opts, "vsseg_loss_pred_bwd_to") != VSSEG_OK) return VSSEG_EINVAL;
  const int out = dice_pred_bwd_layout(dst, n, nvox, "vsseg_loss_pred_bwd_to");
  if (out < 0) return VSSEG_EINVAL;
  return loss_pred_bwd_dispatch(logits, pitch, label, n, nvox, hardness, coef, ce_coef, opts, gscale, dst.ptr, out, dst.pitch, stream, "vsseg_loss_pred_bwd_to");
}

__global__ void dice_att_bwd_kernel(const float* __restrict__ label, int64_t nvox, const float* __restrict__ coef, const float* __restrict__ gscale, float* __restrict__ datt) {
  const int b = blockIdx.y;
  const float gs = gscale ? *gscale : 1.f;
  const float A = coef[b * 2] * gs, B = coef[b * 2 + 1] * gs;
  const float* lb = label + (int64_t)b * nvox;
  float* o = datt + (int64_t)b * nvox;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
  if ((nvox & 3) == 0 && (reinterpret_cast<uintptr_t>(label) & 15) == 0 && (reinterpret_cast<uintptr_t>(datt) & 15) == 0) {
    for (int64_t i = tid; i < (nvox >> 2); i += nthr) {
      const float4 g = reinterpret_cast<const float4*>(lb)[i];
      reinterpret_cast<float4*>(o)[i] = make_float4(A * g.x + B, A * g.y + B, A * g.z + B, A * g.w + B);
    }
  } else {
    for (int64_t v = tid; v < nvox; v += nthr) o[v] = A * lb[v] + B;
  }
}
extern "C" int vsseg_dice_att_bwd(const float* label, int32_t n, int64_t nvox, const float* coef, float inv_levels, const float* gscale, float* datt, void* stream) {
  (void)inv_levels;  // the 1/L factor is already folded into coef by vsseg_dice_finalize
  VSSEG_CHECK(label && coef && datt && n >= 1 && nvox >= 1, "vsseg_dice_att_bwd: bad arguments");
  dim3 g(grid_for((nvox + 3) / 4, 256, 2048), n);
  hipLaunchKernelGGL(dice_att_bwd_kernel, g, dim3(256), 0, as_stream(stream), label, nvox, coef, gscale, datt);
  VSSEG_LAUNCH_CHECK("vsseg_dice_att_bwd");
  return VSSEG_OK;
}

// d(loss)/d(att) of several levels in one launch (the coarse levels: a few thousand voxels each)
struct DiceBwdLevelsK {
  vsseg_dice_bwd_levels_desc d;
  int first[VSSEG_DICE_MAX_LEVELS + 1];
};
__global__ __launch_bounds__(256) void dice_att_bwd_levels_kernel(const DiceBwdLevelsK k) {
  const int b = blockIdx.y;
  int l = 0;
  while (l + 1 < k.d.nlevels && (int)blockIdx.x >= k.first[l + 1]) ++l;
  const int nb = k.first[l + 1] - k.first[l], lb = (int)blockIdx.x - k.first[l];
  const float gs = k.d.gscale ? *k.d.gscale : 1.f;
  const float A = k.d.coef[l][b * 2] * gs, B = k.d.coef[l][b * 2 + 1] * gs;
  const int64_t nvox = k.d.nvox[l];
  const float* lb_ = k.d.label[l] + (int64_t)b * nvox;
  float* o = k.d.datt[l] + (int64_t)b * nvox;
  for (int64_t v = (int64_t)lb * 256 + threadIdx.x; v < nvox; v += (int64_t)nb * 256) o[v] = A * lb_[v] + B;
}
extern "C" int vsseg_dice_att_bwd_levels(const vsseg_dice_bwd_levels_desc* d, void* stream) {
  VSSEG_CHECK(d && d->n >= 1 && d->nlevels >= 1 && d->nlevels <= VSSEG_DICE_MAX_LEVELS, "vsseg_dice_att_bwd_levels: bad arguments");
  DiceBwdLevelsK k;
  k.d = *d;
  int nb = 0;
  for (int l = 0; l < d->nlevels; ++l) {
    VSSEG_CHECK(d->label[l] && d->datt[l] && d->coef[l] && d->nvox[l] >= 1, "vsseg_dice_att_bwd_levels: level %d is incomplete", l);
    k.first[l] = nb;
    nb += (int)std::min<int64_t>(256, (d->nvox[l] + 2047) / 2048);
  }
  for (int l = d->nlevels; l <= VSSEG_DICE_MAX_LEVELS; ++l) k.first[l] = nb;
  hipLaunchKernelGGL(dice_att_bwd_levels_kernel, dim3(nb, d->n), dim3(256), 0, as_stream(stream), k);
  VSSEG_LAUNCH_CHECK("vsseg_dice_att_bwd_levels");
  return VSSEG_OK;
}

// hard Dice: argmax over the 2 channels vs label (ties -> class 0, like torch.argmax)
__global__ void hard_dice_kernel(const float* __restrict__ logits, int pitch, const float* __restrict__ label, int64_t nvox, double* __restrict__ counts) {
  float pg = 0, p = 0, g = 0;
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
    float2 l = *reinterpret_cast<const float2*>(logits + v * pitch);
    float pr = vsseg_pred_fg(l) ? 1.f : 0.f;
    float gg = vsseg_label_fg(label[v]) ? 1.f : 0.f;
    pg += pr * gg; p += pr; g += gg;
  }
  double vals[3] = {pg, p, g};
  block_reduce_add(vals, 3, counts, 0.0, nullptr);
}
extern "C" int vsseg_hard_dice_counts(const float* logits, int32_t pitch, const float* label, int64_t nvox, double* counts, void* stream) {
  VSSEG_CHECK(logits && label && counts && pitch >= 2 && pitch % 2 == 0, "vsseg_hard_dice_counts: bad arguments");
  hipLaunchKernelGGL(hard_dice_kernel, dim3(grid_for(nvox, 256, 1024)), dim3(256), 0, as_stream(stream), logits, pitch, label, nvox, counts);
  VSSEG_LAUNCH_CHECK("vsseg_hard_dice_counts");
  return VSSEG_OK;
}
__global__ void argmax2_kernel(const float* __restrict__ logits, int pitch, int64_t nvox, uint8_t* __restrict__ dst) {
  for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
    float2 l = *reinterpret_cast<const float2*>(logits + v * pitch);
    dst[v] = vsseg_pred_fg(l) ? 1 : 0;
  }
}
extern "C" int vsseg_argmax2(const float* logits, int32_t pitch, int64_t nvox, uint8_t* dst, void* stream) {
  VSSEG_CHECK(logits && dst && pitch >= 2 && pitch % 2 == 0, "vsseg_argmax2: bad arguments");
  hipLaunchKernelGGL(argmax2_kernel, dim3(grid_for(nvox, 256)), dim3(256), 0, as_stream(stream), logits, pitch, nvox, dst);
  VSSEG_LAUNCH_CHECK("vsseg_argmax2");
  return VSSEG_OK;
}
