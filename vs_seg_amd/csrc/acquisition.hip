// Acquisition-artefact augmentation of a training batch after the crop launch (semantics: include/vsseg_hip.h): vsseg_patch_acquisition = thick slices along z, then
// phase-encode ghosting along x or y, then a k-space spike, each in its exact image-domain form.  Patches are [rx][ry][rz] fp32 with z contiguous.
//   acq_thick_kernel   T: one thread per four consecutive z of one (x, y) column; it forms the (at most five) slab means its outputs interpolate between.
//   acq_line_kernel    G and S (and the plain copy): one workgroup per (line, 128 bytes of the contiguous index) tile, the spike folded into the store.
// A job with thick slices and a later stage passes T(v) through its patch of `scratch`; every other job is touched by one of the two kernels only.
#include "common.h"
#include <math.h>

namespace {
__device__ __forceinline__ bool acq_ghost(const vsseg_acquisition_job& j) { return j.ghosts != 0; }
__device__ __forceinline__ bool acq_spike(const vsseg_acquisition_job& j) { return j.spike_amp != 0.f; }

// ---- thick slices ----
constexpr int THICK_MAX = 8;
// four consecutive z see at most three slabs (f >= 2), and one more on either side for the interpolation
constexpr int THICK_SLABS = 5;

__device__ __forceinline__ float pick5(const float (&m)[THICK_SLABS], int s) { return s == 0 ? m[0] : s == 1 ? m[1] : s == 2 ? m[2] : s == 3 ? m[3] : m[4]; }

__global__ __launch_bounds__(256) void acq_thick_kernel(const vsseg_acquisition_job* __restrict__ jobs, const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ scratch,
                                                        int rx, int ry, int rz, int nzq) {
  const vsseg_acquisition_job job = jobs[blockIdx.z];
  const int f = job.thick, o = job.thick_offset;
  if (f == 1) return;  // left to acq_line_kernel, which reads src itself
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)ry * (unsigned)nzq) return;
  const int y = (int)(t / (unsigned)nzq), z0 = (int)(t - (unsigned)y * (unsigned)nzq) * 4, x = blockIdx.y;
  const int64_t patch = (int64_t)rx * ry * rz, at = ((int64_t)x * ry + y) * rz;
  const float* col = src + blockIdx.z * patch + at;
  float* out = ((acq_ghost(job) || acq_spike(job)) ? scratch : dst) + blockIdx.z * patch + at + z0;
  const int K = (rz - 1 + o) / f + 1;  // slabs of the column; slab k holds the z with (z + o) / f == k
  auto first = [&](int k) { return max(k * f - o, 0); };
  auto last = [&](int k) { return min((k + 1) * f - o, rz) - 1; };
  auto centre = [&](int k) { return 0.5f * (float)(first(k) + last(k)); };  // a multiple of 0.5: exact
  const int k0 = (z0 + o) / f, r0 = z0 + o - k0 * f;
  int a[4], b[4];
  float phi[4];
  int lo = 0, hi = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int z = z0 + e, r = r0 + e, k = k0 + (r >= f) + (r >= 2 * f);  // (e <= 3 and f >= 2: at most two slabs further)
    if (z >= rz) {  // past the column (rz % 4 != 0): computed from slab `lo`, never stored
      a[e] = b[e] = 0, phi[e] = 0.f;
      continue;
    }
    int ka = (float)z >= centre(k) ? k : k - 1, kb = ka + 1;
    if (ka < 0) ka = kb = 0;
    if (kb > K - 1) ka = kb = K - 1;
    phi[e] = ka == kb ? 0.f : ((float)z - centre(ka)) / (centre(kb) - centre(ka));
    if (e == 0) lo = ka;
    a[e] = ka - lo, b[e] = kb - lo, hi = kb;
  }
  float m[THICK_SLABS];
#pragma unroll
  for (int s = 0; s < THICK_SLABS; ++s) {
    m[s] = 0.f;
    const int k = lo + s;
    if (k <= hi) {
      const int z1 = first(k), cnt = last(k) - z1 + 1;
      float acc = 0.f;
#pragma unroll
      for (int i = 0; i < THICK_MAX; ++i)
        if (i < cnt) acc += col[z1 + i];  // ascending z
      m[s] = acc / (float)cnt;
    }
  }
  float r[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float ma = pick5(m, a[e]), mb = pick5(m, b[e]);
    r[e] = __builtin_fmaf(phi[e], mb - ma, ma);
  }
  if ((rz & 3) == 0) {
    st4(out, make_float4(r[0], r[1], r[2], r[3]));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (z0 + e < rz) out[e] = r[e];
  }
}

// ---- ghosting and spike ----
// A line runs along x (elements ry * rz floats apart) or along y (rz floats apart); the index that is contiguous in memory across neighbouring lines is q = y * rz + z
// for lines along x and q = z for lines along y.  A workgroup owns GQ consecutive q of every element of a line (128 bytes per element: whole cache lines) and holds
// them in LDS, so the n reads per output of the ghost sum and the second read of the line cost no memory traffic.  Threads are (ti, tq): tq along q, ti along the line.
// A line longer than the LDS tile (N > tile_rows) reads the n terms from global memory instead (the L2 serves them): same arithmetic, same bits.
// Jobs without ghosting take the geometry of lines along x and skip the first pass: one read, one write.
constexpr int GQ = 32;
constexpr int ACQ_TILE_ROWS = 440;          // 440 * 128 + 8192 + 128 bytes = 64640 <= 64 KiB of LDS
constexpr int ACQ_RED_DOUBLES = 256 / (GQ / 4) * GQ;  // [TI][GQ] partial sums of the vector form (the scalar form needs a quarter of it)

template <int V> struct AcqVec;
template <> struct AcqVec<4> {
  static __device__ __forceinline__ void ld(const float* p, float (&v)[4]) {
    const float4 q = ld4(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  }
  static __device__ __forceinline__ void st(float* p, const float (&v)[4]) { st4(p, make_float4(v[0], v[1], v[2], v[3])); }
};
template <> struct AcqVec<1> {
  static __device__ __forceinline__ void ld(const float* p, float (&v)[1]) { v[0] = *p; }
  static __device__ __forceinline__ void st(float* p, const float (&v)[1]) { *p = v[0]; }
};

// V = 4: rz % 4 == 0, a thread owns a float4 of q (one (x, y) per element of the line: one cosf per four outputs); V = 1: any rz, one float per thread.
template <int V>
__global__ __launch_bounds__(256) void acq_line_kernel(const vsseg_acquisition_job* __restrict__ jobs, const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ scratch,
                                                       int rx, int ry, int rz, int tile_rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char acq_lds[];
  constexpr int TQ = GQ / V, TI = 256 / TQ;
  float* tile = reinterpret_cast<float*>(acq_lds);                                              // [tile_rows][GQ]
  double* red = reinterpret_cast<double*>(acq_lds + (size_t)tile_rows * GQ * sizeof(float));    // [TI][GQ]
  float* mus = reinterpret_cast<float*>(red + ACQ_RED_DOUBLES);                                 // [GQ]
  const vsseg_acquisition_job job = jobs[blockIdx.y];
  const bool ghost = acq_ghost(job), spike = acq_spike(job);
  if (job.thick != 1 && !ghost && !spike) return;  // thick slices alone: acq_thick_kernel wrote dst
  const bool ya = ghost && job.ghost_axis == 1;
  const int N = ya ? ry : rx;
  const unsigned plane = (unsigned)ry * (unsigned)rz;  // < 2^32
  const unsigned inner = ya ? (unsigned)rz : plane, tpo = (inner + GQ - 1) / GQ;
  const int64_t istride = ya ? rz : plane;
  if ((uint64_t)blockIdx.x >= (uint64_t)tpo * (ya ? rx : 1)) return;
  const unsigned outer = ya ? blockIdx.x / tpo : 0;  // the x of a line along y
  const int tq = threadIdx.x % TQ, ti = threadIdx.x / TQ;
  const unsigned q = (blockIdx.x - outer * tpo) * GQ + tq * V;
  const bool qin = q < inner;  // (V == 4: inner % 4 == 0, the whole float4 is in or out)
  const int64_t patch = (int64_t)rx * ry * rz, at = blockIdx.y * patch + (int64_t)outer * plane + q;
  const float* u = (job.thick != 1 ? scratch : src) + at;
  float* out = dst + at;
  const bool in_lds = ghost && N <= tile_rows;
  float mu[V];
#pragma unroll
  for (int e = 0; e < V; ++e) mu[e] = 0.f;
  if (ghost) {  // pass 1: the line into LDS, its sum in fp64 (every thread its elements in ascending order, the TI partial sums in a fixed order)
    double acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.0;
#pragma unroll 4
    for (int i = ti; i < N; i += TI) {
      float v[V];
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = 0.f;
      if (qin) AcqVec<V>::ld(u + i * istride, v);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] += (double)v[e];
      if (in_lds) AcqVec<V>::st(tile + i * GQ + tq * V, v);
    }
#pragma unroll
    for (int e = 0; e < V; ++e) red[ti * GQ + tq * V + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < GQ) {
      double s = 0.0;
      for (int t = 0; t < TI; ++t) s += red[t * GQ + threadIdx.x];
      mus[threadIdx.x] = (float)(s / (double)N);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < V; ++e) mu[e] = mus[tq * V + e];
  }
  if (!qin) return;
  const int n = job.ghosts, step = ghost ? N / n : 0;
  const float alpha = job.ghost_alpha, c = ghost ? alpha / (float)n : 0.f, amp = job.spike_amp, phase = job.spike_phase;
  // spike: t = (k_L i mod N) r_F + (k_F F mod r_F) N, reduced once by rx ry, with L the axis of the line and F the other in-plane axis
  const unsigned rF = ya ? rx : ry, kL = job.spike_k[ya ? 1 : 0], kF = job.spike_k[ya ? 0 : 1];
  const uint64_t period = (uint64_t)rx * ry;
  const float fperiod = (float)(unsigned)period;
  uint64_t fixed[V];
#pragma unroll
  for (int e = 0; e < V; ++e) fixed[e] = 0;
  unsigned along = 0, along_step = 0;
  if (spike) {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const unsigned F = ya ? outer : (q + e) / (unsigned)rz;
      fixed[e] = (uint64_t)((kF * F) % rF) * (unsigned)N;
    }
    along = (kL * (unsigned)ti) % (unsigned)N, along_step = (kL * (unsigned)TI) % (unsigned)N;
  }
#pragma unroll 4
  for (int i = ti; i < N; i += TI) {
    float w[V];
    if (in_lds) AcqVec<V>::ld(tile + i * GQ + tq * V, w);
    else AcqVec<V>::ld(u + i * istride, w);
    if (ghost) {
      float S[V];
#pragma unroll
      for (int e = 0; e < V; ++e) S[e] = 0.f;
      int idx = i;
      for (int j = 0; j < n; ++j) {
        float v[V];
        if (in_lds) AcqVec<V>::ld(tile + idx * GQ + tq * V, v);
        else AcqVec<V>::ld(u + idx * istride, v);
#pragma unroll
        for (int e = 0; e < V; ++e) S[e] += v[e];
        idx += step;
        if (idx >= N) idx -= N;
      }
#pragma unroll
      for (int e = 0; e < V; ++e) w[e] = __builtin_fmaf(alpha, mu[e], __builtin_fmaf(-c, S[e], w[e]));
    }
    if (spike) {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if (V == 4 && e > 0) continue;  // the four z of a float4 share (x, y)
        uint64_t t = (uint64_t)along * rF + fixed[e];
        if (t >= period) t -= period;
        const float cs = cosf(__builtin_fmaf(6.2831853f, (float)(unsigned)t / fperiod, phase));
        if (V == 4) {
#pragma unroll
          for (int k = 0; k < V; ++k) w[k] = __builtin_fmaf(amp, cs, w[k]);
        } else {
          w[e] = __builtin_fmaf(amp, cs, w[e]);
        }
      }
      along += along_step;
      if (along >= (unsigned)N) along -= (unsigned)N;
    }
    AcqVec<V>::st(out + i * istride, w);
  }
}

bool acq_finite(float f) { return f - f == 0.f; }
}  // namespace

extern "C" int vsseg_patch_acquisition(const vsseg_acquisition_job* jobs_host, const void* jobs_dev, int32_t njobs, const float* src, float* dst, float* scratch, const int32_t roi[3], void* stream) {
  VSSEG_CHECK(jobs_host && jobs_dev && src && dst && roi, "vsseg_patch_acquisition: null pointer");
  VSSEG_CHECK(src != dst, "vsseg_patch_acquisition: src == dst (the stages do not work in place)");
  VSSEG_CHECK(njobs >= 1 && njobs <= 65535, "vsseg_patch_acquisition: njobs = %d outside [1, 65535]", njobs);
  VSSEG_CHECK(roi[0] >= 1 && roi[1] >= 1 && roi[2] >= 1 && roi[0] <= 65535 && roi[1] <= 65535 && roi[2] <= 65535, "vsseg_patch_acquisition: bad roi (%d, %d, %d): each in [1, 65535]", roi[0], roi[1], roi[2]);
  VSSEG_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)scratch) & 15) == 0, "vsseg_patch_acquisition: misaligned src, dst or scratch (16 bytes)");
  bool any_thick = false, any_line = false, any_y = false;
  int tile_rows = 0;
  for (int32_t i = 0; i < njobs; ++i) {
    const vsseg_acquisition_job& j = jobs_host[i];
    VSSEG_CHECK(j.thick >= 1 && j.thick <= THICK_MAX, "vsseg_patch_acquisition: job %d: thick = %d outside [1, %d]", i, j.thick, THICK_MAX);
    VSSEG_CHECK(j.thick_offset >= 0 && j.thick_offset < j.thick, "vsseg_patch_acquisition: job %d: thick_offset = %d outside [0, thick = %d)", i, j.thick_offset, j.thick);
    VSSEG_CHECK(j.ghost_axis == 0 || j.ghost_axis == 1, "vsseg_patch_acquisition: job %d: ghost_axis = %d: 0 (x) or 1 (y)", i, j.ghost_axis);
    if (j.ghosts != 0) {
      const int N = roi[j.ghost_axis];
      VSSEG_CHECK(j.ghosts >= 2 && N % j.ghosts == 0, "vsseg_patch_acquisition: job %d: ghosts = %d: 0, or at least 2 and a divisor of roi[%d] = %d", i, j.ghosts, j.ghost_axis, N);
      VSSEG_CHECK(acq_finite(j.ghost_alpha) && j.ghost_alpha > 0.f && j.ghost_alpha <= 1.f, "vsseg_patch_acquisition: job %d: ghost_alpha = %g not finite or outside (0, 1]", i, (double)j.ghost_alpha);
      if (N <= ACQ_TILE_ROWS && N > tile_rows) tile_rows = N;
      any_y = any_y || j.ghost_axis == 1;
    }
    VSSEG_CHECK(acq_finite(j.spike_amp), "vsseg_patch_acquisition: job %d: non-finite spike_amp", i);
    VSSEG_CHECK(acq_finite(j.spike_phase), "vsseg_patch_acquisition: job %d: non-finite spike_phase", i);
    if (j.spike_amp != 0.f) {
      VSSEG_CHECK(j.spike_k[0] >= 0 && j.spike_k[0] < roi[0] && j.spike_k[1] >= 0 && j.spike_k[1] < roi[1], "vsseg_patch_acquisition: job %d: spike_k = (%d, %d) outside [0, roi) = (%d, %d)", i, j.spike_k[0], j.spike_k[1], roi[0], roi[1]);
      VSSEG_CHECK(j.spike_k[0] != 0 || j.spike_k[1] != 0, "vsseg_patch_acquisition: job %d: spike_k = (0, 0) with spike_amp != 0 (a spike on the DC line is a bias)", i);
    }
    const bool later = j.ghosts != 0 || j.spike_amp != 0.f;
    any_thick = any_thick || j.thick != 1;
    any_line = any_line || later || j.thick == 1;
    VSSEG_CHECK(scratch || !(j.thick != 1 && later), "vsseg_patch_acquisition: job %d has thick slices and a later stage: scratch must not be null", i);
  }
  hipStream_t s = as_stream(stream);
  const int rx = roi[0], ry = roi[1], rz = roi[2];
  if (any_thick) {
    const int nzq = (rz + 3) / 4;
    hipLaunchKernelGGL(acq_thick_kernel, dim3((unsigned)(((int64_t)ry * nzq + 255) / 256), rx, njobs), dim3(256), 0, s, (const vsseg_acquisition_job*)jobs_dev, src, dst, scratch, rx, ry, rz, nzq);
  }
  if (any_line) {
    const int64_t tiles_x = ((int64_t)ry * rz + GQ - 1) / GQ, tiles_y = any_y ? (int64_t)rx * ((rz + GQ - 1) / GQ) : 0;
    const dim3 grid((unsigned)(tiles_x > tiles_y ? tiles_x : tiles_y), njobs);
    const size_t lds = (size_t)tile_rows * GQ * sizeof(float) + ACQ_RED_DOUBLES * sizeof(double) + GQ * sizeof(float);
    if ((rz & 3) == 0) hipLaunchKernelGGL(acq_line_kernel<4>, grid, dim3(256), lds, s, (const vsseg_acquisition_job*)jobs_dev, src, dst, (const float*)scratch, rx, ry, rz, tile_rows);
    else hipLaunchKernelGGL(acq_line_kernel<1>, grid, dim3(256), lds, s, (const vsseg_acquisition_job*)jobs_dev, src, dst, (const float*)scratch, rx, ry, rz, tile_rows);
  }
  VSSEG_LAUNCH_CHECK("vsseg_patch_acquisition");
  return VSSEG_OK;
}
