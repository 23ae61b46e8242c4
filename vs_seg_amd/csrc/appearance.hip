// Appearance augmentation of a training batch after the crop launch (semantics: include/vsseg_hip.h): vsseg_patch_filter (in-plane Gaussian blur, simulated
// low-resolution acquisition) and vsseg_patch_tone (contrast about the mean with the range preserved, gamma curve).  Patches are [rx][ry][rz] fp32 with z contiguous: lanes
// run along z, the filters act along the two strided axes.
#include "common.h"
#include <math.h>

namespace {
// ---- vsseg_patch_filter ----
// Blur: one workgroup owns a tile of FT_X x FT_Y x FT_Z output voxels.  It stages the tile of v with its in-plane halo of R voxels in LDS (the halo comes from the
// reflection, so every global address lies inside the job's own patch), filters along x into a second LDS array and along y into the output.  An LDS row is FT_Z
// consecutive floats: the 16 lanes of a row group and the 4 row groups of a wave read consecutive banks, so every access is conflict-free.
// At R = 5 the two arrays are 18 x 26 x 16 and 8 x (26 x 16 + 16) floats = 43 KB: three workgroups per CU.
constexpr int FT_X = 8, FT_Y = 16, FT_Z = 16, FR_MAX = 5;
constexpr int FH_X = FT_X + 2 * FR_MAX, FH_Y = FT_Y + 2 * FR_MAX;
constexpr int F_GROUPS = 256 / FT_Z;  // row groups of a workgroup

// the edge-repeating reflection (..., 1, 0 | 0, 1, ..., n-1 | n-1, n-2, ...) of period 2n, for any i
__device__ __forceinline__ int reflect_index(int i, int n) {
  if ((unsigned)i < (unsigned)n) return i;  // inside: all but the border tiles
  const int p = 2 * n;
  int m = i % p;
  if (m < 0) m += p;
  return m < n ? m : p - 1 - m;
}
__device__ __forceinline__ bool filter_low(const vsseg_filter_job& j, int rx, int ry) { return j.coarse[0] != rx || j.coarse[1] != ry; }

// Staging and the two passes over the tile, for a compile-time radius: a thread filters a whole line of the tile from a sliding window in registers, so an LDS value is read
// once per pass instead of once per tap.  x pass: one thread per (y row of the tile and its halo, z), FT_X outputs; y pass: one thread per (x, half of the y rows, z),
// FT_Y / 2 outputs.  Consecutive threads touch consecutive LDS words; the x planes of B are FB_XS = 16 mod 32 words apart, so the two x planes of a 32-lane group fall on
// different banks.
constexpr int FB_XS = FH_Y * FT_Z + 16;
template <int R>
__device__ __forceinline__ void blur_tile(const vsseg_filter_job& job, float* A, float* B, const float* __restrict__ v, float* __restrict__ out, int x0, int y0, int z, bool zin, int rx, int ry, int rz) {
  constexpr int hx = FT_X + 2 * R, hy = FT_Y + 2 * R;
  float w[R + 1];
#pragma unroll
  for (int k = 0; k <= R; ++k) w[k] = job.taps[k];
  const int stz = threadIdx.x & (FT_Z - 1);
#pragma unroll 4
  for (int r = threadIdx.x / FT_Z; r < hx * hy; r += F_GROUPS) {  // the tile of v and its halo, one row of FT_Z lanes per (x, y)
    const int lx = r / hy, ly = r - lx * hy;
    const int x = reflect_index(x0 - R + lx, rx), y = reflect_index(y0 - R + ly, ry);
    A[(lx * FH_Y + ly) * FT_Z + stz] = zin ? v[((int64_t)x * ry + y) * rz + z] : 0.f;
  }
  __syncthreads();
  for (int item = threadIdx.x; item < hy * FT_Z; item += 256) {  // item = ly * FT_Z + tz
    float win[FT_X + 2 * R];
#pragma unroll
    for (int i = 0; i < FT_X + 2 * R; ++i) win[i] = A[i * FH_Y * FT_Z + item];
#pragma unroll
    for (int lx = 0; lx < FT_X; ++lx) {
      float acc = w[0] * win[lx + R];
#pragma unroll
      for (int k = 1; k <= R; ++k) {
        acc = __builtin_fmaf(w[k], win[lx + R - k], acc);
        acc = __builtin_fmaf(w[k], win[lx + R + k], acc);
      }
      B[lx * FB_XS + item] = acc;
    }
  }
  __syncthreads();
  const int tz = threadIdx.x & (FT_Z - 1), lx = (threadIdx.x / FT_Z) & (FT_X - 1), half = threadIdx.x / (FT_Z * FT_X);
  static_assert(FT_Z * FT_X * 2 == 256 && FT_Y == 16, "one thread per (z, x, half of the y rows)");
  const float* b = B + lx * FB_XS + half * (FT_Y / 2) * FT_Z + tz;
  float win[FT_Y / 2 + 2 * R];
#pragma unroll
  for (int i = 0; i < FT_Y / 2 + 2 * R; ++i) win[i] = b[i * FT_Z];
  const int x = x0 + lx;
#pragma unroll
  for (int j = 0; j < FT_Y / 2; ++j) {
    float acc = w[0] * win[j + R];
#pragma unroll
    for (int k = 1; k <= R; ++k) {
      acc = __builtin_fmaf(w[k], win[j + R - k], acc);
      acc = __builtin_fmaf(w[k], win[j + R + k], acc);
    }
    const int y = y0 + half * (FT_Y / 2) + j;
    if (zin && x < rx && y < ry) out[((int64_t)x * ry + y) * rz + z] = acc;
  }
}

// Jobs with a blur write u to dst, or to scratch when the low-resolution gather follows; jobs with neither family are copied; jobs with low resolution alone are left
// to patch_lowres_kernel, which reads src itself.
__global__ __launch_bounds__(256) void patch_blur_kernel(const vsseg_filter_job* __restrict__ jobs, const float* __restrict__ src, float* __restrict__ dst, float* __restrict__ scratch,
                                                         int rx, int ry, int rz, int ntz) {
  __shared__ float A[FH_X * FH_Y * FT_Z];
  __shared__ float B[FT_X * FB_XS];
  const vsseg_filter_job job = jobs[blockIdx.z];
  const int R = job.radius;
  const bool low = filter_low(job, rx, ry);
  if (R == 0 && low) return;
  const int64_t patch = (int64_t)rx * ry * rz;
  const float* v = src + blockIdx.z * patch;
  float* out = (low ? scratch : dst) + blockIdx.z * patch;
  const int tyb = blockIdx.x / ntz, tzb = blockIdx.x - tyb * ntz;
  const int tz = threadIdx.x & (FT_Z - 1), g = threadIdx.x / FT_Z;
  const int x0 = blockIdx.y * FT_X, y0 = tyb * FT_Y, z = tzb * FT_Z + tz;
  const bool zin = z < rz;
  if (R == 0) {  // neither family: a plain copy
    for (int r = g; r < FT_X * FT_Y; r += F_GROUPS) {
      const int x = x0 + r / FT_Y, y = y0 + r % FT_Y;
      if (zin && x < rx && y < ry) out[((int64_t)x * ry + y) * rz + z] = v[((int64_t)x * ry + y) * rz + z];
    }
    return;
  }
  switch (R) {  // workgroup-uniform
    case 1: blur_tile<1>(job, A, B, v, out, x0, y0, z, zin, rx, ry, rz); break;
    case 2: blur_tile<2>(job, A, B, v, out, x0, y0, z, zin, rx, ry, rz); break;
    case 3: blur_tile<3>(job, A, B, v, out, x0, y0, z, zin, rx, ry, rz); break;
    case 4: blur_tile<4>(job, A, B, v, out, x0, y0, z, zin, rx, ry, rz); break;
    default: blur_tile<5>(job, A, B, v, out, x0, y0, z, zin, rx, ry, rz); break;
  }
}

// coarse coordinate of output index p along one axis: the two source indices q(i0), q(i1) and the fraction
__device__ __forceinline__ void lowres_axis(int p, int n, int roi, int& q0, int& q1, float& phi) {
  int i0 = p;
  phi = 0.f;
  if (n != roi) {  // (n == roi: t = p whatever the size, the axis is untouched)
    float t = (p + 0.5f) * (float)n / (float)roi - 0.5f;
    t = fminf(fmaxf(t, 0.f), (float)(n - 1));
    const float fl = floorf(t);
    i0 = (int)fl;
    phi = t - fl;
  }
  const int i1 = i0 + 1 < n ? i0 + 1 : n - 1;
  q0 = (int)(((int64_t)(2 * i0 + 1) * roi) / (2 * (int64_t)n));
  q1 = (int)(((int64_t)(2 * i1 + 1) * roi) / (2 * (int64_t)n));
}

// The low-resolution gather: one thread per four consecutive z of one (x, y); the four in-plane sources are rows of the job's own u (scratch after a blur, src otherwise).
__global__ __launch_bounds__(256) void patch_lowres_kernel(const vsseg_filter_job* __restrict__ jobs, const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ scratch,
                                                           int rx, int ry, int rz, int nzq) {
  const vsseg_filter_job job = jobs[blockIdx.y];
  if (!filter_low(job, rx, ry)) return;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= ry * nzq) return;
  const int y = t / nzq, z0 = (t - y * nzq) * 4, x = blockIdx.z;
  const int64_t patch = (int64_t)rx * ry * rz;
  const float* u = (job.radius > 0 ? scratch : src) + blockIdx.y * patch;
  int qx0, qx1, qy0, qy1;
  float px, py;
  lowres_axis(x, job.coarse[0], rx, qx0, qx1, px);
  lowres_axis(y, job.coarse[1], ry, qy0, qy1, py);
  const float* u00 = u + ((int64_t)qx0 * ry + qy0) * rz + z0;
  const float* u01 = u + ((int64_t)qx0 * ry + qy1) * rz + z0;
  const float* u10 = u + ((int64_t)qx1 * ry + qy0) * rz + z0;
  const float* u11 = u + ((int64_t)qx1 * ry + qy1) * rz + z0;
  float* out = dst + blockIdx.y * patch + ((int64_t)x * ry + y) * rz + z0;
  const bool vec = (rz & 3) == 0;
  float a[4][4];
  if (vec) {
    const float4 q0 = ld4(u00), q1 = ld4(u01), q2 = ld4(u10), q3 = ld4(u11);
    a[0][0] = q0.x, a[0][1] = q0.y, a[0][2] = q0.z, a[0][3] = q0.w;
    a[1][0] = q1.x, a[1][1] = q1.y, a[1][2] = q1.z, a[1][3] = q1.w;
    a[2][0] = q2.x, a[2][1] = q2.y, a[2][2] = q2.z, a[2][3] = q2.w;
    a[3][0] = q3.x, a[3][1] = q3.y, a[3][2] = q3.z, a[3][3] = q3.w;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const bool in = z0 + e < rz;
      a[0][e] = in ? u00[e] : 0.f, a[1][e] = in ? u01[e] : 0.f, a[2][e] = in ? u10[e] : 0.f, a[3][e] = in ? u11[e] : 0.f;
    }
  }
  float o[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float lo = __builtin_fmaf(py, a[1][e] - a[0][e], a[0][e]);  // along y at q_x(i0) and at q_x(i1) ...
    const float hi = __builtin_fmaf(py, a[3][e] - a[2][e], a[2][e]);
    o[e] = __builtin_fmaf(px, hi - lo, lo);  // ... then along x
  }
  if (vec) {
    st4(out, make_float4(o[0], o[1], o[2], o[3]));
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (z0 + e < rz) out[e] = o[e];
  }
}

// ---- vsseg_patch_tone ----
// Pass 1: element i of a job belongs to chunk i / 1024, chunk c to shard c % VSSEG_TONE_SHARDS, and inside a chunk thread t owns the elements 4t .. 4t+3.  A workgroup is
// one shard of one job: every thread adds its elements in index order in fp64, the 64 lanes of a wave are combined by a butterfly and the four waves in a fixed order.
// Nothing depends on the order in which workgroups run, so (S, mn, mx) of a shard, and everything derived from them, has the same bits in every launch.
constexpr int TONE_CHUNK = 1024;

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ bool tone_neutral(const vsseg_tone_job& j) { return j.contrast == 1.f && j.gamma == 1.f; }
// the up to four elements i .. i+3 of a job that exist: v[0 .. count)
__device__ __forceinline__ int tone_load(const float* xj, int64_t i, int64_t n, bool vec, float v[4]) {
  if (vec) {
    if (i >= n) return 0;
    const float4 q = ld4(xj + i);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
    return 4;
  }
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (i + e < n) v[cnt++] = xj[i + e];
  return cnt;
}

__global__ __launch_bounds__(256) void tone_reduce_kernel(const vsseg_tone_job* __restrict__ jobs, const float* __restrict__ x, int64_t n, double* __restrict__ work) {
  __shared__ double ls[4];
  __shared__ float lmn[4], lmx[4];
  const int j = blockIdx.y, s = blockIdx.x;
  if (tone_neutral(jobs[j])) return;
  const float* xj = x + (int64_t)j * n;
  const bool vec = (n & 3) == 0 && ((uintptr_t)x & 15) == 0;
  const int64_t nchunks = (n + TONE_CHUNK - 1) / TONE_CHUNK;
  double sum = 0.0;
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll 4
  for (int64_t c = s; c < nchunks; c += VSSEG_TONE_SHARDS) {
    float v[4];
    const int cnt = tone_load(xj, c * TONE_CHUNK + 4 * (int64_t)threadIdx.x, n, vec, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (e < cnt) {
        sum += (double)v[e];
        mn = fminf(mn, v[e]);
        mx = fmaxf(mx, v[e]);
      }
  }
  sum = wave_sum_d(sum);
  mn = wave_min(mn);
  mx = wave_max(mx);
  if ((threadIdx.x & 63) == 0) ls[threadIdx.x >> 6] = sum, lmn[threadIdx.x >> 6] = mn, lmx[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {  // a shard without elements leaves (0, +inf, -inf): pass 2 reads every shard
    double* w = work + ((int64_t)j * VSSEG_TONE_SHARDS + s) * 3;
    w[0] = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    w[1] = (double)fminf(fminf(lmn[0], lmn[1]), fminf(lmn[2], lmn[3]));
    w[2] = (double)fmaxf(fmaxf(lmx[0], lmx[1]), fmaxf(lmx[2], lmx[3]));
  }
}

// Pass 2: every workgroup combines the shards of its job in the same fixed order (so all of them hold the same mn, mx, mu), then maps its chunks in place.
__global__ __launch_bounds__(256) void tone_apply_kernel(const vsseg_tone_job* __restrict__ jobs, float* __restrict__ x, int64_t n, const double* __restrict__ work, float* __restrict__ stats) {
  static_assert(VSSEG_TONE_SHARDS == 128, "wave 0 combines two shards per lane");
  __shared__ float sh[3];
  const int j = blockIdx.y;
  const vsseg_tone_job job = jobs[j];
  if (tone_neutral(job)) {
    if (blockIdx.x == 0 && threadIdx.x < 4) stats[4 * j + threadIdx.x] = 0.f;
    return;
  }
  if (threadIdx.x < 64) {
    const double* w = work + (int64_t)j * VSSEG_TONE_SHARDS * 3;
    const int l = threadIdx.x;
    const double s = wave_sum_d(w[3 * l] + w[3 * (l + 64)]);
    const float mn = wave_min(fminf((float)w[3 * l + 1], (float)w[3 * (l + 64) + 1]));
    const float mx = wave_max(fmaxf((float)w[3 * l + 2], (float)w[3 * (l + 64) + 2]));
    if (l == 0) sh[0] = mn, sh[1] = mx, sh[2] = (float)(s / (double)n);
  }
  __syncthreads();
  const float mn = sh[0], mx = sh[1], mu = sh[2], c = job.contrast, gam = job.gamma;
  if (blockIdx.x == 0 && threadIdx.x == 0) stats[4 * j] = mn, stats[4 * j + 1] = mx, stats[4 * j + 2] = mu, stats[4 * j + 3] = 0.f;
  auto T = [&](float v) { return c == 1.f ? v : fminf(fmaxf(__builtin_fmaf(v - mu, c, mu), mn), mx); };
  const float a = T(mn), b = T(mx), r = b - a, den = r + 1e-7f;
  float* xj = x + (int64_t)j * n;
  const bool vec = (n & 3) == 0 && ((uintptr_t)x & 15) == 0;
  const int64_t nchunks = (n + TONE_CHUNK - 1) / TONE_CHUNK;
  for (int64_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const int64_t i = ch * TONE_CHUNK + 4 * (int64_t)threadIdx.x;
    float v[4];
    const int cnt = tone_load(xj, i, n, vec, v);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float y = T(v[e]);
      if (gam != 1.f) y = __builtin_fmaf(powf((y - a) / den, gam), r, a);
      v[e] = y;
    }
    if (vec) {
      if (cnt) st4(xj + i, make_float4(v[0], v[1], v[2], v[3]));
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (e < cnt) xj[i + e] = v[e];
    }
  }
}

bool finite_f(float f) { return f - f == 0.f; }
}  // namespace

extern "C" int vsseg_patch_filter(const vsseg_filter_job* jobs_host, const void* jobs_dev, int32_t njobs, const float* src, float* dst, float* scratch, const int32_t roi[3], void* stream) {
  VSSEG_CHECK(jobs_host && jobs_dev && src && dst && roi, "vsseg_patch_filter: null pointer");
  VSSEG_CHECK(src != dst, "vsseg_patch_filter: src == dst (the filter does not work in place)");
  VSSEG_CHECK(njobs >= 1 && njobs <= 65535, "vsseg_patch_filter: njobs = %d outside [1, 65535]", njobs);
  VSSEG_CHECK(roi[0] >= 1 && roi[1] >= 1 && roi[2] >= 1 && roi[0] <= 65535 && roi[1] <= 65535 && roi[2] <= 65535, "vsseg_patch_filter: bad roi (%d, %d, %d): each in [1, 65535]", roi[0], roi[1], roi[2]);
  VSSEG_CHECK((((uintptr_t)src | (uintptr_t)dst | (uintptr_t)scratch) & 15) == 0, "vsseg_patch_filter: misaligned src, dst or scratch (16 bytes)");
  bool any_low = false, any_first = false;
  for (int32_t i = 0; i < njobs; ++i) {
    const vsseg_filter_job& j = jobs_host[i];
    VSSEG_CHECK(j.radius >= 0 && j.radius <= FR_MAX, "vsseg_patch_filter: job %d: radius = %d outside [0, %d]", i, j.radius, FR_MAX);
    if (j.radius > 0) {
      bool fin = true;
      double sum = 0.0;
      for (int k = 0; k <= j.radius; ++k) fin = fin && finite_f(j.taps[k]), sum += (k ? 2.0 : 1.0) * (double)j.taps[k];
      VSSEG_CHECK(fin, "vsseg_patch_filter: job %d: non-finite taps", i);
      VSSEG_CHECK(fabs(sum - 1.0) <= 1e-5, "vsseg_patch_filter: job %d: taps not normalised: w_0 + 2 sum w_k = %.9g", i, sum);
    }
    VSSEG_CHECK(j.coarse[0] >= 1 && j.coarse[0] <= roi[0] && j.coarse[1] >= 1 && j.coarse[1] <= roi[1], "vsseg_patch_filter: job %d: coarse = (%d, %d) outside [1, roi] = (%d, %d)", i, j.coarse[0], j.coarse[1], roi[0], roi[1]);
    const bool low = j.coarse[0] != roi[0] || j.coarse[1] != roi[1];
    any_low = any_low || low;
    any_first = any_first || !(low && j.radius == 0);
    VSSEG_CHECK(scratch || !(low && j.radius > 0), "vsseg_patch_filter: job %d has blur and low resolution: scratch must not be null", i);
  }
  hipStream_t s = as_stream(stream);
  if (any_first) {
    const int ntz = (roi[2] + FT_Z - 1) / FT_Z;
    hipLaunchKernelGGL(patch_blur_kernel, dim3(((roi[1] + FT_Y - 1) / FT_Y) * ntz, (roi[0] + FT_X - 1) / FT_X, njobs), dim3(256), 0, s, (const vsseg_filter_job*)jobs_dev, src, dst, scratch, roi[0], roi[1], roi[2], ntz);
  }
  if (any_low) {
    const int nzq = (roi[2] + 3) / 4;
    hipLaunchKernelGGL(patch_lowres_kernel, dim3((roi[1] * nzq + 255) / 256, njobs, roi[0]), dim3(256), 0, s, (const vsseg_filter_job*)jobs_dev, src, dst, (const float*)scratch, roi[0], roi[1], roi[2], nzq);
  }
  VSSEG_LAUNCH_CHECK("vsseg_patch_filter");
  return VSSEG_OK;
}

extern "C" int vsseg_patch_tone(const vsseg_tone_job* jobs_host, const void* jobs_dev, int32_t njobs, float* x, int64_t n, float* stats, double* work, void* stream) {
  VSSEG_CHECK(jobs_host && jobs_dev && x && stats && work, "vsseg_patch_tone: null pointer");
  VSSEG_CHECK(njobs >= 1 && njobs <= 65535, "vsseg_patch_tone: njobs = %d outside [1, 65535]", njobs);
  VSSEG_CHECK(n >= 1, "vsseg_patch_tone: n = %lld: at least 1", (long long)n);
  bool any = false;
  for (int32_t i = 0; i < njobs; ++i) {
    const vsseg_tone_job& j = jobs_host[i];
    VSSEG_CHECK(finite_f(j.contrast) && j.contrast > 0.f && j.contrast < 2.f, "vsseg_patch_tone: job %d: contrast = %g not finite or outside (0, 2)", i, (double)j.contrast);
    VSSEG_CHECK(finite_f(j.gamma) && j.gamma > 0.f && j.gamma < 2.f, "vsseg_patch_tone: job %d: gamma = %g not finite or outside (0, 2)", i, (double)j.gamma);
    any = any || j.contrast != 1.f || j.gamma != 1.f;
  }
  hipStream_t s = as_stream(stream);
  const int64_t nchunks = (n + TONE_CHUNK - 1) / TONE_CHUNK;
  if (any) hipLaunchKernelGGL(tone_reduce_kernel, dim3(VSSEG_TONE_SHARDS, njobs), dim3(256), 0, s, (const vsseg_tone_job*)jobs_dev, (const float*)x, n, work);
  hipLaunchKernelGGL(tone_apply_kernel, dim3(grid_for(nchunks, 1, 2048), njobs), dim3(256), 0, s, (const vsseg_tone_job*)jobs_dev, x, n, (const double*)work, stats);
  VSSEG_LAUNCH_CHECK("vsseg_patch_tone");
  return VSSEG_OK;
}
