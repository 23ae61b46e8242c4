// Data-side kernels: the random tail of the reference's MONAI transform chain and the intensity
// normalisation, on volumes cached in HBM, so that no CPU DataLoader worker touches the 25 MB/sample tensors
// (ref:params/VSparams.py:205-245: NormalizeIntensityd, SpatialPadd, RandFlipd(spatial_axis=0), RandSpatialCropd).
#include "common.h"
#include <type_traits>

// dst[b][x][y][z] = vol_b[m(sx+x)][m(sy+y)][m(sz+z)], m(g) = dim-1-g on the axes whose bit is set in the job's mirror mask (bit 0 = x, 1 = y, 2 = z) and g on the others,
// 0 outside the volume (= SpatialPadd's constant padding).  Training mirrors x only (RandFlipd); the mirrored passes of sliding-window inference use all three bits.
// One launch crops image and label of a whole batch: `srcs` holds 2*n device pointers (image_0, label_0, image_1, ...).
__global__ void crop_flip_kernel(const vsseg_crop_job* __restrict__ jobs, float* __restrict__ dst, int rx, int ry, int rz) {
  const vsseg_crop_job j = jobs[blockIdx.y];
  const int64_t per = (int64_t)rx * ry * rz;
  float* out = dst + (int64_t)blockIdx.y * per;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = i;
    const int z = (int)(r % rz); r /= rz;
    const int y = (int)(r % ry);
    const int x = (int)(r / ry);
    int gx = x + j.origin[0], gy = y + j.origin[1], gz = z + j.origin[2];
    if (j.flip & 1) gx = j.sdims[0] - 1 - gx;  // the mirror acts on the volume, before the padding and the crop (RandFlipd; flip_m of a mirrored inference pass)
    if (j.flip & 2) gy = j.sdims[1] - 1 - gy;
    if (j.flip & 4) gz = j.sdims[2] - 1 - gz;
    float v = 0.f;
    if ((unsigned)gx < (unsigned)j.sdims[0] && (unsigned)gy < (unsigned)j.sdims[1] && (unsigned)gz < (unsigned)j.sdims[2]) v = j.src[((int64_t)gx * j.sdims[1] + gy) * j.sdims[2] + gz];
    out[i] = v;
  }
}
extern "C" int vsseg_crop_flip(const void* jobs, int32_t njobs, float* dst, const int32_t roi[3], void* stream) {
  VSSEG_CHECK(jobs && dst && njobs >= 1 && roi[0] > 0 && roi[1] > 0 && roi[2] > 0, "vsseg_crop_flip: bad arguments");
  const int64_t per = (int64_t)roi[0] * roi[1] * roi[2];
  dim3 grid(grid_for(per, 256, 2048), njobs);
  hipLaunchKernelGGL(crop_flip_kernel, grid, dim3(256), 0, as_stream(stream), (const vsseg_crop_job*)jobs, dst, roi[0], roi[1], roi[2]);
  VSSEG_LAUNCH_CHECK("vsseg_crop_flip");
  return VSSEG_OK;
}

// ---- vsseg_crop_affine / vsseg_crop_field: the resampling gather of the training augmentation (semantics: include/vsseg_hip.h) ----
// blockIdx.y = job (the record and its matrix are wave-uniform: scalar loads), blockIdx.z = x, lanes run along (y, z / 4): a thread owns four consecutive z of one output row
// and, when rz % 4 == 0, stores them as 16 bytes.  The shipped augmentation rotates about z, so the taps of a wave fall on contiguous source runs.
// One 32-bit division per thread (row index from the quad index), none per voxel.
// ONE kernel template serves both entry points: crop_gather_kernel<vsseg_affine_job> is vsseg_crop_affine, crop_gather_kernel<vsseg_field_job> adds the B-spline field
// (deformation of the patch coordinates, multiplicative bias); every `if constexpr (FIELD)` block below is compiled out of the first.
__device__ __forceinline__ float affine_coord(const float* __restrict__ r, float x, float y, float z) { return __builtin_fmaf(r[2], z, __builtin_fmaf(r[1], y, __builtin_fmaf(r[0], x, r[3]))); }
// a coordinate with every tap outside stays outside when it is clamped to [-2, dim + 1]; NaN becomes -2.  The conversions to int below are then always in range.
__device__ __forceinline__ float affine_clamp(float s, int dim) { return fminf(fmaxf(s, -2.f), (float)dim + 1.f); }
__device__ __forceinline__ float affine_tap(const float* __restrict__ src, int ix, int iy, int iz, int sx, int sy, int sz) {
  const bool in = (unsigned)ix < (unsigned)sx && (unsigned)iy < (unsigned)sy && (unsigned)iz < (unsigned)sz;
  return in ? src[((int64_t)ix * sy + iy) * sz + iz] : 0.f;  // an outside tap is never addressed
}
__device__ __forceinline__ float affine_u01(unsigned w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }
__device__ __forceinline__ void affine_normals(uint64_t g, uint32_t stream, uint2 key, float n[4]) {
  const uint4 r = philox4x32_10(make_uint4((unsigned)g, (unsigned)(g >> 32), stream, 0u), key);
  const float a0 = sqrtf(-2.f * logf(affine_u01(r.x))), a1 = sqrtf(-2.f * logf(affine_u01(r.z)));
  float s0, c0, s1, c1;
  sincosf(6.2831853f * affine_u01(r.y), &s0, &c0);
  sincosf(6.2831853f * affine_u01(r.w), &s1, &c1);
  n[0] = a0 * c0; n[1] = a0 * s0; n[2] = a1 * c1; n[3] = a1 * s1;
}
// The field of vsseg_crop_field: a lattice of Philox values interpolated by uniform cubic B-splines.  x = blockIdx.z is workgroup-uniform, so the workgroup first reduces
// the four x-layers of the lattice with its x-weights into a table of (y node, z node) -> (c_x, c_y, c_b) in LDS: one pass of 4 Philox calls per node, over the y nodes that
// the rows of this workgroup touch and every z node.  A voxel is then a 4 x 4 sum over that table; a thread reduces over y once per z cell (its four voxels share the
// y-weights, and with spacing_z % 4 == 0 the cell) and over z per voxel.  Lanes of a wave read the same or neighbouring table entries: 16-byte LDS reads, mostly broadcast.
struct field_grid {
  int sx, sy, sz;  // spacing
  int ny, nz;      // lattice nodes along y and z
};
constexpr int FIELD_MAX_NODES = 1024;  // ny * nz the table can hold (16 KiB of LDS): the limit stated in the header
__device__ __forceinline__ void bspline_weights(float f, float w[4]) {
  const float g = 1.f - f, f2 = f * f, k = 0.16666667f;
  w[0] = g * g * g * k;
  w[1] = __builtin_fmaf(f2, __builtin_fmaf(3.f, f, -6.f), 4.f) * k;
  w[2] = __builtin_fmaf(f, __builtin_fmaf(f, __builtin_fmaf(-3.f, f, 3.f), 3.f), 1.f) * k;
  w[3] = f2 * f * k;
}
template <class Job>
__global__ __launch_bounds__(256) void crop_gather_kernel(const Job* __restrict__ jobs, float* __restrict__ dst, int rx, int ry, int rz, int nzq, uint64_t seed, field_grid fg) {
  constexpr bool FIELD = std::is_same<Job, vsseg_field_job>::value;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if constexpr (!FIELD)
    if (t >= ry * nzq) return;
  const Job j = jobs[blockIdx.y];
  const int x = blockIdx.z;
  const uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
  [[maybe_unused]] __shared__ float4 tab[FIELD ? FIELD_MAX_NODES : 1];
  [[maybe_unused]] bool field_on = false;  // job-uniform: a job with both ranges 0 (every label job of a bias-only launch) builds no table
  [[maybe_unused]] int jy0 = 0;            // first y node of the table
  if constexpr (FIELD) {
    field_on = j.elastic_mag != 0.f || j.bias_log != 0.f;
    if (field_on) {  // every thread of the workgroup arrives here or none: the barrier is safe
      const int ylo = (blockIdx.x * 256) / nzq, yhi = min(ry - 1, (blockIdx.x * 256 + 255) / nzq);
      jy0 = ylo / fg.sy;
      const int nodes = (yhi / fg.sy + 4 - jy0) * fg.nz;  // <= ny * nz <= FIELD_MAX_NODES (checked on the host)
      const int i0 = x / fg.sx;
      float wx[4];
      bspline_weights((float)(x - i0 * fg.sx) / (float)fg.sx, wx);
      for (int n = threadIdx.x; n < nodes; n += 256) {
        const int a = n / fg.nz, k = n - a * fg.nz;
        float cx = 0.f, cy = 0.f, cb = 0.f;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
          const uint64_t id = ((uint64_t)(i0 + l) * fg.ny + (jy0 + a)) * fg.nz + k;
          const uint4 r = philox4x32_10(make_uint4((unsigned)id, (unsigned)(id >> 32), j.noise_stream, 1u), key);
          cx = __builtin_fmaf(wx[l], __builtin_fmaf(2.f, affine_u01(r.x), -1.f), cx);
          cy = __builtin_fmaf(wx[l], __builtin_fmaf(2.f, affine_u01(r.y), -1.f), cy);
          cb = __builtin_fmaf(wx[l], __builtin_fmaf(2.f, affine_u01(r.z), -1.f), cb);
        }
        tab[n] = make_float4(cx, cy, cb, 0.f);
      }
      __syncthreads();
    }
    if (t >= ry * nzq) return;
  }
  const int y = t / nzq, z0 = (t - y * nzq) * 4;
  const int sx = j.sdims[0], sy = j.sdims[1], sz = j.sdims[2];
  const int64_t row = ((int64_t)x * ry + y) * rz;  // flattened patch index of (x, y, 0)
  [[maybe_unused]] float wy[4];
  [[maybe_unused]] float col[4][3];  // the table reduced over y, for the z nodes have_k .. have_k + 3
  [[maybe_unused]] int ay = 0, kz = 0, fz_rem = 0, have_k = -1;
  if constexpr (FIELD) {
    if (field_on) {
      const int qy = y / fg.sy;
      bspline_weights((float)(y - qy * fg.sy) / (float)fg.sy, wy);
      ay = (qy - jy0) * fg.nz;
      kz = z0 / fg.sz;
      fz_rem = z0 - kz * fg.sz;
    }
  }
  uint64_t have = ~0ull;  // the Philox group whose four normals are in nrm
  float nrm[4] = {0.f, 0.f, 0.f, 0.f};
  float v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int z = z0 + e;  // z >= rz (the tail of a row with rz % 4 != 0) is computed like any other voxel and not stored
    float fx = (float)x, fy = (float)y;
    const float fz = (float)z;
    [[maybe_unused]] float blog = 0.f;
    if constexpr (FIELD) {
      if (field_on) {
        const int kc = min(kz, fg.nz - 4);  // (only a voxel of the tail can lie past the last cell: it stays inside the table)
        if (kc != have_k) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int a = 0; a < 4; ++a) {
              const float4 n = tab[ay + a * fg.nz + kc + c];
              s0 = __builtin_fmaf(wy[a], n.x, s0);
              s1 = __builtin_fmaf(wy[a], n.y, s1);
              s2 = __builtin_fmaf(wy[a], n.z, s2);
            }
            col[c][0] = s0; col[c][1] = s1; col[c][2] = s2;
          }
          have_k = kc;
        }
        float wz[4];
        bspline_weights((float)fz_rem / (float)fg.sz, wz);
        float f0 = 0.f, f1 = 0.f, f2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          f0 = __builtin_fmaf(wz[c], col[c][0], f0);
          f1 = __builtin_fmaf(wz[c], col[c][1], f1);
          f2 = __builtin_fmaf(wz[c], col[c][2], f2);
        }
        fx = fx + j.elastic_mag * f0;  // the deformation acts in patch space; d_z = 0
        fy = fy + j.elastic_mag * f1;
        blog = j.bias_log * f2;
        if (++fz_rem == fg.sz) {
          fz_rem = 0;
          ++kz;
        }
      }
    }
    const float cx = affine_clamp(affine_coord(j.m + 0, fx, fy, fz), sx), cy = affine_clamp(affine_coord(j.m + 4, fx, fy, fz), sy), cz = affine_clamp(affine_coord(j.m + 8, fx, fy, fz), sz);
    float r;
    if (j.interp == 0) {
      const float bx = floorf(cx), by = floorf(cy), bz = floorf(cz);
      const float tx = cx - bx, ty = cy - by, tz = cz - bz, ux = 1.f - tx, uy = 1.f - ty, uz = 1.f - tz;
      const int ix = (int)bx, iy = (int)by, iz = (int)bz;
      const float v000 = affine_tap(j.src, ix, iy, iz, sx, sy, sz), v001 = affine_tap(j.src, ix, iy, iz + 1, sx, sy, sz);
      const float v010 = affine_tap(j.src, ix, iy + 1, iz, sx, sy, sz), v011 = affine_tap(j.src, ix, iy + 1, iz + 1, sx, sy, sz);
      const float v100 = affine_tap(j.src, ix + 1, iy, iz, sx, sy, sz), v101 = affine_tap(j.src, ix + 1, iy, iz + 1, sx, sy, sz);
      const float v110 = affine_tap(j.src, ix + 1, iy + 1, iz, sx, sy, sz), v111 = affine_tap(j.src, ix + 1, iy + 1, iz + 1, sx, sy, sz);
      r = (ux * uy) * (uz * v000 + tz * v001) + (ux * ty) * (uz * v010 + tz * v011) + (tx * uy) * (uz * v100 + tz * v101) + (tx * ty) * (uz * v110 + tz * v111);
    } else {
      r = affine_tap(j.src, (int)floorf(cx + 0.5f), (int)floorf(cy + 0.5f), (int)floorf(cz + 0.5f), sx, sy, sz);
    }
    if constexpr (FIELD) r = r * expf(blog);  // expf(0) = 1: a job without bias field keeps its bits
    r = __builtin_fmaf(r, j.gain, j.bias);
    if (j.noise_std != 0.f) {
      const uint64_t i = (uint64_t)(row + z), g = i >> 2;
      if (g != have) {  // rz % 4 == 0: one Philox call for the four voxels of the thread
        affine_normals(g, j.noise_stream, key, nrm);
        have = g;
      }
      const int k = (int)(i & 3);
      r = __builtin_fmaf(j.noise_std, k == 0 ? nrm[0] : k == 1 ? nrm[1] : k == 2 ? nrm[2] : nrm[3], r);
    }
    v[e] = r;
  }
  float* out = dst + (int64_t)blockIdx.y * ((int64_t)rx * ry * rz) + row + z0;
  if ((rz & 3) == 0) {
    *reinterpret_cast<float4*>(out) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (z0 + e < rz) out[e] = v[e];
  }
}
static bool affine_finite(float f) { return f - f == 0.f; }
// the argument checks both entry points share (on the caller's host copy of the records); `who` names the entry point in the message
template <class Job>
static int crop_gather_check(const char* who, const Job* jobs_host, const void* jobs_dev, int32_t njobs, const float* dst, const int32_t* roi) {
  VSSEG_CHECK(jobs_host && jobs_dev && dst && roi, "%s: null pointer", who);
  VSSEG_CHECK(njobs >= 1 && njobs <= 65535, "%s: njobs = %d outside [1, 65535]", who, njobs);
  VSSEG_CHECK(roi[0] > 0 && roi[1] > 0 && roi[2] > 0 && roi[0] <= 65535 && (int64_t)roi[1] * ((roi[2] + 3) / 4) < (1ll << 31) - 256, "%s: bad roi (%d, %d, %d)", who, roi[0], roi[1], roi[2]);
  VSSEG_CHECK(((uintptr_t)dst & 15) == 0, "%s: misaligned dst (16 bytes)", who);
  for (int32_t i = 0; i < njobs; ++i) {
    const Job& j = jobs_host[i];
    VSSEG_CHECK(j.src, "%s: job %d: null src pointer", who, i);
    VSSEG_CHECK(j.sdims[0] > 0 && j.sdims[1] > 0 && j.sdims[2] > 0, "%s: job %d: bad sdims (%d, %d, %d)", who, i, j.sdims[0], j.sdims[1], j.sdims[2]);
    VSSEG_CHECK(j.interp == 0 || j.interp == 1, "%s: job %d: interp = %d (0 trilinear, 1 nearest)", who, i, j.interp);
    bool fin = affine_finite(j.gain) && affine_finite(j.bias) && affine_finite(j.noise_std);
    for (int k = 0; k < 12; ++k) fin = fin && affine_finite(j.m[k]);
    VSSEG_CHECK(fin, "%s: job %d: non-finite m, gain, bias or noise_std", who, i);
  }
  return VSSEG_OK;
}
extern "C" int vsseg_crop_affine(const vsseg_affine_job* jobs_host, const void* jobs_dev, int32_t njobs, float* dst, const int32_t roi[3], uint64_t seed, void* stream) {
  if (const int rc = crop_gather_check("vsseg_crop_affine", jobs_host, jobs_dev, njobs, dst, roi)) return rc;
  const int nzq = (roi[2] + 3) / 4;
  dim3 grid((roi[1] * nzq + 255) / 256, njobs, roi[0]);
  hipLaunchKernelGGL(crop_gather_kernel<vsseg_affine_job>, grid, dim3(256), 0, as_stream(stream), (const vsseg_affine_job*)jobs_dev, dst, roi[0], roi[1], roi[2], nzq, seed, field_grid{});
  VSSEG_LAUNCH_CHECK("vsseg_crop_affine");
  return VSSEG_OK;
}
extern "C" int vsseg_crop_field(const vsseg_field_job* jobs_host, const void* jobs_dev, int32_t njobs, float* dst, const int32_t roi[3], const int32_t spacing[3], uint64_t seed, void* stream) {
  if (const int rc = crop_gather_check("vsseg_crop_field", jobs_host, jobs_dev, njobs, dst, roi)) return rc;
  VSSEG_CHECK(spacing, "vsseg_crop_field: null pointer");
  VSSEG_CHECK(spacing[0] >= 1 && spacing[1] >= 1 && spacing[2] >= 1, "vsseg_crop_field: bad spacing (%d, %d, %d): at least 1", spacing[0], spacing[1], spacing[2]);
  const float mag_max = 0.25f * (float)(spacing[0] < spacing[1] ? spacing[0] : spacing[1]);
  for (int32_t i = 0; i < njobs; ++i) {
    const vsseg_field_job& j = jobs_host[i];
    VSSEG_CHECK(affine_finite(j.elastic_mag) && affine_finite(j.bias_log) && j.elastic_mag >= 0.f && j.bias_log >= 0.f, "vsseg_crop_field: job %d: elastic_mag or bias_log negative or non-finite", i);
    VSSEG_CHECK(j.elastic_mag <= mag_max, "vsseg_crop_field: job %d: elastic_mag = %g above min(spacing_x, spacing_y) / 4 = %g (the deformation could fold)", i, (double)j.elastic_mag, (double)mag_max);
  }
  const field_grid fg{spacing[0], spacing[1], spacing[2], (roi[1] - 1) / spacing[1] + 4, (roi[2] - 1) / spacing[2] + 4};
  VSSEG_CHECK((int64_t)fg.ny * fg.nz <= FIELD_MAX_NODES, "vsseg_crop_field: lattice of %d x %d nodes along y, z: the kernel cannot hold more than %d (a larger spacing)", fg.ny, fg.nz, FIELD_MAX_NODES);
  const int nzq = (roi[2] + 3) / 4;
  dim3 grid((roi[1] * nzq + 255) / 256, njobs, roi[0]);
  hipLaunchKernelGGL(crop_gather_kernel<vsseg_field_job>, grid, dim3(256), 0, as_stream(stream), (const vsseg_field_job*)jobs_dev, dst, roi[0], roi[1], roi[2], nzq, seed, fg);
  VSSEG_LAUNCH_CHECK("vsseg_crop_field");
  return VSSEG_OK;
}

// NormalizeIntensityd: (x - mean) / std over the whole image, population std, no division when std == 0.
// Pass 1: fp64 sum / sum of squares (sharded atomics); pass 2 applies.  acc = 2 doubles, zeroed by the caller.
__global__ void intensity_sums_kernel(const float* __restrict__ x, int64_t n, double* __restrict__ acc) {
  double s = 0.0, q = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const double v = x[i];
    s += v;
    q += v * v;
  }
  s = wave_sum_d(s);
  q = wave_sum_d(q);
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&acc[0], s);
    atomicAdd(&acc[1], q);
  }
}
__global__ void intensity_apply_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n, const double* __restrict__ acc) {
  const double mean = acc[0] / (double)n;
  double var = acc[1] / (double)n - mean * mean;
  if (var < 0.0) var = 0.0;
  const double sd = sqrt(var);
  const float m = (float)mean, inv = sd == 0.0 ? 1.f : (float)(1.0 / sd);
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) y[i] = (x[i] - m) * inv;
}
extern "C" int vsseg_normalize_intensity(const float* x, float* y, int64_t n, double* acc2, void* stream) {
  VSSEG_CHECK(x && y && acc2 && n > 0, "vsseg_normalize_intensity: bad arguments");
  hipStream_t s = as_stream(stream);
  if (hipMemsetAsync(acc2, 0, 2 * sizeof(double), s) != hipSuccess) { vsseg_set_error("vsseg_normalize_intensity: memset failed"); return VSSEG_ELAUNCH; }
  hipLaunchKernelGGL(intensity_sums_kernel, dim3(grid_for(n, 256, 1024)), dim3(256), 0, s, x, n, acc2);
  hipLaunchKernelGGL(intensity_apply_kernel, dim3(grid_for(n, 256, 2048)), dim3(256), 0, s, x, y, n, acc2);
  VSSEG_LAUNCH_CHECK("vsseg_normalize_intensity");
  return VSSEG_OK;
}
