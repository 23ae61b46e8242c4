// Gaussian-weighted sliding-window blend (MONAI 0.4.0 sliding_window_inference steps 6-7, SURVEY.md App. B;
// call site ref:params/VSparams.py:568-574).  Windows are blended one after the other in the reference's window
// order, each voxel doing the same `out += map*seg; cnt += map` fp32 sequence as the reference, so the result does
// not depend on how windows were distributed over GPUs.
#include "common.h"

__global__ void swi_accumulate_kernel(const float* __restrict__ seg, const float* __restrict__ imap, int rx, int ry, int rz, int sx, int sy, int sz, int c,
                                      float* __restrict__ out, float* __restrict__ cnt, int px, int py, int pz) {
  const int64_t total = (int64_t)rx * ry * rz;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int z = (int)(i % rz);
    int64_t r = i / rz;
    int y = (int)(r % ry), x = (int)(r / ry);
    const int64_t o = (((int64_t)(sx + x)) * py + (sy + y)) * pz + (sz + z);
    const float w = imap[i];
    if (seg != nullptr)
      for (int k = 0; k < c; ++k) out[o * c + k] += w * seg[i * c + k];
    if (cnt != nullptr) cnt[o] += w;
  }
}
extern "C" int vsseg_swi_accumulate(const float* seg, const float* imap, const int32_t roi[3], const int32_t start[3], int32_t c, float* out, float* cnt, const int32_t pdims[3], void* stream) {
  VSSEG_CHECK(imap && ((seg && out) || cnt) && (!seg || out) && c >= 1, "vsseg_swi_accumulate: bad arguments");  // seg == NULL: only the weight map; cnt == NULL: only the blend
  for (int a = 0; a < 3; ++a) VSSEG_CHECK(start[a] >= 0 && start[a] + roi[a] <= pdims[a], "vsseg_swi_accumulate: window outside the padded volume (dim %d)", a);
  int64_t total = (int64_t)roi[0] * roi[1] * roi[2];
  hipLaunchKernelGGL(swi_accumulate_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), seg, imap, roi[0], roi[1], roi[2], start[0], start[1], start[2], c, out, cnt, pdims[0], pdims[1], pdims[2]);
  VSSEG_LAUNCH_CHECK("vsseg_swi_accumulate");
  return VSSEG_OK;
}

__global__ void swi_finalize_kernel(const float* __restrict__ out, const float* __restrict__ cnt, int px, int py, int pz, int bx, int by, int bz, int dx, int dy, int dz, int c, float* __restrict__ dst) {
  const int64_t total = (int64_t)dx * dy * dz;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int z = (int)(i % dz);
    int64_t r = i / dz;
    int y = (int)(r % dy), x = (int)(r / dy);
    const int64_t o = (((int64_t)(bx + x)) * py + (by + y)) * pz + (bz + z);
    const float w = cnt[o];
    for (int k = 0; k < c; ++k) dst[i * c + k] = out[o * c + k] / w;
  }
}
extern "C" int vsseg_swi_finalize(const float* out, const float* cnt, const int32_t pdims[3], const int32_t pad_before[3], const int32_t dims[3], int32_t c, float* dst, void* stream) {
  VSSEG_CHECK(out && cnt && dst && c >= 1, "vsseg_swi_finalize: bad arguments");
  int64_t total = (int64_t)dims[0] * dims[1] * dims[2];
  hipLaunchKernelGGL(swi_finalize_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), out, cnt, pdims[0], pdims[1], pdims[2], pad_before[0], pad_before[1], pad_before[2], dims[0], dims[1], dims[2], c, dst);
  VSSEG_LAUNCH_CHECK("vsseg_swi_finalize");
  return VSSEG_OK;
}

// One pass of mirrored test-time augmentation folded into the running sum: the blend ran in the frame of the mirrored volume, this un-mirrors it while it normalises.  A thread owns
// one image voxel (dst is written z-contiguous; on a mirrored z the wave reads its row of `out` / `cnt` back to front, the same cache lines).  `out[o*c+k] / w` is the expression of
// swi_finalize_kernel, so every pass's quotient has the bits of a plain sliding_window_inference of the mirrored volume.
__global__ void swi_finalize_mirrored_kernel(const float* __restrict__ out, const float* __restrict__ cnt, int px, int py, int pz, int bx, int by, int bz, int dx, int dy, int dz, int c, int mirror,
                                             int softmax, int first, float scale, float* __restrict__ dst) {
  const int64_t total = (int64_t)dx * dy * dz;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int z = (int)(i % dz);
    int64_t r = i / dz;
    int y = (int)(r % dy), x = (int)(r / dy);
    if (mirror & 1) x = dx - 1 - x;
    if (mirror & 2) y = dy - 1 - y;
    if (mirror & 4) z = dz - 1 - z;
    const int64_t o = (((int64_t)(bx + x)) * py + (by + y)) * pz + (bz + z);
    const float w = cnt[o];
    float top = 0.f, sum = 1.f;
    if (softmax) {  // exp(v - max) / sum over the c channels (the rows are re-read from L1: c is 2 in the product, and unbounded here)
      top = out[o * c] / w;
      for (int k = 1; k < c; ++k) top = fmaxf(top, out[o * c + k] / w);
      sum = 0.f;
      for (int k = 0; k < c; ++k) sum += expf(out[o * c + k] / w - top);
    }
    for (int k = 0; k < c; ++k) {
      float v = out[o * c + k] / w;
      if (softmax) v = expf(v - top) / sum;
      dst[i * c + k] = (first ? v : dst[i * c + k] + v) * scale;
    }
  }
}
extern "C" int vsseg_swi_finalize_mirrored(const float* out, const float* cnt, const int32_t pdims[3], const int32_t pad_before[3], const int32_t dims[3], int32_t c, int32_t mirror, int32_t softmax,
                                           int32_t first, float scale, float* dst, void* stream) {
  VSSEG_CHECK(out && cnt && dst && c >= 1 && mirror >= 0 && mirror <= 7 && scale > 0.f, "vsseg_swi_finalize_mirrored: bad arguments");
  for (int a = 0; a < 3; ++a)
    VSSEG_CHECK(dims[a] >= 1 && pad_before[a] >= 0 && pad_before[a] + dims[a] <= pdims[a], "vsseg_swi_finalize_mirrored: image outside the padded volume (dim %d)", a);
  int64_t total = (int64_t)dims[0] * dims[1] * dims[2];
  hipLaunchKernelGGL(swi_finalize_mirrored_kernel, dim3(grid_for(total, 256)), dim3(256), 0, as_stream(stream), out, cnt, pdims[0], pdims[1], pdims[2], pad_before[0], pad_before[1], pad_before[2], dims[0],
                     dims[1], dims[2], c, mirror, softmax, first, scale, dst);
  VSSEG_LAUNCH_CHECK("vsseg_swi_finalize_mirrored");
  return VSSEG_OK;
}
