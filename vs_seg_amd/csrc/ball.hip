// Ball morphology of the foreground of a two-class prediction at a radius in mm: dilation, erosion, closing and opening with the ellipsoid of voxel offsets that an
// anisotropic voxel spacing makes of a ball.  One volume per call, as a sequence of launches on the caller's stream (no host synchronisation, no allocation).
// Foreground P = logits[v][1] > logits[v][0] (vsseg_pred_fg: ties and NaN are background).
//
// The ball.  An integer offset d has the squared length f(d) = fmaf(ax, ax, fmaf(ay, ay, az * az)) in fp32 with a_a = s_a * (float)d_a: the z -> y -> x accumulation of
// surf_edt_kernel.  d belongs to the ball when f(d) <= t2 = (float)((double)r * (double)r); a tie belongs.  dilate(M) = the voxels of the volume with a voxel of M at a
// ball offset; erode(M) = the voxels with no BACKGROUND VOXEL OF THE VOLUME at a ball offset (positions outside the volume are ignored: they are neither foreground
// nor background, so a mask cut by the field of view does not shrink there); close = erode(dilate), open = dilate(erode).  With "features" = the voxels of M (dilation)
// or the background voxels of the volume (erosion), both are one test: F(v) = min over the features u of f(u - v) <= t2; dilate = F, erode = NOT F (a background voxel is
// its own feature at f(0) = 0 <= t2).
//
// Separable and banded.  Rounding is monotone, so fmaf(a, a, c) does not decrease when c grows, and the minimum over all features of f equals
//   min over dx of fmaf(ax, ax, min over dy of fmaf(ay, ay, min over dz of az * az)),
// the three per-axis steps below.  Each step looks h_a = reach_a + 1 voxels to either side only, reach_a = floor(r / s_a) in fp64.  That band is exact where it matters:
// a feature that the compare accepts has round(a_a^2) <= f(d) <= t2 on every axis (again monotone rounding, every addend >= 0), and an offset of reach_a + 2 or more has
// a_a^2 >= r^2 * (1 + 1 / (reach_a + 1))^2 >= r^2 * (1 + 1 / 33)^2, far beyond the few 2^-24 by which the fp32 products and t2 can be off.  So every acceptable feature lies
// inside the band (an offset of reach_a + 1 may be accepted when r / s_a is within rounding of an integer, hence the + 1), the banded minimum is never below the true one,
// and the two are equal whenever either is <= t2.  No feature in the band: +inf.
//
//   init    zero the record in scratch (|P|, bounding box of P) and the four statistics
//   scan    the logits of the whole volume once (8 B per voxel): |P| and the bounding box of P into the record
//   stage   (one for dilate / erode, two for close / open), confined to the work box W = bounding box of P grown by h_a per axis and clipped to the volume:
//     zy    a tile is BT_Y rows of 64 z of one x plane.  The workgroup stages the feature bytes of its rows with a halo of h_y rows and h_z columns in LDS (first stage:
//           from the logits; second stage: from the first stage's byte mask), takes per staged row the distance to the nearest feature along z within the band
//           (az * az, or +inf), then per output row the minimum over dy of fmaf(ay, ay, .), and writes one fp32 per voxel of W.
//     x     a tile is BT_X planes of 64 z of one row y.  The workgroup stages the fp32 field with a halo of h_x planes, takes the minimum over dx, compares with t2 and
//           writes one byte per voxel of W: the mask after this stage.
//   write   the one-hot result for the whole volume (8 B per voxel); inside W it reads the last stage's mask and the logits again, counts |P|, |result|, |result \ P| and
//           |P \ result|, and adds them to the statistics with one set of integer atomics per workgroup that counted anything.
//
// Why W suffices.  Every mask that occurs (P, the first stage's, the result) lies inside W: a dilation grows a mask by at most h_a, an erosion shrinks it.  A position
// outside W therefore is background if it lies in the volume and nothing if it does not, and a stage that looks beyond W needs no memory for it: the loaders below
// supply "not a feature" outside the volume, and inside the volume but outside W "not a feature" for a dilation and "a feature" for an erosion.  Growing W by twice the
// reach, so that every feature an erosion can meet has a byte of its own, would compute the same masks over a larger box.  An empty P has an empty W: the stages exit
// and the write pass stores background.
//
// Grids depend on dims alone: a stage kernel counts its tiles from the corner of W and walks them with a grid-sized stride, with as many workgroups as the whole
// volume has tiles, at most 2048; workgroups without a tile exit at once.  No kernel
// waits for another workgroup, and only integer atomics combine workgroups: a call is bit-identical from run to run.
#include <math.h>
#include "volume.h"

namespace {

constexpr int BALL_MAX_EXTENT = 8192;
constexpr int BALL_MAX_REACH = 32;  // voxels per axis; the band is one more
constexpr int BT_Z = 64;            // every tile: 64 consecutive z, one per lane
constexpr int BT_Y = 16;            // zy kernel: rows of a tile, four per thread (wave w: rows w, w + 4, w + 8, w + 12)
constexpr int BT_X = 16;            // x kernel: planes of a tile, four per thread
constexpr int BALL_MAX_WG = 2048;   // workgroups of a stage kernel: 8 per compute unit, each walks the tiles of W with that stride
enum BallOp { BALL_DILATE, BALL_ERODE, BALL_CLOSE, BALL_OPEN };

struct BallRec {
  unsigned long long fg;  // |P|
  int bmin[3], bmax[3];   // bounding box of P; bmax = -1: empty
};

struct BallGeom {  // by value in the kernel arguments
  int dim[3];      // X, Y, Z
  int h[3];        // the band per axis: reach + 1
  float s[3];      // mm per voxel
  float t2;        // (float)(r * r), the product in fp64
};

struct BallLayout {
  int64_t field, mask_a, mask_b, total;
};
BallLayout ball_layout(int64_t nvox) {
  BallLayout l;
  l.field = align256(sizeof(BallRec));
  l.mask_a = l.field + align256(nvox * 4);
  l.mask_b = l.mask_a + align256(nvox);
  l.total = l.mask_b + align256(nvox);
  return l;
}

struct BallBox {  // the work box W
  int lo[3], hi[3];
  __device__ __forceinline__ BallBox(const BallRec* rec, const BallGeom& g) {
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = max(rec->bmin[a] - g.h[a], 0), hi[a] = min(rec->bmax[a] + g.h[a], g.dim[a] - 1);
    if (rec->bmax[0] < 0) lo[0] = lo[1] = lo[2] = 0, hi[0] = hi[1] = hi[2] = -1;  // P is empty: so is W (lo = 0 keeps the tile origins below small)
  }
  __device__ __forceinline__ bool holds(int a, int i) const { return i >= lo[a] && i <= hi[a]; }
};

__global__ __launch_bounds__(64) void ball_init_kernel(BallRec* rec, unsigned long long* stats) {
  if (threadIdx.x == 0) rec->fg = 0;
  if (stats && threadIdx.x < 4) stats[threadIdx.x] = 0;
  box_reset(rec->bmin, rec->bmax, 3);
}

__global__ __launch_bounds__(256) void ball_scan_kernel(const float* __restrict__ logits, int Y, int Z, int64_t nvox, BallRec* __restrict__ rec) {
  CountBox<3> box;
  box.clear();
  for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < (unsigned)nvox; v += gridDim.x * 256u) {  // (nvox < 2^31 and the stride < 2^24: no wrap)
    if (!vsseg_pred_fg(reinterpret_cast<const float2*>(logits)[v])) continue;
    const unsigned xy = v / (unsigned)Z, x = xy / (unsigned)Y;
    const int p[3] = {(int)x, (int)(xy - x * (unsigned)Y), (int)(v - xy * (unsigned)Z)};
    ++box.n[0];
    box.grow(p, p);
  }
  box.wave_reduce();
  if ((threadIdx.x & 63) == 0) box.merge<true>(&rec->fg, rec->bmin, rec->bmax);  // one merge per wave: with a look first
}

// The tiles of W that a stage kernel walks: nz x ny x nx of them, counted from the corner of W, tile t -> (t % nz, t / nz % ny, t / (nz ny)).  A workgroup takes the
// tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the grid is sized for the tiles of the whole volume and capped, so a tumour-sized W costs the exit of at most
// BALL_MAX_WG workgroups per launch, not of one workgroup per tile of the volume, and W = the volume is walked by workgroups that stay.
struct BallTiles {
  int nz, ny, nx;
  __device__ __forceinline__ BallTiles(const BallBox& w, int ty, int tx) {
    nz = (w.hi[2] - w.lo[2]) / BT_Z + 1, ny = (w.hi[1] - w.lo[1]) / ty + 1, nx = (w.hi[0] - w.lo[0]) / tx + 1;
    if (w.hi[0] < 0) nz = ny = nx = 0;  // an empty W
  }
  __device__ __forceinline__ long long count() const { return (long long)nz * ny * nx; }
};

// The first two steps of a stage.  LOGITS: the mask is P, read from the logits; otherwise the byte mask `mask` of the stage before.  ERODE: the features are the
// background voxels.  A tile: BT_Y rows of 64 z of one x plane.  Dynamic LDS: fp32 gz[rows][64], then the feature bytes [rows][64 + 2 h_z], rows = BT_Y + 2 h_y.
template <bool LOGITS, bool ERODE>
__global__ __launch_bounds__(256) void ball_zy_kernel(const BallRec* __restrict__ rec, BallGeom g, const float* __restrict__ logits, const uint8_t* __restrict__ mask,
                                                     float* __restrict__ field) {
  extern __shared__ __attribute__((aligned(16))) char ball_lds[];
  const BallBox w(rec, g);
  const BallTiles tiles(w, BT_Y, 1);
  const int Y = g.dim[1], Z = g.dim[2], hy = g.h[1], hz = g.h[2];
  const int rows = BT_Y + 2 * hy, cols = BT_Z + 2 * hz;
  float* gz = reinterpret_cast<float*>(ball_lds);
  uint8_t* ft = reinterpret_cast<uint8_t*>(ball_lds) + (size_t)rows * BT_Z * sizeof(float);
  const float INF = __builtin_inff();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long t = blockIdx.x; t < tiles.count(); t += gridDim.x) {  // (the same trip count in every thread of the workgroup)
    const int tq = (int)(t / tiles.nz);
    const int z0 = w.lo[2] + (int)(t - (long long)tq * tiles.nz) * BT_Z, y0 = w.lo[1] + (tq % tiles.ny) * BT_Y, x = w.lo[0] + tq / tiles.ny;
    for (int i = threadIdx.x; i < rows * cols; i += 256) {
      const int r = i / cols, c = i - r * cols;  // consecutive threads along z
      const int y = y0 - hy + r, z = z0 - hz + c;
      bool f = false;
      if (y >= 0 && y < Y && z >= 0 && z < Z) {  // (outside the volume: never a feature)
        if (w.holds(1, y) && w.holds(2, z)) {
          const int64_t v = ((int64_t)x * Y + y) * Z + z;
          const bool m = LOGITS ? vsseg_pred_fg(reinterpret_cast<const float2*>(logits)[v]) : mask[v] != 0;
          f = m != ERODE;
        } else {
          f = ERODE;  // in the volume, outside W: background
        }
      }
      ft[i] = f ? 1 : 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < rows * BT_Z; i += 256) {
      const uint8_t* row = ft + (i >> 6) * cols + (i & 63) + hz;  // the staged row at this lane's z
      float d = INF;
      for (int k = 0; k <= hz; ++k)
        if (row[-k] | row[k]) {
          const float az = g.s[2] * (float)k;
          d = az * az;
          break;
        }
      gz[i] = d;
    }
    __syncthreads();
    const int z = z0 + lane;
    if (z <= w.hi[2]) {
      float b[BT_Y / 4];
#pragma unroll
      for (int j = 0; j < BT_Y / 4; ++j) b[j] = INF;
      for (int k = 0; k <= 2 * hy; ++k) {
        const float ay = g.s[1] * (float)(k - hy);
#pragma unroll
        for (int j = 0; j < BT_Y / 4; ++j) b[j] = fminf(b[j], fmaf(ay, ay, gz[(wave + 4 * j + k) * BT_Z + lane]));
      }
#pragma unroll
      for (int j = 0; j < BT_Y / 4; ++j) {
        const int y = y0 + wave + 4 * j;
        if (y <= w.hi[1]) field[((int64_t)x * Y + y) * Z + z] = b[j];
      }
    }
    __syncthreads();  // the next tile overwrites ft and gz
  }
}

// The third step of a stage and its compare: out = 1 where the mask after this stage is foreground.  A tile: BT_X planes of 64 z of one row y.  Dynamic LDS: fp32
// [BT_X + 2 h_x][64].
template <bool ERODE>
__global__ __launch_bounds__(256) void ball_x_kernel(const BallRec* __restrict__ rec, BallGeom g, const float* __restrict__ field, uint8_t* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char ball_lds[];
  const BallBox w(rec, g);
  const BallTiles tiles(w, 1, BT_X);
  const int X = g.dim[0], Y = g.dim[1], Z = g.dim[2], hx = g.h[0];
  const int rows = BT_X + 2 * hx;
  float* gy = reinterpret_cast<float*>(ball_lds);
  const float INF = __builtin_inff();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (long long t = blockIdx.x; t < tiles.count(); t += gridDim.x) {
    const int tq = (int)(t / tiles.nz);
    const int z0 = w.lo[2] + (int)(t - (long long)tq * tiles.nz) * BT_Z, y = w.lo[1] + tq % tiles.ny, x0 = w.lo[0] + (tq / tiles.ny) * BT_X;
    const int z = z0 + lane;
    for (int r = wave; r < rows; r += 4) {
      const int x = x0 - hx + r;
      float v = INF;  // outside the volume: no feature
      if (x >= 0 && x < X && z <= w.hi[2]) v = w.holds(0, x) ? field[((int64_t)x * Y + y) * Z + z] : ERODE ? 0.f : INF;  // in the volume, outside W: background
      gy[r * BT_Z + lane] = v;
    }
    __syncthreads();
    if (z <= w.hi[2]) {
      float b[BT_X / 4];
#pragma unroll
      for (int j = 0; j < BT_X / 4; ++j) b[j] = INF;
      for (int k = 0; k <= 2 * hx; ++k) {
        const float ax = g.s[0] * (float)(k - hx);
#pragma unroll
        for (int j = 0; j < BT_X / 4; ++j) b[j] = fminf(b[j], fmaf(ax, ax, gy[(wave + 4 * j + k) * BT_Z + lane]));
      }
#pragma unroll
      for (int j = 0; j < BT_X / 4; ++j) {
        const int x = x0 + wave + 4 * j;
        if (x <= w.hi[0]) out[((int64_t)x * Y + y) * Z + z] = ((b[j] <= g.t2) != ERODE) ? 1 : 0;
      }
    }
    __syncthreads();  // the next tile overwrites gy
  }
}

__global__ __launch_bounds__(256) void ball_write_kernel(const BallRec* __restrict__ rec, BallGeom g, int64_t nvox, const float* __restrict__ logits, const uint8_t* __restrict__ mask,
                                                        float* __restrict__ out, unsigned long long* __restrict__ stats) {
  __shared__ unsigned red[4][4];
  const BallBox w(rec, g);
  const int Y = g.dim[1], Z = g.dim[2];
  unsigned n[4] = {0, 0, 0, 0};  // |P|, |result|, added, removed among this thread's voxels
  for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < (unsigned)nvox; v += gridDim.x * 256u) {  // (nvox < 2^31 and the stride < 2^24: no wrap)
    const unsigned xy = v / (unsigned)Z, x = xy / (unsigned)Y;
    const int z = (int)(v - xy * (unsigned)Z), y = (int)(xy - x * (unsigned)Y);
    bool on = false;
    if (w.holds(0, (int)x) && w.holds(1, y) && w.holds(2, z)) {
      on = mask[v] != 0;
      const bool p = vsseg_pred_fg(reinterpret_cast<const float2*>(logits)[v]);
      n[0] += p, n[1] += on, n[2] += on && !p, n[3] += p && !on;
    }
    const float f = on ? 1.f : 0.f;
    reinterpret_cast<float2*>(out)[v] = make_float2(1.f - f, f);
  }
  if (!stats) return;  // (the same in every thread)
#pragma unroll
  for (int c = 0; c < 4; ++c) n[c] = wave_sum_u(n[c]);
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 4; ++c) red[threadIdx.x >> 6][c] = n[c];
  __syncthreads();
  if (threadIdx.x < 4) {
    const unsigned long long s = (unsigned long long)red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    if (s) atomicAdd(stats + threadIdx.x, s);
  }
}

int div_up(int a, int b) { return (a + b - 1) / b; }

// One stage on `s`: the mask `src` (nullptr: P from the logits) eroded or dilated into `dst`.
void ball_stage(hipStream_t s, const BallRec* rec, const BallGeom& g, bool erode, const float* logits, const uint8_t* src, float* field, uint8_t* dst) {
  const int64_t tiles_zy = (int64_t)div_up(g.dim[2], BT_Z) * div_up(g.dim[1], BT_Y) * g.dim[0], tiles_x = (int64_t)div_up(g.dim[2], BT_Z) * g.dim[1] * div_up(g.dim[0], BT_X);
  const dim3 gzy(grid_for(tiles_zy, 1, BALL_MAX_WG)), gx(grid_for(tiles_x, 1, BALL_MAX_WG));
  const int rows_y = BT_Y + 2 * g.h[1], rows_x = BT_X + 2 * g.h[0];
  const size_t lds_zy = ((size_t)rows_y * BT_Z * sizeof(float) + (size_t)rows_y * (BT_Z + 2 * g.h[2]) + 15) & ~(size_t)15, lds_x = (size_t)rows_x * BT_Z * sizeof(float);
  if (!src && !erode) hipLaunchKernelGGL((ball_zy_kernel<true, false>), gzy, dim3(256), lds_zy, s, rec, g, logits, src, field);
  else if (!src) hipLaunchKernelGGL((ball_zy_kernel<true, true>), gzy, dim3(256), lds_zy, s, rec, g, logits, src, field);
  else if (!erode) hipLaunchKernelGGL((ball_zy_kernel<false, false>), gzy, dim3(256), lds_zy, s, rec, g, logits, src, field);
  else hipLaunchKernelGGL((ball_zy_kernel<false, true>), gzy, dim3(256), lds_zy, s, rec, g, logits, src, field);
  if (erode) hipLaunchKernelGGL(ball_x_kernel<true>, gx, dim3(256), lds_x, s, rec, g, (const float*)field, dst);
  else hipLaunchKernelGGL(ball_x_kernel<false>, gx, dim3(256), lds_x, s, rec, g, (const float*)field, dst);
}

}  // namespace

extern "C" int64_t vsseg_ball_scratch_bytes(const int32_t dims[3]) {
  VSSEG_CHECK(dims_ok(dims, BALL_MAX_EXTENT), "vsseg_ball_scratch_bytes: dims must be 1 .. %d on every axis", BALL_MAX_EXTENT);
  const int64_t nvox = (int64_t)dims[0] * dims[1] * dims[2];
  VSSEG_CHECK(nvox < (int64_t)INT32_MAX, "vsseg_ball_scratch_bytes: dims %d x %d x %d hold %lld voxels, the 32-bit voxel index allows fewer than 2^31 - 1", dims[0], dims[1], dims[2],
              (long long)nvox);
  return ball_layout(nvox).total;
}

extern "C" int vsseg_ball_morphology(const float* logits, int32_t pitch, const int32_t dims[3], const float spacing[3], int32_t op, double radius_mm, void* scratch, int64_t scratch_bytes,
                                     float* out, int64_t* stats, void* stream) {
  const char* name = "vsseg_ball_morphology";
  VOLUME_CHECK_ARGS(name, logits && spacing && scratch && out, " (logits, spacing, scratch, out)", pitch, dims, BALL_MAX_EXTENT, (int64_t)dims[0] * dims[1] * dims[2] < (int64_t)INT32_MAX,
                    " and X * Y * Z < 2^31 - 1", spacing, aligned_to(logits, 8) && aligned_to(out, 8) && aligned_to(stats, 8) && aligned_to(scratch, 256),
                    "logits / out / stats 8 B, scratch 256 B", scratch_bytes, ball_layout((int64_t)dims[0] * dims[1] * dims[2]).total, "vsseg_ball_scratch_bytes");
  VSSEG_CHECK(op >= BALL_DILATE && op <= BALL_OPEN, "%s: op must be 0 (dilate), 1 (erode), 2 (close) or 3 (open), got %d", name, op);
  VSSEG_CHECK(radius_mm >= 0.0 && radius_mm < (double)__builtin_inff(), "%s: radius_mm = %g is not a finite value >= 0", name, radius_mm);
  BallGeom g;
  for (int a = 0; a < 3; ++a) {
    const double reach = floor(radius_mm / (double)spacing[a]);
    VSSEG_CHECK(reach <= (double)BALL_MAX_REACH, "%s: radius_mm = %g reaches %.0f voxels along axis %d (spacing %g mm), at most %d are supported", name, radius_mm, reach, a,
                (double)spacing[a], BALL_MAX_REACH);
    g.dim[a] = dims[a], g.h[a] = (int)reach + 1, g.s[a] = spacing[a];
  }
  g.t2 = (float)(radius_mm * radius_mm);
  const int64_t nvox = (int64_t)dims[0] * dims[1] * dims[2];
  const BallLayout l = ball_layout(nvox);
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  BallRec* rec = reinterpret_cast<BallRec*>(base);
  float* field = reinterpret_cast<float*>(base + l.field);
  uint8_t* mask_a = reinterpret_cast<uint8_t*>(base + l.mask_a);
  uint8_t* mask_b = reinterpret_cast<uint8_t*>(base + l.mask_b);
  const int wg = grid_for(nvox, 256, 256 * 32);
  hipLaunchKernelGGL(ball_init_kernel, dim3(1), dim3(64), 0, s, rec, reinterpret_cast<unsigned long long*>(stats));
  hipLaunchKernelGGL(ball_scan_kernel, dim3(wg), dim3(256), 0, s, logits, dims[1], dims[2], nvox, rec);
  const bool first_erodes = op == BALL_ERODE || op == BALL_OPEN, two = op == BALL_CLOSE || op == BALL_OPEN;
  ball_stage(s, rec, g, first_erodes, logits, nullptr, field, mask_a);
  if (two) ball_stage(s, rec, g, !first_erodes, logits, mask_a, field, mask_b);
  hipLaunchKernelGGL(ball_write_kernel, dim3(wg), dim3(256), 0, s, (const BallRec*)rec, g, nvox, logits, (const uint8_t*)(two ? mask_b : mask_a), out,
                     reinterpret_cast<unsigned long long*>(stats));
  VSSEG_LAUNCH_CHECK(name);
  return VSSEG_OK;
}
