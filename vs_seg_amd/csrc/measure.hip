// Size and position of a two-class segmentation and of its label: voxel count, volume, distance between the two centres of mass, and the largest
// distance between two voxel centres of a mask in 3-D (the Feret diameter, pyradiomics' Maximum3DDiameter between voxel centres) and within one
// axial slice (pairs with equal z).  One volume per call, as a sequence of launches on the caller's stream (no host synchronisation, no
// allocation, no kernel waits for another workgroup); P = argmax of the two logits (ties and NaN -> background), G = ((int)label == 1):
//
//   init      the record (counts, index sums, (y, z) bounding boxes, maxima) and the four column tables in scratch
//   stream    one pass over the volume, 12 B per voxel (8 B without a label): the only pass whose cost grows with the volume.  A workgroup owns 256
//             consecutive (y, z) columns x MS_XC planes; a thread walks its column along x.  Per mask: |M| and the sums of the x, y, z indices (64-bit
//             integer atomics, one set per workgroup after wave reductions), the bounding box in (y, z), and the smallest / largest foreground x of
//             every column (integer atomicMin / atomicMax: the pieces of a column that several workgroups hold merge into a function of the mask).
//   pair      the farthest pair.  With dy and dz fixed a pair whose x extent can grow is not the farthest, so it lies among the x extremes of the
//             columns; for two columns a, b the largest |xa - xb| is max(xmax_a - xmin_b, xmax_b - xmin_a), and one evaluation per COLUMN pair
//             covers the four voxel pairs.  Columns are tiled MP_T x MP_T in (y, z); workgroup (i, k-chunk) holds the columns of tile i in
//             registers and stages tile j = (i + k) mod nT in LDS for k <= nT / 2 (every unordered tile pair is met, the load is the same for every
//             i).  Equal-z pairs of the two tiles (same z tile only) give the axial maximum.  Tiles outside the mask's bounding box, which lives in
//             device memory, exit at once, and so do tiles of empty columns inside it: a small tumour in a large volume costs a few tile pairs, with
//             a far island as well.  Quadratic in the occupied columns, hence the domain Y * Z <= 2^18.
//   finalize  the nine fp64 outputs; the square root is taken once, in fp64.
//
// d^2 = (sx dx)^2 + (sy dy)^2 + (sz dz)^2 is formed in fp32 from exact integer differences; its maximum is taken over the bit patterns (non-negative
// floats order like their uint32 bits), with an unsigned atomicMax: nothing depends on the order in which workgroups finish.
#include <math.h>
#include "volume.h"

namespace {

constexpr int MS_XC = 32;              // stream pass: x planes per workgroup
constexpr int MS_U = 8;                // ... loads in flight per thread
constexpr int MP_T = 16;               // pair stage: a tile is MP_T x MP_T columns, one per thread
constexpr int MP_KC = 4;               // ... tile offsets k per workgroup
constexpr int MEAS_MAX_EXTENT = 8192;
constexpr int MEAS_MAX_COLUMNS = 1 << 18;
constexpr int MEAS_EMPTY = 1 << 20;    // an empty column holds xmin = MEAS_EMPTY, xmax = -MEAS_EMPTY: its x extent against any column is negative

struct MeasRec {                       // index 0: P, 1: G
  unsigned long long cnt[2];
  unsigned long long sum[2][3];        // sums of the x, y, z indices
  int bmin[2][2], bmax[2][2];          // bounding box in (y, z); bmax = -1: empty mask
  unsigned best[2][2];                 // fp32 bits of the largest d^2: all pairs, pairs with equal z
};

inline int64_t meas_tables_offset() { return align256(sizeof(MeasRec)); }
inline int64_t meas_total(int64_t ncol) { return meas_tables_offset() + align256(4 * ncol * (int64_t)sizeof(int)); }  // tables [mask][min, max][Y * Z]

__global__ __launch_bounds__(256) void meas_init_kernel(MeasRec* __restrict__ rec, int* __restrict__ tab, int ncol) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < ncol) {
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      tab[(2 * m) * (int64_t)ncol + c] = MEAS_EMPTY;
      tab[(2 * m + 1) * (int64_t)ncol + c] = -MEAS_EMPTY;
    }
  }
  if (blockIdx.x == 0) {
    unsigned* w = reinterpret_cast<unsigned*>(rec);
    for (int i = threadIdx.x; i < (int)(sizeof(MeasRec) / 4); i += 256) w[i] = 0;
    __syncthreads();
    box_reset(&rec->bmin[0][0], &rec->bmax[0][0], 4);  // the two (y, z) boxes
  }
}

template <bool HAS_LABEL>
__global__ __launch_bounds__(256) void meas_stream_kernel(const float* __restrict__ logits, const float* __restrict__ label, int X, int Z, int ncol, int* __restrict__ tab,
                                                         MeasRec* __restrict__ rec) {
  constexpr int NM = HAS_LABEL ? 2 : 1;
  __shared__ CountBox<2> red[2][4];  // mask, wave
  __shared__ unsigned sums[2][4][3];
  const int c = blockIdx.x * 256 + threadIdx.x;
  const int x0 = blockIdx.y * MS_XC;
  const int x1 = c < ncol ? min(x0 + MS_XC, X) : x0;  // a thread past the last column reads nothing
  unsigned n[2] = {0, 0}, sx[2] = {0, 0};             // per thread: at most MS_XC voxels, x sums below 2^18
  int lo[2] = {MEAS_EMPTY, MEAS_EMPTY}, hi[2] = {-MEAS_EMPTY, -MEAS_EMPTY};
  for (int xb = x0; xb < x1; xb += MS_U) {
    float2 l[MS_U];
    float g[MS_U];
#pragma unroll
    for (int u = 0; u < MS_U; ++u) {
      const int64_t v = (int64_t)min(xb + u, x1 - 1) * ncol + c;
      l[u] = *reinterpret_cast<const float2*>(logits + 2 * v);
      g[u] = HAS_LABEL ? label[v] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < MS_U; ++u) {
      const int x = xb + u;
      if (x >= x1) continue;
      const bool in[2] = {vsseg_pred_fg(l[u]), vsseg_label_fg(g[u])};
#pragma unroll
      for (int m = 0; m < NM; ++m)
        if (in[m]) ++n[m], sx[m] += (unsigned)x, lo[m] = min(lo[m], x), hi[m] = max(hi[m], x);
    }
  }
  if (!__syncthreads_or((int)(n[0] | n[1]))) return;  // no foreground in this piece: the usual case
  const int y = c / Z, z = c - y * Z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int m = 0; m < NM; ++m) {
    if (n[m]) {
      atomicMin(&tab[(2 * m) * (int64_t)ncol + c], lo[m]);
      atomicMax(&tab[(2 * m + 1) * (int64_t)ncol + c], hi[m]);
    }
    // per wave: at most 64 * MS_XC voxels with indices below 8192: every sum is at most 2^24
    CountBox<2> box;
    box.clear();
    box.n[0] = n[m];
    if (n[m]) box.grow({y, z}, {y, z});
    box.wave_reduce();
    const unsigned v[3] = {wave_sum_u(sx[m]), wave_sum_u(n[m] * (unsigned)y), wave_sum_u(n[m] * (unsigned)z)};
    if (lane == 0) {
      red[m][wave] = box;
      for (int a = 0; a < 3; ++a) sums[m][wave][a] = v[a];
    }
  }
  __syncthreads();
  if (threadIdx.x < NM) {  // integer atomics: the record does not depend on the order in which workgroups finish
    const int m = threadIdx.x;
    joined(red[m]).merge(&rec->cnt[m], rec->bmin[m], rec->bmax[m]);
    for (int a = 0; a < 3; ++a) {
      const unsigned long long s = ((unsigned long long)sums[m][0][a] + sums[m][1][a]) + ((unsigned long long)sums[m][2][a] + sums[m][3][a]);
      if (s) atomicAdd(&rec->sum[m][a], s);
    }
  }
}

// Workgroup (i = blockIdx.x, k-chunk = blockIdx.y, mask = blockIdx.z).  Thread (ly, lz) owns column (ly, lz) of tile i and meets every column of tile j.
__global__ __launch_bounds__(256) void meas_pair_kernel(MeasRec* __restrict__ rec, const int* __restrict__ tab, int Y, int Z, float sx, float sy, float sz, int ntz, int nt) {
  __shared__ int2 tile[MP_T * MP_T];
  const int m = blockIdx.z;
  const int by0 = rec->bmin[m][0], bz0 = rec->bmin[m][1], by1 = rec->bmax[m][0], bz1 = rec->bmax[m][1];
  if (by1 < 0) return;  // empty mask
  auto in_box = [&](int ty, int tz) { return ty * MP_T <= by1 && ty * MP_T + MP_T - 1 >= by0 && tz * MP_T <= bz1 && tz * MP_T + MP_T - 1 >= bz0; };
  const int i = blockIdx.x, ity = i / ntz, itz = i - ity * ntz;
  if (!in_box(ity, itz)) return;
  const int64_t ncol = (int64_t)Y * Z;
  const int* __restrict__ tmin = tab + (2 * m) * ncol;
  const int* __restrict__ tmax = tab + (2 * m + 1) * ncol;
  const int ly = threadIdx.x / MP_T, lz = threadIdx.x % MP_T;
  const int y = ity * MP_T + ly, z = itz * MP_T + lz;
  int a0 = MEAS_EMPTY, a1 = -MEAS_EMPTY;
  if (y < Y && z < Z) a0 = tmin[(int64_t)y * Z + z], a1 = tmax[(int64_t)y * Z + z];
  if (!__syncthreads_or(a0 <= a1)) return;  // a tile of empty columns inside the box (the box of a tumour and a far island is mostly that)
  float best3 = 0.f, best2 = 0.f;
  for (int kk = 0; kk < MP_KC; ++kk) {
    const int k = blockIdx.y * MP_KC + kk;
    if (k > nt / 2) break;
    int j = i + k;
    if (j >= nt) j -= nt;
    const int jty = j / ntz, jtz = j - jty * ntz;
    if (!in_box(jty, jtz)) continue;  // (uniform over the workgroup)
    __syncthreads();                  // the previous tile has been read
    const int yy = jty * MP_T + ly, zz = jtz * MP_T + lz;
    int2 bj = make_int2(MEAS_EMPTY, -MEAS_EMPTY);
    if (yy < Y && zz < Z) bj = make_int2(tmin[(int64_t)yy * Z + zz], tmax[(int64_t)yy * Z + zz]);
    tile[threadIdx.x] = bj;
    if (!__syncthreads_or(bj.x <= bj.y)) continue;  // (the barrier of the staging as well) tile j holds empty columns only
    float ez[MP_T];  // (sz dz)^2 against the MP_T z positions of tile j
#pragma unroll
    for (int cz = 0; cz < MP_T; ++cz) {
      const float d = sz * (float)(z - (jtz * MP_T + cz));
      ez[cz] = d * d;
    }
    const bool same_z = jtz == itz;
    for (int r = 0; r < MP_T; ++r) {
      const float dy = sy * (float)(y - (jty * MP_T + r));
      const float ey = dy * dy;
#pragma unroll
      for (int cz = 0; cz < MP_T; ++cz) {
        const int2 b = tile[r * MP_T + cz];  // one address per wave: a broadcast
        const int dx = max(a1 - b.x, b.y - a0);  // the largest x extent of the pair of columns; negative when either is empty
        const float fx = sx * (float)dx;
        const float d2 = fmaf(fx, fx, ey + ez[cz]);
        best3 = fmaxf(best3, dx >= 0 ? d2 : 0.f);
      }
      if (same_z) {
        const int2 b = tile[r * MP_T + lz];
        const int dx = max(a1 - b.x, b.y - a0);
        const float fx = sx * (float)dx;
        const float d2 = fmaf(fx, fx, ey);
        best2 = fmaxf(best2, dx >= 0 ? d2 : 0.f);
      }
    }
  }
  const unsigned u3 = (unsigned)wave_max_i((int)__float_as_uint(best3)), u2 = (unsigned)wave_max_i((int)__float_as_uint(best2));  // sign bit clear: int order = float order
  if ((threadIdx.x & 63) == 0) {
    if (u3) atomicMax(&rec->best[m][0], u3);
    if (u2) atomicMax(&rec->best[m][1], u2);
  }
}

__global__ void meas_finalize_kernel(const MeasRec* __restrict__ rec, float sx, float sy, float sz, int has_label, double* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double s[3] = {(double)sx, (double)sy, (double)sz};
  const double voxel = (s[0] * s[1]) * s[2];
  double cen[2][3];
  for (int m = 0; m < 2; ++m) {
    const unsigned long long n = rec->cnt[m];
    const bool on = m == 0 || has_label;
    out[m] = on ? (double)n : nan;
    out[2 + m] = on ? (double)n * voxel : nan;
    out[5 + m] = on && n ? sqrt((double)__uint_as_float(rec->best[m][0])) : nan;
    out[7 + m] = on && n ? sqrt((double)__uint_as_float(rec->best[m][1])) : nan;
    for (int a = 0; a < 3; ++a) cen[m][a] = on && n ? (double)rec->sum[m][a] / (double)n : nan;
  }
  double d2 = 0.0;
  for (int a = 0; a < 3; ++a) {
    const double d = (cen[0][a] - cen[1][a]) * s[a];
    d2 += d * d;
  }
  out[4] = sqrt(d2);  // NaN when either mask is empty or there is no label
}

bool meas_dims_ok(const int32_t* dims) { return dims_ok(dims, MEAS_MAX_EXTENT) && (int64_t)dims[1] * dims[2] <= MEAS_MAX_COLUMNS; }

}  // namespace

extern "C" int64_t vsseg_measure_scratch_bytes(const int32_t dims[3]) {
  VSSEG_CHECK(meas_dims_ok(dims), "vsseg_measure_scratch_bytes: dims must be 1 .. %d on every axis with dims[1] * dims[2] <= %d", MEAS_MAX_EXTENT, MEAS_MAX_COLUMNS);
  return meas_total((int64_t)dims[1] * dims[2]);
}

extern "C" int vsseg_measurements(const float* logits, int32_t pitch, const float* label, const int32_t dims[3], const float spacing[3], void* scratch, int64_t scratch_bytes,
                                  double* out, void* stream) {
  static_assert(MEAS_MAX_COLUMNS == 262144, "the text of the dims message below");
  VOLUME_CHECK_ARGS("vsseg_measurements", logits && scratch && out && spacing, " (only label may be NULL)", pitch, dims, MEAS_MAX_EXTENT, meas_dims_ok(dims),
                    " with dims[1] * dims[2] <= 262144", spacing, aligned_to(logits, 8) && aligned_to(label, 4) && aligned_to(out, 8) && aligned_to(scratch, 256),
                    "logits / out 8 B, label 4 B, scratch 256 B", scratch_bytes, meas_total((int64_t)dims[1] * dims[2]), "vsseg_measure_scratch_bytes");
  const int X = dims[0], Y = dims[1], Z = dims[2], ncol = Y * Z;
  hipStream_t s = as_stream(stream);
  MeasRec* rec = reinterpret_cast<MeasRec*>(scratch);
  int* tab = reinterpret_cast<int*>(static_cast<char*>(scratch) + meas_tables_offset());
  const int cblocks = (ncol + 255) / 256;
  hipLaunchKernelGGL(meas_init_kernel, dim3(cblocks), dim3(256), 0, s, rec, tab, ncol);
  const dim3 sgrid(cblocks, (X + MS_XC - 1) / MS_XC);
  if (label) hipLaunchKernelGGL(meas_stream_kernel<true>, sgrid, dim3(256), 0, s, logits, label, X, Z, ncol, tab, rec);
  else hipLaunchKernelGGL(meas_stream_kernel<false>, sgrid, dim3(256), 0, s, logits, label, X, Z, ncol, tab, rec);
  const int nty = (Y + MP_T - 1) / MP_T, ntz = (Z + MP_T - 1) / MP_T, nt = nty * ntz;  // nt < 2048 in the domain
  hipLaunchKernelGGL(meas_pair_kernel, dim3(nt, (nt / 2 + 1 + MP_KC - 1) / MP_KC, label ? 2 : 1), dim3(256), 0, s, rec, (const int*)tab, Y, Z, spacing[0], spacing[1], spacing[2], ntz, nt);
  hipLaunchKernelGGL(meas_finalize_kernel, dim3(1), dim3(64), 0, s, (const MeasRec*)rec, spacing[0], spacing[1], spacing[2], label ? 1 : 0, out);
  VSSEG_LAUNCH_CHECK("vsseg_measurements");
  return VSSEG_OK;
}
