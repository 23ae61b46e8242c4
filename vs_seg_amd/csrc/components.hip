// Connected components of the foreground of a two-class prediction, the largest of them, and the prediction filtered to it: one volume per call, as a
// sequence of launches on the caller's stream (no host synchronisation, no allocation).  Foreground P = logits[v][1] > logits[v][0] (the rule of vsseg_argmax2:
// ties and NaN are background); connectivity 6 / 18 / 26 = index offsets with every |d_a| <= 1 and |dx| + |dy| + |dz| <= 1 / 2 / 3; outside the volume = background.
//
//   init      zero the record in scratch (foreground count, bounding box of P, number of components, the selection key)
//   local     the only pass that reads the logits: a workgroup owns a tile of CT_X x CT_Y x CT_Z voxels (one wave per z row of 64), keeps the mask as one 64-bit word
//             per row in LDS, labels the tile in LDS with a lock-free union-find (every z run starts out pointing at its first voxel, so only contacts between
//             rows are united, one per pair of touching runs) and writes each voxel's parent as a global linear index (-1: background).  A tile-local root is the
//             smallest index of its tile-local component, so every parent link points to a smaller or equal index from the start.  |P| and the bounding box go
//             into the record with one set of integer atomics per workgroup that saw foreground.  Reads 8 B and writes 4 B per voxel.
//   merge     foreground voxels whose forward neighbour (13 of the 26 offsets, so that each pair is met once) lies in another tile unite with it in global
//             memory: find both roots, atomicMin the larger root's parent to the smaller, continue with the value returned.  Parents only ever decrease, so the
//             final root of a component is its smallest index whatever the order of the unions.
//   flatten   parent[v] = root(v); a root zeroes its own size counter (the only counters that are ever read).
//   sizes     voxels per root: a workgroup sums the component of its smallest root in LDS (one atomic per tile for a compact component), the others per wave.
//   tally     every root offers (size << 32) | (0xFFFFFFFF - label) to one 64-bit atomicMax (largest size, then smallest label) and is counted.
//   write     the whole volume: int32 labels (root + 1), or the one-hot fp32 prediction of the selected component; parents are read inside the box only.
//             Writes 4 B (labels) or 8 B (one-hot) per voxel.  Block 0 also writes the four statistics.
//
// merge .. tally run on grids sized for the volume; workgroups whose tile misses the bounding box (which lives in device memory) exit at once.  No kernel waits for
// another workgroup: every loop either walks parent links towards strictly smaller indices or retries an atomicMin with a strictly smaller operand.  Only integer
// atomics decide anything, so the result is a function of the mask alone.
//
// Two more routes through the same passes, with the same two properties (vsseg_remove_small_components, vsseg_fill_holes):
//   remove small  init, local, merge, flatten, sizes as above; `tally`: the roots, and those with cnt[root] >= min_voxels with their voxels;
//                 `write`: one-hot of cnt[root] >= min_voxels.  min_voxels is a kernel argument.
//   fill holes    init; `scan`: the logits of the whole volume once (8 B per voxel), leaving |P| and the bounding box of P; then local (on the COMPLEMENT of P inside
//                 the box, the logits of the box read again), merge and a flatten that also marks the roots with a voxel on a face of the box, all confined to the
//                 box; `tally`: unmarked roots (holes) and their voxels; `write`: one-hot of P or unmarked, 8 B per voxel.  Why the box suffices: above fh_scan_kernel.
//                 Background comes as whole rows, so this route's local pass labels a tile of 32 equal single-run rows without a union, and its merge pass makes
//                 one union per lane and neighbour tile, not one per row (cc_unite); neither changes a label.
#include "volume.h"

namespace {

constexpr int CT_X = 4, CT_Y = 8, CT_Z = 64;  // tile: CT_X * CT_Y rows of one wave each
constexpr int CT_ROWS = CT_X * CT_Y;          // 32 rows, 8 per wave of the 256-thread workgroup
constexpr int CC_MAX_EXTENT = 8192;

struct CompRec {
  unsigned long long fg;    // |P|
  unsigned long long best;  // max over roots of (size << 32) | (0xFFFFFFFF - label); 0: P is empty
  unsigned ncomp;           // number of roots
  int bmin[3], bmax[3];     // bounding box of P; bmax = -1: empty
  unsigned nkept;           // remove_small: the roots that pass the threshold (best: their voxels); fill_holes: ncomp = holes, best = |H|
};

struct CompLayout {
  int64_t parent, cnt, total;
};
CompLayout cc_layout(int64_t nvox) {
  CompLayout l;
  l.parent = align256(sizeof(CompRec));
  l.cnt = l.parent + align256(nvox * 4);
  l.total = l.cnt + align256(nvox * 4);
  return l;
}
enum CompRoute { CC_LABELS, CC_LARGEST, CC_SMALL, CC_HOLES };  // the four entry points; CC_LABELS and CC_LARGEST differ in what `write` stores only

// the four forward neighbour rows of a row (with dz = -1, 0, 1 each) and the row itself (dz = +1 only): the 13 offsets that follow (0, 0, 0) in raster order
__device__ __forceinline__ int cc_dx(int n) { return n >= 2 ? 1 : 0; }      // n = 0 .. 4: (0, 0), (0, 1), (1, -1), (1, 0), (1, 1)
__device__ __forceinline__ int cc_dy(int n) { return n < 2 ? n : n - 3; }

__device__ __forceinline__ bool cc_bit(unsigned long long m, int i) { return (m >> i) & 1ull; }

// Union-find over an array of parent links with L[i] <= i (a root has L[i] == i).  LDS: workgroup scope; global memory: agent scope, so that a link another
// compute unit has just lowered is seen (a stale link would still be a valid ancestor: links only decrease, and the atomicMin below returns the current one).
template <bool GLOBAL>
__device__ __forceinline__ int cc_find(const int* L, int i) {
  for (;;) {
    const int p = GLOBAL ? __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p == i) return i;
    i = p;  // p < i
  }
}
template <bool GLOBAL>
__device__ __forceinline__ void cc_union(int* L, int a, int b) {
  for (;;) {
    a = cc_find<GLOBAL>(L, a);
    b = cc_find<GLOBAL>(L, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(L + a, b);  // a > b
    if (old == a) return;                 // a was a root and now hangs below b
    a = old;                              // a had a parent old < a already (which now is min(old, b)): unite that one with b
  }
}

// The tile of a workgroup and a thread's place in it: wave w owns the rows r = 4 k + w (x = x0 + r / 8, y = y0 + r % 8), lane l the voxel z = z0 + l of each.
struct CompTile {
  const int x0 = blockIdx.z * CT_X, y0 = blockIdx.y * CT_Y, z0 = blockIdx.x * CT_Z;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, z = z0 + lane;
  __device__ __forceinline__ bool outside_box(const CompRec* rec, int margin = 0) const {  // no voxel within `margin` of the box (an empty box: every tile)
    return rec->bmax[0] + margin < x0 || rec->bmin[0] - margin >= x0 + CT_X || rec->bmax[1] + margin < y0 || rec->bmin[1] - margin >= y0 + CT_Y ||
           rec->bmax[2] + margin < z0 || rec->bmin[2] - margin >= z0 + CT_Z;
  }
  template <typename F>
  __device__ __forceinline__ void rows(int X, int Y, F f) const {  // f(r, x, y) for this wave's rows inside the volume
    for (int k = 0; k < CT_ROWS / 4; ++k) {
      const int r = k * 4 + wave, x = x0 + (r >> 3), y = y0 + (r & 7);
      if (x < X && y < Y) f(r, x, y);  // (the same in every lane of the wave)
    }
  }
};

__global__ __launch_bounds__(256) void cc_init_kernel(CompRec* rec) {
  if (threadIdx.x == 0) {
    rec->fg = 0;
    rec->best = 0;
    rec->ncomp = 0;
    rec->nkept = 0;
  }
  box_reset(rec->bmin, rec->bmax, 3);
}

// HOLES: the mask is the COMPLEMENT of P inside the bounding box of P, which an earlier pass (fh_scan_kernel) has left in the record: background voxels of the box get
// a parent and a zeroed mark in cnt, everything else of the tile -1.  Tiles within one voxel of the box are written too (all -1 when they miss the box itself), so
// that the merge pass, which looks one voxel beyond the voxels it unites, reads nothing that this launch has not written; other tiles exit at once.
template <bool HOLES>
__global__ __launch_bounds__(256) void cc_local_kernel(const float* __restrict__ logits, int X, int Y, int Z, int conn, int* __restrict__ parent, unsigned* __restrict__ cnt,
                                                      CompRec* __restrict__ rec) {
  __shared__ unsigned long long rowmask[CT_ROWS];
  __shared__ int L[CT_ROWS * CT_Z];
  const CompTile t;
  const int x0 = t.x0, y0 = t.y0, z0 = t.z0, wave = t.wave, lane = t.lane, z = t.z;
  int b0x = 0, b0y = 0, b0z = 0, b1x = 0, b1y = 0, b1z = 0;
  if constexpr (HOLES) {
    if (t.outside_box(rec, 1)) return;
    b0x = rec->bmin[0], b0y = rec->bmin[1], b0z = rec->bmin[2], b1x = rec->bmax[0], b1y = rec->bmax[1], b1z = rec->bmax[2];
  }
  float2 lg[CT_ROWS / 4];
  bool in[CT_ROWS / 4];  // HOLES: the voxel lies in the volume and in the box
#pragma unroll
  for (int k = 0; k < CT_ROWS / 4; ++k) {
    const int r = k * 4 + wave, x = x0 + (r >> 3), y = y0 + (r & 7);
    lg[k] = make_float2(0.f, 0.f);
    in[k] = x < X && y < Y && z < Z;
    if constexpr (HOLES) in[k] = in[k] && x >= b0x && x <= b1x && y >= b0y && y <= b1y && z >= b0z && z <= b1z;
    if (in[k]) lg[k] = *reinterpret_cast<const float2*>(logits + 2 * (((int64_t)x * Y + y) * Z + z));
  }
  bool any = false;
#pragma unroll
  for (int k = 0; k < CT_ROWS / 4; ++k) {
    const int r = k * 4 + wave;
    const bool m = HOLES ? in[k] && !vsseg_pred_fg(lg[k]) : vsseg_pred_fg(lg[k]);
    const unsigned long long bits = __ballot(m);
    if (lane == 0) rowmask[r] = bits;
    const unsigned long long gaps = ~bits & ((1ull << lane) - 1ull);  // background voxels below this one: the run starts behind the highest of them
    L[r * CT_Z + lane] = m ? r * CT_Z + (gaps ? 64 - __builtin_clzll(gaps) : 0) : -1;
    any |= bits != 0;
  }
  if (!__syncthreads_or(any)) {  // no foreground in the tile
#pragma unroll
    for (int k = 0; k < CT_ROWS / 4; ++k) {
      const int r = k * 4 + wave, x = x0 + (r >> 3), y = y0 + (r & 7);
      if (x < X && y < Y && z < Z) parent[((int64_t)x * Y + y) * Z + z] = -1;
    }
    return;
  }
  if constexpr (HOLES) {
    // Background is mostly whole rows.  A tile whose 32 rows all hold the same single run is one component at every connectivity (every row touches the next one
    // head-on): its root is the first voxel of row 0, and there is nothing to unite.  (The general path would make all of these unions in lane 0, one after another.)
    const unsigned long long m0 = rowmask[0];
    const bool one_run = m0 != 0 && ((m0 + (m0 & (~m0 + 1ull))) & m0) == 0;
    if (one_run && __all(rowmask[lane & (CT_ROWS - 1)] == m0)) {  // (the same in every wave: the barrier above has published the masks)
      const int root = (int)((((int64_t)x0) * Y + y0) * Z + z0 + __builtin_ctzll(m0));
#pragma unroll
      for (int k = 0; k < CT_ROWS / 4; ++k) {
        const int r = k * 4 + wave, x = x0 + (r >> 3), y = y0 + (r & 7);
        if (x >= X || y >= Y || z >= Z) continue;  // (no row of such a tile lies outside the volume, but its z range may)
        const int64_t v = ((int64_t)x * Y + y) * Z + z;
        const bool m = cc_bit(m0, lane);
        parent[v] = m ? root : -1;
        if (m) cnt[v] = 0;
      }
      return;
    }
  }
  for (int k = 0; k < CT_ROWS / 4; ++k) {
    const int r = k * 4 + wave, lx = r >> 3, ly = r & 7;
    const unsigned long long me = rowmask[r];
    if (!cc_bit(me, lane)) continue;
    const int i = r * CT_Z + lane;
    for (int n = 1; n < 5; ++n) {
      const int dx = cc_dx(n), dy = cc_dy(n), s = dx + (dy < 0 ? -dy : dy);
      if (s > conn || lx + dx >= CT_X || ly + dy < 0 || ly + dy >= CT_Y) continue;
      const int r2 = (lx + dx) * CT_Y + ly + dy;
      const unsigned long long nb = rowmask[r2];
      if (!nb) continue;
      if (cc_bit(nb, lane)) {  // this contact stands for the whole overlap of the two runs: the first voxel of the overlap makes the union
        if (!(lane > 0 && cc_bit(me, lane - 1) && cc_bit(nb, lane - 1))) cc_union<false>(L, i, r2 * CT_Z + lane);
      } else if (s + 1 <= conn) {  // diagonal contacts, unless this run's voxel beside them touches the same run head-on
        if (lane > 0 && cc_bit(nb, lane - 1) && !cc_bit(me, lane - 1)) cc_union<false>(L, i, r2 * CT_Z + lane - 1);
        if (lane < 63 && cc_bit(nb, lane + 1) && !cc_bit(me, lane + 1)) cc_union<false>(L, i, r2 * CT_Z + lane + 1);
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < CT_ROWS / 4; ++k) {
    const int r = k * 4 + wave, x = x0 + (r >> 3), y = y0 + (r & 7);
    if (x >= X || y >= Y || z >= Z) continue;
    int p = -1;
    if (cc_bit(rowmask[r], lane)) {
      const int root = cc_find<false>(L, r * CT_Z + lane);  // local order = raster order inside the tile: the root is the tile-local component's smallest index
      p = (int)((((int64_t)(x0 + (root >> 9))) * Y + (y0 + ((root >> 6) & 7))) * Z + z0 + (root & 63));
    }
    parent[((int64_t)x * Y + y) * Z + z] = p;
    if constexpr (HOLES)
      if (p >= 0) cnt[((int64_t)x * Y + y) * Z + z] = 0;  // the mark of a root that touches a face of the box (cc_flatten_kernel<true>); only a root's is ever read
  }
  if constexpr (HOLES) return;  // |P| and the box are there already
  if (wave == 0) {  // lanes 0 .. 31: one row each
    const unsigned long long bits = lane < CT_ROWS ? rowmask[lane & (CT_ROWS - 1)] : 0ull;
    const int x = x0 + (lane >> 3), y = y0 + (lane & 7);
    CountBox<3> box;
    box.clear();
    box.n[0] = (unsigned)__builtin_popcountll(bits);
    if (bits) box.grow({x, y, z0 + __builtin_ctzll(bits)}, {x, y, z0 + 63 - __builtin_clzll(bits)});
    box.wave_reduce();
    if (lane == 0) box.merge(&rec->fg, rec->bmin, rec->bmax);
  }
}

// MEMO (the fill-holes route, whose mask is mostly whole rows of background): a union is made between the two voxels' current parents - their tile-local roots as `local`
// left them, or a smaller ancestor since - and a lane skips the union whose pair of parents is the pair of its previous one: the rows of a tile that face the same
// neighbour tile then cost one union per lane that makes them, not one per row.  The labels do not change: uniting ancestors unites the voxels.
template <bool MEMO>
__device__ __forceinline__ void cc_unite(int* parent, int va, int vb, int& last_a, int& last_b) {
  if constexpr (MEMO) {
    const int a = __hip_atomic_load(parent + va, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), b = __hip_atomic_load(parent + vb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // both >= 0: mask voxels
    if (a == last_a && b == last_b) return;
    last_a = a, last_b = b;
    cc_union<true>(parent, a, b);
  } else {
    cc_union<true>(parent, va, vb);
  }
}

template <bool MEMO>
__global__ __launch_bounds__(256) void cc_merge_kernel(const CompRec* __restrict__ rec, int X, int Y, int Z, int conn, int* parent) {
  const CompTile t;
  if (t.outside_box(rec)) return;
  const int lane = t.lane, z = t.z;
  int last_a = -1, last_b = -1;  // MEMO: the pair of this lane's previous union
  t.rows(X, Y, [&](int r, int x, int y) {
    const int lx = r >> 3, ly = r & 7;
    const int64_t row = ((int64_t)x * Y + y) * Z;
    const bool mine = z < Z && parent[row + z] >= 0;  // (whether a voxel is foreground never changes)
    const unsigned long long me = __ballot(mine);
    if (!me) return;
    const int v = (int)(row + z);
    // the foreground of the five rows at z - 1, z, z + 1 first (no divergent work between the ballots): bits of the 64 voxels of this tile's z range, and the
    // two voxels just outside it, which lanes 0 and 63 read
    unsigned long long nb[5];
    bool qm[5], qp[5];
#pragma unroll
    for (int n = 0; n < 5; ++n) {
      const int dx = cc_dx(n), dy = cc_dy(n), s = dx + (dy < 0 ? -dy : dy);
      const int xn = x + dx, yn = y + dy;
      nb[n] = 0, qm[n] = qp[n] = false;
      if (s > conn || xn >= X || yn < 0 || yn >= Y) continue;  // (the same in every lane)
      const int64_t row2 = ((int64_t)xn * Y + yn) * Z;
      nb[n] = __ballot(z < Z && parent[row2 + z] >= 0);
      qm[n] = lane == 0 ? (z >= 1 && parent[row2 + z - 1] >= 0) : cc_bit(nb[n], lane - 1);
      qp[n] = lane == 63 ? (z + 1 < Z && parent[row2 + z + 1] >= 0) : cc_bit(nb[n], lane + 1);
    }
    if (!mine) return;
    const bool me_m = lane > 0 && cc_bit(me, lane - 1), me_p = lane < 63 && cc_bit(me, lane + 1);  // this run's voxels beside this one, in this tile
#pragma unroll
    for (int n = 0; n < 5; ++n) {
      const int dx = cc_dx(n), dy = cc_dy(n), s = dx + (dy < 0 ? -dy : dy);
      const int xn = x + dx, yn = y + dy;
      if (s > conn || xn >= X || yn < 0 || yn >= Y) continue;
      const bool other_xy = lx + dx >= CT_X || ly + dy < 0 || ly + dy >= CT_Y;  // the neighbour row belongs to another tile
      const int64_t row2 = ((int64_t)xn * Y + yn) * Z;
      const bool q0 = cc_bit(nb[n], lane);
      // head-on: the first voxel of the overlap of the two runs makes the union for all of it
      if (s > 0 && other_xy && q0 && !(me_m && cc_bit(nb[n], lane - 1))) cc_unite<MEMO>(parent, v, (int)(row2 + z), last_a, last_b);
      // a diagonal neighbour counts when it lies in another tile; inside the z range of this tile it is already joined through a head-on contact if there is one
      if (s > 0 && s + 1 <= conn && qm[n] && (lane == 0 || (other_xy && !q0 && !me_m))) cc_unite<MEMO>(parent, v, (int)(row2 + z - 1), last_a, last_b);
      if ((s == 0 || s + 1 <= conn) && qp[n] && (lane == 63 || (other_xy && !q0 && !me_p))) cc_unite<MEMO>(parent, v, (int)(row2 + z + 1), last_a, last_b);
    }
  });
}

// parent[v] = root(v).  A root zeroes its own size counter; HOLES: a background voxel on a face of the box marks its root instead (cnt[root] = 1; this route's
// local pass zeroed every mark, and every marker stores the same value).
template <bool HOLES>
__global__ __launch_bounds__(256) void cc_flatten_kernel(const CompRec* __restrict__ rec, int X, int Y, int Z, int* parent, unsigned* __restrict__ cnt) {
  const CompTile t;
  if (t.outside_box(rec) || t.z >= Z) return;
  const int z = t.z;
  const int b0x = rec->bmin[0], b0y = rec->bmin[1], b0z = rec->bmin[2], b1x = rec->bmax[0], b1y = rec->bmax[1], b1z = rec->bmax[2];
  t.rows(X, Y, [&](int, int x, int y) {
    const int v = (int)(((int64_t)x * Y + y) * Z + z);
    if (parent[v] < 0) return;                  // (HOLES: a voxel with a parent lies in the box)
    const int root = cc_find<true>(parent, v);  // (a link another thread has flattened meanwhile is as good as the old one)
    parent[v] = root;
    if (HOLES ? x == b0x || x == b1x || y == b0y || y == b1y || z == b0z || z == b1z : root == v) cnt[root] = HOLES;
  });
}

__global__ __launch_bounds__(256) void cc_sizes_kernel(const CompRec* __restrict__ rec, int X, int Y, int Z, const int* __restrict__ parent, unsigned* cnt) {
  __shared__ int s_root;
  __shared__ unsigned s_cnt;
  const CompTile t;
  if (t.outside_box(rec)) return;
  const int x0 = t.x0, y0 = t.y0, wave = t.wave, lane = t.lane, z = t.z;
  if (threadIdx.x == 0) s_root = INT_MAX, s_cnt = 0;
  __syncthreads();
  int p[CT_ROWS / 4], lo = INT_MAX;
#pragma unroll
  for (int k = 0; k < CT_ROWS / 4; ++k) {
    const int r = k * 4 + wave, x = x0 + (r >> 3), y = y0 + (r & 7);
    p[k] = (x < X && y < Y && z < Z) ? parent[((int64_t)x * Y + y) * Z + z] : -1;
    if (p[k] >= 0) lo = min(lo, p[k]);
  }
  lo = wave_min_i(lo);
  if (lane == 0 && lo != INT_MAX) atomicMin(&s_root, lo);
  __syncthreads();
  const int first = s_root;  // the smallest root seen in this tile: summed in LDS; INT_MAX: no foreground here
  if (first == INT_MAX) return;
  unsigned mine = 0;
#pragma unroll
  for (int k = 0; k < CT_ROWS / 4; ++k) {
    mine += (unsigned)__builtin_popcountll(__ballot(p[k] == first));
    bool act = p[k] >= 0 && p[k] != first;
    unsigned long long m = __ballot(act);
    while (m) {  // the other roots of this row: one atomic per root and wave
      const int leader = __builtin_ctzll(m);
      const int root = __shfl(p[k], leader, 64);
      const unsigned long long same = __ballot(act && p[k] == root);
      if (lane == leader) atomicAdd(cnt + root, (unsigned)__builtin_popcountll(same));
      if (p[k] == root) act = false;
      m &= ~same;
    }
  }
  if (lane == 0 && mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(cnt + first, s_cnt);
}

// One walk over the roots of the tiles in the box, one set of integer atomics per wave that met any (integer sums and maxima: the order does not matter):
//   CC_LABELS, CC_LARGEST  every root is counted and offers its key to `best`
//   CC_SMALL               every root is counted; those with cnt[root] >= min_voxels are counted in nkept, their voxels in `best`
//   CC_HOLES               the roots without a mark are the holes (ncomp), the voxels below them |H| (best)
template <CompRoute R>
__global__ __launch_bounds__(256) void cc_tally_kernel(CompRec* __restrict__ rec, int X, int Y, int Z, const int* __restrict__ parent, const unsigned* __restrict__ cnt,
                                                      unsigned long long min_voxels) {
  constexpr bool PICK = R == CC_LABELS || R == CC_LARGEST;
  const CompTile t;
  if (t.outside_box(rec)) return;
  const int z = t.z;
  unsigned long long acc = 0;  // PICK: the largest key; otherwise the voxels kept / filled
  unsigned roots = 0, kept = 0;
  t.rows(X, Y, [&](int, int x, int y) {
    if (z >= Z) return;
    const int v = (int)(((int64_t)x * Y + y) * Z + z);
    const int p = parent[v];
    if constexpr (R == CC_HOLES) {
      if (p < 0 || cnt[p]) return;
      ++acc;
      roots += p == v;
    } else {
      if (p != v) return;
      const unsigned c = cnt[v];
      ++roots;
      const unsigned long long key = ((unsigned long long)c << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(v + 1));
      if (PICK) acc = key > acc ? key : acc;
      else if ((unsigned long long)c >= min_voxels) ++kept, acc += c;
    }
  });
  acc = PICK ? wave_max_u64(acc) : wave_sum_u64(acc);
  roots = wave_sum_u(roots);
  if (R == CC_SMALL) kept = wave_sum_u(kept);
  if (t.lane != 0) return;
  if (roots) atomicAdd(&rec->ncomp, roots);
  if (PICK && roots) atomicMax(&rec->best, acc);
  if (!PICK && acc) atomicAdd(&rec->best, acc);
  if (kept) atomicAdd(&rec->nkept, kept);
}

// The result over the whole volume; parents (and the counter of a voxel's root) are read inside the box only.  CC_LABELS: out = int32 labels [X][Y][Z]; the other
// routes: out = fp32 one-hot [X][Y][Z][2], 1 on the selected component / on the components of P with at least min_voxels voxels / on P (in the box: no parent) and on
// the background components without a mark.  Block 0 also writes the four statistics of the route.
template <CompRoute R>
__global__ __launch_bounds__(256) void cc_write_kernel(const CompRec* __restrict__ rec, int Y, int Z, int64_t nvox, const int* __restrict__ parent, const unsigned* __restrict__ cnt,
                                                      unsigned long long min_voxels, void* __restrict__ out, long long* __restrict__ stats) {
  constexpr bool PICK = R == CC_LABELS || R == CC_LARGEST;
  const unsigned long long best = rec->best;
  const int keep = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)) - 1 : -2;  // PICK: root of the selected component
  if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = (long long)rec->fg;
    stats[1] = (long long)rec->ncomp;
    stats[2] = PICK ? (long long)(best >> 32) : (long long)best;
    stats[3] = PICK ? (best ? (long long)keep + 1 : 0) : R == CC_HOLES ? (long long)(rec->fg + best) : (long long)rec->nkept;
  }
  const int b0x = rec->bmin[0], b0y = rec->bmin[1], b0z = rec->bmin[2], b1x = rec->bmax[0], b1y = rec->bmax[1], b1z = rec->bmax[2];
  for (unsigned v = blockIdx.x * 256u + threadIdx.x; v < (unsigned)nvox; v += gridDim.x * 256u) {  // (nvox < 2^31 and the stride < 2^24: no wrap)
    const unsigned xy = v / (unsigned)Z, x = xy / (unsigned)Y;
    const int z = (int)(v - xy * (unsigned)Z), y = (int)(xy - x * (unsigned)Y);
    const bool in_box = (int)x >= b0x && (int)x <= b1x && y >= b0y && y <= b1y && z >= b0z && z <= b1z;
    const int p = in_box ? parent[v] : -1;
    if constexpr (R == CC_LABELS) {
      static_cast<int*>(out)[v] = p + 1;
    } else {
      bool on;
      if (R == CC_LARGEST) on = p == keep;
      else if (R == CC_SMALL) on = p >= 0 && (unsigned long long)cnt[p] >= min_voxels;
      else on = in_box && (p < 0 || cnt[p] == 0);
      const float f = on ? 1.f : 0.f;
      static_cast<float2*>(out)[v] = make_float2(1.f - f, f);
    }
  }
}

// ---- fill holes: |P| and its box first, then the labelling above on the complement of P inside the box ----
// A hole is a connected component of the complement of P without a voxel on the border of the volume.  Every hole lies inside the box of P (a background voxel
// outside the box reaches the border along a straight line that never enters the box), and a path that leaves the box passes a voxel on one of its faces (a step
// changes every index by at most 1).  So a background component OF THE BOX without a voxel on a face of the box is a component of the whole complement, and it holds
// no border voxel (a border voxel inside the box lies on a face of the box): a hole.  One with a background voxel on a face is not: that face lies on the border of
// the volume, or the voxel's straight neighbour beyond the face starts such a line, and a straight step is allowed at every connectivity.

__global__ __launch_bounds__(256) void fh_scan_kernel(const float* __restrict__ logits, int Y, int Z, int64_t nvox, CompRec* __restrict__ rec) {
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

template <CompRoute R>
int cc_run(const char* name, const float* logits, int32_t pitch, const int32_t* dims, int32_t connectivity, int64_t min_voxels, void* scratch, int64_t scratch_bytes, void* out,
           int64_t* stats, void* stream) {
  constexpr bool labels = R == CC_LABELS, holes = R == CC_HOLES;
  VOLUME_CHECK_ARGS(name, logits && scratch && out && (stats || !labels), labels ? " (logits, scratch, labels, stats)" : " (logits, scratch, out)", pitch, dims, CC_MAX_EXTENT, true,
                    "", (const float*)nullptr, aligned_to(logits, 8) && aligned_to(out, labels ? 4 : 8) && aligned_to(stats, 8) && aligned_to(scratch, 256),
                    labels ? "logits / stats 8 B, labels 4 B, scratch 256 B" : "logits / stats 8 B, out 8 B, scratch 256 B", scratch_bytes,
                    cc_layout((int64_t)dims[0] * dims[1] * dims[2]).total, "vsseg_components_scratch_bytes");
  const int64_t nvox = (int64_t)dims[0] * dims[1] * dims[2];
  VSSEG_CHECK(nvox < (int64_t)INT32_MAX, "%s: dims %d x %d x %d hold %lld voxels, the int32 labels allow fewer than 2^31 - 1", name, dims[0], dims[1], dims[2], (long long)nvox);
  VSSEG_CHECK(connectivity == 6 || connectivity == 18 || connectivity == 26, "%s: connectivity must be 6, 18 or 26, got %d", name, connectivity);
  VSSEG_CHECK(min_voxels >= 0, "%s: min_voxels must not be negative, got %lld", name, (long long)min_voxels);
  const CompLayout l = cc_layout(nvox);
  const int X = dims[0], Y = dims[1], Z = dims[2];
  const int conn = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;  // largest |dx| + |dy| + |dz| of a neighbour
  hipStream_t s = as_stream(stream);
  char* base = static_cast<char*>(scratch);
  CompRec* rec = reinterpret_cast<CompRec*>(base);
  int* parent = reinterpret_cast<int*>(base + l.parent);
  unsigned* cnt = reinterpret_cast<unsigned*>(base + l.cnt);
  const unsigned long long minv = (unsigned long long)min_voxels;
  const dim3 tiles((Z + CT_Z - 1) / CT_Z, (Y + CT_Y - 1) / CT_Y, (X + CT_X - 1) / CT_X);
  const int wg = grid_for(nvox, 256, 256 * 32);
  hipLaunchKernelGGL(cc_init_kernel, dim3(1), dim3(64), 0, s, rec);
  if (holes) hipLaunchKernelGGL(fh_scan_kernel, dim3(wg), dim3(256), 0, s, logits, Y, Z, nvox, rec);
  hipLaunchKernelGGL(cc_local_kernel<holes>, tiles, dim3(256), 0, s, logits, X, Y, Z, conn, parent, cnt, rec);
  hipLaunchKernelGGL(cc_merge_kernel<holes>, tiles, dim3(256), 0, s, (const CompRec*)rec, X, Y, Z, conn, parent);
  hipLaunchKernelGGL(cc_flatten_kernel<holes>, tiles, dim3(256), 0, s, (const CompRec*)rec, X, Y, Z, parent, cnt);
  if (!holes) hipLaunchKernelGGL(cc_sizes_kernel, tiles, dim3(256), 0, s, (const CompRec*)rec, X, Y, Z, (const int*)parent, cnt);
  hipLaunchKernelGGL(cc_tally_kernel<R>, tiles, dim3(256), 0, s, rec, X, Y, Z, (const int*)parent, (const unsigned*)cnt, minv);
  hipLaunchKernelGGL(cc_write_kernel<R>, dim3(wg), dim3(256), 0, s, (const CompRec*)rec, Y, Z, nvox, (const int*)parent, (const unsigned*)cnt, minv, out,
                     reinterpret_cast<long long*>(stats));
  VSSEG_LAUNCH_CHECK(name);
  return VSSEG_OK;
}

}  // namespace

extern "C" int64_t vsseg_components_scratch_bytes(const int32_t dims[3]) {
  VSSEG_CHECK(dims_ok(dims, CC_MAX_EXTENT), "vsseg_components_scratch_bytes: dims must be 1 .. %d on every axis", CC_MAX_EXTENT);
  const int64_t nvox = (int64_t)dims[0] * dims[1] * dims[2];
  VSSEG_CHECK(nvox < (int64_t)INT32_MAX, "vsseg_components_scratch_bytes: dims %d x %d x %d hold %lld voxels, the int32 labels allow fewer than 2^31 - 1", dims[0], dims[1], dims[2],
              (long long)nvox);
  return cc_layout(nvox).total;
}

extern "C" int vsseg_components_label(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, void* scratch, int64_t scratch_bytes, int32_t* labels,
                                      int64_t* stats, void* stream) {
  return cc_run<CC_LABELS>("vsseg_components_label", logits, pitch, dims, connectivity, 0, scratch, scratch_bytes, labels, stats, stream);
}

extern "C" int vsseg_keep_largest_component(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, void* scratch, int64_t scratch_bytes, float* out,
                                            int64_t* stats, void* stream) {
  return cc_run<CC_LARGEST>("vsseg_keep_largest_component", logits, pitch, dims, connectivity, 0, scratch, scratch_bytes, out, stats, stream);
}

extern "C" int vsseg_fill_holes(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, void* scratch, int64_t scratch_bytes, float* out, int64_t* stats,
                                void* stream) {
  return cc_run<CC_HOLES>("vsseg_fill_holes", logits, pitch, dims, connectivity, 0, scratch, scratch_bytes, out, stats, stream);
}

extern "C" int vsseg_remove_small_components(const float* logits, int32_t pitch, const int32_t dims[3], int32_t connectivity, int64_t min_voxels, void* scratch, int64_t scratch_bytes,
                                             float* out, int64_t* stats, void* stream) {
  return cc_run<CC_SMALL>("vsseg_remove_small_components", logits, pitch, dims, connectivity, min_voxels, scratch, scratch_bytes, out, stats, stream);
}
