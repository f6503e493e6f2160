// Connected-component labelling, component statistics and the component filter (label_kernels.h): plain C++ and HIP
// builtins, integer arithmetic only.
//
// Labelling is label equivalence (union-find) on the label map itself.  While it runs, labels[i] of an ON pixel holds
// 1 + the frame-local raster index of its parent, and a parent's index is never larger than the pixel's own: a root
// points at itself, and the root of a finished set is the component's first pixel in raster order.  Six launches,
// one after the other on the stream; what one needs from another workgroup it gets from an earlier LAUNCH:
//   1 tile_kernel     one workgroup per 32 x 128 tile.  The mask rows of the tile are read with 16-byte loads at
//                     16-byte aligned ADDRESSES and single bytes at the ragged ends (the base pointer may be odd), the
//                     pixels are labelled in LDS run-wise along rows (a pixel starts out pointing at the start of its
//                     run), runs are linked to the row above (only where no neighbouring pixel's link already says
//                     so), every pixel is flattened to its tile root and written out with the root's frame index.
//   2 border_kernel   one thread per pixel of a tile's first row (but the frame's) and first column: links across the
//                     tile borders, the larger root to the smaller one by an atomic minimum.
//   3 flatten_kernel  one workgroup per row: every pixel walks to its root and stores it; the row's roots and ON
//                     pixels are counted into the workspace.  The grid also clears all records.
//   4 scan_kernel     one workgroup per frame: exclusive scan of the rows' root counts, and the header.
//   5 rank_kernel     one workgroup per row: a root's id is 1 + the roots of earlier rows + the roots to its left, which
//                     is raster order of first pixels.  The root's cell becomes -id, record word [12] its index, and
//                     the record's two minimum words all-ones.
//   6 stats_kernel    one workgroup per four rows: a pixel's id is |labels[root]|; it overwrites its own cell with it.  Runs
//                     of ON pixels inside a thread's stretch of the row are summed in registers; runs of one
//                     component that end at the same step in a wave are summed through shuffles (a long marking, a
//                     full row, the giant component of a dense mask), the first such component a wave meets stays in
//                     its registers for the row and, while it is the same one, for the four rows, and one lane issues
//                     the atomics; the rest each lane adds itself.
//                     All are integer adds, minima, maxima and ORs: the records do not depend on the order.
//
// Termination.  A find walks strictly decreasing indices (it stops at the first cell that does not point below
// itself), so it ends after at most `index` steps whatever the memory holds.  A link is an atomic minimum on a root's
// cell: cells only ever decrease.  A union that loses its race continues with the value the cell held, which is
// smaller than the root it tried, so the sum of its two indices decreases on every turn.  No workgroup waits for
// another: no spin, no grid-wide barrier, no cooperative launch; the loops over tiles, rows and frames are grid-stride
// loops with uniform bounds.
//
// The eight XCDs.  Only border_kernel, flatten_kernel and stats_kernel touch cells other workgroups write in the same
// launch.  Every such access is an agent-scope atomic (__hip_atomic_load / _store / _fetch_min with
// __HIP_MEMORY_SCOPE_AGENT).  The loads skip the CU's L1 but may be served by the XCD's own L2, so a load may see an
// OLD value of a cell another XCD has since lowered; nothing here needs it to be fresh.  A find that reads an older
// value reads an older ancestor of the same set, which is still a valid step (cells only decrease within their
// set), and ends at some member of the set.  The link itself is a read-modify-write atomic on the one copy all XCDs
// share, and what is acted on is the value it RETURNS: if the cell was not the root any more, the union goes on from
// the value found there.  So a stale find costs a turn of the loop, never a lost or a wrong link.  In stats_kernel
// a root's cell holds -id until its owner overwrites it with +id; a reader takes the absolute value, so either is
// right.  Everything else is read after the launch that wrote it has ended.
//
// Bounds.  Mask reads stay inside the tile's rows of the frame (a 16-byte load is issued only where all its bytes lie
// in the span [x0, x1) of the row).  Cell indices are 0 .. height * width - 1 of the pixel's own frame: a parent index
// comes from a cell as value - 1 and is followed only if 0 <= parent < index.  Record writes are guarded by id <= cap,
// keep-table reads by 0 < id <= cap, workspace indices are rows of the frame.  The mask writer stores 16 bytes only
// where all of them lie inside the output.
//
// Largest sum: S_4 of a full 2048 x 2048 frame, 2048 sum_{y < 2048} y^4 = 14 739 386 724 520 034 304 < 2^64;
// T_2 <= sum_x x * sum_y y^2 < 2^21 * 2^33 = 2^54.
#include "label_kernels.h"

#include "op_entry.h"
#include "wave_ops.h"

#include <algorithm>


namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int TH = 32, TW = 128, THREADS = 256, SEG = 16, SEGS = TW / SEG;   // THREADS = TH * SEGS
constexpr int ON_STRIDE = TW + 4;                                            // a zero column on either side
constexpr int SCAN_THREADS = 1024, KEEP_THREADS = 1024, KEEP_OWN = 4;
constexpr unsigned GRID_MAX = 1u << 18;

static_assert(TH * SEGS == THREADS, "one thread per 16-pixel segment of a tile row");
static_assert(2 * SCAN_THREADS >= LABEL_SIDE_MAX, "scan_kernel takes two rows per thread");

struct LabelArgs {
  const uint8_t* masks;
  int32_t* labels;
  u64* header;
  u64* records;
  uint32_t* work;   // per frame: [0, h) the rows' root counts, then their exclusive scan; [h, 2h) the rows' ON counts
  int n, height, width, level, conn8, cap;
};

__device__ __forceinline__ int ld_agent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int32_t* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- union-find in LDS: L[i] is the parent's tile index, L[i] <= i
__device__ __forceinline__ int lds_find(const int* L, int i) {
  for (;;) {
    const int p = __hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (p >= i || p < 0) return i;
    i = p;
  }
}
__device__ __forceinline__ void lds_union(int* L, int a, int b) {
  for (;;) {
    a = lds_find(L, a), b = lds_find(L, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = atomicMin(L + a, b);   // a > b: the larger root under the smaller one
    if (old >= a || old < 0) return;       // a was a root: linked
    a = old;                               // someone lowered it first: old < a, go on from there
  }
}

// ---- union-find on the frame's cells: P[i] is 1 + the parent's index, 0 for an OFF pixel
__device__ __forceinline__ int g_find(const int32_t* P, int i) {
  for (;;) {
    const int p = ld_agent(P + i) - 1;
    if (p >= i || p < 0) return i;
    i = p;
  }
}
__device__ __forceinline__ void g_union(int32_t* P, int a, int b) {
  for (;;) {
    a = g_find(P, a), b = g_find(P, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b, b = t; }
    const int old = __hip_atomic_fetch_min(P + a, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
    if (old >= a || old < 0) return;
    a = old;
  }
}

// ---- 1. the tiles
__global__ __launch_bounds__(THREADS) void tile_kernel(const LabelArgs a) {
  __shared__ int L[TH * TW];
  __shared__ uint8_t onb[(TH + 1) * ON_STRIDE];   // on(r, lx) for -1 <= r < TH, -1 <= lx <= TW; zero outside the tile
  const int tid = threadIdx.x;
  const int h = a.height, w = a.width;
  const int tilesX = (w + TW - 1) / TW, tilesY = (h + TH - 1) / TH;
  const long long tiles = (long long)a.n * tilesY * tilesX;
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int tx = (int)(t % tilesX), ty = (int)((t / tilesX) % tilesY);
    const long long img = t / ((long long)tilesX * tilesY);
    const int x0 = tx * TW, y0 = ty * TH, tw = min(TW, w - x0), th = min(TH, h - y0);
    const uint8_t* __restrict__ frame = a.masks + (size_t)img * h * w;
    int32_t* __restrict__ out = a.labels + (size_t)img * h * w;
    __syncthreads();   // the last tile's LDS is no longer read
    for (int i = tid; i < (TH + 1) * ON_STRIDE; i += THREADS) onb[i] = 0;
    __syncthreads();
    {
      const int g = tid >> 4, sub = tid & 15;   // 16 lanes a row: at most 9 chunks cover 128 bytes at any alignment
      for (int r = g; r < th; r += THREADS / 16) {
        const uint8_t* __restrict__ row = frame + (size_t)(y0 + r) * w;
        const int x1 = x0 + tw;
        const int mis = (int)(reinterpret_cast<uintptr_t>(row + x0) & 15u);
        const int nch = (mis + tw + 15) >> 4;
        uint8_t* __restrict__ dst = onb + (r + 1) * ON_STRIDE + 1;   // dst[x - x0]
        if (sub < nch) {
          const int xb = x0 - mis + 16 * sub;   // x of the chunk's first byte; may lie in front of x0
          if (xb >= x0 && xb + 16 <= x1) {
            const uint4 v = *reinterpret_cast<const uint4*>(row + xb);
            const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int b = 0; b < 16; ++b) dst[xb - x0 + b] = (int)((wd[b >> 2] >> (8 * (b & 3))) & 255u) > a.level ? 1 : 0;
          } else {
            for (int b = 0; b < 16; ++b) {
              const int x = xb + b;
              if (x >= x0 && x < x1) dst[x - x0] = (int)row[x] > a.level ? 1 : 0;
            }
          }
        }
      }
    }
    __syncthreads();
    const int r = tid / SEGS, lx0 = (tid % SEGS) * SEG;
    const uint8_t* __restrict__ cur = onb + (r + 1) * ON_STRIDE + 1;   // cur[lx], lx = -1 .. TW
    const uint8_t* __restrict__ up = cur - ON_STRIDE;
    {
      int start = lx0;   // a pixel points at the start of its run inside this segment
      for (int j = 0; j < SEG; ++j) {
        const int lx = lx0 + j;
        if (!cur[lx]) start = lx + 1;
        L[r * TW + lx] = cur[lx] ? r * TW + start : r * TW + lx;
      }
    }
    __syncthreads();
    if (lx0 > 0 && cur[lx0] && cur[lx0 - 1]) lds_union(L, r * TW + lx0, r * TW + lx0 - 1);   // a run across two segments
    if (r > 0) {
      for (int j = 0; j < SEG; ++j) {
        const int lx = lx0 + j;
        if (!cur[lx]) continue;
        const int p = r * TW + lx;
        if (up[lx]) {
          // W and NW both on: the pixel to the left links the same two runs
          if (!(cur[lx - 1] && up[lx - 1])) lds_union(L, p, p - TW);
        } else if (a.conn8) {
          if (up[lx - 1] && !cur[lx - 1]) lds_union(L, p, p - TW - 1);   // W on: its own link upwards covers this
          if (up[lx + 1] && !cur[lx + 1]) lds_union(L, p, p - TW + 1);   // E on: likewise
        }
      }
    }
    __syncthreads();
    if (r < th) {
      for (int j = 0; j < SEG; ++j) {
        const int lx = lx0 + j;
        if (lx >= tw) break;
        int v = 0;
        if (cur[lx]) {
          const int root = lds_find(L, r * TW + lx);
          v = (y0 + root / TW) * w + x0 + root % TW + 1;
        }
        out[(size_t)(y0 + r) * w + x0 + lx] = v;
      }
    }
  }
}

// ---- 2. links across tile borders
__global__ __launch_bounds__(THREADS) void border_kernel(const LabelArgs a, int nbh, int nbv) {
  const int h = a.height, w = a.width;
  const long long perFrame = (long long)nbh * w + (long long)nbv * h;
  const long long total = perFrame * a.n;
  for (long long i = (long long)blockIdx.x * THREADS + threadIdx.x; i < total; i += (long long)gridDim.x * THREADS) {
    const long long img = i / perFrame;
    int e = (int)(i % perFrame);
    int32_t* P = a.labels + (size_t)img * h * w;
    if (e < nbh * w) {   // the first row of a tile row: up, and up-left / up-right
      const int y = (e / w + 1) * TH, x = e % w, p = y * w + x;
      if (ld_agent(P + p) == 0) continue;
      if (ld_agent(P + p - w) != 0) {
        g_union(P, p, p - w);
      } else if (a.conn8) {
        if (x > 0 && ld_agent(P + p - w - 1) != 0) g_union(P, p, p - w - 1);
        if (x < w - 1 && ld_agent(P + p - w + 1) != 0) g_union(P, p, p - w + 1);
      }
    } else {             // the first column of a tile column: left, and up-left / down-left
      e -= nbh * w;
      const int x = (e / h + 1) * TW, y = e % h, p = y * w + x;
      if (ld_agent(P + p) == 0) continue;
      if (ld_agent(P + p - 1) != 0) {
        g_union(P, p, p - 1);
      } else if (a.conn8) {
        if (y > 0 && ld_agent(P + p - w - 1) != 0) g_union(P, p, p - w - 1);
        if (y < h - 1 && ld_agent(P + p + w - 1) != 0) g_union(P, p, p + w - 1);
      }
    }
  }
}

// ---- 3. every pixel to its root; roots and ON pixels per row
__global__ __launch_bounds__(THREADS) void flatten_kernel(const LabelArgs a) {
  __shared__ uint32_t red[THREADS / 64][2];
  const int tid = threadIdx.x, h = a.height, w = a.width;
  const long long rows = (long long)a.n * h;
  for (long long rr = blockIdx.x; rr < rows; rr += gridDim.x) {
    const long long img = rr / h;
    const int y = (int)(rr % h);
    int32_t* P = a.labels + (size_t)img * h * w;
    uint32_t roots = 0u, on = 0u;
    for (int x = tid; x < w; x += THREADS) {
      const int i = y * w + x;
      if (ld_agent(P + i) == 0) continue;
      const int root = g_find(P, i);
      st_agent(P + i, root + 1);
      on += 1u, roots += root == i ? 1u : 0u;
    }
    roots = wave_sum32(roots), on = wave_sum32(on);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6][0] = roots, red[tid >> 6][1] = on;
    __syncthreads();
    if (tid == 0) {
      uint32_t* wk = a.work + (size_t)img * 2 * h;
      wk[y] = red[0][0] + red[1][0] + red[2][0] + red[3][0];
      wk[h + y] = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    }
  }
  // the records start out as zeros: all of them, over the whole grid (rank_kernel sets the minima of those in use)
  const size_t words = (size_t)a.n * a.cap * LABEL_WORDS;
  for (size_t i = (size_t)blockIdx.x * THREADS + tid; i < words; i += (size_t)gridDim.x * THREADS) a.records[i] = 0ull;
}

// ---- 4. the scan over rows, the header, the records' initial state
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(const LabelArgs a) {
  __shared__ uint32_t wtot[SCAN_THREADS / 64];
  __shared__ u64 won[SCAN_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = a.height;
  for (long long img = blockIdx.x; img < a.n; img += gridDim.x) {
    uint32_t* wk = a.work + (size_t)img * 2 * h;
    const int r0 = 2 * tid, r1 = r0 + 1;
    const uint32_t c0 = r0 < h ? wk[r0] : 0u, c1 = r1 < h ? wk[r1] : 0u;
    const uint32_t o = (r0 < h ? wk[h + r0] : 0u) + (r1 < h ? wk[h + r1] : 0u);
    uint32_t incl = c0 + c1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += t;
    }
    const u64 osum = wave_sum((u64)o);
    __syncthreads();   // the last frame's totals are no longer read
    if (lane == 63) wtot[wave] = incl;
    if (lane == 0) won[wave] = osum;
    __syncthreads();
    uint32_t before = 0u, K = 0u;
    u64 onTotal = 0ull;
#pragma unroll
    for (int j = 0; j < SCAN_THREADS / 64; ++j) {
      before += j < wave ? wtot[j] : 0u;
      K += wtot[j], onTotal += won[j];
    }
    const uint32_t excl = before + incl - (c0 + c1);
    if (r0 < h) wk[r0] = excl;
    if (r1 < h) wk[r1] = excl + c0;
    const uint32_t nrec = min(K, (uint32_t)a.cap);
    if (tid < 4) a.header[(size_t)img * 4 + tid] = tid == 0 ? (u64)K : tid == 1 ? onTotal : tid == 2 ? (u64)nrec : 0ull;
  }
}

// ---- 5. a root's id: raster order of first pixels
__global__ __launch_bounds__(THREADS) void rank_kernel(const LabelArgs a) {
  __shared__ uint32_t wtot[THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = a.height, w = a.width;
  const int per = (w + THREADS - 1) / THREADS;   // <= 8 consecutive pixels a thread
  const long long rows = (long long)a.n * h;
  for (long long rr = blockIdx.x; rr < rows; rr += gridDim.x) {
    const long long img = rr / h;
    const int y = (int)(rr % h);
    int32_t* P = a.labels + (size_t)img * h * w;
    const uint32_t base = a.work[(size_t)img * 2 * h + y];
    const int xa = min(tid * per, w), xe = min(xa + per, w);
    uint32_t cnt = 0u;
    for (int x = xa; x < xe; ++x) cnt += P[y * w + x] == y * w + x + 1 ? 1u : 0u;
    uint32_t incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += t;
    }
    __syncthreads();
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t id = base + incl - cnt;
    for (int j = 0; j < wave; ++j) id += wtot[j];
    u64* rec = a.records + (size_t)img * a.cap * LABEL_WORDS;
    for (int x = xa; x < xe; ++x) {
      const int i = y * w + x;
      if (P[i] != i + 1) continue;
      ++id;
      P[i] = -(int)id;
      if (id <= (uint32_t)a.cap) {
        u64* r = rec + (size_t)(id - 1) * LABEL_WORDS;
        r[1] = ~0ull, r[3] = ~0ull, r[12] = (u64)i;   // the two minima start at all-ones
      }
    }
  }
}

// ---- 6. ids for every pixel, and the statistics
// what some pixels of one component add to its record
struct Part {
  u64 s0, t0, s1, s2, s3, s4, t1, t2, flags;
  uint32_t xmin, xmax, ymin, ymax;
};

__device__ __forceinline__ Part part_none() {
  return Part{0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0xffffffffu, 0u, 0xffffffffu, 0u};
}

// cnt pixels of row yy with sum of x sx, between columns xmin and xmax
__device__ __forceinline__ void part_row(Part& p, uint32_t cnt, uint32_t sx, uint32_t xmin, uint32_t xmax, int yy, int h,
                                         int w) {
  const u64 y = (u64)yy, y2 = y * y, c = cnt, s = sx;
  p.s0 += c, p.t0 += s, p.s1 += c * y, p.s2 += c * y2, p.s3 += c * (y2 * y), p.s4 += c * (y2 * y2);
  p.t1 += s * y, p.t2 += s * y2;
  p.xmin = min(p.xmin, xmin), p.xmax = max(p.xmax, xmax);
  p.ymin = min(p.ymin, (uint32_t)yy), p.ymax = max(p.ymax, (uint32_t)yy);
  p.flags |= (yy == 0 ? 1ull : 0ull) | (yy == h - 1 ? 2ull : 0ull) | (xmin == 0u ? 4ull : 0ull) |
             (xmax == (uint32_t)(w - 1) ? 8ull : 0ull);
}

__device__ __forceinline__ void part_out(u64* rec, const Part& p) {
  atomicAdd(rec + 0, p.s0);
  atomicMin(rec + 1, (u64)p.xmin);
  atomicMax(rec + 2, (u64)p.xmax);
  atomicMin(rec + 3, (u64)p.ymin);
  atomicMax(rec + 4, (u64)p.ymax);
  if (p.t0) atomicAdd(rec + 5, p.t0);
  if (p.s1) {   // some y > 0
    atomicAdd(rec + 6, p.s1);
    atomicAdd(rec + 7, p.s2);
    atomicAdd(rec + 8, p.s3);
    atomicAdd(rec + 9, p.s4);
    if (p.t1) atomicAdd(rec + 10, p.t1), atomicAdd(rec + 11, p.t2);
  }
  if (p.flags) atomicOr(rec + 13, p.flags);
}

__device__ __forceinline__ void record_add(u64* rec, uint32_t cnt, uint32_t sx, uint32_t xmin, uint32_t xmax, int yy,
                                           int h, int w) {
  Part p = part_none();
  part_row(p, cnt, sx, xmin, xmax, yy, h, w);
  part_out(rec, p);
}

constexpr int PER_MAX = (LABEL_SIDE_MAX + THREADS - 1) / THREADS;   // pixels of a row a thread takes, at most
constexpr int STAT_ROWS = 4;                                        // consecutive rows a workgroup takes

__global__ __launch_bounds__(THREADS) void stats_kernel(const LabelArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, h = a.height, w = a.width;
  const int per = (w + THREADS - 1) / THREADS;
  const int bands = (h + STAT_ROWS - 1) / STAT_ROWS;
  const long long total = (long long)a.n * bands;
  for (long long bb = blockIdx.x; bb < total; bb += gridDim.x) {
    const long long img = bb / bands;
    const int y0 = (int)(bb % bands) * STAT_ROWS, y1 = min(y0 + STAT_ROWS, h);
    int32_t* P = a.labels + (size_t)img * h * w;
    u64* recs = a.records + (size_t)img * a.cap * LABEL_WORDS;
    const int xa = min(tid * per, w), xe = min(xa + per, w);
    // the wave's accumulator over the band, uniform over the wave: the component `bid` and what the wave has of it
    uint32_t bid = 0u;
    Part band = part_none();
    for (int y = y0; y < y1; ++y) {
      // the row's cells, then the cells of their roots, all loads of a kind in flight together
      int v[PER_MAX];
      uint32_t ids[PER_MAX];
#pragma unroll
      for (int j = 0; j < PER_MAX; ++j) v[j] = (j < per && xa + j < xe) ? ld_agent(P + y * w + xa + j) : 0;
#pragma unroll
      for (int j = 0; j < PER_MAX; ++j) {
        int rv = v[j];                                              // a root's own cell: -id
        if (v[j] > 0) rv = ld_agent(P + (v[j] - 1));                // the root's cell: -id, or +id once its owner has been here
        ids[j] = (uint32_t)(rv < 0 ? -rv : rv);
      }
#pragma unroll
      for (int j = 0; j < PER_MAX; ++j)
        if (ids[j]) st_agent(P + y * w + xa + j, (int)ids[j]);
      uint32_t id = 0u, cnt = 0u, sx = 0u, xmin = 0u;                          // the open run
      uint32_t aid = 0u, acnt = 0u, asx = 0u, amin = 0xffffffffu, amax = 0u;   // the wave's accumulator over the row; uniform
#pragma unroll
      for (int j = 0; j <= PER_MAX; ++j) {             // step `per` closes the last run
        if (j > per) continue;                         // uniform over the block
        const int x = xa + j;
        const uint32_t here = j < PER_MAX ? ids[j % PER_MAX] : 0u;
        const bool flush = id != 0u && here != id;     // inside a row a run is one component: here == id or here == 0
        const uint32_t fid = flush ? id : 0u, fcnt = flush ? cnt : 0u, fsx = flush ? sx : 0u;
        const uint32_t fmin = flush ? xmin : 0xffffffffu, fmax = flush ? (uint32_t)(x - 1) : 0u;
        // Runs that end at this step.  Those of one component are summed through shuffles first: up to two
        // components a step, picked by the first lane that still waits (a component that only one lane holds is
        // skipped unless it is the accumulator's).  The first such component a wave meets in the row stays in its
        // accumulator until the row ends; other sums go out through one lane.  What is left after two rounds every
        // lane adds itself.
        u64 pend = __ballot(flush), avoid = 0ull;
        bool mine = flush;
        for (int round = 0; round < 2 && (pend & ~avoid) != 0ull; ++round) {   // uniform over the wave
          const uint32_t t = (uint32_t)__shfl((int)fid, __ffsll((long long)(pend & ~avoid)) - 1, 64);
          const bool in = mine && fid == t;
          const u64 grp = __ballot(in);
          if (__popcll(grp) < 2 && t != aid) {
            avoid |= grp;
            continue;
          }
          const uint32_t c = wave_sum32(in ? fcnt : 0u), s = wave_sum32(in ? fsx : 0u);
          uint32_t mn = in ? fmin : 0xffffffffu, mx = in ? fmax : 0u;
#pragma unroll
          for (int d = 32; d >= 1; d >>= 1) {
            mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
            mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
          }
          if (aid == 0u || aid == t) aid = t, acnt += c, asx += s, amin = min(amin, mn), amax = max(amax, mx);
          else if (lane == 0 && t <= (uint32_t)a.cap) record_add(recs + (size_t)(t - 1) * LABEL_WORDS, c, s, mn, mx, y, h, w);
          if (in) mine = false;
          pend &= ~grp;
        }
        if (mine && fid <= (uint32_t)a.cap) record_add(recs + (size_t)(fid - 1) * LABEL_WORDS, fcnt, fsx, fmin, fmax, y, h, w);
        if (here) {
          if (here != id) id = here, cnt = 0u, sx = 0u, xmin = (uint32_t)x;
          cnt += 1u, sx += (uint32_t)x;
        } else {
          id = 0u;
        }
      }
      // the row's accumulator joins the band's: a marking stays under the same lanes from row to row
      if (aid != 0u) {
        if (bid != aid) {
          if (lane == 0 && bid != 0u && bid <= (uint32_t)a.cap) part_out(recs + (size_t)(bid - 1) * LABEL_WORDS, band);
          bid = aid, band = part_none();
        }
        part_row(band, acnt, asx, amin, amax, y, h, w);
      }
    }
    if (lane == 0 && bid != 0u && bid <= (uint32_t)a.cap) part_out(recs + (size_t)(bid - 1) * LABEL_WORDS, band);
  }
}

// ---- the component filter
struct KeepArgs {
  const int32_t* labels;
  const u64* header;
  const u64* records;
  uint8_t* keep;
  uint8_t* mask;
  int n, height, width, cap, minArea, minHeight, minWidth, keepLargest;
};

// 0 for a component that fails a threshold or has no record, else (area << 16) | (65535 - c): larger area first, lower
// id on equal area; area <= 2^22, so the key has 39 bits
__device__ __forceinline__ u64 keep_key(const KeepArgs& a, const u64* rec, int c, int nrec) {
  if (c >= nrec) return 0ull;
  const u64* r = rec + (size_t)c * LABEL_WORDS;
  const u64 area = r[0], bw = r[2] - r[1] + 1ull, bh = r[4] - r[3] + 1ull;
  if (area == 0ull || r[2] < r[1] || r[4] < r[3]) return 0ull;   // not a record of unet_label_u8_batch
  if (area < (u64)a.minArea || bh < (u64)a.minHeight || bw < (u64)a.minWidth) return 0ull;
  return (min(area, (1ull << 23) - 1ull) << 16) | (u64)(65535 - c);
}

__device__ __forceinline__ uint32_t block_sum(uint32_t v, uint32_t* wred) {   // wred[KEEP_THREADS / 64]
  v = wave_sum32(v);
  __syncthreads();   // the last sum is no longer read
  if ((threadIdx.x & 63) == 0) wred[threadIdx.x >> 6] = v;
  __syncthreads();
  uint32_t t = 0u;
#pragma unroll
  for (int j = 0; j < KEEP_THREADS / 64; ++j) t += wred[j];
  return t;
}

__global__ __launch_bounds__(KEEP_THREADS) void keep_table_kernel(const KeepArgs a) {
  __shared__ uint32_t wred[KEEP_THREADS / 64];
  const int tid = threadIdx.x;
  for (long long img = blockIdx.x; img < a.n; img += gridDim.x) {
    const u64* rec = a.records + (size_t)img * a.cap * LABEL_WORDS;
    const int nrec = (int)min(a.header[(size_t)img * 4 + 2], (u64)a.cap);
    u64 threshold = 1ull;   // keep iff key >= threshold
    // Only records below nrec have a key.  Up to KEEP_OWN of them a thread, thread t's being t, t + 1024, ..., stay in
    // its registers; a frame with more recorded components reads its records again for every count below.
    const bool own = nrec <= KEEP_OWN * KEEP_THREADS;
    u64 kk[KEEP_OWN];
#pragma unroll
    for (int k = 0; k < KEEP_OWN; ++k) kk[k] = own ? keep_key(a, rec, tid + k * KEEP_THREADS, nrec) : 0ull;
    if (a.keepLargest > 0) {
      uint32_t mine = 0u;
      if (own) {
#pragma unroll
        for (int k = 0; k < KEEP_OWN; ++k) mine += kk[k] ? 1u : 0u;
      } else {
        for (int c = tid; c < nrec; c += KEEP_THREADS) mine += keep_key(a, rec, c, nrec) ? 1u : 0u;
      }
      const uint32_t passing = block_sum(mine, wred);
      if ((uint32_t)a.keepLargest < passing) {
        // the keepLargest-th largest key, bit by bit from the top (keys are distinct)
        uint32_t want = (uint32_t)a.keepLargest;
        u64 prefix = 0ull;
        for (int bit = 39; bit >= 0; --bit) {
          const u64 probe = (prefix >> bit) | 1ull;
          uint32_t cntMine = 0u;
          if (own) {
#pragma unroll
            for (int k = 0; k < KEEP_OWN; ++k) cntMine += (kk[k] >> bit) == probe ? 1u : 0u;
          } else {
            for (int c = tid; c < nrec; c += KEEP_THREADS) cntMine += (keep_key(a, rec, c, nrec) >> bit) == probe ? 1u : 0u;
          }
          const uint32_t cnt = block_sum(cntMine, wred);
          if (cnt >= want) prefix |= 1ull << bit;
          else want -= cnt;
        }
        threshold = prefix;
      }
    }
    uint8_t* keep = a.keep + (size_t)img * a.cap;
    for (int c = tid; c < a.cap; c += KEEP_THREADS) {
      const u64 k = c < nrec ? keep_key(a, rec, c, nrec) : 0ull;
      keep[c] = (k != 0ull && k >= threshold) ? 1 : 0;
    }
  }
}

__global__ __launch_bounds__(THREADS) void keep_mask_kernel(const KeepArgs a) {
  const long long hw = (long long)a.height * a.width, B = hw * a.n;
  const int mis = (int)(reinterpret_cast<uintptr_t>(a.mask) & 15u);
  const long long nch = (mis + B + 15) >> 4;
  for (long long c = (long long)blockIdx.x * THREADS + threadIdx.x; c < nch; c += (long long)gridDim.x * THREADS) {
    const long long fb = 16ll * c - mis;   // offset of the chunk's first byte; negative in front of the output
    uint32_t wd[4] = {0u, 0u, 0u, 0u};
    const bool whole = fb >= 0 && fb + 16 <= B;
    long long f = fb < 0 ? 0 : fb;
    const long long fe = fb + 16 < B ? fb + 16 : B;
    long long img = f / hw, next = (img + 1) * hw;   // the frame of byte f, and where the next one starts
    for (; f < fe; ++f) {
      if (f == next) ++img, next += hw;
      const int lab = a.labels[f];
      const uint32_t v = (lab > 0 && lab <= a.cap && a.keep[(size_t)img * a.cap + (lab - 1)]) ? 255u : 0u;
      const int b = (int)(f - fb);
      if (whole) wd[b >> 2] |= v << (8 * (b & 3));
      else a.mask[f] = (uint8_t)v;
    }
    if (whole) *reinterpret_cast<uint4*>(a.mask + fb) = make_uint4(wd[0], wd[1], wd[2], wd[3]);
  }
}

unsigned grid_for(long long items) { return (unsigned)std::min<long long>(std::max<long long>(items, 1), GRID_MAX); }

}  // namespace

size_t label_work_bytes(int n, int height, int width) {
  if (n < 1 || height < 1 || height > LABEL_SIDE_MAX || width < 1 || width > LABEL_SIDE_MAX) return 0;
  if (!fits_int((unsigned long long)n * height * width)) return 0;
  return (((size_t)n * height * 2 * sizeof(uint32_t)) + 255) & ~(size_t)255;
}

hipError_t launch_label(const uint8_t* masks, int n, int height, int width, int level, int connectivity,
                        int32_t* labels, int cap, unsigned long long* header, unsigned long long* records, void* work,
                        hipStream_t s) {
  LabelArgs a;
  a.masks = masks, a.labels = labels, a.header = header, a.records = records, a.work = static_cast<uint32_t*>(work);
  a.n = n, a.height = height, a.width = width, a.level = level, a.conn8 = connectivity == 8 ? 1 : 0, a.cap = cap;
  const long long tiles = (long long)n * ((height + TH - 1) / TH) * ((width + TW - 1) / TW);
  const long long rows = (long long)n * height;
  hipLaunchKernelGGL(tile_kernel, dim3(grid_for(tiles)), dim3(THREADS), 0, s, a);
  const int nbh = (height - 1) / TH, nbv = (width - 1) / TW;
  const long long border = ((long long)nbh * width + (long long)nbv * height) * n;
  if (border > 0)
    hipLaunchKernelGGL(border_kernel, dim3(grid_for((border + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a, nbh, nbv);
  hipLaunchKernelGGL(flatten_kernel, dim3(grid_for(rows)), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(scan_kernel, dim3(grid_for(n)), dim3(SCAN_THREADS), 0, s, a);
  hipLaunchKernelGGL(rank_kernel, dim3(grid_for(rows)), dim3(THREADS), 0, s, a);
  hipLaunchKernelGGL(stats_kernel, dim3(grid_for((long long)n * ((height + STAT_ROWS - 1) / STAT_ROWS))), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_keep_components(const int32_t* labels, int n, int height, int width, const unsigned long long* header,
                                  const unsigned long long* records, int cap, int minArea, int minHeight, int minWidth,
                                  int keepLargest, uint8_t* keep, uint8_t* mask, hipStream_t s) {
  KeepArgs a;
  a.labels = labels, a.header = header, a.records = records, a.keep = keep, a.mask = mask;
  a.n = n, a.height = height, a.width = width, a.cap = cap;
  a.minArea = minArea, a.minHeight = minHeight, a.minWidth = minWidth, a.keepLargest = keepLargest;
  hipLaunchKernelGGL(keep_table_kernel, dim3(grid_for(n)), dim3(KEEP_THREADS), 0, s, a);
  const long long chunks = ((long long)n * height * width + 30) / 16;
  hipLaunchKernelGGL(keep_mask_kernel, dim3(grid_for((chunks + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace unet

namespace {

// the checks both entry points share; nullptr if the shape is in the domain
const char* bad_shape(int n, int height, int width, int maxComponents) {
  if (n <= 0) return "n must be positive";
  if (height < 1 || height > unet::LABEL_SIDE_MAX) return "height must lie in 1 .. 2048";
  if (width < 1 || width > unet::LABEL_SIDE_MAX) return "width must lie in 1 .. 2048";
  if (!unet::fits_int((unsigned long long)n * height * width))
    return "n * height * width must be smaller than 2^31";
  if (maxComponents < 1 || maxComponents > unet::LABEL_COMPONENTS_MAX) return "max_components must lie in 1 .. 65536";
  return nullptr;
}

}  // namespace

extern "C" {

size_t unet_label_work_bytes(int n, int height, int width) { return unet::label_work_bytes(n, height, width); }

int unet_label_u8_batch(int device, const uint8_t* masksDev, int n, int height, int width, int level, int connectivity,
                        int32_t* labelsDev, int maxComponents, unsigned long long* headerDev,
                        unsigned long long* recordsDev, void* workDev, size_t workBytes, void* stream) {
  const unet::OpCall op{"unet_label_u8_batch"};
  if (!masksDev || !labelsDev || !headerDev || !recordsDev || !workDev) return op.refuse("a null pointer");
  if (const char* why = bad_shape(n, height, width, maxComponents)) return op.refuse(why);
  if (level < 0 || level > 255) return op.refuse("level must lie in 0 .. 255");
  if (connectivity != 4 && connectivity != 8) return op.refuse("connectivity must be 4 or 8");
  if (workBytes < unet::label_work_bytes(n, height, width))
    return op.refuse("work_bytes is smaller than unet_label_work_bytes(n, height, width)");
  if (unet::misaligned(labelsDev, 4) || unet::misaligned(workDev, 4) || unet::misaligned(headerDev, 8) ||
      unet::misaligned(recordsDev, 8))
    return op.refuse("labels_dev and work_dev must be 4-byte aligned, header_dev and records_dev 8-byte aligned");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_label(masksDev, n, height, width, level, connectivity, labelsDev, maxComponents, headerDev,
                                    recordsDev, workDev, (hipStream_t)stream));
}

int unet_keep_components_u8_batch(int device, const int32_t* labelsDev, int n, int height, int width,
                                  const unsigned long long* headerDev, const unsigned long long* recordsDev,
                                  int maxComponents, int minArea, int minHeight, int minWidth, int keepLargest,
                                  uint8_t* keepOutDev, uint8_t* maskOutDev, void* stream) {
  const unet::OpCall op{"unet_keep_components_u8_batch"};
  if (!labelsDev || !headerDev || !recordsDev || !keepOutDev || !maskOutDev) return op.refuse("a null pointer");
  if (const char* why = bad_shape(n, height, width, maxComponents)) return op.refuse(why);
  if (minArea < 0) return op.refuse("min_area must not be negative");
  if (minHeight < 0) return op.refuse("min_height must not be negative");
  if (minWidth < 0) return op.refuse("min_width must not be negative");
  if (keepLargest < 0) return op.refuse("keep_largest must not be negative");
  if (unet::misaligned(labelsDev, 4) || unet::misaligned(headerDev, 8) || unet::misaligned(recordsDev, 8))
    return op.refuse("labels_dev must be 4-byte aligned, header_dev and records_dev 8-byte aligned");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_keep_components(labelsDev, n, height, width, headerDev, recordsDev, maxComponents, minArea,
                                              minHeight, minWidth, keepLargest, keepOutDev, maskOutDev, (hipStream_t)stream));
}

}  // extern "C"
