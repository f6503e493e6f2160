// The polygon rasteriser (annotate_kernels.h): plain C++, integer arithmetic, no atomics, one launch.
//
// fill_polygons_kernel   a block of 256 threads owns a 64 x 64 tile of output pixels of one frame; thread t owns 16
//                        consecutive pixels of tile row t / 4.  The tile's source columns and rows (sx, sy) are computed
//                        once into LDS.  Wave 0 walks the frame's polygons in order, 64 edges (vertex i -> i + 1, the
//                        last back to the first) at a time, orients each edge upwards (ya <= yb; a horizontal one
//                        left to right) and keeps those whose rows meet the tile's source rows and whose largest x is
//                        not left of the tile's source columns - an edge further left neither counts for the parity
//                        (only crossings right of the point do) nor draws.  A ballot compacts the kept edges, order
//                        preserved, into LDS records; the first kept edge of a polygon carries a flag.  Then every
//                        thread runs the records: per record the row terms once, per pixel one 32 x 32 -> 64-bit
//                        product shared by the parity's and the outline's sign tests.  A pixel keeps one parity bit
//                        and one outline bit for the polygon in progress; at a polygon's flag the covered pixels take
//                        the finished polygon's value (painter's order).  When the records fill the LDS budget (CAP)
//                        the block runs what it has and wave 0 goes on where it stopped: polygon, parity, outline bit
//                        and value live in registers across the chunks, so a frame's edges are bounded by int32 only.
//                        A thread's 16 bytes leave as one 16-byte store where they are all inside the row and the
//                        address allows, byte by byte otherwise.  Every output byte is written by exactly one thread.
//
// Magnitudes: coordinates are clamped to +-2^20 and sizes are at most 2^14, so differences stay below 2^22, products
// below 2^44 and every sum below 2^46.
//
// Bounds: P = frame_offsets[n] and V = poly_offsets[P] are the table sizes; every other offset is clamped into them and
// made non-decreasing before use, so no table makes the kernel read outside arrays of those sizes.
#include "annotate_kernels.h"

#include "op_entry.h"

namespace unet {

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int THREADS = 256, TILE = 64, PIX = 16;
constexpr int CAP = 1024;          // records per chunk: 20 KB of LDS
constexpr int NEW_POLY = 0x100;    // record flag: the first kept edge of its polygon

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the pixels of `cover` (one bit each) take `value`; vals holds the thread's 16 bytes
__device__ __forceinline__ void paint(uint32_t (&vals)[4], uint32_t cover, int value) {
  const uint32_t v4 = (uint32_t)value * 0x01010101u;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const uint32_t b = (cover >> (4 * w)) & 15u;
    const uint32_t m = ((b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21)) * 0xFFu;
    vals[w] = (vals[w] & ~m) | (v4 & m);
  }
}

__global__ __launch_bounds__(THREADS) void fill_polygons_kernel(FillParams p) {
  __shared__ int4 sPts[CAP];
  __shared__ int sMeta[CAP];
  __shared__ int sSx[TILE], sSy[TILE];
  __shared__ int sCount, sDone;

  const int tid = threadIdx.x, lane = tid & 63;
  const int f = blockIdx.x, X0 = blockIdx.z * TILE, Y0 = blockIdx.y * TILE;
  // columns and rows past the output repeat the last valid one: computed, never stored
  if (tid < TILE) {
    const int X = min(X0 + tid, p.outW - 1);
    sSx[tid] = (int)(((i64)X * p.srcW) / p.outW);
  } else if (tid < 2 * TILE) {
    const int Y = min(Y0 + tid - TILE, p.outH - 1);
    sSy[tid - TILE] = (int)(((i64)Y * p.srcH) / p.outH);
  }
  __syncthreads();
  const int minSx = sSx[0], maxSy = sSy[TILE - 1], minSy = sSy[0];
  const int r = tid >> 2, g = tid & 3;
  const int sy = sSy[r];
  int sx[PIX];
#pragma unroll
  for (int j = 0; j < PIX; ++j) sx[j] = sSx[g * PIX + j];

  const int P = max(p.frameOffsets[p.n], 0);
  const int V = max(p.polyOffsets[P], 0);
  const int pBeg = clampi(p.frameOffsets[f], 0, P);
  const int pEnd = clampi(p.frameOffsets[f + 1], pBeg, P);

  int poly = pBeg, lastKept = -1;   // wave 0's walk: the polygon, the first of its edges not yet seen, ...
  i64 base = 0;
  uint32_t par = 0, hit = 0, vals[4] = {0u, 0u, 0u, 0u};
  int curVal = 0;
  for (;;) {
    if (tid < 64) {
      int cnt = 0;
      while (poly < pEnd && cnt <= CAP - 64) {
        const int v0 = clampi(p.polyOffsets[poly], 0, V);
        const int v1 = clampi(p.polyOffsets[poly + 1], v0, V);
        const i64 k = (i64)v1 - v0;
        if (base >= k) {
          ++poly, base = 0;
          continue;
        }
        const i64 i = base + lane;
        bool keep = false;
        int4 q = make_int4(0, 0, 0, 0);
        if (i < k) {
          const i64 i2 = (i + 1 == k) ? 0 : i + 1;
          const int2 a = reinterpret_cast<const int2*>(p.vertices)[(size_t)v0 + (size_t)i];
          const int2 b = reinterpret_cast<const int2*>(p.vertices)[(size_t)v0 + (size_t)i2];
          int ax = clampi(a.x, -ANNOTATE_COORD_LIMIT, ANNOTATE_COORD_LIMIT);
          int ay = clampi(a.y, -ANNOTATE_COORD_LIMIT, ANNOTATE_COORD_LIMIT);
          int bx = clampi(b.x, -ANNOTATE_COORD_LIMIT, ANNOTATE_COORD_LIMIT);
          int by = clampi(b.y, -ANNOTATE_COORD_LIMIT, ANNOTATE_COORD_LIMIT);
          if (ay > by || (ay == by && ax > bx)) {
            int t = ax; ax = bx; bx = t;
            t = ay; ay = by; by = t;
          }
          keep = by >= minSy && ay <= maxSy && max(ax, bx) >= minSx;
          q = make_int4(ax, ay, bx, by);
        }
        const u64 mask = __ballot(keep);
        if (keep) {
          const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
          sPts[pos] = q;
          sMeta[pos] = (int)p.polyValues[poly] | ((pos == cnt && poly != lastKept) ? NEW_POLY : 0);
        }
        if (mask) lastKept = poly, cnt += __popcll(mask);
        base += 64;
      }
      if (lane == 0) sCount = cnt, sDone = poly >= pEnd ? 1 : 0;
    }
    __syncthreads();
    const int cnt = sCount, done = sDone;
    for (int e = 0; e < cnt; ++e) {
      const int4 q = sPts[e];
      const int mt = sMeta[e];
      if (mt & NEW_POLY) {
        paint(vals, par | hit, curVal);
        par = hit = 0u;
        curVal = mt & 255;
      }
      const int xa = q.x, ya = q.y, xb = q.z, yb = q.w;
      if (sy < ya || sy > yb) continue;   // neither test passes outside the edge's rows
      const int dxp = xb - xa, dyp = yb - ya, adx = dxp < 0 ? -dxp : dxp;
      // parity: ya <= sy < yb and dxp (sy - ya) - dyp (sx - xa) > 0
      const bool rowP = sy < yb;
      const i64 A = (i64)dxp * (sy - ya);
      // outline: 0 <= t < lim with t = E +- 2 dyp (sx - xa), the issue's test on the edge oriented for its major axis
      i64 E;
      u64 lim;
      bool neg;
      if (adx >= dyp) {
        if (dxp == 0) {          // a point (dyp is 0 too, so sy == ya here)
          E = 0, lim = 1, neg = false;
        } else if (dxp > 0) {    // (x0, y0) = (xa, ya)
          E = (i64)dxp - 2 * (i64)dxp * (sy - ya), lim = 2 * (u64)dxp, neg = false;
        } else {                 // (x0, y0) = (xb, yb), dx = -dxp, dy = -dyp
          E = 2 * (i64)dyp * dxp + adx - 2 * (i64)adx * (sy - yb), lim = 2 * (u64)adx, neg = true;
        }
      } else {                   // x and y exchanged; (x0, y0) = (xa, ya)
        E = 2 * (i64)(sy - ya) * dxp + dyp, lim = 2 * (u64)dyp, neg = true;
      }
      const int xlo = min(xa, xb), xhi = max(xa, xb);
#pragma unroll
      for (int j = 0; j < PIX; ++j) {
        const i64 m = (i64)dyp * (sx[j] - xa);
        const bool c = rowP && (A - m > 0);
        const i64 t = neg ? E - 2 * m : E + 2 * m;
        const bool h = sx[j] >= xlo && sx[j] <= xhi && (u64)t < lim;
        par ^= (c ? 1u : 0u) << j;
        hit |= (h ? 1u : 0u) << j;
      }
    }
    __syncthreads();   // the records are free for wave 0's next chunk
    if (done) break;
  }
  paint(vals, par | hit, curVal);

  const int Y = Y0 + r, X = X0 + g * PIX;
  if (Y < p.outH && X < p.outW) {
    uint8_t* dst = p.out + ((size_t)f * p.outH + Y) * p.outW + X;
    if (X + PIX <= p.outW && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {
      *reinterpret_cast<uint4*>(dst) = make_uint4(vals[0], vals[1], vals[2], vals[3]);
    } else {
      const int nv = min(PIX, p.outW - X);
#pragma unroll
      for (int j = 0; j < PIX; ++j)
        if (j < nv) dst[j] = (uint8_t)(vals[j >> 2] >> (8 * (j & 3)));
    }
  }
}

}  // namespace

hipError_t launch_fill_polygons(const FillParams& p, hipStream_t s) {
  const dim3 grid((unsigned)p.n, (unsigned)((p.outH + TILE - 1) / TILE), (unsigned)((p.outW + TILE - 1) / TILE));
  hipLaunchKernelGGL(fill_polygons_kernel, grid, dim3(THREADS), 0, s, p);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

int unet_fill_polygons_u8_batch(int device, const int32_t* verticesDev, const int32_t* polyOffsetsDev,
                                const uint8_t* polyValuesDev, const int32_t* frameOffsetsDev, int n, int srcH, int srcW,
                                int outH, int outW, uint8_t* masksOutDev, void* stream) {
  const unet::OpCall op{"unet_fill_polygons_u8_batch"};
  if (!verticesDev || !polyOffsetsDev || !polyValuesDev || !frameOffsetsDev || !masksOutDev)
    return op.refuse("a null pointer");
  if (n <= 0) return op.refuse("n must be positive");
  if (unet::misaligned(verticesDev, 8) || unet::misaligned(polyOffsetsDev, 4) || unet::misaligned(frameOffsetsDev, 4))
    return op.refuse("vertices_dev must be 8-byte aligned, the offsets 4-byte aligned");
  if (srcH < 1 || srcW < 1 || outH < 1 || outW < 1 || srcH > unet::ANNOTATE_MAX_SIDE || srcW > unet::ANNOTATE_MAX_SIDE ||
      outH > unet::ANNOTATE_MAX_SIDE || outW > unet::ANNOTATE_MAX_SIDE)
    return op.refuse("source and output sizes must be 1 .. 16384", UNET_ERR_SHAPE);
  if (int rc = op.on(device)) return rc;
  unet::FillParams p;
  p.vertices = verticesDev, p.polyOffsets = polyOffsetsDev, p.polyValues = polyValuesDev;
  p.frameOffsets = frameOffsetsDev, p.out = masksOutDev;
  p.n = n, p.srcH = srcH, p.srcW = srcW, p.outH = outH, p.outW = outW;
  return op.done(unet::launch_fill_polygons(p, (hipStream_t)stream));
}

}  // extern "C"
