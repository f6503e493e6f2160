// Lane following's two kernels (follow_kernels.h): plain C++, integer arithmetic only.
//
// hsv_lanes_kernel.  The threshold plane is binary, so a block keeps its part of it as bit words in LDS: a region of
// RW = 256 columns (four 64-bit words a row) by th + 2 halo rows, halo = 2 (kc/2 + ko/2) <= 12, of which the inner
// (256 - 2 halo) x TH pixels are the block's output tile.  One wave ballot turns 64 pixels' inRange results into one
// word.  The frame's bytes come through LDS as well: a wave covers the up to 768 bytes of its region row with 16-byte
// loads at 16-byte aligned ADDRESSES (so the base pointer's alignment does not matter), the first and last chunk of
// the whole buffer byte by byte where a 16-byte access would leave it, and every lane then picks its pixel's three
// bytes out of LDS.  The next rows' loads are in flight while the current ones are thresholded.
//   dilate / erode by a k x k box = OR / AND of the words shifted by -k/2 .. k/2 with carries between neighbouring
//   words (horizontal pass) and of the rows y-k/2 .. y+k/2 (vertical pass).
// Borders: a pixel outside the image is neutral at every step.  The threshold plane is 0 there (neutral to the OR of
// the first dilation); after it the outside bits are set to 1 (neutral to the AND); the two erosions in the middle are
// one erosion of size kc + ko - 1 (on a rectangle with neutral borders the two compose exactly); after it the outside
// bits are cleared for the last dilation.  What the shifts pull in from beyond the REGION is wrong, and reaches
// kc/2 + (kc/2 + ko/2) + ko/2 = halo bits inwards at the most: never the output tile.
// The tile leaves as 16-byte stores at aligned addresses, with single bytes in front of and behind them in each row.
//
// lane_center_kernel.  One wave per (frame, scan row): aligned 16-byte loads of the row, single bytes at its ends, a
// count and a sum of x per lane, a shuffle reduction, two ordinary dword stores by lane 0.
//
// No argument the entry points accept makes either kernel read or write outside its buffers.
#include "follow_kernels.h"
#include "hsv8.h"

#include "op_entry.h"

#include <cstring>

namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int RW = 256, WORDS = RW / 64;          // region columns, as bits of four words
constexpr int TH = 64, HALO_MAX = 12;             // output rows of a tile; 2 * (3 + 3)
constexpr int ROWS_MAX = TH + 2 * HALO_MAX;
constexpr int CHUNKS = (RW * 3 + 15 + 15) / 16;   // 16-byte chunks that cover 768 bytes at any alignment: 49
constexpr int STAGE_PITCH = 52;                   // uint4 per staged row

struct HsvArgs {
  const uint8_t* frames;
  uint8_t* out;
  int n, height, width;
  int tilesX, tilesY, tw;   // tw = RW - 2 * halo: output columns of a tile
  int rc, ro;               // kc / 2, ko / 2
  int swap;                 // frames are BGR
  int lo[3], hi[3];         // inRange bounds on H, S, V
};

// the bytes of region row y of image `img` as a run of 16-byte chunks at aligned addresses: offset of the first chunk
// from the frames' base (-15 at the least), offset of the row's first byte in the run, number of chunks
struct RowSpan {
  long long o0;
  int off, nch;
};

__device__ __forceinline__ RowSpan row_span(const HsvArgs& a, int img, int y, int cx0, int cx1) {
  const long long sb = (((long long)img * a.height + y) * a.width + cx0) * 3;
  RowSpan r;
  r.off = (int)((reinterpret_cast<uintptr_t>(a.frames) + (uintptr_t)sb) & 15u);
  r.o0 = sb - r.off;
  r.nch = (r.off + (cx1 - cx0) * 3 + 15) >> 4;   // <= CHUNKS
  return r;
}

// the 16 bytes at offset o of a buffer of `total` bytes: one 16-byte load, or - where that would leave the buffer -
// its bytes inside it
__device__ __forceinline__ uint4 load_chunk(const uint8_t* __restrict__ base, long long o, long long total) {
  if (o >= 0 && o + 16 <= total) return *reinterpret_cast<const uint4*>(base + o);
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (o + j >= 0 && o + j < total) w[j >> 2] |= (uint32_t)base[o + j] << (8 * (j & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// bits [lo, hi) of a word, 0 <= lo, hi <= 64
__device__ __forceinline__ u64 bit_range(int lo, int hi) {
  if (hi <= lo) return 0ull;
  const u64 upto = hi >= 64 ? ~0ull : ((1ull << hi) - 1ull);
  return upto & ~((1ull << lo) - 1ull);   // lo < hi <= 64, so lo <= 63
}

// the in-image bits of word k of a region row whose bit 0 is column gx0
__device__ __forceinline__ u64 inside_mask(int gx0, int k, int width) {
  const int c0 = gx0 + 64 * k;
  return bit_range(min(max(-c0, 0), 64), min(max(width - c0, 0), 64));
}

// word k of a row after OR (AND) of its shifts by -r .. r; zeros come in from beyond the region
template <bool AND>
__device__ __forceinline__ u64 hpass(const u64* row, int k, int r) {
  const u64 c = row[k], p = k > 0 ? row[k - 1] : 0ull, nx = k < WORDS - 1 ? row[k + 1] : 0ull;
  u64 acc = c;
  for (int s = 1; s <= r; ++s) {
    const u64 l = (c << s) | (p >> (64 - s)), rr = (c >> s) | (nx << (64 - s));
    acc = AND ? (acc & l & rr) : (acc | l | rr);
  }
  return acc;
}

// word k of the rows ry-r .. ry+r inside the region, OR (AND)
template <bool AND>
__device__ __forceinline__ u64 vpass(const u64 (*plane)[WORDS], int rows, int ry, int k, int r) {
  u64 acc = plane[ry][k];
  for (int yy = max(ry - r, 0); yy <= min(ry + r, rows - 1); ++yy) acc = AND ? (acc & plane[yy][k]) : (acc | plane[yy][k]);
  return acc;
}

// 16 bits of a region row from bit b0 on (b0 + 16 <= RW)
__device__ __forceinline__ uint32_t bits16(const u64* row, int b0) {
  const int k = b0 >> 6, sh = b0 & 63;
  u64 v = row[k] >> sh;
  if (sh > 48 && k + 1 < WORDS) v |= row[k + 1] << (64 - sh);
  return (uint32_t)v & 0xffffu;
}

// 4 bits -> 4 bytes of 0 / 255
__device__ __forceinline__ uint32_t spread4(uint32_t x) { return (((x & 15u) * 0x00204081u) & 0x01010101u) * 255u; }

__global__ __launch_bounds__(THREADS) void hsv_lanes_kernel(const HsvArgs a) {
  __shared__ uint4 stage[2][WAVES][STAGE_PITCH];
  __shared__ u64 A[ROWS_MAX][WORDS], B[ROWS_MAX][WORDS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tilesPer = a.tilesX * a.tilesY;
  const int img = (int)(blockIdx.x / (unsigned)tilesPer), tIdx = (int)(blockIdx.x - (unsigned)img * tilesPer);
  const int ty = tIdx / a.tilesX, tx = tIdx - ty * a.tilesX;
  const int re = a.rc + a.ro, halo = 2 * re;
  const int gx0 = tx * a.tw - halo, gy0 = ty * TH - halo;
  const int th = min(TH, a.height - ty * TH), rows = th + 2 * halo;   // <= ROWS_MAX
  const int cx0 = max(gx0, 0), cx1 = min(gx0 + RW, a.width);          // the region's columns inside the image
  const long long total = (long long)a.n * a.height * a.width * 3;

  // ---- the threshold plane: wave w takes region rows w, w + 4, ...
  const int groups = (rows + WAVES - 1) / WAVES;
  uint4 cur = make_uint4(0u, 0u, 0u, 0u);
  {
    const int y = gy0 + wave;
    if (wave < rows && y >= 0 && y < a.height) {
      const RowSpan sp = row_span(a, img, y, cx0, cx1);
      if (lane < sp.nch) cur = load_chunk(a.frames, sp.o0 + 16 * lane, total);
    }
  }
  for (int g = 0; g < groups; ++g) {
    const int ry = g * WAVES + wave, y = gy0 + ry;
    const bool live = ry < rows && y >= 0 && y < a.height;
    if (lane < STAGE_PITCH) stage[g & 1][wave][lane] = cur;
    {
      const int ryn = ry + WAVES, yn = gy0 + ryn;
      cur = make_uint4(0u, 0u, 0u, 0u);
      if (ryn < rows && yn >= 0 && yn < a.height) {
        const RowSpan sp = row_span(a, img, yn, cx0, cx1);
        if (lane < sp.nch) cur = load_chunk(a.frames, sp.o0 + 16 * lane, total);
      }
    }
    __syncthreads();   // the buffer written two steps from now is the one read here: one barrier a step is enough
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage[g & 1][wave]);
    const int off = live ? row_span(a, img, y, cx0, cx1).off : 0;
#pragma unroll
    for (int k = 0; k < WORDS; ++k) {
      const int x = gx0 + 64 * k + lane;
      bool in = false;
      if (live && x >= cx0 && x < cx1) {
        const uint8_t* px = bytes + off + 3 * (x - cx0);
        const int c0 = px[0], c1 = px[1], c2 = px[2];
        in = hsv8_in_range(a.swap ? c2 : c0, c1, a.swap ? c0 : c2, a.lo, a.hi);
      }
      const u64 word = __ballot(in);
      if (lane == k && ry < rows) A[ry][k] = word;
    }
  }
  __syncthreads();

  // ---- CLOSE's dilation; outside the image -> 1
  const int items = rows * WORDS;
  for (int i = tid; i < items; i += THREADS) B[i / WORDS][i % WORDS] = hpass<false>(A[i / WORDS], i % WORDS, a.rc);
  __syncthreads();
  for (int i = tid; i < items; i += THREADS) {
    const int ry = i / WORDS, k = i % WORDS, y = gy0 + ry;
    A[ry][k] = (y >= 0 && y < a.height) ? (vpass<false>(B, rows, ry, k, a.rc) | ~inside_mask(gx0, k, a.width)) : ~0ull;
  }
  __syncthreads();
  // ---- CLOSE's erosion and OPEN's erosion as one; outside the image -> 0
  for (int i = tid; i < items; i += THREADS) B[i / WORDS][i % WORDS] = hpass<true>(A[i / WORDS], i % WORDS, re);
  __syncthreads();
  for (int i = tid; i < items; i += THREADS) {
    const int ry = i / WORDS, k = i % WORDS, y = gy0 + ry;
    A[ry][k] = (y >= 0 && y < a.height) ? (vpass<true>(B, rows, ry, k, re) & inside_mask(gx0, k, a.width)) : 0ull;
  }
  __syncthreads();
  // ---- OPEN's dilation
  for (int i = tid; i < items; i += THREADS) B[i / WORDS][i % WORDS] = hpass<false>(A[i / WORDS], i % WORDS, a.ro);
  __syncthreads();
  for (int i = tid; i < items; i += THREADS) A[i / WORDS][i % WORDS] = vpass<false>(B, rows, i / WORDS, i % WORDS, a.ro);
  __syncthreads();

  // ---- the tile's rows: 32 lanes a row; lanes 0..15 one aligned 16-byte store each, lane 16 the bytes in front of
  // the first of them, lane 17 the bytes behind the last
  const int x0 = tx * a.tw, len = min(a.tw, a.width - x0);   // 1 <= len <= RW
  for (int i = tid; i < th * 32; i += THREADS) {
    const int oy = i >> 5, sub = i & 31;
    const u64* row = A[halo + oy];
    uint8_t* dst = a.out + ((size_t)img * a.height + (ty * TH + oy)) * a.width + x0;
    const int head = min((int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u), len);
    const int nvec = (len - head) >> 4;   // <= 16
    if (sub < nvec) {
      const uint32_t b = bits16(row, halo + head + 16 * sub);
      *reinterpret_cast<uint4*>(dst + head + 16 * sub) = make_uint4(spread4(b), spread4(b >> 4), spread4(b >> 8), spread4(b >> 12));
    } else if (sub == 16) {
      for (int j = 0; j < head; ++j) dst[j] = (uint8_t)(((row[(halo + j) >> 6] >> ((halo + j) & 63)) & 1ull) ? 255 : 0);
    } else if (sub == 17) {
      for (int j = head + 16 * nvec; j < len; ++j) dst[j] = (uint8_t)(((row[(halo + j) >> 6] >> ((halo + j) & 63)) & 1ull) ? 255 : 0);
    }
  }
}

struct LaneArgs {
  const uint8_t* masks;
  uint32_t* out;
  int height, width, nRows, level;
};

__global__ __launch_bounds__(64) void lane_center_kernel(const LaneArgs a, const LaneRows rows) {
  const int item = (int)blockIdx.x, lane = threadIdx.x;   // one wave a block: the item is the wave's own
  const int img = item / a.nRows, j = item - img * a.nRows;
  const uint8_t* __restrict__ row = a.masks + ((size_t)img * a.height + rows.r[j]) * a.width;
  const int mis = (int)(reinterpret_cast<uintptr_t>(row) & 15u);   // the run of aligned chunks starts `mis` bytes in front
  const int nch = (mis + a.width + 15) >> 4;
  uint32_t cnt = 0u, sum = 0u;
  for (int c = lane; c < nch; c += 64) {
    const int xb = 16 * c - mis;   // x of the chunk's first byte; negative in front of the row
    if (xb >= 0 && xb + 16 <= a.width) {
      const uint4 v = *reinterpret_cast<const uint4*>(row + xb);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const uint32_t on = (int)((w[b >> 2] >> (8 * (b & 3))) & 255u) > a.level ? 1u : 0u;
        cnt += on, sum += on * (uint32_t)(xb + b);
      }
    } else {
      for (int b = 0; b < 16; ++b) {
        if (xb + b >= 0 && xb + b < a.width && (int)row[xb + b] > a.level) cnt += 1u, sum += (uint32_t)(xb + b);
      }
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    cnt += __shfl_xor(cnt, d, 64);
    sum += __shfl_xor(sum, d, 64);
  }
  if (lane == 0) {
    a.out[2 * (size_t)item] = cnt;
    a.out[2 * (size_t)item + 1] = sum;
  }
}

}  // namespace

hipError_t launch_hsv_lanes(const uint8_t* frames, int n, int height, int width, int isBgr, const uint8_t lower[3],
                            const uint8_t upper[3], int closeK, int openK, uint8_t* maskOut, hipStream_t s) {
  HsvArgs a;
  a.frames = frames, a.out = maskOut;
  a.n = n, a.height = height, a.width = width;
  a.rc = closeK / 2, a.ro = openK / 2;
  a.tw = RW - 4 * (a.rc + a.ro);
  a.tilesX = (width + a.tw - 1) / a.tw, a.tilesY = (height + TH - 1) / TH;
  a.swap = isBgr ? 1 : 0;
  for (int c = 0; c < 3; ++c) a.lo[c] = lower[c], a.hi[c] = upper[c];
  const unsigned long long blocks = (unsigned long long)a.tilesX * a.tilesY * (unsigned long long)n;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(hsv_lanes_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_lane_center(const uint8_t* masks, int n, int height, int width, const LaneRows& rows, int nRows,
                              int level, uint32_t* out, hipStream_t s) {
  LaneArgs a;
  a.masks = masks, a.out = out;
  a.height = height, a.width = width, a.nRows = nRows, a.level = level;
  hipLaunchKernelGGL(lane_center_kernel, dim3((unsigned)n * (unsigned)nRows), dim3(64), 0, s, a, rows);
  return hipGetLastError();
}

}  // namespace unet

namespace {

bool box_size(int k) { return k == 1 || k == 3 || k == 5 || k == 7; }

}  // namespace

extern "C" {

int unet_hsv_lanes_u8_batch(int device, const uint8_t* framesDev, int n, int height, int width, int isBgr,
                            const uint8_t* lowerHost, const uint8_t* upperHost, int closeK, int openK,
                            uint8_t* maskOutDev, void* stream) {
  const unet::OpCall op{"unet_hsv_lanes_u8_batch"};
  if (!framesDev || !lowerHost || !upperHost || !maskOutDev) return op.refuse("a null pointer");
  if (n <= 0 || height <= 0 || width <= 0) return op.refuse("n, height and width must be positive");
  if (!unet::fits_int((unsigned long long)n * height * width))
    return op.refuse("n * height * width must be smaller than 2^31");
  if (!box_size(closeK) || !box_size(openK)) return op.refuse("close_ksize and open_ksize must be 1, 3, 5 or 7");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_hsv_lanes(framesDev, n, height, width, isBgr, lowerHost, upperHost, closeK, openK, maskOutDev,
                                        (hipStream_t)stream));
}

int unet_lane_center_u8_batch(int device, const uint8_t* masksDev, int n, int height, int width, const int* rowsHost,
                              int nRows, int level, uint32_t* outDev, void* stream) {
  const unet::OpCall op{"unet_lane_center_u8_batch"};
  if (!masksDev || !rowsHost || !outDev) return op.refuse("a null pointer");
  if (n <= 0 || height <= 0 || width <= 0) return op.refuse("n, height and width must be positive");
  if (width > 65535) return op.refuse("width must be at most 65535 (the sum of x is a 32-bit integer)");
  if (nRows < 1 || nRows > UNET_LANE_ROWS_MAX) return op.refuse("n_rows must lie in 1 .. UNET_LANE_ROWS_MAX");
  if (level < 0 || level > 255) return op.refuse("level must lie in 0 .. 255");
  if (!unet::fits_int((unsigned long long)n * nRows)) return op.refuse("n * n_rows must be smaller than 2^31");
  unet::LaneRows rows;   // by value in the kernel's arguments: the caller's array is free once this returns
  memset(&rows, 0, sizeof(rows));
  for (int j = 0; j < nRows; ++j) {
    if (rowsHost[j] < 0 || rowsHost[j] >= height) return op.refuse("a scan row outside [0, height)");
    rows.r[j] = rowsHost[j];
  }
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_lane_center(masksDev, n, height, width, rows, nRows, level, outDev, (hipStream_t)stream));
}

}  // extern "C"
