// The kernels of the frame correction (correct_kernels.h): plain C++, integer arithmetic, no device math library.
//
// init_kernel       zeroes the channel and tile histograms and writes identity tile tables, so that every region of
//                   the work buffer is written by every call and the histogram kernels can add into it.
// hist_kernel       a block takes HIST_ROWS rows of one frame: wave w the rows w, w + 4, ..., a lane every 64th pixel
//                   of a row (three byte loads a pixel: a wave reads 192 consecutive bytes a step; padding is never
//                   addressed).  Each wave counts into 3 x 256 32-bit LDS counters of its own; the four copies are
//                   merged and the non-zero sums added to the frame's histograms with one global atomic each.
// plan_kernel       one block a frame, thread v owns level v: channel sums, gate, gains, the pooled histogram of the
//                   balanced samples (64-bit LDS atomics), its prefix sums (a doubling scan), lo and hi, the channel
//                   tables, the plan words.
// tile_hist_kernel  a block takes TILE_ROWS rows of one tile: the gray value of the corrected pixel, counted as in
//                   hist_kernel.  A frame whose plan does not ask for CLAHE (gated, or CLAHE off) ends the block at once.
// tile_lut_kernel   one block a tile, thread v owns bin v: clip, redistribute, residual, prefix sums, table.
// apply_kernel      a block takes APPLY_ROWS rows of one frame and stages the channel tables and the tile tables these
//                   rows can touch (at most APPLY_ROWS + 1 tile rows of at most 16 tables: 36 KB) in LDS.  A thread
//                   takes 16 pixels (48 bytes) at a time: where the frames' and the output's base and stride are
//                   multiples of 16 these are three 16-byte loads and three 16-byte stores, otherwise - and for the
//                   last, partial group of a row - bytes.  Both paths run the same per-pixel code.  A thread reads
//                   its pixels before it writes them and no thread reads another's, so out == frames is safe.
//
// Exact quotients: the blend's numerator is below 2^38, its quotient at most 255: a double reciprocal and one
// correction step; the channel scaling's numerator is below 2^17: an fp32 reciprocal and one correction step.  The
// corrections make both the integer quotient whatever the reciprocal's last bit is.
//
// No argument the entry point accepts makes a kernel read or write outside its buffers; padding is neither read as
// pixels nor written.
#include "correct_kernels.h"

#include "op_entry.h"
#include "wave_ops.h"

#include <cstring>

namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int HIST_ROWS = 16, TILE_ROWS = 16, APPLY_ROWS = 8;
constexpr int GRID_MAX = 16;
constexpr uint32_t FLAG_CORRECTED = 1u, FLAG_STRETCH = 2u, FLAG_CLAHE = 4u;
constexpr uint32_t UNITY = 65536u;

struct Geo {
  const uint8_t* frames;
  uint8_t* out;
  uint8_t* work;
  int n, height, width;
  long long stride, ostride;
  int swap, gx, gy, th, tw;
  size_t frameBytes, tlutOff;
};

struct PlanCfg {
  int whiteBalance, maxGain, loBp, hiBp, clahe, onlyFlagged, darkLimit, brightLimit;
  uint8_t tone[256];
};

__device__ __forceinline__ uint32_t gray8(uint32_t c0, uint32_t c1, uint32_t c2, int swap) {
  const uint32_t b = swap ? c0 : c2, r = swap ? c2 : c0;
  return (3735u * b + 19235u * c1 + 9798u * r + 16384u) >> 15;
}

// ---- init -----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void init_kernel(const Geo g) {
  const size_t words = g.frameBytes / 4, tlutWord = g.tlutOff / 4;
  const size_t i = (size_t)blockIdx.y * THREADS + threadIdx.x;
  if (i >= words) return;
  uint32_t* frame = reinterpret_cast<uint32_t*>(g.work + (size_t)blockIdx.x * g.frameBytes);
  if (i < CORRECT_PLAN_OFF / 4 || (i >= CORRECT_THIST_OFF / 4 && i < tlutWord))
    frame[i] = 0u;
  else if (i >= tlutWord)
    frame[i] = 0x03020100u + 0x04040404u * (uint32_t)((i - tlutWord) & 63u);   // bytes 4k .. 4k + 3 of the identity
}

// ---- channel histograms ---------------------------------------------------------------------------------------------

// the block's per-wave counters, merged, into dst[0 .. bins)
template <int BINS>
__device__ __forceinline__ void merge_counters(uint32_t (*sub)[BINS], uint32_t* dst) {
  __syncthreads();
  for (int i = threadIdx.x; i < BINS; i += THREADS) {
    uint32_t s = 0u;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += sub[w][i];
    if (s) atomicAdd(dst + i, s);
  }
}

__global__ __launch_bounds__(THREADS) void hist_kernel(const Geo g) {
  __shared__ uint32_t sub[WAVES][768];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < WAVES * 768; i += THREADS) (&sub[0][0])[i] = 0u;
  __syncthreads();
  const int img = blockIdx.x, y0 = blockIdx.y * HIST_ROWS, y1 = min(y0 + HIST_ROWS, g.height);
  for (int y = y0 + wave; y < y1; y += WAVES) {
    const uint8_t* __restrict__ row = g.frames + ((long long)img * g.height + y) * g.stride;
    for (int x = lane; x < g.width; x += 64) {
      const uint8_t* px = row + 3 * x;
      atomicAdd(&sub[wave][px[0]], 1u);
      atomicAdd(&sub[wave][256 + px[1]], 1u);
      atomicAdd(&sub[wave][512 + px[2]], 1u);
    }
  }
  merge_counters<768>(sub, reinterpret_cast<uint32_t*>(g.work + (size_t)img * g.frameBytes + CORRECT_HIST_OFF));
}

// ---- plan -----------------------------------------------------------------------------------------------------------

// inclusive prefix sums over the block's 256 values, thread v's returned; buf is 2 x 256
__device__ __forceinline__ u64 block_scan(u64 v, u64 (*buf)[THREADS]) {
  const int t = threadIdx.x;
  int src = 0;
  buf[0][t] = v;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    buf[src ^ 1][t] = buf[src][t] + (t >= d ? buf[src][t - d] : 0ull);
    src ^= 1;
    __syncthreads();
  }
  const u64 r = buf[src][t];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(THREADS) void plan_kernel(const Geo g, const PlanCfg cfg) {
  __shared__ u64 red[WAVES][3];
  __shared__ u64 pool[THREADS];
  __shared__ u64 scan[2][THREADS];
  __shared__ int lohi[2];
  const int v = threadIdx.x, wave = v >> 6, lane = v & 63, img = blockIdx.x;
  uint8_t* frame = g.work + (size_t)img * g.frameBytes;
  const uint32_t* hist = reinterpret_cast<const uint32_t*>(frame + CORRECT_HIST_OFF);
  uint32_t h[3];
  u64 part[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    h[c] = hist[256 * c + v];
    part[c] = (u64)h[c] * (u64)v;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) part[c] += shfl_xor64(part[c], d);
    if (lane == 0) red[wave][c] = part[c];
  }
  pool[v] = 0ull;
  __syncthreads();
  u64 sc[3], s = 0ull;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sc[c] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
    s += sc[c];
  }
  const u64 samples = 3ull * (u64)g.height * (u64)g.width;   // 3 N < 3 * 2^31
  uint32_t* plan = reinterpret_cast<uint32_t*>(frame + CORRECT_PLAN_OFF);
  uint8_t* lut = frame + CORRECT_LUT_OFF;
  if (cfg.onlyFlagged && (u64)cfg.darkLimit * samples <= s && s <= (u64)cfg.brightLimit * samples) {   // uniform
    lut[v] = lut[256 + v] = lut[512 + v] = (uint8_t)v;
    if (v == 0) {
      plan[0] = 0u, plan[1] = plan[2] = plan[3] = UNITY, plan[4] = 0u, plan[5] = 255u;
      plan[6] = (uint32_t)s, plan[7] = (uint32_t)(s >> 32);
    }
    return;
  }
  uint32_t gain[3], a[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    gain[c] = UNITY;
    if (cfg.whiteBalance && sc[c] != 0ull) {
      const u64 q = (s << 16) / (3ull * sc[c]);   // s < 2^41
      const u64 lo = UNITY / (uint32_t)cfg.maxGain, hi = (u64)UNITY * (uint32_t)cfg.maxGain;
      gain[c] = (uint32_t)(q < lo ? lo : (q > hi ? hi : q));
    }
    a[c] = min(255u, (uint32_t)(((u64)v * gain[c] + 32768ull) >> 16));
  }
  uint32_t flags = FLAG_CORRECTED | (cfg.clahe ? FLAG_CLAHE : 0u);
  int lo = 0, hi = 255;
  const bool stretch = cfg.loBp != 0 || cfg.hiBp != 0;   // uniform
  if (stretch) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (h[c]) atomicAdd(&pool[a[c]], (u64)h[c]);
    __syncthreads();
    const u64 cum = block_scan(pool[v], scan);
    scan[0][v] = cum;
    __syncthreads();
    const u64 below = v ? scan[0][v - 1] : 0ull;
    const u64 loT = (u64)cfg.loBp * samples / 10000ull, hiT = samples - (u64)cfg.hiBp * samples / 10000ull;
    if (cum > loT && !(v && below > loT)) lohi[0] = v;
    if (cum >= hiT && !(v && below >= hiT)) lohi[1] = v;
    __syncthreads();
    lo = lohi[0], hi = lohi[1];
    if (hi > lo) flags |= FLAG_STRETCH;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t u = a[c];
    if (flags & FLAG_STRETCH) {
      const uint32_t d = (uint32_t)(hi - lo);
      u = (int)u < lo ? 0u : min(255u, ((u - (uint32_t)lo) * 255u + d / 2u) / d);
    }
    lut[256 * c + v] = cfg.tone[u];
  }
  if (v == 0) {
    plan[0] = flags, plan[1] = gain[0], plan[2] = gain[1], plan[3] = gain[2];
    plan[4] = (uint32_t)lo, plan[5] = (uint32_t)hi;
    plan[6] = (uint32_t)s, plan[7] = (uint32_t)(s >> 32);
  }
}

// ---- tile histograms ------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void tile_hist_kernel(const Geo g, int bands) {
  __shared__ uint32_t sub[WAVES][256];
  __shared__ uint8_t lut[768];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tiles = g.gx * g.gy;
  const unsigned perImg = (unsigned)tiles * (unsigned)bands;
  const int img = (int)(blockIdx.x / perImg);
  const unsigned rest = blockIdx.x - (unsigned)img * perImg;
  const int tile = (int)(rest / (unsigned)bands), band = (int)(rest - (unsigned)tile * bands);
  uint8_t* frame = g.work + (size_t)img * g.frameBytes;
  if (!(reinterpret_cast<const uint32_t*>(frame + CORRECT_PLAN_OFF)[0] & FLAG_CLAHE)) return;   // uniform
  const int ty = tile / g.gx, tx = tile - ty * g.gx;
  const int y0 = ty * g.th + band * TILE_ROWS;
  const int yEnd = min(min((ty + 1) * g.th, g.height), y0 + TILE_ROWS);
  if (y0 >= yEnd) return;   // uniform: a border tile with fewer bands
  const int x0 = tx * g.tw, x1 = min(x0 + g.tw, g.width);
  for (int i = tid; i < WAVES * 256; i += THREADS) (&sub[0][0])[i] = 0u;
  for (int i = tid; i < 768; i += THREADS) lut[i] = frame[CORRECT_LUT_OFF + i];
  __syncthreads();
  for (int y = y0 + wave; y < yEnd; y += WAVES) {
    const uint8_t* __restrict__ row = g.frames + ((long long)img * g.height + y) * g.stride;
    for (int x = x0 + lane; x < x1; x += 64) {
      const uint8_t* px = row + 3 * x;
      atomicAdd(&sub[wave][gray8(lut[px[0]], lut[256 + px[1]], lut[512 + px[2]], g.swap)], 1u);
    }
  }
  merge_counters<256>(sub, reinterpret_cast<uint32_t*>(frame + CORRECT_THIST_OFF) + 256 * tile);
}

// ---- tile tables ----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(THREADS) void tile_lut_kernel(const Geo g, int clipQ8) {
  __shared__ u64 scan[2][THREADS];
  __shared__ uint32_t red[WAVES];
  const int v = threadIdx.x, wave = v >> 6, lane = v & 63;
  const int tiles = g.gx * g.gy;
  const int img = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x - (unsigned)img * tiles);
  uint8_t* frame = g.work + (size_t)img * g.frameBytes;
  if (!(reinterpret_cast<const uint32_t*>(frame + CORRECT_PLAN_OFF)[0] & FLAG_CLAHE)) return;   // the identity stays
  const int ty = tile / g.gx, tx = tile - ty * g.gx;
  const uint32_t area = (uint32_t)(min(g.th, g.height - ty * g.th) * min(g.tw, g.width - tx * g.tw));   // <= 2^28
  uint32_t h = reinterpret_cast<const uint32_t*>(frame + CORRECT_THIST_OFF)[256 * tile + v];
  const uint32_t limit = max(1u, (uint32_t)min(((u64)(uint32_t)clipQ8 * area) >> 16, (u64)area));   // no bin is above area
  uint32_t over = h > limit ? h - limit : 0u;
  h = min(h, limit);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) over += __shfl_xor(over, d, 64);
  if (lane == 0) red[wave] = over;
  __syncthreads();
  const uint32_t excess = red[0] + red[1] + red[2] + red[3];   // <= area
  h += excess >> 8;
  const uint32_t r = excess & 255u;
  if (r) {
    const uint32_t step = max(256u / r, 1u);
    if ((uint32_t)v % step == 0u && (uint32_t)v / step < r) h += 1u;   // i = 0, step, 2 step, ...: the first r of them
  }
  const u64 cdf = block_scan((u64)h, scan);
  frame[g.tlutOff + 256 * (size_t)tile + v] = (uint8_t)((255ull * cdf + area / 2u) / area);
}

// ---- apply ----------------------------------------------------------------------------------------------------------

struct RowCtx {
  int r0, r1;    // the staged tables' first index of tile rows ty0 and ty1
  uint32_t wy;
};

// exact floor(num / den) for num < 2^38 and a quotient below 2^16, rden = 1.0 / den
__device__ __forceinline__ uint32_t div_wide(u64 num, uint32_t den, double rden) {
  uint32_t q = (uint32_t)((double)num * rden);
  const long long r = (long long)num - (long long)q * (long long)den;
  if (r < 0) --q;
  else if (r >= (long long)den) ++q;
  return q;
}

// exact floor(num / den) for num < 2^17, 1 <= den <= 255
__device__ __forceinline__ uint32_t div_small(uint32_t num, uint32_t den, float rden) {
  uint32_t q = (uint32_t)((float)num * rden);
  const int r = (int)num - (int)(q * den);
  if (r < 0) --q;
  else if (r >= (int)den) ++q;
  return q;
}

struct ColCtx {
  int tx0;       // floor(X / (2 tw)), -1 .. gx - 1
  uint32_t wx;   // X - tx0 * 2 tw
};

__device__ __forceinline__ void correct_pixel(const Geo& g, const uint8_t* lut, const uint8_t* tl, bool clahe,
                                              const RowCtx& rc, ColCtx& cc, double rden, uint32_t& c0, uint32_t& c1,
                                              uint32_t& c2) {
  c0 = lut[c0], c1 = lut[256 + c1], c2 = lut[512 + c2];
  if (!clahe) return;
  const uint32_t y = gray8(c0, c1, c2, g.swap);
  const uint32_t tw2 = 2u * (uint32_t)g.tw, th2 = 2u * (uint32_t)g.th;
  const int t0 = max(cc.tx0, 0), t1 = min(cc.tx0 + 1, g.gx - 1);
  const uint32_t t00 = tl[(rc.r0 + t0) * 256 + y], t01 = tl[(rc.r0 + t1) * 256 + y];
  const uint32_t t10 = tl[(rc.r1 + t0) * 256 + y], t11 = tl[(rc.r1 + t1) * 256 + y];
  const uint32_t top = (tw2 - cc.wx) * t00 + cc.wx * t01, bot = (tw2 - cc.wx) * t10 + cc.wx * t11;   // < 2^23
  const u64 num = (u64)(th2 - rc.wy) * top + (u64)rc.wy * bot + (u64)g.tw * th2;
  const uint32_t y2 = div_wide(num, tw2 * th2, rden);   // 4 tw th <= 2^30
  if (y == 0u) {
    c0 = c1 = c2 = y2;
  } else {
    const float ry = __fdividef(1.0f, (float)y);
    c0 = min(255u, div_small(c0 * y2 + y / 2u, y, ry));
    c1 = min(255u, div_small(c1 * y2 + y / 2u, y, ry));
    c2 = min(255u, div_small(c2 * y2 + y / 2u, y, ry));
  }
  // the next column
  cc.wx += 2u;
  if (cc.wx >= tw2) cc.wx -= tw2, ++cc.tx0;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void apply_kernel(const Geo g) {
  __shared__ uint8_t lut[768];
  __shared__ uint32_t tlw[(APPLY_ROWS + 1) * GRID_MAX * 64];   // up to 9 tile rows of 16 tables of 256 bytes
  const int tid = threadIdx.x;
  const int img = blockIdx.x, y0 = blockIdx.y * APPLY_ROWS, yLast = min(y0 + APPLY_ROWS, g.height) - 1;
  const uint8_t* frame = g.work + (size_t)img * g.frameBytes;
  const bool clahe = (reinterpret_cast<const uint32_t*>(frame + CORRECT_PLAN_OFF)[0] & FLAG_CLAHE) != 0u;   // uniform
  const int th2 = 2 * g.th, tw2 = 2 * g.tw;
  // floor((2 y + 1 - th) / (2 th)): the numerator is above -2 th
  auto tile_row = [&](int y) { const int v = 2 * y + 1 - g.th; return v < 0 ? -1 : v / th2; };
  const int tyA = max(tile_row(y0), 0);
  int tyB = min(tile_row(yLast) + 1, g.gy - 1);
  tyB = min(tyB, tyA + APPLY_ROWS);   // never cuts: rows y0 .. y0 + 7 touch at most 9 tile rows
  for (int i = tid; i < 768; i += THREADS) lut[i] = frame[CORRECT_LUT_OFF + i];
  if (clahe) {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(frame + g.tlutOff) + (size_t)tyA * g.gx * 64;
    const int words = (tyB - tyA + 1) * g.gx * 64;
    for (int i = tid; i < words; i += THREADS) tlw[i] = src[i];
  }
  __syncthreads();
  const uint8_t* tl = reinterpret_cast<const uint8_t*>(tlw);
  const double rden = 1.0 / ((double)tw2 * (double)th2);
  const int groups = (g.width + 15) >> 4, rows = yLast - y0 + 1;
  for (int t = tid; t < rows * groups; t += THREADS) {
    const int r = t / groups, grp = t - r * groups, y = y0 + r, x0 = grp * 16, cnt = min(16, g.width - x0);
    RowCtx rc;
    {
      const int ty0 = tile_row(y);
      rc.wy = (uint32_t)(2 * y + 1 - g.th - ty0 * th2);
      rc.r0 = (max(ty0, 0) - tyA) * g.gx;
      rc.r1 = (min(ty0 + 1, g.gy - 1) - tyA) * g.gx;
    }
    ColCtx cc;
    {
      const int v = 2 * x0 + 1 - g.tw;
      cc.tx0 = v < 0 ? -1 : v / tw2;
      cc.wx = (uint32_t)(v - cc.tx0 * tw2);
    }
    const long long rowIdx = (long long)img * g.height + y;
    const uint8_t* src = g.frames + rowIdx * g.stride + 3ll * x0;
    uint8_t* dst = g.out + rowIdx * g.ostride + 3ll * x0;
    if (VEC && cnt == 16) {
      uint32_t w[12];
      {
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        const uint4 a = s4[0], b = s4[1], c = s4[2];
        w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w, w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
        w[8] = c.x, w[9] = c.y, w[10] = c.z, w[11] = c.w;
      }
      uint32_t o[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
      for (int p = 0; p < 16; ++p) {
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (w[(3 * p + k) >> 2] >> (8 * ((3 * p + k) & 3))) & 255u;
        correct_pixel(g, lut, tl, clahe, rc, cc, rden, c[0], c[1], c[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) o[(3 * p + k) >> 2] |= c[k] << (8 * ((3 * p + k) & 3));
      }
      uint4* d4 = reinterpret_cast<uint4*>(dst);
      d4[0] = make_uint4(o[0], o[1], o[2], o[3]);
      d4[1] = make_uint4(o[4], o[5], o[6], o[7]);
      d4[2] = make_uint4(o[8], o[9], o[10], o[11]);
    } else {
      for (int p = 0; p < cnt; ++p) {
        uint32_t c0 = src[3 * p], c1 = src[3 * p + 1], c2 = src[3 * p + 2];
        correct_pixel(g, lut, tl, clahe, rc, cc, rden, c0, c1, c2);
        dst[3 * p] = (uint8_t)c0, dst[3 * p + 1] = (uint8_t)c1, dst[3 * p + 2] = (uint8_t)c2;
      }
    }
  }
}

}  // namespace

hipError_t launch_correct(const CorrectParams& p, hipStream_t s) {
  Geo g;
  g.frames = p.frames, g.out = p.out, g.work = p.work;
  g.n = p.n, g.height = p.height, g.width = p.width;
  g.stride = p.stride, g.ostride = p.ostride;
  g.swap = p.swap ? 1 : 0;
  g.gx = p.gx, g.gy = p.gy;
  g.th = (p.height + p.gy - 1) / p.gy, g.tw = (p.width + p.gx - 1) / p.gx;
  const int tiles = p.gx * p.gy;
  g.frameBytes = correct_frame_bytes(tiles), g.tlutOff = correct_tlut_off(tiles);

  const unsigned words = (unsigned)(g.frameBytes / 4);
  hipLaunchKernelGGL(init_kernel, dim3((unsigned)p.n, (words + THREADS - 1) / THREADS), dim3(THREADS), 0, s, g);
  hipLaunchKernelGGL(hist_kernel, dim3((unsigned)p.n, (unsigned)((p.height + HIST_ROWS - 1) / HIST_ROWS)), dim3(THREADS),
                     0, s, g);
  PlanCfg cfg;
  cfg.whiteBalance = p.whiteBalance, cfg.maxGain = p.maxGain, cfg.loBp = p.loBp, cfg.hiBp = p.hiBp;
  cfg.clahe = p.clahe, cfg.onlyFlagged = p.onlyFlagged, cfg.darkLimit = p.darkLimit, cfg.brightLimit = p.brightLimit;
  memcpy(cfg.tone, p.tone, 256);
  hipLaunchKernelGGL(plan_kernel, dim3((unsigned)p.n), dim3(THREADS), 0, s, g, cfg);
  if (p.clahe) {
    const int bands = (g.th + TILE_ROWS - 1) / TILE_ROWS;
    const u64 blocks = (u64)p.n * tiles * bands;   // n * 256 * 1024 at the most
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_hist_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, g, bands);
    hipLaunchKernelGGL(tile_lut_kernel, dim3((unsigned)(p.n * tiles)), dim3(THREADS), 0, s, g, p.clipQ8);
  }
  const bool vec = ((reinterpret_cast<uintptr_t>(p.frames) | reinterpret_cast<uintptr_t>(p.out) | (uintptr_t)p.stride |
                     (uintptr_t)p.ostride) & 15u) == 0u;
  const dim3 grid((unsigned)p.n, (unsigned)((p.height + APPLY_ROWS - 1) / APPLY_ROWS));
  if (vec)
    hipLaunchKernelGGL(apply_kernel<true>, grid, dim3(THREADS), 0, s, g);
  else
    hipLaunchKernelGGL(apply_kernel<false>, grid, dim3(THREADS), 0, s, g);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

size_t unet_correct_config_bytes(void) { return sizeof(unet_correct_config); }

size_t unet_correct_work_bytes(int n, int gridX, int gridY) {
  if (n <= 0 || gridX < 1 || gridX > 16 || gridY < 1 || gridY > 16) return 0;
  return (size_t)n * unet::correct_frame_bytes(gridX * gridY);
}

int unet_correct_u8_batch(int device, const uint8_t* framesDev, int n, int height, int width, int rowStride, int isBgr,
                          const unet_correct_config* cfg, uint8_t* outDev, int outRowStride, void* workDev,
                          size_t workBytes, void* stream) {
  const unet::OpCall op{"unet_correct_u8_batch"};
  if (!framesDev || !cfg || !outDev || !workDev) return op.refuse("a null pointer");
  if (n <= 0 || height <= 0 || width <= 0) return op.refuse("n, height and width must be positive");
  if (height > 16384 || width > 16384) return op.refuse("height and width must be at most 16384");
  if (!unet::fits_int((unsigned long long)n * height * width))
    return op.refuse("n * height * width must be smaller than 2^31");
  if (rowStride != 0 && (long long)rowStride < 3ll * width)
    return op.refuse("row_stride must be 0 (dense) or at least 3 * width");
  if (outRowStride != 0 && (long long)outRowStride < 3ll * width)
    return op.refuse("out_row_stride must be 0 (dense) or at least 3 * width");
  const long long stride = rowStride ? (long long)rowStride : 3ll * width;
  const long long ostride = outRowStride ? (long long)outRowStride : 3ll * width;
  if (cfg->grid_x < 1 || cfg->grid_x > 16 || cfg->grid_y < 1 || cfg->grid_y > 16)
    return op.refuse("grid_x and grid_y must be 1 .. 16");
  const int th = (height + cfg->grid_y - 1) / cfg->grid_y, tw = (width + cfg->grid_x - 1) / cfg->grid_x;
  if ((long long)(cfg->grid_y - 1) * th >= height || (long long)(cfg->grid_x - 1) * tw >= width)
    return op.refuse("the grid leaves a tile empty");
  if (cfg->white_balance != 0 && cfg->white_balance != 1) return op.refuse("white_balance must be 0 or 1");
  if (cfg->max_gain < 1 || cfg->max_gain > 8) return op.refuse("max_gain must be 1 .. 8");
  if (cfg->lo_bp < 0 || cfg->hi_bp < 0 || (long long)cfg->lo_bp + cfg->hi_bp >= 10000)
    return op.refuse("lo_bp and hi_bp must not be negative and must sum to less than 10000");
  if (cfg->clip_q8 < 1 || cfg->clip_q8 > (1 << 24)) return op.refuse("clip_q8 must be 1 .. 2^24");
  if (cfg->dark_limit < 0 || cfg->bright_limit > 255 || cfg->dark_limit > cfg->bright_limit)
    return op.refuse("0 <= dark_limit <= bright_limit <= 255");
  if (unet::misaligned(workDev, 4)) return op.refuse("work_dev must be 4-byte aligned");
  if (workBytes < unet_correct_work_bytes(n, cfg->grid_x, cfg->grid_y))
    return op.refuse("work_bytes is smaller than unet_correct_work_bytes(n, grid_x, grid_y)");
  if (outDev == framesDev) {
    if (stride != ostride) return op.refuse("in place (out_dev == frames_dev) needs equal strides");
  } else {
    // two buffers must not overlap: an overlapping output would be read as input by another block
    const long long inBytes = ((long long)n * height - 1) * stride + 3ll * width;
    const long long outBytes = ((long long)n * height - 1) * ostride + 3ll * width;
    const uintptr_t a = reinterpret_cast<uintptr_t>(framesDev), b = reinterpret_cast<uintptr_t>(outDev);
    if (a < b + (uintptr_t)outBytes && b < a + (uintptr_t)inBytes) return op.refuse("out_dev overlaps frames_dev");
  }
  if (int rc = op.on(device)) return rc;
  unet::CorrectParams p;
  p.frames = framesDev, p.out = outDev, p.work = static_cast<uint8_t*>(workDev);
  p.n = n, p.height = height, p.width = width, p.stride = stride, p.ostride = ostride;
  p.swap = isBgr ? 1 : 0;
  p.gx = cfg->grid_x, p.gy = cfg->grid_y;
  p.whiteBalance = cfg->white_balance, p.maxGain = cfg->max_gain, p.loBp = cfg->lo_bp, p.hiBp = cfg->hi_bp;
  p.clahe = cfg->clahe ? 1 : 0, p.clipQ8 = cfg->clip_q8, p.onlyFlagged = cfg->only_flagged ? 1 : 0;
  p.darkLimit = cfg->dark_limit, p.brightLimit = cfg->bright_limit;
  memcpy(p.tone, cfg->tone, 256);
  return op.done(unet::launch_correct(p, (hipStream_t)stream));
}

}  // extern "C"
