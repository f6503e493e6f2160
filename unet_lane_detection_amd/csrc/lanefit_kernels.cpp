// The lane fit's kernel (lanefit_kernels.h): plain C++, integer arithmetic only.
//
// lane_fit_kernel.  One workgroup of 16 waves per frame; both lanes in it, since they share the histogram.  The waves
// with an even index work for the left lane, the odd ones for the right lane, so a thread's sums belong to one lane.
//   window mode   1. the bottom half of the frame is one run of bytes: 16-byte loads at 16-byte aligned ADDRESSES (the
//                    base pointer's alignment does not matter), single bytes where a 16-byte access would leave the
//                    run, and an LDS add per on pixel into the column histogram (at most 8192 x 4 bytes).
//                 2. first maximum of either half: a block-wide maximum of (count << 13 | 8191 - x).
//                 3. the windows in order, bottom up.  A window row of at most 2 margin columns is covered by a group
//                    of G lanes, G the power of two that holds its 16-byte chunks (16 for margin 100), so a wave takes
//                    64 / G rows a step; a lane's chunks in a step lie in one row y, so it multiplies that row's count
//                    and sum of x by y^k into its eight 64-bit sums.  One block-wide reduction of (count, sum of x) per
//                    window and lane recentres; its LDS slots alternate, so one barrier a window is enough.
//   prior mode    step 3's accumulation over all rows at once, the centre of a row taken from the table; the bounds are
//                 formed in 64 bits, so any int32 prior is safe.  Whether a row contributed is a ballot over its group.
//   both          the sums are reduced once at the end through shuffles and LDS; 32 threads write the two records with
//                 ordinary stores.  No global atomics, no scratch buffer.
// The window pass reads rows the histogram pass has touched; they come from cache (profiles/r23/lane_fit.md).
//
// Largest sum: a row gives a lane at most 2 margin <= 1024 pixels, so S_4 <= 1024 sum_{y < 2048} y^4 < 1024 * 2048^5 / 5
// = 2^65 / 5 = 0.4 * 2^64, and T_2 <= 1024 * 8191 * sum y^2 < 2^55.
//
// No argument the entry point accepts makes the kernel read or write outside its buffers: mask reads stay inside the
// frame's rows (a 16-byte load is issued only where all its bytes lie in the span asked for), prior reads at
// [frame][lane][y < height], histogram indices below width.
#include "lanefit_kernels.h"

#include "op_entry.h"
#include "wave_ops.h"


namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 1024, WAVES = THREADS / 64, SIDE_WAVES = WAVES / 2;
constexpr int SUMS = 12;   // S_0..S_4, T_0..T_2, min y, max y, tried, hit

struct FitArgs {
  const uint8_t* masks;
  const int32_t* prior;
  u64* out;
  int height, width, level, nWindows, margin, minPixels;
  int groupLog2;   // G = 1 << groupLog2 lanes cover a window row
};

// count and sum of x of the on pixels in columns [x0, x1) of a row (0 <= x0, x1 <= width), over the 16-byte chunks
// sub, sub + G, ... of the span
__device__ __forceinline__ void scan_span(const uint8_t* __restrict__ row, int x0, int x1, int level, int sub, int G,
                                          uint32_t& cnt, uint32_t& sx) {
  cnt = 0u, sx = 0u;
  if (x1 <= x0) return;
  const int mis = (int)(reinterpret_cast<uintptr_t>(row + x0) & 15u);   // the run of aligned chunks starts `mis` bytes in front
  const int nch = (mis + (x1 - x0) + 15) >> 4;
  for (int c = sub; c < nch; c += G) {
    const int xb = x0 - mis + 16 * c;   // x of the chunk's first byte; may lie in front of x0
    if (xb >= x0 && xb + 16 <= x1) {
      const uint4 v = *reinterpret_cast<const uint4*>(row + xb);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int b = 0; b < 16; ++b) {
        const uint32_t on = (int)((w[b >> 2] >> (8 * (b & 3))) & 255u) > level ? 1u : 0u;
        cnt += on, sx += on * (uint32_t)(xb + b);
      }
    } else {
      for (int b = 0; b < 16; ++b) {
        const int x = xb + b;
        if (x >= x0 && x < x1 && (int)row[x] > level) cnt += 1u, sx += (uint32_t)x;
      }
    }
  }
}

struct Moments {
  u64 s0, s1, s2, s3, s4, t0, t1, t2;
  uint32_t ymin, ymax;
};

__device__ __forceinline__ void add_row(Moments& m, uint32_t cnt, uint32_t sx, int yy) {
  if (cnt == 0u) return;
  const u64 y = (u64)yy, y2 = y * y, c = cnt, s = sx;
  m.s0 += c, m.s1 += c * y, m.s2 += c * y2, m.s3 += c * (y2 * y), m.s4 += c * (y2 * y2);
  m.t0 += s, m.t1 += s * y, m.t2 += s * y2;
  m.ymin = min(m.ymin, (uint32_t)yy), m.ymax = max(m.ymax, (uint32_t)yy);
}

__global__ __launch_bounds__(THREADS) void lane_fit_kernel(const FitArgs a) {
  __shared__ uint32_t hist[LANE_FIT_WIDTH_MAX];
  __shared__ uint32_t kred[WAVES][2];
  __shared__ u64 wred[2][WAVES][2];
  __shared__ u64 red[WAVES][SUMS];
  __shared__ uint32_t state[2][4];   // window mode, per lane: present, base, hit, last centre
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int side = wave & 1, sw = wave >> 1;   // the lane this wave works for, and its index among that lane's waves
  const int G = 1 << a.groupLog2, sub = lane & (G - 1), slot = lane >> a.groupLog2, R = 64 >> a.groupLog2;
  const int h = a.height, w = a.width;
  const int img = (int)blockIdx.x;
  const uint8_t* __restrict__ frame = a.masks + (size_t)img * h * w;
  Moments m = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, (uint32_t)h, 0u};
  uint32_t tried = 0u, hit = 0u;   // prior mode: rows of this thread's groups (counted by the group's first lane)

  if (a.prior == nullptr) {
    // ---- 1. the column histogram of rows [h / 2, h)
    for (int x = tid; x < w; x += THREADS) hist[x] = 0u;
    __syncthreads();
    {
      const uint8_t* __restrict__ p = frame + (size_t)(h / 2) * w;
      const long long B = (long long)(h - h / 2) * w;
      const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 15u);
      const int nch = (int)((mis + B + 15) >> 4);
      for (int c = tid; c < nch; c += THREADS) {
        const long long fb = 16ll * c - mis;   // offset of the chunk's first byte in the run; negative in front of it
        if (fb >= 0 && fb + 16 <= B) {
          const uint4 v = *reinterpret_cast<const uint4*>(p + fb);
          const uint32_t wd[4] = {v.x, v.y, v.z, v.w};
          int x = (int)(fb % w);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (wd[q] == 0u) {   // level >= 0: a zero byte is never on
              x += 4;
              if (x >= w) x = w > 4 ? x - w : x % w;
              continue;
            }
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if ((int)((wd[q] >> (8 * b)) & 255u) > a.level) atomicAdd(&hist[x], 1u);
              if (++x == w) x = 0;
            }
          }
        } else {
          for (int b = 0; b < 16; ++b) {
            const long long f = fb + b;
            if (f >= 0 && f < B && (int)p[f] > a.level) atomicAdd(&hist[(int)(f % w)], 1u);
          }
        }
      }
    }
    __syncthreads();
    // ---- 2. the first maximum of either half
    const int mid = w / 2;
    uint32_t key[2] = {0u, 0u};
    for (int x = tid; x < w; x += THREADS) {
      const uint32_t cnt = hist[x];
      const uint32_t k = cnt ? ((cnt << 13) | (uint32_t)(LANE_FIT_WIDTH_MAX - 1 - x)) : 0u;   // cnt <= 1024
      if (x < mid) key[0] = max(key[0], k);
      else key[1] = max(key[1], k);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      key[0] = max(key[0], (uint32_t)__shfl_xor(key[0], d, 64));
      key[1] = max(key[1], (uint32_t)__shfl_xor(key[1], d, 64));
    }
    if (lane == 0) kred[wave][0] = key[0], kred[wave][1] = key[1];
    __syncthreads();
    uint32_t best = 0u;
#pragma unroll
    for (int j = 0; j < WAVES; ++j) best = max(best, kred[j][side]);
    const bool present = best != 0u;
    const int base = present ? LANE_FIT_WIDTH_MAX - 1 - (int)(best & (uint32_t)(LANE_FIT_WIDTH_MAX - 1)) : 0;
    // ---- 3. the windows, bottom up
    int c = base;
    uint32_t whit = 0u;
    const int wh = h / a.nWindows;
    for (int i = 0; i < a.nWindows; ++i) {
      const int y0 = h - (i + 1) * wh;
      const int x0 = present ? max(c - a.margin, 0) : 0, x1 = present ? min(c + a.margin, w) : 0;
      uint32_t wcnt = 0u;
      u64 wsx = 0ull;
      for (int r0 = sw * R; r0 < wh; r0 += SIDE_WAVES * R) {
        const int r = r0 + slot;
        if (r < wh) {
          uint32_t cnt, sx;
          scan_span(frame + (size_t)(y0 + r) * w, x0, x1, a.level, sub, G, cnt, sx);
          wcnt += cnt, wsx += sx;
          add_row(m, cnt, sx, y0 + r);
        }
      }
      const u64 wc = wave_sum((u64)wcnt), ws = wave_sum(wsx);
      if (lane == 0) wred[i & 1][wave][0] = wc, wred[i & 1][wave][1] = ws;
      __syncthreads();   // the slots written two windows from now are the ones read here: one barrier a window is enough
      u64 tc = 0ull, ts = 0ull;
#pragma unroll
      for (int j = 0; j < SIDE_WAVES; ++j) tc += wred[i & 1][2 * j + side][0], ts += wred[i & 1][2 * j + side][1];
      if (tc > (u64)a.minPixels) c = (int)(ts / tc), ++whit;
    }
    if (lane == 0 && sw == 0) {
      state[side][0] = present ? 1u : 0u, state[side][1] = (uint32_t)base;
      state[side][2] = whit, state[side][3] = present ? (uint32_t)c : 0u;
    }
  } else {
    // ---- prior mode: every row on its own
    const int32_t* __restrict__ pr = a.prior + ((size_t)img * 2 + side) * h;
    const u64 gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    for (int r0 = sw * R; r0 < h; r0 += SIDE_WAVES * R) {
      const int y = r0 + slot;
      uint32_t cnt = 0u, sx = 0u;
      bool searched = false;
      if (y < h) {
        const int p = pr[y];
        if (p >= 0) {
          searched = true;
          const long long lo = max((long long)p - a.margin, 0ll), hi = min((long long)p + a.margin, (long long)w);
          if (lo < hi) scan_span(frame + (size_t)y * w, (int)lo, (int)hi, a.level, sub, G, cnt, sx);
        }
      }
      const u64 any = (__ballot(cnt > 0u) >> (slot * G)) & gmask;   // the loop is uniform over the wave
      if (sub == 0 && searched) tried += 1u, hit += any ? 1u : 0u;
      add_row(m, cnt, sx, y);
    }
  }

  // ---- the sums of the block: shuffles, then LDS
  {
    const u64 v[8] = {wave_sum(m.s0), wave_sum(m.s1), wave_sum(m.s2), wave_sum(m.s3),
                      wave_sum(m.s4), wave_sum(m.t0), wave_sum(m.t1), wave_sum(m.t2)};
    uint32_t ymin = m.ymin, ymax = m.ymax;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      ymin = min(ymin, (uint32_t)__shfl_xor(ymin, d, 64));
      ymax = max(ymax, (uint32_t)__shfl_xor(ymax, d, 64));
    }
    const u64 tr = wave_sum((u64)tried), ht = wave_sum((u64)hit);
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) red[wave][k] = v[k];
      red[wave][8] = ymin, red[wave][9] = ymax, red[wave][10] = tr, red[wave][11] = ht;
    }
  }
  __syncthreads();
  if (tid < 2 * LANE_FIT_WORDS) {
    const int s = tid >> 4, k = tid & 15;
    // the one entry of `red` this word is made from: a moment sum, min y (8), max y (9), tried (10) or hit (11)
    const int q = (k >= 5 && k <= 12) ? k - 5 : k == 13 ? 8 : k == 14 ? 9 : k == 2 ? 11 : 10;
    u64 acc = q == 8 ? (u64)h : 0ull;
    for (int j = 0; j < SIDE_WAVES; ++j) {
      const u64 r = red[2 * j + s][q];
      acc = q == 8 ? min(acc, r) : q == 9 ? max(acc, r) : acc + r;
    }
    const bool window = a.prior == nullptr;
    u64 val = acc;                                                                   // [5] .. [14]; prior mode: hit, tried
    if (k == 0) val = window ? (u64)state[s][0] : (acc != 0ull ? 1ull : 0ull);
    else if (k == 1) val = window ? (u64)state[s][1] : 0ull;
    else if (k == 2 && window) val = state[s][2];
    else if (k == 3 && window) val = state[s][0] ? (u64)a.nWindows : 0ull;
    else if (k == 4) val = window ? (u64)state[s][3] : 0ull;
    else if (k == 15) val = 0ull;
    a.out[((size_t)img * 2 + s) * LANE_FIT_WORDS + k] = val;
  }
}

}  // namespace

hipError_t launch_lane_fit(const uint8_t* masks, int n, int height, int width, int level, int nWindows, int margin,
                           int minPixels, const int32_t* prior, unsigned long long* out, hipStream_t s) {
  FitArgs a;
  a.masks = masks, a.prior = prior, a.out = out;
  a.height = height, a.width = width, a.level = level, a.nWindows = nWindows, a.margin = margin, a.minPixels = minPixels;
  const int chunks = (2 * margin + 30) / 16;   // 16-byte chunks that cover 2 margin bytes at any alignment
  a.groupLog2 = 0;
  while (a.groupLog2 < 6 && (1 << a.groupLog2) < chunks) ++a.groupLog2;
  hipLaunchKernelGGL(lane_fit_kernel, dim3((unsigned)n), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

int unet_lane_fit_u8_batch(int device, const uint8_t* masksDev, int n, int height, int width, int level, int nWindows,
                           int margin, int minPixels, const int32_t* priorDev, unsigned long long* outDev, void* stream) {
  const unet::OpCall op{"unet_lane_fit_u8_batch"};
  if (!masksDev || !outDev) return op.refuse("a null pointer");
  if (n <= 0) return op.refuse("n must be positive");
  if (height < 1 || height > unet::LANE_FIT_HEIGHT_MAX) return op.refuse("height must lie in 1 .. 2048");
  if (width < 1 || width > unet::LANE_FIT_WIDTH_MAX) return op.refuse("width must lie in 1 .. 8192");
  if (!unet::fits_int((unsigned long long)n * height * width))
    return op.refuse("n * height * width must be smaller than 2^31");
  if (level < 0 || level > 255) return op.refuse("level must lie in 0 .. 255");
  if (nWindows < 1 || nWindows > UNET_LANE_FIT_WINDOWS_MAX || nWindows > height)
    return op.refuse("n_windows must lie in 1 .. min(height, UNET_LANE_FIT_WINDOWS_MAX)");
  if (margin < 1 || margin > unet::LANE_FIT_MARGIN_MAX) return op.refuse("margin must lie in 1 .. 512");
  if (minPixels < 0) return op.refuse("min_pixels must not be negative");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_lane_fit(masksDev, n, height, width, level, nWindows, margin, minPixels, priorDev, outDev,
                                       (hipStream_t)stream));
}

}  // extern "C"
