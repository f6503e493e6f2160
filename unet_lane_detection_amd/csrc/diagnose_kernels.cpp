// The two diagnostics kernels (diagnose_kernels.h): plain C++, integer arithmetic only, read-once reductions.
//
// frame_stats_kernel.  A block owns a tile of TW = 254 columns by TR = 32 rows of one frame and keeps the gray values
// of the tile plus one halo column and row on every side in LDS (RW = 256 columns by TR + 2 rows of bytes).  The
// frame's bytes come through LDS as in follow_kernels.cpp: a wave covers the up to 768 bytes of its region row with
// 16-byte loads at 16-byte aligned ADDRESSES (so neither the base pointer's alignment nor the row stride matters), the
// first and last chunk of the whole buffer byte by byte where a 16-byte access would leave it, and every lane then
// picks its pixels' three bytes out of LDS; the next two rows' loads are in flight meanwhile, and since a staging row
// belongs to one wave the waves of a block do not wait for each other until the gray plane is complete.  The padding
// between a row's pixels and the next row may be loaded with a chunk, but no lane ever picks a byte of it.  Only a
// block near the buffer's ends can meet a chunk that leaves it; every other block runs a copy of the loop that loads
// without looking, one load a step, so that its waits are counted.  Minimum, maximum and sum are taken over the tile's
// own pixels while the gray values are written.  Then thread c walks down column c of the tile with the rows above, at
// and below in registers; neighbours outside the image are the reflect-101 ones, all of which lie inside the region
// (reflect(-1) = 1, reflect(w) = w - 2, and the pixel itself where that dimension is 1).
// Sums: a thread adds at most 32 squares of at most 1020^2 and a wave at most 2048 of them, which 32 bits hold
// (4128 would); beyond the wave everything is 64 bits.  Wave shuffle, LDS across the four waves, then one 64-bit
// atomic per word and block on a record that stats_init_kernel, enqueued in front, has set to (255, 0, 0, ...).
//
// prob_stats_kernel.  A frame's floats are cut into runs of 16-byte chunks at aligned addresses, one run per block;
// whole chunks are one 16-byte load, the chunks at a frame's ends are read float by float.  Floats are ordered through
// the usual monotone key (sign bit flipped for positive values, all bits for negative ones), under which -0.0 sorts
// below +0.0 and which NaNs never enter.  floor(clamp(s, 0, 1) * 2^32): the product is exact in fp32 and below 2^32
// for s < 1, so a truncating conversion to 32 bits gives it; values >= 1 are counted and enter as 2^32 each.  Per
// block: one compare-and-swap loop on word 0 (both halves at once) and one 64-bit add on each of the other three.
//
// No argument the entry points accept makes either kernel read or write outside its buffers.
#include "diagnose_kernels.h"

#include "op_entry.h"
#include "wave_ops.h"

#include <cmath>
#include <cstring>

namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int RW = 256, TW = RW - 2;              // region columns; the tile's own
constexpr int TR = 32, ROWS = TR + 2;             // the tile's rows; the region's
constexpr int STAGE_PITCH = 64;                   // uint4 per staged row, one a lane; 49 of them are used at the most

struct FrameArgs {
  const uint8_t* frames;
  u64* out;
  int n, height, width;
  long long stride, total;   // bytes from row to row; bytes from the first pixel to the end of the last
  int tilesX, tilesY;
  int swap;                  // frames are BGR
};

// the bytes of columns [cx0, cx1) of row y of image `img` as a run of 16-byte chunks at aligned addresses
struct RowSpan {
  long long o0;   // offset of the first chunk from the frames' base (-15 at the least)
  int off, nch;   // offset of the first byte in the run; number of chunks
};

__device__ __forceinline__ RowSpan row_span(const FrameArgs& a, int img, int y, int cx0, int cx1) {
  const long long sb = ((long long)img * a.height + y) * a.stride + 3ll * cx0;
  RowSpan r;
  r.off = (int)((reinterpret_cast<uintptr_t>(a.frames) + (uintptr_t)sb) & 15u);
  r.o0 = sb - r.off;
  r.nch = (r.off + (cx1 - cx0) * 3 + 15) >> 4;   // <= 49
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

// cv2's BORDER_REFLECT_101 for an index one step outside [0, n); the pixel itself where n is 1
__device__ __forceinline__ int reflect101(int i, int n) {
  if (n == 1) return 0;
  return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i);
}

__global__ __launch_bounds__(THREADS) void stats_init_kernel(u64* out, size_t words, int recWords, u64 first) {
  const size_t i = (size_t)blockIdx.x * THREADS + threadIdx.x;
  if (i < words) out[i] = (i % (size_t)recWords == 0) ? first : 0ull;
}

// a block's tile: image, first column and row of the region, the tile's columns and rows, the region's rows, the
// region's columns inside the image
struct Tile {
  int img, gx0, gy0, len, th, rows, cx0, cx1;
};

// The gray plane of a block's region into G, and minimum, maximum and sum of the tile's own bytes: wave w takes region
// rows w, w + 4, ...  EDGE: a chunk may leave the buffer (load_chunk); without it every chunk is one aligned load and
// nothing else is loaded inside the loop, so that the loads of the two rows ahead stay in flight.
template <bool EDGE>
__device__ __forceinline__ void gray_plane(const FrameArgs& a, const Tile& t, uint4 (*stage)[WAVES][STAGE_PITCH],
                                           uint8_t (*G)[RW], uint32_t& mn, uint32_t& mx, uint32_t& sum) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int groups = (t.rows + WAVES - 1) / WAVES;
  // this lane's chunk of region row ry, zeros where there is none
  auto fetch = [&](int ry) {
    if (!EDGE) {
      // every lane loads, always: a row past the region repeats the region's last one and a lane past the row's chunks
      // the last of them (all inside the buffer, and never looked at), so the loop holds exactly one load a step and
      // its waits can be counted
      const RowSpan sp = row_span(a, t.img, t.gy0 + min(ry, t.rows - 1), t.cx0, t.cx1);
      return *reinterpret_cast<const uint4*>(a.frames + (sp.o0 + 16 * min(lane, sp.nch - 1)));
    }
    const int y = t.gy0 + ry;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (ry < t.rows && y >= 0 && y < a.height) {
      const RowSpan sp = row_span(a, t.img, y, t.cx0, t.cx1);
      if (lane < sp.nch) v = load_chunk(a.frames, sp.o0 + 16 * lane, a.total);
    }
    return v;
  };
  uint4 cur = fetch(wave), nxt = fetch(wave + WAVES);
  for (int g = 0; g < groups; ++g) {
    const int ry = g * WAVES + wave, y = t.gy0 + ry;
    const bool live = ry < t.rows && y >= 0 && y < a.height;
    stage[g & 1][wave][lane] = cur;
    cur = nxt;
    nxt = fetch(ry + 2 * WAVES);
    // a staging row is its wave's own: what its lanes wrote is read by its lanes only, and the LDS serves a wave's
    // accesses in order, so the wave alone has to be held together here, not the block
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (live) {
      const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage[g & 1][wave]);
      const int off = row_span(a, t.img, y, t.cx0, t.cx1).off;
      const bool ownRow = ry >= 1 && ry <= t.th;
#pragma unroll
      for (int k = 0; k < RW / 64; ++k) {
        const int c = 64 * k + lane, x = t.gx0 + c;
        if (x >= t.cx0 && x < t.cx1) {
          const uint8_t* px = bytes + off + 3 * (x - t.cx0);
          const uint32_t c0 = px[0], c1 = px[1], c2 = px[2];
          const uint32_t b = a.swap ? c0 : c2, r = a.swap ? c2 : c0;
          G[ry][c] = (uint8_t)((3735u * b + 19235u * c1 + 9798u * r + 16384u) >> 15);
          if (ownRow && c >= 1 && c <= t.len) {
            mn = min(mn, min(c0, min(c1, c2)));
            mx = max(mx, max(c0, max(c1, c2)));
            sum += c0 + c1 + c2;
          }
        }
      }
    }
  }
}

__global__ __launch_bounds__(THREADS) void frame_stats_kernel(const FrameArgs a) {
  __shared__ uint4 stage[2][WAVES][STAGE_PITCH];
  __shared__ uint8_t G[ROWS][RW];
  __shared__ u64 red[WAVES][5];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tilesPer = a.tilesX * a.tilesY;
  const int img = (int)(blockIdx.x / (unsigned)tilesPer), tIdx = (int)(blockIdx.x - (unsigned)img * tilesPer);
  const int ty = tIdx / a.tilesX, tx = tIdx - ty * a.tilesX;
  const int x0 = tx * TW, y0 = ty * TR, gx0 = x0 - 1, gy0 = y0 - 1;
  const int len = min(TW, a.width - x0), th = min(TR, a.height - y0), rows = th + 2;   // 1 <= len, th; rows <= ROWS
  const int cx0 = max(gx0, 0), cx1 = min(gx0 + RW, a.width);                          // the region's columns inside the image

  // ---- the gray plane of the region, and minimum, maximum and sum of the tile's bytes.  A chunk starts at most 15
  // bytes in front of its row's first byte and ends at most 15 behind its last: where that keeps all rows of the
  // region, the halo rows outside the image included (they are a neighbouring frame's), inside the buffer, the block
  // runs the copy that loads without looking; else - near the buffer's ends - the one that does.
  uint32_t mn = 255u, mx = 0u, sum = 0u;
  const Tile t = {img, gx0, gy0, len, th, rows, cx0, cx1};
  const long long firstRow = (long long)img * a.height + gy0, lastRow = firstRow + rows - 1;
  if (firstRow * a.stride + 3ll * cx0 - 15 < 0 || lastRow * a.stride + 3ll * cx1 + 15 > a.total)
    gray_plane<true>(a, t, stage, G, mn, mx, sum);
  else
    gray_plane<false>(a, t, stage, G, mn, mx, sum);
  __syncthreads();

  // ---- the Laplacian: thread c walks down region column c
  int s1 = 0;
  uint32_t s2 = 0u;
  if (tid >= 1 && tid <= len) {
    const int c = tid, x = gx0 + c;
    const int cl = reflect101(x - 1, a.width) - gx0, cr = reflect101(x + 1, a.width) - gx0;
    int up = G[reflect101(y0 - 1, a.height) - gy0][c], mid = G[1][c];
    for (int oy = 0; oy < th; ++oy) {
      const int r = oy + 1;
      const int down = G[reflect101(y0 + oy + 1, a.height) - gy0][c];
      const int lap = up + down + (int)G[r][cl] + (int)G[r][cr] - 4 * mid;
      s1 += lap;
      s2 += (uint32_t)(lap * lap);
      up = mid, mid = down;
    }
  }

  // ---- wave, block, record
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor(mn, d, 64));
    mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    sum += __shfl_xor(sum, d, 64);
    s1 += __shfl_xor(s1, d, 64);
    s2 += __shfl_xor(s2, d, 64);
  }
  if (lane == 0) {
    red[wave][0] = mn, red[wave][1] = mx, red[wave][2] = sum;
    red[wave][3] = (u64)(long long)s1;   // two's complement
    red[wave][4] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    u64 v[5] = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4]};
    for (int w = 1; w < WAVES; ++w) {
      v[0] = min(v[0], red[w][0]), v[1] = max(v[1], red[w][1]);
      v[2] += red[w][2], v[3] += red[w][3], v[4] += red[w][4];
    }
    u64* rec = a.out + (size_t)img * FRAME_STATS_WORDS;
    atomicMin(rec + 0, v[0]);
    atomicMax(rec + 1, v[1]);
    atomicAdd(rec + 2, v[2]);
    atomicAdd(rec + 3, v[3]);
    atomicAdd(rec + 4, v[4]);
  }
}

// ---- the probability planes ----------------------------------------------------------------------------------------

constexpr uint32_t KEY_POS_INF = 0xff800000u, KEY_NEG_INF = 0x007fffffu;   // float_key of +inf and of -inf

// monotone in the float's value, -0.0 below +0.0
__device__ __forceinline__ uint32_t float_key(uint32_t bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }
__device__ __forceinline__ uint32_t key_bits(uint32_t key) { return (key >> 31) ? (key ^ 0x80000000u) : ~key; }

struct ProbArgs {
  const float* scores;
  u64* out;
  unsigned numel;
  int bpf;   // blocks per frame
  float threshold;
};

struct ProbAcc {
  uint32_t kmin, kmax, above, ones, nans;
  u64 frac;
};

__device__ __forceinline__ void prob_add(ProbAcc& p, float s, float threshold) {
  const bool isnan = s != s;
  const uint32_t key = float_key(__float_as_uint(s));
  p.kmin = isnan ? p.kmin : min(p.kmin, key);
  p.kmax = isnan ? p.kmax : max(p.kmax, key);
  p.nans += isnan ? 1u : 0u;
  p.above += s > threshold ? 1u : 0u;
  const bool one = s >= 1.0f;
  const float c = (s > 0.0f && !one) ? s : 0.0f;   // a NaN, a negative value and what is counted in `ones`: 0
  p.ones += one ? 1u : 0u;
  p.frac += (uint32_t)(c * 4294967296.0f);         // exact product below 2^32
}

__global__ __launch_bounds__(THREADS) void prob_stats_kernel(const ProbArgs a) {
  __shared__ uint32_t redk[WAVES][2];
  __shared__ u64 reds[WAVES][3];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const unsigned img = blockIdx.x / (unsigned)a.bpf, blk = blockIdx.x - img * (unsigned)a.bpf;
  const float* __restrict__ p = a.scores + (size_t)img * a.numel;
  const long long numel = a.numel;
  const long long mis = (long long)((reinterpret_cast<uintptr_t>(p) & 15u) >> 2);   // floats in front of the frame in its first chunk
  const long long nvec = (mis + numel + 3) >> 2;
  const long long per = (nvec + a.bpf - 1) / a.bpf;
  const long long v0 = (long long)blk * per, v1 = min(v0 + per, nvec);
  ProbAcc acc = {KEY_POS_INF, KEY_NEG_INF, 0u, 0u, 0u, 0ull};
  for (long long v = v0 + tid; v < v1; v += THREADS) {
    const long long e = 4 * v - mis;   // the chunk's first float; negative in front of the frame
    if (e >= 0 && e + 4 <= numel) {
      const float4 f = *reinterpret_cast<const float4*>(p + e);
      prob_add(acc, f.x, a.threshold);
      prob_add(acc, f.y, a.threshold);
      prob_add(acc, f.z, a.threshold);
      prob_add(acc, f.w, a.threshold);
    } else {
      for (int j = 0; j < 4; ++j)
        if (e + j >= 0 && e + j < numel) prob_add(acc, p[e + j], a.threshold);
    }
  }
  u64 above = acc.above, nans = acc.nans, total = acc.frac + ((u64)acc.ones << 32);
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    acc.kmin = min(acc.kmin, (uint32_t)__shfl_xor(acc.kmin, d, 64));
    acc.kmax = max(acc.kmax, (uint32_t)__shfl_xor(acc.kmax, d, 64));
    above += shfl_xor64(above, d);
    nans += shfl_xor64(nans, d);
    total += shfl_xor64(total, d);
  }
  if (lane == 0) {
    redk[wave][0] = acc.kmin, redk[wave][1] = acc.kmax;
    reds[wave][0] = above, reds[wave][1] = total, reds[wave][2] = nans;
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t kmin = redk[0][0], kmax = redk[0][1];
    u64 v[3] = {reds[0][0], reds[0][1], reds[0][2]};
    for (int w = 1; w < WAVES; ++w) {
      kmin = min(kmin, redk[w][0]), kmax = max(kmax, redk[w][1]);
      v[0] += reds[w][0], v[1] += reds[w][1], v[2] += reds[w][2];
    }
    u64* rec = a.out + (size_t)img * PROB_STATS_WORDS;
    // word 0: minimum's bits below, maximum's above, both replaced in one compare-and-swap
    u64 old = atomicAdd(rec, 0ull);
    for (;;) {
      const uint32_t lo = key_bits(min(float_key((uint32_t)old), kmin));
      const uint32_t hi = key_bits(max(float_key((uint32_t)(old >> 32)), kmax));
      const u64 want = ((u64)hi << 32) | lo;
      if (want == old) break;
      const u64 seen = atomicCAS(rec, old, want);
      if (seen == old) break;
      old = seen;
    }
    atomicAdd(rec + 1, v[0]);
    atomicAdd(rec + 2, v[1]);
    atomicAdd(rec + 3, v[2]);
  }
}

hipError_t init_records(u64* out, size_t words, int recWords, u64 first, hipStream_t s) {
  const size_t blocks = (words + THREADS - 1) / THREADS;
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipLaunchKernelGGL(stats_init_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, out, words, recWords, first);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_frame_stats(const uint8_t* frames, int n, int height, int width, long long rowStride, int isBgr,
                              u64* out, hipStream_t s) {
  FrameArgs a;
  a.frames = frames, a.out = out;
  a.n = n, a.height = height, a.width = width;
  a.stride = rowStride;
  a.total = ((long long)n * height - 1) * rowStride + 3ll * width;
  a.tilesX = (width + TW - 1) / TW, a.tilesY = (height + TR - 1) / TR;
  a.swap = isBgr ? 1 : 0;
  const u64 blocks = (u64)a.tilesX * a.tilesY * (u64)n;   // at most n * height * width
  if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
  hipError_t e = init_records(out, (size_t)n * FRAME_STATS_WORDS, FRAME_STATS_WORDS, 255ull, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(frame_stats_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_prob_stats(const float* scores, int n, unsigned numel, float threshold, u64* out, hipStream_t s) {
  ProbArgs a;
  a.scores = scores, a.out = out;
  a.numel = numel, a.threshold = threshold;
  // about 8192 floats a block, at most 256 blocks a frame, and a grid that fits 31 bits
  const u64 chunks = ((u64)numel + 3) / 4 + 1;
  u64 bpf = (chunks + 2047) / 2048;
  if (bpf > 256) bpf = 256;
  if (bpf * (u64)n > 0x7fffffffull) bpf = 0x7fffffffull / (u64)n;   // n < 2^31: at least 1
  a.bpf = (int)bpf;
  const u64 first = ((u64)0xff800000u << 32) | 0x7f800000u;   // maximum -inf, minimum +inf
  hipError_t e = init_records(out, (size_t)n * PROB_STATS_WORDS, PROB_STATS_WORDS, first, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(prob_stats_kernel, dim3((unsigned)(bpf * (u64)n)), dim3(THREADS), 0, s, a);
  return hipGetLastError();
}

}  // namespace unet

extern "C" {

int unet_frame_stats_u8_batch(int device, const uint8_t* framesDev, int n, int height, int width, int rowStride,
                              int isBgr, unsigned long long* outDev, void* stream) {
  const unet::OpCall op{"unet_frame_stats_u8_batch"};
  if (!framesDev || !outDev) return op.refuse("a null pointer");
  if (unet::misaligned(outDev, 8)) return op.refuse("out_dev must be 8-byte aligned");
  if (n <= 0 || height <= 0 || width <= 0) return op.refuse("n, height and width must be positive");
  if (!unet::fits_int((unsigned long long)n * height * width))
    return op.refuse("n * height * width must be smaller than 2^31");
  if (rowStride != 0 && (long long)rowStride < 3ll * width)
    return op.refuse("row_stride must be 0 (dense) or at least 3 * width");
  const long long stride = rowStride ? (long long)rowStride : 3ll * width;
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_frame_stats(framesDev, n, height, width, stride, isBgr, outDev, (hipStream_t)stream));
}

int unet_prob_stats_f32_batch(int device, const float* scoresDev, int n, size_t numelPerFrame, float threshold,
                              unsigned long long* outDev, void* stream) {
  const unet::OpCall op{"unet_prob_stats_f32_batch"};
  if (!scoresDev || !outDev) return op.refuse("a null pointer");
  if (unet::misaligned(scoresDev, 4)) return op.refuse("scores_dev must be 4-byte aligned");
  if (unet::misaligned(outDev, 8)) return op.refuse("out_dev must be 8-byte aligned");
  if (n <= 0 || numelPerFrame == 0) return op.refuse("n and numel_per_frame must be positive");
  if (!unet::fits_int(numelPerFrame)) return op.refuse("numel_per_frame must be smaller than 2^31");
  if (std::isnan(threshold)) return op.refuse("threshold must not be a NaN");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_prob_stats(scoresDev, n, (unsigned)numelPerFrame, threshold, outDev, (hipStream_t)stream));
}

}  // extern "C"
