// The gradient pass (grad_kernels.h): plain C++, memory bound, no atomics.
//
// grad_pass_kernel.  The buffers are cut into 16-byte chunks at aligned ADDRESSES: `head` floats in front of the first
// aligned address, nvec whole chunks, fewer than four floats behind the last.  Chunk v belongs to thread (v mod T) of
// the grid's T = blocks * 256 threads, which takes its chunks in rising order (grid stride); the up to six floats of
// head and tail belong to the first threads of block 0, one each, after their chunks.  dst, a and b can share chunks
// only when they are equally far from a 16-byte boundary; where they are not, the same kernel runs with chunks of one
// float (W = 1), at a quarter of the request width.  Every element is read and then written by the same thread, so dst
// may be a or b.
//
// The record.  A thread adds the squares of its finite values, each formed exactly in double (24-bit significands), to
// a double of its own, in the order it meets them, and counts the others in a 64-bit integer.  The block adds its 256
// pairs in a tree through LDS (partner at distance 128, 64, ... 1) and stores one pair into work[2 * block].
// grad_finish_kernel, one block enqueued behind the pass, adds the pairs of the blocks: thread t those of blocks 8t ..
// 8t + 7 in index order, then the same tree.  Nothing here depends on which CU ran a block or when: for given numel and
// given distances of the pointers from a 16-byte boundary the record is the same bits on every run and every device.
//
// No argument the entry point accepts makes a kernel read or write outside its buffers: a chunk v < nvec covers
// elements head + 4v .. head + 4v + 3 < head + 4 nvec <= numel, and the edge threads index below numel by construction.
#include "grad_kernels.h"

#include "op_entry.h"


namespace unet {

namespace {

typedef unsigned long long u64;

constexpr int MODE_ADD = 0, MODE_COPY = 1, MODE_READ = 2;

struct GradArgs {
  float* dst;
  const float* a;
  const float* b;
  size_t numel, head, nvec;   // floats in front of the chunks; chunks of W floats
  double* work;
};

template <int W>
struct Chunk {
  float v[W];
};

template <int W>
__device__ __forceinline__ Chunk<W> load_chunk(const float* p) {
  Chunk<W> c;
  if constexpr (W == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    c.v[0] = f.x, c.v[1] = f.y, c.v[2] = f.z, c.v[3] = f.w;
  } else {
    c.v[0] = *p;
  }
  return c;
}

template <int W>
__device__ __forceinline__ void store_chunk(float* p, const Chunk<W>& c) {
  if constexpr (W == 4)
    *reinterpret_cast<float4*>(p) = make_float4(c.v[0], c.v[1], c.v[2], c.v[3]);
  else
    *p = c.v[0];
}

__device__ __forceinline__ void record_add(float x, double& sum, u64& bad) {
  const bool finite = (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u;
  const double d = (double)x;
  sum += finite ? d * d : 0.0;   // the square is exact in double, so a fused multiply-add rounds as the sum does
  bad += finite ? 0ull : 1ull;
}

// W floats at p (offset e of the buffers) through the pass
template <int W, int MODE, bool REC>
__device__ __forceinline__ void pass_chunk(const GradArgs& g, size_t e, double& sum, u64& bad) {
  Chunk<W> x = load_chunk<W>(g.a + e);
  if constexpr (MODE == MODE_ADD) {
    const Chunk<W> y = load_chunk<W>(g.b + e);
#pragma unroll
    for (int j = 0; j < W; ++j) x.v[j] = x.v[j] + y.v[j];
  }
  if constexpr (MODE != MODE_READ) store_chunk<W>(g.dst + e, x);
  if constexpr (REC) {
#pragma unroll
    for (int j = 0; j < W; ++j) record_add(x.v[j], sum, bad);
  }
}

// the block's 256 (sum, count) pairs into one, in a fixed tree; the result is thread 0's
__device__ __forceinline__ void block_tree(double& sum, u64& bad, double* sd, u64* sc) {
  const int tid = threadIdx.x;
  sd[tid] = sum, sc[tid] = bad;
  __syncthreads();
#pragma unroll
  for (int d = GRAD_THREADS / 2; d >= 1; d >>= 1) {
    if (tid < d) {
      sd[tid] = sd[tid] + sd[tid + d];
      sc[tid] = sc[tid] + sc[tid + d];
    }
    __syncthreads();
  }
  sum = sd[0], bad = sc[0];
}

template <int W, int MODE, bool REC>
__global__ __launch_bounds__(GRAD_THREADS) void grad_pass_kernel(const GradArgs g) {
  __shared__ double sd[REC ? GRAD_THREADS : 1];
  __shared__ u64 sc[REC ? GRAD_THREADS : 1];
  const size_t gid = (size_t)blockIdx.x * GRAD_THREADS + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * GRAD_THREADS;
  double sum = 0.0;
  u64 bad = 0ull;
  for (size_t v = gid; v < g.nvec; v += stride) pass_chunk<W, MODE, REC>(g, g.head + (size_t)W * v, sum, bad);
  // head and tail: fewer than 2 W floats, one to a thread of block 0
  const size_t body = (size_t)W * g.nvec;
  if (gid < g.numel - body) pass_chunk<1, MODE, REC>(g, gid < g.head ? gid : body + gid, sum, bad);
  if constexpr (REC) {
    block_tree(sum, bad, sd, sc);
    if (threadIdx.x == 0) {
      g.work[2 * (size_t)blockIdx.x] = sum;
      g.work[2 * (size_t)blockIdx.x + 1] = (double)bad;   // exact below 2^53
    }
  }
}

// record = the blocks' pairs added in a fixed order; nblocks <= GRAD_GRID, 0 for an empty buffer
__global__ __launch_bounds__(GRAD_THREADS) void grad_finish_kernel(const double* work, int nblocks, double* record) {
  __shared__ double sd[GRAD_THREADS];
  __shared__ u64 sc[GRAD_THREADS];
  constexpr int PER = GRAD_GRID / GRAD_THREADS;
  double sum = 0.0;
  u64 bad = 0ull;
  for (int j = 0; j < PER; ++j) {
    const int blk = (int)threadIdx.x * PER + j;
    if (blk < nblocks) {
      sum += work[2 * blk];
      bad += (u64)work[2 * blk + 1];
    }
  }
  block_tree(sum, bad, sd, sc);
  if (threadIdx.x == 0) {
    record[0] = sum;
    record[1] = (double)bad;
  }
}

template <int W, int MODE>
void launch_pass(const GradArgs& g, bool rec, unsigned blocks, hipStream_t s) {
  if (rec)
    hipLaunchKernelGGL((grad_pass_kernel<W, MODE, true>), dim3(blocks), dim3(GRAD_THREADS), 0, s, g);
  else
    hipLaunchKernelGGL((grad_pass_kernel<W, MODE, false>), dim3(blocks), dim3(GRAD_THREADS), 0, s, g);
}

template <int W>
void launch_mode(const GradArgs& g, int mode, bool rec, unsigned blocks, hipStream_t s) {
  if (mode == MODE_ADD)
    launch_pass<W, MODE_ADD>(g, rec, blocks, s);
  else if (mode == MODE_COPY)
    launch_pass<W, MODE_COPY>(g, rec, blocks, s);
  else
    launch_pass<W, MODE_READ>(g, true, blocks, s);
}

}  // namespace

hipError_t launch_grad_accumulate(float* dst, const float* a, const float* b, size_t numel, double* record, double* work,
                                  hipStream_t s) {
  const int mode = b ? MODE_ADD : (dst == a ? MODE_READ : MODE_COPY);
  const bool rec = record != nullptr;
  if (mode == MODE_READ && !rec) return hipSuccess;   // nothing to store, nothing to report
  unsigned blocks = 0;
  if (numel > 0) {
    GradArgs g;
    g.dst = dst, g.a = a, g.b = b, g.numel = numel, g.work = work;
    const uintptr_t off = reinterpret_cast<uintptr_t>(a) & 15u;
    const bool together = (mode == MODE_READ || (reinterpret_cast<uintptr_t>(dst) & 15u) == off) &&
                          (!b || (reinterpret_cast<uintptr_t>(b) & 15u) == off);
    blocks = grad_blocks(numel);
    if (together) {
      const size_t head = ((16u - off) & 15u) / 4;
      g.head = head < numel ? head : numel;
      g.nvec = (numel - g.head) / 4;
      launch_mode<4>(g, mode, rec, blocks, s);
    } else {
      g.head = 0, g.nvec = numel;
      launch_mode<1>(g, mode, rec, blocks, s);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (rec) {
    hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(GRAD_THREADS), 0, s, work, (int)blocks, record);
    return hipGetLastError();
  }
  return hipSuccess;
}

}  // namespace unet

namespace {

// [p, p + n) and [q, q + n) share some but not all floats
bool partly_overlap(const float* p, const float* q, size_t n) {
  if (!p || !q || p == q) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(p), y = reinterpret_cast<uintptr_t>(q), len = n * sizeof(float);
  return x < y ? y - x < len : x - y < len;
}

}  // namespace

extern "C" {

size_t unet_grad_work_bytes(void) { return unet::grad_work_bytes(); }

int unet_grad_accumulate_f32(int device, float* dst, const float* a, const float* b, size_t numel, double* record,
                             double* work, void* stream) {
  const unet::OpCall op{"unet_grad_accumulate_f32"};
  if (!dst || !a) return op.refuse("dst and a must not be null");
  if (unet::misaligned(dst, 4) || unet::misaligned(a, 4) || unet::misaligned(b, 4))
    return op.refuse("dst, a and b must be 4-byte aligned");
  if (numel > ((size_t)1 << 48)) return op.refuse("numel must not exceed 2^48");
  if (record && !work) return op.refuse("a record needs the work buffer (unet_grad_work_bytes)");
  if (unet::misaligned(record, 8) || unet::misaligned(work, 8))
    return op.refuse("record and work must be 8-byte aligned");
  if (partly_overlap(dst, a, numel) || partly_overlap(dst, b, numel))
    return op.refuse("dst may be a or b, or apart from them, but not overlap them in part");
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_grad_accumulate(dst, a, b, numel, record, work, (hipStream_t)stream));
}

}  // extern "C"
