// Kernels and entry points of the ensemble combine and the threshold sweep (ensemble_kernels.h): two bandwidth
// kernels, plain C++, 16-byte loads and stores, integer counters, vector stores and vector atomics only.
#include "ensemble_kernels.h"

#include "op_entry.h"

#include <atomic>
#include <cmath>

// ensemble.combine_model rounds every floating-point operation on its own (numpy has no fused multiply-add); so does
// this file.  The products and sums below are plain operators under this pragma and not __fmul_rn / __fadd_rn: those
// are inline functions of a header compiled ahead of it, whose operations the compiler remains free to contract.
#pragma clang fp contract(off)

namespace unet {

namespace {

constexpr int THREADS = 256;
constexpr unsigned COMBINE_MAX_BLOCKS = 4096;

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---------------------------------------------------------------------------------------------------
// Weighted mean of K probability planes (reference README.md:2623-2647, `ensemble_predict`:
// torch.stack([sigmoid(m(x)) ...]).mean(0) > 0.5).  The arithmetic is the contract - ensemble.combine_model restates it
// in numpy float32, bit for bit:
//   acc = w[0] * p0;  acc = acc + w[k] * pk  for k = 1 .. K-1, in that order, each product and each sum rounded to fp32
//   mask = acc > threshold ? 255 : 0        (NaN: 0)
// A lane takes four consecutive elements: K 16-byte loads, one 16-byte store of the means, one 32-bit store of the four
// mask bytes.  VEC = false (a pointer that is not 16-byte aligned) takes everything one element at a time; the last
// numel % 4 elements always go that way.
// ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ float combine_one(const EnsembleMembers& m, int k, size_t i) {
  float acc = m.w[0] * m.p[0][i];
  for (int j = 1; j < k; ++j) acc = acc + m.w[j] * m.p[j][i];
  return acc;
}

template <bool VEC>
__global__ __launch_bounds__(THREADS) void ensemble_combine_kernel(const EnsembleMembers m, int k, size_t numel,
                                                                   float thr, float* __restrict__ probsOut,
                                                                   uint8_t* __restrict__ maskOut) {
  const size_t first = (size_t)blockIdx.x * THREADS + threadIdx.x, stride = (size_t)gridDim.x * THREADS;
  const size_t nvec = VEC ? numel / 4 : 0;
  if (VEC) {
    for (size_t i = first; i < nvec; i += stride) {
      float4 v = reinterpret_cast<const float4*>(m.p[0])[i];
      float4 a;
      a.x = m.w[0] * v.x, a.y = m.w[0] * v.y, a.z = m.w[0] * v.z, a.w = m.w[0] * v.w;
      for (int j = 1; j < k; ++j) {
        v = reinterpret_cast<const float4*>(m.p[j])[i];
        const float w = m.w[j];
        a.x = a.x + w * v.x;
        a.y = a.y + w * v.y;
        a.z = a.z + w * v.z;
        a.w = a.w + w * v.w;
      }
      if (probsOut) reinterpret_cast<float4*>(probsOut)[i] = a;
      if (maskOut)
        reinterpret_cast<uint32_t*>(maskOut)[i] = (a.x > thr ? 0xffu : 0u) | (a.y > thr ? 0xff00u : 0u) |
                                                  (a.z > thr ? 0xff0000u : 0u) | (a.w > thr ? 0xff000000u : 0u);
    }
  }
  for (size_t i = nvec * 4 + first; i < numel; i += stride) {
    const float a = combine_one(m, k, i);
    if (probsOut) probsOut[i] = a;
    if (maskOut) maskOut[i] = a > thr ? 255 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------
// Confusion counts of a score plane at T ascending thresholds in one read of scores and targets.  The counting rule -
// metrics.sweep_model restates it in numpy:
//   bin = #{ j : score > t[j] }   in 0 .. T; a score equal to t[j] is not above it, a NaN is above nothing (bin 0)
//   cls = target != 0             (floats and bytes alike)
//   counts[cls * (T + 1) + bin] += 1
// The scores may be logits, probabilities or an ensemble's means: only the order matters.  The thresholds arrive by
// value and sit in scalar registers; the bin is a branch-free sum of T compares.
//
// Counters: 32-bit in LDS, one copy per wave, flushed after a barrier with one 64-bit global atomic per non-zero
// counter (sweep_grid keeps a block's share below 2^32).  All integers: the result does not depend on any order.
//
// COMBINE: on a lane mask over 90 % of the pixels are confident negatives, so a whole wave wants counts[0][0] and
// per-lane LDS atomics serialise 64 deep.  Instead the wave walks the distinct slots present: the first lane still
// unserved names its slot, a ballot finds every lane that holds the same one, that first lane adds their number with
// one LDS atomic.  One round for the common wave, two where lane and background meet; after SWEEP_COMBINE_ROUNDS
// rounds the lanes still unserved add their own (walking every distinct slot of a wave whose scores are spread over
// all bins took twice the time of the per-lane form, profiles/r20/ensemble_sweep.md).  The rounds run on ballots, which
// are the same in every lane, so all 64 lanes take every round (and every call: the callers' loops are bounded per wave,
// not per lane).  COMBINE = false keeps the per-lane atomic alone for comparison (unet_set_sweep_combine,
// tools/ensemble_sweep_timing.py).
// ---------------------------------------------------------------------------------------------------
constexpr int SWEEP_COMBINE_ROUNDS = 2;

template <bool COMBINE>
__device__ __forceinline__ void tally(unsigned* mine, bool valid, int slot, int lane) {
  if (!COMBINE) {
    if (valid) atomicAdd(&mine[slot], 1u);
    return;
  }
  unsigned long long rest = __ballot(valid);
#pragma unroll
  for (int round = 0; round < SWEEP_COMBINE_ROUNDS && rest; ++round) {
    const int leader = __builtin_ctzll(rest);
    const int s = __builtin_amdgcn_readlane(slot, leader);
    const unsigned long long same = __ballot(valid && slot == s);
    if (lane == leader) atomicAdd(&mine[s], (unsigned)__popcll(same));
    rest &= ~same;
  }
  if ((rest >> lane) & 1) atomicAdd(&mine[slot], 1u);   // a wave with more distinct slots than rounds: the rest one by one
}

__device__ __forceinline__ int sweep_bin(float v, const SweepThresholds& thr, int nT) {
  int bin = 0;
  for (int j = 0; j < nT; ++j) bin += v > thr.t[j] ? 1 : 0;
  return bin;
}

constexpr int SWEEP_SLOTS = 2 * (SWEEP_MAX + 1);
constexpr int SWEEP_UNROLL = 4;

template <bool U8, bool COMBINE>
__global__ __launch_bounds__(THREADS) void score_sweep_kernel(const float* __restrict__ x, const void* __restrict__ tRaw,
                                                              size_t numel, int vec, const SweepThresholds thr, int nT,
                                                              unsigned long long* __restrict__ counts) {
  __shared__ unsigned sh[THREADS / 64][SWEEP_SLOTS];
  const int slots = 2 * (nT + 1), lane = threadIdx.x & 63;
  for (int i = threadIdx.x; i < (THREADS / 64) * SWEEP_SLOTS; i += THREADS) (&sh[0][0])[i] = 0;
  __syncthreads();
  unsigned* mine = sh[threadIdx.x >> 6];
  // every loop below is bounded by the index of the wave's lane 0, so that the lanes of a wave leave it together
  const size_t wave0 = (size_t)blockIdx.x * THREADS + (threadIdx.x & ~63), stride = (size_t)gridDim.x * THREADS;
  const size_t nvec = vec ? numel / 4 : 0;
  // SWEEP_UNROLL rounds at a time: all their loads are issued before the first compare, which is what keeps enough
  // bytes in flight for a kernel with this little arithmetic; the thresholds are walked once for all 16 elements
  for (size_t base = wave0; base < nvec; base += stride * SWEEP_UNROLL) {
    float v[SWEEP_UNROLL][4];
    int slot[SWEEP_UNROLL][4];
    bool valid[SWEEP_UNROLL];
#pragma unroll
    for (int u = 0; u < SWEEP_UNROLL; ++u) {
      const size_t i = base + u * stride + lane;
      valid[u] = i < nvec;
      float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
      int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
      if (valid[u]) {
        q = reinterpret_cast<const float4*>(x)[i];
        if (U8) {
          const uint32_t t = reinterpret_cast<const uint32_t*>(tRaw)[i];
          c0 = (t & 0xffu) != 0, c1 = (t & 0xff00u) != 0, c2 = (t & 0xff0000u) != 0, c3 = (t & 0xff000000u) != 0;
        } else {
          const float4 t = reinterpret_cast<const float4*>(tRaw)[i];
          c0 = t.x != 0.f, c1 = t.y != 0.f, c2 = t.z != 0.f, c3 = t.w != 0.f;
        }
      }
      v[u][0] = q.x, v[u][1] = q.y, v[u][2] = q.z, v[u][3] = q.w;
      slot[u][0] = c0 * (nT + 1), slot[u][1] = c1 * (nT + 1), slot[u][2] = c2 * (nT + 1), slot[u][3] = c3 * (nT + 1);
    }
    for (int j = 0; j < nT; ++j) {
      const float tj = thr.t[j];
#pragma unroll
      for (int u = 0; u < SWEEP_UNROLL; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) slot[u][e] += v[u][e] > tj ? 1 : 0;
    }
#pragma unroll
    for (int u = 0; u < SWEEP_UNROLL; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e) tally<COMBINE>(mine, valid[u], slot[u][e], lane);
  }
  for (size_t base = nvec * 4 + wave0; base < numel; base += stride) {
    const size_t i = base + lane;
    const bool valid = i < numel;
    float v = 0.f;
    int c = 0;
    if (valid) {
      v = x[i];
      c = U8 ? static_cast<const uint8_t*>(tRaw)[i] != 0 : static_cast<const float*>(tRaw)[i] != 0.f;
    }
    tally<COMBINE>(mine, valid, c * (nT + 1) + sweep_bin(v, thr, nT), lane);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < slots; b += THREADS) {
    unsigned n = 0;
    for (int k = 0; k < THREADS / 64; ++k) n += sh[k][b];
    if (n) atomicAdd(&counts[b], (unsigned long long)n);
  }
}

}  // namespace

hipError_t launch_ensemble_combine(const EnsembleMembers& m, int k, size_t numel, float threshold, float* probsOut,
                                   uint8_t* maskOut, hipStream_t s) {
  if (k < 1 || k > ENSEMBLE_MAX || numel == 0 || (!probsOut && !maskOut)) return hipErrorInvalidValue;
  bool vec = (!probsOut || aligned16(probsOut)) && (!maskOut || aligned16(maskOut));
  for (int j = 0; j < k; ++j) vec = vec && aligned16(m.p[j]);
  const size_t work = vec ? (numel + 3) / 4 : numel;
  const size_t blocks = (work + THREADS - 1) / THREADS;
  const unsigned grid = (unsigned)(blocks > COMBINE_MAX_BLOCKS ? COMBINE_MAX_BLOCKS : blocks);
  if (vec)
    hipLaunchKernelGGL(ensemble_combine_kernel<true>, dim3(grid), dim3(THREADS), 0, s, m, k, numel, threshold, probsOut,
                       maskOut);
  else
    hipLaunchKernelGGL(ensemble_combine_kernel<false>, dim3(grid), dim3(THREADS), 0, s, m, k, numel, threshold, probsOut,
                       maskOut);
  return hipGetLastError();
}

hipError_t launch_score_sweep(const float* scores, const void* targets, bool targetsU8, size_t numel,
                              const SweepThresholds& thr, int nThresholds, bool waveCombine, unsigned long long* counts,
                              hipStream_t s) {
  if (!sweep_numel_supported(numel) || nThresholds < 1 || nThresholds > SWEEP_MAX) return hipErrorInvalidValue;
  // the byte targets of four elements are read as one 32-bit word: 4-byte alignment is all they need
  const int vec = aligned16(scores) && (targetsU8 ? (reinterpret_cast<uintptr_t>(targets) & 3) == 0 : aligned16(targets));
  const dim3 grid(sweep_grid(numel)), block(THREADS);
  if (targetsU8) {
    if (waveCombine)
      hipLaunchKernelGGL((score_sweep_kernel<true, true>), grid, block, 0, s, scores, targets, numel, vec, thr,
                         nThresholds, counts);
    else
      hipLaunchKernelGGL((score_sweep_kernel<true, false>), grid, block, 0, s, scores, targets, numel, vec, thr,
                         nThresholds, counts);
  } else {
    if (waveCombine)
      hipLaunchKernelGGL((score_sweep_kernel<false, true>), grid, block, 0, s, scores, targets, numel, vec, thr,
                         nThresholds, counts);
    else
      hipLaunchKernelGGL((score_sweep_kernel<false, false>), grid, block, 0, s, scores, targets, numel, vec, thr,
                         nThresholds, counts);
  }
  return hipGetLastError();
}

}  // namespace unet

namespace {

std::atomic<int> g_sweepCombine{1};

}  // namespace

extern "C" {

int unet_ensemble_combine(int device, const float* const* probsDev, int k, const float* weightsHost, size_t numel,
                          float threshold, float* probsOutDev, uint8_t* maskOutDev, void* stream) {
  const unet::OpCall op{"unet_ensemble_combine"};
  if (!probsDev) return op.refuse("a null pointer");
  if (k < 1 || k > UNET_ENSEMBLE_MAX) return op.refuse("k must lie in 1 .. UNET_ENSEMBLE_MAX");
  if (!probsOutDev && !maskOutDev) return op.refuse("both outputs are null");
  if (numel == 0) return op.refuse("numel is 0");
  unet::EnsembleMembers m = {};
  for (int j = 0; j < k; ++j) {
    if (!probsDev[j]) return op.refuse("a null pointer");
    m.p[j] = probsDev[j];
    m.w[j] = weightsHost ? weightsHost[j] : (float)(1.0 / k);
    if (!std::isfinite(m.w[j]) || m.w[j] < 0.f) return op.refuse("every weight must be finite and not negative");
  }
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_ensemble_combine(m, k, numel, threshold, probsOutDev, maskOutDev, (hipStream_t)stream));
}

int unet_score_sweep_accumulate(int device, const float* scoresDev, const void* targetsDev, int targetsAreU8, size_t numel,
                                const float* thresholdsHost, int nThresholds, unsigned long long* countsDev,
                                void* stream) {
  const unet::OpCall op{"unet_score_sweep_accumulate"};
  if (!scoresDev || !targetsDev || !thresholdsHost || !countsDev) return op.refuse("a null pointer");
  if (numel == 0) return op.refuse("numel is 0");
  if (nThresholds < 1 || nThresholds > UNET_SWEEP_MAX) return op.refuse("n_thresholds must lie in 1 .. UNET_SWEEP_MAX");
  unet::SweepThresholds thr = {};
  for (int j = 0; j < nThresholds; ++j) {
    thr.t[j] = thresholdsHost[j];
    // written so that a NaN on either side refuses
    if (std::isnan(thr.t[j]) || (j > 0 && !(thr.t[j] > thr.t[j - 1])))
      return op.refuse("the thresholds must be strictly ascending and free of NaN");
  }
  if (!unet::sweep_numel_supported(numel))
    return op.refuse("numel must stay below 2^41 (the 32-bit counters of a block, sweep_grid)", UNET_ERR_SHAPE);
  if (int rc = op.on(device)) return rc;
  return op.done(unet::launch_score_sweep(scoresDev, targetsDev, targetsAreU8 != 0, numel, thr, nThresholds,
                                          g_sweepCombine.load() != 0, countsDev, (hipStream_t)stream));
}

int unet_set_sweep_combine(int on) { return g_sweepCombine.exchange(on ? 1 : 0); }

}  // extern "C"
