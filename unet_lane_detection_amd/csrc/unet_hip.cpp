// libunet_hip.so - host side of the C ABI declared in include/unet_hip.h.
//
// Owns: parameter intake in PyTorch layout, BatchNorm folding, packing of conv
// weights into MFMA fragment order, the activation workspace and the launch
// sequence of the forward pass (reference README.md:1460-1481).  All
// arithmetic on activations happens in the HIP kernels of igemm_f32.h and
// elementwise.h; there is no CPU fallback.
#include "../../include/unet_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "elementwise.h"
#include "igemm_f32.h"
#include "igemm_bf16.h"
#include "conv_bf16_ws.h"
#include "conv_first_bf16x3.h"
#include "upconv_bf16_ws.h"
#include "upconv_bf16_r512.h"
#include "conv_x3_ws.h"
#include "conv_x3_r512.h"
#include "conv_x3_t448.h"
#include "conv_x3_dec.h"
#include "conv_q8_r512.h"
#include "conv_bf16_r512.h"
#include "upconv_x3_ws.h"
#include "upconv_x3_r512.h"
#include "upconv_x3_win.h"
#include "conv_first_x3.h"
#include "conv_x3_enc1_args.h"
#include "plane_kernels.h"
#include "conv_i8.h"
#include "wino_f32.h"
#include "train_kernels.h"
#include "wgrad_f32.h"
#include "wgrad_wino_f32.h"
#include "wgrad_gemm_f32.h"
#include "wgrad_x3_ws.h"
#include "camera_stage.h"
#include "calib_kernels.h"
#include "conv_h16.h"
#include "launch.h"
#include "op_entry.h"
#include "multiclass_kernels.h"
#include "i8_classes_kernels.h"
#include "i8_head_check.h"

// Kernels that need more dynamic LDS than the default opt in once per (device, kernel): the attribute is per device.
// Shared with the launch units (launch.h).
hipError_t unet::ensure_dyn_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({dev, fn})) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess) done.insert({dev, fn});
  return e;
}

namespace {

using unet::ConvArgs;
using unet::ensure_dyn_lds;

constexpr float kBnEps = 1e-5f;  // nn.BatchNorm2d default (reference README.md:1453)

#define HIPCHK(ctx_err, expr)                                                                   \
  do {                                                                                          \
    hipError_t _e = (expr);                                                                     \
    if (_e != hipSuccess) {                                                                     \
      (ctx_err) = std::string(#expr) + ": " + hipGetErrorString(_e);                            \
      return UNET_ERR_HIP;                                                                      \
    }                                                                                           \
  } while (0)

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// A device buffer that only grows (workspaces, the f16q8 q plane).  Growing waits for the device first: launches still
// in flight may read the old block.  `what` names the buffer in the error text.
struct GrowBuf {
  char* p = nullptr;
  size_t bytes = 0;
  int reserve(std::string& err, size_t need, const char* what) {
    if (need <= bytes) return UNET_OK;
    if (p) {
      HIPCHK(err, hipDeviceSynchronize());
      release();
    }
    if (hipMalloc((void**)&p, need) != hipSuccess) {
      p = nullptr;
      err = std::string(what) + " allocation of " + std::to_string(need) + " bytes failed";
      return UNET_ERR_NOMEM;
    }
    bytes = need;
    return UNET_OK;
  }
  void release() {
    if (p) hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// ------------------------------------------------------------------------------------------
// Optional per-launch timing: a hipEvent pair around every kernel launch, recorded on the stream
// the kernel runs on.  Used by bench.py for the live roofline numbers; off by default.
// ------------------------------------------------------------------------------------------
struct ProfRecord {
  std::string name;
  double flops = 0, bytes = 0, ms = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
};
struct Profiler {
  bool on = false;
  std::vector<ProfRecord> recs;
  void begin(const char* name, double flops, double bytes, hipStream_t s) {
    if (!on) return;
    ProfRecord r;
    r.name = name;
    r.flops = flops;
    r.bytes = bytes;
    hipEventCreate(&r.e0);
    hipEventCreate(&r.e1);
    hipEventRecord(r.e0, s);
    recs.push_back(r);
  }
  void end(hipStream_t s) {
    if (!on) return;
    hipEventRecord(recs.back().e1, s);
  }
  void resolve() {
    for (auto& r : recs)
      if (r.e0) {
        hipEventSynchronize(r.e1);
        float ms = 0;
        hipEventElapsedTime(&ms, r.e0, r.e1);
        r.ms = ms;
        hipEventDestroy(r.e0);
        hipEventDestroy(r.e1);
        r.e0 = r.e1 = nullptr;
      }
  }
  void clear() {
    resolve();
    recs.clear();
  }
};
// Per-call launch context of the calling thread: the handle's profiler (or none) and its device error word.
// thread_local, so two handles driven from two threads do not see each other's scope.
thread_local Profiler* g_prof = nullptr;
// the handle's device-visible error block: word 0 = a bounded spin gave up, word 1 = an activation of the f16x3 tier left
// the fp16 range (conv_x3_ws.h, range watch)
thread_local unsigned* g_errWord = nullptr;

// Device error word for launches made outside a handle (the single-operator test entry points): one per device.
unsigned* op_err_word() {
  static std::mutex mu;
  static std::map<int, unsigned*> words;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(mu);
  auto it = words.find(dev);
  if (it != words.end()) return it->second;
  unsigned* w = nullptr;
  if (hipMalloc((void**)&w, 2 * sizeof(unsigned)) != hipSuccess) return nullptr;
  hipMemset(w, 0, 2 * sizeof(unsigned));
  words[dev] = w;
  return w;
}

inline void prof_begin(const char* n, double fl, double by, hipStream_t s) { if (g_prof) g_prof->begin(n, fl, by, s); }
inline void prof_end(hipStream_t s) { if (g_prof) g_prof->end(s); }

// ------------------------------------------------------------------------------------------
// One GEMM-shaped operator (3x3 conv or 2x2 transposed conv) with device-resident packed weights
// ------------------------------------------------------------------------------------------
struct GemmOp {
  int taps = 9;      // 9: conv3x3, 1: upconv 2x2
  int cinReal = 0;   // channels of the PyTorch tensor
  int cin = 0;       // padded to CK
  int cout = 0;      // real channels (per (a,b) group for upconv)
  int coutPad = 0;   // rounded up to 16
  int nTotal = 0;    // GEMM N padded to BN
  int ck = 16;
  int relu = 0;
  const char* name = nullptr;  // profiler label override for the direct kernel
  const char* nameWino = nullptr;  // ... and for the Winograd kernel on the same operator
  int plain = 0;     // taps == 1 only: 1 = ordinary 1x1 GEMM output (no pixel-shuffle scatter)
  float* wt = nullptr;
  float* wtWino = nullptr;  // Winograd F(2x2,3x3) transformed weights (3x3 convs with Cin % 16 == 0)
  float* scale = nullptr;
  float* shift = nullptr;
  void free_dev() {
    if (wt) hipFree(wt);
    if (wtWino) hipFree(wtWino);
    wtWino = nullptr;
    if (scale) hipFree(scale);
    if (shift) hipFree(shift);
    wt = scale = shift = nullptr;
  }
};

struct TileChoice {
  int ms, th, tw, nld;
};

// Pick the pixel tile: BM = 32*MS pixels as TH global rows x TW columns.  Candidates are the
// factorizations of 128 (MS=4) and 224 (MS=7); cost = padded work / useful work, then halo size.
TileChoice choose_tile(int nh, int w, int ck, bool halo) {
  TileChoice best{4, 8, 16, 4};
  double bestCost = 1e30;
  for (int ms : {7, 4}) {
    const int bm = 32 * ms;
    const int nld = (ck == 16) ? (ms == 7 ? 6 : 4) : (ms == 7 ? 2 : 1);
    const int vpp = ck / 4;
    for (int tw = 2; tw <= bm; ++tw) {
      if (bm % tw) continue;
      const int th = bm / tw;
      const int hp = halo ? (th + 2) * (tw + 2) : th * tw;
      if (hp * vpp > nld * 256) continue;
      const double padW = (double)((w + tw - 1) / tw * tw) / w;
      const double padH = (double)((nh + th - 1) / th * th) / nh;
      const double haloF = (double)hp / (th * tw);
      // padded MFMA work dominates; halo traffic is a mild tie-breaker; prefer the larger tile
      const double cost = padW * padH * (1.0 + 0.02 * haloF) * (ms == 7 ? 0.97 : 1.0);
      if (cost < bestCost) {
        bestCost = cost;
        best = {ms, th, tw, nld};
      }
    }
  }
  return best;
}

template <int CK, int TAPS, int MS, int NS, int NLD, int MODE>
hipError_t launch_one(const ConvArgs& a, dim3 grid, hipStream_t s) {
  // two halo-tile buffers + zero slot, or the epilogue's transposed half tile, whichever is larger
  const size_t lds = std::max<size_t>((size_t)2 * NLD * 256 * 16 + 64, (size_t)MS * 16 * (32 * NS + 4) * 4);
  hipLaunchKernelGGL((unet::igemm_f32_kernel<CK, TAPS, MS, NS, NLD, MODE>), grid, dim3(256), lds, s, a);
  return hipGetLastError();
}

template <int CK, int TAPS, int MODE>
hipError_t launch_cfg(const ConvArgs& a, dim3 grid, int ms, int ns, hipStream_t s) {
  constexpr int NLD7 = (CK == 16) ? 6 : 2;
  constexpr int NLD4 = (CK == 16) ? 4 : 1;
  if (ms == 7) return launch_one<CK, TAPS, 7, 2, NLD7, MODE>(a, grid, s);
  if (ms == 4 && ns == 4) return launch_one<CK, TAPS, 4, 4, NLD4, MODE>(a, grid, s);
  return launch_one<CK, TAPS, 4, 2, NLD4, MODE>(a, grid, s);
}

std::atomic<int> g_winoMode{-1};  // -1: read UNET_NO_WINOGRAD once; 0 / 1: forced by unet_set_winograd
bool wino_enabled() {
  if (g_winoMode < 0) {
    const char* e = getenv("UNET_NO_WINOGRAD");
    g_winoMode = (e && e[0] == '1') ? 0 : 1;
  }
  return g_winoMode == 1;
}

struct WinoTile {
  int tht, twt;
};

// Tile grid of one Winograd block: THt x TWt tiles (<= 128), raw halo (2THt+2)(2TWt+2) <= 640 pixels.
WinoTile choose_wino_tile(int gt, int wt) {
  WinoTile best{8, 16};
  double bestCost = 1e30;
  for (int twt = 1; twt <= unet::WINO_TILES; ++twt) {
    const int tht = unet::WINO_TILES / twt;
    if ((2 * tht + 2) * (2 * twt + 2) > unet::WINO_NLD * unet::WINO_THREADS / 4) continue;
    const double padW = (double)((wt + twt - 1) / twt * twt) / wt;
    const double padH = (double)((gt + tht - 1) / tht * tht) / gt;
    const double fill = (double)unet::WINO_TILES / (tht * twt);
    const double halo = (double)(2 * tht + 2) * (2 * twt + 2) / (4.0 * tht * twt);
    const double cost = padW * padH * fill * (1.0 + 0.03 * halo);
    if (cost < bestCost) {
      bestCost = cost;
      best = {tht, twt};
    }
  }
  return best;
}

// the Winograd kernel takes 3x3 convolutions with transformed weights (Cin % 16 == 0) on even maps ...
bool wino_takes(const GemmOp& op, int h, int w) { return op.taps == 9 && op.wtWino && (h % 2 == 0) && (w % 2 == 0); }
// ... and runs them unless unet_set_winograd / UNET_NO_WINOGRAD switched it off
bool wino_applicable(const GemmOp& op, int h, int w) { return wino_takes(op, h, w) && wino_enabled(); }
// the Winograd kernel addresses its input with 32-bit float4 indices
bool wino_fits(int n, int h, int w, int cin) { return (double)n * h * w * cin < 17179869184.0; }
bool wino_fits(const GemmOp& op, int n, int h, int w) { return wino_fits(n, h, w, op.cin); }

// GEMM N of an operator, padded to the channel tile: 3x3 conv and plain 1x1 over cout, the transposed conv over its
// four (a,b) groups of coutPad columns
inline int gemm_n_total(bool upconv, int cout) {
  const int cols = upconv ? 4 * round_up(cout, 16) : cout;
  return round_up(cols, cols >= 128 ? 128 : 64);
}

// One launch of the fp32 tier's GEMM-shaped operators: the template instance and its grid.  Decided here, for
// run_direct / run_wino, for the path_out of the unet_op_*_f32 test entry points and for unet_host_plan_conv_f32.
struct F32Plan {
  int algo = 0;            // 1: igemm_f32_kernel, 2: wino_f32_kernel
  int ms = 0, ns = 0;      // direct: MS, NS of the instance (Winograd: 0)
  int th = 0, tw = 0;      // direct: pixel tile TH x TW; Winograd: tile grid THt x TWt of one block
  int tilesX = 0, pixTiles = 0, coTiles = 0, coGroup = 1;
  int grid = 0;            // blocks
};

inline int co_group_of(int coTiles) {
  for (int g : {8, 4, 2})
    if (coTiles % g == 0) return g;
  return 1;
}

F32Plan plan_direct(int n, int h, int w, int ck, bool halo, int nTotal) {
  const TileChoice t = choose_tile(n * h, w, ck, halo);
  F32Plan p;
  p.algo = 1;
  p.ms = t.ms;
  // The packed fragment order does not depend on NS, so the channel tile is a launch-time choice:
  // 128 columns with the 128-pixel tile, 64 with the 224-pixel tile (224x128 does not fit 256 VGPRs).
  p.ns = (t.ms == 4 && nTotal % 128 == 0) ? 4 : 2;
  p.th = t.th;
  p.tw = t.tw;
  p.tilesX = (w + t.tw - 1) / t.tw;
  p.pixTiles = p.tilesX * ((n * h + t.th - 1) / t.th);
  p.coTiles = nTotal / (32 * p.ns);
  p.coGroup = co_group_of(p.coTiles);
  p.grid = (int)((size_t)p.pixTiles * p.coTiles);
  return p;
}

F32Plan plan_wino(int n, int h, int w, int nTotal) {
  const int gt = n * (h / 2), wt = w / 2;
  const WinoTile t = choose_wino_tile(gt, wt);
  F32Plan p;
  p.algo = 2;
  p.th = t.tht;
  p.tw = t.twt;
  p.tilesX = (wt + t.twt - 1) / t.twt;
  p.pixTiles = p.tilesX * ((gt + t.tht - 1) / t.tht);
  p.coTiles = nTotal / 32;
  p.coGroup = co_group_of(p.coTiles);
  p.grid = (int)((size_t)p.pixTiles * p.coTiles);
  return p;
}

hipError_t run_wino(const GemmOp& op, const float* in, int n, int h, int w, float* out, int ldo, int coOff,
                    float* pool, hipStream_t s, F32Plan* planOut = nullptr) {
  const F32Plan p = plan_wino(n, h, w, op.nTotal);
  if (planOut) *planOut = p;
  unet::WinoArgs a;
  a.in = in;
  a.wt = op.wtWino;
  a.scale = op.scale;
  a.shift = op.shift;
  a.out = out;
  a.pool = pool;
  a.N = n;
  a.H = h;
  a.W = w;
  a.Cin = op.cin;
  a.Cout = op.cout;
  a.ldo = ldo;
  a.co_off = coOff;
  a.THt = p.th;
  a.TWt = p.tw;
  a.tilesX = p.tilesX;
  a.nChunks = op.cin / 16;
  a.relu = op.relu;
  a.pixTiles = p.pixTiles;
  a.coTiles = p.coTiles;
  a.coGroup = p.coGroup;
  // keep a pixel tile's channel tiles on one XCD so the input tile crosses the fabric once, not once per XCD
  // (measured +0.6 % frames/s over spreading them, on every layer; UNET_WINO_XCD=0 restores the spread)
  static const int xcdMode = [] { const char* e = getenv("UNET_WINO_XCD"); return e ? atoi(e) : -1; }();
  a.xcdLocal = xcdMode >= 0 ? xcdMode : 1;
  a.err = g_errWord ? g_errWord : op_err_word();
  {  // 144 KiB of dynamic LDS needs the opt-in
    hipError_t ea = ensure_dyn_lds(reinterpret_cast<const void*>(&unet::wino_f32_kernel<2>), unet::WINO_LDS_BYTES);
    if (ea != hipSuccess) return ea;
  }
  const double px = (double)n * h * w;
  prof_begin(op.nameWino ? op.nameWino : "conv3x3_wino_f32", 2.0 * px * 9 * op.cinReal * op.cout,
             4.0 * (px * op.cinReal + px * op.cout + 9.0 * op.cinReal * op.cout), s);
  hipLaunchKernelGGL((unet::wino_f32_kernel<2>), dim3((unsigned)p.grid), dim3(unet::WINO_THREADS),
                     unet::WINO_LDS_BYTES, s, a);
  prof_end(s);
  return hipGetLastError();
}

// the direct kernel: in (N,H,W,op.cin) -> out with pixel stride ldo at channel offset coOff
hipError_t run_direct(const GemmOp& op, const float* in, int n, int h, int w, float* out, int ldo, int coOff,
                      hipStream_t s, int outBf16 = 0, F32Plan* planOut = nullptr) {
  const F32Plan p = plan_direct(n, h, w, op.ck, op.taps == 9, op.nTotal);
  if (planOut) *planOut = p;
  ConvArgs a;
  a.in = in;
  a.wt = op.wt;
  a.scale = op.scale;
  a.shift = op.shift;
  a.out = out;
  a.N = n;
  a.H = h;
  a.W = w;
  a.Cin = op.cin;
  a.Cout = op.cout;
  a.CoutPad = op.coutPad;
  a.ldo = ldo;
  a.co_off = coOff;
  a.TH = p.th;
  a.TW = p.tw;
  a.tilesX = p.tilesX;
  a.nChunks = op.cin / op.ck;
  a.relu = op.relu;
  a.out_bf16 = outBf16;
  a.pixTiles = p.pixTiles;
  a.coTiles = p.coTiles;
  a.coGroup = p.coGroup;
  dim3 grid((unsigned)p.grid);
  // algorithmic work of this launch: 2*MAC flops on the real (unpadded) channel counts; bytes = read the
  // input once + write the output once + the weights once
  const double px = (double)n * h * w;
  const double nOut = (op.taps == 9 || op.plain) ? op.cout : 4.0 * op.cout;
  const double flops = 2.0 * px * op.taps * op.cinReal * nOut;
  const double bytes = 4.0 * (px * op.cinReal + px * nOut + (double)op.taps * op.cinReal * nOut);
  prof_begin(op.name ? op.name : (op.taps == 9 ? "conv3x3_igemm_f32" : "upconv2x2_igemm_f32"), flops, bytes, s);
  hipError_t e;
  if (op.taps == 9) {
    e = (op.ck == 16) ? launch_cfg<16, 9, 0>(a, grid, p.ms, p.ns, s) : launch_cfg<4, 9, 0>(a, grid, p.ms, p.ns, s);
  } else {
    if (op.plain)
      e = (op.ck == 16) ? launch_cfg<16, 1, 0>(a, grid, p.ms, p.ns, s) : launch_cfg<4, 1, 0>(a, grid, p.ms, p.ns, s);
    else
      e = (op.ck == 16) ? launch_cfg<16, 1, 1>(a, grid, p.ms, p.ns, s) : launch_cfg<4, 1, 1>(a, grid, p.ms, p.ns, s);
  }
  prof_end(s);
  return e;
}

// in: (N,H,W,op.cin) -> out with pixel stride ldo at channel offset coOff
hipError_t run_gemm_op(const GemmOp& op, const float* in, int n, int h, int w, float* out, int ldo, int coOff,
                       hipStream_t s, int outBf16 = 0) {
  if (!outBf16 && wino_applicable(op, h, w) && wino_fits(op, n, h, w))
    return run_wino(op, in, n, h, w, out, ldo, coOff, nullptr, s);
  return run_direct(op, in, n, h, w, out, ldo, coOff, s, outBf16);
}

// Pack W into [subtile][chunk][tap][lane][KPL]; column -> (source fetch) is given by `col(n, ci, tap)`.
template <class F>
std::vector<float> pack_fragments(int nTotal, int cin, int ck, int taps, F&& col) {
  const int kpl = ck / 4;
  const int nSub = nTotal / 16;
  const int nChunks = cin / ck;
  std::vector<float> out(((size_t)nSub * nChunks * taps + 1) * 64 * kpl, 0.f);  // +1 spare fragment (prefetch overrun)
  for (int cs = 0; cs < nSub; ++cs)
    for (int kc = 0; kc < nChunks; ++kc)
      for (int t = 0; t < taps; ++t) {
        float* dst = out.data() + (((size_t)cs * nChunks + kc) * taps + t) * 64 * kpl;
        for (int lane = 0; lane < 64; ++lane) {
          const int n = cs * 16 + (lane & 15);
          for (int e = 0; e < kpl; ++e) {
            const int ci = kc * ck + (lane >> 4) * kpl + e;
            dst[lane * kpl + e] = col(n, ci, t);
          }
        }
      }
  return out;
}

int upload(std::string& err, float** dst, const std::vector<float>& v) {
  HIPCHK(err, hipMalloc((void**)dst, v.size() * sizeof(float)));
  HIPCHK(err, hipMemcpy(*dst, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return UNET_OK;
}

// conv3x3: w (O,I,3,3), scale/shift per O
int build_conv3x3(std::string& err, GemmOp& op, const float* w, int cout, int cinReal, const float* scale,
                  const float* shift, int relu) {
  op.free_dev();
  op.taps = 9;
  op.cinReal = cinReal;
  op.ck = (cinReal % 16 == 0) ? 16 : 4;
  op.cin = round_up(cinReal, op.ck);
  op.cout = cout;
  op.coutPad = round_up(cout, 16);
  op.nTotal = gemm_n_total(false, cout);
  op.relu = relu;
  auto packed = pack_fragments(op.nTotal, op.cin, op.ck, 9, [&](int n, int ci, int t) -> float {
    if (n >= cout || ci >= cinReal) return 0.f;
    return w[((size_t)n * cinReal + ci) * 9 + t];
  });
  std::vector<float> sc(op.nTotal, 0.f), sh(op.nTotal, 0.f);
  for (int i = 0; i < cout; ++i) {
    sc[i] = scale[i];
    sh[i] = shift[i];
  }
  int rc;
  if ((rc = upload(err, &op.wt, packed))) return rc;
  if (op.ck == 16) {
    // Winograd F(2x2,3x3): U = G g G^T per (co, ci), computed in double
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    auto wino = pack_fragments(op.nTotal, op.cin, 16, 16, [&](int n, int ci, int p) -> float {
      if (n >= cout || ci >= cinReal) return 0.f;
      const float* g = w + ((size_t)n * cinReal + ci) * 9;
      const int pa = p >> 2, pb = p & 3;
      double u = 0.0;
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) u += G[pa][a] * (double)g[a * 3 + b] * G[pb][b];
      return (float)u;
    });
    if ((rc = upload(err, &op.wtWino, wino))) return rc;
  }
  if ((rc = upload(err, &op.scale, sc))) return rc;
  return upload(err, &op.shift, sh);
}

// upconv 2x2 s2: w (I,O,2,2), bias per O. GEMM column n = (a*2+b)*coutPad + co.
int build_upconv(std::string& err, GemmOp& op, const float* w, int cinReal, int cout, const float* bias) {
  op.free_dev();
  op.taps = 1;
  op.cinReal = cinReal;
  op.ck = (cinReal % 16 == 0) ? 16 : 4;
  op.cin = round_up(cinReal, op.ck);
  op.cout = cout;
  op.coutPad = round_up(cout, 16);
  op.nTotal = gemm_n_total(true, cout);
  op.relu = 0;
  const int cp = op.coutPad;
  auto packed = pack_fragments(op.nTotal, op.cin, op.ck, 1, [&](int n, int ci, int) -> float {
    const int ab = n / cp, co = n % cp;
    if (ab >= 4 || co >= cout || ci >= cinReal) return 0.f;
    return w[((size_t)ci * cout + co) * 4 + ab];
  });
  std::vector<float> sc(op.nTotal, 0.f), sh(op.nTotal, 0.f);
  for (int n = 0; n < 4 * cp; ++n) {
    const int co = n % cp;
    if (co < cout) {
      sc[n] = 1.f;
      sh[n] = bias[co];
    }
  }
  int rc;
  if ((rc = upload(err, &op.wt, packed))) return rc;
  if ((rc = upload(err, &op.scale, sc))) return rc;
  return upload(err, &op.shift, sh);
}

inline unsigned grid_for(size_t items, int perBlock = 256) {
  size_t b = (items + perBlock - 1) / perBlock;
  return (unsigned)std::min<size_t>(std::max<size_t>(b, 1), 256 * 8 * 4);
}

hipError_t run_maxpool(const float* in, float* out, int n, int h, int w, int c, int ldi, hipStream_t s) {
  const size_t total = (size_t)n * (h / 2) * (w / 2) * (c / 4);
  prof_begin("maxpool2x2", 0.0, 4.0 * total * 4 * 5, s);
  hipLaunchKernelGGL(unet::maxpool2x2_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, n, h, w, c, ldi);
  prof_end(s);
  return hipGetLastError();
}

hipError_t run_head(const float* in, const float* w, float bias, size_t npix, int c, float* logits, float* probs,
                    uint8_t* mask, float thr, hipStream_t s, const float* biasPtr = nullptr) {
  int lpp = 1;
  while (lpp < 16 && lpp * 2 * 4 <= c) lpp *= 2;
  const unsigned g = grid_for(npix, 256 / lpp);
  prof_begin("head1x1", 2.0 * npix * c, 4.0 * npix * (c + 1), s);
#define HEAD(L)                                                                                              \
  hipLaunchKernelGGL((unet::head1x1_kernel<L>), dim3(g), dim3(256), 0, s, in, w, bias, biasPtr, npix, c, logits, \
                     probs, mask, thr)
  switch (lpp) {
    case 1: HEAD(1); break;
    case 2: HEAD(2); break;
    case 4: HEAD(4); break;
    case 8: HEAD(8); break;
    default: HEAD(16); break;
  }
#undef HEAD
  prof_end(s);
  return hipGetLastError();
}

struct ParamSpec {
  std::string name;
  size_t numel;
};

}  // namespace

// ------------------------------------------------------------------------------------------
// Context
// ------------------------------------------------------------------------------------------
struct TrainState;
struct Bf16Net;
struct X3Net;
static void train_free(unet_ctx* h);
static void bf16_free(unet_ctx* h);
static void x3_free(unet_ctx* h);

struct unet_ctx {
  TrainState* train = nullptr;
  Bf16Net* bf = nullptr;
  X3Net* x3 = nullptr;
  unet_config cfg{};
  std::vector<ParamSpec> spec;
  std::map<std::string, std::vector<float>> params;
  bool finalized = false;

  std::vector<GemmOp> enc;  // 2 per level
  std::vector<GemmOp> bott; // 2
  std::vector<GemmOp> up;   // 1 per level (decoder order: deepest first)
  std::vector<GemmOp> dec;  // 2 per level (decoder order)
  float* headW = nullptr;
  float headB = 0.f;
  float* headBk = nullptr;   // out_channels > 1: the K biases on the device

  GrowBuf ws;   // workspace

  std::string err;
  Profiler prof;
  // Device-visible error block (pinned host memory mapped into the device).  Word 0: a kernel whose bounded
  // wave-progress wait gives up stores a non-zero value here instead of silently continuing with stale data; the next
  // entry point that sees it returns UNET_ERR_HIP and clears it (the failing launch may be an earlier one: like an
  // asynchronous HIP error).  Word 1: an f16x3 kernel had to store an activation beyond the fp16 range
  // (conv_x3_ws.h); only unet_device_error, which synchronises first and can therefore name the call, reports it
  // (UNET_ERR_RANGE) and clears it.
  unsigned* errHost = nullptr;
  unsigned* errDev = nullptr;
  unsigned* rangeKeys = nullptr;   // calibration pass (unet_forward_u8_ranges): 2 order keys per activation tensor
  // histogram pass (unet_forward_u8_histograms), armed while hist is set: (lo, hi) per tensor on the host, bins + 1
  // words per tensor on the device
  unsigned long long* hist = nullptr;
  const float* histSpans = nullptr;
  int histBins = 0;
  void ensure_err_word() {
    if (errHost) return;
    if (hipHostMalloc((void**)&errHost, 2 * sizeof(unsigned), hipHostMallocMapped) != hipSuccess) {
      errHost = nullptr;
      return;
    }
    errHost[0] = errHost[1] = 0;
    if (hipHostGetDevicePointer((void**)&errDev, errHost, 0) != hipSuccess) errDev = nullptr;
  }
  int async_error() {
    volatile unsigned* w = errHost;
    if (w && w[0]) {
      w[0] = 0;   // reported once: a transient failure must not fail every later call
      err = "a bounded wave-progress wait timed out inside a kernel: the results of that launch are invalid";
      return UNET_ERR_HIP;
    }
    return UNET_OK;
  }
  // after a device synchronisation: everything the launches so far have reported, cleared
  int take_device_status() {
    volatile unsigned* w = errHost;
    if (!w) return UNET_OK;
    const unsigned timeout = w[0], range = w[1];
    w[0] = 0;
    w[1] = 0;
    if (timeout) {
      err = "a bounded wave-progress wait timed out inside a kernel: the results of that launch are invalid";
      return UNET_ERR_HIP;
    }
    if (range) {
      err = "f16x3 tier: an activation left the fp16 range (|v| > 65504); the results are not at fp32 parity - run "
            "these frames on the fp32 tier";
      return UNET_ERR_RANGE;
    }
    return UNET_OK;
  }

  void free_all() {
    if (errHost) hipHostFree(errHost);
    errHost = errDev = nullptr;
    for (auto* v : {&enc, &bott, &up, &dec})
      for (auto& op : *v) op.free_dev();
    if (headW) hipFree(headW);
    if (headBk) hipFree(headBk);
    headW = headBk = nullptr;
    ws.release();
  }
};

namespace {

// Single-class and K-class handles have entry points of their own (include/unet_hip.h, "multi-class segmentation"): the
// refusal of a call on the other kind, before any device is touched.  UNET_OK where the call may go on.
int single_class_only(unet_ctx* h, const char* who) {
  if (!h || h->cfg.out_channels == 1) return UNET_OK;
  h->err = std::string(who) + ": this entry point serves out_channels == 1; a handle with " +
           std::to_string(h->cfg.out_channels) + " classes runs unet_forward_classes_* and unet_train_forward_backward_labels_*";
  return UNET_ERR_INVALID_ARG;
}
int multi_class_only(unet_ctx* h, const char* who) {
  if (!h || h->cfg.out_channels > 1) return UNET_OK;
  h->err = std::string(who) + ": this entry point serves out_channels >= 2; the handle has the single-class head";
  return UNET_ERR_INVALID_ARG;
}

// what a K-class forward writes (every pointer optional)
struct ClassOut {
  float* logits = nullptr;
  float* probs = nullptr;
  uint8_t* labels = nullptr;
  int maskClass = 0;
  uint8_t* mask = nullptr;
};

// Profiler and error word of handle `h` become the calling thread's launch context for the scope's lifetime.
struct LaunchScope {
  Profiler* prevProf;
  unsigned* prevErr;
  explicit LaunchScope(unet_ctx* h) : prevProf(g_prof), prevErr(g_errWord) {
    h->ensure_err_word();
    g_prof = h->prof.on ? &h->prof : nullptr;
    g_errWord = h->errDev;
  }
  ~LaunchScope() {
    g_prof = prevProf;
    g_errWord = prevErr;
  }
};

void add_double_conv(std::vector<ParamSpec>& spec, const std::string& prefix, int cin, int cout) {
  const int convIdx[2] = {0, 3}, bnIdx[2] = {1, 4};
  for (int k = 0; k < 2; ++k) {
    const int ci = k == 0 ? cin : cout;
    spec.push_back({prefix + "." + std::to_string(convIdx[k]) + ".weight", (size_t)cout * ci * 9});
    for (const char* leaf : {"weight", "bias", "running_mean", "running_var"})
      spec.push_back({prefix + "." + std::to_string(bnIdx[k]) + "." + leaf, (size_t)cout});
  }
}

// Same key set as the reference module's state_dict minus the integer num_batches_tracked counters.
std::vector<ParamSpec> build_spec(const unet_config& c) {
  std::vector<ParamSpec> spec;
  int cin = c.in_channels;
  for (int i = 0; i < c.depth; ++i) {
    add_double_conv(spec, "encoder_blocks." + std::to_string(i), cin, c.features[i]);
    cin = c.features[i];
  }
  for (int j = 0; j < c.depth; ++j) {
    const int f = c.features[c.depth - 1 - j];
    spec.push_back({"decoder_blocks." + std::to_string(2 * j) + ".weight", (size_t)2 * f * f * 4});
    spec.push_back({"decoder_blocks." + std::to_string(2 * j) + ".bias", (size_t)f});
    add_double_conv(spec, "decoder_blocks." + std::to_string(2 * j + 1), 2 * f, f);
  }
  add_double_conv(spec, "bottleneck", c.features[c.depth - 1], 2 * c.features[c.depth - 1]);
  spec.push_back({"output.weight", (size_t)c.out_channels * c.features[0]});
  spec.push_back({"output.bias", (size_t)c.out_channels});
  return spec;
}

// Workspace layout for (n,h,w): offsets in floats.
struct WsPlan {
  size_t x0 = 0;                // (N,H,W,4)
  std::vector<size_t> cat, pool;  // per level
  size_t tmpA = 0, tmpB = 0;
  size_t total = 0;
};

WsPlan plan_ws(const unet_config& c, int n, int h, int w) {
  WsPlan p;
  size_t off = 0;
  auto take = [&](size_t floats) {
    size_t o = off;
    off += (floats + 63) / 64 * 64;  // 256-byte granules
    return o;
  };
  const size_t px0 = (size_t)n * h * w;
  p.x0 = take(px0 * 4);
  size_t maxT = 0;
  for (int l = 0; l < c.depth; ++l) {
    const size_t px = px0 >> (2 * l);
    p.cat.push_back(take(px * 2 * c.features[l]));
    p.pool.push_back(take((px >> 2) * c.features[l]));
    maxT = std::max(maxT, px * c.features[l]);
  }
  maxT = std::max(maxT, (px0 >> (2 * c.depth)) * 2 * c.features[c.depth - 1]);
  p.tmpA = take(maxT);
  p.tmpB = take(maxT);
  p.total = off;
  return p;
}

// eval BatchNorm (x - mean) / sqrt(var + eps) * gamma + beta (reference README.md:1453) of the module named `bn`
// ("....1.") as a scale and shift per channel; every tier folds through here, so they agree to the bit
void fold_bn(std::map<std::string, std::vector<float>>& P, const std::string& bn, int c, std::vector<float>& sc,
             std::vector<float>& sh) {
  const auto &g = P[bn + "weight"], &b = P[bn + "bias"], &m = P[bn + "running_mean"], &v = P[bn + "running_var"];
  sc.resize(c);
  sh.resize(c);
  for (int i = 0; i < c; ++i) {
    const float inv = 1.0f / std::sqrt(v[i] + kBnEps);
    sc[i] = g[i] * inv;
    sh[i] = b[i] - m[i] * sc[i];
  }
}

int fold_bn_and_build(unet_ctx* h, GemmOp& op, const std::string& prefix, int convIdx, int bnIdx, int cin, int cout) {
  const auto& w = h->params[prefix + "." + std::to_string(convIdx) + ".weight"];
  std::vector<float> sc, sh;
  fold_bn(h->params, prefix + "." + std::to_string(bnIdx) + ".", cout, sc, sh);
  return build_conv3x3(h->err, op, w.data(), cout, cin, sc.data(), sh.data(), 1);
}

int forward_common(unet_ctx* h, int n, int height, int width, float* logits, float* probs, uint8_t* mask,
                   float thr, hipStream_t s, const WsPlan& p, const ClassOut* classes = nullptr) {
  const unet_config& c = h->cfg;
  LaunchScope scope(h);
  float* ws = reinterpret_cast<float*>(h->ws.p);
  const float* cur = ws + p.x0;
  int ch = height, cw = width;
  float* tmpA = ws + p.tmpA;
  float* tmpB = ws + p.tmpB;
  // calibration passes, on tensor `idx` (order: quant.tensor_names) right after it has been produced: its (min, max),
  // or its histogram over the span the caller gave for it
  hipError_t histStatus = hipSuccess;   // the first failing histogram launch, reported when the walk is through
  auto probe = [&](int idx, const float* x, size_t npx, int cc, int ld) {
    if (h->hist) {
      // the input is counted over its real channels: the pad channel of the NHWC4 image would add 25 % exact zeros
      // that the int8 input never holds
      const hipError_t e = unet::launch_histogram_f32(x, npx, idx == 0 ? c.in_channels : cc, ld, h->histSpans[2 * idx],
                                                      h->histSpans[2 * idx + 1], h->histBins,
                                                      h->hist + (size_t)idx * (h->histBins + 1), s);
      if (histStatus == hipSuccess) histStatus = e;
      return;
    }
    if (!h->rangeKeys) return;
    hipLaunchKernelGGL(unet::minmax_f32_kernel, dim3(grid_for(npx * cc)), dim3(256), 0, s, x, npx, cc, ld,
                       h->rangeKeys + 2 * idx);
  };
  const int D = c.depth;
  probe(0, cur, (size_t)n * height * width, 4, 4);
  for (int l = 0; l < c.depth; ++l) {
    const int f = c.features[l];
    float* cat = ws + p.cat[l];
    float* pool = ws + p.pool[l];
    HIPCHK(h->err, run_gemm_op(h->enc[2 * l], cur, n, ch, cw, tmpA, f, 0, s));
    probe(1 + 2 * l, tmpA, (size_t)n * ch * cw, f, f);
    if (wino_applicable(h->enc[2 * l + 1], ch, cw) && wino_fits(h->enc[2 * l + 1], n, ch, cw)) {
      // the 2x2 output tile of the Winograd kernel is one pooling window: pooled copy written from registers
      HIPCHK(h->err, run_wino(h->enc[2 * l + 1], tmpA, n, ch, cw, cat, 2 * f, 0, pool, s));
    } else {
      HIPCHK(h->err, run_gemm_op(h->enc[2 * l + 1], tmpA, n, ch, cw, cat, 2 * f, 0, s));  // skip half of concat
      HIPCHK(h->err, run_maxpool(cat, pool, n, ch, cw, f, 2 * f, s));
    }
    cur = pool;
    ch /= 2;
    cw /= 2;
  }
  const int fb = 2 * c.features[c.depth - 1];
  HIPCHK(h->err, run_gemm_op(h->bott[0], cur, n, ch, cw, tmpA, fb, 0, s));
  probe(1 + 2 * D, tmpA, (size_t)n * ch * cw, fb, fb);
  HIPCHK(h->err, run_gemm_op(h->bott[1], tmpA, n, ch, cw, tmpB, fb, 0, s));
  probe(2 + 2 * D, tmpB, (size_t)n * ch * cw, fb, fb);
  cur = tmpB;
  for (int j = 0; j < c.depth; ++j) {
    const int l = c.depth - 1 - j;
    const int f = c.features[l];
    float* cat = ws + p.cat[l];
    // ConvTranspose writes the upper channel half of the concat buffer: torch.cat([skip, x]) elided
    HIPCHK(h->err, run_gemm_op(h->up[j], cur, n, ch, cw, cat, 2 * f, f, s));
    ch *= 2;
    cw *= 2;
    probe(2 + 2 * l, cat, (size_t)n * ch * cw, 2 * f, 2 * f);   // skip half and upconv half: one concat tensor
    HIPCHK(h->err, run_gemm_op(h->dec[2 * j], cat, n, ch, cw, tmpA, f, 0, s));
    probe(3 + 2 * D + 2 * j, tmpA, (size_t)n * ch * cw, f, f);
    HIPCHK(h->err, run_gemm_op(h->dec[2 * j + 1], tmpA, n, ch, cw, tmpB, f, 0, s));
    probe(4 + 2 * D + 2 * j, tmpB, (size_t)n * ch * cw, f, f);
    cur = tmpB;
  }
  if (classes) {   // out_channels > 1
    const size_t npx = (size_t)n * height * width;
    prof_begin("headk", 2.0 * npx * c.features[0] * c.out_channels, 4.0 * npx * c.features[0], s);
    const hipError_t e = unet::launch_headk(cur, h->headW, h->headBk, n, (size_t)height * width, c.features[0], c.out_channels,
                                            classes->logits, classes->probs, classes->labels, classes->maskClass,
                                            classes->mask, s);
    prof_end(s);
    HIPCHK(h->err, e);
  } else {
    HIPCHK(h->err, run_head(cur, h->headW, h->headB, (size_t)n * height * width, c.features[0], logits, probs, mask,
                            thr, s));
  }
  HIPCHK(h->err, histStatus);
  return h->async_error();
}

int check_shape(unet_ctx* h, int n, int height, int width) {
  const int m = 1 << h->cfg.depth;
  if (n <= 0 || height <= 0 || width <= 0) {
    h->err = "batch and spatial sizes must be positive";
    return UNET_ERR_INVALID_ARG;
  }
  if (height % m || width % m) {
    h->err = "H and W must be multiples of " + std::to_string(m);
    return UNET_ERR_SHAPE;
  }
  return UNET_OK;
}

}  // namespace

extern "C" {

int unet_set_winograd(int on) {
  const int prev = wino_enabled() ? 1 : 0;
  g_winoMode = on ? 1 : 0;
  return prev;
}

const char* unet_version(void) { return "unet_hip 0.1 (gfx950, fp32 MFMA implicit GEMM)"; }

int unet_create(const unet_config* cfg, unet_handle_t* out) {
  if (!cfg || !out) return UNET_ERR_INVALID_ARG;
  if (cfg->depth < 1 || cfg->depth > UNET_MAX_DEPTH || cfg->out_channels < 1 || cfg->out_channels > UNET_MAX_CLASSES ||
      cfg->in_channels < 1 || cfg->in_channels > 4)
    return UNET_ERR_INVALID_ARG;
  for (int i = 0; i < cfg->depth; ++i)
    if (cfg->features[i] <= 0 || cfg->features[i] % 4) return UNET_ERR_INVALID_ARG;
  for (int i = 0; i + 1 < cfg->depth; ++i)  // ConvTranspose2d(2f -> f) feeds on the level below: widths must double
    if (cfg->features[i + 1] != 2 * cfg->features[i]) return UNET_ERR_INVALID_ARG;
  if (cfg->device < 0) return UNET_ERR_INVALID_ARG;  // the device itself is first touched by unet_finalize
  // the K-way head keeps its K * f0 weights in LDS (csrc/multiclass_kernels.h)
  if (cfg->out_channels > 1 && (long long)cfg->out_channels * cfg->features[0] > unet::MC_MAX_WEIGHTS) return UNET_ERR_INVALID_ARG;
  auto* h = new unet_ctx();
  h->cfg = *cfg;
  h->spec = build_spec(*cfg);
  *out = h;
  return UNET_OK;
}

int unet_num_params(unet_handle_t h) { return h ? (int)h->spec.size() : 0; }
const char* unet_param_name(unet_handle_t h, int i) {
  return (h && i >= 0 && i < (int)h->spec.size()) ? h->spec[i].name.c_str() : nullptr;
}
size_t unet_param_numel(unet_handle_t h, int i) {
  return (h && i >= 0 && i < (int)h->spec.size()) ? h->spec[i].numel : 0;
}

int unet_load_param(unet_handle_t h, const char* name, const float* data, size_t numel) {
  if (!h || !name || !data) return UNET_ERR_INVALID_ARG;
  for (const auto& s : h->spec) {
    if (s.name == name) {
      if (s.numel != numel) {
        h->err = std::string(name) + ": expected " + std::to_string(s.numel) + " elements, got " + std::to_string(numel);
        return UNET_ERR_SHAPE;
      }
      h->params[s.name].assign(data, data + numel);
      h->finalized = false;
      return UNET_OK;
    }
  }
  h->err = std::string("unknown parameter ") + name;
  return UNET_ERR_UNKNOWN_PARAM;
}

int unet_finalize(unet_handle_t h) {
  if (!h) return UNET_ERR_INVALID_ARG;
  for (const auto& s : h->spec)
    if (!h->params.count(s.name)) {
      h->err = "missing parameter " + s.name;
      return UNET_ERR_STATE;
    }
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  const unet_config& c = h->cfg;
  // the other tiers pack their operands lazily from h->params (and the bf16 tier borrows this tier's scale/shift
  // arrays): drop them so that they are rebuilt from the tensors being finalised now
  bf16_free(h);
  x3_free(h);
  for (auto* v : {&h->enc, &h->bott, &h->up, &h->dec})
    for (auto& op : *v) op.free_dev();
  h->enc.assign(2 * c.depth, GemmOp());
  h->dec.assign(2 * c.depth, GemmOp());
  h->up.assign(c.depth, GemmOp());
  h->bott.assign(2, GemmOp());
  int rc;
  int cin = c.in_channels;
  for (int l = 0; l < c.depth; ++l) {
    const std::string p = "encoder_blocks." + std::to_string(l);
    if ((rc = fold_bn_and_build(h, h->enc[2 * l], p, 0, 1, cin, c.features[l]))) return rc;
    if ((rc = fold_bn_and_build(h, h->enc[2 * l + 1], p, 3, 4, c.features[l], c.features[l]))) return rc;
    cin = c.features[l];
  }
  const int fl = c.features[c.depth - 1];
  if ((rc = fold_bn_and_build(h, h->bott[0], "bottleneck", 0, 1, fl, 2 * fl))) return rc;
  if ((rc = fold_bn_and_build(h, h->bott[1], "bottleneck", 3, 4, 2 * fl, 2 * fl))) return rc;
  for (int j = 0; j < c.depth; ++j) {
    const int f = c.features[c.depth - 1 - j];
    const std::string pu = "decoder_blocks." + std::to_string(2 * j);
    if ((rc = build_upconv(h->err, h->up[j], h->params[pu + ".weight"].data(), 2 * f, f,
                           h->params[pu + ".bias"].data())))
      return rc;
    const std::string pd = "decoder_blocks." + std::to_string(2 * j + 1);
    if ((rc = fold_bn_and_build(h, h->dec[2 * j], pd, 0, 1, 2 * f, f))) return rc;
    if ((rc = fold_bn_and_build(h, h->dec[2 * j + 1], pd, 3, 4, f, f))) return rc;
  }
  if (h->headW) hipFree(h->headW);
  h->headW = nullptr;
  if ((rc = upload(h->err, &h->headW, h->params["output.weight"]))) return rc;
  h->headB = h->params["output.bias"][0];
  if (h->headBk) hipFree(h->headBk);
  h->headBk = nullptr;
  if (c.out_channels > 1 && (rc = upload(h->err, &h->headBk, h->params["output.bias"]))) return rc;
  h->finalized = true;
  return UNET_OK;
}

size_t unet_workspace_bytes(unet_handle_t h, int n, int height, int width) {
  if (!h || check_shape(h, n, height, width)) return 0;
  return plan_ws(h->cfg, n, height, width).total * sizeof(float);
}

int unet_reserve(unet_handle_t h, int n, int height, int width) {
  if (!h) return UNET_ERR_INVALID_ARG;
  int rc = check_shape(h, n, height, width);
  if (rc) return rc;
  const size_t need = plan_ws(h->cfg, n, height, width).total * sizeof(float);
  if (need <= h->ws.bytes) return UNET_OK;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  return h->ws.reserve(h->err, need, "workspace");
}

static int forward_prologue(unet_handle_t h, const void* in, int n, int height, int width) {
  if (!h || !in) return UNET_ERR_INVALID_ARG;
  if (!h->finalized) {
    h->err = "unet_finalize has not been called";
    return UNET_ERR_STATE;
  }
  int rc = check_shape(h, n, height, width);
  if (rc) return rc;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  return unet_reserve(h, n, height, width);
}

int unet_forward_u8(unet_handle_t h, const uint8_t* frames, int n, int height, int width, float* logits,
                    float* probs, uint8_t* mask, float thr, void* stream) {
  int rc = single_class_only(h, "unet_forward_u8");
  if (!rc) rc = forward_prologue(h, frames, n, height, width);
  if (rc) return rc;
  if (h->cfg.in_channels != 3) {
    h->err = "uint8 frames need in_channels == 3";
    return UNET_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const WsPlan p = plan_ws(h->cfg, n, height, width);
  const size_t npix = (size_t)n * height * width;
  const unet_config& c = h->cfg;
  hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames,
                     reinterpret_cast<float*>(h->ws.p) + p.x0, npix, c.input_mean[0], c.input_mean[1], c.input_mean[2],
                     c.input_std[0], c.input_std[1], c.input_std[2]);
  HIPCHK(h->err, hipGetLastError());
  return forward_common(h, n, height, width, logits, probs, mask, thr, s, p);
}

int unet_forward_f32(unet_handle_t h, const float* image, int n, int height, int width, float* logits, float* probs,
                     uint8_t* mask, float thr, void* stream) {
  int rc = single_class_only(h, "unet_forward_f32");
  if (!rc) rc = forward_prologue(h, image, n, height, width);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const WsPlan p = plan_ws(h->cfg, n, height, width);
  const size_t npix = (size_t)n * height * width;
  hipLaunchKernelGGL(unet::pack_nchw_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, image,
                     reinterpret_cast<float*>(h->ws.p) + p.x0, n, (size_t)height * width, h->cfg.in_channels);
  HIPCHK(h->err, hipGetLastError());
  return forward_common(h, n, height, width, logits, probs, mask, thr, s, p);
}

// csrc/unet_x3.inc
namespace {
int forward_x3(unet_ctx* h, const void* input, bool u8, int n, int height, int width, float* logits, float* probs,
               uint8_t* mask, float thr, hipStream_t s, const ClassOut* classes);
}

// the checks of a K-class forward that need no device
static int classes_prologue(unet_handle_t h, const char* who, int precision, int maskClass, const uint8_t* mask) {
  if (!h) return UNET_ERR_INVALID_ARG;
  if (int rc = multi_class_only(h, who)) return rc;
  if (precision != 0 && precision != 1) {
    h->err = std::string(who) + ": the K-class forward runs on the fp32 tier (precision 0) and the f16x3 tier (1)";
    return UNET_ERR_INVALID_ARG;
  }
  if (mask && (maskClass < 0 || maskClass >= h->cfg.out_channels)) {
    h->err = std::string(who) + ": mask_class must name a class of the handle";
    return UNET_ERR_INVALID_ARG;
  }
  return UNET_OK;
}

int unet_forward_classes_u8(unet_handle_t h, const uint8_t* frames, int n, int height, int width, int precision,
                            float* logits, float* probs, uint8_t* labels, int maskClass, uint8_t* mask, void* stream) {
  int rc = classes_prologue(h, "unet_forward_classes_u8", precision, maskClass, mask);
  if (rc) return rc;
  ClassOut co;
  co.logits = logits, co.probs = probs, co.labels = labels, co.maskClass = maskClass, co.mask = mask;
  if (precision == 1) return forward_x3(h, frames, true, n, height, width, nullptr, nullptr, nullptr, 0.f, (hipStream_t)stream, &co);
  if ((rc = forward_prologue(h, frames, n, height, width))) return rc;
  if (h->cfg.in_channels != 3) {
    h->err = "uint8 frames need in_channels == 3";
    return UNET_ERR_INVALID_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const WsPlan p = plan_ws(h->cfg, n, height, width);
  const size_t npix = (size_t)n * height * width;
  const unet_config& c = h->cfg;
  hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames,
                     reinterpret_cast<float*>(h->ws.p) + p.x0, npix, c.input_mean[0], c.input_mean[1], c.input_mean[2],
                     c.input_std[0], c.input_std[1], c.input_std[2]);
  HIPCHK(h->err, hipGetLastError());
  return forward_common(h, n, height, width, nullptr, nullptr, nullptr, 0.f, s, p, &co);
}

int unet_forward_classes_f32(unet_handle_t h, const float* image, int n, int height, int width, int precision,
                             float* logits, float* probs, uint8_t* labels, int maskClass, uint8_t* mask, void* stream) {
  int rc = classes_prologue(h, "unet_forward_classes_f32", precision, maskClass, mask);
  if (rc) return rc;
  ClassOut co;
  co.logits = logits, co.probs = probs, co.labels = labels, co.maskClass = maskClass, co.mask = mask;
  if (precision == 1) return forward_x3(h, image, false, n, height, width, nullptr, nullptr, nullptr, 0.f, (hipStream_t)stream, &co);
  if ((rc = forward_prologue(h, image, n, height, width))) return rc;
  hipStream_t s = (hipStream_t)stream;
  const WsPlan p = plan_ws(h->cfg, n, height, width);
  const size_t npix = (size_t)n * height * width;
  hipLaunchKernelGGL(unet::pack_nchw_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, image,
                     reinterpret_cast<float*>(h->ws.p) + p.x0, n, (size_t)height * width, h->cfg.in_channels);
  HIPCHK(h->err, hipGetLastError());
  return forward_common(h, n, height, width, nullptr, nullptr, nullptr, 0.f, s, p, &co);
}

int unet_destroy(unet_handle_t h) {
  if (!h) return UNET_OK;
  hipSetDevice(h->cfg.device);
  hipDeviceSynchronize();
  train_free(h);
  bf16_free(h);
  x3_free(h);
  h->free_all();
  delete h;
  return UNET_OK;
}

int unet_profile_enable(unet_handle_t h, int on) {
  if (!h) return UNET_ERR_INVALID_ARG;
  h->prof.clear();
  h->prof.on = on != 0;
  return UNET_OK;
}

int unet_profile_count(unet_handle_t h) {
  if (!h) return 0;
  h->prof.resolve();
  return (int)h->prof.recs.size();
}

int unet_profile_get(unet_handle_t h, int i, char* name, size_t nameCap, double* ms, double* flops, double* bytes) {
  if (!h || i < 0 || i >= (int)h->prof.recs.size()) return UNET_ERR_INVALID_ARG;
  h->prof.resolve();
  const ProfRecord& r = h->prof.recs[i];
  if (name && nameCap) {
    std::strncpy(name, r.name.c_str(), nameCap - 1);
    name[nameCap - 1] = 0;
  }
  if (ms) *ms = r.ms;
  if (flops) *flops = r.flops;
  if (bytes) *bytes = r.bytes;
  return UNET_OK;
}

const char* unet_last_error(unet_handle_t h) { return h ? h->err.c_str() : "null handle"; }

int unet_device_error(unet_handle_t h) {
  if (!h) return UNET_ERR_INVALID_ARG;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  HIPCHK(h->err, hipDeviceSynchronize());
  return h->take_device_status();
}

int unet_device_error_on(unet_handle_t h, void* stream) {
  if (!h) return UNET_ERR_INVALID_ARG;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  HIPCHK(h->err, hipStreamSynchronize((hipStream_t)stream));
  return h->take_device_status();
}

namespace {
__global__ void status_word_kernel(const unsigned* __restrict__ err, float* __restrict__ dst) {
  const volatile unsigned* e = err;
  *dst = (e[0] | e[1]) ? 1.f : 0.f;
}
}  // namespace

int unet_device_status_to(unet_handle_t h, float* dst, void* stream) {
  if (!h || !dst) return UNET_ERR_INVALID_ARG;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  h->ensure_err_word();
  if (!h->errDev) return UNET_ERR_NOMEM;
  hipLaunchKernelGGL(status_word_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (const unsigned*)h->errDev, dst);
  HIPCHK(h->err, hipGetLastError());
  return UNET_OK;
}

int unet_debug_set_error_block(unet_handle_t h, int word, unsigned value) {
  if (!h || word < 0 || word > 1) return UNET_ERR_INVALID_ARG;
  h->ensure_err_word();
  if (!h->errHost) return UNET_ERR_NOMEM;
  reinterpret_cast<volatile unsigned*>(h->errHost)[word] = value;
  return UNET_OK;
}

}  // extern "C"

// ---- single operators (test entry points) -------------------------------------------------
//
// The handle-less entry points of all four files (unet_op_*, the loss, metric and camera helpers) share what follows:
// g_opErr is the text of the calling thread's last failure (unet_op_last_error), OpScratch owns the device memory of one
// call, OpGuard the operator built for it, and op_done is the one exit that turns the launches' hipError_t into a status.

static thread_local std::string g_opErr;

// declared in op_entry.h for the handle-less entry points of the *_kernels.cpp translation units; not exported
namespace unet {
int op_fail(int status, const std::string& text) {
  g_opErr = text;
  return status;
}
}  // namespace unet
// what an entry point returns for arguments its own checks refuse (before any device work)
static int op_bad_args() { return unet::op_fail(UNET_ERR_INVALID_ARG, "invalid argument: refused by the entry point's checks"); }

namespace {

// Every device allocation of one call, freed when it returns, on every path.  Zeroing, where asked, is on the call's stream.
struct OpScratch {
  hipStream_t s;
  std::vector<void*> all;
  explicit OpScratch(hipStream_t stream) : s(stream) {}
  OpScratch(const OpScratch&) = delete;
  OpScratch& operator=(const OpScratch&) = delete;
  ~OpScratch() {
    for (void* q : all) hipFree(q);
  }
  template <class T>
  hipError_t get(T** p, size_t bytes, bool zero = false) {
    bytes = std::max<size_t>(bytes, 64);
    hipError_t e = hipMalloc((void**)p, bytes);
    if (e != hipSuccess) return e;
    all.push_back(*p);
    return zero ? hipMemsetAsync(*p, 0, bytes, s) : hipSuccess;
  }
  // `count` host elements, copied before the call returns to the caller's launches
  template <class T>
  hipError_t upload(T** p, const T* host, size_t count) {
    hipError_t e = get(p, count * sizeof(T));
    return e == hipSuccess ? hipMemcpy(*p, host, count * sizeof(T), hipMemcpyHostToDevice) : e;
  }
  // a buffer that one of the tiers' own pack functions allocated for this call
  void adopt(void* p) {
    if (p) all.push_back(p);
  }
  // the zero page the kernels read for an out-of-image halo (x3_build: 4096 bytes; bf16_build: 8192 elements)
  hipError_t zero_page(uint16_t** p, size_t bytes = 4096) { return get(p, bytes, true); }
};

// The operator a call builds (GemmOp, GemmOpBf, GemmOpX3, DecStepX3): its device arrays are released on every exit
template <class Op>
struct OpGuard {
  Op op;
  OpGuard() = default;
  OpGuard(const OpGuard&) = delete;
  ~OpGuard() { op.free_dev(); }
};

// fp32 dense tensor -> fp16 hi / lo planes (lo plane `elems` halfs behind the hi plane, together the bytes of the fp32
// tensor).  absmaxKey / inv: for tensors far below the fp16 range (gradients): scaled by the power of two that
// brings the maximum to ~2^13, its inverse left in *inv.
void split_to_planes(const float* x, size_t elems, void* planes, hipStream_t s, const unsigned* absmaxKey = nullptr,
                     float* inv = nullptr) {
  uint16_t* hi = reinterpret_cast<uint16_t*>(planes);
  prof_begin("split_planes", 0.0, 8.0 * elems, s);
  if (absmaxKey)
    hipLaunchKernelGGL(unet::split_planes_scaled_kernel, dim3(grid_for(elems / 2)), dim3(256), 0, s, x, elems / 2,
                       reinterpret_cast<uint32_t*>(hi), reinterpret_cast<uint32_t*>(hi + elems), absmaxKey, inv);
  else
    hipLaunchKernelGGL(unet::split_planes_kernel, dim3(grid_for(elems / 2)), dim3(256), 0, s, x, elems / 2,
                       reinterpret_cast<uint32_t*>(hi), reinterpret_cast<uint32_t*>(hi + elems));
  prof_end(s);
}
// ... and back: planes laid out the same way -> fp32 dense tensor
void merge_from_planes(const void* planes, size_t elems, float* y, hipStream_t s) {
  const uint16_t* hi = reinterpret_cast<const uint16_t*>(planes);
  hipLaunchKernelGGL(unet::merge_planes_kernel, dim3(grid_for(elems / 2)), dim3(256), 0, s,
                     reinterpret_cast<const uint32_t*>(hi), reinterpret_cast<const uint32_t*>(hi + elems), elems / 2, y);
}

// The plane-level test entry points (unet_op_*_x3_planes) watch the range with a word of their own: for the scope's
// lifetime the calling thread's launches report into it instead of the per-device word of the other entry points
struct OpRangeScope {
  unsigned* dev = nullptr;
  unsigned* prev = nullptr;
  bool armed = false;
  hipError_t arm() {
    hipError_t e = hipMalloc((void**)&dev, 2 * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(dev, 0, 2 * sizeof(unsigned));
    if (e != hipSuccess) return e;
    prev = g_errWord;
    g_errWord = dev;
    armed = true;
    return hipSuccess;
  }
  // after the stream has been synchronised: did a kernel of the call set word 1?
  hipError_t read(int* rangeOut) {
    unsigned host[2] = {0, 0};
    const hipError_t e = hipMemcpy(host, dev, sizeof(host), hipMemcpyDeviceToHost);
    if (e == hipSuccess && rangeOut) *rangeOut = host[1] != 0 ? 1 : 0;
    return e;
  }
  ~OpRangeScope() {
    if (armed) g_errWord = prev;
    if (dev) hipFree(dev);
  }
};

// The one exit of a handle-less entry point.  `e`: what the call's allocations and launches returned.  The stream is
// synchronised (also after a failure: the scratch is freed when the caller returns) unless kOpNoSync says that the entry
// point is asynchronous; then an armed `range` is read into *rangeOut.  A failure leaves its text in g_opErr and is
// UNET_ERR_HIP, or with kOpMapCodes UNET_ERR_INVALID_ARG / UNET_ERR_NOMEM for the runtime's codes of those names.
// kOpWaitWord: the call may have launched wino_f32_kernel with the per-device error word (op_err_word): word 0 is read
// back after the synchronisation, and a bounded wait that gave up is UNET_ERR_HIP with a text that says so; the word is
// cleared for the next call.
enum : unsigned { kOpNoSync = 1, kOpMapCodes = 2, kOpWaitWord = 4 };
int op_done(hipError_t e, hipStream_t s, unsigned flags = 0, OpRangeScope* range = nullptr, int* rangeOut = nullptr) {
  if (!(flags & kOpNoSync)) {
    const hipError_t es = hipStreamSynchronize(s);
    if (e == hipSuccess) e = es;
  }
  if (e == hipSuccess && range) e = range->read(rangeOut);
  if (e == hipSuccess && (flags & kOpWaitWord) && !(flags & kOpNoSync)) {
    unsigned* word = g_errWord ? g_errWord : op_err_word();
    unsigned gaveUp = 0;
    if (word) e = hipMemcpy(&gaveUp, word, sizeof(gaveUp), hipMemcpyDeviceToHost);
    if (e == hipSuccess && gaveUp) {
      hipMemset(word, 0, sizeof(unsigned));
      g_opErr = "a bounded wave-progress wait gave up inside wino_f32_kernel: the results of this call are invalid";
      return UNET_ERR_HIP;
    }
  }
  if (e == hipSuccess) return UNET_OK;
  g_opErr = hipGetErrorString(e);
  if (flags & kOpMapCodes) {
    if (e == hipErrorInvalidValue) return UNET_ERR_INVALID_ARG;
    if (e == hipErrorOutOfMemory) return UNET_ERR_NOMEM;
  }
  return UNET_ERR_HIP;
}

}  // namespace

namespace {

// plain 1x1 convolution (an ordinary GEMM over the pixels): w (O,I), no scale / shift
int build_conv1x1(std::string& err, GemmOp& op, const float* w, int cout, int cin) {
  op.free_dev();
  op.taps = 1;
  op.plain = 1;
  op.cinReal = cin;
  op.ck = (cin % 16 == 0) ? 16 : 4;
  op.cin = round_up(cin, op.ck);
  op.cout = cout;
  op.coutPad = round_up(cout, 16);
  op.nTotal = gemm_n_total(false, cout);
  auto packed = pack_fragments(op.nTotal, op.cin, op.ck, 1, [&](int nn, int ci, int) -> float {
    return (nn < cout && ci < cin) ? w[(size_t)nn * cin + ci] : 0.f;
  });
  std::vector<float> sc(op.nTotal, 1.f), sh(op.nTotal, 0.f);
  int rc = upload(err, &op.wt, packed);
  if (!rc) rc = upload(err, &op.scale, sc);
  if (!rc) rc = upload(err, &op.shift, sh);
  return rc;
}

// the output slice of the unet_op_*_f32 entry points: ldo 0 = dense; else channels [coOff, coOff + cout) of ldo
bool f32_slice_ok(int cout, int& ldo, int coOff) {
  if (ldo == 0) {
    ldo = cout;
    return coOff == 0;
  }
  return ldo % 4 == 0 && coOff % 4 == 0 && coOff >= 0 && coOff + cout <= ldo;
}

// path_out of the unet_op_*_f32 entry points and the plan of unet_host_plan_conv_f32
void f32_plan_to_ints(const F32Plan& p, bool poolFused, int* out) {
  const int v[8] = {p.algo, p.ms, p.ns, p.th, p.tw, p.grid, p.coGroup, poolFused ? 1 : 0};
  std::copy(v, v + 8, out);
}

// Which kernel a 3x3 convolution of the fp32 tier runs: 1 direct, 2 Winograd, 0 = the forced choice cannot take the
// shape.  algo 0: run_gemm_op's / the encoder's choice; 1 / 2: forced (a forced Winograd ignores unet_set_winograd).
int f32_conv_algo(int algo, int n, int h, int w, int cin) {
  const bool takes = cin % 16 == 0 && h % 2 == 0 && w % 2 == 0 && wino_fits(n, h, w, cin);
  if (algo == 2) return takes ? 2 : 0;
  if (algo == 1) return 1;
  return takes && wino_enabled() ? 2 : 1;
}

}  // namespace

extern "C" {

const char* unet_op_last_error(void) { return g_opErr.c_str(); }

int unet_op_conv3x3(int device, const float* x, int n, int h, int w, int cin, const float* wHost,
                    const float* scale, const float* shift, int cout, int relu, float* y, void* stream) {
  if (!x || !wHost || !scale || !shift || !y || cin % 4 || cout % 4) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOp> g;
  const int rc = build_conv3x3(g_opErr, g.op, wHost, cout, cin, scale, shift, relu);
  return rc ? rc : op_done(run_gemm_op(g.op, x, n, h, w, y, cout, 0, s), s, kOpWaitWord);
}

int unet_op_upconv2x2(int device, const float* x, int n, int h, int w, int cin, const float* wHost,
                      const float* bias, int cout, float* y, void* stream) {
  if (!x || !wHost || !bias || !y || cin % 4 || cout % 4) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOp> g;
  const int rc = build_upconv(g_opErr, g.op, wHost, cin, cout, bias);
  return rc ? rc : op_done(run_gemm_op(g.op, x, n, h, w, y, cout, 0, s), s);
}

int unet_op_conv1x1(int device, const float* x, int n, int h, int w, int cin, const float* wHost, int cout, float* y,
                    void* stream) {
  if (!x || !wHost || !y || cin % 4 || cout % 4) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOp> g;
  const int rc = build_conv1x1(g_opErr, g.op, wHost, cout, cin);
  return rc ? rc : op_done(run_gemm_op(g.op, x, n, h, w, y, cout, 0, s), s);
}

int unet_op_maxpool2x2(int device, const float* x, int n, int h, int w, int c, float* y, void* stream) {
  if (!x || !y || c % 4 || h % 2 || w % 2) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  return op_done(run_maxpool(x, y, n, h, w, c, c, s), s);
}

int unet_op_head1x1(int device, const float* x, int n, int h, int w, int c, const float* wHost, float bias,
                    float* logits, void* stream) {
  if (!x || !wHost || !logits || c % 4) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  float* wd = nullptr;
  hipError_t e = sc.upload(&wd, wHost, (size_t)c);
  if (e == hipSuccess) e = run_head(x, wd, bias, (size_t)n * h * w, c, logits, nullptr, nullptr, 0.f, s);
  return op_done(e, s);
}

// ---- the fp32 tier on the network's own paths (include/unet_hip.h; tests/test_f32_ops_gpu.py) ----

int unet_op_conv3x3_f32(int device, const float* x, int n, int h, int w, int cin, const float* wHost, const float* scale,
                        const float* shift, int cout, int relu, int algo, int ldo, int coOff, float* y, float* yPool,
                        int* pathOut, void* stream) {
  if (!x || !wHost || !scale || !shift || !y || n < 1 || h < 1 || w < 1 || cin < 4 || cout < 4 || cin % 4 || cout % 4 ||
      algo < 0 || algo > 2 || !f32_slice_ok(cout, ldo, coOff) || (yPool && (h % 2 || w % 2)))
    return op_bad_args();
  const int ran = f32_conv_algo(algo, n, h, w, cin);
  if (!ran) return op_bad_args();   // a forced Winograd on a shape it does not take
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOp> g;
  const int rc = build_conv3x3(g_opErr, g.op, wHost, cout, cin, scale, shift, relu);
  if (rc) return rc;
  F32Plan plan;
  hipError_t e;
  if (ran == 2) {   // the pooled copy from the output registers, as the encoder's second convolutions
    e = run_wino(g.op, x, n, h, w, y, ldo, coOff, yPool, s, &plan);
  } else {          // ... and as their else branch: the direct kernel, then the pool over the slice it wrote
    e = run_direct(g.op, x, n, h, w, y, ldo, coOff, s, 0, &plan);
    if (e == hipSuccess && yPool) e = run_maxpool(y + coOff, yPool, n, h, w, cout, ldo, s);
  }
  if (pathOut) f32_plan_to_ints(plan, ran == 2 && yPool, pathOut);
  return op_done(e, s, kOpWaitWord);
}

int unet_op_upconv2x2_f32(int device, const float* x, int n, int h, int w, int cin, const float* wHost, const float* bias,
                          int cout, int ldo, int coOff, float* y, int* pathOut, void* stream) {
  if (!x || !wHost || !bias || !y || n < 1 || h < 1 || w < 1 || cin < 4 || cout < 4 || cin % 4 || cout % 4 ||
      !f32_slice_ok(cout, ldo, coOff))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOp> g;
  const int rc = build_upconv(g_opErr, g.op, wHost, cin, cout, bias);
  if (rc) return rc;
  F32Plan plan;
  const hipError_t e = run_direct(g.op, x, n, h, w, y, ldo, coOff, s, 0, &plan);
  if (pathOut) f32_plan_to_ints(plan, false, pathOut);
  return op_done(e, s);
}

int unet_op_conv1x1_f32(int device, const float* x, int n, int h, int w, int cin, const float* wHost, int cout, int ldo,
                        int coOff, float* y, int* pathOut, void* stream) {
  if (!x || !wHost || !y || n < 1 || h < 1 || w < 1 || cin < 4 || cout < 4 || cin % 4 || cout % 4 ||
      !f32_slice_ok(cout, ldo, coOff))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOp> g;
  const int rc = build_conv1x1(g_opErr, g.op, wHost, cout, cin);
  if (rc) return rc;
  F32Plan plan;
  const hipError_t e = run_direct(g.op, x, n, h, w, y, ldo, coOff, s, 0, &plan);
  if (pathOut) f32_plan_to_ints(plan, false, pathOut);
  return op_done(e, s);
}

int unet_op_maxpool2x2_f32(int device, const float* x, int n, int h, int w, int c, int ldi, float* y, void* stream) {
  if (ldi == 0) ldi = c;
  if (!x || !y || n < 1 || h < 2 || w < 2 || c < 4 || c % 4 || h % 2 || w % 2 || ldi % 4 || ldi < c) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  return op_done(run_maxpool(x, y, n, h, w, c, ldi, s), s);
}

int unet_op_head1x1_f32(int device, const float* x, int n, int h, int w, int c, const float* wHost, float bias, float thr,
                        float* logits, float* probs, uint8_t* mask, void* stream) {
  if (!x || !wHost || (!logits && !probs && !mask) || n < 1 || h < 1 || w < 1 || c < 4 || c % 4) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  float* wd = nullptr;
  hipError_t e = sc.upload(&wd, wHost, (size_t)c);
  if (e == hipSuccess) e = run_head(x, wd, bias, (size_t)n * h * w, c, logits, probs, mask, thr, s);
  return op_done(e, s);
}

int unet_op_pack_input_f32(int device, const void* src, int isU8, int n, int h, int w, const float* mean, const float* stdv,
                           float* y, void* stream) {
  if (!src || !y || n < 1 || h < 1 || w < 1 || (isU8 && (!mean || !stdv))) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * h * w;
  if (isU8)   // as unet_forward_u8
    hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s,
                       reinterpret_cast<const uint8_t*>(src), y, npix, mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]);
  else        // as unet_forward_f32, in_channels == 3
    hipLaunchKernelGGL(unet::pack_nchw_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s,
                       reinterpret_cast<const float*>(src), y, n, (size_t)h * w, 3);
  return op_done(hipGetLastError(), s);
}

int unet_host_plan_conv_f32(const int* query, int nQuery, int* planOut, int nPlan) {
  if (!query || nQuery != 7 || !planOut || nPlan != 8) return op_bad_args();
  const int taps = query[0], n = query[1], h = query[2], w = query[3], cin = query[4], cout = query[5], algo = query[6];
  if ((taps != 9 && taps != 1 && taps != 2) || n < 1 || h < 1 || w < 1 || cin < 4 || cout < 4 || cin % 4 || cout % 4 ||
      algo < 0 || algo > 2 || (taps != 9 && algo == 2))
    return op_bad_args();
  const int ck = (cin % 16 == 0) ? 16 : 4;   // as the build_* functions
  const int nTotal = gemm_n_total(taps == 1, cout);
  const int ran = taps == 9 ? f32_conv_algo(algo, n, h, w, cin) : 1;
  if (!ran) return op_bad_args();
  f32_plan_to_ints(ran == 2 ? plan_wino(n, h, w, nTotal) : plan_direct(n, h, w, ck, taps == 9, nTotal), false, planOut);
  return UNET_OK;
}

}  // extern "C"

#include "unet_bf16.inc"
#include "unet_x3.inc"
#include "unet_train.inc"
#include "unet_i8.inc"

// ---- camera stage (camera_stage.h) ---------------------------------------------------------------------------
extern "C" {

int unet_ipm_prestage_u8(int device, const uint8_t* img, int height, int width, int step, int bgrIn,
                         const double minv[9], int warpW, int warpH, int outW, int outH, uint8_t* outRgb,
                         void* stream) {
  if (!img || !minv || !outRgb || height <= 0 || width <= 0 || step < 3 * width || warpW <= 0 || warpH <= 0 ||
      outW <= 0 || outH <= 0)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  unet::CameraArgs a;
  a.img = img;
  a.out = outRgb;
  for (int i = 0; i < 9; ++i) a.minv[i] = minv[i];
  a.scale_x = 1.0 / ((double)outW / (double)warpW);
  a.scale_y = 1.0 / ((double)outH / (double)warpH);
  a.height = height;
  a.width = width;
  a.step = step;
  a.swap_rb = bgrIn ? 1 : 0;
  a.warp_w = warpW;
  a.warp_h = warpH;
  a.out_w = outW;
  a.out_h = outH;
  hipLaunchKernelGGL(unet::ipm_prestage_kernel, dim3((unsigned)(((size_t)outW * outH + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return op_done(hipGetLastError(), (hipStream_t)stream, kOpNoSync);
}

int unet_resize_u8(int device, const uint8_t* src, int height, int width, int channels, int outW, int outH,
                   uint8_t* dst, void* stream) {
  if (!src || !dst || height <= 0 || width <= 0 || channels <= 0 || outW <= 0 || outH <= 0) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  const size_t total = (size_t)outW * outH * channels;
  hipLaunchKernelGGL(unet::resize_u8_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, src, height,
                     width, channels, 1.0 / ((double)outW / (double)width), 1.0 / ((double)outH / (double)height), outW,
                     outH, dst);
  return op_done(hipGetLastError(), (hipStream_t)stream, kOpNoSync);
}

}  // extern "C"
