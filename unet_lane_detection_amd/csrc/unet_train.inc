// Training step of the U-Net (included at the end of unet_hip.cpp; same translation unit).
//
// Follows the reference's loop body (README.md:2060-2084): zero_grad -> model(images) in train mode ->
// BCEWithLogitsLoss -> backward -> optimizer.step().  The all-reduce of a data-parallel run sits between
// unet_train_forward_backward_* and unet_train_adam_step and is done by the caller on the flat
// gradient buffer (RCCL through torch.distributed); this file never communicates.
//
// Memory contract: parameters, gradients, Adam moments and BatchNorm running statistics live in five
// caller-owned flat device buffers (PyTorch tensor layouts back to back, in unet_param_name order).

namespace {

using unet::PackArgs;
using unet::WgradArgs;

constexpr float kBnMomentum = 0.1f;  // nn.BatchNorm2d default
constexpr int kRedBlocks = 1024;     // blocks of the two-stage column reductions (4 per CU)
constexpr size_t kPartialFloats = (size_t)kRedBlocks * 2 * 4096;   // the reductions' scratch (TrainPlan::partial)

struct ConvUnit {
  std::string prefix;
  int convIdx = 0, bnIdx = 1;
  int cin = 0, cout = 0;  // real channel counts
  int level = 0;          // spatial level (0 = full resolution)
  int dbgId = 0;
  GemmOp fwd, dgrad;
  bool needDgrad = true;
  // split-operand (f16x3) copies of the two operators (csrc/conv_x3_ws.h), for Cin % 64 == 0 and Cout % 64 == 0
  uint16_t *x3Fwd = nullptr, *x3Dgrad = nullptr;
  size_t offW = 0, offG = 0, offB = 0, offRM = 0, offRV = 0;
  float *scale = nullptr, *shift = nullptr, *mean = nullptr, *invstd = nullptr;
  float *evScale = nullptr, *evShift = nullptr;   // BatchNorm folded with the running statistics (eval pass, TrainState::evalArena)
};

struct UpUnit {
  int cin = 0, cout = 0;  // ConvTranspose2d(cin = 2f, cout = f)
  GemmOp fwd, dgrad;
  uint16_t* x3Fwd = nullptr;   // split-operand copy of the forward operator (upconv_x3_ws.h), widths multiples of 64
  uint16_t* x3Dgrad = nullptr; // ... and of its input gradient as a plain GEMM (pack_upconv_dgrad_x3_kernel)
  size_t offW = 0, offB = 0;
};

struct TrainPlan {
  size_t x0 = 0;
  size_t gzPlanes = 0;  // hi/lo planes of the current unit's dZ (f16x3 weight and input gradients)
  size_t gzPlanes2 = 0; // its twin: units alternate while the weight gradients run on the side stream (TrainState::side)
  size_t xPlanes = 0;   // hi/lo planes of the current convolution's input (f16x3 path), as many bytes as its fp32 form
  // planes mode (every unit but the first on the split-operand kernels): encA1, pool, decA1 and botA1 hold fp16 hi + lo
  // planes instead of fp32 (the same bytes), catP is the operand form of the concat buffer
  bool planes = false;
  std::vector<size_t> catP;
  std::vector<size_t> upInP;   // per decoder step j: planes of the transposed convolution's input (botA2 / decA2[l+1])
  std::vector<size_t> encZ1, encA1, encZ2, cat, pool, dCat;
  size_t botZ1 = 0, botA1 = 0, botZ2 = 0, botA2 = 0;
  std::vector<size_t> decZ1, decA1, decZ2, decA2;
  size_t logits = 0, dlogits = 0;
  size_t gA = 0, gB = 0, gZ = 0, s2d = 0;  // gradient scratch
  size_t slab = 0, partial = 0;
  size_t slabFloats = 0;
  size_t s2dFloats = 0;
  size_t total = 0;
};

// Weight gradients beside the chain (train_side_mode): nothing in the backward pass waits for a dW, so the f16x3 weight-
// gradient kernels run on a second stream of lower priority, each forked behind its unit's input-gradient convolution,
// and the HBM-bound passes of the NEXT unit (BatchNorm backward, pooling backward, space-to-depth) run under them
// instead of leaving the matrix pipes idle.  A slot is a set of buffers the side stream reads: the dZ planes alternate
// between two (slots 0 and 1: a unit's planes are rewritten two units later, behind wait_slot), the transposed
// convolutions' space-to-depth planes are the third.  The split-K slab belongs to the side stream while anything is
// pending there (join before every main-stream use).  join() is the only place that clears the flags.
struct SideStream {
  static constexpr int kUpSlot = 2;
  hipStream_t stream = nullptr;
  hipEvent_t evFork = nullptr, evJoin = nullptr, evSlot[3] = {nullptr, nullptr, nullptr};
  bool busy[3] = {false, false, false}, any = false;
  int nextUnit = 0;   // conv units of this backward pass forked so far
  int unit_slot() { return nextUnit++ & 1; }
  hipError_t init() {
    if (stream) return hipSuccess;
    int lo = 0, hi = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&lo, &hi);   // lo = least urgent
    if (e != hipSuccess) return e;
    int prio = lo;   // UNET_TRAIN_SIDE_PRIO=n|h: the caller's / the highest priority (A/B measurements)
    if (const char* pe = getenv("UNET_TRAIN_SIDE_PRIO")) prio = pe[0] == 'h' ? hi : (pe[0] == 'n' ? 0 : lo);
    if ((e = hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, prio)) != hipSuccess) return e;
    for (hipEvent_t* ev : {&evFork, &evJoin, &evSlot[0], &evSlot[1], &evSlot[2]})
      if ((e = hipEventCreateWithFlags(ev, hipEventDisableTiming)) != hipSuccess) return e;
    return hipSuccess;
  }
  // whatever the side stream last ran on this slot's buffers happens before what is queued on s next
  hipError_t wait_slot(int slot, hipStream_t s) { return busy[slot] ? hipStreamWaitEvent(s, evSlot[slot], 0) : hipSuccess; }
  // launch(stream) on the side stream, behind everything queued on s so far; the slot is busy until the next join
  template <class F>
  hipError_t fork(int slot, hipStream_t s, F&& launch) {
    hipError_t e = hipEventRecord(evFork, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(stream, evFork, 0);
    if (e != hipSuccess) return e;
    any = true;   // from here on something may be queued there: an error below still needs the join
    if ((e = launch(stream)) == hipSuccess && (e = hipEventRecord(evSlot[slot], stream)) == hipSuccess) busy[slot] = true;
    return e;
  }
  // everything queued on the side stream so far happens before whatever is queued on s next
  hipError_t join(hipStream_t s) {
    if (!any) return hipSuccess;
    hipError_t e = hipEventRecord(evJoin, stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(s, evJoin, 0);
    any = busy[0] = busy[1] = busy[2] = false;
    return e;
  }
  void destroy() {
    if (stream) {
      hipStreamSynchronize(stream);
      hipStreamDestroy(stream);
    }
    for (hipEvent_t ev : {evFork, evJoin, evSlot[0], evSlot[1], evSlot[2]})
      if (ev) hipEventDestroy(ev);
  }
};
// joins the side stream into s when the backward pass is left, on whichever return: a no-op after the pass's own final join
struct SideJoinOnExit {
  SideStream& side;
  hipStream_t s;
  ~SideJoinOnExit() { side.join(s); }
};

}  // namespace

#include "validate_kernels.h"
#include "loss_kernels.h"

struct TrainState {
  float *params = nullptr, *grads = nullptr, *m = nullptr, *v = nullptr, *bn = nullptr;
  size_t P = 0, B = 0;
  std::vector<int> isBuffer;    // per spec entry
  std::vector<size_t> offset;   // per spec entry (into params or bn)
  std::vector<ConvUnit> enc, bott, dec;
  std::vector<UpUnit> up;
  size_t offHeadW = 0, offHeadB = 0;
  float *ones = nullptr, *zeros = nullptr;
  float* statArena = nullptr;
  GrowBuf ws;
  bool packed = false;
  PackArgs* packDescs = nullptr;   // device table of every packed operand (train_repack)
  unsigned* packStart = nullptr;   // first block of each table entry, nPack + 1 entries
  int nPackT[2] = {0, 0};            // table 0: every fp32 operand; table 1: those still read beside the f16x3 copies
  unsigned packBlocksT[2] = {0, 0};
  unet::PackX3Desc* packX3Descs = nullptr;   // the split-operand packs of the 3x3 units (pack_x3_lds_multi_kernel)
  unsigned* packX3Start = nullptr;
  int nPackX3 = 0;
  unsigned packX3Blocks = 0;
  int packedX3 = -1;                 // which table the last repack used (train_x3_enabled() at that time)
  int lossMode = 0;          // 0: BCEWithLogits(mean); 1: bce_w * BCE(pos_weight) + dice_w * Dice; 2: + focal_w * Focal
  float bceW = 1.f, diceW = 0.f, posWeight = 1.f, diceSmooth = 1e-6f;
  float focalW = 0.f, focalAlpha = 0.25f, focalGamma = 2.f;   // mode 2 only (loss_kernels.h)
  float* lossCoef = nullptr; // 2 floats (device) for the Dice gradient
  // out_channels > 1 (multiclass_kernels.h): the class loss and its reduction scratch, allocated by the first step
  unet::ClassLossParams classLoss{1.f, 0.f, 1.f, {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, -1};
  void* classWork = nullptr;
  hipStream_t commStream = nullptr;   // data-parallel overlap: see unet_train_set_comm_stream
  hipEvent_t lateGradsReady = nullptr;
  SideStream side;            // the weight gradients' stream (train_side_mode)
  std::vector<ConvUnit*> units;   // every conv unit in dbgId order: enc, bott, dec (fixed once attached)
  unsigned* gzKeys = nullptr; // 8 order keys per unit, zeroed every step: [0..4] the maxima behind bn_bwd_scale_exponent,
                              // [7] max |dZ| (fp16 range scaling of dZ when it is split by a separate pass)
  float* gzInv = nullptr;     // per unit: 2^-k undoing that scaling
  // the tables' layout: the conv units by dbgId, then the transposed convolutions by decoder step
  size_t scaled_units() const { return units.size() + up.size(); }
  unsigned* unit_keys(const ConvUnit& u) const { return gzKeys ? gzKeys + 8 * u.dbgId : nullptr; }
  unsigned* up_keys(int j) const { return gzKeys + 8 * (units.size() + j); }
  float* unit_inv(const ConvUnit& u) const { return gzInv + u.dbgId; }
  float* up_inv(int j) const { return gzInv + units.size() + j; }
  // Eval-mode forward (unet_train_eval_*): per-unit folded scale / shift, rewritten by one launch at the start of every
  // eval pass from the live gamma / beta / running statistics; apart from the step's own scale / shift / mean / invstd,
  // which a later backward pass reads
  float* evalArena = nullptr;
  unet::BnFoldDesc* evalDescs = nullptr;
  int nEvalUnits = 0;
  int dbgStage = -1;       // debug: copy an internal gradient buffer out at a numbered checkpoint
  float* dbgDst = nullptr;
  size_t dbgMax = 0;
};

namespace {

size_t spec_index(unet_ctx* h, const std::string& name) {
  for (size_t i = 0; i < h->spec.size(); ++i)
    if (h->spec[i].name == name) return i;
  return (size_t)-1;
}

// Allocate the packed-weight buffer of a GEMM op without filling it (filled by pack_weights_kernel).
int alloc_gemm(std::string& err, GemmOp& op, int taps, int kReal, int nRealTotal, int coutGroup, int coutPadGroup) {
  op.free_dev();
  op.taps = taps;
  op.cinReal = kReal;
  op.ck = (kReal % 16 == 0) ? 16 : 4;
  op.cin = round_up(kReal, op.ck);
  op.cout = coutGroup;
  op.coutPad = coutPadGroup;
  op.nTotal = round_up(nRealTotal, nRealTotal >= 128 ? 128 : 64);
  op.relu = 0;
  const size_t floats = ((size_t)(op.nTotal / 16) * (op.cin / op.ck) * taps + 1) * 64 * (op.ck / 4);
  HIPCHK(err, hipMalloc((void**)&op.wt, floats * sizeof(float)));
  HIPCHK(err, hipMemset(op.wt, 0, floats * sizeof(float)));
  if (taps == 9 && op.ck == 16) {  // Winograd-transformed copy, refreshed together with op.wt
    const size_t wf = ((size_t)(op.nTotal / 16) * (op.cin / 16) * 16 + 1) * 64 * 4;
    HIPCHK(err, hipMalloc((void**)&op.wtWino, wf * sizeof(float)));
    HIPCHK(err, hipMemset(op.wtWino, 0, wf * sizeof(float)));
  }
  return UNET_OK;
}

PackArgs make_pack(const GemmOp& op, const float* w, int mode, int nReal, int kReal, int aux) {
  PackArgs a;
  a.w = w;
  a.out = (mode == 4 || mode == 5) ? op.wtWino : op.wt;
  a.mode = mode;
  a.ck = op.ck;
  a.taps = (mode == 4 || mode == 5) ? 16 : op.taps;
  a.nChunks = op.cin / op.ck;
  a.nSub = op.nTotal / 16;
  a.nReal = nReal;
  a.kReal = kReal;
  a.coutPad = op.coutPad;
  a.aux = aux;
  return a;
}

hipError_t run_pack(const GemmOp& op, const float* w, int mode, int nReal, int kReal, int aux, hipStream_t s) {
  const PackArgs a = make_pack(op, w, mode, nReal, kReal, aux);
  hipLaunchKernelGGL(unet::pack_weights_kernel, dim3(grid_for(unet::pack_total(a))), dim3(256), 0, s, a);
  return hipGetLastError();
}

__global__ void upconv_shift_kernel(const float* bias, int cout, int coutPad, int nTotal, float* out) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= nTotal) return;
  const int co = n % coutPad;
  out[n] = (n / coutPad < 4 && co < cout) ? bias[co] : 0.f;
}

__global__ void fill_kernel(float* p, size_t n, float v) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * 256;
  for (; i < n; i += stride) p[i] = v;
}

bool train_x3_enabled();
bool train_x3_wgrad_enabled();
bool train_pool_fused();

// ---- the split-operand (fp16 hi + lo) copies of the operators: sizes, table and launches, shared by train_repack /
//      unet_train_create and the operator test entry points ----
size_t x3_conv_pack_halfs(int cout, int cin) { return (size_t)cout * cin * 9 * 2; }   // hi + lo, either operator
size_t x3_upconv_pack_halfs(int cin, int cout) { return (size_t)cin * cout * 4 * 2; }
// [tiles of 256 columns][4 cout / 32 chunks][2 planes][16][64][8]
size_t x3_upconv_dgrad_pack_halfs(int cin, int cout) {
  return (size_t)((cin + 255) / 256) * (4 * cout / 32) * 2 * 16 * 64 * 8;
}
// one 3x3 unit's entries of pack_x3_lds_multi_kernel's table: the forward operator, then the input-gradient operator
// ("cout" of the input-gradient convolution = the forward cin); either destination may be null
void pack_x3_table_add(std::vector<unet::PackX3Desc>& d, std::vector<unsigned>& start, const float* w, uint16_t* x3Fwd,
                       uint16_t* x3Dgrad, int cout, int cin) {
  if (x3Fwd) {
    d.push_back({w, x3Fwd, cout, cin, 0});
    start.push_back(start.back() + (unsigned)((cout / 64) * (cin / 32)));
  }
  if (x3Dgrad) {
    d.push_back({w, x3Dgrad, cin, cout, 1});
    start.push_back(start.back() + (unsigned)((cin / 64) * (cout / 32)));
  }
}
hipError_t launch_pack_x3_lds_multi(const unet::PackX3Desc* descs, const unsigned* start, int n, unsigned blocks,
                                    hipStream_t s) {
  const hipError_t e = ensure_dyn_lds((const void*)unet::pack_x3_lds_multi_kernel, unet::kPackX3LdsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(unet::pack_x3_lds_multi_kernel, dim3(blocks), dim3(256), (size_t)unet::kPackX3LdsBytes, s, descs, start,
                     n);
  return hipGetLastError();
}
// the gathering packer, one operator: mode 0 forward (cout, cin), mode 1 input gradient (its cout = the forward cin)
void launch_pack_x3(const float* w, uint16_t* out, int cout, int cin, int mode, hipStream_t s) {
  hipLaunchKernelGGL(unet::pack_x3_kernel, dim3(grid_for((size_t)cout * cin * 9 / 8)), dim3(256), 0, s, w, out, cout, cin,
                     mode);
}
void launch_pack_upconv_x3(const float* w, uint16_t* out, int cin, int cout, hipStream_t s) {
  hipLaunchKernelGGL(unet::pack_upconv_x3_kernel, dim3(grid_for((size_t)cin * cout * 4 / 8)), dim3(256), 0, s, w, out, cin,
                     cout);
}
void launch_pack_upconv_dgrad_x3(const float* w, uint16_t* out, int cin, int cout, hipStream_t s) {
  hipLaunchKernelGGL(unet::pack_upconv_dgrad_x3_kernel,
                     dim3(grid_for((size_t)((cin + 255) / 256) * (4 * cout / 32) * 16 * 64)), dim3(256), 0, s, w, out, cin,
                     cout);
}

// Re-derive every packed operand from the flat parameter buffer (after load and after each Adam step): one
// multi-operand launch over a descriptor table built on first use (all pointers are fixed once attached).
int train_repack(unet_ctx* h, hipStream_t s) {
  TrainState* T = h->train;
  if (!T->packDescs) {
    // two tables: every fp32 operand, and only those the step still reads when the 3x3 units that have split-operand
    // copies run on them (the first convolution and the transposed convolutions)
    std::vector<PackArgs> d[2];
    auto unit = [&](ConvUnit& u) {
      for (int t = 0; t < 2; ++t) {
        if (t == 1 && u.x3Fwd) continue;
        d[t].push_back(make_pack(u.fwd, T->params + u.offW, 0, u.cout, u.cin, u.cin));
        if (u.fwd.wtWino) d[t].push_back(make_pack(u.fwd, T->params + u.offW, 4, u.cout, u.cin, u.cin));
        if (u.needDgrad) {
          d[t].push_back(make_pack(u.dgrad, T->params + u.offW, 1, u.cin, u.cout, u.cin));
          if (u.dgrad.wtWino) d[t].push_back(make_pack(u.dgrad, T->params + u.offW, 5, u.cin, u.cout, u.cin));
        }
      }
    };
    for (ConvUnit* u : T->units) unit(*u);
    for (auto& u : T->up)
      for (int t = 0; t < 2; ++t) {
        d[t].push_back(make_pack(u.fwd, T->params + u.offW, 2, u.cout, u.cin, u.cout));
        d[t].push_back(make_pack(u.dgrad, T->params + u.offW, 3, u.cin, 4 * u.cout, u.cout));
      }
    std::vector<PackArgs> all(d[0]);
    all.insert(all.end(), d[1].begin(), d[1].end());
    std::vector<unsigned> start;
    for (int t = 0; t < 2; ++t) {
      unsigned at = 0;
      start.push_back(0);
      for (size_t i = 0; i < d[t].size(); ++i) {
        // 4096 elements per block, at least one block
        at += (unsigned)std::max<size_t>(1, (unet::pack_total(d[t][i]) + 4095) / 4096);
        start.push_back(at);
      }
      T->nPackT[t] = (int)d[t].size();
      T->packBlocksT[t] = at;
    }
    HIPCHK(h->err, hipMalloc((void**)&T->packDescs, all.size() * sizeof(PackArgs)));
    HIPCHK(h->err, hipMalloc((void**)&T->packStart, start.size() * sizeof(unsigned)));
    HIPCHK(h->err, hipMemcpy(T->packDescs, all.data(), all.size() * sizeof(PackArgs), hipMemcpyHostToDevice));
    HIPCHK(h->err, hipMemcpy(T->packStart, start.data(), start.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  }
  const int t = train_x3_enabled() ? 1 : 0;
  T->packedX3 = t;
  hipLaunchKernelGGL(unet::pack_weights_multi_kernel, dim3(T->packBlocksT[t]), dim3(256), 0, s,
                     T->packDescs + (t ? T->nPackT[0] : 0), T->packStart + (t ? T->nPackT[0] + 1 : 0), T->nPackT[t]);
  HIPCHK(h->err, hipGetLastError());
  for (auto& u : T->up) {
    hipLaunchKernelGGL(upconv_shift_kernel, dim3((u.fwd.nTotal + 255) / 256), dim3(256), 0, s, T->params + u.offB,
                       u.cout, u.fwd.coutPad, u.fwd.nTotal, u.fwd.shift);
    HIPCHK(h->err, hipGetLastError());
  }
  // the split-operand (fp16 hi + lo) copies of the 3x3 operators: one launch over a table of (tensor, pack, mode), one
  // block per (64-channel tile, 32-channel chunk) with the tile's weights through LDS (float4 loads: every tensor starts
  // on a 16-byte boundary of the parameter buffer, else the gathering kernel per operator)
  bool viaLds = (reinterpret_cast<uintptr_t>(T->params) & 15) == 0;
  for (const ConvUnit* u : T->units)
    if ((u->x3Fwd || u->x3Dgrad) && u->offW % 4 != 0) viaLds = false;
  if (viaLds) {
    if (!T->packX3Descs) {
      std::vector<unet::PackX3Desc> d;
      std::vector<unsigned> start{0};
      for (const ConvUnit* u : T->units) pack_x3_table_add(d, start, T->params + u->offW, u->x3Fwd, u->x3Dgrad, u->cout, u->cin);
      T->nPackX3 = (int)d.size();
      T->packX3Blocks = start.back();
      if (T->nPackX3) {
        HIPCHK(h->err, hipMalloc((void**)&T->packX3Descs, d.size() * sizeof(unet::PackX3Desc)));
        HIPCHK(h->err, hipMalloc((void**)&T->packX3Start, start.size() * sizeof(unsigned)));
        HIPCHK(h->err, hipMemcpy(T->packX3Descs, d.data(), d.size() * sizeof(unet::PackX3Desc), hipMemcpyHostToDevice));
        HIPCHK(h->err, hipMemcpy(T->packX3Start, start.data(), start.size() * sizeof(unsigned), hipMemcpyHostToDevice));
      }
    }
    if (T->nPackX3) HIPCHK(h->err, launch_pack_x3_lds_multi(T->packX3Descs, T->packX3Start, T->nPackX3, T->packX3Blocks, s));
  } else {
    for (const ConvUnit* u : T->units) {
      if (u->x3Fwd) launch_pack_x3(T->params + u->offW, u->x3Fwd, u->cout, u->cin, 0, s);
      if (u->x3Dgrad) launch_pack_x3(T->params + u->offW, u->x3Dgrad, u->cin, u->cout, 1, s);
    }
  }
  for (auto& u : T->up) {
    if (u.x3Fwd) launch_pack_upconv_x3(T->params + u.offW, u.x3Fwd, u.cin, u.cout, s);
    if (u.x3Dgrad) launch_pack_upconv_dgrad_x3(T->params + u.offW, u.x3Dgrad, u.cin, u.cout, s);
  }
  HIPCHK(h->err, hipGetLastError());
  T->packed = true;
  return UNET_OK;
}

// Split-K factor of the f16x3 weight gradient (wgrad_x3_ws.h): a multiple of 8 (one residue class per XCD), about two
// rounds of blocks over the 256 CUs, at least 8 K-steps per block.
size_t wgrad_x3_splits(size_t tiles, size_t steps) {
  size_t splits = round_up((int)std::max<size_t>(8, (512 + tiles - 1) / tiles), 8);
  const size_t cap = std::max<size_t>(8, steps / 8 / 8 * 8);
  return std::min(splits, cap);
}

// Planes mode: activations that only feed 3x3 convolutions are produced directly as fp16 hi + lo planes (by the
// BatchNorm / pooling kernels) instead of fp32 + a split pass per consumer.  Needs every unit but the first on the
// split-operand kernels: widths multiples of 64 and even map heights down to the bottleneck.  UNET_TRAIN_PLANES=0
// keeps fp32 activations (A/B measurements; results are bit-identical, the split is the same function either way).
bool train_planes_mode(const unet_config& c, int h) {
  static const bool on = [] {
    const char* e = getenv("UNET_TRAIN_PLANES");
    return !(e && e[0] == '0');
  }();
  if (!on || !train_x3_enabled() || !train_x3_wgrad_enabled()) return false;
  for (int l = 0; l < c.depth; ++l)
    if (c.features[l] % 64) return false;
  return h % (2 << c.depth) == 0;
}

TrainPlan plan_train(const unet_config& c, int n, int h, int w) {
  TrainPlan p;
  size_t off = 0;
  auto take = [&](size_t floats) {
    size_t o = off;
    off += (floats + 63) / 64 * 64;
    return o;
  };
  const size_t px0 = (size_t)n * h * w;
  p.x0 = take(px0 * 4);
  size_t maxAct = 0, maxSlab = 0;
  auto slabFor = [&](int rows, int cols, int taps, size_t pixels) {
    // splits chosen at launch time never exceed 2048 / tiles, see run_wgrad
    const size_t tiles = (size_t)(round_up(rows, 64) / 64) * (round_up(cols, 64) / 64);
    size_t splits = std::max<size_t>(1, 1536 / tiles);
    splits = std::min(splits, std::max<size_t>(1, pixels / 64));
    maxSlab = std::max(maxSlab, splits * taps * (size_t)round_up(rows, 64) * round_up(cols, 64));
  };
  int cin = 4;
  for (int l = 0; l < c.depth; ++l) {
    const size_t px = px0 >> (2 * l);
    const int f = c.features[l];
    p.encZ1.push_back(take(px * f));
    p.encA1.push_back(take(px * f));
    p.encZ2.push_back(take(px * f));
    p.cat.push_back(take(px * 2 * f));
    p.pool.push_back(take((px >> 2) * f));
    p.dCat.push_back(take(px * 2 * f));
    p.decZ1.push_back(take(px * f));
    p.decA1.push_back(take(px * f));
    p.decZ2.push_back(take(px * f));
    p.decA2.push_back(take(px * f));
    maxAct = std::max(maxAct, px * f);
    slabFor(f, cin, 9, px);
    slabFor(f, f, 9, px);
    slabFor(f, 2 * f, 9, px);
    slabFor(4 * f, 2 * f, 1, px >> 2);
    cin = f;
  }
  const size_t pxb = px0 >> (2 * c.depth);
  const int fb = 2 * c.features[c.depth - 1];
  p.botZ1 = take(pxb * fb);
  p.botA1 = take(pxb * fb);
  p.botZ2 = take(pxb * fb);
  p.botA2 = take(pxb * fb);
  maxAct = std::max(maxAct, pxb * fb);
  slabFor(fb, fb / 2, 9, pxb);
  slabFor(fb, fb, 9, pxb);
  p.planes = train_planes_mode(c, h);
  if (p.planes) {
    for (int l = 0; l < c.depth; ++l) p.catP.push_back(take((px0 >> (2 * l)) * 2 * c.features[l]));
    for (int j = 0; j < c.depth; ++j) {   // input of decoder step j: level l + 1 = depth - j, 2 f_l channels
      const int l = c.depth - 1 - j;
      p.upInP.push_back(take((px0 >> (2 * (l + 1))) * 2 * c.features[l]));
    }
  }
  p.xPlanes = take(px0 * 2 * c.features[0]);   // the widest convolution input: the level-0 concat buffer
  p.gzPlanes = take(maxAct);                   // planes of the current unit's dZ
  p.gzPlanes2 = take(maxAct);
  {
    // f16x3 weight gradient: slab[splits][9][cout][cin] with wgrad_x3_splits() splits
    auto slabX3 = [&](int rows, int cols, size_t pixels) {
      if (rows % 64 || cols % 64) return;
      const size_t tiles = (size_t)(rows / 64) * (cols / 64);
      maxSlab = std::max(maxSlab, wgrad_x3_splits(tiles, std::max<size_t>(1, pixels / 32)) * 9 * (size_t)rows * cols);
    };
    int ci = 4;
    for (int l = 0; l < c.depth; ++l) {
      const size_t px = px0 >> (2 * l);
      const int f = c.features[l];
      slabX3(f, ci, px);
      slabX3(f, f, px);
      slabX3(f, 2 * f, px);
      ci = f;
    }
    slabX3(fb, fb / 2, pxb);
    slabX3(fb, fb, pxb);
  }
  p.logits = take(px0 * c.out_channels);
  p.dlogits = take(px0 * c.out_channels);
  p.gA = take(maxAct);
  p.gB = take(maxAct);
  p.gZ = take(maxAct);
  p.s2d = take(maxAct);
  p.s2dFloats = maxAct;
  p.slabFloats = maxSlab;
  p.slab = take(maxSlab);
  p.partial = take(kPartialFloats);
  p.total = off;
  return p;
}

// ---- launch helpers -----------------------------------------------------------------------------------

// zero page of the current device (out-of-tensor pixels of the LDS-DMA staged kernels), allocated on first use
const float* zero_page() {
  static float* z[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!z[dev]) {
    if (hipMalloc((void**)&z[dev], 4096) != hipSuccess) return nullptr;
    if (hipMemset(z[dev], 0, 4096) != hipSuccess) return nullptr;
  }
  return z[dev];
}

template <int GH, int GW>
void launch_wgrad_wino(const unet::WgradWinoArgs& a, dim3 grid, hipStream_t s) {
  using S = unet::WgradWinoShape<GH, GW>;
  auto kern = unet::wgrad_wino_f32_kernel<GH, GW>;
  ensure_dyn_lds((const void*)kern, S::LDS_BYTES);   // on failure the launch below reports the error
  hipLaunchKernelGGL(kern, grid, dim3(512), (size_t)S::LDS_BYTES, s, a);
}

// 3x3 weight gradient by Winograd F(3x3,2x2) (wgrad_wino_f32.h): channel counts multiples of 64, even maps
hipError_t run_wgrad_wino(const float* dz, int cout, const float* x, int ldx, int cin, int n, int h, int w, float* slab,
                          size_t slabFloats, float* out, hipStream_t s) {
  unet::WgradWinoArgs a;
  a.dz = dz;
  a.x = x;
  a.zeros = zero_page();
  if (!a.zeros) return hipErrorOutOfMemory;
  a.slab = slab;
  a.N = n;
  a.H = h;
  a.W = w;
  a.Cout = cout;
  a.Cin = cin;
  a.ldx = ldx;
  const int tr = n * h / 2, tc = w / 2;
  // tile group 4x8 or 8x4 tiles: whichever pads the tile grid less
  const double waste48 = (double)((tr + 3) / 4 * 4) * ((tc + 7) / 8 * 8);
  const double waste84 = (double)((tr + 7) / 8 * 8) * ((tc + 3) / 4 * 4);
  const bool wide = waste48 <= waste84;
  const int gh = wide ? 4 : 8, gw = wide ? 8 : 4;
  a.groupsX = (tc + gw - 1) / gw;
  a.nGroups = a.groupsX * ((tr + gh - 1) / gh);
  const size_t tiles = (size_t)(cout / 64) * (cin / 64);
  size_t splits = std::max<size_t>(1, (512 + tiles - 1) / tiles);
  splits = std::min<size_t>(splits, (size_t)a.nGroups);
  while (splits > 1 && splits * 16 * (size_t)cout * cin > slabFloats) --splits;
  if (splits * 16 * (size_t)cout * cin > slabFloats) return hipErrorInvalidValue;
  a.groupsPerSplit = (int)((a.nGroups + splits - 1) / splits);
  splits = (a.nGroups + a.groupsPerSplit - 1) / a.groupsPerSplit;
  const double px = (double)n * h * w;
  prof_begin("wgrad3x3_wino_f32", 2.0 * px * 9 * cout * cin, 4.0 * (px * cout + px * cin), s);
  dim3 grid((unsigned)splits, (unsigned)(cin / 64), (unsigned)(cout / 64));
  if (wide)
    launch_wgrad_wino<4, 8>(a, grid, s);
  else
    launch_wgrad_wino<8, 4>(a, grid, s);
  prof_end(s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  prof_begin("wgrad_reduce", 0.0, 4.0 * splits * 16 * cout * cin, s);
  hipLaunchKernelGGL(unet::wgrad_wino_reduce_kernel, dim3((unsigned)((size_t)cout * cin / 64)), dim3(256), 0, s, slab,
                     (int)splits, cout, cin, out);
  prof_end(s);
  return hipGetLastError();
}

template <int MS, int NS>
void launch_wgrad_gemm(const unet::WgradGemmArgs& a, dim3 grid, hipStream_t s) {
  constexpr size_t lds = 2 * (32 * 64 * MS * 4 + 32 * 32 * NS * 4);
  auto kern = unet::wgrad_gemm_f32_kernel<MS, NS>;
  ensure_dyn_lds((const void*)kern, (int)lds);   // on failure the launch below reports the error
  hipLaunchKernelGGL(kern, grid, dim3(512), lds, s, a);
}

// out = sum over K pixels of A[k][rows] * B[k][cols] through wgrad_gemm_f32.h + the slab reduction.
// reduceMode / cgrp / colsOut as wgrad_reduce_kernel (taps = 1).
hipError_t run_wgrad_gemm(const char* name, const float* A, int lda, int rows, const float* B, int ldb, int cols, long K,
                          float* slab, size_t slabFloats, float* out, int reduceMode, int cgrp, hipStream_t s) {
  unet::WgradGemmArgs a;
  a.a = A;
  a.b = B;
  a.zeros = zero_page();
  if (!a.zeros) return hipErrorOutOfMemory;
  a.slab = slab;
  a.K = K;
  a.lda = lda;
  a.ldb = ldb;
  a.rows = rows;
  a.cols = cols;
  const bool big = rows >= 256;
  const int RT = big ? 256 : 64, CT = big ? 64 : 32;
  a.RowsPad = round_up(rows, RT);
  a.ColsPad = round_up(cols, CT);
  a.nStages = (int)((K + 31) / 32);
  const size_t tiles = (size_t)(a.RowsPad / RT) * (a.ColsPad / CT);
  size_t splits = std::max<size_t>(1, (512 + tiles - 1) / tiles);
  splits = std::min<size_t>(splits, (size_t)a.nStages);
  while (splits > 1 && splits * (size_t)a.RowsPad * a.ColsPad > slabFloats) --splits;
  if (splits * (size_t)a.RowsPad * a.ColsPad > slabFloats) return hipErrorInvalidValue;
  a.stagesPerSplit = (int)((a.nStages + splits - 1) / splits);
  splits = (a.nStages + a.stagesPerSplit - 1) / a.stagesPerSplit;
  prof_begin(name, 2.0 * (double)K * rows * cols, 4.0 * ((double)K * rows + (double)K * cols), s);
  dim3 grid((unsigned)splits, (unsigned)(a.ColsPad / CT), (unsigned)(a.RowsPad / RT));
  if (big)
    launch_wgrad_gemm<4, 2>(a, grid, s);
  else
    launch_wgrad_gemm<1, 1>(a, grid, s);
  prof_end(s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t total = (size_t)rows * cols;
  prof_begin("wgrad_reduce", 0.0, 4.0 * splits * a.RowsPad * a.ColsPad, s);
  hipLaunchKernelGGL(unet::wgrad_reduce_kernel, dim3(grid_for(total, 64)), dim3(256), 0, s, slab, (int)splits, 1,
                     a.RowsPad, a.ColsPad, rows, cols, reduceMode, cgrp, out, (const float*)nullptr);
  prof_end(s);
  return hipGetLastError();
}

// scratch / scratchFloats: optional work buffer (the first layer's im2col, N*H*W*32 floats)
hipError_t run_wgrad(const float* dz, int coutRows, const float* x, int ldx, int cinCols, int taps, int n, int h,
                     int w, float* slab, size_t slabFloats, float* out, int mode, int cgrp, hipStream_t s,
                     float* scratch = nullptr, size_t scratchFloats = 0) {
  const long npx = (long)n * h * w;
  if (taps == 1 && coutRows % 4 == 0 && cinCols % 4 == 0)
    return run_wgrad_gemm("wgrad1x1_gemm_f32", dz, coutRows, coutRows, x, ldx, cinCols, npx, slab, slabFloats, out, mode,
                          cgrp, s);
  if (taps == 9 && mode == 0 && cinCols == 3 && ldx == 4 && coutRows % 4 == 0 && scratch &&
      scratchFloats >= (size_t)npx * 32) {
    // first layer: columns (ci, tap) of an im2col'd input; out[(co*3 + ci)*9 + t] = C[co][ci*9 + t]
    prof_begin("im2col27", 0.0, 4.0 * npx * 36, s);
    hipLaunchKernelGGL(unet::im2col27_kernel, dim3(grid_for((size_t)npx * 8)), dim3(256), 0, s, x, n, h, w, scratch);
    prof_end(s);
    return run_wgrad_gemm("wgrad3x3_first_gemm_f32", dz, coutRows, coutRows, scratch, 32, 27 + 1, npx, slab, slabFloats,
                          out, 3, 0, s);
  }
  if (taps == 9 && mode == 0 && wino_enabled() && coutRows % 64 == 0 && cinCols % 64 == 0 && h % 2 == 0 && w % 2 == 0)
    return run_wgrad_wino(dz, coutRows, x, ldx, cinCols, n, h, w, slab, slabFloats, out, s);
  // pixel tile inside an image: <= 128 pixels, halo <= WG_MAX_HALO
  int th = 1, tw = 1;
  double best = 1e30;
  for (int cw = 1; cw <= std::min(w, 128); ++cw) {
    if (w % cw) continue;
    for (int chh = 1; chh <= std::min(h, 128); ++chh) {
      if (h % chh || cw * chh > 128) continue;
      const int halo = taps == 9 ? (cw + 2) * (chh + 2) : cw * chh;
      if (halo > unet::WG_MAX_HALO) continue;
      const int kt = cw * chh;
      // fewer, fuller tiles: pad to k-steps of 4, staging cost per pixel ~ halo/kt
      const double cost = (double)((kt + 3) / 4 * 4) / kt * (1.0 + 0.15 * halo / kt) + 8.0 / kt;
      if (cost < best) {
        best = cost;
        th = chh;
        tw = cw;
      }
    }
  }
  WgradArgs a;
  a.dz = dz;
  a.x = x;
  a.slab = slab;
  a.N = n;
  a.H = h;
  a.W = w;
  a.Cout = coutRows;
  a.Cin = cinCols;
  a.ldx = ldx;
  a.CoPad = round_up(coutRows, 64);
  a.CiPad = round_up(cinCols, 64);
  a.TH = th;
  a.TW = tw;
  a.tilesY = h / th;
  a.tilesX = w / tw;
  a.nTiles = n * a.tilesY * a.tilesX;
  const size_t tiles = (size_t)(a.CoPad / 64) * (a.CiPad / 64);
  size_t splits = std::max<size_t>(1, 1536 / tiles);
  splits = std::min<size_t>(splits, (size_t)a.nTiles);
  while (splits > 1 && splits * taps * (size_t)a.CoPad * a.CiPad > slabFloats) --splits;
  a.tilesPerSplit = (int)((a.nTiles + splits - 1) / splits);
  splits = (a.nTiles + a.tilesPerSplit - 1) / a.tilesPerSplit;
  const double px = (double)n * h * w;
  prof_begin(taps == 9 ? "wgrad3x3_f32" : "wgrad1x1_f32", 2.0 * px * taps * coutRows * cinCols,
             4.0 * (px * coutRows + px * cinCols), s);
  dim3 grid((unsigned)splits, (unsigned)(a.CiPad / 64), (unsigned)(a.CoPad / 64));
  if (taps == 9)
    hipLaunchKernelGGL(unet::wgrad_f32_kernel<9>, grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(unet::wgrad_f32_kernel<1>, grid, dim3(256), 0, s, a);
  prof_end(s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t total = (size_t)coutRows * cinCols * taps;
  prof_begin("wgrad_reduce", 0.0, 4.0 * splits * taps * a.CoPad * a.CiPad, s);
  hipLaunchKernelGGL(unet::wgrad_reduce_kernel, dim3(grid_for(total, 64)), dim3(256), 0, s, slab, (int)splits, taps,
                     a.CoPad, a.CiPad, coutRows, cinCols, mode, cgrp, out, (const float*)nullptr);
  prof_end(s);
  return hipGetLastError();
}

int red_blocks(size_t P) { return (int)std::min<size_t>(kRedBlocks, std::max<size_t>(1, P / 64)); }

// Training convolutions on the fp16 matrix pipe: the forward and input-gradient 3x3 convolutions of every unit with
// channel counts that are multiples of 64 run on the split-operand kernel (fp16 hi + lo operands, three MFMAs per
// product, fp32 accumulate: products exact to ~2^-22, the accuracy class of the fp32 kernels - conv_x3_ws.h) at
// about twice the speed of the fp32 Winograd kernel.  The fp32 input is split into planes by one pass, the output is
// written as fp32 (BatchNorm statistics, the weight-gradient kernels and the pooling routes stay fp32).
// unet_set_train_x3(0) / UNET_TRAIN_X3=0 keeps everything on the exact-fp32 kernels.
std::atomic<int> g_trainX3{-1};
// UNET_TRAIN_X3_WGRAD=0 keeps the weight gradients on the fp32 Winograd kernel while the forward and input-gradient
// convolutions stay on the split-operand kernel (A/B measurements)
bool train_x3_wgrad_enabled() {
  static const bool on = [] {
    const char* e = getenv("UNET_TRAIN_X3_WGRAD");
    return !(e && e[0] == '0');
  }();
  return on;
}
// UNET_TRAIN_POOL_FUSED=0: the encoder's pooling as a pass of its own again (A/B measurements; same bits)
bool train_pool_fused() {
  static const bool on = [] {
    const char* e = getenv("UNET_TRAIN_POOL_FUSED");
    return !(e && e[0] == '0');
  }();
  return on;
}
bool train_x3_enabled() {
  if (g_trainX3 < 0) {
    const char* e = getenv("UNET_TRAIN_X3");
    g_trainX3 = (e && e[0] == '0') ? 0 : 1;
  }
  return g_trainX3 == 1;
}

// An operator of the f16x3 tier over packs and epilogue arrays that live elsewhere (a unit's x3Fwd / x3Dgrad, the
// parameter buffer, TrainState::ones / zeros): GemmOpX3 frees nothing on its own, so the copy is simply dropped.
GemmOpX3 x3_borrowed(int taps, int cin, int cout, int relu, const uint16_t* wt, const float* scale, const float* shift) {
  GemmOpX3 op;
  op.taps = taps;
  op.cin = cin;
  op.cout = cout;
  op.relu = relu;
  op.wt = const_cast<uint16_t*>(wt);
  op.scale = const_cast<float*>(scale);
  op.shift = const_cast<float*>(shift);
  return op;
}

// y (fp32, pixel stride ldo, channel offset off) = conv3x3(planes of a dense (n,hh,ww,cin) tensor, packed hi/lo
// weights); inv: the device scalar split_to_planes left for a scaled input, or null
hipError_t run_train_conv_x3_planes(TrainState* T, const uint16_t* wt, int cin, int cout, const float* planes, int n,
                                    int hh, int ww, float* y, int ldo, int off, const char* label, hipStream_t s,
                                    const float* inv = nullptr, float* statPartial = nullptr, int* statRows = nullptr,
                                    int forceTw = 0, X3Path* path = nullptr) {
  // forceTw / path: the forced form and the path report of X3ConvOpts (the test entry point; the step passes neither)
  const size_t elems = (size_t)n * hh * ww * cin;
  const GemmOpX3 op = x3_borrowed(9, cin, cout, 0, wt, T->ones, T->zeros);
  const X3ConvIo io = x3_from(reinterpret_cast<const uint16_t*>(zero_page()), reinterpret_cast<const uint16_t*>(planes), elems,
                              n, hh, ww).to(nullptr, 0, ldo, off);
  X3ConvOpts o;
  o.forceTw = forceTw;
  o.outF = y;
  o.label = label;
  o.dynScale = inv;
  o.statPartial = statPartial, o.statRows = statRows;
  o.path = path;
  return run_conv_x3(op, io, o, s);
}

hipError_t run_train_conv_x3(TrainState* T, const uint16_t* wt, int cin, int cout, const float* x, int n, int hh, int ww,
                             float* y, int ldo, int off, float* planes, const char* label, hipStream_t s,
                             const unsigned* absmaxKey = nullptr, float* inv = nullptr, float* statPartial = nullptr,
                             int* statRows = nullptr) {
  split_to_planes(x, (size_t)n * hh * ww * cin, planes, s, absmaxKey, inv);
  return run_train_conv_x3_planes(T, wt, cin, cout, planes, n, hh, ww, y, ldo, off, label, s, absmaxKey ? inv : nullptr,
                                  statPartial, statRows);
}

// out = sum over P pixels of A[p][rows] (x) B[p][cols] from hi/lo planes (wgrad1x1_x3_ws_kernel) + the slab reduction
// (reduceMode / cgrp as wgrad_reduce_kernel, taps = 1); inv: scale of the A planes or null
hipError_t run_wgrad1_x3(const float* aPlanes, int lda, int rows, const float* bPlanes, int ldb, int cols, long P,
                         float* slab, size_t slabFloats, float* out, int reduceMode, int cgrp, const float* inv,
                         hipStream_t s) {
  if (rows % 128 || cols % 128) return hipErrorInvalidValue;
  unet::Wgrad1X3Args a;
  a.a = reinterpret_cast<const uint16_t*>(aPlanes);
  a.aLo = (size_t)P * lda;
  a.b = reinterpret_cast<const uint16_t*>(bPlanes);
  a.bLo = (size_t)P * ldb;
  a.zeros = reinterpret_cast<const uint16_t*>(zero_page());
  if (!a.zeros) return hipErrorOutOfMemory;
  a.slab = slab;
  a.P = P;
  a.lda = lda;
  a.ldb = ldb;
  a.rows = rows;
  a.cols = cols;
  a.steps = (int)((P + 31) / 32);
  a.colTiles = cols / 128;
  a.tiles = (rows / 128) * a.colTiles;
  size_t splits = wgrad_x3_splits((size_t)a.tiles, (size_t)a.steps);
  while (splits > 8 && splits * (size_t)rows * cols > slabFloats) splits -= 8;
  if (splits * (size_t)rows * cols > slabFloats) return hipErrorInvalidValue;
  a.splits = (int)splits;
  a.stepsPerSplit = (int)((a.steps + splits - 1) / splits);
  auto kern = unet::wgrad1x1_x3_ws_kernel;
  {
    const hipError_t ea = ensure_dyn_lds((const void*)kern, unet::Wg1X3::LDS_BYTES);
    if (ea != hipSuccess) return ea;
  }
  prof_begin("wgrad1x1_f16x3", 2.0 * (double)P * rows * cols, 4.0 * ((double)P * rows + (double)P * cols), s);
  hipLaunchKernelGGL(kern, dim3((unsigned)(splits * a.tiles)), dim3(512), (size_t)unet::Wg1X3::LDS_BYTES, s, a);
  prof_end(s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t total = (size_t)rows * cols;
  prof_begin("wgrad_reduce", 0.0, 4.0 * splits * rows * cols, s);
  hipLaunchKernelGGL(unet::wgrad_reduce_kernel, dim3(grid_for(total, 64)), dim3(256), 0, s, slab, (int)splits, 1, rows,
                     cols, rows, cols, reduceMode, cgrp, out, inv);
  prof_end(s);
  return hipGetLastError();
}

// dW (OIHW, fp32) = sum over pixels of dZ (x) X from the hi/lo planes of both; inv: scale of the dZ planes or null
hipError_t run_wgrad_x3(const float* dzPlanes, const float* xPlanes, int cout, int cin, int n, int h, int w, float* slab,
                        size_t slabFloats, float* out, const float* inv, hipStream_t s) {
  if (cout % 64 || cin % 64 || h % 2) return hipErrorInvalidValue;
  unet::WgradX3Args a;
  a.dz = reinterpret_cast<const uint16_t*>(dzPlanes);
  a.dzLo = (size_t)n * h * w * cout;
  a.x = reinterpret_cast<const uint16_t*>(xPlanes);
  a.xLo = (size_t)n * h * w * cin;
  a.zeros = reinterpret_cast<const uint16_t*>(zero_page());
  if (!a.zeros) return hipErrorOutOfMemory;
  a.slab = slab;
  a.N = n;
  a.H = h;
  a.W = w;
  a.Cout = cout;
  a.Cin = cin;
  a.strips = (w + 15) / 16;
  a.steps = n * (h / 2) * a.strips;
  a.ciTiles = cin / 64;
  a.tiles = (cout / 64) * a.ciTiles;
  size_t splits = wgrad_x3_splits((size_t)a.tiles, (size_t)a.steps);
  while (splits > 8 && splits * 9 * (size_t)cout * cin > slabFloats) splits -= 8;
  if (splits * 9 * (size_t)cout * cin > slabFloats) return hipErrorInvalidValue;
  a.splits = (int)splits;
  a.stepsPerSplit = (int)((a.steps + splits - 1) / splits);
  auto kern = unet::wgrad3x3_x3_ws_kernel;
  {
    const hipError_t ea = ensure_dyn_lds((const void*)kern, unet::WgX3::LDS_BYTES);
    if (ea != hipSuccess) return ea;
  }
  const double px = (double)n * h * w;
  prof_begin("wgrad3x3_f16x3", 2.0 * px * 9 * cout * cin, 4.0 * (px * cout + px * cin), s);
  hipLaunchKernelGGL(kern, dim3((unsigned)(splits * a.tiles)), dim3(512), (size_t)unet::WgX3::LDS_BYTES, s, a);
  prof_end(s);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t total = (size_t)cout * cin * 9;
  prof_begin("wgrad_reduce", 0.0, 4.0 * splits * 9 * cout * cin, s);
  hipLaunchKernelGGL(unet::wgrad_reduce_kernel, dim3(grid_for(total, 64)), dim3(256), 0, s, slab, (int)splits, 9, cout,
                     cin, cout, cin, 0, 0, out, inv);
  prof_end(s);
  return hipGetLastError();
}

// Where the f16x3 weight gradients run (TrainState::side): 0 = in line on the caller's stream; 1 (default) = on the side
// stream, forked as soon as the unit's dZ planes exist (beside the unit's own input-gradient convolution); 2 = forked
// behind the input-gradient convolution (beside the next unit's BatchNorm backward).  UNET_TRAIN_SIDE,
// unet_set_train_side().  The arithmetic does not change: every mode gives the same bits (tests/test_train_gpu.py).
// Measured, batch 64, unprofiled steps, one box (profiles/r04/train_side_stream.txt): in line 44.6 - 45.0 ms; mode 1 with
// the side stream at the lowest priority 43.4, at the caller's priority 43.8, at the highest 43.5; mode 2: 43.5 / 44.8 /
// 44.0.  A kernel trace of mode 1 shows why the gain is a fortieth and not the 8 ms of HBM-bound passes: under the
// package power cap the passes that run beside a weight-gradient kernel slow it down (and are slowed 1.45x themselves);
// what is gained is the power the HBM-bound passes left unused (1,250 W average in line, against 1,330 W when every
// kernel is MFMA dense).
int g_trainSide = -1;
int train_side_mode() {
  if (g_trainSide < 0) {
    const char* e = getenv("UNET_TRAIN_SIDE");
    g_trainSide = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 1;
  }
  return g_trainSide;
}
// the side stream is used unless per-launch timing is on (overlapping kernels would make the event pairs meaningless)
// or a debug snapshot is being taken
bool side_on(const TrainState* T) { return train_side_mode() > 0 && !(g_prof && g_prof->on) && T->dbgStage < 0; }

// One backward operator with a weight gradient, a conv unit or a transposed convolution: producer() on s writes what
// both gradients read (into the buffers of `slot`), dgrad() on s is the input gradient, wgrad(stream) the weight gradient:
// beside the chain on the side stream - forked before the input gradient in mode 1, behind it in mode 2 - or, with
// slot < 0, in line on s between the two, where it takes the split-K slab back from the side stream first.
template <class Producer, class Wgrad, class Dgrad>
int backward_with_wgrad(unet_ctx* h, hipStream_t s, int slot, Producer&& producer, Wgrad&& wgrad, Dgrad&& dgrad) {
  SideStream& side = h->train->side;
  int rc;
  if (slot >= 0) {
    HIPCHK(h->err, side.init());
    HIPCHK(h->err, side.wait_slot(slot, s));   // the weight gradient that last read these buffers must be through
  } else {
    HIPCHK(h->err, side.join(s));
  }
  if ((rc = producer())) return rc;
  if (slot < 0) HIPCHK(h->err, wgrad(s));
  else if (train_side_mode() == 1) HIPCHK(h->err, side.fork(slot, s, wgrad));
  if ((rc = dgrad())) return rc;
  if (slot >= 0 && train_side_mode() != 1) HIPCHK(h->err, side.fork(slot, s, wgrad));
  return UNET_OK;
}

// ConvTranspose2d(2f -> f) of the training forward on planes: planes (n,h,w,cin) in, planes out with pixel stride ldo at
// channel offset coOff; wt from pack_upconv_x3_kernel (un-prescaled: unit scale), bias the fp32 parameter itself
hipError_t run_train_upconv_x3(TrainState* T, const uint16_t* wt, const float* bias, int cin, int cout, const uint16_t* in,
                               size_t inLo, int n, int h, int w, uint16_t* out, size_t outLo, int ldo, int coOff,
                               hipStream_t s, X3Path* path = nullptr) {
  const GemmOpX3 op = x3_borrowed(1, cin, cout, 0, wt, T->ones, bias);
  return run_upconv_x3(op, x3_from(reinterpret_cast<const uint16_t*>(zero_page()), in, inLo, n, h, w).to(out, outLo, ldo, coOff), s,
                       nullptr, path);
}

// ConvTranspose2d backward, f16x3: the bias gradient is the column sum of the gradient slice dY (P hi-res pixels, pixel
// stride ldd, f channels at offset offd); the same pass leaves max |.| of the slice in *key (zeroed by the caller)
hipError_t run_up_bias_grad_x3(const float* dY, int ldd, int offd, size_t Ph, int f, float* partial, unsigned* key, float* db,
                               hipStream_t s) {
  const int nb = red_blocks(Ph);
  prof_begin("bias_grad", 0.0, 4.0 * Ph * f, s);
  hipLaunchKernelGGL(unet::colsum_partial_kernel, dim3(nb), dim3(256), 0, s, dY, ldd, offd, Ph, f, partial, key);
  hipLaunchKernelGGL(unet::colsum_finalize_kernel, dim3((f + unet::FIN_CH - 1) / unet::FIN_CH), dim3(256), 0, s, partial, nb, f, f,
                     db);
  prof_end(s);
  return hipGetLastError();
}

// ... and the slice in space-to-depth order as scaled operand planes S (n,lh,lw,4f), 2^-k left in *inv
hipError_t run_up_s2d_planes_x3(const float* dY, int ldd, int offd, int n, int lh, int lw, int f, const unsigned* key, float* S,
                                float* inv, hipStream_t s) {
  const size_t Pl = (size_t)n * lh * lw;
  prof_begin("space_to_depth", 0.0, 8.0 * Pl * 4 * f, s);
  hipLaunchKernelGGL(unet::space_to_depth_planes_kernel, dim3(grid_for(Pl * 4 * (f / 4))), dim3(256), 0, s, dY, ldd, offd, n, lh,
                     lw, f, key, reinterpret_cast<uint32_t*>(S), Pl * 4 * (size_t)f / 2, inv);
  prof_end(s);
  return hipGetLastError();
}

// Where a unit's activation goes: fp32 (pixel stride ld, channel offset off) and / or fp16 hi + lo planes (pixel
// stride ldp, channel offset offp; the lo plane behind a hi plane of P * ldp halfs) - either may be null
struct ActOut {
  float* f32 = nullptr;
  int ld = 0, off = 0;
  float* planes = nullptr;
  int ldp = 0, offp = 0;
  float* pooled = nullptr;   // planes mode: also the MaxPool2d(2,2) of the activation as dense planes (the encoder's skips)
  const float *headW = nullptr, *headB = nullptr;   // the last unit (64 channels): the 1x1 head in the same pass
  float* logits = nullptr;
};
// a dense activation of ld channels as fp32 and / or planes (either may be null)
ActOut act_out(float* f32, float* planes, int ld) {
  ActOut o;
  o.f32 = f32;
  o.planes = planes;
  o.ld = o.ldp = ld;
  return o;
}

// conv (raw) -> batch statistics -> a = relu(bn(z)).  inPlanes: the input already in operand form (planes mode),
// else `in` is fp32 and is split into `planes` scratch when the unit runs on the split-operand kernel
int unit_forward(unet_ctx* h, ConvUnit& u, const float* in, const float* inPlanes, int n, int hh, int ww, float* z,
                 const ActOut& o, float* partial, float* planes, hipStream_t s) {
  TrainState* T = h->train;
  const size_t P = (size_t)n * hh * ww;
  // the second and third convolution structures sum the statistics' first pass in their epilogues (statRows rows of
  // `partial`; UNET_TRAIN_FUSED_STATS=0 restores the separate pass over z).  Measured (batch 64): bn_stats 1.43 -> 0.84 ms,
  // forward convolutions +0.05 ms.  The rows are sums of the same stored fp32 values z over the image's pixels only (each
  // pixel once, no padded or out-of-image pixel): exact up to the fp32 summation order, which
  // tests/test_train_x3_ops_gpu.py proves bit for bit on integer-valued inputs.  The other summation order moves which
  // near-zero BatchNorm outputs take which side of the ReLU, and with it the BatchNorm-weight gradient norms of the
  // reference's batch-4 golden step: 1.75e-3 from a float64 run of the reference's network against 1.15e-3
  // with the separate pass - and 1.71e-3 for this library's exact-fp32 kernels, 1.14e-3 for the reference's own fp32 run
  // (tools/probes/gradnorm_dev.py, profiles/r04/gradnorm_vs_f64.txt).  The test bound is twice the reference's own distance
  // (tests/test_train_gpu.py, GRADNORM_K), so the fused form is the default since round 4.
  static const bool fuseStats = [] {
    const char* e = getenv("UNET_TRAIN_FUSED_STATS");
    return !(e && e[0] == '0');
  }();
  int statRows = 0;
  float* sp = fuseStats ? partial : nullptr;
  if (inPlanes)
    HIPCHK(h->err, run_train_conv_x3_planes(T, u.x3Fwd, u.cin, u.cout, inPlanes, n, hh, ww, z, u.cout, 0, "conv3x3_f16x3", s,
                                            nullptr, sp, &statRows));
  else if (u.x3Fwd && train_x3_enabled())
    HIPCHK(h->err, run_train_conv_x3(T, u.x3Fwd, u.cin, u.cout, in, n, hh, ww, z, u.cout, 0, planes, "conv3x3_f16x3", s,
                                     nullptr, nullptr, sp, &statRows));
  else
    HIPCHK(h->err, run_gemm_op(u.fwd, in, n, hh, ww, z, u.cout, 0, s));
  const int nb = statRows > 0 ? statRows : red_blocks(P);
  prof_begin("bn_stats", 0.0, 4.0 * P * u.cout, s);
  if (statRows == 0) hipLaunchKernelGGL(unet::bn_stats_partial_kernel, dim3(nb), dim3(256), 0, s, z, P, u.cout, partial);
  hipLaunchKernelGGL(unet::bn_finalize_kernel, dim3((u.cout + unet::FIN_CH - 1) / unet::FIN_CH), dim3(256), 0, s, partial, nb, u.cout,
                     (double)P, T->params + u.offG, T->params + u.offB, kBnEps, kBnMomentum, u.scale, u.shift, u.mean,
                     u.invstd, T->bn + u.offRM, T->bn + u.offRV);
  prof_end(s);
  prof_begin("bn_apply_relu", 0.0, (4.0 + (o.f32 ? 4.0 : 0.0) + (o.planes ? 4.0 : 0.0)) * P * u.cout, s);
  if (o.pooled) {
    // the pooling rides in the same pass (measured, batch 64: bn_apply_relu + maxpool2x2 over the four levels 1.31 ->
    // 0.98 ms; same bits).  Only the walk asks for it, in front of a pooling: check_shape has made that map even.
    hipLaunchKernelGGL(unet::bn_apply_relu_pool_kernel, dim3(grid_for((P / 4) * (u.cout / 4))), dim3(256), 0, s, z, u.scale,
                       u.shift, n, hh, ww, u.cout, o.f32, o.ld, o.off, reinterpret_cast<uint32_t*>(o.planes),
                       P * (size_t)o.ldp / 2, o.ldp, o.offp, reinterpret_cast<uint32_t*>(o.pooled),
                       (P / 4) * (size_t)u.cout / 2, g_errWord);
  } else {
    const bool head = o.headW && u.cout == 64;
    hipLaunchKernelGGL(unet::bn_apply_relu_kernel, dim3(grid_for(P * (u.cout / 4))), dim3(256), 0, s, z, u.scale,
                       u.shift, P, u.cout, o.f32, o.ld, o.off, reinterpret_cast<uint32_t*>(o.planes),
                       P * (size_t)o.ldp / 2, o.ldp, o.offp, g_errWord, head ? o.headW : (const float*)nullptr,
                       head ? o.headB : (const float*)nullptr, head ? o.logits : (float*)nullptr);
  }
  prof_end(s);
  HIPCHK(h->err, hipGetLastError());
  return UNET_OK;
}

// dA (ld, off) -> dgamma/dbeta, dZ, dW and (optionally) the input gradient written to (dIn, ldIn, offIn)
// xPlanesIn: the unit's input in operand form (planes mode: x itself is then not read), or null
int unit_backward(unet_ctx* h, ConvUnit& u, const float* dA, int ldd, int offd, const float* z, const float* x,
                  int ldx, int n, int hh, int ww, float* gZ, float* dIn, int ldIn, int offIn, const TrainPlan& p,
                  hipStream_t s, const float* xPlanesIn = nullptr, const float* r1p = nullptr,
                  const float* r1c = nullptr, int partialRows = 0) {
  // partialRows > 0: the kernel that produced dA already left the BatchNorm backward's partial sums (that many rows of
  // `partial`) and the two maxima in the unit's keys (maxpool_bwd_add_bnstat_kernel)
  // r1p / r1c: dA is the outer product r1p[pixel] * r1c[channel] (the unit under the 1x1 head) and is never stored
  TrainState* T = h->train;
  float* ws = reinterpret_cast<float*>(T->ws.p);
  float* partial = ws + p.partial;
  const size_t P = (size_t)n * hh * ww;
  const int nb = partialRows > 0 ? partialRows : red_blocks(P);
  const bool x3Path = u.x3Dgrad && train_x3_enabled() && T->gzKeys;
  const bool wgradX3 = x3Path && ldx == u.cin && hh % 2 == 0 && (xPlanesIn || train_x3_wgrad_enabled());
  // planes mode: dZ leaves the BatchNorm backward directly in operand form (scaled by a power of two derived from a
  // bound on |dZ|, bn_bwd_scale_exponent); fp32 dZ is then only written for a debug snapshot
  const bool fusedPlanes = wgradX3 && xPlanesIn;
  if (xPlanesIn && !fusedPlanes) {
    h->err = "training plan inconsistent: a unit outside the split-operand path was handed an input in planes";
    return UNET_ERR_STATE;
  }
  unsigned* keys = T->unit_keys(u);
  float* inv = T->unit_inv(u);
  // on the side stream the dZ planes alternate between two buffers, one per slot
  const int slot = fusedPlanes && side_on(T) ? T->side.unit_slot() : -1;
  float* gzPlanes = ws + (slot == 1 ? p.gzPlanes2 : p.gzPlanes);
  float* gzF32 = (!fusedPlanes || T->dbgStage == 300 + u.dbgId) ? gZ : nullptr;
  auto producer = [&]() -> int {
    prof_begin("bn_relu_bwd", 0.0, 4.0 * P * u.cout * 5, s);
    if (partialRows <= 0)
      hipLaunchKernelGGL(unet::bn_bwd_partial_kernel, dim3(nb), dim3(256), 0, s, dA, ldd, offd, z, u.scale, u.shift,
                         u.mean, u.invstd, P, u.cout, partial, fusedPlanes ? keys : (unsigned*)nullptr, r1p, r1c);
    hipLaunchKernelGGL(unet::reduce2_finalize_kernel, dim3((u.cout + unet::FIN_CH - 1) / unet::FIN_CH), dim3(256), 0, s, partial, nb, u.cout,
                       T->grads + u.offB, T->grads + u.offG, fusedPlanes ? keys : (unsigned*)nullptr, (const float*)u.scale);
    hipLaunchKernelGGL(unet::bn_bwd_apply_kernel, dim3(grid_for(P * (u.cout / 4))), dim3(256), 0, s, dA, ldd, offd, z,
                       u.scale, u.shift, u.mean, u.invstd, T->grads + u.offB, T->grads + u.offG, (float)(1.0 / (double)P),
                       P, u.cout, gzF32, (keys && !fusedPlanes) ? keys + 7 : (unsigned*)nullptr,
                       (const unsigned*)(fusedPlanes ? keys : nullptr),
                       fusedPlanes ? reinterpret_cast<uint32_t*>(gzPlanes) : (uint32_t*)nullptr, P * (size_t)u.cout / 2,
                       fusedPlanes ? inv : (float*)nullptr, r1p, r1c);
    prof_end(s);
    HIPCHK(h->err, hipGetLastError());
    if (T->dbgStage == 300 + u.dbgId) hipMemcpyAsync(T->dbgDst, gZ, std::min(T->dbgMax, P * u.cout) * 4, hipMemcpyDeviceToDevice, s);
    if (T->dbgStage == 400 + u.dbgId) hipMemcpyAsync(T->dbgDst, z, std::min(T->dbgMax, P * u.cout) * 4, hipMemcpyDeviceToDevice, s);
    if (T->dbgStage == 500 + u.dbgId) hipMemcpyAsync(T->dbgDst, u.scale, std::min<size_t>(T->dbgMax, 4 * round_up(u.cout, 64)) * 4, hipMemcpyDeviceToDevice, s);
    // f16x3: dZ in operand form (scaled into the fp16 range) serves the weight gradient and the input gradient
    if (x3Path && !fusedPlanes) split_to_planes(gZ, P * u.cout, gzPlanes, s, keys + 7, inv);
    return UNET_OK;
  };
  auto wgrad = [&](hipStream_t st) -> hipError_t {
    if (!wgradX3)   // (p.s2d is free here: only the upconv backward uses it, and never inside a conv unit)
      return run_wgrad(gZ, u.cout, x, ldx, u.cin, 9, n, hh, ww, ws + p.slab, p.slabFloats, T->grads + u.offW, 0, 0, st,
                       ws + p.s2d, p.s2dFloats);
    if (!xPlanesIn) split_to_planes(x, P * u.cin, ws + p.xPlanes, st);
    return run_wgrad_x3(gzPlanes, xPlanesIn ? xPlanesIn : ws + p.xPlanes, u.cout, u.cin, n, hh, ww, ws + p.slab,
                        p.slabFloats, T->grads + u.offW, inv, st);
  };
  auto dgrad = [&]() -> int {
    if (!u.needDgrad || !dIn) return UNET_OK;
    if (x3Path)
      HIPCHK(h->err, run_train_conv_x3_planes(T, u.x3Dgrad, u.cout, u.cin, gzPlanes, n, hh, ww, dIn, ldIn, offIn,
                                              "dgrad3x3_f16x3", s, inv));
    else
      HIPCHK(h->err, run_gemm_op(u.dgrad, gZ, n, hh, ww, dIn, ldIn, offIn, s));
    return UNET_OK;
  };
  return backward_with_wgrad(h, s, slot, producer, wgrad, dgrad);
}

// What a pass over the attached state needs before its first launch, for either pass: the attached state ...
int pass_state(unet_ctx* h) {
  if (!h) return UNET_ERR_INVALID_ARG;
  if (!h->train || !h->train->packed) {
    h->err = "unet_train_attach has not been called";
    return UNET_ERR_STATE;
  }
  return UNET_OK;
}
// ... and a legal shape, its plan and a workspace that holds it
int pass_workspace(unet_ctx* h, int n, int height, int width, TrainPlan& plan) {
  int rc = check_shape(h, n, height, width);
  if (rc) return rc;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  plan = plan_train(h->cfg, n, height, width);
  return h->train->ws.reserve(h->err, plan.total * sizeof(float), "training workspace");
}

int train_prologue(unet_ctx* h, const void* in, const float* targets, float* loss, int n, int height, int width,
                   TrainPlan& plan) {
  if (!h || !in || !targets || !loss) return UNET_ERR_INVALID_ARG;
  const int rc = pass_state(h);
  return rc ? rc : pass_workspace(h, n, height, width, plan);
}

int eval_prologue(unet_ctx* h, const void* in, float* logits, int n, int height, int width, TrainPlan& plan) {
  const int rc = pass_state(h);
  if (rc) return rc;
  if (!in || !logits) return UNET_ERR_INVALID_ARG;
  return pass_workspace(h, n, height, width, plan);
}

// ---- eval-mode forward on the attached parameters (reference README.md:2089-2099: model.eval(); no_grad) --------
//
// The same operand packs and the same dispatch as unit_forward, with BatchNorm in eval form: one launch folds gamma,
// beta and the running statistics of every unit into scale / shift (bn_eval_fold_kernel), and the convolution applies
// them and the ReLU in its epilogue.  Nothing of z is stored where a unit runs on the split-operand kernels: planes in,
// planes (or the fp32 activation) out, the encoder's pooling in the same epilogue.  An exact-fp32 unit writes its fp32
// activation from the convolution's epilogue as well; only where its consumer wants operand planes (the first
// convolution in planes mode) it writes raw z and bn_apply_relu_kernel produces the planes.
// It writes the eval arena, the workspace (every buffer of which a training step rewrites before it reads it) and the
// caller's logits - and nothing else: no parameter, gradient, moment, running statistic or saved per-unit statistic.

int eval_init(unet_ctx* h) {
  TrainState* T = h->train;
  if (T->evalArena) return UNET_OK;
  size_t floats = 0;
  for (const ConvUnit* u : T->units) floats += 2 * (size_t)round_up(u->cout, 128);
  HIPCHK(h->err, hipMalloc((void**)&T->evalArena, floats * sizeof(float)));
  std::vector<unet::BnFoldDesc> d;
  float* sp = T->evalArena;
  for (ConvUnit* u : T->units) {
    const int cp = round_up(u->cout, 128);
    u->evScale = sp;
    u->evShift = sp + cp;
    sp += 2 * cp;
    d.push_back({T->params + u->offG, T->params + u->offB, T->bn + u->offRM, T->bn + u->offRV, u->evScale, u->evShift, u->cout, cp});
  }
  T->nEvalUnits = (int)d.size();
  HIPCHK(h->err, hipMalloc((void**)&T->evalDescs, d.size() * sizeof(unet::BnFoldDesc)));
  HIPCHK(h->err, hipMemcpy(T->evalDescs, d.data(), d.size() * sizeof(unet::BnFoldDesc), hipMemcpyHostToDevice));
  return UNET_OK;
}

// One conv unit in eval form.  Output: operand planes (o.planes, optionally with the pooled planes o.pooled) or fp32
// (o.f32), never both.  z: scratch for raw z (exact-fp32 unit with a planes output only)
int eval_unit(unet_ctx* h, ConvUnit& u, const float* in, const float* inPlanes, int n, int hh, int ww, float* z,
              const ActOut& o, float* planes, hipStream_t s) {
  TrainState* T = h->train;
  const size_t P = (size_t)n * hh * ww;
  if (inPlanes && !u.x3Fwd) {
    h->err = "training plan inconsistent: a unit outside the split-operand path was handed an input in planes";
    return UNET_ERR_STATE;
  }
  if (inPlanes || (u.x3Fwd && train_x3_enabled())) {
    if (!inPlanes) {
      split_to_planes(in, P * u.cin, planes, s);
      inPlanes = planes;
    }
    const GemmOpX3 op = x3_borrowed(9, u.cin, u.cout, 1, u.x3Fwd, u.evScale, u.evShift);
    X3ConvIo io = x3_from(reinterpret_cast<const uint16_t*>(zero_page()), reinterpret_cast<const uint16_t*>(inPlanes), P * u.cin,
                          n, hh, ww);
    X3ConvOpts co;
    X3Fuse fz;
    co.label = "eval_conv3x3_f16x3";
    if (o.planes) {
      io = io.to(reinterpret_cast<uint16_t*>(o.planes), P * (size_t)o.ldp, o.ldp, o.offp);
      if (o.pooled) {
        fz.pool = reinterpret_cast<uint16_t*>(o.pooled);
        fz.poolLo = (P / 4) * (size_t)u.cout;
        co.fuse = &fz;
        co.label = "eval_conv3x3_pool_f16x3";
      }
    } else {
      io = io.to(nullptr, 0, o.ld, o.off);
      co.outF = o.f32;
    }
    HIPCHK(h->err, run_conv_x3(op, io, co, s));
    return UNET_OK;
  }
  if (o.planes) {
    GemmOp op = u.fwd;   // a copy of plain pointers (ones / zeros epilogue: raw z)
    op.name = "eval_conv3x3_igemm_f32";
    op.nameWino = "eval_conv3x3_wino_f32";
    HIPCHK(h->err, run_gemm_op(op, in, n, hh, ww, z, u.cout, 0, s));
    prof_begin("eval_bn_apply_relu", 0.0, 8.0 * P * u.cout, s);
    hipLaunchKernelGGL(unet::bn_apply_relu_kernel, dim3(grid_for(P * (u.cout / 4))), dim3(256), 0, s, z, u.evScale,
                       u.evShift, P, u.cout, (float*)nullptr, 0, 0, reinterpret_cast<uint32_t*>(o.planes),
                       P * (size_t)o.ldp / 2, o.ldp, o.offp, g_errWord, (const float*)nullptr, (const float*)nullptr,
                       (float*)nullptr);
    prof_end(s);
    HIPCHK(h->err, hipGetLastError());
    if (o.pooled) {
      h->err = "eval pass: a pooled planes output was asked of an exact-fp32 unit";
      return UNET_ERR_STATE;
    }
    return UNET_OK;
  }
  GemmOp op = u.fwd;   // the folded BatchNorm and the ReLU in the convolution's epilogue
  op.scale = u.evScale;
  op.shift = u.evShift;
  op.relu = 1;
  op.name = "eval_conv3x3_igemm_f32";
  op.nameWino = "eval_conv3x3_wino_f32";
  HIPCHK(h->err, run_gemm_op(op, in, n, hh, ww, o.f32, o.ld, o.off, s));
  return UNET_OK;
}

// unet_set_train_x3 since the last repack: the packs follow the switch
int repack_if_switched(unet_ctx* h, hipStream_t s) {
  return h->train->packedX3 != (train_x3_enabled() ? 1 : 0) ? train_repack(h, s) : UNET_OK;
}

// The forward traversal of the network, once for both passes: the training step (unit_forward: batch statistics, everything
// the backward pass reads is kept) and the eval pass (eval_unit: folded running statistics, nothing kept).  The rules that
// differ between the two stand side by side in the lambdas at the top; the loops, the level arithmetic, the workspace
// offsets, the transposed convolutions' dispatch and the strided split below them exist once.  Logits to `logits`.
enum class Pass { Train, Eval };

int forward_walk(unet_ctx* h, Pass pass, int n, int height, int width, float* logits, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  const unet_config& c = h->cfg;
  const int D = c.depth;
  const bool train = pass == Pass::Train, PM = p.planes;
  float* ws = reinterpret_cast<float*>(T->ws.p);
  int rc;
  // one conv unit; `in` is planes where inP says so
  auto unit = [&](ConvUnit& u, const float* in, bool inP, int hh, int ww, float* z, const ActOut& o) {
    const float *f32 = inP ? nullptr : in, *pl = inP ? in : nullptr;
    return train ? unit_forward(h, u, f32, pl, n, hh, ww, z, o, ws + p.partial, ws + p.xPlanes, s)
                 : eval_unit(h, u, f32, pl, n, hh, ww, z, o, ws + p.xPlanes, s);
  };
  // an activation only 3x3 convolutions read (either pass): planes in planes mode, else fp32
  auto inner = [&](float* buf, int ld) { return PM ? act_out(nullptr, buf, ld) : act_out(buf, nullptr, ld); };
  // pooling: inside the unit that writes the skip (train: its BatchNorm pass, unless UNET_TRAIN_POOL_FUSED=0; eval: the
  // convolution's epilogue), else as a pass over the fp32 skip.  The maps are even: check_shape, at every level above
  // the bottleneck
  const bool poolInUnit = PM && (!train || train_pool_fused());
  // the skip half of the concat buffer: train keeps fp32 (its pooling's backward reads it) beside the planes of planes
  // mode; eval writes planes or fp32, never both
  auto skipOut = [&](int l, int f) {
    ActOut o = act_out(train || !PM ? ws + p.cat[l] : nullptr, PM ? ws + p.catP[l] : nullptr, 2 * f);
    if (poolInUnit) o.pooled = ws + p.pool[l];
    return o;
  };
  // the output of the unit in front of decoder step j (j == D: the last unit, which feeds the head in fp32): planes where
  // the transposed convolution runs on the split-operand kernel.  Eval then writes no fp32; train keeps fp32 unless nobody
  // reads it (only the exact-fp32 GEMMs of the transposed convolution's backward do, and a debug snapshot)
  auto upInOut = [&](float* buf, int j, int chn) {
    const bool asP = PM && j < D && T->up[j].x3Fwd;
    const bool f32 = !asP || (train && !(T->up[j].x3Dgrad && train_x3_wgrad_enabled() && T->dbgStage < 0));
    return act_out(f32 ? buf : nullptr, asP ? ws + p.upInP[j] : nullptr, chn);
  };
  // the 1x1 head: train lets it ride in the last unit's BatchNorm pass (64 channels; the same A/B switch as the pooling
  // fusions), eval always launches it
  const bool headInUnit = train && c.out_channels == 1 && c.features[0] == 64 && train_pool_fused();

  const float* cur = ws + p.x0;   // fp32 activation, or planes where PM says so
  int ch = height, cw = width;
  for (int l = 0; l < D; ++l) {
    const int f = c.features[l];
    if ((rc = unit(T->enc[2 * l], cur, PM && l > 0, ch, cw, ws + p.encZ1[l], inner(ws + p.encA1[l], f)))) return rc;
    if ((rc = unit(T->enc[2 * l + 1], ws + p.encA1[l], PM, ch, cw, ws + p.encZ2[l], skipOut(l, f)))) return rc;
    if (poolInUnit) {
      // pooled planes already written by the unit
    } else if (PM) {
      const size_t total = (size_t)n * (ch / 2) * (cw / 2) * (f / 4);
      prof_begin("maxpool2x2", 0.0, 4.0 * total * 4 * 5, s);
      hipLaunchKernelGGL(unet::maxpool2x2_to_planes_kernel, dim3(grid_for(total)), dim3(256), 0, s, ws + p.cat[l], n, ch,
                         cw, f, 2 * f, reinterpret_cast<uint32_t*>(ws + p.pool[l]), total * 2);
      prof_end(s);
      HIPCHK(h->err, hipGetLastError());
    } else {
      HIPCHK(h->err, run_maxpool(ws + p.cat[l], ws + p.pool[l], n, ch, cw, f, 2 * f, s));
    }
    cur = ws + p.pool[l];
    ch /= 2;
    cw /= 2;
  }
  const int fb = 2 * c.features[D - 1];
  if ((rc = unit(T->bott[0], cur, PM, ch, cw, ws + p.botZ1, inner(ws + p.botA1, fb)))) return rc;
  if ((rc = unit(T->bott[1], ws + p.botA1, PM, ch, cw, ws + p.botZ2, upInOut(ws + p.botA2, 0, fb)))) return rc;
  cur = ws + p.botA2;
  for (int j = 0; j < D; ++j) {
    const int l = D - 1 - j;
    const int f = c.features[l];
    const bool upX3 = PM && T->up[j].x3Fwd;
    if (upX3) {   // planes in, planes out: straight into the upper channel half of the concat buffer's operand form
      const size_t Pin = (size_t)n * ch * cw;
      HIPCHK(h->err, run_train_upconv_x3(T, T->up[j].x3Fwd, T->params + T->up[j].offB, 2 * f, f,
                                         reinterpret_cast<const uint16_t*>(ws + p.upInP[j]), Pin * 2 * f, n, ch, cw,
                                         reinterpret_cast<uint16_t*>(ws + p.catP[l]), Pin * 4 * 2 * f, 2 * f, f, s));
    } else {
      HIPCHK(h->err, run_gemm_op(T->up[j].fwd, cur, n, ch, cw, ws + p.cat[l], 2 * f, f, s));
    }
    ch *= 2;
    cw *= 2;
    if (PM && !upX3) {   // upper half of the concat buffer -> operand form
      const size_t Pl = (size_t)n * ch * cw;
      prof_begin("split_planes", 0.0, 8.0 * Pl * f, s);
      hipLaunchKernelGGL(unet::split_planes_strided_kernel, dim3(grid_for(Pl * (f / 4))), dim3(256), 0, s, ws + p.cat[l],
                         2 * f, f, Pl, f, reinterpret_cast<uint32_t*>(ws + p.catP[l]), Pl * (size_t)(2 * f) / 2, 2 * f, f);
      prof_end(s);
      HIPCHK(h->err, hipGetLastError());
    }
    if ((rc = unit(T->dec[2 * j], PM ? ws + p.catP[l] : ws + p.cat[l], PM, ch, cw, ws + p.decZ1[l], inner(ws + p.decA1[l], f))))
      return rc;
    ActOut last = upInOut(ws + p.decA2[l], j + 1, f);
    if (headInUnit && j == D - 1) {
      last.headW = T->params + T->offHeadW;
      last.headB = T->params + T->offHeadB;
      last.logits = logits;
    }
    if ((rc = unit(T->dec[2 * j + 1], ws + p.decA1[l], PM, ch, cw, ws + p.decZ2[l], last))) return rc;
    cur = ws + p.decA2[l];
  }
  if (c.out_channels > 1) {   // the K-way head on the fp32 activation of the last unit: logits (N,K,H,W)
    const size_t P0 = (size_t)n * height * width;
    prof_begin("headk", 2.0 * P0 * c.features[0] * c.out_channels, 4.0 * P0 * (c.features[0] + c.out_channels), s);
    const hipError_t e = unet::launch_headk(cur, T->params + T->offHeadW, T->params + T->offHeadB, n, (size_t)height * width,
                                            c.features[0], c.out_channels, logits, nullptr, nullptr, 0, nullptr, s);
    prof_end(s);
    HIPCHK(h->err, e);
  } else if (!headInUnit)
    HIPCHK(h->err, run_head(cur, T->params + T->offHeadW, 0.f, (size_t)n * height * width, c.features[0], logits, nullptr,
                            nullptr, 0.f, s, T->params + T->offHeadB));
  return UNET_OK;
}

// the loss of lossMode over P0 logits: its terms to lossDev, its logit gradient to the workspace's dlogits
int run_loss_grad(unet_ctx* h, const float* targets, size_t P0, float* lossDev, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  float* ws = reinterpret_cast<float*>(T->ws.p);
  float* partial = ws + p.partial;
  if (T->lossMode == 2) {
    // the reduction scratch holds kRedBlocks * 2 * 4096 floats, far beyond loss_scratch_bytes of any batch
    const unet::LossParams lp{T->bceW, T->focalW, T->diceW, T->posWeight, T->focalAlpha, T->focalGamma, T->diceSmooth};
    prof_begin("focal_loss_grad", 0.0, 20.0 * P0, s);
    const hipError_t e = unet::launch_loss_grad(ws + p.logits, targets, P0, lp, partial, lossDev, ws + p.dlogits, s);
    prof_end(s);
    HIPCHK(h->err, e);
  } else if (T->lossMode == 1) {
    const int nb = red_blocks(P0);
    prof_begin("bce_dice_loss_grad", 0.0, 20.0 * P0, s);
    hipLaunchKernelGGL(unet::bce_dice_partial_kernel, dim3(nb), dim3(256), 0, s, ws + p.logits, targets, P0,
                       T->posWeight, partial);
    hipLaunchKernelGGL(unet::bce_dice_finalize_kernel, dim3(1), dim3(1), 0, s, partial, nb, (double)P0, T->bceW,
                       T->diceW, T->diceSmooth, lossDev, T->lossCoef);
    hipLaunchKernelGGL(unet::bce_dice_grad_kernel, dim3(grid_for(P0)), dim3(256), 0, s, ws + p.logits, targets, P0,
                       (float)((double)T->bceW / (double)P0), T->diceW, T->posWeight, T->lossCoef, ws + p.dlogits);
    prof_end(s);
    HIPCHK(h->err, hipGetLastError());
  } else {
    const int nb = red_blocks(P0);
    prof_begin("bce_loss_grad", 0.0, 12.0 * P0, s);
    hipLaunchKernelGGL(unet::bce_loss_grad_kernel, dim3(nb), dim3(256), 0, s, ws + p.logits, targets, P0,
                       (float)(1.0 / (double)P0), ws + p.dlogits, partial);
    hipLaunchKernelGGL(unet::scalar_sum_finalize_kernel, dim3(1), dim3(1), 0, s, partial, nb, 1.0 / (double)P0,
                       lossDev);
    prof_end(s);
    HIPCHK(h->err, hipGetLastError());
  }
  return UNET_OK;
}

// out_channels > 1: the class loss over (N,K,H,W) logits against uint8 labels, its terms to lossDev, its gradient to dlogits
int run_class_loss_grad(unet_ctx* h, const uint8_t* labels, int n, size_t hw, float* lossDev, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  float* ws = reinterpret_cast<float*>(T->ws.p);
  if (!T->classWork) HIPCHK(h->err, hipMalloc(&T->classWork, unet::class_loss_work_bytes()));
  prof_begin("class_loss_grad", 0.0, (8.0 * h->cfg.out_channels + 2.0) * n * hw, s);
  const hipError_t e = unet::launch_class_loss_grad(ws + p.logits, labels, n, hw, h->cfg.out_channels, T->classLoss, T->classWork,
                                                    lossDev, ws + p.dlogits, s);
  prof_end(s);
  HIPCHK(h->err, e);
  return UNET_OK;
}

// ConvTranspose2d backward of decoder step j, on the upper channel half of dCat[l] (n x ch x cw pixels): db, dW, and the
// gradient w.r.t. the transposed convolution's input (botA2 / decA2[l + 1]) into gA
int upconv_backward(unet_ctx* h, int j, int n, int ch, int cw, float* gA, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  const int l = h->cfg.depth - 1 - j;
  const int f = h->cfg.features[l];
  float* ws = reinterpret_cast<float*>(T->ws.p);
  float* partial = ws + p.partial;
  UpUnit& U = T->up[j];
  const int lh = ch / 2, lw = cw / 2;
  const size_t Pl = (size_t)n * lh * lw;
  float* S = ws + p.s2d;
  const float* dY = ws + p.dCat[l];
  if (p.planes && U.x3Dgrad && U.x3Fwd && train_x3_wgrad_enabled()) {
    // f16x3: the bias gradient is the column sum of the gradient slice itself; the same pass takes max |.|, the
    // space-to-depth pass writes the scaled operand planes, both GEMMs run on the fp16 pipe
    unsigned* key = T->up_keys(j);
    float* inv = T->up_inv(j);
    HIPCHK(h->err, run_up_bias_grad_x3(dY, 2 * f, f, Pl * 4, f, partial, key, T->grads + U.offB, s));
    // (the slot: the previous level's weight gradient reads S on the side stream)
    const int rc = backward_with_wgrad(
        h, s, side_on(T) ? SideStream::kUpSlot : -1,
        [&]() -> int {
          HIPCHK(h->err, run_up_s2d_planes_x3(dY, 2 * f, f, n, lh, lw, f, key, S, inv, s));
          return UNET_OK;
        },
        [&](hipStream_t st) {
          return run_wgrad1_x3(S, 4 * f, 4 * f, ws + p.upInP[j], U.cin, U.cin, (long)Pl, ws + p.slab, p.slabFloats,
                               T->grads + U.offW, 1, f, inv, st);
        },
        [&]() -> int {
          HIPCHK(h->err, run_gemm1x1_x3(U.x3Dgrad, x3_from(reinterpret_cast<const uint16_t*>(zero_page()), reinterpret_cast<const uint16_t*>(S),
                                                           Pl * 4 * (size_t)f, n, lh, lw).to(nullptr, 0, U.cin),
                                        4 * f, U.cin, gA, inv, "upconv_dgrad_f16x3", s));
          return UNET_OK;
        });
    if (rc) return rc;
    if (T->dbgStage == 200 + j)   // the fp32 form of S only exists for the snapshot
      hipLaunchKernelGGL(unet::space_to_depth_kernel, dim3(grid_for(Pl * 4 * (f / 4))), dim3(256), 0, s, dY, 2 * f, f, n, lh,
                         lw, f, S);
  } else {
    const float* upIn = (j == 0) ? ws + p.botA2 : ws + p.decA2[l + 1];
    HIPCHK(h->err, T->side.join(s));   // S and the slab are used on s below
    prof_begin("space_to_depth", 0.0, 8.0 * Pl * 4 * f, s);
    hipLaunchKernelGGL(unet::space_to_depth_kernel, dim3(grid_for(Pl * 4 * (f / 4))), dim3(256), 0, s, dY, 2 * f, f, n, lh,
                       lw, f, S);
    prof_end(s);
    {
      const int nb = red_blocks(Pl);
      prof_begin("bias_grad", 0.0, 4.0 * Pl * 4 * f, s);
      hipLaunchKernelGGL(unet::colsum_partial_kernel, dim3(nb), dim3(256), 0, s, S, 4 * f, 0, Pl, 4 * f, partial,
                         (unsigned*)nullptr);
      hipLaunchKernelGGL(unet::colsum_finalize_kernel, dim3((f + unet::FIN_CH - 1) / unet::FIN_CH), dim3(256), 0, s, partial, nb, 4 * f, f,
                         T->grads + U.offB);
      prof_end(s);
    }
    HIPCHK(h->err, hipGetLastError());
    HIPCHK(h->err, run_wgrad(S, 4 * f, upIn, U.cin, U.cin, 1, n, lh, lw, ws + p.slab, p.slabFloats,
                             T->grads + U.offW, 1, f, s));
    HIPCHK(h->err, run_gemm_op(U.dgrad, S, n, lh, lw, gA, U.cin, 0, s));  // gradient w.r.t. the upconv input
  }
  if (T->dbgStage == 100 + j) hipMemcpyAsync(T->dbgDst, gA, std::min(T->dbgMax, Pl * U.cin) * 4, hipMemcpyDeviceToDevice, s);
  if (T->dbgStage == 200 + j) hipMemcpyAsync(T->dbgDst, S, std::min(T->dbgMax, Pl * 4 * f) * 4, hipMemcpyDeviceToDevice, s);
  return UNET_OK;
}

// Backward of the head, the decoder (shallowest level first: the reverse of the forward order) and the bottleneck; leaves
// the gradient w.r.t. pool[D-1] in the workspace's gA
int backward_decoder(unet_ctx* h, int n, int height, int width, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  const unet_config& c = h->cfg;
  const int D = c.depth, f0 = c.features[0];
  const bool PM = p.planes;
  float* ws = reinterpret_cast<float*>(T->ws.p);
  float *gA = ws + p.gA, *gB = ws + p.gB, *gZ = ws + p.gZ;
  const size_t P0 = (size_t)n * height * width;
  int rc;
  // The gradient w.r.t. the last unit's activation is dlogits[p] * w_head[c]: its BatchNorm backward forms that product
  // itself instead of reading a P0 x f0 buffer written here (3 x 4 bytes per element less; same bits).  A debug snapshot
  // keeps the buffer.
  const bool headRank1 = T->dbgStage < 0 && c.out_channels == 1;
  if (c.out_channels > 1) {   // K-way head: dA dense into gA, dW (K, f0) and db (K) through block partials
    prof_begin("headk_bwd", 4.0 * P0 * f0 * c.out_channels, 4.0 * P0 * (2 * f0 + c.out_channels), s);
    const hipError_t e = unet::launch_headk_backward(ws + p.dlogits, ws + p.decA2[0], T->params + T->offHeadW, n,
                                                     (size_t)height * width, f0, c.out_channels, gA, ws + p.partial,
                                                     T->grads + T->offHeadW, T->grads + T->offHeadB, s);
    prof_end(s);
    HIPCHK(h->err, e);
  } else {  // head: dW, db; dA (dense f0) into gA unless headRank1
    const int nb = red_blocks(P0);
    prof_begin("head_bwd", 0.0, 4.0 * P0 * ((headRank1 ? 1 : 2) * f0 + 1), s);
    hipLaunchKernelGGL(unet::head_bwd_kernel, dim3(nb), dim3(256), 0, s, ws + p.dlogits, ws + p.decA2[0],
                       T->params + T->offHeadW, P0, f0, headRank1 ? (float*)nullptr : gA, ws + p.partial);
    hipLaunchKernelGGL(unet::reduce2_finalize_kernel, dim3((f0 + unet::FIN_CH - 1) / unet::FIN_CH), dim3(256), 0, s, ws + p.partial, nb, f0,
                       T->grads + T->offHeadW, gB /* per-channel copies of sum(dl); column 0 is db */);
    prof_end(s);
    HIPCHK(h->err, hipMemcpyAsync(T->grads + T->offHeadB, gB, sizeof(float), hipMemcpyDeviceToDevice, s));
  }
  int ch = height, cw = width;
  for (int j = D - 1; j >= 0; --j) {
    const int l = D - 1 - j;
    const int f = c.features[l];
    // conv2: dA in gA (dense f) -> input gradient (w.r.t. decA1) into gB
    const bool r1 = headRank1 && j == D - 1;
    if ((rc = unit_backward(h, T->dec[2 * j + 1], gA, f, 0, ws + p.decZ2[l], ws + p.decA1[l], f, n, ch, cw, gZ, gB, f,
                            0, p, s, PM ? ws + p.decA1[l] : nullptr, r1 ? ws + p.dlogits : nullptr,
                            r1 ? T->params + T->offHeadW : nullptr)))
      return rc;
    // conv1: dA in gB -> gradient w.r.t. the concat buffer (2f channels) into dCat[l]
    if ((rc = unit_backward(h, T->dec[2 * j], gB, f, 0, ws + p.decZ1[l], ws + p.cat[l], 2 * f, n, ch, cw, gZ,
                            ws + p.dCat[l], 2 * f, 0, p, s, PM ? ws + p.catP[l] : nullptr)))
      return rc;
    if ((rc = upconv_backward(h, j, n, ch, cw, gA, s, p))) return rc;
    ch /= 2;
    cw /= 2;
  }
  // bottleneck (gA holds the gradient w.r.t. botA2)
  const int fl = c.features[D - 1], fb = 2 * fl;
  if ((rc = unit_backward(h, T->bott[1], gA, fb, 0, ws + p.botZ2, ws + p.botA1, fb, n, ch, cw, gZ, gB, fb, 0, p, s,
                          PM ? ws + p.botA1 : nullptr)))
    return rc;
  // gradient w.r.t. pool[D-1] into gA (dense fl channels)
  return unit_backward(h, T->bott[0], gB, fb, 0, ws + p.botZ1, ws + p.pool[D - 1], fl, n, ch, cw, gZ, gA, fl, 0, p, s,
                       PM ? ws + p.pool[D - 1] : nullptr);
}

// Backward of the encoder, deepest level first; gA = gradient w.r.t. pool[l]
int backward_encoder(unet_ctx* h, int n, int height, int width, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  const unet_config& c = h->cfg;
  const int D = c.depth;
  const bool PM = p.planes;
  float* ws = reinterpret_cast<float*>(T->ws.p);
  float *gA = ws + p.gA, *gB = ws + p.gB, *gZ = ws + p.gZ;
  int rc;
  for (int l = D - 1; l >= 0; --l) {
    const int f = c.features[l];
    const int ch = height >> l, cw = width >> l;   // even: check_shape (a pooling follows this level)
    const size_t P = (size_t)n * ch * cw;
    // dA(conv2 output) = skip half of dCat[l] + unpooled gA   -> gB (dense f)
    // ... with the first pass of that unit's BatchNorm backward in the same kernel (UNET_TRAIN_POOL_FUSED=0: separately)
    int poolRows = 0;
    if (train_pool_fused() && T->dbgStage < 0) {
      ConvUnit& u2 = T->enc[2 * l + 1];
      poolRows = red_blocks(P / 4);
      prof_begin("maxpool_bwd_add_bnstat", 0.0, 4.0 * P * f * 4.25, s);
      hipLaunchKernelGGL(unet::maxpool_bwd_add_bnstat_kernel, dim3(poolRows), dim3(256), 0, s, ws + p.cat[l], 2 * f,
                         ws + p.dCat[l], 2 * f, 0, gA, n, ch, cw, f, gB, ws + p.encZ2[l], u2.mean, u2.invstd, ws + p.partial,
                         T->unit_keys(u2));
      prof_end(s);
    } else {
      prof_begin("maxpool_bwd_add", 0.0, 4.0 * P * f * 3.25, s);
      hipLaunchKernelGGL(unet::maxpool_bwd_add_kernel, dim3(grid_for((P / 4) * (f / 4))), dim3(256), 0, s, ws + p.cat[l],
                         2 * f, ws + p.dCat[l], 2 * f, 0, gA, n, ch, cw, f, gB);
      prof_end(s);
    }
    HIPCHK(h->err, hipGetLastError());
    if ((rc = unit_backward(h, T->enc[2 * l + 1], gB, f, 0, ws + p.encZ2[l], ws + p.encA1[l], f, n, ch, cw, gZ, gA, f,
                            0, p, s, PM ? ws + p.encA1[l] : nullptr, nullptr, nullptr, poolRows)))
      return rc;
    const float* xin = (l == 0) ? ws + p.x0 : ws + p.pool[l - 1];
    const int ldx = (l == 0) ? 4 : c.features[l - 1];
    if ((rc = unit_backward(h, T->enc[2 * l], gA, f, 0, ws + p.encZ1[l], xin, ldx, n, ch, cw, gZ,
                            (l == 0) ? nullptr : gB, ldx, 0, p, s, (PM && l > 0) ? xin : nullptr)))
      return rc;
    if (l > 0) std::swap(gA, gB);  // the input gradient (w.r.t. pool[l-1]) is now in gA
  }
  return UNET_OK;
}

// targets: float (N,1,H,W) of a single-class handle; labels: uint8 (N,H,W) of a K-class handle - the other one null
int train_forward_backward(unet_ctx* h, int n, int height, int width, const float* targets, const uint8_t* labels,
                           float* lossDev, float* logitsOut, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  LaunchScope scope(h);
  float* ws = reinterpret_cast<float*>(T->ws.p);
  const size_t P0 = (size_t)n * height * width;
  int rc;
  if ((rc = repack_if_switched(h, s))) return rc;
  if ((rc = forward_walk(h, Pass::Train, n, height, width, ws + p.logits, s, p))) return rc;
  if (logitsOut)
    HIPCHK(h->err, hipMemcpyAsync(logitsOut, ws + p.logits, P0 * h->cfg.out_channels * sizeof(float), hipMemcpyDeviceToDevice, s));
  if ((rc = labels ? run_class_loss_grad(h, labels, n, (size_t)height * width, lossDev, s, p)
                   : run_loss_grad(h, targets, P0, lossDev, s, p)))
    return rc;
  // backward.  Whatever return ends it, the caller's stream has been joined with the side stream and no slot is left
  // busy: a caller that reuses the workspace, the gradients or the slab after an error meets no weight gradient in flight
  SideJoinOnExit joinOnExit{T->side, s};
  T->side.nextUnit = 0;
  HIPCHK(h->err, hipMemsetAsync(T->gzKeys, 0, 8 * T->scaled_units() * sizeof(unsigned), s));
  if ((rc = backward_decoder(h, n, height, width, s, p))) return rc;
  // Every gradient of the decoder, the bottleneck and the head is final now: they are the tail of the flat buffer
  // (unet_train_grad_split).  A data-parallel caller's communication stream may start reducing that tail while the
  // encoder's backward still runs.
  if (T->commStream) {
    HIPCHK(h->err, T->side.join(s));   // ... once the side stream's weight gradients are in
    if (!T->lateGradsReady) HIPCHK(h->err, hipEventCreateWithFlags(&T->lateGradsReady, hipEventDisableTiming));
    HIPCHK(h->err, hipEventRecord(T->lateGradsReady, s));
    HIPCHK(h->err, hipStreamWaitEvent(T->commStream, T->lateGradsReady, 0));
  }
  if ((rc = backward_encoder(h, n, height, width, s, p))) return rc;
  HIPCHK(h->err, T->side.join(s));   // the caller's stream owns every gradient again
  return h->async_error();
}

int train_eval_forward(unet_ctx* h, int n, int height, int width, float* logitsOut, hipStream_t s, const TrainPlan& p) {
  TrainState* T = h->train;
  LaunchScope scope(h);
  int rc;
  if ((rc = repack_if_switched(h, s))) return rc;
  if ((rc = eval_init(h))) return rc;
  prof_begin("eval_bn_fold", 0.0, 24.0 * T->B, s);
  const hipError_t ef = unet::launch_bn_eval_fold(T->evalDescs, T->nEvalUnits, kBnEps, s);
  prof_end(s);
  HIPCHK(h->err, ef);
  if ((rc = forward_walk(h, Pass::Eval, n, height, width, logitsOut, s, p))) return rc;
  return h->async_error();
}

}  // namespace

static void train_free(unet_ctx* h) {
  TrainState* T = h->train;
  if (!T) return;
  for (ConvUnit* u : T->units) {
    u->fwd.scale = u->fwd.shift = nullptr;  // shared ones/zeros arrays, freed below
    u->dgrad.scale = u->dgrad.shift = nullptr;
    u->fwd.free_dev();
    u->dgrad.free_dev();
    if (u->x3Fwd) hipFree(u->x3Fwd);
    if (u->x3Dgrad) hipFree(u->x3Dgrad);
    u->x3Fwd = u->x3Dgrad = nullptr;
  }
  for (auto& u : T->up) {
    u.fwd.scale = nullptr;
    u.dgrad.scale = u.dgrad.shift = nullptr;
    u.fwd.free_dev();  // owns its shift (bias) array
    u.dgrad.free_dev();
    if (u.x3Fwd) hipFree(u.x3Fwd);
    if (u.x3Dgrad) hipFree(u.x3Dgrad);
    u.x3Fwd = u.x3Dgrad = nullptr;
  }
  if (T->ones) hipFree(T->ones);
  if (T->zeros) hipFree(T->zeros);
  if (T->statArena) hipFree(T->statArena);
  if (T->lossCoef) hipFree(T->lossCoef);
  if (T->classWork) hipFree(T->classWork);
  if (T->evalArena) hipFree(T->evalArena);
  if (T->evalDescs) hipFree(T->evalDescs);
  if (T->lateGradsReady) hipEventDestroy(T->lateGradsReady);
  T->side.destroy();
  if (T->gzKeys) hipFree(T->gzKeys);
  if (T->gzInv) hipFree(T->gzInv);
  if (T->packDescs) hipFree(T->packDescs);
  if (T->packX3Descs) hipFree(T->packX3Descs);
  if (T->packX3Start) hipFree(T->packX3Start);
  if (T->packStart) hipFree(T->packStart);
  T->ws.release();
  delete T;
  h->train = nullptr;
}

extern "C" {

int unet_train_debug_snapshot(unet_handle_t h, int stage, float* dst, size_t maxFloats) {
  if (!h || !h->train) return UNET_ERR_STATE;
  h->train->dbgStage = stage;
  h->train->dbgDst = dst;
  h->train->dbgMax = maxFloats;
  return UNET_OK;
}

size_t unet_train_param_numel(unet_handle_t h) {
  if (!h) return 0;
  size_t n = 0;
  for (const auto& s : h->spec)
    if (s.name.find("running_") == std::string::npos) n += s.numel;
  return n;
}

size_t unet_train_buffer_numel(unet_handle_t h) {
  if (!h) return 0;
  size_t n = 0;
  for (const auto& s : h->spec)
    if (s.name.find("running_") != std::string::npos) n += s.numel;
  return n;
}

int unet_train_layout(unet_handle_t h, int index, int* isBuffer, size_t* offset) {
  if (!h || index < 0 || index >= (int)h->spec.size() || !isBuffer || !offset) return UNET_ERR_INVALID_ARG;
  size_t po = 0, bo = 0;
  for (int i = 0; i < index; ++i) {
    if (h->spec[i].name.find("running_") != std::string::npos)
      bo += h->spec[i].numel;
    else
      po += h->spec[i].numel;
  }
  *isBuffer = h->spec[index].name.find("running_") != std::string::npos;
  *offset = *isBuffer ? bo : po;
  return UNET_OK;
}

int unet_train_attach(unet_handle_t h, float* params, float* grads, float* expAvg, float* expAvgSq, float* bnBuffers) {
  if (!h || !params || !grads || !expAvg || !expAvgSq || !bnBuffers) return UNET_ERR_INVALID_ARG;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  train_free(h);
  TrainState* T = new TrainState();
  h->train = T;
  T->params = params;
  T->grads = grads;
  T->m = expAvg;
  T->v = expAvgSq;
  T->bn = bnBuffers;
  T->P = unet_train_param_numel(h);
  T->B = unet_train_buffer_numel(h);
  T->isBuffer.resize(h->spec.size());
  T->offset.resize(h->spec.size());
  for (size_t i = 0; i < h->spec.size(); ++i) {
    int b;
    size_t o;
    unet_train_layout(h, (int)i, &b, &o);
    T->isBuffer[i] = b;
    T->offset[i] = o;
  }
  const unet_config& c = h->cfg;
  int maxN = 64, statFloats = 0;
  auto off = [&](const std::string& name) { return T->offset[spec_index(h, name)]; };
  auto makeUnit = [&](const std::string& prefix, int convIdx, int bnIdx, int cin, int cout, int level, bool dgrad) {
    ConvUnit u;
    u.prefix = prefix;
    u.convIdx = convIdx;
    u.bnIdx = bnIdx;
    u.cin = cin;
    u.cout = cout;
    u.level = level;
    u.needDgrad = dgrad;
    u.offW = off(prefix + "." + std::to_string(convIdx) + ".weight");
    const std::string bn = prefix + "." + std::to_string(bnIdx) + ".";
    u.offG = off(bn + "weight");
    u.offB = off(bn + "bias");
    u.offRM = off(bn + "running_mean");
    u.offRV = off(bn + "running_var");
    statFloats += 4 * round_up(cout, 64);
    return u;
  };
  int cin = c.in_channels;
  for (int l = 0; l < c.depth; ++l) {
    const std::string p = "encoder_blocks." + std::to_string(l);
    T->enc.push_back(makeUnit(p, 0, 1, cin, c.features[l], l, l > 0));
    T->enc.push_back(makeUnit(p, 3, 4, c.features[l], c.features[l], l, true));
    cin = c.features[l];
  }
  const int fl = c.features[c.depth - 1];
  T->bott.push_back(makeUnit("bottleneck", 0, 1, fl, 2 * fl, c.depth, true));
  T->bott.push_back(makeUnit("bottleneck", 3, 4, 2 * fl, 2 * fl, c.depth, true));
  for (int j = 0; j < c.depth; ++j) {
    const int l = c.depth - 1 - j;
    const int f = c.features[l];
    UpUnit U;
    U.cin = 2 * f;
    U.cout = f;
    U.offW = off("decoder_blocks." + std::to_string(2 * j) + ".weight");
    U.offB = off("decoder_blocks." + std::to_string(2 * j) + ".bias");
    T->up.push_back(U);
    const std::string p = "decoder_blocks." + std::to_string(2 * j + 1);
    T->dec.push_back(makeUnit(p, 0, 1, 2 * f, f, l, true));
    T->dec.push_back(makeUnit(p, 3, 4, f, f, l, true));
  }
  for (auto* vec : {&T->enc, &T->bott, &T->dec})   // the one place that fixes the order of TrainState::units
    for (auto& u : *vec) {
      u.dbgId = (int)T->units.size();
      T->units.push_back(&u);
    }
  T->offHeadW = off("output.weight");
  T->offHeadB = off("output.bias");

  int rc;
  HIPCHK(h->err, hipMalloc((void**)&T->statArena, (size_t)statFloats * sizeof(float)));
  float* sp = T->statArena;
  for (ConvUnit* unit : T->units) {
    ConvUnit& u = *unit;
    const int cp = round_up(u.cout, 64);
    u.scale = sp;
    u.shift = sp + cp;
    u.mean = sp + 2 * cp;
    u.invstd = sp + 3 * cp;
    sp += 4 * cp;
    // the first layer reads the 4-channel packed input: GEMM K = 4 with a zero weight row for the pad channel
    const int kFwd = u.cin;
    if ((rc = alloc_gemm(h->err, u.fwd, 9, kFwd, u.cout, u.cout, round_up(u.cout, 16)))) return rc;
    u.fwd.name = "conv3x3_igemm_f32";
    u.fwd.nameWino = "conv3x3_wino_f32";
    maxN = std::max(maxN, u.fwd.nTotal);
    if (u.needDgrad) {
      if ((rc = alloc_gemm(h->err, u.dgrad, 9, u.cout, u.cin, u.cin, round_up(u.cin, 16)))) return rc;
      u.dgrad.name = "dgrad3x3_igemm_f32";
      u.dgrad.nameWino = "dgrad3x3_wino_f32";
      maxN = std::max(maxN, u.dgrad.nTotal);
    }
    if (u.cin % 64 == 0 && u.cout % 64 == 0 && u.cin <= 1024 && u.cout <= 1024) {
      const size_t halfs = x3_conv_pack_halfs(u.cout, u.cin);   // the same count for both operators
      HIPCHK(h->err, hipMalloc((void**)&u.x3Fwd, halfs * sizeof(uint16_t)));
      if (u.needDgrad) HIPCHK(h->err, hipMalloc((void**)&u.x3Dgrad, halfs * sizeof(uint16_t)));
    }
  }
  for (auto& U : T->up) {
    const int cp = round_up(U.cout, 16);
    if ((rc = alloc_gemm(h->err, U.fwd, 1, U.cin, 4 * cp, U.cout, cp))) return rc;
    HIPCHK(h->err, hipMalloc((void**)&U.fwd.shift, (size_t)U.fwd.nTotal * sizeof(float)));
    if ((rc = alloc_gemm(h->err, U.dgrad, 1, 4 * U.cout, U.cin, U.cin, round_up(U.cin, 16)))) return rc;
    U.dgrad.plain = 1;
    U.dgrad.name = "upconv_dgrad_igemm_f32";
    if (U.cin % 64 == 0 && U.cout % 64 == 0 && U.cout <= 1024) {
      HIPCHK(h->err, hipMalloc((void**)&U.x3Fwd, x3_upconv_pack_halfs(U.cin, U.cout) * sizeof(uint16_t)));
      HIPCHK(h->err, hipMalloc((void**)&U.x3Dgrad, x3_upconv_dgrad_pack_halfs(U.cin, U.cout) * sizeof(uint16_t)));
    }
    maxN = std::max(maxN, std::max(U.fwd.nTotal, U.dgrad.nTotal));
  }
  HIPCHK(h->err, hipMalloc((void**)&T->ones, (size_t)maxN * sizeof(float)));
  HIPCHK(h->err, hipMalloc((void**)&T->zeros, (size_t)maxN * sizeof(float)));
  hipLaunchKernelGGL(fill_kernel, dim3(4), dim3(256), 0, 0, T->ones, (size_t)maxN, 1.0f);
  hipLaunchKernelGGL(fill_kernel, dim3(4), dim3(256), 0, 0, T->zeros, (size_t)maxN, 0.0f);
  for (ConvUnit* u : T->units) {
    u->fwd.scale = u->dgrad.scale = T->ones;
    u->fwd.shift = u->dgrad.shift = T->zeros;
  }
  for (auto& U : T->up) {
    U.fwd.scale = T->ones;
    U.dgrad.scale = T->ones;
    U.dgrad.shift = T->zeros;
  }
  HIPCHK(h->err, hipMalloc((void**)&T->lossCoef, 2 * sizeof(float)));
  HIPCHK(h->err, hipMalloc((void**)&T->gzKeys, 8 * T->scaled_units() * sizeof(unsigned)));
  HIPCHK(h->err, hipMalloc((void**)&T->gzInv, T->scaled_units() * sizeof(float)));
  HIPCHK(h->err, hipMemset(T->gzKeys, 0, 8 * T->scaled_units() * sizeof(unsigned)));
  rc = train_repack(h, 0);
  if (rc) return rc;
  HIPCHK(h->err, hipDeviceSynchronize());
  return UNET_OK;
}

int unet_train_set_loss(unet_handle_t h, int mode, float bceWeight, float diceWeight, float posWeight, float smooth) {
  if (int rc = single_class_only(h, "unet_train_set_loss")) return rc;
  if (!h || !h->train || (mode != 0 && mode != 1)) return UNET_ERR_INVALID_ARG;
  h->train->lossMode = mode;
  h->train->bceW = bceWeight;
  h->train->diceW = diceWeight;
  h->train->posWeight = posWeight;
  h->train->diceSmooth = smooth;
  return UNET_OK;
}

namespace {
unet::LossParams loss_params_of(const unet_loss_config& c) {
  return unet::LossParams{c.bce_weight, c.focal_weight, c.dice_weight, c.pos_weight, c.alpha, c.gamma, c.smooth};
}
}  // namespace

// The loss of the step from one structure: modes 0 and 1 are unet_train_set_loss; mode 2 is the general loss of
// loss_kernels.h, its parameters checked before anything else (so the check needs no attached training state).
int unet_train_set_loss_cfg(unet_handle_t h, const unet_loss_config* cfg) {
  if (!h || !cfg) return UNET_ERR_INVALID_ARG;
  if (int rc = single_class_only(h, "unet_train_set_loss_cfg")) return rc;
  if (cfg->mode == 0 || cfg->mode == 1)
    return unet_train_set_loss(h, cfg->mode, cfg->bce_weight, cfg->dice_weight, cfg->pos_weight, cfg->smooth);
  if (cfg->mode != 2 || !unet::loss_params_valid(loss_params_of(*cfg))) return UNET_ERR_INVALID_ARG;
  if (!h->train) return UNET_ERR_STATE;
  TrainState* T = h->train;
  T->lossMode = 2;
  T->bceW = cfg->bce_weight;
  T->diceW = cfg->dice_weight;
  T->posWeight = cfg->pos_weight;
  T->diceSmooth = cfg->smooth;
  T->focalW = cfg->focal_weight;
  T->focalAlpha = cfg->alpha;
  T->focalGamma = cfg->gamma;
  return UNET_OK;
}

// Re-derive every packed MFMA operand from the attached parameter buffer (after the caller overwrote it, e.g. on
// checkpoint load).  Keeps the TrainState: loss configuration and workspace survive, unlike a second attach.
int unet_train_repack(unet_handle_t h, void* stream) {
  if (!h || !h->train) return UNET_ERR_STATE;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  LaunchScope scope(h);
  int rc = train_repack(h, (hipStream_t)stream);
  if (rc) return rc;
  HIPCHK(h->err, hipStreamSynchronize((hipStream_t)stream));
  return UNET_OK;
}

// Data-parallel overlap.  The backward pass finishes the gradients of the decoder, the bottleneck and the head - the
// tail [unet_train_grad_split, unet_train_param_numel) of the flat gradient buffer - before it starts on the encoder.
// With a communication stream set, unet_train_forward_backward_* makes that stream wait (event) for the point where
// the tail is final, so an all-reduce of the tail enqueued on it overlaps the encoder's backward; the head
// [0, split) is reduced after the call as before.  NULL switches the event off.
int unet_train_set_comm_stream(unet_handle_t h, void* commStream) {
  if (!h || !h->train) return UNET_ERR_STATE;
  h->train->commStream = (hipStream_t)commStream;
  return UNET_OK;
}

size_t unet_train_grad_split(unet_handle_t h) {
  if (!h) return 0;
  size_t n = 0;
  for (const auto& s : h->spec) {
    if (s.name.rfind("encoder_blocks.", 0) != 0) break;   // spec order: encoder, decoder, bottleneck, head
    if (s.name.find("running_") == std::string::npos) n += s.numel;
  }
  return n;
}

// Process-wide switch: 1 (default) = forward and input-gradient 3x3 convolutions of the training step on the
// split-operand fp16 kernel where the channel counts allow it, 0 = exact-fp32 kernels everywhere.  Returns the previous
// setting.  Environment UNET_TRAIN_X3=0 sets the initial value to 0.
int unet_set_train_side(int mode) {
  const int prev = train_side_mode();
  if (mode >= 0 && mode <= 2) g_trainSide = mode;
  return prev;
}

int unet_set_train_x3(int on) {
  const int prev = train_x3_enabled() ? 1 : 0;
  g_trainX3 = on ? 1 : 0;
  return prev;
}

size_t unet_train_workspace_bytes(unet_handle_t h, int n, int height, int width) {
  if (!h || check_shape(h, n, height, width)) return 0;
  return plan_train(h->cfg, n, height, width).total * sizeof(float);
}

int unet_train_forward_backward_u8(unet_handle_t h, const uint8_t* frames, const float* targets, int n, int height,
                                   int width, float* lossDev, float* logitsDev, void* stream) {
  TrainPlan p;
  int rc = single_class_only(h, "unet_train_forward_backward_u8");
  if (!rc) rc = train_prologue(h, frames, targets, lossDev, n, height, width, p);
  if (rc) return rc;
  if (h->cfg.in_channels != 3) return UNET_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * height * width;
  const unet_config& c = h->cfg;
  hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames,
                     reinterpret_cast<float*>(h->train->ws.p) + p.x0, npix, c.input_mean[0], c.input_mean[1],
                     c.input_mean[2], c.input_std[0], c.input_std[1], c.input_std[2]);
  HIPCHK(h->err, hipGetLastError());
  return train_forward_backward(h, n, height, width, targets, nullptr, lossDev, logitsDev, s, p);
}

int unet_train_forward_backward_f32(unet_handle_t h, const float* image, const float* targets, int n, int height,
                                    int width, float* lossDev, float* logitsDev, void* stream) {
  TrainPlan p;
  int rc = single_class_only(h, "unet_train_forward_backward_f32");
  if (!rc) rc = train_prologue(h, image, targets, lossDev, n, height, width, p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * height * width;
  hipLaunchKernelGGL(unet::pack_nchw_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, image,
                     reinterpret_cast<float*>(h->train->ws.p) + p.x0, n, (size_t)height * width, h->cfg.in_channels);
  HIPCHK(h->err, hipGetLastError());
  return train_forward_backward(h, n, height, width, targets, nullptr, lossDev, logitsDev, s, p);
}

// The step of a K-class handle: uint8 labels (N,H,W) in place of the float targets, the class loss in place of BCE
int unet_train_forward_backward_labels_u8(unet_handle_t h, const uint8_t* frames, const uint8_t* labels, int n, int height,
                                          int width, float* lossDev, float* logitsDev, void* stream) {
  TrainPlan p;
  int rc = multi_class_only(h, "unet_train_forward_backward_labels_u8");
  if (!rc) rc = train_prologue(h, frames, reinterpret_cast<const float*>(labels), lossDev, n, height, width, p);
  if (rc) return rc;
  if (h->cfg.in_channels != 3) return UNET_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * height * width;
  const unet_config& c = h->cfg;
  hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames,
                     reinterpret_cast<float*>(h->train->ws.p) + p.x0, npix, c.input_mean[0], c.input_mean[1],
                     c.input_mean[2], c.input_std[0], c.input_std[1], c.input_std[2]);
  HIPCHK(h->err, hipGetLastError());
  return train_forward_backward(h, n, height, width, nullptr, labels, lossDev, logitsDev, s, p);
}

int unet_train_forward_backward_labels_f32(unet_handle_t h, const float* image, const uint8_t* labels, int n, int height,
                                           int width, float* lossDev, float* logitsDev, void* stream) {
  TrainPlan p;
  int rc = multi_class_only(h, "unet_train_forward_backward_labels_f32");
  if (!rc) rc = train_prologue(h, image, reinterpret_cast<const float*>(labels), lossDev, n, height, width, p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * height * width;
  hipLaunchKernelGGL(unet::pack_nchw_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, image,
                     reinterpret_cast<float*>(h->train->ws.p) + p.x0, n, (size_t)height * width, h->cfg.in_channels);
  HIPCHK(h->err, hipGetLastError());
  return train_forward_backward(h, n, height, width, nullptr, labels, lossDev, logitsDev, s, p);
}

// The loss of a K-class handle: the configuration is checked first, so that answer does not depend on the handle's state
int unet_train_set_class_loss(unet_handle_t h, const unet_class_loss_config* cfg) {
  if (!h || !cfg) return UNET_ERR_INVALID_ARG;
  if (int rc = multi_class_only(h, "unet_train_set_class_loss")) return rc;
  unet::ClassLossParams lp;
  lp.ceW = cfg->ce_weight, lp.diceW = cfg->dice_weight, lp.smooth = cfg->smooth, lp.ignore = cfg->ignore_index;
  for (int k = 0; k < UNET_MAX_CLASSES; ++k) lp.cw[k] = cfg->class_weight[k];
  if (!unet::class_loss_params_valid(lp, h->cfg.out_channels)) {
    h->err = "unet_train_set_class_loss: weights >= 0 and not both 0, smooth > 0, class weights >= 0 and finite, "
             "ignore_index -1 or 0..255";
    return UNET_ERR_INVALID_ARG;
  }
  if (!h->train) return UNET_ERR_STATE;
  h->train->classLoss = lp;
  return UNET_OK;
}

int unet_train_adam_step(unet_handle_t h, int step, float lr, float beta1, float beta2, float eps, float weightDecay,
                         int decoupled, float gradScale, void* stream) {
  if (!h || !h->train || step < 1) return UNET_ERR_INVALID_ARG;
  TrainState* T = h->train;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const double bc1 = 1.0 - std::pow((double)beta1, step);
  const double bc2 = 1.0 - std::pow((double)beta2, step);
  LaunchScope scope(h);
  prof_begin("adam", 0.0, 28.0 * T->P, s);
  hipLaunchKernelGGL(unet::adam_kernel, dim3(grid_for(T->P)), dim3(256), 0, s, T->params, T->grads, T->m, T->v, T->P,
                     lr, beta1, beta2, eps, weightDecay, decoupled, (float)bc1, (float)std::sqrt(bc2), gradScale);
  prof_end(s);
  HIPCHK(h->err, hipGetLastError());
  prof_begin("repack_weights", 0.0, 12.0 * T->P, s);
  int rc = train_repack(h, s);
  prof_end(s);
  return rc;
}

// unet_train_adam_step with the gradient multiplier formed on the device from a record of unet_grad_accumulate_f32
// (global-norm clipping; include/unet_hip.h), and no update at all when the record counts a non-finite gradient.  The
// host reads nothing: the repack runs either way (on unchanged parameters it reproduces the packs it overwrites).
int unet_train_adam_step_rec(unet_handle_t h, int step, float lr, float beta1, float beta2, float eps, float weightDecay,
                             int decoupled, float gradScale, float maxNorm, const double* recordDev, void* stream) {
  if (!h || !h->train || step < 1) return UNET_ERR_INVALID_ARG;
  if (!recordDev || (reinterpret_cast<uintptr_t>(recordDev) & 7u)) return UNET_ERR_INVALID_ARG;
  if (!(maxNorm > 0.f)) return UNET_ERR_INVALID_ARG;   // a NaN too
  TrainState* T = h->train;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  hipStream_t s = (hipStream_t)stream;
  const double bc1 = 1.0 - std::pow((double)beta1, step);
  const double bc2 = 1.0 - std::pow((double)beta2, step);
  LaunchScope scope(h);
  prof_begin("adam_rec", 0.0, 28.0 * T->P, s);
  hipLaunchKernelGGL(unet::adam_rec_kernel, dim3(grid_for(T->P)), dim3(256), 0, s, T->params, T->grads, T->m, T->v, T->P,
                     lr, beta1, beta2, eps, weightDecay, decoupled, (float)bc1, (float)std::sqrt(bc2), gradScale,
                     (double)maxNorm, recordDev);
  prof_end(s);
  HIPCHK(h->err, hipGetLastError());
  prof_begin("repack_weights", 0.0, 12.0 * T->P, s);
  int rc = train_repack(h, s);
  prof_end(s);
  return rc;
}

// Eval-mode forward on the attached parameters and BatchNorm buffers (reference README.md:2087-2099): see
// train_eval_forward.  Logits (N,1,H,W) to logitsDev; no training state is written.
int unet_train_eval_u8(unet_handle_t h, const uint8_t* frames, int n, int height, int width, float* logitsDev,
                       void* stream) {
  TrainPlan p;
  int rc = eval_prologue(h, frames, logitsDev, n, height, width, p);
  if (rc) return rc;
  if (h->cfg.in_channels != 3) return UNET_ERR_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * height * width;
  const unet_config& c = h->cfg;
  hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames,
                     reinterpret_cast<float*>(h->train->ws.p) + p.x0, npix, c.input_mean[0], c.input_mean[1],
                     c.input_mean[2], c.input_std[0], c.input_std[1], c.input_std[2]);
  HIPCHK(h->err, hipGetLastError());
  return train_eval_forward(h, n, height, width, logitsDev, s, p);
}

int unet_train_eval_f32(unet_handle_t h, const float* image, int n, int height, int width, float* logitsDev,
                        void* stream) {
  TrainPlan p;
  int rc = eval_prologue(h, image, logitsDev, n, height, width, p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t npix = (size_t)n * height * width;
  hipLaunchKernelGGL(unet::pack_nchw_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, image,
                     reinterpret_cast<float*>(h->train->ws.p) + p.x0, n, (size_t)height * width, h->cfg.in_channels);
  HIPCHK(h->err, hipGetLastError());
  return train_eval_forward(h, n, height, width, logitsDev, s, p);
}

// Segmentation metrics and validation loss of one batch, added to 16 running accumulators on the device (reference
// README.md:2101-2110, :2115-2120, :4177-4184): see include/unet_hip.h.  No host synchronisation.
int unet_seg_metrics_accumulate(int device, const float* logitsDev, const void* targetsDev, int targetsAreU8,
                                size_t numel, float thresholdLogit, int lossMode, float bceWeight, float diceWeight,
                                float posWeight, float smooth, double* accDev, void* stream) {
  if (!logitsDev || !targetsDev || !accDev || numel == 0 || (lossMode != 0 && lossMode != 1)) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = std::min<unsigned>(grid_for(numel), 1024);
  double* partial = nullptr;
  HIPCHK(g_opErr, hipMallocAsync((void**)&partial, (size_t)nb * unet::SEG_PARTIALS * sizeof(double), s));
  const hipError_t e = unet::launch_seg_metrics(logitsDev, targetsDev, targetsAreU8 != 0, numel, thresholdLogit, lossMode,
                                                  bceWeight, diceWeight, posWeight, smooth, partial, nb, accDev, s);
  HIPCHK(g_opErr, hipFreeAsync(partial, s));
  return op_done(e, s, kOpNoSync);
}

// The same reduction with the loss given as a structure; mode 2 runs the general loss (loss_kernels.h) and adds the
// batch's focal term to accumulator 10.
int unet_seg_metrics_accumulate_cfg(int device, const float* logitsDev, const void* targetsDev, int targetsAreU8,
                                    size_t numel, float thresholdLogit, const unet_loss_config* cfg, double* accDev,
                                    void* stream) {
  if (!cfg) return op_bad_args();
  if (cfg->mode == 0 || cfg->mode == 1)
    return unet_seg_metrics_accumulate(device, logitsDev, targetsDev, targetsAreU8, numel, thresholdLogit, cfg->mode,
                                       cfg->bce_weight, cfg->dice_weight, cfg->pos_weight, cfg->smooth, accDev, stream);
  const unet::LossParams lp = loss_params_of(*cfg);
  if (!logitsDev || !targetsDev || !accDev || numel == 0 || cfg->mode != 2 || !unet::loss_params_valid(lp))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  void* scratch = nullptr;
  HIPCHK(g_opErr, hipMallocAsync(&scratch, unet::seg_metrics_cfg_scratch_bytes(numel), s));
  const hipError_t e = unet::launch_seg_metrics_cfg(logitsDev, targetsDev, targetsAreU8 != 0, numel, thresholdLogit, lp,
                                                      scratch, accDev, s);
  HIPCHK(g_opErr, hipFreeAsync(scratch, s));
  return op_done(e, s, kOpNoSync);
}

// Test entry: the general loss and its logit gradient through launch_loss_grad, the helper the training step calls.
int unet_op_loss_grad(int device, const float* logitsDev, const float* targetsDev, size_t numel,
                      const unet_loss_config* cfg, float* lossTermsDev, float* dlogitsDev, void* stream) {
  if (!logitsDev || !targetsDev || !cfg || !lossTermsDev || !dlogitsDev || numel == 0 || cfg->mode != 2)
    return op_bad_args();
  const unet::LossParams lp = loss_params_of(*cfg);
  if (!unet::loss_params_valid(lp)) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  void* scratch = nullptr;
  HIPCHK(g_opErr, hipMallocAsync(&scratch, unet::loss_scratch_bytes(numel), s));
  const hipError_t e = unet::launch_loss_grad(logitsDev, targetsDev, numel, lp, scratch, lossTermsDev, dlogitsDev, s);
  HIPCHK(g_opErr, hipFreeAsync(scratch, s));
  return op_done(e, s, kOpNoSync);
}

// Positive pixels per mask (reference README.md:2514-2530, :2544-2553): see include/unet_hip.h.
int unet_mask_positive_counts(int device, const uint8_t* masksDev, int n, size_t pixelsPerImage, int threshold,
                              unsigned long long* countsDev, void* stream) {
  if (!masksDev || !countsDev || n <= 0 || pixelsPerImage == 0) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  return op_done(unet::launch_mask_positive_counts(masksDev, n, pixelsPerImage, threshold, countsDev, s), s, kOpNoSync);
}

// Dice metric of the validation loop (reference README.md:2115-2120) on device buffers; out_dev holds 4 floats.
int unet_dice_metric(int device, const float* logitsDev, const float* targetsDev, size_t numel, float thresholdLogit,
                     float smooth, float* outDev, void* stream) {
  if (!logitsDev || !targetsDev || !outDev || numel == 0) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const unsigned nb = std::min<unsigned>(grid_for(numel), 1024);
  float* partial = nullptr;
  HIPCHK(g_opErr, hipMallocAsync((void**)&partial, (size_t)nb * 3 * sizeof(float), s));
  hipLaunchKernelGGL(unet::dice_metric_partial_kernel, dim3(nb), dim3(256), 0, s, logitsDev, targetsDev, numel,
                     thresholdLogit, partial);
  hipLaunchKernelGGL(unet::dice_metric_finalize_kernel, dim3(1), dim3(64), 0, s, partial, (int)nb, smooth, outDev);
  const hipError_t e = hipGetLastError();
  HIPCHK(g_opErr, hipFreeAsync(partial, s));
  return op_done(e, s, kOpNoSync);
}

// Test entry: dW of a 3x3 convolution.  dz (N,H,W,Cout) and x (N,H,W,Cin) dense device buffers -> dw_dev (Cout,Cin,3,3).
int unet_op_wgrad3x3(int device, const float* dz, const float* x, int n, int hh, int ww, int cin, int cout,
                     float* dwDev, void* stream) {
  if (!dz || !x || !dwDev || cin % 4 || cout % 4) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  const size_t tiles = (size_t)(round_up(cout, 64) / 64) * (round_up(cin, 64) / 64);
  const size_t splits = std::max<size_t>(1, 1536 / tiles);
  const size_t slabFloats = splits * 9 * (size_t)round_up(cout, 64) * round_up(cin, 64);
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  float* slab = nullptr;
  hipError_t e = sc.get(&slab, slabFloats * sizeof(float));
  if (e == hipSuccess) e = run_wgrad(dz, cout, x, cin, cin, 9, n, hh, ww, slab, slabFloats, dwDev, 0, 0, s);
  return op_done(e, s);
}

// Test entry: the same weight gradient through the split-operand kernel (wgrad_x3_ws.h).  scaled != 0: dz is first
// scaled into the fp16 range by the power of two derived from its maximum, as the training step does for gradients.
int unet_op_wgrad3x3_x3(int device, const float* dz, const float* x, int n, int hh, int ww, int cin, int cout,
                        float* dwDev, int scaled, void* stream) {
  if (!dz || !x || !dwDev || cin % 64 || cout % 64 || hh % 2) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const size_t px = (size_t)n * hh * ww;
  const size_t tiles = (size_t)(cout / 64) * (cin / 64);
  const size_t slabFloats = wgrad_x3_splits(tiles, std::max<size_t>(1, px / 32)) * 9 * (size_t)cout * cin;
  OpScratch sc(s);
  float *slab = nullptr, *dzP = nullptr, *xP = nullptr, *inv = nullptr;
  unsigned* key = nullptr;
  hipError_t e = sc.get(&slab, slabFloats * sizeof(float));
  if (e == hipSuccess) e = sc.get(&dzP, px * cout * sizeof(float));
  if (e == hipSuccess) e = sc.get(&xP, px * cin * sizeof(float));
  if (e == hipSuccess) e = sc.get(&inv, 64);
  if (e == hipSuccess) e = sc.get(&key, 64, true);
  if (e == hipSuccess) {
    if (scaled) {
      hipLaunchKernelGGL(unet::absmax_key_kernel, dim3(256), dim3(256), 0, s, dz, px * cout, key);
      split_to_planes(dz, px * cout, dzP, s, key, inv);
    } else {
      split_to_planes(dz, px * cout, dzP, s);
    }
    split_to_planes(x, px * cin, xP, s);
    e = run_wgrad_x3(dzP, xP, cout, cin, n, hh, ww, slab, slabFloats, dwDev, scaled ? inv : nullptr, s);
  }
  return op_done(e, s);
}

// ---- test entry points of the training step's MFMA operators (include/unet_hip.h, "The training step's f16x3 operators"):
//      fp32 device weights in PyTorch layout, packed by the device packers; the run_* helpers of unit_forward /
//      unit_backward / the transposed convolution's backward; scratch, keys and range word owned by the call ----

}  // extern "C"

namespace {
// the unit scale / zero shift of the training operators (TrainState::ones / zeros), c floats each
hipError_t op_ones_zeros(OpScratch& sc, TrainState& T, int c) {
  hipError_t e = sc.get(&T.ones, (size_t)c * sizeof(float));
  if (e == hipSuccess) e = sc.get(&T.zeros, (size_t)c * sizeof(float), true);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fill_kernel, dim3(4), dim3(256), 0, sc.s, T.ones, (size_t)c, 1.0f);   // as unet_train_create
  return hipGetLastError();
}
}  // namespace

extern "C" {

int unet_op_train_conv3x3_x3(int device, const uint16_t* xPlanes, const float* xF32, int scaled, int n, int hh, int ww,
                             int cin, int cout, const float* wDev, int mode, int packer, int tileWidth, float* y, int ldo,
                             int off, float* statPartialDev, int statCapRows, int* statRowsOut, float* invOut, int* pathOut,
                             int* rangeOut, void* stream) {
  X3Force force;   // (the f16q8 forms have no fp32 epilogue)
  if (ldo == 0) ldo = cout;
  if ((xPlanes == nullptr) == (xF32 == nullptr) || (scaled && !xF32) || !wDev || !y || n < 1 || hh < 1 || ww < 1 || cin < 64 ||
      cin % 64 || cin > 1024 || cout < 64 || cout % 64 || cout > unet::X3Shape<32>::MAX_COUT || (mode != 0 && mode != 1) ||
      (packer != 0 && packer != 1) || (packer == 1 && (reinterpret_cast<uintptr_t>(wDev) & 15)) ||
      !x3_decode_force(tileWidth, &force) || force.family == kX3Q8 || ldo % 64 || off < 0 || off % 64 ||
      off + cout > ldo || (statPartialDev && (!statRowsOut || (size_t)statCapRows * 2 * cout > kPartialFloats)))
    return op_bad_args();
  // the epilogue writes its rows straight into the caller's buffer, so the room must be there before the structure and
  // its grid are known: at most 256 blocks x 4 rows (run_conv_x3)
  if (statRowsOut) *statRowsOut = 0;
  if (statPartialDev && statCapRows < 256 * 4) {
    *statRowsOut = 256 * 4;
    return op_bad_args();
  }
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (invOut) *invOut = 1.f;
  const size_t elems = (size_t)n * hh * ww * cin;
  OpScratch sc(s);
  TrainState T;
  OpRangeScope range;
  X3Path path;
  uint16_t *wt = nullptr, *wtOther = nullptr;
  float *planes = nullptr, *inv = nullptr;
  unsigned *key = nullptr, *start = nullptr;
  unet::PackX3Desc* desc = nullptr;
  int rows = 0;
  hipError_t e = op_ones_zeros(sc, T, cout);
  if (e == hipSuccess) e = sc.get(&wt, x3_conv_pack_halfs(cout, cin) * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.get(&key, 64, true);
  if (e == hipSuccess) e = sc.get(&inv, 64, true);
  if (e == hipSuccess && xF32) e = sc.get(&planes, elems * sizeof(float));
  if (e == hipSuccess && !zero_page()) e = hipErrorOutOfMemory;
  if (e == hipSuccess && packer == 1) {
    // the table train_repack builds for this layer: its forward and its input-gradient operator, one launch; the one
    // `mode` selects is used, the other goes to scratch
    e = sc.get(&wtOther, x3_conv_pack_halfs(cout, cin) * sizeof(uint16_t));
    std::vector<unet::PackX3Desc> d;
    std::vector<unsigned> st{0};
    if (mode == 0)
      pack_x3_table_add(d, st, wDev, wt, wtOther, cout, cin);
    else
      pack_x3_table_add(d, st, wDev, wtOther, wt, cin, cout);
    if (e == hipSuccess) e = sc.upload(&desc, d.data(), d.size());
    if (e == hipSuccess) e = sc.upload(&start, st.data(), st.size());
    if (e == hipSuccess) e = launch_pack_x3_lds_multi(desc, start, (int)d.size(), st.back(), s);
  } else if (e == hipSuccess) {
    launch_pack_x3(wDev, wt, cout, cin, mode, s);
  }
  if (e == hipSuccess) e = hipGetLastError();
  if (e == hipSuccess) e = range.arm();
  if (e == hipSuccess && xF32) {
    if (scaled) {
      hipLaunchKernelGGL(unet::absmax_key_kernel, dim3(256), dim3(256), 0, s, xF32, elems, key);
      split_to_planes(xF32, elems, planes, s, key, inv);
    } else {
      split_to_planes(xF32, elems, planes, s);
    }
    e = hipGetLastError();
  }
  if (e == hipSuccess)
    e = run_train_conv_x3_planes(&T, wt, cin, cout, xF32 ? planes : reinterpret_cast<const float*>(xPlanes), n, hh, ww, y, ldo,
                                 off, mode ? "dgrad3x3_f16x3" : "conv3x3_f16x3", s, scaled ? inv : nullptr, statPartialDev,
                                 statPartialDev ? &rows : nullptr, tileWidth, &path);
  if (e == hipSuccess && scaled && invOut) e = hipMemcpyAsync(invOut, inv, sizeof(float), hipMemcpyDeviceToHost, s);
  const int st = op_done(e, s, kOpMapCodes, &range, rangeOut);
  T.ones = T.zeros = nullptr;   // owned by sc
  path_to_ints(path, pathOut);
  if (statPartialDev) *statRowsOut = rows;
  return st;
}

int unet_op_upconv_bwd_x3(int device, const float* dY, int ldd, int offd, const uint16_t* inPlanes, const float* wDev, int n,
                          int lh, int lw, int f, float* db, float* dW, float* dIn, float* invOut, int* structureOut,
                          void* stream) {
  const int cin = 2 * f, rowsG = 4 * f;
  if (!dY || !inPlanes || !wDev || !db || !dW || !dIn || n < 1 || lh < 1 || lw < 1 || f < 64 || f % 64 || f > 512 ||
      rowsG % 128 || cin % 128 || ldd % 4 || offd < 0 || offd % 4 || offd + f > ldd)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  if (structureOut) *structureOut = 0;
  const size_t Pl = (size_t)n * lh * lw;
  const size_t tiles = (size_t)(rowsG / 128) * (cin / 128);
  const size_t slabFloats = wgrad_x3_splits(tiles, (Pl + 31) / 32) * (size_t)rowsG * cin;
  OpScratch sc(s);
  float *S = nullptr, *partial = nullptr, *inv = nullptr, *slab = nullptr;
  unsigned* key = nullptr;
  uint16_t* wt = nullptr;
  int structure = 0;
  hipError_t e = sc.get(&S, Pl * 4 * f * sizeof(float));
  if (e == hipSuccess) e = sc.get(&partial, kPartialFloats * sizeof(float));
  if (e == hipSuccess) e = sc.get(&slab, slabFloats * sizeof(float));
  if (e == hipSuccess) e = sc.get(&wt, x3_upconv_dgrad_pack_halfs(cin, f) * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.get(&key, 64, true);
  if (e == hipSuccess) e = sc.get(&inv, 64, true);
  if (e == hipSuccess && !zero_page()) e = hipErrorOutOfMemory;
  if (e == hipSuccess) {
    launch_pack_upconv_dgrad_x3(wDev, wt, cin, f, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = run_up_bias_grad_x3(dY, ldd, offd, Pl * 4, f, partial, key, db, s);
  if (e == hipSuccess) e = run_up_s2d_planes_x3(dY, ldd, offd, n, lh, lw, f, key, S, inv, s);
  if (e == hipSuccess)
    e = run_wgrad1_x3(S, rowsG, rowsG, reinterpret_cast<const float*>(inPlanes), cin, cin, (long)Pl, slab, slabFloats, dW, 1, f,
                      inv, s);
  if (e == hipSuccess)
    e = run_gemm1x1_x3(wt, x3_from(reinterpret_cast<const uint16_t*>(zero_page()), reinterpret_cast<const uint16_t*>(S),
                                   Pl * 4 * (size_t)f, n, lh, lw).to(nullptr, 0, cin),
                       rowsG, cin, dIn, inv, "upconv_dgrad_f16x3", s, &structure);
  if (e == hipSuccess && invOut) e = hipMemcpyAsync(invOut, inv, sizeof(float), hipMemcpyDeviceToHost, s);
  if (structureOut) *structureOut = structure;
  return op_done(e, s, kOpMapCodes);
}

int unet_op_upconv_fwd_train_x3(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int cin, const float* wDev,
                                const float* biasDev, int cout, uint16_t* y, size_t yLo, int ldo, int coOff, int* pathOut,
                                int* rangeOut, void* stream) {
  if (ldo == 0) ldo = cout;
  if (!x || !wDev || !biasDev || !y || n < 1 || hh < 1 || ww < 1 || cin < 64 || cin % 64 || cout < 64 || cout % 64 ||
      cout > unet::UpconvX3Shape::MAX_COUT || xLo % 8 || yLo % 8 || ldo % 64 || coOff < 0 || coOff % 64 || coOff + cout > ldo)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  TrainState T;
  OpRangeScope range;
  X3Path path;
  uint16_t* wt = nullptr;
  hipError_t e = op_ones_zeros(sc, T, cout);
  if (e == hipSuccess) e = sc.get(&wt, x3_upconv_pack_halfs(cin, cout) * sizeof(uint16_t));
  if (e == hipSuccess && !zero_page()) e = hipErrorOutOfMemory;
  if (e == hipSuccess) {
    launch_pack_upconv_x3(wDev, wt, cin, cout, s);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = range.arm();
  if (e == hipSuccess) e = run_train_upconv_x3(&T, wt, biasDev, cin, cout, x, xLo, n, hh, ww, y, yLo, ldo, coOff, s, &path);
  const int st = op_done(e, s, kOpMapCodes, &range, rangeOut);
  T.ones = T.zeros = nullptr;   // owned by sc
  path_to_ints(path, pathOut);
  return st;
}

}  // extern "C"
