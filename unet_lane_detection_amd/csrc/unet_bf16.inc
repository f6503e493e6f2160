// bf16 inference tier (BASELINE.json configs[2]; included at the end of unet_hip.cpp).
//
// bf16 storage for activations and weights, fp32 accumulation, fp32 folded-BatchNorm epilogue.  The first
// convolution (3 input channels, K = 27) runs on the fp32 kernel and writes bf16; everything downstream runs
// on igemm_bf16.h.  This is a separate accuracy tier: logits differ from the fp32 oracle by ~1e-2..1e-1, so
// the north star's 1e-3 logit bound does not apply; tests state the measured band and the mask IoU.

namespace {

struct GemmOpBf {
  int taps = 9, cin = 0, cout = 0, coutPad = 0, nTotal = 0, relu = 0;
  uint16_t* wt = nullptr;
  uint16_t* wtWs = nullptr;                  // conv_bf16_ws.h packing (3x3, Cin % 64 == 0, Cout % 64 == 0)
  const uint16_t* zeros = nullptr;           // zero page for that kernel's out-of-image halo (borrowed)
  float *scale = nullptr, *shift = nullptr;  // borrowed from the fp32 op (not owned)
  void free_dev() {
    if (wt) hipFree(wt);
    if (wtWs) hipFree(wtWs);
    wt = wtWs = nullptr;
  }
};

uint16_t host_f2bf(float v) {
  uint32_t u;
  std::memcpy(&u, &v, 4);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

template <class F>
std::vector<uint16_t> pack_fragments_bf16(int nTotal, int cin, int taps, F&& col) {
  const int nSub = nTotal / 16, nChunks = cin / 32;
  std::vector<uint16_t> out(((size_t)nSub * nChunks * taps + 1) * 64 * 8, 0);
  for (int cs = 0; cs < nSub; ++cs)
    for (int kc = 0; kc < nChunks; ++kc)
      for (int t = 0; t < taps; ++t) {
        uint16_t* dst = out.data() + (((size_t)cs * nChunks + kc) * taps + t) * 64 * 8;
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 8; ++e)
            dst[lane * 8 + e] = host_f2bf(col(cs * 16 + (lane & 15), kc * 32 + (lane >> 4) * 8 + e, t));
      }
  return out;
}

// conv_bf16_ws.h: weights are the MFMA A operand (rows = output channels).  Row j of 16-channel subtile cs of
// 64-channel tile ct is channel 64*ct + 16*(j>>2) + 4*cs + (j&3), so that an accumulator lane ends up with 16
// consecutive channels of one pixel.  Layout [ct][chunk(32)][tap][cs][lane][8] plus one tap of padding (the
// kernel prefetches one tap past the end).
template <class F>
std::vector<uint16_t> pack_fragments_ws(int cout, int cin, F&& wgt) {
  const int nCt = cout / 64, nChunks = cin / 32;
  std::vector<uint16_t> out(((size_t)nCt * nChunks * 9 + 1) * 4 * 64 * 8, 0);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < nChunks; ++kc)
      for (int t = 0; t < 9; ++t)
        for (int cs = 0; cs < 4; ++cs) {
          uint16_t* dst = out.data() + ((((size_t)ct * nChunks + kc) * 9 + t) * 4 + cs) * 64 * 8;
          for (int lane = 0; lane < 64; ++lane) {
            const int j = lane & 15, lq = lane >> 4;
            const int co = 64 * ct + 16 * (j >> 2) + 4 * cs + (j & 3);
            for (int e = 0; e < 8; ++e) dst[lane * 8 + e] = host_f2bf(wgt(co, kc * 32 + lq * 8 + e, t));
          }
        }
  return out;
}

int upload_bf(std::string& err, uint16_t** dst, const std::vector<uint16_t>& v) {
  HIPCHK(err, hipMalloc((void**)dst, v.size() * sizeof(uint16_t)));
  HIPCHK(err, hipMemcpy(*dst, v.data(), v.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  return UNET_OK;
}

// The bf16 operators of a 3x3 convolution / a transposed convolution from the fp32 operator built for the same layer
// (build_conv3x3 / build_upconv: GEMM shape, folded scale / shift or bias, borrowed), w in PyTorch layout on the host.
// Used by bf16_build and by the unet_op_*_bf16 test entry points alike.  `zeros`: the tier's zero page (8192 elements).
int pack_conv_bf(std::string& err, GemmOpBf& o, const GemmOp& f, const float* w, const uint16_t* zeros) {
  o.taps = 9;
  o.cin = f.cinReal;
  o.cout = f.cout;
  o.coutPad = f.coutPad;
  o.nTotal = f.nTotal;
  o.relu = f.relu;
  o.scale = f.scale;
  o.shift = f.shift;
  const int cinR = f.cinReal, coutR = f.cout;
  auto packed = pack_fragments_bf16(o.nTotal, o.cin, 9, [&](int n, int ci, int t) -> float {
    return (n < coutR && ci < cinR) ? w[((size_t)n * cinR + ci) * 9 + t] : 0.f;
  });
  int rc = upload_bf(err, &o.wt, packed);
  if (rc) return rc;
  if (cinR % 64 == 0 && coutR % 64 == 0) {
    auto pw = pack_fragments_ws(coutR, cinR, [&](int n, int ci, int t) -> float {
      return w[((size_t)n * cinR + ci) * 9 + t];
    });
    rc = upload_bf(err, &o.wtWs, pw);
    o.zeros = zeros;
  }
  return rc;
}

int pack_upconv_bf(std::string& err, GemmOpBf& o, const GemmOp& f, const float* w, const uint16_t* zeros) {
  o.taps = 1;
  o.cin = f.cinReal;
  o.cout = f.cout;
  o.coutPad = f.coutPad;
  o.nTotal = f.nTotal;
  o.relu = 0;
  o.scale = f.scale;
  o.shift = f.shift;
  const int cp = o.coutPad, coutR = o.cout, cinR = o.cin;
  auto packed = pack_fragments_bf16(o.nTotal, o.cin, 1, [&](int n, int ci, int) -> float {
    const int ab = n / cp, co = n % cp;
    return (ab < 4 && co < coutR && ci < cinR) ? w[((size_t)ci * coutR + co) * 4 + ab] : 0.f;
  });
  int rc;
  if ((rc = upload_bf(err, &o.wt, packed))) return rc;
  if (cinR % 64 == 0 && coutR % 64 == 0) {
    // upconv_bf16_ws.h: [coTile(64)][chunk(64 ch)][kstep(2)][ab(4)][cs(4)][lane][8]; row j of subtile cs =
    // channel 64*ct + 16*(j>>2) + 4*cs + (j&3), k = chunk*64 + kstep*32 + 8*(lane>>4) + e
    const int nCt = coutR / 64, nCh = cinR / 64;
    std::vector<uint16_t> pw((size_t)nCt * nCh * 32 * 64 * 8, 0);
    for (int ct = 0; ct < nCt; ++ct)
      for (int kc = 0; kc < nCh; ++kc)
        for (int ks = 0; ks < 2; ++ks)
          for (int ab = 0; ab < 4; ++ab)
            for (int cs = 0; cs < 4; ++cs) {
              uint16_t* dst = pw.data() + (((((size_t)ct * nCh + kc) * 2 + ks) * 4 + ab) * 4 + cs) * 64 * 8;
              for (int lane = 0; lane < 64; ++lane) {
                const int jr = lane & 15, lq = lane >> 4;
                const int co = 64 * ct + 16 * (jr >> 2) + 4 * cs + (jr & 3);
                for (int e = 0; e < 8; ++e) {
                  const int ci = kc * 64 + ks * 32 + lq * 8 + e;
                  dst[lane * 8 + e] = host_f2bf(w[((size_t)ci * coutR + co) * 4 + ab]);
                }
              }
            }
    if ((rc = upload_bf(err, &o.wtWs, pw))) return rc;
    o.zeros = zeros;
  }
  return UNET_OK;
}

// First convolution as one K = 27 bf16 MFMA per tile with hi/lo split operands (conv_first_bf16x3.h), w (f0,3,3,3):
// [coTile][cs][hi|lo][lane][8], row j of subtile cs = channel 64*ct + 16*(j>>2) + 4*cs + (j&3), k = tap*3 + ci
int pack_first_bf16x3(std::string& err, uint16_t** dst, const float* w, int f0) {
  std::vector<uint16_t> pw((size_t)(f0 / 64) * 4 * 2 * 64 * 8, 0);
  for (int ct = 0; ct < f0 / 64; ++ct)
    for (int cs = 0; cs < 4; ++cs)
      for (int lane = 0; lane < 64; ++lane) {
        const int j = lane & 15, lq = lane >> 4;
        const int co = 64 * ct + 16 * (j >> 2) + 4 * cs + (j & 3);
        for (int e = 0; e < 8; ++e) {
          const int k = lq * 8 + e;
          float v = 0.f;
          if (k < 27) v = w[((size_t)co * 3 + (k % 3)) * 9 + k / 3];
          const uint16_t hi = host_f2bf(v);
          uint32_t hb = (uint32_t)hi << 16;
          float hf;
          std::memcpy(&hf, &hb, 4);
          const uint16_t lo = host_f2bf(v - hf);
          pw[((((size_t)ct * 4 + cs) * 2 + 0) * 64 + lane) * 8 + e] = hi;
          pw[((((size_t)ct * 4 + cs) * 2 + 1) * 64 + lane) * 8 + e] = lo;
        }
      }
  return upload_bf(err, dst, pw);
}

struct BfFuse {
  uint16_t* pool = nullptr;         // fused 2x2 max-pool output (set to nullptr by run_gemm_bf if it could not fuse)
  const float* headW = nullptr;     // fused 1x1 head
  float headB = 0.f, headThr = 0.f;
  float* logits = nullptr;
  float* probs = nullptr;
  uint8_t* mask = nullptr;
};

// Kernel choices of run_gemm_bf (also what the unet_op_*_bf16 test entry points force and report): 0 = none (the forced
// kernel cannot take the shape), 1 = igemm_bf16.h, 2 = the wave-specialised kernel (conv_bf16_ws.h / upconv_bf16_ws.h),
// 3 = the one-wave-per-SIMD kernel (conv_bf16_r512.h / upconv_bf16_r512.h).
enum : int { BF_NONE = 0, BF_IGEMM = 1, BF_WS = 2, BF_R512 = 3 };

// The eligibility rules take the unet_set_bf16_persistent mode explicitly: -1 automatic, 0 the 2x2-wave kernel alone,
// 1 the wave-specialised kernels wherever the shape allows, 2 the one-wave-per-SIMD kernels wherever the shape allows.
std::atomic<int> g_bfWsMode{-1};   // unet_set_bf16_persistent

// ---- the persistent wave-specialised kernel (conv_bf16_ws.h) for wide layers ----
bool conv_ws_eligible(const GemmOpBf& op, int n, int h, int w, int mode) {
  static const int minW = [] { const char* e = getenv("UNET_BF16_WS_MINW"); return e ? atoi(e) : 100; }();
  if (mode == 0 || !op.wtWs || !op.zeros || op.taps != 9 || h % 16 || op.cout > unet::WsShape::MAX_COUT)
    return false;
  const long work = (long)((w + 31) / 32) * (n * h / 16) * (op.cout / 64);
  if (mode == 1) return work >= 8;    // the persistent grid is work / 8 * 8 blocks: none below that
  return w >= minW && work >= 1024;   // at least four tiles per CU, else the 2x2-wave kernel's finer grain wins
}

// ---- the one-wave-per-SIMD kernel (conv_bf16_r512.h) for the 56 x 56 ... 14 x 14 levels ----
struct BfR512Plan {
  int twx, thx, wpx;
  bool flat;
  long tiles, items;
};
BfR512Plan conv_bf_r512_plan(const GemmOpBf& op, int n, int h, int w) {
  BfR512Plan p;
  p.twx = w == 14 ? 14 : 28;
  p.thx = 224 / p.twx;
  p.flat = n > 1 && h % p.thx != 0 && 2 * h >= p.thx;
  p.tiles = p.flat ? (long)((n * h + p.thx - 1) / p.thx) * (w / p.twx) : (long)n * ((h + p.thx - 1) / p.thx) * (w / p.twx);
  auto balance = [](long items) { return (double)items / (double)((items + 255) / 256 * 256); };
  p.wpx = 2;
  if (op.cout % 256 == 0) p.wpx = balance(p.tiles * (op.cout / 256)) >= 0.93 * balance(p.tiles * (op.cout / 128)) ? 1 : 2;
  p.items = p.tiles * (op.cout / (256 / p.wpx));
  return p;
}
// mode 2: wherever the shape allows; automatic: once there is an item for half the CUs; modes 0 and 1 never (the 2x2-wave
// kernel alone / the wave-specialised kernel forced)
bool conv_bf_r512_eligible(const GemmOpBf& op, int n, int h, int w, int mode) {
  if (!op.wtWs || !op.zeros || op.taps != 9 || op.cin % 32 || op.cout % 128 || !(w % 28 == 0 || w == 14)) return false;
  if (mode == 0 || mode == 1) return false;
  return mode == 2 || conv_bf_r512_plan(op, n, h, w).items >= 128;
}
hipError_t run_conv_bf_r512(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo,
                            int coOff, hipStream_t s) {
  const BfR512Plan p = conv_bf_r512_plan(op, n, h, w);
  unet::ConvBfRArgs a;
  a.in = in;
  a.wt = op.wtWs;
  a.zeros = op.zeros;
  a.scale = op.scale;
  a.shift = op.shift;
  a.out = out;
  a.N = p.flat ? 1 : n;
  a.H = p.flat ? n * h : h;
  a.W = w;
  a.Cin = op.cin;
  a.Cout = op.cout;
  a.ldo = ldo;
  a.co_off = coOff;
  a.tilesX = w / p.twx;
  a.tilesY = (a.H + p.thx - 1) / p.thx;
  a.nChunks = op.cin / 32;
  a.relu = op.relu;
  a.pixTiles = a.N * a.tilesY * a.tilesX;
  a.coTiles = op.cout / (256 / p.wpx);
  a.coGroup = a.coTiles;
  a.imgH = h;
  const int grid = (int)std::max<long>(8, std::min<long>(256, p.items / 8 * 8));
  const double px = (double)n * h * w;
  prof_begin("conv3x3_r512_bf16", 2.0 * px * 9 * op.cin * op.cout, 2.0 * (px * op.cin + px * op.cout + 9.0 * op.cin * op.cout), s);
  const hipError_t e = unet::launch_bf_r512(a, grid, p.twx, p.wpx, p.flat, s);
  prof_end(s);
  return e;
}

// upconv_bf16_r512.h: shapes it takes (Cin % 128 == 0, w >= 4); mode 2 (unet_set_bf16_persistent) whenever the shape
// allows, automatic once there is a work item for half of the CUs, modes 0 / 1 never
bool upconv_r512_wanted(const GemmOpBf& op, int n, int h, int w, int mode) {
  if (!(op.taps == 1 && op.wtWs && op.zeros && op.cin % 128 == 0 && op.cout % 64 == 0 && w >= 4 &&
        op.cout <= unet::UpconvWsShape::MAX_COUT))
    return false;
  const long workR = ((long)n * h * w + 223) / 224 * (op.cout / 64);
  return mode == 2 || (mode < 0 && workR >= 128);
}

// ---- the persistent wave-specialised transposed convolution (upconv_bf16_ws.h) ----
bool upconv_ws_eligible(const GemmOpBf& op, int n, int h, int w, int mode) {
  static const bool on = [] { const char* e = getenv("UNET_BF16_UPWS"); return !(e && e[0] == '0'); }();
  if (!on || mode == 0 || op.taps != 1 || !op.wtWs || !op.zeros || op.cout > unet::UpconvWsShape::MAX_COUT)
    return false;
  const long work = ((long)n * h * w + 127) / 128 * (op.cout / 64);
  return mode == 1 ? work >= 8 : work >= 1024;
}

unet::UpconvWsArgs upconv_bf_args(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo,
                                  int coOff, int tp) {
  unet::UpconvWsArgs a;
  a.in = in;
  a.wt = op.wtWs;
  a.zeros = op.zeros;
  a.bias = op.shift;   // (a,b) = (0,0) block of the per-column shifts = the bias
  a.out = out;
  a.npix = (long)n * h * w;
  a.h = h;
  a.w = w;
  a.Cin = op.cin;
  a.Cout = op.cout;
  a.ldo = ldo;
  a.co_off = coOff;
  a.nChunks = op.cin / 64;
  a.coTiles = op.cout / 64;
  a.pixTiles = (int)((a.npix + tp - 1) / tp);
  return a;
}

// the one-wave-per-SIMD structure (upconv_bf16_r512.h; bit-identical to the wave-specialised kernel)
hipError_t run_upconv_bf_r512(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo,
                              int coOff, hipStream_t s) {
  using R = unet::UpconvBfRShape;
  const unet::UpconvWsArgs a = upconv_bf_args(op, in, n, h, w, out, ldo, coOff, R::TP);
  const long workR = (long)a.pixTiles * a.coTiles;
  auto kernR = unet::upconv2x2_bf16_r512_kernel;
  hipError_t e = ensure_dyn_lds((const void*)kernR, R::LDS_BYTES);
  if (e != hipSuccess) return e;
  const int gridR = (int)std::max<long>(8, std::min<long>(256, workR / 8 * 8));
  const double pxr = (double)a.npix;
  prof_begin("upconv2x2_r512_bf16", 2.0 * pxr * op.cin * 4.0 * op.cout, 2.0 * (pxr * op.cin + 4.0 * pxr * op.cout), s);
  hipLaunchKernelGGL(kernR, dim3(gridR), dim3(256), (size_t)R::LDS_BYTES, s, a);
  prof_end(s);
  return hipGetLastError();
}

hipError_t run_upconv_ws(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo, int coOff,
                         hipStream_t s) {
  using S = unet::UpconvWsShape;
  const unet::UpconvWsArgs a = upconv_bf_args(op, in, n, h, w, out, ldo, coOff, S::TP);
  auto kern = unet::upconv2x2_bf16_ws_kernel;
  {
    hipError_t e = ensure_dyn_lds((const void*)kern, S::LDS_BYTES);
    if (e != hipSuccess) return e;
  }
  const long work = (long)a.pixTiles * a.coTiles;
  const int grid = (int)std::min<long>(256, work / 8 * 8);
  const double px = (double)a.npix;
  prof_begin("upconv2x2_ws_bf16", 2.0 * px * op.cin * 4.0 * op.cout, 2.0 * (px * op.cin + 4.0 * px * op.cout), s);
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)S::LDS_BYTES, s, a);
  prof_end(s);
  return hipGetLastError();
}

// Which kernel run_gemm_bf launches for this operator and shape: `force` BF_IGEMM / BF_WS / BF_R512 asks for that
// kernel (BF_NONE if it cannot take the shape), 0 = the automatic choice under the current unet_set_bf16_persistent mode.
int bf_kernel_for(const GemmOpBf& op, int n, int h, int w, int force) {
  const bool conv = op.taps == 9;
  switch (force) {
    case BF_IGEMM:
      return BF_IGEMM;
    case BF_WS:
      return (conv ? conv_ws_eligible(op, n, h, w, 1) : upconv_ws_eligible(op, n, h, w, 1)) ? BF_WS : BF_NONE;
    case BF_R512:
      return (conv ? conv_bf_r512_eligible(op, n, h, w, 2) : upconv_r512_wanted(op, n, h, w, 2)) ? BF_R512 : BF_NONE;
    default:
      break;
  }
  const int mode = g_bfWsMode;
  if (conv) {
    if (conv_ws_eligible(op, n, h, w, mode)) return BF_WS;
    if (conv_bf_r512_eligible(op, n, h, w, mode)) return BF_R512;   // no fused pooling / head: the caller's passes run
    return BF_IGEMM;
  }
  if (upconv_r512_wanted(op, n, h, w, mode)) return BF_R512;
  if (upconv_ws_eligible(op, n, h, w, mode)) return BF_WS;
  return BF_IGEMM;
}

// Returns through `fusedPool` / `fusedHead` which of the requested epilogue fusions the launch performed.
hipError_t run_conv_ws(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo, int coOff,
                       hipStream_t s, BfFuse* fuse, bool* fusedPool, bool* fusedHead) {
  unet::ConvWsArgs a;
  a.in = in;
  a.wt = op.wtWs;
  a.zeros = op.zeros;
  a.scale = op.scale;
  a.shift = op.shift;
  a.out = out;
  a.N = n;
  a.H = h;
  a.W = w;
  a.Cin = op.cin;
  a.Cout = op.cout;
  a.ldo = ldo;
  a.co_off = coOff;
  a.tilesX = (w + 31) / 32;
  a.nChunks = op.cin / 32;
  a.relu = op.relu;
  a.pixTiles = a.tilesX * (n * h / 16);
  a.coTiles = op.cout / 64;
  a.coGroup = 1;
  for (int g : {8, 4, 2})
    if (a.coTiles % g == 0) {
      a.coGroup = g;
      break;
    }
  a.pool = nullptr;
  a.headW = nullptr;
  a.headB = a.headThr = 0.f;
  a.logits = a.probs = nullptr;
  a.mask = nullptr;
  a.storeOut = 1;
  if (fusedPool) *fusedPool = false;
  if (fusedHead) *fusedHead = false;
  if (fuse) {
    if (fuse->pool && op.relu && h % 2 == 0 && w % 2 == 0) {   // packed-bf16 max needs non-negative values
      a.pool = fuse->pool;
      if (fusedPool) *fusedPool = true;
    }
    if (fuse->headW && op.cout == 64) {
      a.headW = fuse->headW;
      a.headB = fuse->headB;
      a.headThr = fuse->headThr;
      a.logits = fuse->logits;
      a.probs = fuse->probs;
      a.mask = fuse->mask;
      a.storeOut = 0;
      if (fusedHead) *fusedHead = true;
    }
  }
  a.stamps = nullptr;
#if UNET_WS_STAMPS
  static unsigned long long* stampBuf = nullptr;
  if (!stampBuf) hipMalloc((void**)&stampBuf, 256 * 8 * sizeof(unsigned long long));
  a.stamps = stampBuf;
#endif
  const int epi = a.headW ? 2 : (a.pool ? 1 : 0);
  const int work = a.pixTiles * a.coTiles;
  const int grid = std::min(256, work / 8 * 8);
  const double px = (double)n * h * w;
  prof_begin("conv3x3_ws_bf16", 2.0 * px * 9 * op.cin * op.cout,
             2.0 * (px * op.cin + px * op.cout + 9.0 * op.cin * op.cout), s);
  const hipError_t e = unet::launch_bf_ws(a, grid, epi, s);
  prof_end(s);
#if UNET_WS_STAMPS
  {
    hipStreamSynchronize(s);
    unsigned long long hb[256 * 8];
    hipMemcpy(hb, stampBuf, sizeof(hb), hipMemcpyDeviceToHost);
    double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int b = 0; b < grid; ++b)
      for (int k = 0; k < 8; ++k) t[k] += (double)hb[b * 8 + k] / grid;
    const double tiles = (double)work / grid;
    fprintf(stderr, "ws stamps %dx%d cin %d cout %d, per tile (s_memtime ticks): mfma wave %.0f = loop %.0f + barrier %.0f "
            "+ epilogue %.0f | loader %.0f: dma wait %.0f barrier %.0f\n", h, w, op.cin, op.cout, t[0] / tiles,
            (t[0] - t[1] - t[2]) / tiles, t[1] / tiles, t[2] / tiles, t[6] / tiles, t[4] / tiles, t[5] / tiles);
  }
#endif
  return e;
}

// ---- the 2x2-wave kernel (igemm_bf16.h): every shape, the 3x3 convolution and the transposed convolution ----
hipError_t run_igemm_bf(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo, int coOff,
                        hipStream_t s, BfFuse* fuse, bool* fusedPool, bool* fusedHead) {
  const TileChoice t = choose_tile(n * h, w, 16, op.taps == 9);   // same 64-byte pixel rows as fp32 CK=16
  unet::ConvArgsBf a;
  a.pool = nullptr;
  a.headW = nullptr;
  a.headB = a.headThr = 0.f;
  a.logits = a.probs = nullptr;
  a.mask = nullptr;
  a.storeOut = 1;
  if (fusedPool) *fusedPool = false;
  if (fusedHead) *fusedHead = false;
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
  a.TH = t.th;
  a.TW = t.tw;
  a.tilesX = (w + t.tw - 1) / t.tw;
  a.nChunks = op.cin / 32;
  a.relu = op.relu;
  const int tilesY = (n * h + t.th - 1) / t.th;
  // 128-channel tiles halve the LDS reads of the input tile per MFMA (the bf16 kernel is LDS-bound, not MFMA-bound)
  static const bool wide = [] { const char* e = getenv("UNET_BF16_NS"); return !(e && e[0] == '2'); }();
  const int ns = (op.nTotal % 128 == 0 && (t.ms == 4 || wide)) ? 4 : 2;
  a.pixTiles = a.tilesX * tilesY;
  a.coTiles = op.nTotal / (32 * ns);
  a.coGroup = 1;
  for (int g : {8, 4, 2})
    if (a.coTiles % g == 0) {
      a.coGroup = g;
      break;
    }
  if (fuse && op.taps == 9) {
    if (fuse->pool && t.th % 4 == 0 && t.tw % 2 == 0 && h % 2 == 0 && w % 2 == 0) {
      a.pool = fuse->pool;
      if (fusedPool) *fusedPool = true;
    }
    if (fuse->headW && a.coTiles == 1 && op.cout % 4 == 0) {
      a.headW = fuse->headW;
      a.headB = fuse->headB;
      a.headThr = fuse->headThr;
      a.logits = fuse->logits;
      a.probs = fuse->probs;
      a.mask = fuse->mask;
      a.storeOut = 0;
      if (fusedHead) *fusedHead = true;
    }
  }
  const double px = (double)n * h * w;
  const double nOut = (op.taps == 9) ? op.cout : 4.0 * op.cout;
  prof_begin(op.taps == 9 ? "conv3x3_igemm_bf16" : "upconv2x2_igemm_bf16", 2.0 * px * op.taps * op.cin * nOut,
             2.0 * (px * op.cin + px * nOut + (double)op.taps * op.cin * nOut), s);
  dim3 grid((unsigned)((size_t)a.pixTiles * a.coTiles));
  hipError_t e = unet::launch_bf(a, grid, op.taps, t.ms, ns, s);
  prof_end(s);
  return e;
}

hipError_t run_gemm_bf(const GemmOpBf& op, const uint16_t* in, int n, int h, int w, uint16_t* out, int ldo, int coOff,
                       hipStream_t s, BfFuse* fuse = nullptr, bool* fusedPool = nullptr, bool* fusedHead = nullptr,
                       int force = 0, int* ran = nullptr) {
  const int k = bf_kernel_for(op, n, h, w, force);
  if (ran) *ran = k;
  if (fusedPool) *fusedPool = false;
  if (fusedHead) *fusedHead = false;
  const bool conv = op.taps == 9;
  switch (k) {
    case BF_WS:
      return conv ? run_conv_ws(op, in, n, h, w, out, ldo, coOff, s, fuse, fusedPool, fusedHead)
                  : run_upconv_ws(op, in, n, h, w, out, ldo, coOff, s);
    case BF_R512:
      return conv ? run_conv_bf_r512(op, in, n, h, w, out, ldo, coOff, s) : run_upconv_bf_r512(op, in, n, h, w, out, ldo, coOff, s);
    case BF_IGEMM:
      return run_igemm_bf(op, in, n, h, w, out, ldo, coOff, s, fuse, fusedPool, fusedHead);
    default:
      return hipErrorInvalidValue;
  }
}

// MaxPool2d(2,2) of (N,H,W,ldi) bf16 -> dense (N,H/2,W/2,C) (when the convolution before it could not fuse it)
hipError_t run_maxpool_bf(const uint16_t* in, uint16_t* out, int n, int h, int w, int c, int ldi, hipStream_t s) {
  const size_t total = (size_t)n * (h / 2) * (w / 2) * (c / 8);
  prof_begin("maxpool2x2_bf16", 0.0, 2.0 * total * 8 * 5, s);
  hipLaunchKernelGGL(unet::maxpool2x2_bf16_kernel, dim3(grid_for(total)), dim3(256), 0, s, in, out, n, h, w, c, ldi);
  prof_end(s);
  return hipGetLastError();
}

// 1x1 head on dense (npix, c) bf16 activations (when the last convolution could not fuse it); headW on the device
hipError_t run_head_bf(const uint16_t* in, const float* headW, float headB, size_t npix, int c, float* logits,
                       float* probs, uint8_t* mask, float thr, hipStream_t s) {
  int lpp = 1;
  while (lpp < 16 && lpp * 2 * 8 <= c) lpp *= 2;
  const unsigned g = grid_for(npix, 256 / lpp);
  prof_begin("head1x1_bf16", 2.0 * npix * c, 2.0 * npix * c + 4.0 * npix, s);
#define HEADBF(L)                                                                                                  \
  hipLaunchKernelGGL((unet::head1x1_bf16_kernel<L>), dim3(g), dim3(256), 0, s, in, headW, headB, npix, c, logits, \
                     probs, mask, thr)
  switch (lpp) {
    case 1: HEADBF(1); break;
    case 2: HEADBF(2); break;
    case 4: HEADBF(4); break;
    case 8: HEADBF(8); break;
    default: HEADBF(16); break;
  }
#undef HEADBF
  prof_end(s);
  return hipGetLastError();
}

// First convolution on conv_first_bf16x3.h: uint8 (N,H,W,3) frames -> dense (N,H,W,Cout) bf16 (H % 8 == 0,
// Cout % 64 == 0); wt from pack_first_bf16x3
hipError_t run_first_bf16x3(const uint8_t* frames, const uint16_t* wt, const float* scale, const float* shift,
                            uint16_t* out, int n, int h, int w, int cout, int relu, const float* mean, const float* std_,
                            hipStream_t s) {
  unet::ConvFirstArgs fa;
  fa.frames = frames;
  fa.wt = wt;
  fa.scale = scale;
  fa.shift = shift;
  fa.out = out;
  fa.N = n;
  fa.H = h;
  fa.W = w;
  fa.Cout = cout;
  fa.ldo = cout;
  fa.tilesX = (w + 31) / 32;
  fa.relu = relu;
  fa.m0 = mean[0];
  fa.m1 = mean[1];
  fa.m2 = mean[2];
  fa.s0 = std_[0];
  fa.s1 = std_[1];
  fa.s2 = std_[2];
  const double px = (double)n * h * w;
  prof_begin("conv3x3_first_bf16x3", 2.0 * px * 27 * cout, px * 3 + 2.0 * px * cout, s);
  hipLaunchKernelGGL(unet::conv_first_bf16x3_kernel, dim3((unsigned)(fa.tilesX * (n * h / 8))), dim3(256), 0, s, fa);
  prof_end(s);
  return hipGetLastError();
}

}  // namespace

struct Bf16Net {
  uint16_t* zeros = nullptr;
  uint16_t* firstWt = nullptr;   // conv_first_bf16x3.h packing of the first convolution (3 input channels)
  std::vector<GemmOpBf> enc, bott, up, dec;
  GrowBuf ws;
};

static void bf16_free(unet_ctx* h) {
  if (!h->bf) return;
  for (auto* v : {&h->bf->enc, &h->bf->bott, &h->bf->up, &h->bf->dec})
    for (auto& op : *v) op.free_dev();
  h->bf->ws.release();
  if (h->bf->zeros) hipFree(h->bf->zeros);
  if (h->bf->firstWt) hipFree(h->bf->firstWt);
  delete h->bf;
  h->bf = nullptr;
}

namespace {

int bf16_build(unet_ctx* h) {
  const unet_config& c = h->cfg;
  for (int l = 0; l < c.depth; ++l)
    if (c.features[l] % 32) {
      h->err = "the bf16 tier needs every feature width to be a multiple of 32";
      return UNET_ERR_INVALID_ARG;
    }
  bf16_free(h);
  h->bf = new Bf16Net();
  Bf16Net* B = h->bf;
  auto conv = [&](GemmOpBf& o, const GemmOp& f, const std::string& wname) -> int {
    return pack_conv_bf(h->err, o, f, h->params[wname].data(), B->zeros);
  };
  HIPCHK(h->err, hipMalloc((void**)&B->zeros, 8192 * sizeof(uint16_t)));
  HIPCHK(h->err, hipMemset(B->zeros, 0, 8192 * sizeof(uint16_t)));
  if (c.in_channels == 3 && c.features[0] % 64 == 0) {
    const int rcw = pack_first_bf16x3(h->err, &B->firstWt, h->params["encoder_blocks.0.0.weight"].data(), c.features[0]);
    if (rcw) return rcw;
  }
  int rc;
  B->enc.assign(2 * c.depth, GemmOpBf());
  B->dec.assign(2 * c.depth, GemmOpBf());
  B->up.assign(c.depth, GemmOpBf());
  B->bott.assign(2, GemmOpBf());
  for (int l = 0; l < c.depth; ++l) {
    const std::string p = "encoder_blocks." + std::to_string(l);
    if (l > 0 && (rc = conv(B->enc[2 * l], h->enc[2 * l], p + ".0.weight"))) return rc;  // enc[0] stays fp32
    if ((rc = conv(B->enc[2 * l + 1], h->enc[2 * l + 1], p + ".3.weight"))) return rc;
  }
  if ((rc = conv(B->bott[0], h->bott[0], "bottleneck.0.weight"))) return rc;
  if ((rc = conv(B->bott[1], h->bott[1], "bottleneck.3.weight"))) return rc;
  for (int j = 0; j < c.depth; ++j) {
    const std::string pd = "decoder_blocks." + std::to_string(2 * j + 1);
    if ((rc = conv(B->dec[2 * j], h->dec[2 * j], pd + ".0.weight"))) return rc;
    if ((rc = conv(B->dec[2 * j + 1], h->dec[2 * j + 1], pd + ".3.weight"))) return rc;
    if ((rc = pack_upconv_bf(h->err, B->up[j], h->up[j], h->params["decoder_blocks." + std::to_string(2 * j) + ".weight"].data(),
                             B->zeros)))
      return rc;
  }
  return UNET_OK;
}

struct WsPlanBf {
  size_t x0 = 0;  // fp32 (N,H,W,4), offsets in bytes
  std::vector<size_t> cat, pool;
  size_t tmpA = 0, tmpB = 0, total = 0;
};

WsPlanBf plan_ws_bf(const unet_config& c, int n, int h, int w) {
  WsPlanBf p;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
  };
  const size_t px0 = (size_t)n * h * w;
  p.x0 = take(px0 * 4 * sizeof(float));
  size_t maxT = 0;
  for (int l = 0; l < c.depth; ++l) {
    const size_t px = px0 >> (2 * l);
    p.cat.push_back(take(px * 2 * c.features[l] * 2));
    p.pool.push_back(take((px >> 2) * c.features[l] * 2));
    maxT = std::max(maxT, px * c.features[l] * 2);
  }
  maxT = std::max(maxT, (px0 >> (2 * c.depth)) * 2 * c.features[c.depth - 1] * 2);
  p.tmpA = take(maxT);
  p.tmpB = take(maxT);
  p.total = off;
  return p;
}

}  // namespace

extern "C" {

int unet_set_bf16_persistent(int mode) {
  const int prev = g_bfWsMode;
  g_bfWsMode = mode < 0 ? -1 : (mode > 2 ? 1 : mode);
  return prev;
}

// Forward in the bf16 tier: uint8 NHWC frames -> fp32 logits (N,1,H,W) / probabilities / mask, like
// unet_forward_u8.  Packs the bf16 weights on first use (after unet_finalize).
int unet_forward_u8_bf16(unet_handle_t h, const uint8_t* frames, int n, int height, int width, float* logits,
                         float* probs, uint8_t* mask, float thr, void* stream) {
  if (!h || !frames) return UNET_ERR_INVALID_ARG;
  if (int rc = single_class_only(h, "unet_forward_u8_bf16")) return rc;
  if (!h->finalized) {
    h->err = "unet_finalize has not been called";
    return UNET_ERR_STATE;
  }
  int rc = check_shape(h, n, height, width);
  if (rc) return rc;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  if (!h->bf && (rc = bf16_build(h))) return rc;
  Bf16Net* B = h->bf;
  const unet_config& c = h->cfg;
  const WsPlanBf p = plan_ws_bf(c, n, height, width);
  if ((rc = B->ws.reserve(h->err, p.total, "bf16 workspace"))) return rc;
  hipStream_t s = (hipStream_t)stream;
  LaunchScope scope(h);
  const size_t npix = (size_t)n * height * width;
  float* x0 = reinterpret_cast<float*>(B->ws.p + p.x0);
  static const bool firstOk = [] { const char* e = getenv("UNET_BF16_FIRST"); return !(e && e[0] == '0'); }();
  const bool firstFused = firstOk && B->firstWt && height % 8 == 0;
  if (!firstFused) {
    hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames, x0, npix,
                       c.input_mean[0], c.input_mean[1], c.input_mean[2], c.input_std[0], c.input_std[1],
                       c.input_std[2]);
    HIPCHK(h->err, hipGetLastError());
  }
  auto U = [&](size_t off) { return reinterpret_cast<uint16_t*>(B->ws.p + off); };
  uint16_t* tmpA = U(p.tmpA);
  uint16_t* tmpB = U(p.tmpB);
  const uint16_t* cur = nullptr;
  int ch = height, cw = width;
  for (int l = 0; l < c.depth; ++l) {
    const int f = c.features[l];
    if (l == 0 && firstFused) {
      HIPCHK(h->err, run_first_bf16x3(frames, B->firstWt, h->enc[0].scale, h->enc[0].shift, tmpA, n, ch, cw, f,
                                      h->enc[0].relu, c.input_mean, c.input_std, s));
    } else if (l == 0) {
      // first convolution on the fp32 kernel, output rounded to bf16
      HIPCHK(h->err, run_gemm_op(h->enc[0], x0, n, ch, cw, reinterpret_cast<float*>(tmpA), f, 0, s, 1));
    } else {
      HIPCHK(h->err, run_gemm_bf(B->enc[2 * l], cur, n, ch, cw, tmpA, f, 0, s));
    }
    BfFuse fz;
    fz.pool = U(p.pool[l]);
    bool pooled = false;
    HIPCHK(h->err, run_gemm_bf(B->enc[2 * l + 1], tmpA, n, ch, cw, U(p.cat[l]), 2 * f, 0, s, &fz, &pooled));
    if (!pooled) HIPCHK(h->err, run_maxpool_bf(U(p.cat[l]), U(p.pool[l]), n, ch, cw, f, 2 * f, s));
    cur = U(p.pool[l]);
    ch /= 2;
    cw /= 2;
  }
  bool headFused = false;
  const int fb = 2 * c.features[c.depth - 1];
  HIPCHK(h->err, run_gemm_bf(B->bott[0], cur, n, ch, cw, tmpA, fb, 0, s));
  HIPCHK(h->err, run_gemm_bf(B->bott[1], tmpA, n, ch, cw, tmpB, fb, 0, s));
  cur = tmpB;
  for (int j = 0; j < c.depth; ++j) {
    const int l = c.depth - 1 - j;
    const int f = c.features[l];
    HIPCHK(h->err, run_gemm_bf(B->up[j], cur, n, ch, cw, U(p.cat[l]), 2 * f, f, s));
    ch *= 2;
    cw *= 2;
    HIPCHK(h->err, run_gemm_bf(B->dec[2 * j], U(p.cat[l]), n, ch, cw, tmpA, f, 0, s));
    if (j == c.depth - 1) {
      // last DoubleConv: its only consumer is the 1x1 head, fused into the epilogue when one channel tile
      // covers all of Cout (the activation is then never written)
      BfFuse fz;
      fz.headW = h->headW;
      fz.headB = h->headB;
      fz.headThr = thr;
      fz.logits = logits;
      fz.probs = probs;
      fz.mask = mask;
      HIPCHK(h->err, run_gemm_bf(B->dec[2 * j + 1], tmpA, n, ch, cw, tmpB, f, 0, s, &fz, nullptr, &headFused));
    } else {
      HIPCHK(h->err, run_gemm_bf(B->dec[2 * j + 1], tmpA, n, ch, cw, tmpB, f, 0, s));
    }
    cur = tmpB;
  }
  if (!headFused) HIPCHK(h->err, run_head_bf(cur, h->headW, h->headB, npix, c.features[0], logits, probs, mask, thr, s));
  return h->async_error();
}

}  // extern "C"

// ---- single operators of the tier (test entry points): bf16 NHWC device tensors in and out, weights in PyTorch layout
//      on the host, packed by the same functions as bf16_build; include/unet_hip.h ----

namespace {

void clear_path(int* path) {
  if (path) path[0] = path[1] = path[2] = 0;
}

// The operator of one test call as bf16_build makes it: the fp32 operator of the layer (taps 9: build_conv3x3 with
// scale / shift; taps 1: build_upconv with `shift` as the bias), the tier's zero page, the tier's packing.  A forced
// kernel that does not take the shape is refused here, after the allocations.
int bf_op_build(OpScratch& sc, GemmOp& f, GemmOpBf& op, int taps, const float* w, int cin, int cout, const float* scale,
                const float* shift, int relu, int n, int hh, int ww, int kernel) {
  int rc = taps == 9 ? build_conv3x3(g_opErr, f, w, cout, cin, scale, shift, relu ? 1 : 0)
                     : build_upconv(g_opErr, f, w, cin, cout, shift);
  if (rc) return rc;
  uint16_t* zeros = nullptr;
  const hipError_t e = sc.zero_page(&zeros, 8192 * sizeof(uint16_t));
  if (e != hipSuccess) return op_done(e, sc.s, kOpNoSync);
  if ((rc = taps == 9 ? pack_conv_bf(g_opErr, op, f, w, zeros) : pack_upconv_bf(g_opErr, op, f, w, zeros))) return rc;
  if (bf_kernel_for(op, n, hh, ww, kernel) == BF_NONE) {
    g_opErr = "the forced bf16 kernel does not take this shape";
    return UNET_ERR_INVALID_ARG;
  }
  return UNET_OK;
}

}  // namespace

extern "C" {

int unet_op_conv3x3_bf16(int device, const uint16_t* x, int n, int hh, int ww, int cin, const float* wHost,
                         const float* scale, const float* shift, int cout, int relu, int kernel, int ldo, int coOff,
                         uint16_t* y, uint16_t* yPool, int* pathOut, void* stream) {
  clear_path(pathOut);
  if (ldo == 0) ldo = cout;
  if (!x || !wHost || !scale || !shift || !y || n < 1 || hh < 1 || ww < 1 || cin < 32 || cin % 32 || cout < 32 ||
      cout % 32 || kernel < 0 || kernel > 3 || ldo % 32 || coOff < 0 || coOff % 32 || coOff + cout > ldo ||
      (yPool && (hh % 2 || ww % 2)))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOp> f;
  OpGuard<GemmOpBf> t;
  const int rc = bf_op_build(sc, f.op, t.op, 9, wHost, cin, cout, scale, shift, relu, n, hh, ww, kernel);
  if (rc) return rc;
  BfFuse fz;
  fz.pool = yPool;
  bool pooled = false;
  int ran = BF_NONE;
  hipError_t e = run_gemm_bf(t.op, x, n, hh, ww, y, ldo, coOff, s, yPool ? &fz : nullptr, &pooled, nullptr, kernel, &ran);
  if (pathOut) {
    pathOut[0] = ran;
    pathOut[1] = pooled ? 1 : 0;
  }
  return op_done(e, s);
}

int unet_op_conv3x3_bf16_head(int device, const uint16_t* x, int n, int hh, int ww, int cin, const float* wHost,
                              const float* scale, const float* shift, int cout, int relu, int kernel,
                              const float* headWHost, float headB, float thr, float* logits, float* probs, uint8_t* mask,
                              int* pathOut, void* stream) {
  clear_path(pathOut);
  if (!x || !wHost || !scale || !shift || !headWHost || n < 1 || hh < 1 || ww < 1 || cin < 32 || cin % 32 ||
      cout < 32 || cout % 32 || kernel < 0 || kernel > 3)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOp> f;
  OpGuard<GemmOpBf> t;
  const int rc = bf_op_build(sc, f.op, t.op, 9, wHost, cin, cout, scale, shift, relu, n, hh, ww, kernel);
  if (rc) return rc;
  const size_t npix = (size_t)n * hh * ww;
  BfFuse fz;
  uint16_t* act = nullptr;
  float* headW = nullptr;
  hipError_t e = sc.upload(&headW, headWHost, (size_t)cout);
  if (e == hipSuccess) e = sc.get(&act, npix * cout * sizeof(uint16_t));
  fz.headW = headW;
  fz.headB = headB;
  fz.headThr = thr;
  fz.logits = logits;
  fz.probs = probs;
  fz.mask = mask;
  bool headFused = false;
  int ran = BF_NONE;
  if (e == hipSuccess) e = run_gemm_bf(t.op, x, n, hh, ww, act, cout, 0, s, &fz, nullptr, &headFused, kernel, &ran);
  // as the forward: the unfused head reads the stored activation
  if (e == hipSuccess && !headFused) e = run_head_bf(act, headW, headB, npix, cout, logits, probs, mask, thr, s);
  if (pathOut) {
    pathOut[0] = ran;
    pathOut[2] = headFused ? 1 : 0;
  }
  return op_done(e, s);
}

int unet_op_upconv2x2_bf16(int device, const uint16_t* x, int n, int hh, int ww, int cin, const float* wHost,
                           const float* bias, int cout, int kernel, int ldo, int coOff, uint16_t* y, int* pathOut,
                           void* stream) {
  clear_path(pathOut);
  if (ldo == 0) ldo = cout;
  if (!x || !wHost || !bias || !y || n < 1 || hh < 1 || ww < 1 || cin < 32 || cin % 32 || cout < 32 || cout % 32 ||
      kernel < 0 || kernel > 3 || ldo % 32 || coOff < 0 || coOff % 32 || coOff + cout > ldo)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOp> f;
  OpGuard<GemmOpBf> t;
  const int rc = bf_op_build(sc, f.op, t.op, 1, wHost, cin, cout, nullptr, bias, 0, n, hh, ww, kernel);
  if (rc) return rc;
  int ran = BF_NONE;
  hipError_t e = run_gemm_bf(t.op, x, n, hh, ww, y, ldo, coOff, s, nullptr, nullptr, nullptr, kernel, &ran);
  if (pathOut) pathOut[0] = ran;
  return op_done(e, s);
}

int unet_op_conv_first_bf16(int device, const uint8_t* frames, int n, int hh, int ww, const float* wHost,
                            const float* scale, const float* shift, int cout, int relu, const float* meanHost,
                            const float* stdHost, int kernel, uint16_t* y, int* pathOut, void* stream) {
  clear_path(pathOut);
  if (!frames || !wHost || !scale || !shift || !meanHost || !stdHost || !y || n < 1 || hh < 1 || ww < 1 ||
      cout < 32 || cout % 32 || kernel < 0 || kernel > 2)
    return op_bad_args();
  // the forward's choice (unet_forward_u8_bf16): conv_first_bf16x3.h where H % 8 == 0 and Cout % 64 == 0, else the fp32
  // kernel with a bf16 store
  static const bool firstOk = [] { const char* e = getenv("UNET_BF16_FIRST"); return !(e && e[0] == '0'); }();
  const bool fusedOk = hh % 8 == 0 && cout % 64 == 0;
  if (kernel == 1 && !fusedOk) {
    g_opErr = "conv_first_bf16x3 needs H % 8 == 0 and Cout % 64 == 0";
    return UNET_ERR_INVALID_ARG;
  }
  const int k = kernel ? kernel : (firstOk && fusedOk ? 1 : 2);
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOp> f;
  int rc = build_conv3x3(g_opErr, f.op, wHost, cout, 3, scale, shift, relu ? 1 : 0);
  if (rc) return rc;
  hipError_t e;
  if (k == 1) {
    uint16_t* wtFirst = nullptr;
    rc = pack_first_bf16x3(g_opErr, &wtFirst, wHost, cout);
    sc.adopt(wtFirst);
    if (rc) return rc;
    e = run_first_bf16x3(frames, wtFirst, f.op.scale, f.op.shift, y, n, hh, ww, cout, f.op.relu, meanHost, stdHost, s);
  } else {
    const size_t npix = (size_t)n * hh * ww;
    float* x0 = nullptr;
    e = sc.get(&x0, npix * 4 * sizeof(float));
    if (e == hipSuccess) {
      hipLaunchKernelGGL(unet::pack_u8_nhwc4_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames, x0, npix, meanHost[0],
                         meanHost[1], meanHost[2], stdHost[0], stdHost[1], stdHost[2]);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = run_gemm_op(f.op, x0, n, hh, ww, reinterpret_cast<float*>(y), cout, 0, s, 1);
  }
  if (pathOut) pathOut[0] = k;
  return op_done(e, s);
}

int unet_op_maxpool2x2_bf16(int device, const uint16_t* x, int n, int hh, int ww, int c, int ldi, uint16_t* y,
                            void* stream) {
  if (ldi == 0) ldi = c;
  if (!x || !y || n < 1 || hh < 2 || ww < 2 || hh % 2 || ww % 2 || c < 8 || c % 8 || ldi % 8 || ldi < c)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  return op_done(run_maxpool_bf(x, y, n, hh, ww, c, ldi, s), s);
}

int unet_op_head1x1_bf16(int device, const uint16_t* x, int n, int hh, int ww, int c, const float* wHost, float bias,
                         float thr, float* logits, float* probs, uint8_t* mask, void* stream) {
  if (!x || !wHost || n < 1 || hh < 1 || ww < 1 || c < 8 || c % 8) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  float* headW = nullptr;
  hipError_t e = sc.upload(&headW, wHost, (size_t)c);
  if (e == hipSuccess) e = run_head_bf(x, headW, bias, (size_t)n * hh * ww, c, logits, probs, mask, thr, s);
  return op_done(e, s);
}

}  // extern "C"
