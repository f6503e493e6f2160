// Split-operand (f16x3) inference tier (included at the end of unet_hip.cpp): fp32-level accuracy on the fp16 MFMA
// pipe - every operand as fp16 hi + lo, three MFMAs per product, fp32 accumulate (csrc/conv_x3_ws.h).  Same forward
// as unet_forward_u8 / unet_forward_f32 (reference README.md:1460-1481) and the same acceptance as the exact-fp32
// tier (tests/test_x3_gpu.py runs the fp32 parity tests on it).
//
// Needs in_channels == 3 and every feature width a multiple of 64; |activation| < 65504.

namespace {

struct GemmOpX3 {   // no destructor: an owner calls free_dev(), a copy over borrowed pointers is simply dropped
  int taps = 9, cin = 0, cout = 0, relu = 0;
  uint16_t* wt = nullptr;     // packed hi/lo fragments (conv_x3_ws.h / upconv_x3_ws.h)
  float* scale = nullptr;     // per channel: folded BN scale (1 for the upconv) / the weights' power-of-two pre-scale
  float* shift = nullptr;     // folded BN shift / bias
  uint32_t* wq = nullptr;     // fp8 cross-term fragments of the f16q8 tier (conv_q8_r512.h); only where it applies
  void free_dev() {
    if (wq) hipFree(wq);
    wq = nullptr;
    if (wt) hipFree(wt);
    if (scale) hipFree(scale);
    if (shift) hipFree(shift);
    wt = nullptr;
    scale = shift = nullptr;
  }
};

inline uint16_t f16_bits(_Float16 v) {
  uint16_t u;
  std::memcpy(&u, &v, 2);
  return u;
}

// fp32 -> fp16 hi, lo (round to nearest even), as split_pk_f16 on the device
inline void host_split_f16(float v, uint16_t& hi, uint16_t& lo) {
  const _Float16 h = (_Float16)v;
  const _Float16 l = (_Float16)(v - (float)h);
  hi = f16_bits(h);
  lo = f16_bits(l);
}

// power of two that brings max |w| of an output channel into [512, 1024): lo parts stay normal fp16
inline float prescale_pow2(float maxabs) {
  if (!(maxabs > 0.f) || !std::isfinite(maxabs)) return 1.f;
  int e;
  std::frexp(maxabs, &e);          // maxabs = m * 2^e, m in [0.5, 1)
  return std::ldexp(1.f, 10 - e);  // maxabs * 2^(10-e) in [512, 1024)
}

// The lane order of every weight fragment of the tier (conv_bf16_ws.h), here and nowhere else on the host: row
// j = lane & 15 of subtile cs of channel tile ct is channel x3_frag_channel(ct, cs, j); the lane's eight halfs are
// k = 32 kc + 8 (lane >> 4) + e.  x3_each_frag_elem visits the 64 x 8 elements of one subtile fragment in memory order
inline int x3_frag_channel(int ct, int cs, int j) { return 64 * ct + 16 * (j >> 2) + 4 * cs + (j & 3); }
template <class F>
void x3_each_frag_elem(int ct, int kc, int cs, F&& f) {
  for (int lane = 0; lane < 64; ++lane)
    for (int e = 0; e < 8; ++e) f(lane * 8 + e, x3_frag_channel(ct, cs, lane & 15), kc * 32 + (lane >> 4) * 8 + e);
}
// hi / lo: the 64 x 8 halfs of subtile cs in the two planes; val(co, k): the weight, pre-scaled
template <class V>
void x3_put_frag(uint16_t* hi, uint16_t* lo, int ct, int kc, int cs, V&& val) {
  x3_each_frag_elem(ct, kc, cs, [&](int i, int co, int k) { host_split_f16(val(co, k), hi[i], lo[i]); });
}
constexpr size_t kX3Frag = 64 * 8;

// 3x3: w (O,I,3,3) -> [coTile][chunk(32)][tapRow][plane][kx][cs][lane][8]
std::vector<uint16_t> pack_conv_x3(const float* w, int cout, int cin, const std::vector<float>& pre) {
  const int nCt = cout / 64, nCh = cin / 32;
  std::vector<uint16_t> out((size_t)nCt * nCh * 3 * 2 * 3 * 4 * kX3Frag, 0);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < nCh; ++kc)
      for (int r = 0; r < 3; ++r)
        for (int kx = 0; kx < 3; ++kx)
          for (int cs = 0; cs < 4; ++cs) {
            uint16_t* row = out.data() + (((size_t)ct * nCh + kc) * 3 + r) * (2 * 3 * 4 * kX3Frag);
            x3_put_frag(row + ((0 * 3 + kx) * 4 + cs) * kX3Frag, row + ((1 * 3 + kx) * 4 + cs) * kX3Frag, ct, kc, cs,
                        [&](int co, int ci) { return w[((size_t)co * cin + ci) * 9 + r * 3 + kx] * pre[co]; });
          }
  return out;
}

// round to nearest even OCP fp8 e4m3fn, saturating (the device side converts activations with v_cvt_pk_fp8_f32)
inline uint8_t f32_to_e4m3(float v) {
  const uint8_t s = std::signbit(v) ? 0x80 : 0;
  const float a = std::fabs(v);
  if (!(a == a)) return s | 0x7F;
  if (a >= 448.f) return s | 0x7E;
  if (a == 0.f) return s;
  int e;
  std::frexp(a, &e);
  const int E = e - 1;   // a = 1.m x 2^E
  if (E < -6) return s | (uint8_t)std::nearbyint(std::ldexp(a, 9));   // subnormals: steps of 2^-9 (8 = the first normal)
  int m = (int)std::nearbyint((std::ldexp(a, -E) - 1.f) * 8.f), EE = E;
  if (m == 8) {
    m = 0;
    ++EE;
  }
  return s | (uint8_t)std::min(((EE + 7) << 3) | m, 0x7E);
}

// f16q8 tier: the cross-term operands of a 3x3 convolution, [coTile(64)][chunk(32)][step(5)][cs(4)][half(2)][lane(64)][16]:
// lane (row j = lane & 15, k group lq = lane >> 4) of step s holds, for its output channel, 32 input channels of
// fp8(2^8 w_lo) (lq even) or fp8(2^-3 w_hi) (lq odd) of the step's first tap (lq < 2) or second tap (lq >= 2; zeros for
// the ninth tap, which has no partner) - conv_q8_r512.h
std::vector<uint8_t> pack_conv_q8(const float* w, int cout, int cin, const std::vector<float>& pre) {
  const int nCt = cout / 64, nCh = cin / 32;
  static const int tapA[5] = {0, 1, 2, 6, 8}, tapB[5] = {3, 4, 5, 7, -1};
  std::vector<uint8_t> out((size_t)nCt * nCh * 5 * 4 * 2 * 64 * 16, 0);
  const float hs = std::ldexp(1.f, unet::kQ8HiShift), ls = std::ldexp(1.f, unet::kQ8LoShift);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < nCh; ++kc)
      for (int s = 0; s < 5; ++s)
        for (int cs = 0; cs < 4; ++cs)
          for (int half = 0; half < 2; ++half)
            for (int lane = 0; lane < 64; ++lane) {
              const int lq = lane >> 4;
              const int co = x3_frag_channel(ct, cs, lane & 15);
              const int tap = (lq >> 1) ? tapB[s] : tapA[s];
              uint8_t* d = out.data() + ((((((size_t)ct * nCh + kc) * 5 + s) * 4 + cs) * 2 + half) * 64 + lane) * 16;
              if (tap < 0) continue;
              for (int e = 0; e < 16; ++e) {
                const int ci = kc * 32 + half * 16 + e;
                const float v = w[((size_t)co * cin + ci) * 9 + tap] * pre[co];
                const float hi = (float)(_Float16)v;
                d[e] = (lq & 1) ? f32_to_e4m3(hi * hs) : f32_to_e4m3((float)(_Float16)(v - hi) * ls);
              }
            }
  return out;
}

// upconv: w (I,O,2,2) -> [coTile][chunk(32)][plane][ab][cs][lane][8]
std::vector<uint16_t> pack_upconv_x3(const float* w, int cin, int cout, const std::vector<float>& pre) {
  const int nCt = cout / 64, nCh = cin / 32;
  std::vector<uint16_t> out((size_t)nCt * nCh * 2 * 16 * kX3Frag, 0);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < nCh; ++kc)
      for (int ab = 0; ab < 4; ++ab)
        for (int cs = 0; cs < 4; ++cs) {
          uint16_t* chunk = out.data() + ((size_t)ct * nCh + kc) * (2 * 16 * kX3Frag);
          x3_put_frag(chunk + (0 * 16 + ab * 4 + cs) * kX3Frag, chunk + (1 * 16 + ab * 4 + cs) * kX3Frag, ct, kc, cs,
                      [&](int co, int ci) { return w[((size_t)ci * cout + co) * 4 + ab] * pre[co]; });
        }
  return out;
}

// first convolution: w (O,3,3,3) -> [coTile][cs][hi|lo][lane][8], k = tap*3 + ci (27..31 zero)
std::vector<uint16_t> pack_first_x3(const float* w, int cout, const std::vector<float>& pre) {
  std::vector<uint16_t> pw((size_t)(cout / 64) * 4 * 2 * kX3Frag, 0);
  for (int ct = 0; ct < cout / 64; ++ct)
    for (int cs = 0; cs < 4; ++cs) {
      uint16_t* sub = pw.data() + ((size_t)ct * 4 + cs) * 2 * kX3Frag;
      x3_put_frag(sub, sub + kX3Frag, ct, 0, cs,
                  [&](int co, int k) { return k < 27 ? w[((size_t)co * 3 + (k % 3)) * 9 + k / 3] * pre[co] : 0.f; });
    }
  return pw;
}

std::vector<float> row_prescale(const float* w, int rows, size_t perRow) {
  std::vector<float> pre(rows);
  for (int r = 0; r < rows; ++r) {
    float m = 0.f;
    for (size_t i = 0; i < perRow; ++i) m = std::max(m, std::fabs(w[(size_t)r * perRow + i]));
    pre[r] = prescale_pow2(m);
  }
  return pre;
}

// Activation scales.  The planes of tensor T hold T[c] * act[c] with act[c] a power of two chosen, from the parameters
// of the BatchNorm that produces T, so that four standard deviations of channel c (4 |gamma| + |beta|: the BatchNorm
// output is gamma * xhat + beta with xhat ~ N(0,1) under the running statistics) land in [512, 1024): every channel then
// uses the same part of the fp16 range whatever its gamma - small channels keep 22 significant bits (lo parts stay normal
// above 2^-13 of that scale) and the range ends 64 times above the 4-sigma point.  The consumer's weights are divided
// by act[ci] (exact), ReLU and max-pooling commute with a positive scale, so the network computes the same function.
struct ActScale {
  std::vector<float> act;   // power of two per channel
  std::vector<float> mag;   // the magnitude estimate it came from (4 sigma), for the estimates further down
};
// The power of two for an ACTIVATION magnitude.  prescale_pow2 alone overflows to +inf for a channel that is almost, but
// not exactly, dead (4 |gamma| + |beta| below 2^-118): the producer's scale and shift then become inf / NaN, the planes
// hold inf, the range watch fires on every frame and the tier is lost for good (the consumer's 1 / act = 0 would have
// been harmless).  Such a channel carries nothing: below 1e-30 it is stored unscaled, and the scale is kept inside
// [2^-40, 2^40] either way (the consumer's weights are divided by it: still far inside the fp32 range).
inline float act_scale_pow2(float mag) {
  if (!(mag >= 1e-30f)) return 1.f;
  const float s = prescale_pow2(mag);
  return std::min(std::max(s, std::ldexp(1.f, -40)), std::ldexp(1.f, 40));
}
ActScale act_from_bn(const float* gamma, const float* beta, int c) {
  ActScale a;
  a.act.resize(c);
  a.mag.resize(c);
  for (int i = 0; i < c; ++i) {
    a.mag[i] = 4.f * std::fabs(gamma[i]) + std::fabs(beta[i]);
    a.act[i] = act_scale_pow2(a.mag[i]);
  }
  return a;
}
ActScale act_concat(const ActScale& a, const ActScale& b) {
  ActScale r = a;
  r.act.insert(r.act.end(), b.act.begin(), b.act.end());
  r.mag.insert(r.mag.end(), b.mag.begin(), b.mag.end());
  return r;
}

inline bool x3_conv_has_q8(int cin, int cout) { return cin % 64 == 0 && cout % 256 == 0; }   // the 3x3 operators that get fp8 fragments
int build_conv_x3(std::string& err, GemmOpX3& op, const float* w, int cout, int cin, const float* scale,
                  const float* shift, int relu, bool first, const ActScale* in = nullptr,
                  const ActScale* out = nullptr, bool withQ8 = false) {
  op.free_dev();
  op.taps = 9;
  op.cin = cin;
  op.cout = cout;
  op.relu = relu;
  std::vector<float> wIn;   // weights with the input tensor's activation scale divided out
  if (in) {
    wIn.assign(w, w + (size_t)cout * cin * 9);
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci) {
        const float inv = 1.f / in->act[ci];
        for (int t = 0; t < 9; ++t) wIn[((size_t)co * cin + ci) * 9 + t] *= inv;
      }
    w = wIn.data();
  }
  const std::vector<float> pre = row_prescale(w, cout, (size_t)cin * 9);
  std::vector<float> sc(cout), sh(shift, shift + cout);
  for (int i = 0; i < cout; ++i) {
    const float o = out ? out->act[i] : 1.f;
    sc[i] = scale[i] / pre[i] * o;   // exact: pre and o are powers of two
    sh[i] *= o;
  }
  const std::vector<uint16_t> packed = first ? pack_first_x3(w, cout, pre) : pack_conv_x3(w, cout, cin, pre);
  int rc = upload_bf(err, &op.wt, packed);
  if (!rc && withQ8 && !first && x3_conv_has_q8(cin, cout)) {
    const std::vector<uint8_t> q = pack_conv_q8(w, cout, cin, pre);
    if (hipMalloc((void**)&op.wq, q.size()) != hipSuccess ||
        hipMemcpy(op.wq, q.data(), q.size(), hipMemcpyHostToDevice) != hipSuccess) {
      err = "f16q8 weight upload failed";
      rc = UNET_ERR_HIP;
    }
  }
  if (!rc) rc = upload(err, &op.scale, sc);
  if (!rc) rc = upload(err, &op.shift, sh);
  return rc;
}

// The transposed convolution has no BatchNorm behind it: its output scale is estimated from its weights, its bias and
// the input's magnitudes (independent channels: 4 sigma of the sum); `outEst` receives it
int build_upconv_x3(std::string& err, GemmOpX3& op, const float* w, int cin, int cout, const float* bias,
                    const ActScale* in = nullptr, ActScale* outEst = nullptr) {
  op.free_dev();
  op.taps = 1;
  op.cin = cin;
  op.cout = cout;
  op.relu = 0;
  std::vector<float> wIn;
  if (in) {
    if (outEst) {
      outEst->act.assign(cout, 1.f);
      outEst->mag.assign(cout, 0.f);
      for (int co = 0; co < cout; ++co) {
        double var = 0;
        for (int ci = 0; ci < cin; ++ci) {
          float m = 0.f;
          for (int ab = 0; ab < 4; ++ab) m = std::max(m, std::fabs(w[((size_t)ci * cout + co) * 4 + ab]));
          const double sd = in->mag[ci] / 4.0;
          var += (double)m * m * sd * sd;
        }
        outEst->mag[co] = (float)(4.0 * std::sqrt(var)) + std::fabs(bias[co]);
        outEst->act[co] = act_scale_pow2(outEst->mag[co]);
      }
    }
    wIn.assign(w, w + (size_t)cin * cout * 4);
    for (int ci = 0; ci < cin; ++ci) {
      const float inv = 1.f / in->act[ci];
      for (size_t i = 0; i < (size_t)cout * 4; ++i) wIn[(size_t)ci * cout * 4 + i] *= inv;
    }
    w = wIn.data();
  }
  std::vector<float> pre(cout, 0.f);   // per OUTPUT channel: w is (I,O,2,2)
  for (int ci = 0; ci < cin; ++ci)
    for (int co = 0; co < cout; ++co)
      for (int ab = 0; ab < 4; ++ab) pre[co] = std::max(pre[co], std::fabs(w[((size_t)ci * cout + co) * 4 + ab]));
  for (auto& p : pre) p = prescale_pow2(p);
  std::vector<float> sc(cout), sh(bias, bias + cout);
  for (int i = 0; i < cout; ++i) {
    const float o = (in && outEst) ? outEst->act[i] : 1.f;
    sc[i] = o / pre[i];
    sh[i] *= o;
  }
  int rc = upload_bf(err, &op.wt, pack_upconv_x3(w, cin, cout, pre));
  if (!rc) rc = upload(err, &op.scale, sc);
  if (!rc) rc = upload(err, &op.shift, sh);
  return rc;
}

// ---- dispatch of the tier's 3x3 and transposed convolutions (DESIGN.md, section 4.15) ----
// Which kernel runs, on which tiles and grid, is decided by x3_plan_conv / x3_plan_upconv: pure functions of integers.
// run_conv_x3 / run_upconv_x3 fill the kernel arguments from the plan and launch it; forward_x3 asks the same functions
// what a layer will do before it launches the layer's producer.

// The A/B levers of the dispatch as a plan sees them.  x3_switches() reads them: the environment once per process, the
// f16q8 switch per call.
//   UNET_X3_FLAT=0     per-image tiles everywhere (default: n > 1 images whose height is no multiple of the tile height are
//                      tiled as one tall image of n * h rows, the kernels' FLAT instances, so only the last tile pads rows)
//   UNET_X3_R512=0     every layer stays off the second structure (conv_x3_r512.h)
//   UNET_X3_T448=0     the 64- / 128-channel layers stay on the first two structures
//   UNET_X3_T448_C4=0  the second structure instead of the third's 256-channel form where both apply (the third is 1.2 -
//                      3.4 % faster per layer and has the pooled epilogue: profiles/r04/t448_c4_probe.txt)
// f16q8 tier (conv_q8_r512.h): unet_set_x3_cross_fp8.  0 = off (the f16x3 tier as tested to 2e-4), 1 = the layers
// that suit it (Cin % 64 == 0, Cout % 256 == 0, map width a multiple of 28 or 14, enough work items) form their two
// cross terms on the fp8 matrix pipe
struct X3Switches {
  bool flat = true, r512 = true, t448 = true, t448c4 = true;
  int crossFp8 = 0;
};
inline bool x3_env_off(const char* name) {   // NAME=0 in the environment
  const char* e = getenv(name);
  return e && e[0] == '0';
}
thread_local int g_x3CrossFp8 = 0;   // per calling thread: a caller's set / restore around its own forward cannot leak into another thread's
X3Switches x3_switches() {
  static const X3Switches env = [] {
    X3Switches s;
    s.flat = !x3_env_off("UNET_X3_FLAT");
    s.r512 = !x3_env_off("UNET_X3_R512");
    s.t448 = !x3_env_off("UNET_X3_T448");
    s.t448c4 = !x3_env_off("UNET_X3_T448_C4");
    return s;
  }();
  X3Switches s = env;
  s.crossFp8 = g_x3CrossFp8;
  return s;
}

struct X3Fuse {
  uint16_t* pool = nullptr;   // fused 2x2 max-pool output (hi plane)
  size_t poolLo = 0;
  const float* headW = nullptr;
  float headB = 0.f, headThr = 0.f;
  float* logits = nullptr;
  float* probs = nullptr;
  uint8_t* mask = nullptr;
};

// Scratch of the split-K path (small batches): a layer with too few work items for the chip takes it
constexpr size_t kSplitFloats = (size_t)256 * 256 * 64;
struct X3SplitK {
  float* scratch = nullptr;   // kSplit x pixels x Cout partial sums
  size_t floats = 0;
  const float* ones = nullptr;    // >= 1024 floats of 1.0 / 0.0: the split pass runs unscaled
  const float* zerosF = nullptr;
};

enum { kX3Ws = 1, kX3R512 = 2, kX3T448 = 3, kX3Q8 = 4 };   // X3Path::structure
// What a plan launches (the plane-level test entry points report it through path_out)
struct X3Path {
  int structure = 0;   // 1 = conv_x3_ws.h / upconv_x3_ws.h, 2 = conv_x3_r512.h / upconv_x3_r512.h, 3 = conv_x3_t448.h, 4 = conv_q8_r512.h
  int tileW = 0;       // pixel-tile width
  int epi = 0;         // the kernel's epilogue: 0 planes, 1 planes + fused 2x2 max-pool, 2 fused head, 3 fp32, 4 (q8) hi + q planes
  int flat = 0;        // the batch tiled as one tall image
  int kSplit = 1;      // > 1: split-K partial sums + x3_splitk_finish_kernel
  int waves = 0;       // r512: waves along the pixels (1 / 2); t448: waves along the channels (1 / 2 / 4); upconv ws: abSplit
  int poolPass = 0;    // the pooled copy came from maxpool2x2_planes_kernel, not from the epilogue
  void set(int st, int tw, int e, bool fl, int ks, int wv, bool pp) {
    structure = st, tileW = tw, epi = e, flat = fl ? 1 : 0, kSplit = ks, waves = wv, poolPass = pp ? 1 : 0;
  }
};

// The forced form of the test entry points' tile_width argument, decoded here and nowhere else (what each ABI integer
// stands for: DESIGN.md, section 4.15, "The forced form")
struct X3Force {
  int family = 0;   // 0 = none, else X3Path::structure
  int tileW = 0;
  int waves = 0;    // 0 = the form's own choice
};
bool x3_decode_force(int code, X3Force* out) {
  static const struct {
    int code;
    X3Force f;
  } kForms[] = {{0, {0, 0, 0}},         {16, {kX3Ws, 16, 0}},     {32, {kX3Ws, 32, 0}},     {28, {kX3R512, 28, 0}},
                {14, {kX3R512, 14, 0}}, {228, {kX3R512, 28, 2}},  {214, {kX3R512, 14, 2}},  {332, {kX3R512, 32, 1}},
                {316, {kX3R512, 16, 1}}, {308, {kX3R512, 8, 1}},  {532, {kX3R512, 32, 2}},  {428, {kX3Q8, 28, 1}},
                {414, {kX3Q8, 14, 1}},  {628, {kX3T448, 28, 0}},  {632, {kX3T448, 32, 0}},  {728, {kX3T448, 28, 4}}};
  for (const auto& k : kForms)
    if (k.code == code) {
      if (out) *out = k.f;
      return true;
    }
  return false;
}

// Pixel-tile width of the first structure for an H x W map: the shape that wastes fewer MFMAs on padding
bool x3_flat_rows(int n, int h, int tw, bool flatOn) { return flatOn && n > 1 && h % (256 / tw) != 0; }
int x3_tile_width(int h, int w, int n, bool flatOn) {
  auto eff = [&](int tw) {
    const int th = 256 / tw;
    const double rows = x3_flat_rows(n, h, tw, flatOn) ? (double)n * h / round_up(n * h, th) : (double)h / round_up(h, th);
    return rows * w / (double)round_up(w, tw);
  };
  return eff(16) > eff(32) + 1e-9 ? 16 : 32;
}
int x3_r512_tile_width(int w) {   // 0: no tile width of the second structure divides this map
  if (w % 28 == 0) return 28;
  if (w == 14) return 14;
  if (w % 32 == 0) return 32;
  if (w % 16 == 0) return 16;
  if (w % 8 == 0) return 8;
  return 0;
}
inline int x3_grid(long items) { return (int)std::max<long>(8, std::min<long>(256, items / 8 * 8)); }

struct X3ConvQuery {
  int n = 0, h = 0, w = 0, cin = 0, cout = 0;
  int epi = 0;                // the epilogue asked for: 0 planes, 1 planes + pooled copy, 2 fused head, 3 fp32
  X3Force force;
  int coOff = 0;
  bool splitScratch = false;  // split-K scratch handed over, splitFloats floats of it
  size_t splitFloats = 0;
  bool qScratch = false;      // f16q8: room for the input's q plane / the operator has its packed fp8 fragments
  bool wq = false;
  // f16q8, how the tensors pass between two convolutions of the tier (X3Q8Link)
  bool inIsQ = false, wantOutQ = false, poolSrcQ = false, poolDstQ = false;
  bool wantStats = false;     // fp32 epilogue: the caller takes fused BatchNorm partial sums if the structure has them
  X3Switches sw;
};
struct X3ConvPlan {
  bool valid = false;         // false: a forced form that does not fit the shape, or a q-plane input off the q8 form
  X3Path path;
  int N = 0, H = 0, imgH = 0, tilesX = 0, tilesY = 0, pixTiles = 0, coTiles = 0, coGroup = 0, nChunks = 0, kSplit = 1;
  int grid = 0;
  int statRows = 0;           // > 0: the epilogue writes that many rows of BatchNorm partial sums
  bool toQ8Pass = false;      // planes_to_q8_kernel runs first
  int poolPass = 0;           // 1: maxpool2x2_planes_kernel follows, 2: maxpool2x2_planes_q8_kernel
  bool finishPass = false;    // x3_splitk_finish_kernel follows
  bool outQ = false;          // the output's q plane is written in its lo plane's place
  void tiles(int n, int h, int w, int tw, int th, bool flat) {
    N = flat ? 1 : n;
    H = flat ? n * h : h;
    imgH = h;
    tilesX = (w + tw - 1) / tw;
    tilesY = (H + th - 1) / th;
    pixTiles = N * tilesY * tilesX;
  }
};

// Precedence: third structure, f16q8 form, second structure, split-K on the first structure, the first structure.  A
// forced form never falls through to the first structure.
X3ConvPlan x3_plan_conv(const X3ConvQuery& q) {
  X3ConvPlan p;
  const int n = q.n, h = q.h, w = q.w, cin = q.cin, cout = q.cout, epi = q.epi;
  const X3Force& f = q.force;
  const bool unforced = f.family == 0;
  const bool stats = q.wantStats && epi == 3;
  p.nChunks = cin / 32;
  // ---- third structure (conv_x3_t448.h): forced (16-row tiles, 64 or 128 channels per block; 8-row tiles, 256 channels
  //      per block), or by itself: the 64- / 128-channel form for the layers whose Cout is no multiple of 256 (the 224 x 224
  //      and 112 x 112 levels), the 256-channel form for the others on maps of width 28k (56 x 56, 28 x 28; heights that
  //      are no multiple of 8 as one tall image), wherever its tiles are filled to >= 90 % and there is a work item for at
  //      least half of the CUs.  Plane, pooled and fp32 epilogues; the fused head with Cout = 64. ----
  {
    const bool forcedT = f.family == kX3T448;
    const bool forcedC4 = forcedT && f.waves == 4;
    const int twt = forcedT ? f.tileW : (w % 28 == 0 ? 28 : (w % 32 == 0 ? 32 : 0));
    const bool c4 = forcedC4 || (!forcedT && cout % 256 == 0);
    // waves along the channels: 4 (256 per block, 8-row tiles), 2 (128 per block where the 16 x 28 tile's 14 fragments
    // per wave fit the registers), 1 (64 per block)
    const int wco = c4 ? 4 : (twt == 28 && cout % 128 == 0 && epi != 2) ? 2 : 1;
    const int tht = c4 ? 8 : 16;
    const bool shapeT = twt != 0 && w % twt == 0 && cin % 32 == 0 && cout % (64 * wco) == 0 && (epi != 2 || cout == 64) &&
                        (epi != 1 || (h % 2 == 0 && w % 2 == 0)) && !(c4 && (twt != 28 || epi == 2));
    const bool flatT = c4 && n > 1 && h % tht != 0 && 2 * h >= tht;
    const int tilesYT = flatT ? (n * h + tht - 1) / tht : (h + tht - 1) / tht;
    const long itemsT = shapeT ? (long)(flatT ? 1 : n) * tilesYT * (w / twt) * (cout / (64 * wco)) : 0;
    const bool fillT = flatT || 10 * h >= 9 * tht * tilesYT;
    // (the 256-channel form steps aside for the f16q8 tier's own form)
    const bool autoT = unforced && (c4 ? q.sw.t448c4 && q.sw.r512 : q.sw.t448) && itemsT >= 128 && fillT && !q.inIsQ &&
                       !(c4 && q.sw.crossFp8 == 1 && q.qScratch);
    if (shapeT && (forcedT || autoT)) {
      const int coTiles = cout / (64 * wco);
      int grid = x3_grid(itemsT);
      if (stats)   // a block must keep ONE channel group for its per-channel sums: the grid a multiple of the groups' count
        while (grid > 0 && grid % coTiles) grid -= 8;
      if (grid > 0) {
        p.tiles(n, h, w, twt, tht, flatT);
        p.coTiles = p.coGroup = coTiles;
        p.grid = grid;
        p.statRows = stats ? grid * (4 / wco) : 0;
        p.path.set(kX3T448, twt, epi, flatT, 1, wco, false);
        p.valid = true;
        return p;
      }
    }
    if (forcedT) return p;
  }
  // ---- second structure and the f16q8 form on its tiles: forced, or by itself for every layer it supports once there
  //      is a work item for at least half of the CUs ----
  {
    // tile width by the map's width: 28 (224, 112, 56, 28), 14, else 32 / 16 / 8 (the 640 x 640 configuration's 160-, 80-
    // and 40-wide levels; 256-channel form only)
    const bool forced = f.family == kX3R512;
    const bool forcedW2 = forced && f.waves == 2;
    const int twxRaw = forced ? f.tileW : x3_r512_tile_width(w);
    const int twx = twxRaw ? twxRaw : 28;             // (no width fits: shapeOk below is false)
    const bool narrowOnly = twx != 28 && twx != 14 && twx != 32;   // widths without the two-wave form
    const bool narrow = twx != 28 && twx != 14;
    const int thx = 224 / twx;
    const bool flatR = n > 1 && h % thx != 0 && 2 * h >= thx;
    const long tiles = flatR ? (long)((n * h + thx - 1) / thx) * (w / twx) : (long)n * ((h + thx - 1) / thx) * (w / twx);
    // 256-channel block tiles (one wave per 64 channels) where Cout allows, unless the 128-channel form fills the
    // chip's 256 CUs so much more evenly that it wins although its loop is ~7 % slower (the 14 x 14 layers at batch 256:
    // 896 items = 3.5 per CU against 1792 = 7 per CU)
    auto balance = [](long items) { return (double)items / (double)((items + 255) / 256 * 256); };
    int wpx = 2;
    if (cout % 256 == 0 && !forcedW2) {
      const long i1 = tiles * (cout / 256), i2 = tiles * (cout / 128);
      wpx = (forced || narrow || balance(i1) >= 0.93 * balance(i2)) ? 1 : 2;
    }
    const long items = tiles * (cout / (256 / wpx));
    // a pooled layer of the two-wave form stays on the first structure's fused epilogue (measured at 112 x 112, batch
    // 256: 2.15 ms fused against 2.04 + 0.42 ms with the separate pooling pass; at Cout >= 256 the second structure wins
    // with the pass included: 1.95 against 2.12 ms, 1.72 against 2.13 ms)
    const bool autoOk = unforced && q.sw.r512 && items >= 128 && !(epi == 1 && wpx == 2);
    const bool shapeOk = twxRaw != 0 && w % twx == 0 && (twx != 14 || w == 14) && cin % 32 == 0 &&
                         cout % (narrowOnly ? 256 : 128) == 0 && !(narrowOnly && wpx != 1);
    const bool q8Forced = f.family == kX3Q8;
    const int tq = q8Forced ? f.tileW : twx;
    const bool q8Shape = q.qScratch && q.wq && epi != 3 && epi != 2 && cin % 64 == 0 && cout % 256 == 0 &&
                         (tq == 28 ? w % 28 == 0 : w == 14);
    // by itself: the tier on, and the layer one the second structure would run as 224 x 256 tiles (not where the balance
    // rule picked the 128-channel form - the 14 x 14 layers at batch 256: with them the tier's logit error against the
    // f16x3 tier reaches 1.0e-3 over 256 frames, without them 9.2e-4 (7.8e-4 against the reference's golden logits): the
    // margin is kept)
    const bool q8Auto = q.sw.crossFp8 == 1 && shapeOk && autoOk && wpx == 1 && !narrow;
    if (q.inIsQ && !(q8Shape && q8Auto)) return p;   // the input has no lo plane
    if (q8Shape && (q8Forced || q8Auto)) {
      const int thq = 224 / tq;
      const bool flatQ = n > 1 && h % thq != 0 && 2 * h >= thq;
      p.tiles(n, h, w, tq, thq, flatQ);
      p.coTiles = p.coGroup = cout / 256;
      p.grid = x3_grid((long)p.pixTiles * p.coTiles);
      p.toQ8Pass = !q.inIsQ;
      p.outQ = q.wantOutQ && epi == 0 && q.coOff % 32 == 0;
      if (epi == 1) p.poolPass = ((q.poolSrcQ || q.poolDstQ) && q.coOff % 32 == 0) ? 2 : 1;
      p.path.set(kX3Q8, tq, p.outQ ? 4 : 0, flatQ, 1, 1, epi == 1);
      p.valid = true;
      return p;
    }
    if (q8Forced) return p;
    if (epi != 2 && shapeOk && (forced || autoOk)) {
      p.tiles(n, h, w, twx, thx, flatR);
      p.coTiles = p.coGroup = cout / (256 / wpx);
      p.grid = x3_grid(items);
      p.statRows = stats ? p.grid * wpx : 0;
      p.poolPass = epi == 1 ? 1 : 0;   // (this structure has no fused pooling epilogue)
      p.path.set(kX3R512, twx, epi == 3 ? 3 : 0, flatR, 1, wpx, epi == 1);
      p.valid = true;
      return p;
    }
    if (forced) return p;
  }
  // ---- first structure (conv_x3_ws.h); the fused-head epilogue (224 x 224 only) has no FLAT instance ----
  const int tw = f.family == kX3Ws ? f.tileW : x3_tile_width(h, w, n, q.sw.flat);
  const bool flat = x3_flat_rows(n, h, tw, q.sw.flat) && epi != 2;
  p.tiles(n, h, w, tw, 256 / tw, flat);
  p.coTiles = cout / 64;
  p.coGroup = 1;
  for (int g : {8, 4, 2})
    if (p.coTiles % g == 0) {
      p.coGroup = g;
      break;
    }
  // Split-K: with fewer work items than half of the CUs (single frames: a 14x14 map is one pixel tile), the input
  // channels are divided over kSplit items per tile; the items write raw fp32 partial sums (EPI 3, unit scale) and
  // x3_splitk_finish_kernel adds them, applies scale / shift / ReLU and writes the planes (+ the pooled copy).
  const long items = (long)p.pixTiles * p.coTiles;
  int kSplit = 1;
  if (q.splitScratch && epi != 3 && epi != 2 && cout <= 1024) {
    const int chunks = cin / 32;
    while (items * kSplit * 2 <= 256 && (chunks / (kSplit * 2)) >= 2 && (chunks % (kSplit * 4)) == 0 &&
           (size_t)(kSplit * 2) * (size_t)n * h * w * cout <= q.splitFloats)
      kSplit *= 2;
    if (items > 128) kSplit = 1;
  }
  p.kSplit = kSplit;
  p.nChunks = cin / 32 / kSplit;   // even: chunks are consumed in pairs
  p.grid = x3_grid(items * kSplit);
  p.finishPass = kSplit > 1;
  p.poolPass = kSplit > 1 && epi == 1 ? 1 : 0;
  p.path.set(kX3Ws, tw, kSplit > 1 ? 0 : epi, flat, kSplit, 0, p.poolPass != 0);
  p.valid = true;
  return p;
}

// The profiler label of a plan's main kernel: one per template instance, so that bench.py's per-kernel figures line up
// with rocprofv3's kernel names (bench.py:rocprof_name parses it)
void x3_conv_label(const X3ConvPlan& p, char* buf, size_t cap) {
  const X3Path& k = p.path;
  const char* fl = k.flat ? "_flat" : "";
  switch (k.structure) {
    case kX3T448: snprintf(buf, cap, "conv3x3_t448_f16x3_t%d_c%d_e%d%s", k.tileW, k.waves, k.epi, fl); break;
    case kX3Q8: snprintf(buf, cap, "conv3x3_q8_f16q8_t%d%s%s", k.tileW, p.outQ ? "_q" : "", fl); break;
    case kX3R512: snprintf(buf, cap, "conv3x3_r512_f16x3_t%d_w%d_e%d%s", k.tileW, k.waves, k.epi, fl); break;
    case kX3Ws:
      if (k.kSplit > 1)
        snprintf(buf, cap, "conv3x3_ws_f16x3_splitk");
      else
        snprintf(buf, cap, "conv3x3_ws_f16x3_tw%d_e%d%s", k.tileW, k.epi, fl);
      break;
    default: snprintf(buf, cap, "%s", ""); break;
  }
}

// One launch of the plan's instance, through the structure's launch unit (launch.h)
hipError_t launch_conv_plan(const X3ConvPlan& p, const unet::ConvQ8Args& a, hipStream_t s) {
  const X3Path& k = p.path;
  const int grid = p.grid, tw = k.tileW;
  const bool flat = k.flat != 0;
  switch (k.structure) {
    case kX3T448: return unet::launch_conv_t448(a, grid, tw, k.waves, k.epi, flat, s);
    case kX3Q8: return unet::launch_conv_q8(a, grid, tw, k.epi, flat, s);
    case kX3R512: return unet::launch_conv_r512(a, grid, tw, k.waves, flat, k.epi == 3, s);
    case kX3Ws: {
      const int epi = k.kSplit > 1 ? 3 : k.epi;   // split-K items write raw fp32 partial sums
      return unet::launch_conv_x3(a, grid, tw, epi, flat, s);
    }
    default: return hipErrorInvalidValue;
  }
}

// f16q8 tier: how a tensor passes between two convolutions of the tier.  inIsQ: the input's lo-plane region already holds
// its q plane (the producer wrote it: no conversion pass); wantOutQ: write the output's q plane instead of its lo plane
// (asked for only when the one consumer is known to run on conv_q8_r512.h); wroteQ: the launch did so
struct X3Q8Link {
  bool inIsQ = false, wantOutQ = false, wroteQ = false;
  // a pooled layer of the tier (its pooling pass is maxpool2x2_planes_q8_kernel): poolSrcQ - the pass also writes the q
  // plane of the layer's own output over its lo plane (the skip half of a concat buffer whose other consumer, the
  // decoder's first convolution, is of this tier and whose upper half gets its q plane from the transposed
  // convolution); poolDstQ - the pooled tensor gets its q plane instead of its lo plane; pooledQ: it did
  bool poolSrcQ = false, poolDstQ = false, pooledQ = false, srcQDone = false;
};

// The tensors of one convolution: planes (n,h,w,op.cin) in -> planes out with pixel stride ldo at channel offset coOff
// (out may be null where the epilogue writes no planes: fused head, fp32 output)
struct X3ConvIo {
  const uint16_t* zeros = nullptr;   // >= 64 zero halfs
  const uint16_t* in = nullptr;      // hi plane; the lo plane inLo halfs behind it
  size_t inLo = 0;
  int n = 0, h = 0, w = 0;
  uint16_t* out = nullptr;
  size_t outLo = 0;
  int ldo = 0, coOff = 0;
  X3ConvIo to(uint16_t* o, size_t oLo, int ld, int off = 0) const {
    X3ConvIo r = *this;
    r.out = o, r.outLo = oLo, r.ldo = ld, r.coOff = off;
    return r;
  }
};
inline X3ConvIo x3_from(const uint16_t* zeros, const uint16_t* in, size_t inLo, int n, int h, int w) {
  X3ConvIo io;
  io.zeros = zeros, io.in = in, io.inLo = inLo, io.n = n, io.h = h, io.w = w;
  return io;
}
struct X3ConvOpts {
  const X3Fuse* fuse = nullptr;       // exactly one of its fusions (pool or head) may be requested
  int forceTw = 0;                    // the test entry points' tile_width (x3_decode_force)
  float* outF = nullptr;              // fp32 output (training) at pixel stride ldo, channel offset coOff
  const float* dynScale = nullptr;
  const char* label = nullptr;        // profiler label instead of the plan's own
  const X3SplitK* splitK = nullptr;
  // training forward, fp32 output: where the structure that runs fuses the BatchNorm statistics' per-block sums
  // (ConvX3Args::statPartial) *statRows is their row count; otherwise 0 and the caller runs its own statistics pass
  float* statPartial = nullptr;
  int* statRows = nullptr;
  uint8_t* qScratch = nullptr;        // f16q8 tier: room for the input's q plane (n * h * w * cin * 2 bytes)
  X3Q8Link* q8Link = nullptr;
  X3Path* path = nullptr;             // what ran (test entry points)
};

X3ConvQuery x3_conv_query(const GemmOpX3& op, const X3ConvIo& io, const X3ConvOpts& o) {
  X3ConvQuery q;
  q.n = io.n, q.h = io.h, q.w = io.w, q.cin = op.cin, q.cout = op.cout;
  q.epi = o.outF ? 3 : (o.fuse && o.fuse->pool) ? 1 : (o.fuse && o.fuse->headW) ? 2 : 0;
  q.coOff = io.coOff;
  q.splitScratch = o.splitK && o.splitK->scratch;
  q.splitFloats = o.splitK ? o.splitK->floats : 0;
  q.qScratch = o.qScratch != nullptr;
  q.wq = op.wq != nullptr;
  if (o.q8Link) q.inIsQ = o.q8Link->inIsQ, q.wantOutQ = o.q8Link->wantOutQ, q.poolSrcQ = o.q8Link->poolSrcQ, q.poolDstQ = o.q8Link->poolDstQ;
  q.wantStats = o.outF && o.statPartial && o.statRows;
  q.sw = x3_switches();
  return q;
}

// One 3x3 convolution of the tier: plan, fill the kernel's arguments from the plan, launch (+ the passes the plan names)
hipError_t run_conv_x3(const GemmOpX3& op, const X3ConvIo& io, const X3ConvOpts& o, hipStream_t s) {
  if (o.statRows) *o.statRows = 0;
  X3ConvQuery q = x3_conv_query(op, io, o);
  if (!x3_decode_force(o.forceTw, &q.force)) return hipErrorInvalidValue;
  const X3ConvPlan p = x3_plan_conv(q);
  if (!p.valid) return hipErrorInvalidValue;
  const X3Path& k = p.path;
  const int n = io.n, h = io.h, w = io.w;
  const size_t P = (size_t)n * h * w;
  const bool split = p.kSplit > 1;
  unet::ConvQ8Args a{};   // (pool, head, statistics: null unless the plan's epilogue takes them)
  a.in = io.in, a.inLo = io.inLo, a.zeros = io.zeros;
  a.wt = op.wt, a.wq = op.wq;
  a.out = io.out, a.outLo = io.outLo;
  a.N = p.N, a.H = p.H, a.W = w, a.imgH = p.imgH, a.Cin = op.cin, a.Cout = op.cout;
  a.tilesX = p.tilesX, a.tilesY = p.tilesY, a.pixTiles = p.pixTiles;
  a.coTiles = p.coTiles, a.coGroup = p.coGroup, a.nChunks = p.nChunks;
  a.kSplit = p.kSplit, a.chunksTotal = op.cin / 32;
  a.dynScale = o.dynScale;
  a.err = g_errWord ? g_errWord : op_err_word();
  if (split) {   // raw fp32 partial sums into the scratch, unscaled: the finish pass applies scale / shift / ReLU
    a.scale = o.splitK->ones, a.shift = o.splitK->zerosF, a.relu = 0;
    a.outF = o.splitK->scratch, a.ldo = op.cout, a.co_off = 0, a.splitStride = P * op.cout;
  } else {
    a.scale = op.scale, a.shift = op.shift, a.relu = op.relu;
    a.outF = o.outF, a.ldo = io.ldo, a.co_off = io.coOff;
  }
  if (k.epi == 1) a.pool = o.fuse->pool, a.poolLo = o.fuse->poolLo;
  if (k.epi == 2) {
    const X3Fuse& z = *o.fuse;
    a.headW = z.headW, a.headB = z.headB, a.headThr = z.headThr, a.logits = z.logits, a.probs = z.probs, a.mask = z.mask;
  }
  if (p.toQ8Pass) {
    // the q plane of the input: fp8(x_hi / 8) and fp8(256 x_lo) per 32 channels, from the two fp16 planes
    prof_begin("planes_to_q8", 0.0, 6.0 * (double)P * op.cin, s);
    hipLaunchKernelGGL(unet::planes_to_q8_kernel, dim3(grid_for(P * (op.cin / 16))), dim3(256), 0, s, io.in, io.inLo, P, op.cin,
                       op.cin, o.qScratch);
    prof_end(s);
    a.inLo = (size_t)(reinterpret_cast<const uint16_t*>(o.qScratch) - io.in);   // halfs; the kernel adds it in bytes
  }
  if (p.statRows) {
    const hipError_t em = hipMemsetAsync(o.statPartial, 0, (size_t)p.statRows * 2 * op.cout * sizeof(float), s);
    if (em != hipSuccess) return em;
    a.statPartial = o.statPartial;
    *o.statRows = p.statRows;
  }
  // algorithmic (direct-convolution) flops; the kernels execute 3x that many fp16 MFMA flops.  The label is only spelt
  // out while a profiler listens: the unprofiled launch path does no string work
  char autoLabel[48];
  const char* label = o.label ? o.label : "";
  if (!o.label && g_prof && g_prof->on) {
    x3_conv_label(p, autoLabel, sizeof(autoLabel));
    label = autoLabel;
  }
  const double px = (double)P;
  const double outShare = split ? (double)p.kSplit : k.structure != kX3T448 ? 1.0 : k.epi == 2 ? 0.0 : k.epi == 1 ? 1.25 : 1.0;
  prof_begin(label, 2.0 * px * 9 * op.cin * op.cout, 4.0 * (px * op.cin + outShare * px * op.cout + 9.0 * op.cin * op.cout), s);
  const hipError_t e = launch_conv_plan(p, a, s);
  prof_end(s);
  if (e != hipSuccess) return e;
  auto pool_pass = [&]() {   // the pooled copy a fused epilogue would have written (of the channels at coOff)
    hipLaunchKernelGGL(unet::maxpool2x2_planes_kernel, dim3(grid_for(P / 4 * (op.cout / 2))), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(io.out + io.coOff), io.outLo / 2, n, h, w, op.cout, io.ldo,
                       reinterpret_cast<uint32_t*>(o.fuse->pool), o.fuse->poolLo / 2);
  };
  if (p.finishPass) {
    prof_begin("splitk_finish_f16x3", 0.0, 4.0 * (double)(p.kSplit + 1) * P * op.cout, s);
    hipLaunchKernelGGL(unet::x3_splitk_finish_kernel, dim3(grid_for(P * (op.cout / 4))), dim3(256), 0, s,
                       (const float*)o.splitK->scratch, p.kSplit, P, op.cout, (const float*)op.scale, (const float*)op.shift,
                       op.relu, reinterpret_cast<uint32_t*>(io.out), io.outLo / 2, io.ldo, io.coOff, a.err);
    if (p.poolPass) pool_pass();
    prof_end(s);
  } else if (p.poolPass == 2) {
    X3Q8Link& lk = *o.q8Link;
    prof_begin("maxpool2x2_planes_q8", 0.0, (double)P * op.cout * (4.0 + (lk.poolSrcQ ? 2.0 : 0.0) + 1.0), s);
    hipLaunchKernelGGL(unet::maxpool2x2_planes_q8_kernel, dim3(grid_for(P / 4 * (op.cout / 32))), dim3(256), 0, s,
                       io.out + io.coOff, io.outLo, n, h, w, op.cout, io.ldo, o.fuse->pool, o.fuse->poolLo, lk.poolSrcQ ? 1 : 0,
                       lk.poolDstQ ? 1 : 0);
    prof_end(s);
    lk.pooledQ = lk.poolDstQ;
    lk.srcQDone = lk.poolSrcQ;
  } else if (p.poolPass == 1) {
    prof_begin("maxpool2x2_planes_f16x3", 0.0, 4.0 * (double)P * op.cout * 1.25, s);
    pool_pass();
    prof_end(s);
  }
  if (o.q8Link && k.structure == kX3Q8) o.q8Link->wroteQ = p.outQ;
  if (o.path) *o.path = k;
  return hipGetLastError();
}

// ---- the transposed convolution and the plain GEMM on its kernels ----

// which launches the one-wave-per-SIMD structure (upconv_x3_r512.h) takes (unet_set_x3_upconv_r512): -1 = automatic
// (shapes it supports with a work item for at least half of the CUs; UNET_X3_UPCONV_R512=0 in the environment: never),
// 0 = never, 1 = whenever the shape allows
std::atomic<int> g_x3UpconvR512{-1};

int x3_upconv_r512_mode() {
  static const bool envOff = x3_env_off("UNET_X3_UPCONV_R512");
  const int m = g_x3UpconvR512;
  return m < 0 ? (envOff ? 0 : -1) : m;
}

struct X3UpconvQuery {
  long npix = 0;          // input pixels
  int w = 0;              // map width (ConvTranspose2d; a plain GEMM passes gemm = true instead)
  int cin = 0, cout = 0;  // GEMM: K and the column count
  bool gemm = false;      // MODE 1: a channel tile is 256 columns
  int coOff = 0;
  bool wantOutQ = false;  // f16q8: the output's q plane in its lo plane's place (second structure only)
  int mode = -1;          // x3_upconv_r512_mode()
};
struct X3UpconvPlan {
  bool valid = false;     // false: a q plane was asked of a launch the second structure does not take
  X3Path path;
  int coTiles = 0, pixTiles = 0, abSplit = 1, grid = 0;
  bool outQ = false;
};
X3UpconvPlan x3_plan_upconv(const X3UpconvQuery& q) {
  X3UpconvPlan p;
  p.coTiles = q.gemm ? (q.cout + 255) / 256 : q.cout / 64;
  const int tilesW = (int)((q.npix + unet::UpconvX3Shape::TP - 1) / unet::UpconvX3Shape::TP);
  const int tilesR = (int)((q.npix + unet::UpconvX3RShape::TP - 1) / unet::UpconvX3RShape::TP);
  const int abSplit = !q.gemm && (long)tilesW * p.coTiles <= 64 ? 4 : 1;   // small batches: one item per (a,b)
  const long workR = (long)tilesR * p.coTiles;
  const bool r512 = !(q.mode == 0 || q.cin % 128 != 0 || (!q.gemm && q.w < 4) || (q.mode < 0 && (workR < 128 || abSplit != 1)));
  if (q.wantOutQ && !(r512 && q.coOff % 32 == 0 && !q.gemm)) return p;   // the consumer has been told
  p.valid = true;
  p.outQ = q.wantOutQ;
  p.pixTiles = r512 ? tilesR : tilesW;
  p.abSplit = r512 ? 1 : abSplit;
  p.grid = x3_grid(r512 ? workR : (long)tilesW * p.coTiles * abSplit);
  p.path.set(r512 ? kX3R512 : kX3Ws, 0, 0, false, 1, p.abSplit, false);
  return p;
}
const char* x3_upconv_label(const X3UpconvPlan& p) {
  return p.path.structure == kX3Ws ? "upconv2x2_ws_f16x3" : p.outQ ? "upconv2x2_r512_f16x3_q" : "upconv2x2_r512_f16x3";
}

// One launch on the plan's kernel; MODE 0: ConvTranspose2d, MODE 1: the plain GEMM.  The fill both share: `a` arrives with
// what differs between the two (scale / bias / out / h / w / err, or outF / dynScale)
template <int MODE>
hipError_t launch_upconv_plan(const X3UpconvPlan& p, unet::UpconvX3Args a, const uint16_t* wt, const X3ConvIo& io, long npix,
                              int cin, int cout, const char* label, hipStream_t s) {
  a.in = io.in, a.inLo = io.inLo, a.zeros = io.zeros, a.wt = wt;
  a.npix = npix, a.Cin = cin, a.Cout = cout, a.ldo = io.ldo, a.co_off = io.coOff;
  a.nChunks = cin / 32, a.coTiles = p.coTiles, a.pixTiles = p.pixTiles, a.abSplit = p.abSplit;
  const double px = (double)npix, cols = MODE == 0 ? 4.0 * cout : (double)cout;
  const bool r512 = p.path.structure == kX3R512;
  prof_begin(label, 2.0 * px * cin * cols, 4.0 * (px * cin + px * cols), s);
  const hipError_t e = unet::launch_upconv_x3(a, p.grid, r512, MODE, p.outQ, s);
  prof_end(s);
  return e;
}

// in: planes (n,h,w,op.cin) -> out planes (n,2h,2w) with pixel stride ldo at channel offset coOff.
// q8Link (f16q8 tier): wantOutQ - write the output's q plane in its lo plane's place (an error where the second structure
// does not take the launch, because the consumer has been told)
X3UpconvQuery x3_upconv_query(const GemmOpX3& op, const X3ConvIo& io, bool wantOutQ) {
  X3UpconvQuery q;
  q.npix = (long)io.n * io.h * io.w, q.w = io.w, q.cin = op.cin, q.cout = op.cout, q.coOff = io.coOff;
  q.wantOutQ = wantOutQ;
  q.mode = x3_upconv_r512_mode();
  return q;
}
hipError_t run_upconv_x3(const GemmOpX3& op, const X3ConvIo& io, hipStream_t s, X3Q8Link* q8Link = nullptr, X3Path* path = nullptr) {
  const X3UpconvQuery q = x3_upconv_query(op, io, q8Link && q8Link->wantOutQ);
  const X3UpconvPlan p = x3_plan_upconv(q);
  if (!p.valid) return hipErrorInvalidValue;
  unet::UpconvX3Args a{};
  a.scale = op.scale, a.bias = op.shift, a.out = io.out, a.outLo = io.outLo, a.h = io.h, a.w = io.w;
  a.err = g_errWord ? g_errWord : op_err_word();
  const hipError_t e = launch_upconv_plan<0>(p, a, op.wt, io, q.npix, op.cin, op.cout, x3_upconv_label(p), s);
  if (q8Link && p.outQ) q8Link->wroteQ = e == hipSuccess;
  if (path) *path = p.path;
  return e;
}

// Plain GEMM on planes through the same kernels (MODE 1): outF[p][coOff + n] = dyn * sum_k in[p][k] W[k][n], n < nCols, for
// the npix = io.n * io.h * io.w pixels of `io` (only its input side, ldo and coOff are read); wt packed by
// pack_upconv_dgrad_x3_kernel; K % 64 == 0, nCols % 64 == 0.  structure (test entry point): as X3Path::structure
hipError_t run_gemm1x1_x3(const uint16_t* wt, const X3ConvIo& io, int K, int nCols, float* outF, const float* dynScale,
                          const char* label, hipStream_t s, int* structure = nullptr) {
  X3UpconvQuery q;
  q.npix = (long)io.n * io.h * io.w, q.cin = K, q.cout = nCols, q.coOff = io.coOff;
  q.gemm = true;
  q.mode = x3_upconv_r512_mode();
  const X3UpconvPlan p = x3_plan_upconv(q);
  unet::UpconvX3Args a{};
  a.outF = outF, a.dynScale = dynScale, a.h = a.w = 1;
  if (structure) *structure = p.path.structure;
  return launch_upconv_plan<1>(p, a, wt, io, q.npix, K, nCols, label, s);
}

// ---- the decoder's composed first convolution (conv_x3_dec.h) ----

// ConvTranspose2d(2f -> f, k2, s2, bias bt) followed by the up half W3[:, f:2f] of a 3x3 convolution (pad 1), composed in
// float64 (DESIGN.md, "The decoder's composed first convolution"): for the output pixel (2i + a, 2j + b), high-resolution
// tap ky reads the transposed convolution's output row 2i + a + ky - 1 = 2 (i + floor((a + ky - 1) / 2)) + ((a + ky - 1) & 1):
// low-resolution row i + a - 1 + di with di = floor((a + ky - 1) / 2) - (a - 1) in {0, 1}, kernel row (a + ky - 1) & 1.
//   wp [parity a * 2 + b][co][ci (2f)][di * 2 + dj], bias [class][co] with class = row class * 3 + column class (0 first
//   row / column of the image, 1 interior, 2 last): the sum over the taps whose high-resolution pixel lies inside the
//   image (a high-resolution row is inside iff its low-resolution row is: H = 2h)
void compose_upcat(const float* wt, const float* bt, const float* w3, int f, std::vector<double>& wp, std::vector<double>& bias) {
  const int c2 = 2 * f;
  wp.assign((size_t)4 * f * c2 * 4, 0.0);
  bias.assign((size_t)9 * f, 0.0);
  std::vector<double> w3u((size_t)f * f), wtp((size_t)c2 * f), m((size_t)f * c2);
  auto fl2 = [](int v) { return v >= 0 ? v / 2 : -((1 - v) / 2); };   // floor(v / 2)
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      for (int co = 0; co < f; ++co)
        for (int c = 0; c < f; ++c) w3u[(size_t)co * f + c] = w3[(((size_t)co * c2 + f + c) * 3 + ky) * 3 + kx];
      for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) {
          const int py = (a + ky - 1) & 1, px = (b + kx - 1) & 1;
          const int di = fl2(a + ky - 1) - (a - 1), dj = fl2(b + kx - 1) - (b - 1);
          // wtp [c][ci]: the sum over c runs as f updates of a row of 2f sums (contiguous, independent: the compiler
          // vectorises it), each sum adding its terms in the order c = 0, 1, ... of the plain dot product - the same bits
          for (int ci = 0; ci < c2; ++ci)
            for (int c = 0; c < f; ++c) wtp[(size_t)c * c2 + ci] = wt[(((size_t)ci * f + c) * 2 + py) * 2 + px];
          auto rows = [&](int co0, int co1) {
            std::vector<double> acc(c2);
            for (int co = co0; co < co1; ++co) {
              const double* wr = &w3u[(size_t)co * f];
              double* out = &wp[((size_t)(a * 2 + b) * f + co) * c2 * 4];
              std::fill(acc.begin(), acc.end(), 0.0);
              for (int c = 0; c < f; ++c) {
                const double s = wr[c];
                const double* tr = &wtp[(size_t)c * c2];
                for (int ci = 0; ci < c2; ++ci) acc[ci] += s * tr[ci];
              }
              for (int ci = 0; ci < c2; ++ci) out[(size_t)ci * 4 + di * 2 + dj] += acc[ci];
            }
          };
          // output channels over a few host threads where the level is wide (f = 512: 10 G multiply-adds in all)
          const int nThr = f >= 256 ? 8 : 1;
          std::vector<std::thread> pool;
          for (int t = 1; t < nThr; ++t) pool.emplace_back(rows, f * t / nThr, f * (t + 1) / nThr);
          rows(0, f / nThr);
          for (auto& th : pool) th.join();
        }
      // the bias through this tap, into every class whose pixels see the tap inside the image
      for (int co = 0; co < f; ++co) {
        double v = 0.0;
        for (int c = 0; c < f; ++c) v += w3u[(size_t)co * f + c] * (double)bt[c];
        for (int rc = 0; rc < 3; ++rc)
          for (int cc = 0; cc < 3; ++cc)
            if (!(rc == 0 && ky == 0) && !(rc == 2 && ky == 2) && !(cc == 0 && kx == 0) && !(cc == 2 && kx == 2))
              bias[(size_t)(rc * 3 + cc) * f + co] += v;
      }
    }
}

// What every form of one decoder step is built from, on the host: wt (2f,f,2,2), bt (f), w3 (f,2f,3,3) with the BatchNorm
// scale / shift folded -> compose_upcat's result and both halves of the weights with their inputs' activation scales
// (skipAct (f), xAct (2f); null: none) divided out (exact: powers of two), as float
struct DecHostX3 {
  int f = 0;
  std::vector<double> wp, bias;   // compose_upcat
  std::vector<float> ws;          // the skip half W3[:, :f] / skipAct, (f,f,3,3)
  std::vector<float> wx;          // wp / xAct, [parity][co][ci (2f)][tap]
  std::vector<float> maxS, maxX;  // max |ws|, max |wx| per output channel: what the pre-scales come from
};
void dec_host_x3(DecHostX3& hst, const float* wt, const float* bt, const float* w3, int f, const float* skipAct, const float* xAct) {
  const int c2 = 2 * f;
  hst.f = f;
  compose_upcat(wt, bt, w3, f, hst.wp, hst.bias);
  hst.ws.resize((size_t)f * f * 9);
  hst.wx.resize(hst.wp.size());
  hst.maxS.assign(f, 0.f);
  hst.maxX.assign(f, 0.f);
  for (int co = 0; co < f; ++co)
    for (int ci = 0; ci < f; ++ci)
      for (int t = 0; t < 9; ++t) {
        const float v = w3[((size_t)co * c2 + ci) * 9 + t] / (skipAct ? skipAct[ci] : 1.f);
        hst.ws[((size_t)co * f + ci) * 9 + t] = v;
        hst.maxS[co] = std::max(hst.maxS[co], std::fabs(v));
      }
  for (int p = 0; p < 4; ++p)
    for (int co = 0; co < f; ++co)
      for (int ci = 0; ci < c2; ++ci)
        for (int t = 0; t < 4; ++t) {
          const size_t i = (((size_t)p * f + co) * c2 + ci) * 4 + t;
          hst.wx[i] = (float)hst.wp[i] / (xAct ? xAct[ci] : 1.f);
          hst.maxX[co] = std::max(hst.maxX[co], std::fabs(hst.wx[i]));
        }
}

// composed form (conv_x3_dec.h): per 64-channel tile the f / 32 skip chunks [tap 9][plane][cs][lane][8], then the 2f / 32
// x chunks [parity 4][tap 4][plane][cs][lane][8]; one pre-scale per output channel over both halves (one accumulator)
std::vector<uint16_t> pack_upcat_x3(const float* ws, const float* wx, int f, const std::vector<float>& pre) {
  const int c2 = 2 * f, nS = f / 32, nX = c2 / 32, nCt = f / 64;
  const size_t tap = 2 * 4 * kX3Frag, skipChunk = 9 * tap, xChunk = 16 * tap, perCt = nS * skipChunk + nX * xChunk;
  std::vector<uint16_t> packed(nCt * perCt, 0);
  auto put = [&](size_t base, int ct, int kc, auto&& val) {   // one tap: [plane][cs][lane][8]
    for (int cs = 0; cs < 4; ++cs)
      x3_put_frag(packed.data() + base + cs * kX3Frag, packed.data() + base + (4 + cs) * kX3Frag, ct, kc, cs,
                  [&](int co, int ci) { return val(co, ci) * pre[co]; });
  };
  for (int ct = 0; ct < nCt; ++ct) {
    for (int kc = 0; kc < nS; ++kc)
      for (int t = 0; t < 9; ++t)
        put(ct * perCt + kc * skipChunk + t * tap, ct, kc, [&](int co, int ci) { return ws[((size_t)co * f + ci) * 9 + t]; });
    for (int kc = 0; kc < nX; ++kc)
      for (int p = 0; p < 4; ++p)
        for (int t = 0; t < 4; ++t)
          put(ct * perCt + nS * skipChunk + kc * xChunk + (p * 4 + t) * tap, ct, kc,
              [&](int co, int ci) { return wx[(((size_t)p * f + co) * c2 + ci) * 4 + t]; });
  }
  return packed;
}

// unet_set_x3_compose: -1 = automatic (default; UNET_X3_COMPOSE=0 in the environment makes it 0), 0 = the two-kernel
// path everywhere, 1 = the composed operator wherever its shape rules allow (also below the work-item threshold)
int& x3_compose_mode() {
  static int mode = x3_env_off("UNET_X3_COMPOSE") ? 0 : -1;
  return mode;
}

// unet_set_x3_dec_form: which block tile the composed decoder step runs on.  -1 = automatic, 1 = the 64-channel form
// (upcat_conv3x3_dec_f16x3_kernel<1>) everywhere, 2 = the 128-channel form (<2>) wherever f % 128 == 0.  Both forms add
// each accumulator's terms in the same order from the same packed weights: bit-identical results.  UNET_X3_DEC_FORM=1 / 2
// in the environment sets the initial value
int& x3_dec_form_mode() {
  static int mode = [] {
    const char* e = getenv("UNET_X3_DEC_FORM");
    return (e && (e[0] == '1' || e[0] == '2') && !e[1]) ? e[0] - '0' : -1;
  }();
  return mode;
}

// ---- the deep decoder levels' split first convolution (upconv_x3_win.h + the addend epilogue of conv_x3_t448.h) ----
// The same algebra as the composed operator above, as two launches: kernel 1 forms P = the up half (2 x 2-tap window
// convolution of x per output parity + the border-class constant) into the up half of the concat buffer, where the
// transposed convolution writes on the two-kernel path; kernel 2 runs the 3x3 convolution over the skip half only and
// adds P in its epilogue.  In real units y = relu((accS / preS + P) scale + shift) out; P is stored as P aP with aP a
// power of two from the magnitude estimate of x (1 where there is none), so sP = scale out / aP.

// unet_set_x3_compose_deep: 1 = on (default; UNET_X3_COMPOSE_DEEP=0 in the environment makes it 0), 0 = the deep levels
// keep the two-kernel path.  unet_set_x3_compose(0) turns both composed paths off
int& x3_compose_deep_mode() {
  static int mode = x3_env_off("UNET_X3_COMPOSE_DEEP") ? 0 : 1;
  return mode;
}

// window weights: [coTile(64)][chunk(32)][tap(4) = di * 2 + dj][plane(2)][ab(4)][cs(4)][lane(64)][8], packed hi / lo with
// the per-channel pre-scale `pre`; `ordered` (optional: the CPU test reads it): the window weights in float64 in the
// pack's order (plane 0's positions)
std::vector<uint16_t> pack_updeep_x3(const DecHostX3& hst, std::vector<float>& pre, std::vector<double>* ordered) {
  const int f = hst.f, c2 = 2 * f, nCt = f / 64, nCh = c2 / 32;
  pre.resize(f);
  for (int co = 0; co < f; ++co) pre[co] = prescale_pow2(hst.maxX[co]);
  std::vector<uint16_t> packed((size_t)nCt * nCh * 4 * 2 * 4 * 4 * kX3Frag, 0);
  if (ordered) ordered->assign(packed.size(), 0.0);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < nCh; ++kc)
      for (int tap = 0; tap < 4; ++tap)
        for (int ab = 0; ab < 4; ++ab)
          for (int cs = 0; cs < 4; ++cs) {
            const size_t hi = ((((((size_t)ct * nCh + kc) * 4 + tap) * 2 + 0) * 4 + ab) * 4 + cs) * kX3Frag, lo = hi + 16 * kX3Frag;
            auto src = [&](int co, int ci) { return (((size_t)ab * f + co) * c2 + ci) * 4 + tap; };
            x3_put_frag(&packed[hi], &packed[lo], ct, kc, cs, [&](int co, int ci) { return hst.wx[src(co, ci)] * pre[co]; });
            if (ordered) x3_each_frag_elem(ct, kc, cs, [&](int i, int co, int ci) { (*ordered)[hi + i] = hst.wp[src(co, ci)]; });
          }
  return packed;
}

// ---- one decoder step: ConvTranspose2d(2f -> f) -> cat([skip, up]) -> Conv3x3(2f -> f) -> Conv3x3(f -> f) ----
// Its operators in every form the step can run in (x3_plan_dec_step chooses per launch): the two-kernel form's up +
// conv1, the composed and the deep operator where the width has them (x3_dec_step_forms), and the second convolution
enum { kX3DecTwoKernel = 0, kX3DecComposed = 1, kX3DecDeep = 2 };   // X3DecStepPlan::form; as bits 1 / 2: a set of operators
struct DecStepX3 {
  int f = 0, relu = 0;
  GemmOpX3 up, conv1, conv2;
  struct Composed {   // UpcatX3Args::wt, scale, shift, dshift
    uint16_t* wt = nullptr;
    float *scale = nullptr, *shift = nullptr, *dshift = nullptr;
  } comp;
  struct Deep {   // kernel 1: the window weights, scale aP / pre, the nine class constants x aP; kernel 2: W3[:, :f] packed
    uint16_t *wtWin = nullptr, *wtSkip = nullptr;   // as every 3x3 weight, s, t, sP
    float *scaleWin = nullptr, *cls = nullptr, *scale = nullptr, *shift = nullptr, *addScale = nullptr;
  } deep;
  void free_forms() {
    for (void* p : {(void*)comp.wt, (void*)comp.scale, (void*)comp.shift, (void*)comp.dshift, (void*)deep.wtWin, (void*)deep.wtSkip,
                    (void*)deep.scaleWin, (void*)deep.cls, (void*)deep.scale, (void*)deep.shift, (void*)deep.addScale})
      if (p) hipFree(p);
    comp = Composed(), deep = Deep();
  }
  void free_dev() { up.free_dev(), conv1.free_dev(), conv2.free_dev(), free_forms(); }
};
// Which of the two operators a step of width f can have.  The forward's handle: composed up to 128 channels (the 8-row,
// 256-channel tiles of the wider levels are not built), deep where kernel 2's 256-channel form tiles f.  An operator entry
// point: composed up to 256 channels (several channel groups per pixel tile), deep at any width x3_plan_updeep takes
inline int x3_dec_step_forms(int f, bool entry) {
  return (f % 64 == 0 && f <= (entry ? 256 : 128) ? kX3DecComposed : 0) | (entry || f % 256 == 0 ? kX3DecDeep : 0);
}

// The operators `forms` of one step (st.comp, st.deep) from one composition: wt (2f,f,2,2), bt (f), w3 (f,2f,3,3) with
// BatchNorm scale / shift folded; skipIn / xIn / out: activation scales of the skip, of x (the transposed convolution's
// input) and of the output (null: none)
int build_dec_step_x3(std::string& err, DecStepX3& st, int forms, const float* wt, const float* bt, const float* w3, int f,
                      const float* scale, const float* shift, int relu, const ActScale* skipIn, const ActScale* xIn,
                      const ActScale* out) {
  st.free_forms();
  st.f = f, st.relu = relu;
  if (!forms) return UNET_OK;
  const int c2 = 2 * f;
  DecHostX3 hst;
  dec_host_x3(hst, wt, bt, w3, f, skipIn ? skipIn->act.data() : nullptr, xIn ? xIn->act.data() : nullptr);
  int rc = UNET_OK;
  if (forms & kX3DecComposed) {
    DecStepX3::Composed& op = st.comp;
    std::vector<float> pre(f), sc(f), sh(f), dsh((size_t)9 * f);
    for (int co = 0; co < f; ++co) {
      pre[co] = prescale_pow2(std::max(hst.maxS[co], hst.maxX[co]));
      const float o = out ? out->act[co] : 1.f;
      sc[co] = scale[co] / pre[co] * o;
      double cls[9];
      for (int k = 0; k < 9; ++k) cls[k] = ((double)shift[co] + (double)scale[co] * hst.bias[(size_t)k * f + co]) * o;
      sh[co] = (float)cls[4];
      for (int k = 0; k < 9; ++k) dsh[(size_t)k * f + co] = k == 4 ? 0.f : (float)(cls[k] - (double)sh[co]);
    }
    rc = upload_bf(err, &op.wt, pack_upcat_x3(hst.ws.data(), hst.wx.data(), f, pre));
    if (!rc) rc = upload(err, &op.scale, sc);
    if (!rc) rc = upload(err, &op.shift, sh);
    if (!rc) rc = upload(err, &op.dshift, dsh);
  }
  if (!rc && (forms & kX3DecDeep)) {
    DecStepX3::Deep& op = st.deep;
    std::vector<float> preW;
    const std::vector<uint16_t> win = pack_updeep_x3(hst, preW, nullptr);
    auto cls0 = [&](int k, int co) { return (float)hst.bias[(size_t)k * f + co]; };   // the class constants, unscaled
    // P's scale: four standard deviations of the window sum (independent channels, as build_upconv_x3 estimates its
    // output) plus the interior constant, where x carries magnitudes
    std::vector<float> aP(f, 1.f);
    if (xIn && std::any_of(xIn->mag.begin(), xIn->mag.end(), [](float m) { return m > 0.f; })) {
      for (int co = 0; co < f; ++co) {
        double var = 0;
        for (int ci = 0; ci < c2; ++ci) {
          const double sd = xIn->mag[ci] / 4.0;
          for (int t = 0; t < 4; ++t) {
            double m = 0;
            for (int p = 0; p < 4; ++p) m = std::max(m, std::fabs(hst.wp[(((size_t)p * f + co) * c2 + ci) * 4 + t]));
            var += m * m * sd * sd;
          }
        }
        aP[co] = act_scale_pow2((float)(4.0 * std::sqrt(var)) + std::fabs(cls0(4, co)));
      }
    }
    std::vector<float> scW(f), cls((size_t)9 * f), preS(f), sc(f), sh(f), sp(f);
    for (int co = 0; co < f; ++co) {
      scW[co] = aP[co] / preW[co];
      for (int k = 0; k < 9; ++k) cls[(size_t)k * f + co] = cls0(k, co) * aP[co];
      preS[co] = prescale_pow2(hst.maxS[co]);   // the skip half runs as a 3x3 convolution of its own
      const float o = out ? out->act[co] : 1.f;
      sc[co] = scale[co] / preS[co] * o;
      sh[co] = shift[co] * o;
      sp[co] = scale[co] * o / aP[co];
    }
    rc = upload_bf(err, &op.wtWin, win);
    if (!rc) rc = upload(err, &op.scaleWin, scW);
    if (!rc) rc = upload(err, &op.cls, cls);
    if (!rc) rc = upload_bf(err, &op.wtSkip, pack_conv_x3(hst.ws.data(), f, f, preS));
    if (!rc) rc = upload(err, &op.scale, sc);
    if (!rc) rc = upload(err, &op.shift, sh);
    if (!rc) rc = upload(err, &op.addScale, sp);
  }
  return rc;
}

// ---- which form a decoder step runs in (DESIGN.md, section 4.15): a pure function of integers, like the other plans ----
// Asked in this order: the composed operator, the deep levels' split form, else the two kernels (whose own dispatch is
// x3_plan_upconv / x3_plan_conv).  h, w: the LOW-resolution map of x, here and in X3DecIo; H = 2h, W = 2w below
struct X3DecStepQuery {
  int n = 0, h = 0, w = 0, f = 0;
  int compose = -1;         // x3_compose_mode(): 0 two kernels everywhere, -1 automatic, 1 wherever the shapes allow
  bool deep = true;         // x3_compose_deep_mode()
  int decForm = -1;         // x3_dec_form_mode()
  bool q8 = false;          // the forward holds f16q8 scratch
  bool entry = false;       // who asks: the forward, or an operator entry point (which forces its operator: compose = 1)
  int have = kX3DecComposed | kX3DecDeep;   // the operators the asker holds, of those x3_dec_step_forms gives its width
  bool windowOnly = false;  // (entry point) the deep form's kernel 1 alone: f % 64 == 0 is enough
  int upconvMode = -1;      // x3_upconv_r512_mode(): only the two-kernel form's labels depend on it
  X3Switches sw;
};
// The deep form's own plan (its two launches); it reads n, h, w, f, compose, deep, q8, windowOnly and the switches
struct X3UpdeepPlan {
  bool take = false;
  int wmax = 0, pixTiles = 0, coTiles = 0, grid = 0;   // kernel 1
  X3ConvPlan conv;                                     // kernel 2: the third structure's 256-channel form
};
X3UpdeepPlan x3_plan_updeep(const X3DecStepQuery& q) {
  X3UpdeepPlan p;
  const long npix = (long)q.n * q.h * q.w;
  if (q.compose == 0 || !q.deep || q.q8 || q.n < 1 || q.h < 1 || q.w < 4 || q.w > 28 || q.f < 64 || q.f % 64 ||
      npix >= (1L << 31) - 224 - 64)
    return p;
  p.wmax = q.w <= 14 ? 14 : 28;
  p.pixTiles = (int)((npix + unet::UpconvX3RShape::TP - 1) / unet::UpconvX3RShape::TP);
  p.coTiles = q.f / 64;
  const long items = (long)p.pixTiles * p.coTiles;
  p.grid = x3_grid(items);
  if (!q.windowOnly) {
    if (q.f % 256) return p;
    X3ConvQuery c;
    c.n = q.n, c.h = 2 * q.h, c.w = 2 * q.w, c.cin = q.f, c.cout = q.f, c.epi = 0;
    c.sw = q.sw;
    if (q.compose == 1) x3_decode_force(728, &c.force);
    p.conv = x3_plan_conv(c);
    // automatic: the work-item rule of the composed path for both launches - the third structure takes the layer by
    // itself (>= 128 items, tiles filled) and kernel 1 has an item for half of the CUs
    if (!p.conv.valid || p.conv.path.structure != kX3T448 || p.conv.path.waves != 4) return p;
    if (q.compose < 0 && items < 128) return p;
  }
  p.take = true;
  return p;
}

struct X3DecStepPlan {
  int form = kX3DecTwoKernel;
  int wco = 0, tilesX = 0, tilesY = 0, pixTiles = 0, coTiles = 0, grid = 0;   // composed: upcat_conv3x3_dec_f16x3_kernel<wco>
  X3UpdeepPlan deep;        // deep
  int nLaunch = 0;          // composed / deep: the launches run_dec_step_x3 makes and their profiler labels
  const char* label[2] = {nullptr, nullptr};
};
X3DecStepPlan x3_plan_dec_step(const X3DecStepQuery& q) {
  X3DecStepPlan p;
  const int have = q.have & x3_dec_step_forms(q.f, q.entry);
  if (q.compose == 0) return p;
  const int H = 2 * q.h, W = 2 * q.w;   // (H is even as the composed kernel needs it)
  if ((have & kX3DecComposed) && (q.entry || !q.q8) && W % 28 == 0 && H >= 2) {
    // 128 output channels per block where the channels allow (the 112 x 112 level of model A): both halos staged once per
    // pixel tile instead of twice, every skip weight fragment serves 14 pixel fragments instead of 7
    p.wco = (q.decForm != 1 && q.f % 128 == 0) ? 2 : 1;
    p.tilesX = W / 28, p.tilesY = (H + 15) / 16;
    p.coTiles = q.f / (64 * p.wco), p.pixTiles = q.n * p.tilesY * p.tilesX;
    const long items = (long)p.pixTiles * p.coTiles;
    // unless forced: a work item for half of the CUs and 16-row tiles filled to >= 90 %
    if (q.entry || q.compose == 1 || !(items < 128 || 10 * H < 9 * 16 * p.tilesY)) {
      p.form = kX3DecComposed, p.grid = x3_grid(items);
      p.nLaunch = 1, p.label[0] = "upcat_conv3x3_dec_f16x3";
      return p;
    }
  }
  if (have & kX3DecDeep) {
    p.deep = x3_plan_updeep(q);
    if (p.deep.take) {
      p.form = kX3DecDeep, p.nLaunch = q.windowOnly ? 1 : 2;
      p.label[0] = "upconv2x2_win_f16x3";
      p.label[1] = p.deep.conv.path.flat ? "conv3x3_t448add_f16x3_t28_c4_flat" : "conv3x3_t448add_f16x3_t28_c4";
    }
  }
  return p;
}
// the query as the library's switches stand
X3DecStepQuery x3_dec_step_query(int n, int h, int w, int f, bool q8, bool entry, int have = kX3DecComposed | kX3DecDeep) {
  X3DecStepQuery q;
  q.n = n, q.h = h, q.w = w, q.f = f, q.q8 = q8, q.entry = entry, q.have = have;
  q.compose = entry ? 1 : x3_compose_mode(), q.deep = x3_compose_deep_mode() != 0, q.decForm = x3_dec_form_mode();
  q.upconvMode = x3_upconv_r512_mode(), q.sw = x3_switches();
  return q;
}
// The profiler labels of the step's launches up to its second convolution, comma-separated.  Two-kernel form: of the
// launches as the forward makes them while no q plane is handed on (X3Q8Link), its split-K scratch included
void x3_dec_step_labels(const X3DecStepQuery& q, const X3DecStepPlan& p, char* buf, size_t cap) {
  std::string out;
  auto add = [&](const char* lb) { out += (out.empty() ? "" : ",") + std::string(lb); };
  for (int i = 0; i < p.nLaunch; ++i) add(p.label[i]);
  if (p.form == kX3DecTwoKernel) {
    X3UpconvQuery u;
    u.npix = (long)q.n * q.h * q.w, u.w = q.w, u.cin = 2 * q.f, u.cout = q.f, u.coOff = q.f, u.mode = q.upconvMode;
    add(x3_upconv_label(x3_plan_upconv(u)));
    X3ConvQuery c;
    c.n = q.n, c.h = 2 * q.h, c.w = 2 * q.w, c.cin = 2 * q.f, c.cout = q.f;
    c.splitScratch = true, c.splitFloats = kSplitFloats, c.sw = q.sw;
    c.qScratch = q.q8, c.wq = q.q8 && x3_conv_has_q8(c.cin, c.cout);
    const X3ConvPlan cp = x3_plan_conv(c);
    char lb[48];
    x3_conv_label(cp, lb, sizeof(lb));
    if (cp.toQ8Pass) add("planes_to_q8");
    add(lb);
    if (cp.finishPass) add("splitk_finish_f16x3");
  }
  snprintf(buf, cap, "%s", out.c_str());
}

// The tensors of one decoder step.  xo: x planes (n,h,w,2f) in -> out planes (n,2h,2w,f) at pixel stride ldo (xo.coOff
// unused; n, h, w as in the query: the low-resolution map).  cat: planes (n,2h,2w) at pixel stride ldCat whose channels
// [0,f) hold the skip; the deep form writes P into its channels [upOff, upOff + f) (composed: only the skip is read)
struct X3DecIo {
  X3ConvIo xo;
  uint16_t* cat = nullptr;
  size_t catLo = 0;
  int ldCat = 0, upOff = 0;
};

// Runs a composed or deep plan (a two-kernel plan is the caller's: run_upconv_x3 + run_conv_x3).  A deep plan of one launch
// (windowOnly) writes P alone and leaves `out` alone
hipError_t run_dec_step_x3(const DecStepX3& st, const X3DecStepPlan& p, const X3DecIo& io, hipStream_t s) {
  const X3ConvIo& xo = io.xo;
  const int n = xo.n, h = xo.h, w = xo.w, f = st.f;
  const double pxLo = (double)n * h * w, px = 4.0 * pxLo;
  if (p.form == kX3DecComposed && st.comp.wt) {
    const DecStepX3::Composed& op = st.comp;
    unet::UpcatX3Args a;
    a.skip = io.cat, a.skipLo = io.catLo, a.ldSkip = io.ldCat;
    a.x = xo.in, a.xLo = xo.inLo;
    a.wt = op.wt, a.zeros = xo.zeros, a.scale = op.scale, a.shift = op.shift, a.dshift = op.dshift, a.relu = st.relu;
    a.out = xo.out, a.outLo = xo.outLo, a.ldo = xo.ldo;
    a.N = n, a.H = 2 * h, a.W = 2 * w, a.F = f;
    a.tilesX = p.tilesX, a.tilesY = p.tilesY, a.pixTiles = p.pixTiles, a.coTiles = p.coTiles;
    a.nS = f / 32, a.nX = 2 * f / 32;
    a.err = g_errWord ? g_errWord : op_err_word();
    // executed multiply-adds: 9 f^2 (skip) + 8 f^2 (x: 4 taps x 2f) per pixel
    prof_begin(p.label[0], 2.0 * px * 17.0 * f * f, 4.0 * (px * f + px / 4 * 2 * f + px * f) + 2.0 * (9.0 * f * f + 32.0 * f * f), s);
    const hipError_t e = unet::launch_upcat_dec(a, p.grid, p.wco, s);
    prof_end(s);
    return e;
  }
  if (p.form != kX3DecDeep || !st.deep.wtWin) return hipErrorInvalidValue;
  const DecStepX3::Deep& op = st.deep;
  {
    unet::UpconvX3Args a{};
    a.in = xo.in, a.inLo = xo.inLo, a.zeros = xo.zeros, a.wt = op.wtWin;
    a.scale = op.scaleWin, a.bias = op.cls;
    a.out = io.cat, a.outLo = io.catLo;
    a.npix = (long)n * h * w, a.h = h, a.w = w, a.Cin = 2 * f, a.Cout = f, a.ldo = io.ldCat, a.co_off = io.upOff;
    a.nChunks = 2 * f / 32, a.coTiles = p.deep.coTiles, a.pixTiles = p.deep.pixTiles, a.abSplit = 1;
    a.err = g_errWord ? g_errWord : op_err_word();
    // executed multiply-adds: 4 taps x 2f per output pixel and channel; x read, P written, the window weights
    prof_begin(p.label[0], 2.0 * px * 8.0 * f * f, 4.0 * (pxLo * 2 * f + px * f) + 2.0 * 32.0 * f * f, s);
    const hipError_t e = unet::launch_upconv_win(a, p.deep.grid, p.deep.wmax == 14, s);
    prof_end(s);
    if (e != hipSuccess || p.nLaunch == 1) return e;
  }
  const X3ConvPlan& c = p.deep.conv;
  unet::ConvX3AddArgs a{};
  a.in = io.cat, a.inLo = io.catLo, a.zeros = xo.zeros, a.wt = op.wtSkip;
  a.scale = op.scale, a.shift = op.shift, a.relu = st.relu;
  a.out = xo.out, a.outLo = xo.outLo, a.ldo = xo.ldo, a.co_off = 0;
  a.N = c.N, a.H = c.H, a.W = 2 * w, a.imgH = c.imgH, a.Cin = f, a.Cout = f;
  a.tilesX = c.tilesX, a.tilesY = c.tilesY, a.pixTiles = c.pixTiles;
  a.coTiles = c.coTiles, a.coGroup = c.coGroup, a.nChunks = c.nChunks, a.kSplit = 1, a.chunksTotal = f / 32;
  a.err = g_errWord ? g_errWord : op_err_word();
  a.ldi = io.ldCat, a.ldAdd = io.ldCat, a.add = io.cat + io.upOff, a.addLo = io.catLo, a.addScale = op.addScale;
  // the skip half's 3x3 convolution; the skip and P read, the output written
  prof_begin(p.label[1], 2.0 * px * 9.0 * f * f, 4.0 * (px * f + px * f + px * f) + 2.0 * 9.0 * f * f, s);
  const hipError_t e = unet::launch_conv_t448add(a, c.grid, c.path.flat != 0, s);
  prof_end(s);
  return e;
}

// First convolution on conv_first_x3.h: uint8 (N,H,W,3) frames (u8) or an fp32 NCHW image -> planes (N,H,W,op.cout) with
// pixel stride ldo; op from build_conv_x3(first = true).  mean / stdv: the input normalisation, null = none
hipError_t run_first_x3(const GemmOpX3& op, const void* input, bool u8, int n, int h, int w, uint16_t* out, size_t outLo,
                        int ldo, const float* mean, const float* stdv, hipStream_t s) {
  unet::ConvFirstX3Args fa;
  fa.frames = input;
  fa.wt = op.wt;
  fa.scale = op.scale;
  fa.shift = op.shift;
  fa.out = out;
  fa.outLo = outLo;
  fa.N = n;
  fa.H = h;
  fa.W = w;
  fa.Cout = op.cout;
  fa.ldo = ldo;
  fa.tilesX = (w + 31) / 32;
  fa.tilesY = (h + 7) / 8;
  fa.relu = op.relu;
  fa.m0 = mean ? mean[0] : 0.f;
  fa.m1 = mean ? mean[1] : 0.f;
  fa.m2 = mean ? mean[2] : 0.f;
  fa.s0 = stdv ? stdv[0] : 1.f;
  fa.s1 = stdv ? stdv[1] : 1.f;
  fa.s2 = stdv ? stdv[2] : 1.f;
  fa.err = g_errWord;
  const double px = (double)n * h * w;
  prof_begin("conv3x3_first_f16x3", 2.0 * px * 27 * op.cout, px * (u8 ? 3 : 12) + 4.0 * px * op.cout, s);
  const dim3 grid((unsigned)(fa.tilesX * fa.tilesY * n));
  if (u8)
    hipLaunchKernelGGL(unet::conv_first_x3_kernel<true>, grid, dim3(256), 0, s, fa);
  else
    hipLaunchKernelGGL(unet::conv_first_x3_kernel<false>, grid, dim3(256), 0, s, fa);
  prof_end(s);
  return hipGetLastError();
}

// ---- the first encoder block as one kernel (conv_x3_enc1.h; DESIGN.md 4.12) ----
// unet_set_x3_fuse_first: 1 = on (default; UNET_X3_FUSE_FIRST=0 in the environment makes it 0), 0 = the block keeps its
// two launches (conv_first_x3.h, then conv_x3_t448.h)
int& x3_fuse_first_mode() {
  static int mode = x3_env_off("UNET_X3_FUSE_FIRST") ? 0 : 1;
  return mode;
}

// The fused kernel stands for exactly one pair of launches: uint8 frames into a 64-channel first convolution, and a
// second convolution that x3_plan_conv itself puts on the third structure's 64-channel form with the pooled epilogue on
// 16 x 28 tiles.  Everything else keeps the two launches: fp32 input, batches whose second convolution lands on another
// structure, widths tiled 32 wide, the training forward, the f16q8 tier (its scratch present).
// conv2: the second convolution's query, as run_conv_x3 would ask it
struct X3Enc1Plan {
  bool take = false;
  X3ConvPlan conv;   // the second convolution's plan: tiles and grid of the fused launch
};
X3Enc1Plan x3_plan_enc1(bool u8, bool on, const X3ConvQuery& conv2) {
  X3Enc1Plan p;
  if (!on || !u8 || conv2.cin != 64 || conv2.cout != 64 || conv2.qScratch || conv2.w % 28 != 0) return p;
  const X3ConvPlan c = x3_plan_conv(conv2);
  const X3Path& k = c.path;
  if (!c.valid || k.structure != kX3T448 || k.waves != 1 || k.epi != 1 || k.tileW != 28 || k.kSplit != 1 || k.flat) return p;
  p.take = true;
  p.conv = c;
  return p;
}

// op1 from build_conv_x3(first = true), op2 the block's second convolution; frames (n,h,w,3) uint8 -> io.out planes
// (pixel stride io.ldo, channel offset io.coOff) and their pooled copy fuse.pool; io's input side is not read
hipError_t run_enc1_x3(const X3Enc1Plan& p, const GemmOpX3& op1, const GemmOpX3& op2, const void* frames, const X3ConvIo& io,
                       const X3Fuse& fuse, const float* mean, const float* stdv, hipStream_t s, X3Path* path = nullptr) {
  if (!p.take || op1.cout != 64 || op2.cin != 64 || op2.cout != 64 || !fuse.pool) return hipErrorInvalidValue;
  const X3ConvPlan& c = p.conv;
  unet::ConvEnc1X3Args a{};
  a.c.wt = op2.wt, a.c.scale = op2.scale, a.c.shift = op2.shift, a.c.relu = op2.relu;
  a.c.out = io.out, a.c.outLo = io.outLo, a.c.ldo = io.ldo, a.c.co_off = io.coOff;
  a.c.N = c.N, a.c.H = c.H, a.c.W = io.w, a.c.imgH = c.imgH, a.c.Cin = 64, a.c.Cout = 64;
  a.c.tilesX = c.tilesX, a.c.tilesY = c.tilesY, a.c.pixTiles = c.pixTiles;
  a.c.coTiles = a.c.coGroup = 1, a.c.nChunks = 2, a.c.kSplit = 1, a.c.chunksTotal = 2;
  a.c.pool = fuse.pool, a.c.poolLo = fuse.poolLo;
  a.c.err = g_errWord ? g_errWord : op_err_word();
  a.frames = static_cast<const uint8_t*>(frames);
  a.wt1 = op1.wt, a.scale1 = op1.scale, a.shift1 = op1.shift, a.relu1 = op1.relu;
  a.m0 = mean ? mean[0] : 0.f, a.m1 = mean ? mean[1] : 0.f, a.m2 = mean ? mean[2] : 0.f;
  a.s0 = stdv ? stdv[0] : 1.f, a.s1 = stdv ? stdv[1] : 1.f, a.s2 = stdv ? stdv[2] : 1.f;
  // the algorithmic flops of both convolutions (the halo's recomputed pixels are not counted); the frames read, the
  // planes and their pooled copy written
  const double px = (double)io.n * io.h * io.w;
  prof_begin("conv3x3_enc1_f16x3", 2.0 * px * (27.0 * 64 + 9.0 * 64 * 64), 3.0 * px + 4.0 * px * 64 + px * 64, s);
  const hipError_t e = unet::launch_conv_enc1(a, c.grid, s);
  prof_end(s);
  if (path) *path = c.path;
  return e;
}

}  // namespace

struct X3Net {
  float* ones = nullptr;         // 1024 x 1.0f (unit scale of the split-K pass)
  float* splitScratch = nullptr; // split-K partial sums (kSplitFloats floats)
  uint16_t* zeros = nullptr;
  float* headW = nullptr;        // head weights with the last activation's scale divided out
  std::vector<GemmOpX3> enc, bott;
  std::vector<DecStepX3> dec;    // per decoder step j: its operators in every form it can run in
  GrowBuf ws;
  bool hasQ8 = false;            // the operators carry their fp8 cross-term fragments (f16q8 tier)
  GrowBuf qbuf;                  // q plane of the layer input being consumed (f16q8 tier)
};

static void x3_free(unet_ctx* h) {
  if (!h->x3) return;
  for (auto* v : {&h->x3->enc, &h->x3->bott})
    for (auto& op : *v) op.free_dev();
  for (auto& st : h->x3->dec) st.free_dev();
  h->x3->ws.release();
  h->x3->qbuf.release();
  if (h->x3->zeros) hipFree(h->x3->zeros);
  if (h->x3->ones) hipFree(h->x3->ones);
  if (h->x3->splitScratch) hipFree(h->x3->splitScratch);
  if (h->x3->headW) hipFree(h->x3->headW);
  delete h->x3;
  h->x3 = nullptr;
}

namespace {

int x3_build(unet_ctx* h) {
  const unet_config& c = h->cfg;
  if (c.in_channels != 3) {
    h->err = "the f16x3 tier needs in_channels == 3";
    return UNET_ERR_INVALID_ARG;
  }
  for (int l = 0; l < c.depth; ++l)
    if (c.features[l] % 64) {
      h->err = "the f16x3 tier needs every feature width to be a multiple of 64";
      return UNET_ERR_INVALID_ARG;
    }
  if (2 * c.features[c.depth - 1] > unet::X3Shape<32>::MAX_COUT) {
    h->err = "the f16x3 tier supports at most 1024 channels";
    return UNET_ERR_INVALID_ARG;
  }
  x3_free(h);
  h->x3 = new X3Net();
  X3Net* X = h->x3;
  HIPCHK(h->err, hipMalloc((void**)&X->zeros, 4096));
  HIPCHK(h->err, hipMemset(X->zeros, 0, 4096));
  {
    std::vector<float> one(1024, 1.f);
    HIPCHK(h->err, hipMalloc((void**)&X->ones, 4096));
    HIPCHK(h->err, hipMemcpy(X->ones, one.data(), 4096, hipMemcpyHostToDevice));
    // split-K is only chosen for layers of <= 128 work items (256 pixels x 64 channels each) and <= 256 items after the
    // split: partial sums of at most 256 x 256 x 64 floats
    HIPCHK(h->err, hipMalloc((void**)&X->splitScratch, kSplitFloats * sizeof(float)));
  }
  auto& P = h->params;
  const bool withQ8 = g_x3CrossFp8 == 1;   // pack the fp8 cross-term fragments too (58 MB for model A)
  X->hasQ8 = withQ8;
  // UNET_X3_ACT_SCALE=0: planes hold the activations themselves (A/B against the per-channel scales)
  const bool useAct = !x3_env_off("UNET_X3_ACT_SCALE");
  auto conv = [&](GemmOpX3& o, const std::string& prefix, int convIdx, int bnIdx, int cin, int cout, bool first,
                  const ActScale* in, ActScale* out) -> int {
    const auto& w = P[prefix + "." + std::to_string(convIdx) + ".weight"];
    const std::string bn = prefix + "." + std::to_string(bnIdx) + ".";
    std::vector<float> sc, sh;
    fold_bn(P, bn, cout, sc, sh);
    *out = act_from_bn(P[bn + "weight"].data(), P[bn + "bias"].data(), cout);
    return build_conv_x3(h->err, o, w.data(), cout, cin, sc.data(), sh.data(), 1, first, useAct ? in : nullptr,
                         useAct ? out : nullptr, withQ8);
  };
  X->enc.assign(2 * c.depth, GemmOpX3());
  X->dec.assign(c.depth, DecStepX3());
  X->bott.assign(2, GemmOpX3());
  int rc;
  int cin = 3;
  std::vector<ActScale> skip(c.depth);   // scales of the encoder outputs (the skip halves; pooling keeps them)
  ActScale cur, tmp;
  for (int l = 0; l < c.depth; ++l) {
    const std::string p = "encoder_blocks." + std::to_string(l);
    if ((rc = conv(X->enc[2 * l], p, 0, 1, cin, c.features[l], l == 0, l == 0 ? nullptr : &cur, &tmp))) return rc;
    if ((rc = conv(X->enc[2 * l + 1], p, 3, 4, c.features[l], c.features[l], false, &tmp, &skip[l]))) return rc;
    cur = skip[l];
    cin = c.features[l];
  }
  const int fl = c.features[c.depth - 1];
  if ((rc = conv(X->bott[0], "bottleneck", 0, 1, fl, 2 * fl, false, &cur, &tmp))) return rc;
  if ((rc = conv(X->bott[1], "bottleneck", 3, 4, 2 * fl, 2 * fl, false, &tmp, &cur))) return rc;
  for (int j = 0; j < c.depth; ++j) {
    const int l = c.depth - 1 - j;
    const int f = c.features[l];
    const std::string pu = "decoder_blocks." + std::to_string(2 * j);
    ActScale upOut;
    if ((rc = build_upconv_x3(h->err, X->dec[j].up, P[pu + ".weight"].data(), 2 * f, f, P[pu + ".bias"].data(),
                              useAct ? &cur : nullptr, useAct ? &upOut : nullptr)))
      return rc;
    if (!useAct) {
      upOut.act.assign(f, 1.f);
      upOut.mag.assign(f, 1.f);
    }
    const ActScale cat = act_concat(skip[l], upOut);   // torch.cat([skip, x]) (reference README.md:1478)
    const std::string pd = "decoder_blocks." + std::to_string(2 * j + 1);
    if ((rc = conv(X->dec[j].conv1, pd, 0, 1, 2 * f, f, false, &cat, &tmp))) return rc;
    {
      // the same step composed (conv_x3_dec.h) and split over two launches (upconv_x3_win.h, conv_x3_t448.h's addend
      // epilogue), where the width has them: x = the transposed convolution's input, scale `cur`
      std::vector<float> sc, sh;
      fold_bn(P, pd + ".1.", f, sc, sh);
      if ((rc = build_dec_step_x3(h->err, X->dec[j], x3_dec_step_forms(f, false), P[pu + ".weight"].data(), P[pu + ".bias"].data(),
                                  P[pd + ".0.weight"].data(), f, sc.data(), sh.data(), 1, useAct ? &skip[l] : nullptr,
                                  useAct ? &cur : nullptr, useAct ? &tmp : nullptr)))
        return rc;
    }
    if ((rc = conv(X->dec[j].conv2, pd, 3, 4, f, f, false, &tmp, &cur))) return rc;
  }
  {   // the 1x1 head reads the last activation: its scale goes into the head's weights
    const int f0 = c.features[0];
    const auto& hw = P["output.weight"];   // (out_channels, f0): every row by the same scales
    std::vector<float> hs(hw.size());
    for (size_t i = 0; i < hs.size(); ++i) hs[i] = hw[i] / (useAct ? cur.act[i % f0] : 1.f);
    if ((rc = upload(h->err, &X->headW, hs))) return rc;
  }
  return UNET_OK;
}

// Workspace: every tensor is two fp16 planes (hi, then lo `elems` halfs behind); offsets in bytes
struct WsTensor {
  size_t off = 0, elems = 0;   // hi plane at off, lo plane at off + 2 * elems bytes
};
struct WsPlanX3 {
  std::vector<WsTensor> cat, pool;
  WsTensor tmpA, tmpB;
  size_t total = 0;
};

WsPlanX3 plan_ws_x3(const unet_config& c, int n, int h, int w) {
  WsPlanX3 p;
  size_t off = 0;
  auto take = [&](size_t elems) {
    WsTensor t;
    t.off = off;
    t.elems = (elems + 127) / 128 * 128;   // planes stay 256-byte aligned
    off += 2 * t.elems * sizeof(uint16_t);
    return t;
  };
  const size_t px0 = (size_t)n * h * w;
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

// classes: the outputs of a K-class handle (unet_forward_classes_*: the head never rides in the last convolution, which
// stores its operand planes, and the K-way head reads them); null for the single-class entry points
int forward_x3(unet_ctx* h, const void* input, bool u8, int n, int height, int width, float* logits, float* probs,
               uint8_t* mask, float thr, hipStream_t s, const ClassOut* classes) {
  if (!h || !input) return UNET_ERR_INVALID_ARG;
  if (!classes)
    if (int rc = single_class_only(h, u8 ? "unet_forward_u8_x3" : "unet_forward_f32_x3")) return rc;
  if (classes && g_x3CrossFp8 == 1) {
    h->err = "the K-class forward runs on the fp32 and f16x3 tiers; the f16q8 switch (unet_set_x3_cross_fp8) is on";
    return UNET_ERR_INVALID_ARG;
  }
  if (!h->finalized) {
    h->err = "unet_finalize has not been called";
    return UNET_ERR_STATE;
  }
  int rc = check_shape(h, n, height, width);
  if (rc) return rc;
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  if (h->x3 && g_x3CrossFp8 == 1 && !h->x3->hasQ8) {   // the f16q8 tier was switched on after the operators were built
    HIPCHK(h->err, hipDeviceSynchronize());
    x3_free(h);
  }
  if (!h->x3 && (rc = x3_build(h))) return rc;
  X3Net* X = h->x3;
  const unet_config& c = h->cfg;
  const WsPlanX3 p = plan_ws_x3(c, n, height, width);
  uint8_t* qs = nullptr;
  if (g_x3CrossFp8 == 1 && X->hasQ8) {
    // largest input of a layer the tier can take: n * (h w / 4^l) * cin * 2 bytes over the levels l >= 1
    size_t need = 0;
    for (int l = 1; l <= c.depth; ++l) {
      const size_t px = (size_t)n * (height >> l) * (width >> l);
      const size_t cinMax = l < c.depth ? 2 * (size_t)c.features[l] : 2 * (size_t)c.features[c.depth - 1];
      need = std::max(need, px * cinMax * 2);
    }
    if ((rc = X->qbuf.reserve(h->err, need, "f16q8 q-plane"))) return rc;
    qs = reinterpret_cast<uint8_t*>(X->qbuf.p);
  }
  if ((rc = X->ws.reserve(h->err, p.total, "f16x3 workspace"))) return rc;
  LaunchScope scope(h);
  auto U = [&](const WsTensor& t) { return reinterpret_cast<uint16_t*>(X->ws.p + t.off); };
  X3SplitK sk;
  sk.scratch = X->splitScratch;
  sk.floats = kSplitFloats;
  sk.ones = X->ones;
  sk.zerosF = reinterpret_cast<const float*>(X->zeros);
  const size_t npix = (size_t)n * height * width;
  const WsTensor* cur = nullptr;
  int ch = height, cw = width;
  X3Q8Link lk1, lk2;
  // a layer as the forward launches it: its tensors by workspace slot; the forward's split-K and q-plane scratch
  auto io_of = [&](const WsTensor& in, int hh, int ww, const WsTensor& out, int ldo, int coOff) {
    return x3_from(X->zeros, U(in), in.elems, n, hh, ww).to(U(out), out.elems, ldo, coOff);
  };
  auto opts_of = [&](X3Q8Link* lk, const X3Fuse* fuse) {
    X3ConvOpts o;
    o.fuse = fuse;
    o.splitK = &sk;
    o.qScratch = qs;
    o.q8Link = lk;
    return o;
  };
  // the look-ahead of the f16q8 tier: will that launch run on conv_q8_r512.h (x3_plan_conv's own answer for the same
  // epilogue and scratch)?  Its producer then writes a q plane in the lo plane's place
  auto lands_on_q8 = [&](const GemmOpX3& op, const X3ConvIo& io, const X3Fuse* fuse) {
    const X3ConvPlan pl = x3_plan_conv(x3_conv_query(op, io, opts_of(nullptr, fuse)));
    return qs && pl.valid && pl.path.structure == kX3Q8;
  };
  // f16q8 tier, decided per level before anything is overwritten: catQ - the concat buffer's lo plane becomes its q plane
  // (skip half: by the encoder's pooling pass, in place; upper half: by the transposed convolution) because the
  // decoder's first convolution, its only other reader, is of the tier; poolQ - the same for the pooled tensor and
  // the next level's first convolution
  std::vector<char> catQ(c.depth, 0), poolQ(c.depth, 0);
  for (int l = 0; l < c.depth; ++l) {
    const int f = c.features[l];
    // the block's second convolution: pooled, into the skip half of the concat buffer
    X3Fuse fz;
    fz.pool = U(p.pool[l]);
    fz.poolLo = p.pool[l].elems;
    const X3ConvIo conv2Io = io_of(p.tmpA, ch, cw, p.cat[l], 2 * f, 0);
    const bool conv2OnQ8 = lands_on_q8(X->enc[2 * l + 1], conv2Io, &fz);
    if (l == 0) {
      // the whole block as one launch where x3_plan_enc1 takes it: the first convolution's planes are never stored
      const X3Enc1Plan ep = x3_plan_enc1(u8, x3_fuse_first_mode() != 0, x3_conv_query(X->enc[1], conv2Io, opts_of(nullptr, &fz)));
      if (ep.take) {
        HIPCHK(h->err, run_enc1_x3(ep, X->enc[0], X->enc[1], input, conv2Io, fz, c.input_mean, c.input_std, s));
        cur = &p.pool[l];
        ch /= 2;
        cw /= 2;
        continue;
      }
      HIPCHK(h->err, run_first_x3(X->enc[0], input, u8, n, ch, cw, U(p.tmpA), p.tmpA.elems, f, c.input_mean, c.input_std, s));
    } else {
      // f16q8 tier: tmpA has one consumer, the block's second convolution; where that one runs on conv_q8_r512.h the
      // first writes tmpA's q plane in the lo plane's place (X3Q8Link) and no conversion pass is needed
      lk1 = X3Q8Link();
      lk1.inIsQ = poolQ[l - 1];
      lk1.wantOutQ = conv2OnQ8;
      HIPCHK(h->err, run_conv_x3(X->enc[2 * l], io_of(*cur, ch, cw, p.tmpA, f, 0), opts_of(&lk1, nullptr), s));
    }
    lk2 = X3Q8Link();
    lk2.inIsQ = l > 0 && lk1.wroteQ;
    if (conv2OnQ8) {
      const int jd = c.depth - 1 - l;
      const GemmOpX3& nextConv1 = l + 1 < c.depth ? X->enc[2 * (l + 1)] : X->bott[0];
      catQ[l] = lands_on_q8(X->dec[jd].conv1, io_of(p.cat[l], ch, cw, p.tmpA, f, 0), nullptr) &&
                x3_plan_upconv(x3_upconv_query(X->dec[jd].up, io_of(p.tmpB, ch / 2, cw / 2, p.cat[l], 2 * f, f), true)).valid;
      poolQ[l] = lands_on_q8(nextConv1, io_of(p.pool[l], ch / 2, cw / 2, p.tmpA, 2 * f, 0), nullptr);
      lk2.poolSrcQ = catQ[l];
      lk2.poolDstQ = poolQ[l];
    }
    HIPCHK(h->err, run_conv_x3(X->enc[2 * l + 1], conv2Io, opts_of(&lk2, &fz), s));
    if (lk2.srcQDone != (bool)catQ[l] || lk2.pooledQ != (bool)poolQ[l]) {
      h->err = "f16q8: a pooling pass did not hand its q planes on as planned";
      return UNET_ERR_STATE;
    }
    cur = &p.pool[l];
    ch /= 2;
    cw /= 2;
  }
  const int fb = 2 * c.features[c.depth - 1];
  lk1 = X3Q8Link();
  lk1.inIsQ = poolQ[c.depth - 1];
  const X3ConvIo bott2Io = io_of(p.tmpA, ch, cw, p.tmpB, fb, 0);
  lk1.wantOutQ = lands_on_q8(X->bott[1], bott2Io, nullptr);
  HIPCHK(h->err, run_conv_x3(X->bott[0], io_of(*cur, ch, cw, p.tmpA, fb, 0), opts_of(&lk1, nullptr), s));
  lk2 = X3Q8Link();
  lk2.inIsQ = lk1.wroteQ;
  HIPCHK(h->err, run_conv_x3(X->bott[1], bott2Io, opts_of(&lk2, nullptr), s));
  cur = &p.tmpB;
  bool headFused = false;
  for (int j = 0; j < c.depth; ++j) {
    const int l = c.depth - 1 - j;
    const int f = c.features[l];
    // ConvTranspose writes the upper channel half of the concat buffer: torch.cat([skip, x]) elided
    const bool headNext = j == c.depth - 1 && f == 64 && !classes;
    // the step's form (x3_plan_dec_step): composed (conv_x3_dec.h) or deep (upconv_x3_win.h + the addend epilogue), it
    // reads the skip half of the concat buffer and x itself and writes tmpA like conv1; else the two kernels below
    const DecStepX3& st = X->dec[j];
    const X3DecStepPlan dp = x3_plan_dec_step(x3_dec_step_query(n, ch, cw, f, qs != nullptr, false));
    const bool composed = dp.form != kX3DecTwoKernel;
    if (composed) {
      const X3DecIo dio{x3_from(X->zeros, U(*cur), cur->elems, n, ch, cw).to(U(p.tmpA), p.tmpA.elems, f), U(p.cat[l]),
                        p.cat[l].elems, 2 * f, f};
      HIPCHK(h->err, run_dec_step_x3(st, dp, dio, s));
    }
    ch *= 2;
    cw *= 2;
    lk1 = X3Q8Link();
    const X3ConvIo conv2Io = io_of(p.tmpA, ch, cw, p.tmpB, f, 0);
    if (!composed) {
      X3Q8Link lku;
      lku.wantOutQ = catQ[l];
      HIPCHK(h->err, run_upconv_x3(st.up, io_of(*cur, ch / 2, cw / 2, p.cat[l], 2 * f, f), s, &lku));
      lk1.inIsQ = catQ[l];
      // (the fused-head launch below is handed no q-plane scratch: it never takes a q plane)
      lk1.wantOutQ = !headNext && lands_on_q8(st.conv2, conv2Io, nullptr);
      HIPCHK(h->err, run_conv_x3(st.conv1, io_of(p.cat[l], ch, cw, p.tmpA, f, 0), opts_of(&lk1, nullptr), s));
    }
    lk2 = X3Q8Link();
    lk2.inIsQ = lk1.wroteQ;
    if (headNext) {
      // last DoubleConv: its only consumer is the 1x1 head, fused into the epilogue (the activation is never written)
      X3Fuse fz;
      fz.headW = X->headW;
      fz.headB = h->headB;
      fz.headThr = thr;
      fz.logits = logits;
      fz.probs = probs;
      fz.mask = mask;
      X3ConvOpts oh;
      oh.fuse = &fz;
      HIPCHK(h->err, run_conv_x3(st.conv2, conv2Io, oh, s));
      headFused = true;
    } else {
      HIPCHK(h->err, run_conv_x3(st.conv2, conv2Io, opts_of(&lk2, nullptr), s));
    }
    cur = &p.tmpB;
  }
  if (classes) {
    const int f0 = c.features[0];
    prof_begin("headk_f16x3", 2.0 * npix * f0 * c.out_channels, 4.0 * npix * f0, s);
    const hipError_t e = unet::launch_headk_planes(U(*cur), cur->elems, X->headW, h->headBk, n, (size_t)height * width, f0,
                                                   c.out_channels, classes->logits, classes->probs, classes->labels,
                                                   classes->maskClass, classes->mask, s);
    prof_end(s);
    HIPCHK(h->err, e);
  } else if (!headFused) {
    const int f0 = c.features[0];
    prof_begin("head1x1_f16x3", 2.0 * npix * f0, 4.0 * npix * f0 + 4.0 * npix, s);
    hipLaunchKernelGGL(unet::head1x1_planes_kernel, dim3(grid_for(npix)), dim3(256), 0, s,
                       reinterpret_cast<const uint32_t*>(U(*cur)), cur->elems / 2, X->headW, h->headB, npix, f0, logits,
                       probs, mask, thr);
    prof_end(s);
    HIPCHK(h->err, hipGetLastError());
  }
  return h->async_error();
}

ActScale act_from_host(const float* act, int c) {
  ActScale a;
  a.act.assign(act, act + c);
  a.mag.assign(c, 0.f);
  return a;
}

// An operator entry point's decoder step: the plan for the one operator it built (`have`), forced; a plan that declines
// is an invalid call
hipError_t run_dec_step_entry(const DecStepX3& st, int have, bool windowOnly, const X3DecIo& io, int f, hipStream_t s) {
  X3DecStepQuery q = x3_dec_step_query(io.xo.n, io.xo.h, io.xo.w, f, false, true, have);
  q.windowOnly = windowOnly;
  const X3DecStepPlan p = x3_plan_dec_step(q);
  return p.form == kX3DecTwoKernel ? hipErrorInvalidValue : run_dec_step_x3(st, p, io, s);
}

// the deep operator's two entry points: build it, run it (or its kernel 1 alone) on caller-owned planes under a range watch
int updeep_entry(int device, const float* wt, const float* bt, const float* w3, int f, const float* scale, const float* shift,
                 int relu, const float* xAct, const float* skipAct, bool windowOnly, X3DecIo io, int* rangeOut, void* stream) {
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<DecStepX3> g;
  const ActScale xa = act_from_host(xAct, xAct ? 2 * f : 0), sa = act_from_host(skipAct, skipAct ? f : 0);
  const int rc = build_dec_step_x3(g_opErr, g.op, kX3DecDeep, wt, bt, w3, f, scale, shift, relu, skipAct ? &sa : nullptr,
                                   xAct ? &xa : nullptr, nullptr);
  if (rc) return rc;
  uint16_t* zeros = nullptr;
  OpRangeScope range;
  hipError_t e = sc.zero_page(&zeros);
  io.xo.zeros = zeros;
  if (e == hipSuccess) e = range.arm();
  if (e == hipSuccess) e = run_dec_step_entry(g.op, kX3DecDeep, windowOnly, io, f, s);
  return op_done(e, s, 0, &range, rangeOut);
}

void path_to_ints(const X3Path& p, int* out) {
  if (!out) return;
  const int v[8] = {p.structure, p.tileW, p.epi, p.flat, p.kSplit, p.waves, p.poolPass, 0};
  std::copy(v, v + 8, out);
}

}  // namespace

extern "C" {

int unet_forward_u8_x3(unet_handle_t h, const uint8_t* frames, int n, int height, int width, float* logits,
                       float* probs, uint8_t* mask, float thr, void* stream) {
  return forward_x3(h, frames, true, n, height, width, logits, probs, mask, thr, (hipStream_t)stream, nullptr);
}

int unet_forward_f32_x3(unet_handle_t h, const float* image, int n, int height, int width, float* logits,
                        float* probs, uint8_t* mask, float thr, void* stream) {
  return forward_x3(h, image, false, n, height, width, logits, probs, mask, thr, (hipStream_t)stream, nullptr);
}

// ---- single operators of the tier (test entry points): fp32 NHWC in / out, planes internally ----

int unet_op_conv3x3_x3(int device, const float* x, int n, int hh, int ww, int cin, const float* wHost,
                       const float* scale, const float* shift, int cout, int relu, int tileWidth, float* y,
                       float* yPool, void* stream) {
  X3Force force;
  if (!x || !wHost || !scale || !shift || !y || cin % 64 || cout % 64 || cout > unet::X3Shape<32>::MAX_COUT ||
      !x3_decode_force(tileWidth, &force) || (yPool && (hh % 2 || ww % 2)))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOpX3> g;
  const bool q8 = force.family == kX3Q8;
  const int rc = build_conv_x3(g_opErr, g.op, wHost, cout, cin, scale, shift, relu, false, nullptr, nullptr, q8);
  if (rc) return rc;
  const size_t px = (size_t)n * hh * ww;
  const size_t ein = px * cin, eout = px * cout, epool = (px / 4) * cout;
  uint16_t *zeros = nullptr, *pin = nullptr, *pout = nullptr, *ppool = nullptr, *qsc = nullptr;
  hipError_t e = sc.zero_page(&zeros);
  if (e == hipSuccess) e = sc.get(&pin, 2 * ein * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.get(&pout, 2 * eout * sizeof(uint16_t));
  if (e == hipSuccess && yPool) e = sc.get(&ppool, 2 * epool * sizeof(uint16_t));
  if (e == hipSuccess && q8) e = sc.get(&qsc, ein * sizeof(uint16_t));
  if (e == hipSuccess) {
    split_to_planes(x, ein, pin, s);
    X3Fuse fz;
    fz.pool = ppool;
    fz.poolLo = epool;
    X3ConvOpts o;
    o.fuse = yPool ? &fz : nullptr;
    o.forceTw = tileWidth;
    o.qScratch = reinterpret_cast<uint8_t*>(qsc);
    e = run_conv_x3(g.op, x3_from(zeros, pin, ein, n, hh, ww).to(pout, eout, cout), o, s);
  }
  if (e == hipSuccess) {
    merge_from_planes(pout, eout, y, s);
    if (yPool) merge_from_planes(ppool, epool, yPool, s);
    e = hipGetLastError();
  }
  return op_done(e, s);
}

// Test entry point: the 64-channel 3x3 convolution with the 1x1 head fused into its epilogue (the network's last two
// layers, reference README.md:1447, :1481): x (n,h,w,cin) fp32 NHWC -> logits (n,h,w) fp32.  tileWidth 0 / 16 / 32: first
// structure, 628 / 632: third structure.
int unet_op_conv3x3_x3_head(int device, const float* x, int n, int hh, int ww, int cin, const float* wHost,
                            const float* scale, const float* shift, int relu, int tileWidth, const float* headW,
                            float headB, float* logits, void* stream) {
  // (the fused head exists on the first structure and on the third's 16-row tiles)
  X3Force force;
  if (!x || !wHost || !scale || !shift || !headW || !logits || cin % 64 || !x3_decode_force(tileWidth, &force) ||
      !(force.family == 0 || force.family == kX3Ws || (force.family == kX3T448 && force.waves != 4)))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOpX3> g;
  const int rc = build_conv_x3(g_opErr, g.op, wHost, 64, cin, scale, shift, relu, false, nullptr, nullptr, false);
  if (rc) return rc;
  const size_t px = (size_t)n * hh * ww, ein = px * cin;
  uint16_t *zeros = nullptr, *pin = nullptr;
  float* hwDev = nullptr;
  hipError_t e = sc.zero_page(&zeros);
  if (e == hipSuccess) e = sc.get(&pin, 2 * ein * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.upload(&hwDev, headW, 64);
  if (e == hipSuccess) {
    split_to_planes(x, ein, pin, s);
    X3Fuse fz;
    fz.headW = hwDev;
    fz.headB = headB;
    fz.headThr = 0.f;
    fz.logits = logits;
    X3ConvOpts o;
    o.fuse = &fz;
    o.forceTw = tileWidth;
    e = run_conv_x3(g.op, x3_from(zeros, pin, ein, n, hh, ww).to(nullptr, 0, 64), o, s);
  }
  return op_done(e, s);
}

// Test hook (host arithmetic only, no device): the power-of-two activation scale the f16x3 tier picks for a BatchNorm
// channel with these parameters (act_from_bn)
float unet_debug_act_scale(float gamma, float beta) { return act_from_bn(&gamma, &beta, 1).act[0]; }

// Test entry point: the decoder step ConvTranspose2d(2f -> f, k2, s2, bias) -> cat([skip, up]) -> Conv3x3(2f -> f) ->
// scale / shift (+ ReLU) as the composed operator (conv_x3_dec.h): skip (n,h,w,f) and x (n,h/2,w/2,2f) fp32 NHWC on the
// device -> y (n,h,w,f); wt (2f,f,2,2), bt (f), w3 (f,2f,3,3), scale / shift (f) on the host
int unet_op_upcat_conv3x3_x3(int device, const float* skip, const float* x, int n, int hh, int ww, int f, const float* wt,
                             const float* bt, const float* w3, const float* scale, const float* shift, int relu, float* y,
                             void* stream) {
  if (!skip || !x || !wt || !bt || !w3 || !scale || !shift || !y || n < 1 || f % 64 || f > 256 || ww % 28 || hh % 2 || hh < 2)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<DecStepX3> g;
  const int rc = build_dec_step_x3(g_opErr, g.op, kX3DecComposed, wt, bt, w3, f, scale, shift, relu, nullptr, nullptr, nullptr);
  if (rc) return rc;
  const size_t px = (size_t)n * hh * ww;
  const size_t es = px * f, ex = px / 4 * 2 * f, eo = px * f;
  uint16_t *zeros = nullptr, *ps = nullptr, *pxl = nullptr, *po = nullptr;
  hipError_t e = sc.zero_page(&zeros);
  if (e == hipSuccess) e = sc.get(&ps, 2 * es * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.get(&pxl, 2 * ex * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.get(&po, 2 * eo * sizeof(uint16_t));
  if (e == hipSuccess) {
    split_to_planes(skip, es, ps, s);
    split_to_planes(x, ex, pxl, s);
    e = run_dec_step_entry(g.op, kX3DecComposed, false, {x3_from(zeros, pxl, ex, n, hh / 2, ww / 2).to(po, eo, f), ps, es, f, 0}, f, s);
  }
  if (e == hipSuccess) {
    merge_from_planes(po, eo, y, s);
    e = hipGetLastError();
  }
  return op_done(e, s);
}

// Test hook (host arithmetic only, no device): the float64 composition the operator above is built from (compose_upcat)
int unet_host_compose_upcat(const float* wt, const float* bt, const float* w3, int f, double* wp, double* bias) {
  if (!wt || !bt || !w3 || !wp || !bias || f < 1) return op_bad_args();
  std::vector<double> a, b;
  compose_upcat(wt, bt, w3, f, a, b);
  std::copy(a.begin(), a.end(), wp);
  std::copy(b.begin(), b.end(), bias);
  return UNET_OK;
}

// Test hook (host arithmetic only, no device): the packed fp16 hi / lo halfs of host weights x pre[cout], as the
// operators upload them.  kind 0: 3x3, w (cout,cin,3,3); 1: transposed, w (cin,cout,2,2); 2: first convolution, w
// (cout,3,3,3), cin = 3; 3: the composed decoder step, w = the skip half (f,f,3,3), wx = the window weights
// [parity 4][f][2f][tap 4], cout = f, cin = 2f.  nPacked: the pack's size in halfs, checked
int unet_host_pack_x3(int kind, const float* w, const float* wx, int cout, int cin, const float* pre, uint16_t* packed,
                      size_t nPacked) {
  if (!w || !pre || !packed || kind < 0 || kind > 3 || cout < 64 || cout % 64 || (kind == 2 ? cin != 3 : cin < 32 || cin % 32) ||
      (kind == 3 && (!wx || cin != 2 * cout)))
    return op_bad_args();
  const std::vector<float> pv(pre, pre + cout);
  const std::vector<uint16_t> out = kind == 0   ? pack_conv_x3(w, cout, cin, pv)
                                    : kind == 1 ? pack_upconv_x3(w, cin, cout, pv)
                                    : kind == 2 ? pack_first_x3(w, cout, pv)
                                                : pack_upcat_x3(w, wx, cout, pv);
  if (out.size() != nPacked) return op_bad_args();
  std::copy(out.begin(), out.end(), packed);
  return UNET_OK;
}

// Test hook (host arithmetic only, no device): what build_dec_step_x3 packs for kernel 1 of the deep form
// (pack_updeep_x3).  ordered: the float64 window weights at the pack's hi-plane positions (the lo-plane positions stay
// 0); packed: the fp16 hi / lo planes of weight / xAct x pre; pre [f]; cls [9][f] in float64 (kernel 1 gets them rounded
// to fp32)
int unet_host_pack_updeep_x3(const float* wt, const float* bt, const float* w3, int f, const float* xAct, double* ordered,
                             uint16_t* packed, float* pre, double* cls) {
  if (!wt || !bt || !w3 || !ordered || !packed || !pre || !cls || f < 64 || f % 64) return op_bad_args();
  DecHostX3 hst;
  std::vector<float> preW;
  std::vector<double> ord;
  dec_host_x3(hst, wt, bt, w3, f, nullptr, xAct);
  const std::vector<uint16_t> win = pack_updeep_x3(hst, preW, &ord);
  std::copy(ord.begin(), ord.end(), ordered);
  std::copy(win.begin(), win.end(), packed);
  std::copy(preW.begin(), preW.end(), pre);
  std::copy(hst.bias.begin(), hst.bias.end(), cls);
  return UNET_OK;
}

namespace {
void updeep_to_ints(const X3UpdeepPlan& p, int* out) {   // all 0 where the plan declines
  const int v[8] = {1, p.wmax, p.pixTiles, p.coTiles, p.grid, p.conv.grid, p.conv.path.flat, p.conv.pixTiles};
  std::fill(out, out + 8, 0);
  if (p.take) std::copy(v, v + 8, out);
}
inline int mode3(int v) { return v < 0 ? -1 : (v > 1 ? 1 : v); }
}  // namespace

// Test hook (no device): x3_plan_updeep for query = {n, h, w, f, compose mode, deep switch, f16q8 on} (h, w: the
// low-resolution map) -> planOut = {taken, kernel 1: widest map of its instance, pixel tiles, channel tiles, grid;
// kernel 2: grid, flat tiling, pixel tiles}, all 0 where the plan declines
int unet_host_plan_updeep_x3(const int* query, int nQuery, int* planOut, int nPlan) {
  if (!query || nQuery != 7 || !planOut || nPlan != 8) return op_bad_args();
  X3DecStepQuery q;
  q.n = query[0], q.h = query[1], q.w = query[2], q.f = query[3];
  q.compose = mode3(query[4]);
  q.deep = query[5] != 0, q.q8 = query[6] != 0;
  updeep_to_ints(x3_plan_updeep(q), planOut);
  return UNET_OK;
}

// Test hook (no device): x3_plan_dec_step and the labels of the step's launches (include/unet_hip.h lists the layouts)
int unet_host_plan_dec_step_x3(const int* query, int nQuery, int* planOut, int nPlan, char* labelOut, int labelCap) {
  if (!query || nQuery != 17 || !planOut || nPlan != 16 || (labelOut && labelCap < 128)) return op_bad_args();
  if (query[0] < 1 || query[1] < 1 || query[2] < 1 || query[3] < 64 || query[3] % 64) return op_bad_args();
  X3DecStepQuery q;
  q.n = query[0], q.h = query[1], q.w = query[2], q.f = query[3];
  q.compose = mode3(query[4]), q.deep = query[5] != 0, q.decForm = (query[6] == 1 || query[6] == 2) ? query[6] : -1;
  q.q8 = query[7] != 0, q.entry = query[8] != 0, q.have = query[9], q.windowOnly = query[10] != 0;
  q.upconvMode = mode3(query[11]);
  q.sw.flat = query[12] != 0, q.sw.r512 = query[13] != 0, q.sw.t448 = query[14] != 0, q.sw.t448c4 = query[15] != 0;
  q.sw.crossFp8 = query[16];
  const X3DecStepPlan p = x3_plan_dec_step(q);
  const int head[8] = {p.form, p.wco, p.tilesX, p.tilesY, p.pixTiles, p.coTiles, p.grid, p.nLaunch};
  std::fill(planOut, planOut + 16, 0);
  if (p.form == kX3DecComposed) std::copy(head, head + 8, planOut);
  if (p.form == kX3DecDeep) planOut[0] = p.form, planOut[7] = p.nLaunch, updeep_to_ints(p.deep, planOut + 8);
  if (labelOut) x3_dec_step_labels(q, p, labelOut, (size_t)labelCap);
  return UNET_OK;
}

int unet_set_x3_compose_deep(int on) {
  const int prev = x3_compose_deep_mode();
  x3_compose_deep_mode() = on ? 1 : 0;
  return prev;
}

int unet_set_x3_fuse_first(int on) {
  const int prev = x3_fuse_first_mode();
  x3_fuse_first_mode() = on ? 1 : 0;
  return prev;
}

namespace {
// the second convolution of the first block as forward_x3 asks for it: 64 -> cout, pooled epilogue, the forward's split-K
// scratch, the f16q8 scratch and fragments where the tier is on
X3ConvQuery enc1_conv2_query(int n, int h, int w, int cout, bool q8, const X3Force& force, const X3Switches& sw) {
  X3ConvQuery q;
  q.n = n, q.h = h, q.w = w, q.cin = 64, q.cout = cout, q.epi = 1;
  q.force = force;
  q.splitScratch = true, q.splitFloats = kSplitFloats;
  q.qScratch = q.wq = q8;
  q.sw = sw;
  return q;
}
}  // namespace

// Test hook (no device): x3_plan_enc1 for query = {input is uint8, n, h, w, cout, forced form of the second convolution
// (0 = none), f16q8 scratch present, unet_set_x3_fuse_first's switch, UNET_X3_FLAT, _R512, _T448, _T448_C4, cross-fp8
// mode} -> planOut = {taken, grid, tiles along x, tiles along y, pixel tiles, 0, 0, 0}, all 0 where the plan declines
int unet_host_plan_enc1_x3(const int* query, int nQuery, int* planOut, int nPlan) {
  if (!query || nQuery != 13 || !planOut || nPlan != 8) return op_bad_args();
  X3Force force;
  if (query[1] < 1 || query[2] < 1 || query[3] < 1 || query[4] < 64 || query[4] % 64 || !x3_decode_force(query[5], &force))
    return op_bad_args();
  X3Switches sw;
  sw.flat = query[8] != 0, sw.r512 = query[9] != 0, sw.t448 = query[10] != 0, sw.t448c4 = query[11] != 0;
  sw.crossFp8 = query[12];
  const X3Enc1Plan p =
      x3_plan_enc1(query[0] != 0, query[7] != 0, enc1_conv2_query(query[1], query[2], query[3], query[4], query[6] != 0, force, sw));
  std::fill(planOut, planOut + 8, 0);
  if (p.take) {
    const int v[5] = {1, p.conv.grid, p.conv.tilesX, p.conv.tilesY, p.conv.pixTiles};
    std::copy(v, v + 5, planOut);
  }
  return UNET_OK;
}

// Test entry point: the first encoder block on the fused kernel (conv_x3_enc1.h), operators built as x3_build builds
// them.  frames (n,hh,ww,3) uint8 -> y planes (pixel stride ldo, channels [coOff, coOff + 64)) and their pooled planes
// (n,hh/2,ww/2,64).  act1 / act2 (64 each, or null): the activation scales of the two layers' outputs.  tileWidth: the
// forced form of the second convolution (0: the dispatch's own answer, 628: the third structure); a plan that declines
// is an invalid call.  pathOut[0..6]: the second convolution's path, pathOut[7] = 1: the fused kernel ran
int unet_op_enc1_x3_planes(int device, const void* frames, int n, int hh, int ww, const float* w1Host, const float* scale1,
                           const float* shift1, int relu1, const float* mean, const float* stdv, const float* act1,
                           const float* w2Host, const float* scale2, const float* shift2, int relu2, const float* act2,
                           int tileWidth, uint16_t* y, size_t yLo, int ldo, int coOff, uint16_t* pool, size_t poolLo,
                           int* pathOut, int* rangeOut, void* stream) {
  X3Force force;
  if (ldo == 0) ldo = 64;
  if (!frames || !w1Host || !scale1 || !shift1 || !mean || !stdv || !w2Host || !scale2 || !shift2 || !y || !pool || n < 1 ||
      hh < 2 || ww < 2 || hh % 2 || ww % 2 || yLo % 8 || poolLo % 8 || ldo % 64 || coOff < 0 || coOff % 64 || coOff + 64 > ldo ||
      !x3_decode_force(tileWidth, &force))
    return op_bad_args();
  path_to_ints(X3Path(), pathOut);
  X3Enc1Plan plan = x3_plan_enc1(true, true, enc1_conv2_query(n, hh, ww, 64, false, force, x3_switches()));
  if (!plan.take) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOpX3> g1, g2;
  ActScale a1, a2;
  if (act1) a1 = act_from_host(act1, 64);
  if (act2) a2 = act_from_host(act2, 64);
  int rc = build_conv_x3(g_opErr, g1.op, w1Host, 64, 3, scale1, shift1, relu1, true, nullptr, act1 ? &a1 : nullptr, false);
  if (!rc)
    rc = build_conv_x3(g_opErr, g2.op, w2Host, 64, 64, scale2, shift2, relu2, false, act1 ? &a1 : nullptr, act2 ? &a2 : nullptr,
                       false);
  if (rc) return rc;
  OpRangeScope range;
  X3Path path;
  hipError_t e = range.arm();
  if (e == hipSuccess) {
    X3Fuse fz;
    fz.pool = pool;
    fz.poolLo = poolLo;
    e = run_enc1_x3(plan, g1.op, g2.op, frames, x3_from(nullptr, nullptr, 0, n, hh, ww).to(y, yLo, ldo, coOff), fz, mean, stdv, s,
                    &path);
  }
  const int st = op_done(e, s, 0, &range, rangeOut);
  path_to_ints(path, pathOut);
  if (pathOut && st == UNET_OK) pathOut[7] = 1;
  return st;
}

// Test entry point: kernel 1 of the deep levels' split step alone (upconv_x3_win.h), on caller-owned planes.  x planes
// (n,hh,ww,2f) -> P planes (n,2hh,2ww) at pixel stride ldo, channels [coOff, coOff + f) of y; wt (2f,f,2,2), bt (f),
// w3 (f,2f,3,3) on the host; inAct: x's per-channel activation scales (2f) or null
int unet_op_updeep_window_x3_planes(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int f, const float* wt,
                                    const float* bt, const float* w3, const float* inAct, uint16_t* y, size_t yLo, int ldo,
                                    int coOff, int* rangeOut, void* stream) {
  if (ldo == 0) ldo = f;
  if (!x || !wt || !bt || !w3 || !y || n < 1 || hh < 1 || ww < 4 || ww > 28 || f < 64 || f % 64 || f > 1024 || xLo % 8 ||
      yLo % 8 || ldo % 64 || coOff < 0 || coOff % 64 || coOff + f > ldo)
    return op_bad_args();
  const std::vector<float> one(f, 1.f), zero(f, 0.f);
  return updeep_entry(device, wt, bt, w3, f, one.data(), zero.data(), 0, inAct, nullptr, true,
                      {x3_from(nullptr, x, xLo, n, hh, ww), y, yLo, ldo, coOff}, rangeOut, stream);
}

// Test entry point: both kernels as the forward runs them.  cat: the concat buffer's planes (n,2hh,2ww,2f) with the skip
// in channels [0,f) (the caller's bits; they are only read) - P goes to channels [f,2f); out planes (n,2hh,2ww,f).
// xAct (2f) / skipAct (f): activation scales of x and of the skip, or null
int unet_op_updeep_conv3x3_x3_planes(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int f, const float* wt,
                                     const float* bt, const float* w3, const float* scale, const float* shift, int relu,
                                     const float* xAct, const float* skipAct, uint16_t* cat, size_t catLo, uint16_t* out,
                                     size_t outLo, int* rangeOut, void* stream) {
  if (!x || !wt || !bt || !w3 || !scale || !shift || !cat || !out || n < 1 || hh < 1 || ww < 4 || ww > 28 || f < 256 ||
      f % 256 || f > 1024 || xLo % 8 || catLo % 8 || outLo % 8)
    return op_bad_args();
  return updeep_entry(device, wt, bt, w3, f, scale, shift, relu, xAct, skipAct, false,
                      {x3_from(nullptr, x, xLo, n, hh, ww).to(out, outLo, f), cat, catLo, 2 * f, f}, rangeOut, stream);
}

// Test hooks (host arithmetic only, no device): the plan the dispatch makes for a query given as integers, the switches
// included (include/unet_hip.h lists both layouts)
int unet_host_plan_conv3x3_x3(const int* query, int nQuery, int* planOut, int nPlan, char* labelOut, int labelCap) {
  if (!query || nQuery != 22 || !planOut || nPlan != 24 || (labelOut && labelCap < 48)) return op_bad_args();
  X3ConvQuery q;
  q.n = query[0], q.h = query[1], q.w = query[2], q.cin = query[3], q.cout = query[4], q.epi = query[5];
  if (q.n < 1 || q.h < 1 || q.w < 1 || q.cin < 32 || q.cout < 64 || q.epi < 0 || q.epi > 3 || query[9] < 0 ||
      !x3_decode_force(query[6], &q.force))
    return op_bad_args();
  q.coOff = query[7], q.splitScratch = query[8] != 0, q.splitFloats = (size_t)query[9];
  q.qScratch = query[10] != 0, q.wq = query[11] != 0;
  q.inIsQ = query[12] != 0, q.wantOutQ = query[13] != 0, q.poolSrcQ = query[14] != 0, q.poolDstQ = query[15] != 0;
  q.wantStats = query[16] != 0;
  q.sw.flat = query[17] != 0, q.sw.r512 = query[18] != 0, q.sw.t448 = query[19] != 0, q.sw.t448c4 = query[20] != 0;
  q.sw.crossFp8 = query[21];
  const X3ConvPlan p = x3_plan_conv(q);
  path_to_ints(p.path, planOut);
  const int rest[17] = {p.grid,   p.statRows, p.toQ8Pass ? 1 : 0, p.poolPass, p.finishPass ? 1 : 0, p.outQ ? 1 : 0,
                        p.valid ? 1 : 0, p.N,  p.H,  p.imgH,     p.tilesX,   p.tilesY, p.pixTiles, p.coTiles, p.coGroup,
                        p.nChunks, p.kSplit};
  std::copy(rest, rest + 17, planOut + 7);
  if (!p.valid) std::fill(planOut, planOut + 24, 0);
  if (labelOut) {
    labelOut[0] = 0;
    if (p.valid) x3_conv_label(p, labelOut, (size_t)labelCap);
  }
  return UNET_OK;
}

int unet_host_plan_upconv2x2_x3(const int* query, int nQuery, int* planOut, int nPlan, char* labelOut, int labelCap) {
  if (!query || nQuery != 9 || !planOut || nPlan != 16 || (labelOut && labelCap < 48)) return op_bad_args();
  X3UpconvQuery q;
  if (query[0] < 1 || query[1] < 1 || query[2] < 1 || query[3] < 64 || query[4] < 64) return op_bad_args();
  q.npix = (long)query[0] * query[1] * query[2], q.w = query[2], q.cin = query[3], q.cout = query[4];
  q.coOff = query[5], q.wantOutQ = query[6] != 0;
  q.mode = query[7] < 0 ? -1 : (query[7] > 1 ? 1 : query[7]);
  q.gemm = query[8] != 0;
  const X3UpconvPlan p = x3_plan_upconv(q);
  path_to_ints(p.path, planOut);
  const int rest[9] = {p.grid, 0, 0, 0, 0, p.outQ ? 1 : 0, p.valid ? 1 : 0, p.pixTiles, p.coTiles};
  std::copy(rest, rest + 9, planOut + 7);
  if (!p.valid) std::fill(planOut, planOut + 16, 0);
  if (labelOut) snprintf(labelOut, (size_t)labelCap, "%s", p.valid && !q.gemm ? x3_upconv_label(p) : "");
  return UNET_OK;
}

int unet_set_x3_compose(int mode) {
  const int prev = x3_compose_mode();
  x3_compose_mode() = mode < 0 ? -1 : (mode > 1 ? 1 : mode);
  return prev;
}

int unet_set_x3_dec_form(int mode) {
  const int prev = x3_dec_form_mode();
  x3_dec_form_mode() = (mode == 1 || mode == 2) ? mode : -1;
  return prev;
}

int unet_set_x3_cross_fp8(int mode) {
  const int prev = g_x3CrossFp8;
  g_x3CrossFp8 = mode == 1 ? 1 : 0;
  return prev;
}

int unet_set_x3_upconv_r512(int mode) {
  const int prev = g_x3UpconvR512;
  g_x3UpconvR512 = mode < 0 ? -1 : (mode > 1 ? 1 : mode);
  return prev;
}

int unet_op_upconv2x2_x3(int device, const float* x, int n, int hh, int ww, int cin, const float* wHost,
                         const float* bias, int cout, float* y, void* stream) {
  if (!x || !wHost || !bias || !y || cin % 64 || cout % 64 || cout > unet::UpconvX3Shape::MAX_COUT)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  OpGuard<GemmOpX3> g;
  const int rc = build_upconv_x3(g_opErr, g.op, wHost, cin, cout, bias);
  if (rc) return rc;
  const size_t px = (size_t)n * hh * ww;
  const size_t ein = px * cin, eout = 4 * px * cout;
  uint16_t *zeros = nullptr, *pin = nullptr, *pout = nullptr;
  hipError_t e = sc.zero_page(&zeros);
  if (e == hipSuccess) e = sc.get(&pin, 2 * ein * sizeof(uint16_t));
  if (e == hipSuccess) e = sc.get(&pout, 2 * eout * sizeof(uint16_t));
  if (e == hipSuccess) {
    split_to_planes(x, ein, pin, s);
    e = run_upconv_x3(g.op, x3_from(zeros, pin, ein, n, hh, ww).to(pout, eout, cout), s);
  }
  if (e == hipSuccess) {
    merge_from_planes(pout, eout, y, s);
    e = hipGetLastError();
  }
  return op_done(e, s);
}

// ---- plane-level test entry points: caller-owned fp16 hi / lo planes in and out, the network's own packing, dispatch
//      and kernels (include/unet_hip.h, "The split-operand tier's operators on planes") ----

int unet_op_conv3x3_x3_planes(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int cin, const float* wHost,
                              const float* scale, const float* shift, int cout, int relu, int tileWidth, const float* inAct,
                              const float* outAct, int splitK, uint16_t* y, size_t yLo, int ldo, int coOff, uint16_t* pool,
                              size_t poolLo, const float* headW, float headB, float headThr, float* logits, float* probs,
                              uint8_t* mask, int* pathOut, int* rangeOut, void* stream) {
  X3Force force;   // (the f16q8 forms have no plane-level entry point)
  if (ldo == 0) ldo = cout;
  if (!x || !wHost || !scale || !shift || n < 1 || hh < 1 || ww < 1 || cin < 64 || cin % 64 || cout < 64 || cout % 64 ||
      cout > unet::X3Shape<32>::MAX_COUT || !x3_decode_force(tileWidth, &force) || force.family == kX3Q8 ||
      xLo % 8 || yLo % 8 || poolLo % 8 || ldo % 64 || coOff < 0 || coOff % 64 || coOff + cout > ldo ||
      (pool && (headW || hh % 2 || ww % 2)) || (headW ? (cout != 64 || !(logits || probs || mask)) : !y))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  path_to_ints(X3Path(), pathOut);
  OpScratch sc(s);
  OpGuard<GemmOpX3> g;
  ActScale ia, oa;
  if (inAct) ia = act_from_host(inAct, cin);
  if (outAct) oa = act_from_host(outAct, cout);
  const int rc = build_conv_x3(g_opErr, g.op, wHost, cout, cin, scale, shift, relu, false, inAct ? &ia : nullptr,
                               outAct ? &oa : nullptr, false);
  if (rc) return rc;
  uint16_t* zeros = nullptr;
  float *ones = nullptr, *scratch = nullptr, *hwDev = nullptr;
  OpRangeScope range;
  X3Path path;
  hipError_t e = sc.zero_page(&zeros);
  if (e == hipSuccess && splitK) {   // as x3_build / forward_x3 set the X3SplitK up
    const std::vector<float> one(1024, 1.f);
    e = sc.upload(&ones, one.data(), one.size());
    if (e == hipSuccess) e = sc.get(&scratch, kSplitFloats * sizeof(float));
  }
  if (e == hipSuccess && headW) e = sc.upload(&hwDev, headW, 64);
  if (e == hipSuccess) e = range.arm();
  if (e == hipSuccess) {
    X3Fuse fz;
    if (pool) {
      fz.pool = pool;
      fz.poolLo = poolLo;
    } else if (headW) {
      fz.headW = hwDev;
      fz.headB = headB;
      fz.headThr = headThr;
      fz.logits = logits;
      fz.probs = probs;
      fz.mask = mask;
    }
    X3SplitK sk;
    sk.scratch = scratch;
    sk.floats = kSplitFloats;
    sk.ones = ones;
    sk.zerosF = reinterpret_cast<const float*>(zeros);
    X3ConvOpts o;
    o.fuse = (pool || headW) ? &fz : nullptr;
    o.forceTw = tileWidth;
    o.splitK = splitK ? &sk : nullptr;
    o.path = &path;
    e = run_conv_x3(g.op, x3_from(zeros, x, xLo, n, hh, ww).to(y, yLo, ldo, coOff), o, s);
  }
  const int st = op_done(e, s, 0, &range, rangeOut);
  path_to_ints(path, pathOut);
  return st;
}

int unet_op_upconv2x2_x3_planes(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int cin, const float* wHost,
                                const float* bias, int cout, const float* inAct, uint16_t* y, size_t yLo, int ldo, int coOff,
                                int* pathOut, int* rangeOut, void* stream) {
  if (ldo == 0) ldo = cout;
  if (!x || !wHost || !bias || !y || n < 1 || hh < 1 || ww < 1 || cin < 64 || cin % 64 || cout < 64 || cout % 64 ||
      cout > unet::UpconvX3Shape::MAX_COUT || xLo % 8 || yLo % 8 || ldo % 64 || coOff < 0 || coOff % 64 || coOff + cout > ldo)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  path_to_ints(X3Path(), pathOut);
  OpScratch sc(s);
  OpGuard<GemmOpX3> g;
  ActScale ia;
  if (inAct) ia = act_from_host(inAct, cin);
  const int rc = build_upconv_x3(g_opErr, g.op, wHost, cin, cout, bias, inAct ? &ia : nullptr, nullptr);
  if (rc) return rc;
  uint16_t* zeros = nullptr;
  OpRangeScope range;
  X3Path path;
  hipError_t e = sc.zero_page(&zeros);
  if (e == hipSuccess) e = range.arm();
  if (e == hipSuccess) e = run_upconv_x3(g.op, x3_from(zeros, x, xLo, n, hh, ww).to(y, yLo, ldo, coOff), s, nullptr, &path);
  const int st = op_done(e, s, 0, &range, rangeOut);
  path_to_ints(path, pathOut);
  return st;
}

int unet_op_conv_first_x3_planes(int device, const void* input, int isU8, int n, int hh, int ww, const float* wHost,
                                 const float* scale, const float* shift, int cout, int relu, const float* mean,
                                 const float* stdv, const float* outAct, uint16_t* y, size_t yLo, int ldo, int* rangeOut,
                                 void* stream) {
  if (ldo == 0) ldo = cout;
  if (!input || !wHost || !scale || !shift || !y || (isU8 && (!mean || !stdv)) || n < 1 || hh < 1 || ww < 1 || cout < 64 ||
      cout % 64 || yLo % 8 || ldo % 64 || cout > ldo)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpGuard<GemmOpX3> g;
  ActScale oa;
  if (outAct) oa = act_from_host(outAct, cout);
  const int rc = build_conv_x3(g_opErr, g.op, wHost, cout, 3, scale, shift, relu, true, nullptr, outAct ? &oa : nullptr, false);
  if (rc) return rc;
  OpRangeScope range;
  hipError_t e = range.arm();
  if (e == hipSuccess) e = run_first_x3(g.op, input, isU8 != 0, n, hh, ww, y, yLo, ldo, mean, stdv, s);
  return op_done(e, s, 0, &range, rangeOut);
}

int unet_op_maxpool2x2_x3_planes(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int c, int ldi, uint16_t* y,
                                 size_t yLo, void* stream) {
  if (ldi == 0) ldi = c;
  if (!x || !y || n < 1 || hh < 2 || ww < 2 || hh % 2 || ww % 2 || c < 2 || c % 2 || ldi % 2 || c > ldi || xLo % 2 || yLo % 2)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  const size_t P = (size_t)n * hh * ww;
  hipLaunchKernelGGL(unet::maxpool2x2_planes_kernel, dim3(grid_for(P / 4 * (c / 2))), dim3(256), 0, s,
                     reinterpret_cast<const uint32_t*>(x), xLo / 2, n, hh, ww, c, ldi, reinterpret_cast<uint32_t*>(y), yLo / 2);
  return op_done(hipGetLastError(), s);
}

int unet_op_head1x1_x3_planes(int device, const uint16_t* x, size_t xLo, int n, int hh, int ww, int c, const float* wHost,
                              float bias, float thr, float* logits, float* probs, uint8_t* mask, void* stream) {
  if (!x || !wHost || !(logits || probs || mask) || n < 1 || hh < 1 || ww < 1 || c < 2 || c % 2 || xLo % 2)
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpScratch sc(s);
  float* wd = nullptr;
  hipError_t e = sc.upload(&wd, wHost, (size_t)c);
  if (e == hipSuccess) {
    const size_t npix = (size_t)n * hh * ww;
    hipLaunchKernelGGL(unet::head1x1_planes_kernel, dim3(grid_for(npix)), dim3(256), 0, s, reinterpret_cast<const uint32_t*>(x),
                       xLo / 2, wd, bias, npix, c, logits, probs, mask, thr);
    e = hipGetLastError();
  }
  return op_done(e, s);
}

int unet_op_split_planes_x3(int device, const float* x, size_t count, uint16_t* y, size_t yLo, int* rangeOut, void* stream) {
  if (!x || !y || count < 2 || count % 2 || yLo % 2) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  OpRangeScope range;
  hipError_t e = range.arm();
  if (e == hipSuccess) {   // (not split_to_planes: lo plane where the caller says, range watched)
    hipLaunchKernelGGL(unet::split_planes_kernel, dim3(grid_for(count / 2)), dim3(256), 0, s, x, count / 2,
                       reinterpret_cast<uint32_t*>(y), reinterpret_cast<uint32_t*>(y + yLo), g_errWord);
    e = hipGetLastError();
  }
  return op_done(e, s, 0, &range, rangeOut);
}

}  // extern "C"
