// int8 tier of model B (SURVEY.md section 8 row f4; included at the end of unet_hip.cpp): host side of the
// unet_i8_* entry points and the calibration pass of the float tier.  Kernels: conv_i8.h; quantisation scheme:
// unet_lane_detection_amd/quant.py; integer oracle: oracle/int8_oracle.py (HIP must match it bit for bit).

namespace {

struct I8Unit {
  std::string key;
  int taps = 9;          // 9: conv3x3, 1: transposed conv (scatter) or the first layer (im2col rows)
  int pair = 0;          // conv3x3 on a 32-byte pixel stride: two taps per K = 64 step (conv_i8.h), packed as 5 "taps"
  int scatter = 0;
  int cinReal = 0, cinPad = 0, coutReal = 0, coutPad = 0, colsPad = 0, cols = 0;
  int xzp = 0, yzp = 0, relu = 0;
  int8_t* wt = nullptr;
  int32_t *c0 = nullptr, *wzp = nullptr;
  float* mult = nullptr;
  // hybrid unit (quant.py, "hybrid quantisation"; conv_h16.h): fp16 weights in fragment order, m and b per column
  bool hyb = false, in16 = false, out16 = false, narrow = false;
  int cinStage = 0, chunks = 0;
  float yscale = 1.f;
  uint16_t* wh = nullptr;
  float *hm = nullptr, *hb = nullptr;
  void free_dev() {
    for (void* p : {(void*)wt, (void*)c0, (void*)wzp, (void*)mult, (void*)wh, (void*)hm, (void*)hb})
      if (p) hipFree(p);
    wt = nullptr;
    c0 = wzp = nullptr;
    mult = hm = hb = nullptr;
    wh = nullptr;
  }
};

struct I8Tensor {
  int c = 0, ld = 0;      // real channels, pixel stride in elements (multiple of 64, or 32)
  int level = 0;          // spatial size = input >> level
  int f16 = 0;            // elements are fp16 (every unit that writes or reads the tensor is hybrid), two bytes each
  size_t off = 0;         // byte offset in the workspace
};

}  // namespace

struct unet_i8_ctx {
  int depth = 0, device = 0;
  std::vector<int> features;
  std::map<std::string, std::vector<unsigned char>> arrays;
  bool finalized = false;
  std::vector<I8Unit> enc, bott, up, dec;
  I8Unit first;                      // encoder_blocks.0.0 on im2col rows
  int8_t* lut = nullptr;
  int zin = 0;
  int8_t* headW = nullptr;
  int headWzp = 0, headXzp = 0, headBias = 0;
  float headMult = 0.f;
  // hybrid quantisation: honoured unless unet_i8_set_hybrid(h, 0); which tensors are fp16 (by name, cat<l>.pool as cat<l>)
  bool hybridOn = true;
  std::map<std::string, int> f16Tensor;
  bool headHyb = false;
  uint16_t* headWh = nullptr;
  float headM = 0.f, headB = 0.f;
  // classes of the head: 0 until unet_i8_finalize has read output.bias_q, 1 the single-class head (the scalars above), K >= 2
  // the K-class head (i8_classes_kernels.h) with one entry per row in the device arrays below
  int classes = 0;
  int32_t *headWzpK = nullptr, *headBiasK = nullptr;
  float *headMultK = nullptr, *headMK = nullptr, *headBK = nullptr;
  void free_head() {
    for (void* p : {(void*)headW, (void*)headWh, (void*)headWzpK, (void*)headBiasK, (void*)headMultK, (void*)headMK, (void*)headBK})
      if (p) hipFree(p);
    headW = nullptr;
    headWh = nullptr;
    headWzpK = headBiasK = nullptr;
    headMultK = headMK = headBK = nullptr;
  }
  std::map<std::string, I8Tensor> tensors;   // by name, incl. "im2col"
  GrowBuf ws;
  int wsN = 0, wsH = 0, wsW = 0;
  std::string err;
  void free_all() {
    for (auto* v : {&enc, &bott, &up, &dec})
      for (auto& u : *v) u.free_dev();
    first.free_dev();
    if (lut) hipFree(lut);
    free_head();
    ws.release();
    lut = nullptr;
  }
};

namespace {

template <class T>
bool i8_get(unet_i8_ctx* h, const std::string& name, std::vector<T>& out, size_t expect) {
  auto it = h->arrays.find(name);
  if (it == h->arrays.end()) {
    h->err = "missing array " + name;
    return false;
  }
  if (it->second.size() != expect * sizeof(T)) {
    h->err = name + ": expected " + std::to_string(expect * sizeof(T)) + " bytes, got " + std::to_string(it->second.size());
    return false;
  }
  out.resize(expect);
  std::memcpy(out.data(), it->second.data(), expect * sizeof(T));
  return true;
}

template <class T>
int i8_upload(std::string& err, T** dst, const std::vector<T>& v) {
  HIPCHK(err, hipMalloc((void**)dst, std::max<size_t>(v.size(), 1) * sizeof(T)));
  HIPCHK(err, hipMemcpy(*dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return UNET_OK;
}

// Pack one unit.  W(k, col) gives the int8 weight of GEMM row k (< kReal) and column col (< colsReal); padded rows hold
// the column's zero point (they contribute exactly 0), padded columns are all zero with zero point 0.
template <class F>
int i8_build_unit(unet_i8_ctx* h, I8Unit& u, int taps, int kRealPerTap, int kPadPerTap, int colsReal, int colsPad, F&& W,
                  const std::vector<int32_t>& wzpCol, const std::vector<int32_t>& biasCol,
                  const std::vector<float>& multCol) {
  const int nCt = colsPad / 64, nCh = kPadPerTap / 64;
  std::vector<int8_t> packed((size_t)nCt * nCh * taps * 4 * 64 * 16, 0);
  std::vector<int32_t> c0(colsPad, 0), wz(colsPad, 0);
  std::vector<float> mu(colsPad, 0.f);
  std::vector<int64_t> sw(colsPad, 0);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < nCh; ++kc)
      for (int t = 0; t < taps; ++t)
        for (int cs = 0; cs < 4; ++cs) {
          int8_t* dst = packed.data() + ((((size_t)ct * nCh + kc) * taps + t) * 4 + cs) * 64 * 16;
          for (int lane = 0; lane < 64; ++lane) {
            const int j = lane & 15, lq = lane >> 4;
            const int col = 64 * ct + 16 * (j >> 2) + 4 * cs + (j & 3);
            for (int e = 0; e < 16; ++e) {
              const int k = kc * 64 + lq * 16 + e;
              int v = 0;
              if (col < colsReal) v = k < kRealPerTap ? (int)W(t, k, col) : wzpCol[col];
              dst[lane * 16 + e] = (int8_t)v;
              sw[col] += v;
            }
          }
        }
  const long K = (long)taps * kPadPerTap;
  for (int col = 0; col < colsReal; ++col) {
    wz[col] = wzpCol[col];
    mu[col] = multCol[col];
    c0[col] = (int32_t)((int64_t)biasCol[col] + (int64_t)K * u.xzp * wzpCol[col] - (int64_t)u.xzp * sw[col]);
  }
  u.taps = taps;
  u.colsPad = colsPad;
  int rc = i8_upload(h->err, &u.wt, packed);
  if (!rc) rc = i8_upload(h->err, &u.c0, c0);
  if (!rc) rc = i8_upload(h->err, &u.wzp, wz);
  if (!rc) rc = i8_upload(h->err, &u.mult, mu);
  return rc;
}

// conv3x3 unit `key` (state_dict prefix + conv index): input cinReal channels at stride cinPad
int i8_build_conv(unet_i8_ctx* h, I8Unit& u, const std::string& key, int cinReal, int cinPad, int cout, bool firstLayer) {
  u.free_dev();
  u.key = key;
  u.cinReal = cinReal;
  u.cinPad = cinPad;
  u.coutReal = cout;
  u.coutPad = round_up(cout, 64);
  u.cols = cout;
  std::vector<int8_t> wq;
  std::vector<int32_t> wzp, bias, s1;
  std::vector<float> mult;
  if (!i8_get(h, key + ".w_q", wq, (size_t)cout * cinReal * 9) || !i8_get(h, key + ".w_zp", wzp, cout) ||
      !i8_get(h, key + ".bias_q", bias, cout) || !i8_get(h, key + ".mult", mult, cout))
    return UNET_ERR_STATE;
  if (!i8_get(h, key + ".x_zp", s1, 1)) return UNET_ERR_STATE;
  u.xzp = s1[0];
  if (!i8_get(h, key + ".y_zp", s1, 1)) return UNET_ERR_STATE;
  u.yzp = s1[0];
  if (!i8_get(h, key + ".relu", s1, 1)) return UNET_ERR_STATE;
  u.relu = s1[0];
  u.scatter = 0;
  u.pair = 0;
  if (firstLayer)   // one "tap" over 64-byte im2col rows: k = tap*3 + ci
    return i8_build_unit(h, u, 1, 27, 64, cout, u.coutPad,
                         [&](int, int k, int col) { return wq[((size_t)col * 3 + (k % 3)) * 9 + k / 3]; }, wzp, bias, mult);
  if (cinPad == 32) {   // two taps per step: rows 0..31 = tap 2s, rows 32..63 = tap 2s + 1 (step 4: padding = zw)
    u.pair = 1;
    const int rc = i8_build_unit(h, u, 5, 64, 64, cout, u.coutPad,
                                 [&](int sN, int k, int col) -> int {
                                   const int t = 2 * sN + k / 32, ci = k % 32;
                                   return (t < 9 && ci < cinReal) ? (int)wq[((size_t)col * cinReal + ci) * 9 + t] : wzp[col];
                                 },
                                 wzp, bias, mult);
    u.taps = 9;   // still the 3x3 kernel
    return rc;
  }
  return i8_build_unit(h, u, 9, cinReal, cinPad, cout, u.coutPad,
                       [&](int t, int k, int col) { return wq[((size_t)col * cinReal + k) * 9 + t]; }, wzp, bias, mult);
}

// transposed conv: w_q (I,O,2,2); GEMM columns n = ab * coutPad + co
int i8_build_upconv(unet_i8_ctx* h, I8Unit& u, const std::string& key, int cinReal, int cinPad, int cout) {
  u.free_dev();
  u.key = key;
  u.cinReal = cinReal;
  u.cinPad = cinPad;
  u.coutReal = cout;
  u.coutPad = round_up(cout, 64);
  u.cols = 4 * u.coutPad;
  u.scatter = 1;
  std::vector<int8_t> wq;
  std::vector<int32_t> wzp, bias, s1;
  std::vector<float> mult;
  if (!i8_get(h, key + ".w_q", wq, (size_t)cinReal * cout * 4) || !i8_get(h, key + ".w_zp", wzp, cout) ||
      !i8_get(h, key + ".bias_q", bias, cout) || !i8_get(h, key + ".mult", mult, cout))
    return UNET_ERR_STATE;
  if (!i8_get(h, key + ".x_zp", s1, 1)) return UNET_ERR_STATE;
  u.xzp = s1[0];
  if (!i8_get(h, key + ".y_zp", s1, 1)) return UNET_ERR_STATE;
  u.yzp = s1[0];
  u.relu = 0;
  const int cp = u.coutPad, colsReal = 4 * cp;
  std::vector<int32_t> wzc(colsReal, 0), bc(colsReal, 0);
  std::vector<float> mc(colsReal, 0.f);
  for (int n = 0; n < colsReal; ++n) {
    const int co = n % cp;
    if (co < cout) {
      wzc[n] = wzp[co];
      bc[n] = bias[co];
      mc[n] = mult[co];
    }
  }
  return i8_build_unit(h, u, 1, cinReal, cinPad, colsReal, colsReal,
                       [&](int, int k, int n) -> int {
                         const int ab = n / cp, co = n % cp;
                         return co < cout ? (int)wq[((size_t)k * cout + co) * 4 + ab] : 0;
                       },
                       wzc, bc, mc);
}

// ---- hybrid units (quant.py, "hybrid quantisation"; kernels: conv_h16.h) ----
bool i8_unit_hybrid(const unet_i8_ctx* h, const std::string& key) {
  if (!h->hybridOn) return false;
  auto it = h->arrays.find(key + ".hybrid");
  if (it == h->arrays.end() || it->second.size() != sizeof(int32_t)) return false;
  int32_t v = 0;
  std::memcpy(&v, it->second.data(), sizeof(v));
  return v != 0;
}

// A tensor is fp16 iff every unit that writes it and every unit that reads it is hybrid (quant.tensor_dtypes states the
// same rule); cat<l>.pool goes with cat<l>; the input is always int8.
void i8_derive_dtypes(unet_i8_ctx* h) {
  const int d = h->depth;
  std::map<std::string, bool> all;
  auto use = [&](const std::string& key, const std::string& x, const std::string& y) {
    const bool hy = i8_unit_hybrid(h, key);
    for (const std::string* t : {&x, &y})
      if (!t->empty()) {
        auto it = all.find(*t);
        if (it == all.end())
          all[*t] = hy;
        else
          it->second = it->second && hy;
      }
  };
  for (int l = 0; l < d; ++l) {
    const std::string p = "encoder_blocks." + std::to_string(l), ea = "enc" + std::to_string(l) + ".a";
    use(p + ".0", l == 0 ? std::string("input") : "cat" + std::to_string(l - 1), ea);
    use(p + ".3", ea, "cat" + std::to_string(l));
  }
  use("bottleneck.0", "cat" + std::to_string(d - 1), "bott.a");
  use("bottleneck.3", "bott.a", "bott.b");
  for (int j = 0; j < d; ++j) {
    const std::string cat = "cat" + std::to_string(d - 1 - j), dj = "dec" + std::to_string(j);
    use("decoder_blocks." + std::to_string(2 * j), j == 0 ? std::string("bott.b") : "dec" + std::to_string(j - 1) + ".b", cat);
    use("decoder_blocks." + std::to_string(2 * j + 1) + ".0", cat, dj + ".a");
    use("decoder_blocks." + std::to_string(2 * j + 1) + ".3", dj + ".a", dj + ".b");
  }
  use("output", "dec" + std::to_string(d - 1) + ".b", "");
  all["input"] = false;
  h->f16Tensor.clear();
  for (auto& kv : all) h->f16Tensor[kv.first] = kv.second ? 1 : 0;
  for (int l = 0; l < d; ++l) h->f16Tensor["cat" + std::to_string(l) + ".pool"] = h->f16Tensor["cat" + std::to_string(l)];
  h->f16Tensor["im2col"] = 0;
}

// Pack one hybrid unit.  W(t, k, col) gives the fp16 bits of the weight of tap t, GEMM row k (< kReal) and column col
// (< colsReal); everything padded is +0.  Fragment order of conv_h16.h: [coTile][chunk][tap][kstep][cs][lane][8], with four
// subtiles cs per 64-column tile, or - a plain unit of <= 32 columns (u.narrow) - two per 32-column tile.
template <class F>
int h16_build_unit(unet_i8_ctx* h, I8Unit& u, int taps, int kReal, int colsReal, int colsPad, F&& W,
                   const std::vector<float>& mCol, const std::vector<float>& bCol) {
  u.cinStage = round_up(kReal, 8);
  u.chunks = (u.cinStage + 63) / 64;
  u.narrow = !u.scatter && colsReal <= 32;
  const int nCt = colsPad / 64, ncs = u.narrow ? 2 : 4;
  std::vector<uint16_t> packed((size_t)nCt * u.chunks * taps * 2 * ncs * 64 * 8, 0);
  for (int ct = 0; ct < nCt; ++ct)
    for (int kc = 0; kc < u.chunks; ++kc)
      for (int t = 0; t < taps; ++t)
        for (int ks = 0; ks < 2; ++ks)
          for (int cs = 0; cs < ncs; ++cs) {
            uint16_t* dst = packed.data() + (((((size_t)ct * u.chunks + kc) * taps + t) * 2 + ks) * ncs + cs) * 64 * 8;
            for (int lane = 0; lane < 64; ++lane) {
              const int j = lane & 15, lq = lane >> 4;
              const int col = 64 * ct + 4 * ncs * (j >> 2) + 4 * cs + (j & 3);
              for (int e = 0; e < 8; ++e) {
                const int k = kc * 64 + ks * 32 + lq * 8 + e;
                if (col < colsReal && k < kReal) dst[lane * 8 + e] = W(t, k, col);
              }
            }
          }
  std::vector<float> m(colsPad, 0.f), b(colsPad, 0.f);
  for (int col = 0; col < colsReal; ++col) {
    m[col] = mCol[col];
    b[col] = bCol[col];
  }
  u.taps = taps;
  u.colsPad = colsPad;
  u.hyb = true;
  int rc = i8_upload(h->err, &u.wh, packed);
  if (!rc) rc = i8_upload(h->err, &u.hm, m);
  if (!rc) rc = i8_upload(h->err, &u.hb, b);
  return rc;
}

// the arrays every hybrid unit carries: gain (x x_scale for an int8 input) and bias per output channel, zero points, scales
int h16_get_common(unet_i8_ctx* h, I8Unit& u, const std::string& key, int cout, bool hasOut, std::vector<float>& m,
                   std::vector<float>& b) {
  std::vector<int32_t> s1;
  std::vector<float> f1;
  if (!i8_get(h, key + ".gain", m, cout) || !i8_get(h, key + ".bias_f", b, cout) || !i8_get(h, key + ".x_scale", f1, 1))
    return UNET_ERR_STATE;
  if (!u.in16)
    for (auto& v : m) v *= f1[0];   // a power of two times a float: exact
  if (!i8_get(h, key + ".x_zp", s1, 1)) return UNET_ERR_STATE;
  u.xzp = s1[0];
  u.yzp = 0;
  u.yscale = 1.f;
  if (hasOut) {
    if (!i8_get(h, key + ".y_zp", s1, 1) || !i8_get(h, key + ".y_scale", f1, 1)) return UNET_ERR_STATE;
    u.yzp = s1[0];
    u.yscale = f1[0];
  }
  return UNET_OK;
}

int h16_build_conv(unet_i8_ctx* h, I8Unit& u, const std::string& key, int cinReal, int cout, bool firstLayer, bool in16,
                   bool out16) {
  u.free_dev();
  u.key = key;
  u.cinReal = cinReal;
  u.coutReal = cout;
  u.coutPad = round_up(cout, 64);
  u.cols = cout;
  u.scatter = 0;
  u.pair = 0;
  u.in16 = in16;
  u.out16 = out16;
  std::vector<uint16_t> wh;
  std::vector<float> m, b;
  std::vector<int32_t> s1;
  if (!i8_get(h, key + ".w_h", wh, (size_t)cout * cinReal * 9)) return UNET_ERR_STATE;
  if (const int rc = h16_get_common(h, u, key, cout, true, m, b)) return rc;
  if (!i8_get(h, key + ".relu", s1, 1)) return UNET_ERR_STATE;
  u.relu = s1[0];
  if (firstLayer)   // one "tap" over the im2col rows: k = tap*3 + ci
    return h16_build_unit(h, u, 1, 27, cout, u.coutPad,
                          [&](int, int k, int col) { return wh[((size_t)col * 3 + (k % 3)) * 9 + k / 3]; }, m, b);
  return h16_build_unit(h, u, 9, cinReal, cout, u.coutPad,
                        [&](int t, int k, int col) { return wh[((size_t)col * cinReal + k) * 9 + t]; }, m, b);
}

// transposed conv: w_h (I,O,2,2); GEMM columns n = ab * coutPad + co
int h16_build_upconv(unet_i8_ctx* h, I8Unit& u, const std::string& key, int cinReal, int cout, bool in16, bool out16) {
  u.free_dev();
  u.key = key;
  u.cinReal = cinReal;
  u.coutReal = cout;
  u.coutPad = round_up(cout, 64);
  u.cols = 4 * u.coutPad;
  u.scatter = 1;
  u.pair = 0;
  u.relu = 0;
  u.in16 = in16;
  u.out16 = out16;
  std::vector<uint16_t> wh;
  std::vector<float> m, b;
  if (!i8_get(h, key + ".w_h", wh, (size_t)cinReal * cout * 4)) return UNET_ERR_STATE;
  if (const int rc = h16_get_common(h, u, key, cout, true, m, b)) return rc;
  const int cp = u.coutPad, colsReal = 4 * cp;
  std::vector<float> mc(colsReal, 0.f), bc(colsReal, 0.f);
  for (int n = 0; n < colsReal; ++n)
    if (n % cp < cout) {
      mc[n] = m[n % cp];
      bc[n] = b[n % cp];
    }
  return h16_build_unit(h, u, 1, cinReal, colsReal, colsReal,
                        [&](int, int k, int n) -> uint16_t {
                          const int ab = n / cp, co = n % cp;
                          return co < cout ? wh[((size_t)k * cout + co) * 4 + ab] : (uint16_t)0;
                        },
                        mc, bc);
}

hipError_t h16_run(const I8Unit& u, const void* in, int ldi, int n, int hh, int ww, void* out, int ldo, int coOff, hipStream_t s) {
  unet::ConvH16Args a = {};
  a.in = in;
  a.wt = u.wh;
  a.mult = u.hm;
  a.bias = u.hb;
  a.out = out;
  a.N = n;
  a.H = hh;
  a.W = ww;
  a.ldi = ldi;
  a.ldo = ldo;
  a.co_off = coOff;
  a.cinStage = u.cinStage;
  a.chunks = u.chunks;
  a.cols = u.cols;
  a.coutReal = u.coutReal;
  a.coutPad = u.coutPad;
  a.xzp = u.xzp;
  a.yzp = u.yzp;
  a.lo = u.relu ? u.yzp : -128;
  a.relu = u.relu;
  a.scatter = u.scatter;
  a.narrow = u.narrow;
  a.yscale = u.yscale;
  const double px = (double)n * hh * ww;
  const double k = u.taps == 9 ? 9.0 * u.cinReal : (u.scatter ? 4.0 * u.cinReal : 27.0);
  prof_begin(u.taps == 9 ? "conv3x3_h16" : (u.scatter ? "upconv2x2_h16" : "conv3x3_first_h16"), 2.0 * px * k * u.coutReal,
             px * ((u.in16 ? 2.0 : 1.0) * (u.taps == 9 || u.scatter ? u.cinReal : 64) +
                   (u.out16 ? 2.0 : 1.0) * (u.scatter ? 4.0 : 1.0) * u.coutReal), s);
  const hipError_t e = unet::launch_conv_h16(a, u.taps, u.in16, u.out16, s);
  prof_end(s);
  return e;
}

int i8_plan(unet_i8_ctx* h, int n, int height, int width) {
  h->tensors.clear();
  size_t off = 0;
  auto add = [&](const std::string& name, int c, int level, bool feedsUpconv = false) {
    I8Tensor t;
    t.c = c;
    // narrow tensors keep a 32-byte pixel stride (pair mode of the 3x3 kernel); the 1x1 kernel behind the transposed
    // convolutions needs 64-byte rows
    t.ld = (c <= 32 && !feedsUpconv) ? 32 : round_up(c, 64);
    t.level = level;
    t.off = off;
    auto dt = h->f16Tensor.find(name);
    t.f16 = dt != h->f16Tensor.end() ? dt->second : 0;   // an fp16 tensor: the same stride in elements, two bytes each
    off += (((size_t)n * (height >> level) * (width >> level) * t.ld * (t.f16 ? 2 : 1)) + 255) / 256 * 256;
    h->tensors[name] = t;
  };
  const int d = h->depth;
  add("im2col", 64, 0);
  for (int l = 0; l < d; ++l) {
    add("enc" + std::to_string(l) + ".a", h->features[l], l);
    add("cat" + std::to_string(l), 2 * h->features[l], l);
    add("cat" + std::to_string(l) + ".pool", h->features[l], l + 1);
  }
  add("bott.a", 2 * h->features[d - 1], d);
  add("bott.b", 2 * h->features[d - 1], d, true);
  for (int j = 0; j < d; ++j) {
    const int l = d - 1 - j;
    add("dec" + std::to_string(j) + ".a", h->features[l], l);
    add("dec" + std::to_string(j) + ".b", h->features[l], l, j + 1 < d);
  }
  h->wsN = n;
  h->wsH = height;
  h->wsW = width;
  if (off <= h->ws.bytes) return UNET_OK;
  const int rc = h->ws.reserve(h->err, off, "int8 workspace");
  if (!rc) hipMemset(h->ws.p, 0, off);   // padded channels are never written; they are multiplied by zero either way
  return rc;
}

// scratch page of the current device for the lanes of conv_i8_lw_kernel that have nothing to store
int8_t* i8_dump_page() {
  static int8_t* page[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!page[dev] && hipMalloc((void**)&page[dev], 65536) != hipSuccess) return nullptr;
  return page[dev];
}

// UNET_I8_LW=0: the narrow layers on conv_i8_kernel as well (A/B measurements; bit-identical)
bool i8_lw_enabled() {
  static const bool on = [] {
    const char* e = getenv("UNET_I8_LW");
    return !(e && e[0] == '0');
  }();
  return on;
}

hipError_t i8_run(const I8Unit& u, const int8_t* in, int n, int hh, int ww, int8_t* out, int ldo, int coOff, hipStream_t s) {
  unet::ConvI8Args a;
  a.dump = i8_dump_page();
  if (!a.dump) return hipErrorOutOfMemory;
  a.in = in;
  a.wt = u.wt;
  a.c0 = u.c0;
  a.wzp = u.wzp;
  a.mult = u.mult;
  a.out = out;
  a.N = n;
  a.H = hh;
  a.W = ww;
  a.Cin = u.taps == 9 ? u.cinPad : (u.scatter ? u.cinPad : 64);
  a.ldo = ldo;
  a.co_off = coOff;
  a.cols = u.cols;
  a.coutReal = u.coutReal;
  a.coutPad = u.coutPad;
  a.xzp = u.xzp;
  a.yzp = u.yzp;
  a.lo = u.relu ? u.yzp : -128;
  a.scatter = u.scatter;
  a.pair = u.pair;
  a.coTiles = u.colsPad / 64;
  const double px = (double)n * hh * ww;
  if ((long)n * hh * ww * 4 >= (1L << 31) || ww >= (1 << 23)) return hipErrorInvalidValue;   // 32-bit pixel indices (x 4: scatter)
  // persistent blocks: six per CU over all channel tiles (conv_i8.h), never more than there are pixel tiles.  Two or three are
  // resident (their registers); the rest queue up and even out the tail (profiles/r04/int8_blocks_per_cu_sweep.txt: 2 / 3 /
  // 4 / 6 / 8 per CU: 5.81 / 5.83 / 5.82 / 5.67 / - ms per step with the narrow layers' kernel, 6.8 / 6.7 / 6.9 / 6.45 / 6.6 before)
  auto tile_blocks = [&](int pixTiles, int perCu) {
    static const int forced = [] {   // UNET_I8_BLOCKS_PER_CU: A/B measurements
      const char* e = getenv("UNET_I8_BLOCKS_PER_CU");
      return e ? atoi(e) : 0;
    }();
    if (forced > 0) perCu = forced;
    return std::max(1, std::min(pixTiles, 256 * perCu / std::max(1, a.coTiles)));
  };
  // (MS = 4, 16 x 16-pixel tiles, was measured for the narrow layers: 0 - 15 % slower, conv_i8.h)
  if (u.taps == 9) {
    a.tilesX = (ww + 15) / 16;
    a.tilesY = (hh + 7) / 8;
    a.pixTiles = n * a.tilesY * a.tilesX;
    a.tileBlocks = tile_blocks(a.pixTiles, 6);
    const size_t lds = (size_t)10 * 18 * unet::conv_i8_pitch(a.Cin) + 768;
    const dim3 grid((unsigned)((size_t)a.tileBlocks * a.coTiles));
    if (a.Cin > 256) return hipErrorInvalidValue;   // (LDS: 10 x 18 pixels x (Cin + 32) bytes must stay below 64 KiB)
    prof_begin("conv3x3_i8", 2.0 * px * 9 * u.cinReal * u.coutReal, px * (u.cinReal + u.coutReal), s);
    const bool lw = i8_lw_enabled() && (u.pair || a.Cin == 64);   // the narrow layers' kernel: weights in LDS behind the tile
    const size_t ldsLw = lds + (size_t)(u.pair ? 5 : 9) * 4096;
    if (lw && u.pair)
      hipLaunchKernelGGL((unet::conv_i8_lw_kernel<9, true, 2>), grid, dim3(256), ldsLw, s, a);
    else if (lw)
      hipLaunchKernelGGL((unet::conv_i8_lw_kernel<9, false, 3>), grid, dim3(256), ldsLw, s, a);
    else if (u.pair)
      hipLaunchKernelGGL((unet::conv_i8_kernel<9, true, 2, 2>), grid, dim3(256), lds, s, a);
    else if (a.Cin <= 64)
      hipLaunchKernelGGL((unet::conv_i8_kernel<9, false, 3, 2>), grid, dim3(256), lds, s, a);
    else
      hipLaunchKernelGGL((unet::conv_i8_kernel<9, false, 6, 2>), grid, dim3(256), lds, s, a);
  } else {
    a.tilesX = a.tilesY = 0;
    a.pixTiles = (int)(((long)n * hh * ww + 127) / 128);
    a.tileBlocks = tile_blocks(a.pixTiles, 6);
    const size_t lds = (size_t)128 * unet::conv_i8_pitch(a.Cin) + 768;
    const dim3 grid((unsigned)((size_t)a.tileBlocks * a.coTiles));
    if (a.Cin > 448) return hipErrorInvalidValue;   // (LDS: 128 pixels x (Cin + 32) bytes below 64 KiB)
    prof_begin(u.scatter ? "upconv2x2_i8" : "conv3x3_first_i8", 2.0 * px * (u.scatter ? u.cinReal * 4.0 : 27.0) * u.coutReal,
               px * (u.scatter ? u.cinReal + 4.0 * u.coutReal : 64.0 + u.coutReal), s);
    if (i8_lw_enabled() && a.Cin == 64 && !u.scatter)   // (the transposed convolution's scatter stores: 10 % slower there)
      hipLaunchKernelGGL((unet::conv_i8_lw_kernel<1, false, 2>), grid, dim3(256), lds + 4096, s, a);
    else if (a.Cin <= 64)
      hipLaunchKernelGGL((unet::conv_i8_kernel<1, false, 2, 2>), grid, dim3(256), lds, s, a);
    else
      hipLaunchKernelGGL((unet::conv_i8_kernel<1, false, 6, 2>), grid, dim3(256), lds, s, a);
  }
  prof_end(s);
#if UNET_I8_STAMPS
  {
    hipStreamSynchronize(s);
    unsigned long long st[8] = {}, zero[8] = {};
    hipMemcpyFromSymbol(st, HIP_SYMBOL(unet::g_i8Stamps), sizeof(st));
    hipMemcpyToSymbol(HIP_SYMBOL(unet::g_i8Stamps), zero, sizeof(zero));
    const double t = st[6] ? (double)st[6] : 1.0;
    fprintf(stderr, "i8 stamps taps %d cin %3d cols %3d pair %d blocks %5d tiles %7llu | per tile (s_memtime ticks, 100 MHz): store %.1f bar1 %.1f pre %.1f "
            "loop %.1f epi %.1f bar2 %.1f | kernel per block %.0f\n", u.taps, a.Cin, a.cols, (int)u.pair, a.tileBlocks * a.coTiles, st[6],
            st[0] / t, st[1] / t, st[2] / t, st[3] / t, st[4] / t, st[5] / t, (double)st[7] / (a.tileBlocks * a.coTiles));
  }
#endif
  return hipGetLastError();
}

}  // namespace

extern "C" {

int unet_i8_create(int depth, const int* features, int device, unet_i8_handle_t* out) {
  if (!features || !out || depth < 1 || depth > UNET_MAX_DEPTH || device < 0) return UNET_ERR_INVALID_ARG;
  for (int i = 0; i < depth; ++i)
    if (features[i] <= 0 || features[i] % 16) return UNET_ERR_INVALID_ARG;
  for (int i = 0; i + 1 < depth; ++i)
    if (features[i + 1] != 2 * features[i]) return UNET_ERR_INVALID_ARG;
  if (2 * features[depth - 1] > 256) return UNET_ERR_INVALID_ARG;   // the staged input tile must fit LDS (<= 256 channels)
  auto* h = new unet_i8_ctx();
  h->depth = depth;
  h->device = device;
  h->features.assign(features, features + depth);
  *out = h;
  return UNET_OK;
}

int unet_i8_load(unet_i8_handle_t h, const char* name, const void* data, size_t bytes) {
  if (!h || !name || !data) return UNET_ERR_INVALID_ARG;
  auto& v = h->arrays[name];
  v.assign((const unsigned char*)data, (const unsigned char*)data + bytes);
  h->finalized = false;
  return UNET_OK;
}

int unet_i8_finalize(unet_i8_handle_t h) {
  if (!h) return UNET_ERR_INVALID_ARG;
  // the class count and the head's arrays: host work, settled before a device is touched
  h->classes = unet::i8_head_classes(h->arrays, h->features[0], i8_unit_hybrid(h, "output"), h->err);
  if (!h->classes) return UNET_ERR_STATE;
  const int K = h->classes;
  HIPCHK(h->err, hipSetDevice(h->device));
  const int d = h->depth;
  h->enc.assign(2 * d, I8Unit());
  h->dec.assign(2 * d, I8Unit());
  h->up.assign(d, I8Unit());
  h->bott.assign(2, I8Unit());
  int rc;
  auto pad = [](int c) { return c <= 32 ? 32 : round_up(c, 64); };   // = the pixel stride i8_plan gives a c-channel tensor
  // a hybrid unit (hybrid quantisation, quant.py) is packed for conv_h16.h instead; x, y: the tensors it reads and writes
  i8_derive_dtypes(h);
  h->wsN = h->wsH = h->wsW = 0;   // tensor types may have changed: the next forward plans again
  auto conv = [&](I8Unit& u, const std::string& key, int cinReal, int cinPad, int cout, bool firstLayer, const std::string& x,
                  const std::string& y) {
    if (i8_unit_hybrid(h, key)) return h16_build_conv(h, u, key, cinReal, cout, firstLayer, h->f16Tensor[x], h->f16Tensor[y]);
    u.hyb = false;
    return i8_build_conv(h, u, key, cinReal, cinPad, cout, firstLayer);
  };
  for (int l = 0; l < d; ++l) {
    const std::string p = "encoder_blocks." + std::to_string(l), ea = "enc" + std::to_string(l) + ".a";
    const int f = h->features[l];
    if (l == 0) {
      if ((rc = conv(h->enc[0], p + ".0", 3, 64, f, true, "input", ea))) return rc;
    } else {
      if ((rc = conv(h->enc[2 * l], p + ".0", h->features[l - 1], pad(h->features[l - 1]), f, false,
                     "cat" + std::to_string(l - 1), ea)))
        return rc;
    }
    if ((rc = conv(h->enc[2 * l + 1], p + ".3", f, pad(f), f, false, ea, "cat" + std::to_string(l)))) return rc;
  }
  const int fl = h->features[d - 1];
  if ((rc = conv(h->bott[0], "bottleneck.0", fl, pad(fl), 2 * fl, false, "cat" + std::to_string(d - 1), "bott.a"))) return rc;
  if ((rc = conv(h->bott[1], "bottleneck.3", 2 * fl, pad(2 * fl), 2 * fl, false, "bott.a", "bott.b"))) return rc;
  for (int j = 0; j < d; ++j) {
    const int f = h->features[d - 1 - j];
    const std::string cat = "cat" + std::to_string(d - 1 - j), dj = "dec" + std::to_string(j);
    const std::string src = j == 0 ? std::string("bott.b") : "dec" + std::to_string(j - 1) + ".b";
    const std::string uk = "decoder_blocks." + std::to_string(2 * j);
    if (i8_unit_hybrid(h, uk))
      rc = h16_build_upconv(h, h->up[j], uk, 2 * f, f, h->f16Tensor[src], h->f16Tensor[cat]);
    else
      rc = i8_build_upconv(h, h->up[j], uk, 2 * f, round_up(2 * f, 64), f);
    if (rc) return rc;
    const std::string p = "decoder_blocks." + std::to_string(2 * j + 1);
    if ((rc = conv(h->dec[2 * j], p + ".0", 2 * f, pad(2 * f), f, false, cat, dj + ".a"))) return rc;
    if ((rc = conv(h->dec[2 * j + 1], p + ".3", f, pad(f), f, false, dj + ".a", dj + ".b"))) return rc;
  }
  h->headHyb = i8_unit_hybrid(h, "output");
  h->free_head();
  const size_t c0 = (size_t)h->features[0];
  if (h->headHyb) {
    I8Unit hu;
    hu.in16 = h->f16Tensor["dec" + std::to_string(d - 1) + ".b"];
    std::vector<uint16_t> wh;
    std::vector<float> m, b;
    if (!i8_get(h, "output.w_h", wh, K * c0)) return UNET_ERR_STATE;
    if ((rc = h16_get_common(h, hu, "output", K, false, m, b))) return rc;
    h->headM = m[0];
    h->headB = b[0];
    if ((rc = i8_upload(h->err, &h->headWh, wh))) return rc;
    if (K > 1 && ((rc = i8_upload(h->err, &h->headMK, m)) || (rc = i8_upload(h->err, &h->headBK, b)))) return rc;
  }
  std::vector<int8_t> lut, hw;
  std::vector<int32_t> s1, wzpK, biasK;
  std::vector<float> multK;
  if (!i8_get(h, "input.lut", lut, 768) || !i8_get(h, "input.zp", s1, 1)) return UNET_ERR_STATE;
  h->zin = s1[0];
  if (h->lut) hipFree(h->lut);
  h->lut = nullptr;
  if ((rc = i8_upload(h->err, &h->lut, lut))) return rc;
  if (!i8_get(h, "output.w_q", hw, K * c0) || !i8_get(h, "output.w_zp", wzpK, K)) return UNET_ERR_STATE;
  h->headWzp = wzpK[0];
  if (!i8_get(h, "output.x_zp", s1, 1)) return UNET_ERR_STATE;
  h->headXzp = s1[0];
  if (!i8_get(h, "output.bias_q", biasK, K)) return UNET_ERR_STATE;
  h->headBias = biasK[0];
  if (!i8_get(h, "output.mult", multK, K)) return UNET_ERR_STATE;
  h->headMult = multK[0];
  if ((rc = i8_upload(h->err, &h->headW, hw))) return rc;
  if (K > 1 && ((rc = i8_upload(h->err, &h->headWzpK, wzpK)) || (rc = i8_upload(h->err, &h->headBiasK, biasK)) ||
                (rc = i8_upload(h->err, &h->headMultK, multK))))
    return rc;
  h->finalized = true;
  return UNET_OK;
}

// what the head of one forward writes: the single-class outputs, or those of the K-class head
struct I8HeadOut {
  float* logits = nullptr;
  float* probs = nullptr;
  uint8_t* mask = nullptr;
  float thr = 0.f;
  uint8_t* labels = nullptr;
  int maskClass = 0;
};

// the head on tensor `cur` of the last forward: head_i8_kernel / head_h16_kernel of a single-class model, the K-class
// kernels of i8_classes_kernels.h otherwise
static int i8_run_head(unet_i8_ctx* h, const I8Tensor& cur, size_t npix, size_t hw, const I8HeadOut& o, hipStream_t s) {
  const int8_t* x = reinterpret_cast<const int8_t*>(h->ws.p + cur.off);
  if (h->classes > 1) {
    unet::HeadKI8Args a = {};
    a.x = x;
    a.ld = cur.ld;
    a.C = h->features[0];
    a.K = h->classes;
    a.npix = npix;
    a.hw = hw;
    a.xzp = h->headXzp;
    a.w = h->headW;
    a.wzp = h->headWzpK;
    a.bias = h->headBiasK;
    a.mult = h->headMultK;
    a.wh = h->headWh;
    a.hm = h->headMK;
    a.hb = h->headBK;
    a.logits = o.logits;
    a.probs = o.probs;
    a.labels = o.labels;
    a.mask = o.mask;
    a.maskClass = o.maskClass;
    HIPCHK(h->err, h->headHyb ? unet::launch_headk_h16(a, cur.f16, s) : unet::launch_headk_i8(a, s));
  } else if (h->headHyb) {
    HIPCHK(h->err, unet::launch_head_h16(x, cur.f16, cur.ld, h->features[0], npix, h->headWh, h->headXzp, h->headM, h->headB,
                                         o.logits, o.probs, o.mask, o.thr, s));
  } else {
    hipLaunchKernelGGL(unet::head_i8_kernel, dim3(grid_for(npix)), dim3(256), 0, s, x, cur.ld, h->features[0], npix, h->headW,
                       h->headWzp, h->headXzp, h->headBias, h->headMult, o.logits, o.probs, o.mask, o.thr);
    HIPCHK(h->err, hipGetLastError());
  }
  return UNET_OK;
}

// The refusals of a forward that need no device, in this order: the handle's kind (known once unet_i8_finalize has read
// the head), the outputs asked for (i8_classes_args), the handle's state (i8_state_gate).  wantClasses: the caller is a
// K-class entry point.
static int i8_kind_gate(unet_i8_ctx* h, const char* who, bool wantClasses) {
  if (h->classes && (h->classes > 1) != wantClasses) {
    h->err = std::string(who) +
             (wantClasses ? std::string(": this entry point serves a K-class model (2 or more entries in output.bias_q); the "
                                        "handle has the single-class head and runs unet_i8_forward_u8")
                          : ": this entry point serves the single-class head; a handle with " + std::to_string(h->classes) +
                                " classes runs unet_i8_forward_classes_u8");
    return UNET_ERR_INVALID_ARG;
  }
  return UNET_OK;
}

static int i8_state_gate(unet_i8_ctx* h) {
  if (h->finalized) return UNET_OK;
  h->err = "unet_i8_finalize has not been called";
  return UNET_ERR_STATE;
}

static int i8_forward(unet_i8_ctx* h, const uint8_t* frames, int n, int height, int width, const I8HeadOut& out, void* stream) {
  const int m = 1 << h->depth;
  if (n <= 0 || height <= 0 || width <= 0) return UNET_ERR_INVALID_ARG;
  if (height % m || width % m) {
    h->err = "H and W must be multiples of " + std::to_string(m);
    return UNET_ERR_SHAPE;
  }
  HIPCHK(h->err, hipSetDevice(h->device));
  if (n != h->wsN || height != h->wsH || width != h->wsW || !h->ws.p) {
    const int rc = i8_plan(h, n, height, width);
    if (rc) return rc;
  }
  hipStream_t s = (hipStream_t)stream;
  const int d = h->depth;
  auto T = [&](const std::string& name) -> const I8Tensor& { return h->tensors.at(name); };
  auto P = [&](const I8Tensor& t) { return reinterpret_cast<int8_t*>(h->ws.p + t.off); };
  const size_t npix = (size_t)n * height * width;
  hipLaunchKernelGGL(unet::im2col27_i8_kernel, dim3(grid_for(npix)), dim3(256), 0, s, frames, h->lut, n, height, width, h->zin,
                     P(T("im2col")));
  HIPCHK(h->err, hipGetLastError());
  int ch = height, cw = width;
  const I8Tensor* cur = nullptr;
  // one unit: the int8 kernels, or the fp16 kernels of a hybrid unit between tensors of either type (co_off in elements)
  auto run = [&](const I8Unit& u, const I8Tensor& x, int hh, int ww, const I8Tensor& y, int coOff) {
    return u.hyb ? h16_run(u, P(x), x.ld, n, hh, ww, P(y), y.ld, coOff, s) : i8_run(u, P(x), n, hh, ww, P(y), y.ld, coOff, s);
  };
  for (int l = 0; l < d; ++l) {
    const I8Tensor &ea = T("enc" + std::to_string(l) + ".a"), &cat = T("cat" + std::to_string(l)),
                   &pl = T("cat" + std::to_string(l) + ".pool");
    if (l == 0)
      HIPCHK(h->err, run(h->enc[0], T("im2col"), ch, cw, ea, 0));
    else
      HIPCHK(h->err, run(h->enc[2 * l], *cur, ch, cw, ea, 0));
    HIPCHK(h->err, run(h->enc[2 * l + 1], ea, ch, cw, cat, 0));   // skip half of the concat
    if (cat.f16) {
      HIPCHK(h->err, unet::launch_maxpool2x2_h16(reinterpret_cast<const uint16_t*>(P(cat)), n, ch, cw, h->features[l], cat.ld,
                                                 reinterpret_cast<uint16_t*>(P(pl)), pl.ld, s));
    } else {
      const size_t tot = (size_t)n * (ch / 2) * (cw / 2) * (h->features[l] / 16);
      hipLaunchKernelGGL(unet::maxpool2x2_i8_kernel, dim3(grid_for(tot)), dim3(256), 0, s, P(cat), n, ch, cw, h->features[l],
                         cat.ld, P(pl), pl.ld);
      HIPCHK(h->err, hipGetLastError());
    }
    cur = &pl;
    ch /= 2;
    cw /= 2;
  }
  HIPCHK(h->err, run(h->bott[0], *cur, ch, cw, T("bott.a"), 0));
  HIPCHK(h->err, run(h->bott[1], T("bott.a"), ch, cw, T("bott.b"), 0));
  cur = &T("bott.b");
  for (int j = 0; j < d; ++j) {
    const int l = d - 1 - j;
    const int f = h->features[l];
    const I8Tensor &cat = T("cat" + std::to_string(l)), &da = T("dec" + std::to_string(j) + ".a"),
                   &db = T("dec" + std::to_string(j) + ".b");
    HIPCHK(h->err, run(h->up[j], *cur, ch, cw, cat, f));   // upper half: cat([skip, x]) elided
    ch *= 2;
    cw *= 2;
    HIPCHK(h->err, run(h->dec[2 * j], cat, ch, cw, da, 0));
    HIPCHK(h->err, run(h->dec[2 * j + 1], da, ch, cw, db, 0));
    cur = &db;
  }
  return i8_run_head(h, *cur, npix, (size_t)height * width, out, s);
}

int unet_i8_forward_u8(unet_i8_handle_t h, const uint8_t* frames, int n, int height, int width, float* logits,
                       float* probs, uint8_t* mask, float thr, void* stream) {
  if (!h || !frames) return UNET_ERR_INVALID_ARG;
  int rc = i8_kind_gate(h, "unet_i8_forward_u8", false);
  if (!rc) rc = i8_state_gate(h);
  if (rc) return rc;
  I8HeadOut o;
  o.logits = logits, o.probs = probs, o.mask = mask, o.thr = thr;
  return i8_forward(h, frames, n, height, width, o, stream);
}

int unet_i8_out_channels(unet_i8_handle_t h) { return h ? h->classes : 0; }

// the checks of the K-class outputs that need no device
static int i8_classes_args(unet_i8_ctx* h, const char* who, const float* logits, const float* probs, const uint8_t* labels,
                           int maskClass, const uint8_t* mask) {
  if (!logits && !probs && !labels && !mask) {
    h->err = std::string(who) + ": no output asked for (logits, probs, labels and mask are all null)";
    return UNET_ERR_INVALID_ARG;
  }
  if (mask && h->classes && (maskClass < 0 || maskClass >= h->classes)) {
    h->err = std::string(who) + ": mask_class must name a class of the handle (0 .. " + std::to_string(h->classes - 1) + ")";
    return UNET_ERR_INVALID_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(probs)) % 16 ||
      (reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(mask)) % 4) {
    h->err = std::string(who) + ": logits and probs must be 16-byte aligned, labels and mask 4-byte aligned";
    return UNET_ERR_INVALID_ARG;
  }
  return UNET_OK;
}

int unet_i8_forward_classes_u8(unet_i8_handle_t h, const uint8_t* frames, int n, int height, int width, float* logits,
                               float* probs, uint8_t* labels, int maskClass, uint8_t* mask, void* stream) {
  if (!h || !frames) return UNET_ERR_INVALID_ARG;
  int rc = i8_kind_gate(h, "unet_i8_forward_classes_u8", true);
  if (!rc) rc = i8_classes_args(h, "unet_i8_forward_classes_u8", logits, probs, labels, maskClass, mask);
  if (!rc) rc = i8_state_gate(h);
  if (rc) return rc;
  I8HeadOut o;
  o.logits = logits, o.probs = probs, o.labels = labels, o.maskClass = maskClass, o.mask = mask;
  return i8_forward(h, frames, n, height, width, o, stream);
}

// The head alone, on the last tensor of the handle's last forward (its n, height, width): the outputs of unet_i8_forward_u8
// for a single-class handle (labels and mask_class unused), those of unet_i8_forward_classes_u8 otherwise (the threshold
// unused).  For timing the head and for comparing its output configurations with one another.
int unet_i8_run_head(unet_i8_handle_t h, float* logits, float* probs, uint8_t* labels, int maskClass, uint8_t* mask, float thr,
                     void* stream) {
  if (!h) return UNET_ERR_INVALID_ARG;
  if (!h->finalized || !h->ws.p || !h->wsN) {
    h->err = "unet_i8_run_head: no forward has run on this handle since unet_i8_finalize";
    return UNET_ERR_STATE;
  }
  if (h->classes > 1)
    if (int rc = i8_classes_args(h, "unet_i8_run_head", logits, probs, labels, maskClass, mask)) return rc;
  HIPCHK(h->err, hipSetDevice(h->device));
  I8HeadOut o;
  o.logits = logits, o.probs = probs, o.labels = labels, o.maskClass = maskClass, o.mask = mask, o.thr = thr;
  const I8Tensor& cur = h->tensors.at("dec" + std::to_string(h->depth - 1) + ".b");
  return i8_run_head(h, cur, (size_t)h->wsN * h->wsH * h->wsW, (size_t)h->wsH * h->wsW, o, (hipStream_t)stream);
}

// Copy one activation tensor of the last forward call to the host as dense NHWC int8 with its real channels
// (parity tests): name = "im2col", "enc<l>.a", "cat<l>", "cat<l>.pool", "bott.a", "bott.b", "dec<j>.a", "dec<j>.b".
int unet_i8_read_tensor(unet_i8_handle_t h, const char* name, int8_t* dstHost, size_t capBytes, int* channels) {
  if (!h || !name || !dstHost || !h->ws.p) return UNET_ERR_INVALID_ARG;
  auto it = h->tensors.find(name);
  if (it == h->tensors.end()) return UNET_ERR_UNKNOWN_PARAM;
  HIPCHK(h->err, hipSetDevice(h->device));
  HIPCHK(h->err, hipDeviceSynchronize());
  const I8Tensor& t = it->second;
  if (t.f16) {
    h->err = std::string(name) + " is an fp16 tensor of a hybrid model: unet_i8_read_tensor_f16 reads it";
    return UNET_ERR_INVALID_ARG;
  }
  const size_t px = (size_t)h->wsN * (h->wsH >> t.level) * (h->wsW >> t.level);
  if (capBytes < px * t.c) return UNET_ERR_INVALID_ARG;
  if (channels) *channels = t.c;
  HIPCHK(h->err, hipMemcpy2D(dstHost, t.c, h->ws.p + t.off, t.ld, t.c, px, hipMemcpyDeviceToHost));
  return UNET_OK;
}

// The fp16 twin: dense NHWC fp16 bits of a tensor that unet_i8_tensor_dtype reports as fp16 (UNET_ERR_INVALID_ARG for an
// int8 tensor).
int unet_i8_read_tensor_f16(unet_i8_handle_t h, const char* name, uint16_t* dstHost, size_t capBytes, int* channels) {
  if (!h || !name || !dstHost || !h->ws.p) return UNET_ERR_INVALID_ARG;
  auto it = h->tensors.find(name);
  if (it == h->tensors.end()) return UNET_ERR_UNKNOWN_PARAM;
  HIPCHK(h->err, hipSetDevice(h->device));
  HIPCHK(h->err, hipDeviceSynchronize());
  const I8Tensor& t = it->second;
  if (!t.f16) {
    h->err = std::string(name) + " is an int8 tensor: unet_i8_read_tensor reads it";
    return UNET_ERR_INVALID_ARG;
  }
  const size_t px = (size_t)h->wsN * (h->wsH >> t.level) * (h->wsW >> t.level);
  if (capBytes < px * t.c * 2) return UNET_ERR_INVALID_ARG;
  if (channels) *channels = t.c;
  HIPCHK(h->err, hipMemcpy2D(dstHost, (size_t)t.c * 2, h->ws.p + t.off, (size_t)t.ld * 2, (size_t)t.c * 2, px, hipMemcpyDeviceToHost));
  return UNET_OK;
}

// Hybrid quantisation: on (the default) = the units a model marks '<key>.hybrid' run in fp16; off = the same arrays run
// as pure int8.  Takes effect at the next unet_i8_finalize.
int unet_i8_set_hybrid(unet_i8_handle_t h, int on) {
  if (!h) return UNET_ERR_INVALID_ARG;
  h->hybridOn = on != 0;
  h->finalized = false;
  return UNET_OK;
}

// 0: int8, 1: fp16, -1: no such tensor or not finalized.  Names: "input", "im2col" and those of unet_i8_read_tensor.
int unet_i8_tensor_dtype(unet_i8_handle_t h, const char* name) {
  if (!h || !name || !h->finalized) return -1;
  auto it = h->f16Tensor.find(name);
  return it == h->f16Tensor.end() ? -1 : it->second;
}

int unet_i8_destroy(unet_i8_handle_t h) {
  if (!h) return UNET_OK;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  h->free_all();
  delete h;
  return UNET_OK;
}

const char* unet_i8_last_error(unet_i8_handle_t h) { return h ? h->err.c_str() : "null handle"; }

// ---- calibration on the float handle: per-tensor (min, max) of one forward, for quant.quantize_model ----
int unet_num_range_tensors(unet_handle_t h) { return h ? 3 + 4 * h->cfg.depth : 0; }

// the float forward of a calibration pass: the handle's own kind of forward with no output asked for (the range tensors
// are quant.tensor_names; none of them is the head's output)
static int calib_forward(unet_handle_t h, const uint8_t* frames, int n, int height, int width, void* stream) {
  if (h->cfg.out_channels > 1)
    return unet_forward_classes_u8(h, frames, n, height, width, 0, nullptr, nullptr, nullptr, 0, nullptr, stream);
  return unet_forward_u8(h, frames, n, height, width, nullptr, nullptr, nullptr, 0.f, stream);
}

// body of unet_forward_u8_ranges (single-class handles) and unet_forward_classes_u8_ranges (K-class handles)
static int forward_ranges(unet_handle_t h, const char* who, bool classes, const uint8_t* frames, int n, int height, int width,
                          float* rangesHost, void* stream) {
  if (!h || !frames || !rangesHost) return UNET_ERR_INVALID_ARG;
  if (int rc = classes ? multi_class_only(h, who) : single_class_only(h, who)) return rc;
  const int nt = unet_num_range_tensors(h);
  HIPCHK(h->err, hipSetDevice(h->cfg.device));
  std::vector<unsigned> init((size_t)nt * 2);
  for (int i = 0; i < nt; ++i) {
    init[2 * i] = 0xFFFFFFFFu;
    init[2 * i + 1] = 0u;
  }
  OpScratch sc((hipStream_t)stream);
  unsigned* keys = nullptr;
  HIPCHK(h->err, sc.upload(&keys, init.data(), init.size()));
  h->rangeKeys = keys;
  // direct kernels only: the Winograd kernel fuses the pool and the algorithms agree to 3e-5 anyway; ranges are
  // taken on the tensors the forward materialises
  const int rc = calib_forward(h, frames, n, height, width, stream);
  h->rangeKeys = nullptr;
  int rc2 = UNET_OK;
  if (!rc) {
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc2 = UNET_ERR_HIP;
    std::vector<unsigned> k((size_t)nt * 2);
    hipMemcpy(k.data(), keys, k.size() * sizeof(unsigned), hipMemcpyDeviceToHost);
    for (size_t i = 0; i < k.size(); ++i) {
      const unsigned u = (k[i] & 0x80000000u) ? (k[i] & 0x7FFFFFFFu) : ~k[i];
      float f;
      std::memcpy(&f, &u, 4);
      rangesHost[i] = f;
    }
  }
  return rc ? rc : rc2;
}

int unet_forward_u8_ranges(unet_handle_t h, const uint8_t* frames, int n, int height, int width, float* rangesHost,
                           void* stream) {
  return forward_ranges(h, "unet_forward_u8_ranges", false, frames, n, height, width, rangesHost, stream);
}

int unet_forward_classes_u8_ranges(unet_handle_t h, const uint8_t* frames, int n, int height, int width, float* rangesHost,
                                   void* stream) {
  return forward_ranges(h, "unet_forward_classes_u8_ranges", true, frames, n, height, width, rangesHost, stream);
}

// ---- histogram calibration ('mmse', 'kl_divergence'): the distribution of every range tensor over a given span ----
// The kernel on its own (tests): hist_dev[0 .. bins] += the histogram of x over [lo, hi), exact zeros in word `bins`.
int unet_op_histogram_f32(int device, const float* x, size_t npix, int c, int ld, float lo, float hi, int bins,
                          unsigned long long* histDev, void* stream) {
  if (!x || !histDev || npix == 0 || c < 1 || c > ld || !unet::histogram_bins_supported(bins) || !(hi > lo) ||
      !std::isfinite(lo) || !std::isfinite(hi) || !std::isfinite(hi - lo) || !std::isfinite(unet::histogram_inv(lo, hi, bins)))
    return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  return op_done(unet::launch_histogram_f32(x, npix, c, ld, lo, hi, bins, histDev, s), s, kOpMapCodes);
}

// The forward of unet_forward_u8_ranges with the probes in their second mode: tensor i (order: quant.tensor_names) is
// binned over spans_host[2 i], spans_host[2 i + 1] into hist_dev[i * (bins + 1) ...], which accumulates across calls and
// stays on the device.  No host synchronisation.
// body of unet_forward_u8_histograms (single-class handles) and unet_forward_classes_u8_histograms (K-class handles)
static int forward_histograms(unet_handle_t h, const char* who, bool classes, const uint8_t* frames, int n, int height,
                              int width, const float* spansHost, int bins, unsigned long long* histDev, void* stream) {
  if (!h || !frames || !spansHost || !histDev) return UNET_ERR_INVALID_ARG;
  if (int rc = classes ? multi_class_only(h, who) : single_class_only(h, who)) return rc;
  if (!unet::histogram_bins_supported(bins)) {
    h->err = "histogram bins must be a power of two from 64 to 4096";
    return UNET_ERR_INVALID_ARG;
  }
  const int nt = unet_num_range_tensors(h);
  for (int i = 0; i < nt; ++i) {
    const float lo = spansHost[2 * i], hi = spansHost[2 * i + 1];
    if (!(hi > lo) || !std::isfinite(hi - lo) || !std::isfinite(unet::histogram_inv(lo, hi, bins))) {
      h->err = "histogram span of range tensor " + std::to_string(i) + " is empty or not finite";
      return UNET_ERR_INVALID_ARG;
    }
  }
  h->hist = histDev;
  h->histSpans = spansHost;
  h->histBins = bins;
  const int rc = calib_forward(h, frames, n, height, width, stream);
  h->hist = nullptr;
  h->histSpans = nullptr;
  h->histBins = 0;
  return rc;
}

int unet_forward_u8_histograms(unet_handle_t h, const uint8_t* frames, int n, int height, int width,
                               const float* spansHost, int bins, unsigned long long* histDev, void* stream) {
  return forward_histograms(h, "unet_forward_u8_histograms", false, frames, n, height, width, spansHost, bins, histDev, stream);
}

int unet_forward_classes_u8_histograms(unet_handle_t h, const uint8_t* frames, int n, int height, int width,
                                       const float* spansHost, int bins, unsigned long long* histDev, void* stream) {
  return forward_histograms(h, "unet_forward_classes_u8_histograms", true, frames, n, height, width, spansHost, bins, histDev,
                            stream);
}

// compare_outputs (reference README.md:3512-3565): acc_dev[f] += sum over frame f of |pa - pb|, f < frames, each frame
// per_frame floats.  Two fixed-order passes into float64; no host synchronisation.
int unet_prob_mae_accumulate(int device, const float* paDev, const float* pbDev, int frames, size_t perFrame,
                             double* accDev, void* stream) {
  if (!paDev || !pbDev || !accDev || frames < 1 || frames > 65535 || perFrame == 0) return op_bad_args();
  HIPCHK(g_opErr, hipSetDevice(device));
  hipStream_t s = (hipStream_t)stream;
  double* partial = nullptr;
  HIPCHK(g_opErr, hipMallocAsync((void**)&partial, (size_t)frames * unet::MAE_BLOCKS_PER_FRAME * sizeof(double), s));
  const hipError_t e = unet::launch_prob_mae(paDev, pbDev, frames, perFrame, partial, accDev, s);
  HIPCHK(g_opErr, hipFreeAsync(partial, s));
  return op_done(e, s, kOpNoSync);
}

}  // extern "C"
