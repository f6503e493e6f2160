// The project's 8-bit HSV of an RGB pixel (augment.py: rgb_to_hsv), shared by the augmenter's colour step
// (augment_kernels.cpp) and the colour-threshold lane extractor (follow_kernels.cpp): integers, round-half-up,
//   V = max(R,G,B),  S = round(255 diff / V),  H = round(30 num / diff) + {0, 60, 120} for V == R, G, B in that order
// of preference, folded into [0, 180); a grey has H = 0.
// hsv8_terms states the two quotients once; rgb_to_hsv8 divides, hsv8_in_range compares without dividing.
#pragma once
#include <hip/hip_runtime.h>

namespace unet {

// S = sa / sb and, unless diff == 0, H = fold(off - 30 + ha / hb): floor divisions of non-negative integers
struct Hsv8Terms {
  int v, diff, sa, sb, ha, hb, off;
};

__device__ __forceinline__ Hsv8Terms hsv8_terms(int r, int g, int b) {
  Hsv8Terms t;
  t.v = max(max(r, g), b);
  t.diff = t.v - min(min(r, g), b);
  t.sa = 510 * t.diff + t.v;
  t.sb = max(2 * t.v, 1);
  const bool isR = t.v == r, isG = t.v == g;
  const int num = isR ? g - b : (isG ? b - r : r - g);
  t.off = isR ? 0 : (isG ? 60 : 120);
  t.ha = 60 * (num + t.diff) + t.diff;   // diff .. 121 diff: the quotient lies in 0 .. 60
  t.hb = 2 * t.diff;
  return t;
}

__device__ __forceinline__ void rgb_to_hsv8(int r, int g, int b, int& h, int& s, int& v) {
  const Hsv8Terms t = hsv8_terms(r, g, b);
  v = t.v;
  s = (int)((unsigned)t.sa / (unsigned)t.sb);
  h = 0;
  if (t.diff != 0) {
    h = t.off - 30 + (int)((unsigned)t.ha / (unsigned)t.hb);
    if (h < 0) h += 180;
    if (h >= 180) h -= 180;
  }
}

// lo[c] <= (H, S, V)[c] <= hi[c] for c = 0, 1, 2 (bounds in 0 .. 255), the same answer as comparing rgb_to_hsv8's
// result: for b > 0, lo <= floor(a / b) <= hi  <=>  lo * b <= a < (hi + 1) * b.  H = base + ha / hb, where base is
// off - 30, or off - 30 + 180 = 150 when that sum is negative - only for off == 0 and a quotient below 30; the fold at
// 180 never applies (off - 30 + 60 <= 150).
__device__ __forceinline__ bool hsv8_in_range(int r, int g, int b, const int (&lo)[3], const int (&hi)[3]) {
  const Hsv8Terms t = hsv8_terms(r, g, b);
  // bit-wise & and selects: straight-line code, no branch per condition
  const bool vin = (t.v >= lo[2]) & (t.v <= hi[2]);
  const bool sin = (t.sa >= __mul24(lo[1], t.sb)) & (t.sa < __mul24(hi[1] + 1, t.sb));   // every factor is below 2^10
  const int base = ((t.off == 0) & (t.ha < 30 * t.hb)) ? 150 : t.off - 30;
  const bool hue = (t.ha >= __mul24(lo[0] - base, t.hb)) & (t.ha < __mul24(hi[0] - base + 1, t.hb));
  const bool hin = t.diff == 0 ? lo[0] <= 0 : hue;
  return vin & sin & hin;
}

}  // namespace unet
