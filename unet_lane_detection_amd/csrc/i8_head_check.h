// int8 tier, host only (no HIP): the class count of a loaded quantised model and the consistency of its head arrays.
// unet_i8_finalize calls it before it touches a device; tools/i8_head_check_main.cpp runs it on its own under the host
// sanitizers.
#pragma once

#include <cstddef>
#include <map>
#include <string>
#include <vector>

namespace unet {

constexpr int I8_MAX_CLASSES = 8;   // == UNET_MAX_CLASSES

typedef std::map<std::string, std::vector<unsigned char>> I8Arrays;

// K = the entries of output.bias_q (int32), 1 .. I8_MAX_CLASSES; output.w_q must hold K rows of c0 int8 weights,
// output.w_zp and output.mult K entries each, and - for a head that runs hybrid - output.w_h K rows of c0 fp16
// weights, output.gain and output.bias_f K entries each.  Returns K, or 0 with a text in `err`.
inline int i8_head_classes(const I8Arrays& arrays, int c0, bool hybridHead, std::string& err) {
  auto bytes = [&](const char* name, size_t& out) {
    auto it = arrays.find(name);
    if (it == arrays.end()) {
      err = std::string("missing array ") + name;
      return false;
    }
    out = it->second.size();
    return true;
  };
  size_t nb = 0;
  if (!bytes("output.bias_q", nb)) return 0;
  if (nb == 0 || nb % 4 || nb / 4 > (size_t)I8_MAX_CLASSES) {
    err = "output.bias_q: " + std::to_string(nb) + " bytes; the head has 1 .. " + std::to_string(I8_MAX_CLASSES) +
          " classes, one int32 each";
    return 0;
  }
  const int K = (int)(nb / 4);
  if (c0 <= 0) {
    err = "the head needs a positive channel count";
    return 0;
  }
  auto expect = [&](const char* name, size_t want) {
    size_t got = 0;
    if (!bytes(name, got)) return false;
    if (got != want) {
      err = std::string(name) + ": expected " + std::to_string(want) + " bytes for the " + std::to_string(K) +
            " classes of output.bias_q, got " + std::to_string(got);
      return false;
    }
    return true;
  };
  if (!expect("output.w_q", (size_t)K * c0) || !expect("output.w_zp", (size_t)K * 4) || !expect("output.mult", (size_t)K * 4))
    return 0;
  if (hybridHead && (!expect("output.w_h", (size_t)K * c0 * 2) || !expect("output.gain", (size_t)K * 4) ||
                     !expect("output.bias_f", (size_t)K * 4)))
    return 0;
  return K;
}

}  // namespace unet
