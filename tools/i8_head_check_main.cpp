// Stand-alone host program around unet::i8_head_classes (csrc/i8_head_check.h): the class count of a quantised model and
// the consistency checks unet_i8_finalize makes before it touches a device.  For the host sanitizers, no GPU needed:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/i8_head_check_main.cpp -o i8_head_check && ./i8_head_check
// Exit status 0 when every case gives what it must.
#include "../unet_lane_detection_amd/csrc/i8_head_check.h"

#include <cstdio>

namespace {

unet::I8Arrays head(int k, int c0, bool hybrid) {
  unet::I8Arrays a;
  a["output.bias_q"].assign((size_t)k * 4, 1);
  a["output.w_q"].assign((size_t)k * c0, 2);
  a["output.w_zp"].assign((size_t)k * 4, 3);
  a["output.mult"].assign((size_t)k * 4, 4);
  if (hybrid) {
    a["output.w_h"].assign((size_t)k * c0 * 2, 5);
    a["output.gain"].assign((size_t)k * 4, 6);
    a["output.bias_f"].assign((size_t)k * 4, 7);
  }
  return a;
}

int failures = 0;

void expect(const char* what, const unet::I8Arrays& a, int c0, bool hybrid, int want) {
  std::string err;
  const int got = unet::i8_head_classes(a, c0, hybrid, err);
  const bool ok = got == want && (want != 0 || err.size() > 10);
  std::printf("%-44s -> %d %s%s\n", what, got, ok ? "ok" : "WRONG", err.empty() ? "" : ("  [" + err + "]").c_str());
  if (!ok) ++failures;
}

}  // namespace

int main() {
  for (int k = 1; k <= unet::I8_MAX_CLASSES; ++k)
    for (int hyb = 0; hyb < 2; ++hyb) expect("a well-formed head", head(k, 32, hyb), 32, hyb, k);
  expect("no arrays at all", unet::I8Arrays(), 32, false, 0);
  expect("nine classes", head(9, 32, false), 32, false, 0);
  {
    auto a = head(3, 32, false);
    a["output.bias_q"].clear();
    expect("an empty output.bias_q", a, 32, false, 0);
    a["output.bias_q"].assign(7, 0);
    expect("output.bias_q of 7 bytes", a, 32, false, 0);
  }
  for (const char* name : {"output.w_q", "output.w_zp", "output.mult"}) {
    auto a = head(3, 32, false);
    a[name].pop_back();
    expect((std::string(name) + " one byte short").c_str(), a, 32, false, 0);
    a.erase(name);
    expect((std::string(name) + " missing").c_str(), a, 32, false, 0);
  }
  for (const char* name : {"output.w_h", "output.gain", "output.bias_f"}) {
    auto a = head(4, 64, true);
    a[name].push_back(0);
    expect((std::string(name) + " one byte long (hybrid head)").c_str(), a, 64, true, 0);
    expect((std::string(name) + " one byte long (head not hybrid)").c_str(), a, 64, false, 4);
    a.erase(name);
    expect((std::string(name) + " missing (hybrid head)").c_str(), a, 64, true, 0);
  }
  expect("a channel count that is not the model's", head(2, 32, false), 64, false, 0);
  expect("no channels", head(2, 32, false), 0, false, 0);
  std::printf("%d failure(s)\n", failures);
  return failures ? 1 : 0;
}
