// record_check_main.cpp — the host-side check of dsp_loop_record (dispatches_amd/csrc/dsp_record_check.hpp, the very function
// dsp_capi_loop.hip calls before it launches) as a stand-alone program for the host sanitizers: it is fed a sound descriptor and every
// malformed one the header lists, and must accept the first, refuse the rest and run clean.  No GPU, no HIP runtime.
//     clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/record_check_main.cpp -o record_check && ./record_check
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "../dispatches_amd/csrc/dsp_record_check.hpp"

static int64_t clock_word;          // never read by the check: only its address is taken
static double source[16], record[64];

static dsp_loop_record_desc sound() {
  dsp_loop_record_desc d;
  std::memset(&d, 0, sizeof d);
  d.n_plants = 3, d.n_segments = 2;
  d.plants[0] = 1, d.plants[1] = 4, d.plants[2] = 8;
  d.clock = &clock_word, d.divisor = 1, d.offset = 0, d.rows = 3;
  d.segments[0] = {source, record, 5, 1, 5, 8};
  d.segments[1] = {source, record, 1, 9, 3, 4};
  return d;
}

static int failures = 0;
static void expect(bool want, int32_t B, const char *what, const std::function<void(dsp_loop_record_desc &)> &edit) {
  dsp_loop_record_desc d = sound();
  edit(d);
  if (dsp::loop_record_ok(&d, B) != want) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}
#define REFUSED(B, stmt) expect(false, B, #stmt, [](dsp_loop_record_desc &d) { stmt; })

int main() {
  const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
  const int64_t lmax = std::numeric_limits<int64_t>::max(), lmin = std::numeric_limits<int64_t>::min();
  expect(true, 9, "the sound descriptor", [](dsp_loop_record_desc &) {});
  expect(true, 64, "64 plants, 16 segments", [](dsp_loop_record_desc &d) {
    d.n_plants = 64, d.n_segments = 16;
    for (int q = 0; q < 64; ++q) d.plants[q] = q;
    for (int g = 2; g < 16; ++g) d.segments[g] = d.segments[0];
  });
  if (dsp::loop_record_ok(nullptr, 9)) std::printf("FAILED: NULL descriptor\n"), ++failures;
  REFUSED(9, d.clock = nullptr);
  REFUSED(0, (void)d);
  REFUSED(-1, (void)d);
  REFUSED(8, (void)d);                                   // plants[2] = 8 is not below B = 8
  REFUSED(9, d.n_plants = 0);
  REFUSED(9, d.n_plants = 65);                           // would index past plants[64]: refused before any element is read
  REFUSED(9, d.n_plants = imax);
  REFUSED(9, d.n_plants = imin);
  REFUSED(9, d.n_segments = 0);
  REFUSED(9, d.n_segments = 17);
  REFUSED(9, d.n_segments = imax);
  REFUSED(9, d.n_segments = imin);
  REFUSED(9, d.rows = 0);
  REFUSED(9, d.rows = (1 << 24) + 1);
  REFUSED(9, d.rows = imin);
  REFUSED(9, d.divisor = 0);
  REFUSED(9, d.divisor = 8785);
  REFUSED(9, d.divisor = imin);
  REFUSED(9, d.offset = 1);
  REFUSED(9, d.offset = -2);
  REFUSED(9, d.offset = imin);
  REFUSED(9, d.reserved = 1);
  REFUSED(9, d.plants[1] = 1);                           // not strictly increasing
  REFUSED(9, d.plants[2] = 3);
  REFUSED(9, d.plants[0] = -1);
  REFUSED(9, d.plants[0] = imin);
  REFUSED(9, d.plants[2] = 9);
  REFUSED(9, d.plants[2] = imax);
  for (int g = 0; g < 2; ++g) {
    expect(false, 9, "NULL src", [g](dsp_loop_record_desc &d) { d.segments[g].src = nullptr; });
    expect(false, 9, "NULL dst", [g](dsp_loop_record_desc &d) { d.segments[g].dst = nullptr; });
    for (int32_t w : {0, -1, DSP_RECORD_MAX_WIDTH + 1, imax, imin})
      expect(false, 9, "width", [g, w](dsp_loop_record_desc &d) { d.segments[g].width = w; });
    for (int32_t e : {0, 1, 2, 16, -8, imax, imin})
      expect(false, 9, "elem_bytes", [g, e](dsp_loop_record_desc &d) { d.segments[g].elem_bytes = e; });
    for (int64_t s : {(int64_t)0, (int64_t)-1, ((int64_t)1 << 40) + 1, lmax, lmin}) {
      expect(false, 9, "plant_stride", [g, s](dsp_loop_record_desc &d) { d.segments[g].plant_stride = s; });
      expect(false, 9, "elem_stride", [g, s](dsp_loop_record_desc &d) { d.segments[g].elem_stride = s; });
    }
  }
  expect(true, 9, "an unused segment is not looked at", [](dsp_loop_record_desc &d) { d.segments[2].width = -1; });
  std::printf(failures ? "%d checks failed\n" : "all descriptors judged as the header states (%d failures)\n", failures);
  return failures ? 1 : 0;
}
