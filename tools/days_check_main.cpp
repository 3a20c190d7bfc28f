// days_check_main.cpp — the host-side checks of dsp_loop_profile, dsp_days_assign, dsp_days_update and dsp_days_frequency
// (dispatches_amd/csrc/dsp_days_check.hpp, the very functions dsp_days.hip calls before it launches) as a stand-alone program for the host
// sanitizers: it is fed sound descriptors and every malformed one the header lists, and must accept the first, refuse the rest and run
// clean.  No GPU, no HIP runtime.
//     clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/days_check_main.cpp -o days_check && ./days_check
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>

#include "../dispatches_amd/csrc/dsp_days_check.hpp"

static int64_t clock_word, start_words[4], counts[64];          // never read by the checks: only addresses are taken
static double buffer[64];
static int32_t labels[16];

static dsp_loop_profile_desc sound_profile() {
  dsp_loop_profile_desc p;
  std::memset(&p, 0, sizeof p);
  p.B = 4, p.days = 2, p.clock = &clock_word, p.delivered = buffer, p.profile = buffer;
  return p;
}

static dsp_days_desc sound_days(int channels) {
  dsp_days_desc d;
  std::memset(&d, 0, sizeof d);
  d.B = 4, d.days = 2, d.channels = channels, d.filter = 1;
  d.profile = buffer, d.p_min = buffer, d.p_max = buffer;
  if (channels == 2) d.cf_series = buffer, d.start = start_words, d.N = 48;
  return d;
}

static int failures = 0;
static void check(bool got, bool want, const char *what) {
  if (got != want) {
    std::printf("FAILED: %s\n", what);
    ++failures;
  }
}

// all three entry points' checks on one descriptor: each must say `want`
static void all_three(const dsp_days_desc *d, int32_t K, bool want, const char *what) {
  const int64_t need = d && K >= 1 && K <= DSP_DAYS_MAX_K && d->channels >= 1 && d->channels <= 2 && d->B >= 0 && d->days >= 1
                           ? dsp::days_work_doubles((int64_t)d->B * d->days, K, d->channels) : 0;
  check(dsp::days_assign_ok(d, buffer, K, labels, buffer), want, what);
  check(dsp::days_update_ok(d, labels, buffer, K, buffer, counts, buffer, buffer, need < 0 ? 0 : need), want, what);
  check(dsp::days_frequency_ok(d, labels, K, buffer), want, what);
}

static void days(bool want, int channels, int32_t K, const char *what, const std::function<void(dsp_days_desc &)> &edit) {
  dsp_days_desc d = sound_days(channels);
  edit(d);
  all_three(&d, K, want, what);
}
#define DAYS_REFUSED(ch, stmt) days(false, ch, 3, #stmt, [](dsp_days_desc &d) { stmt; })

static void profile(bool want, const char *what, const std::function<void(dsp_loop_profile_desc &)> &edit) {
  dsp_loop_profile_desc p = sound_profile();
  edit(p);
  check(dsp::loop_profile_ok(&p), want, what);
}
#define PROFILE_REFUSED(stmt) profile(false, #stmt, [](dsp_loop_profile_desc &p) { stmt; })

int main() {
  const int32_t imax = std::numeric_limits<int32_t>::max(), imin = std::numeric_limits<int32_t>::min();
  const int64_t lmin = std::numeric_limits<int64_t>::min();

  // dsp_loop_profile
  profile(true, "the sound profile descriptor", [](dsp_loop_profile_desc &) {});
  profile(true, "B == 0", [](dsp_loop_profile_desc &p) { p.B = 0; });
  profile(true, "the largest span", [](dsp_loop_profile_desc &p) { p.B = DSP_DAYS_MAX_PLANTS, p.days = DSP_DAYS_MAX_DAYS; });
  check(dsp::loop_profile_ok(nullptr), false, "NULL profile descriptor");
  PROFILE_REFUSED(p.clock = nullptr);
  PROFILE_REFUSED(p.delivered = nullptr);
  PROFILE_REFUSED(p.profile = nullptr);
  PROFILE_REFUSED(p.B = -1);
  PROFILE_REFUSED(p.B = imin);
  PROFILE_REFUSED(p.B = DSP_DAYS_MAX_PLANTS + 1);
  PROFILE_REFUSED(p.B = imax);
  PROFILE_REFUSED(p.days = 0);
  PROFILE_REFUSED(p.days = -1);
  PROFILE_REFUSED(p.days = imin);
  PROFILE_REFUSED(p.days = DSP_DAYS_MAX_DAYS + 1);
  PROFILE_REFUSED(p.days = imax);
  for (int q = 0; q < 4; ++q) profile(false, "reserved", [q](dsp_loop_profile_desc &p) { p.reserved[q] = 1; });

  // the representative-day entry points
  for (int ch = 1; ch <= 2; ++ch) {
    days(true, ch, 3, "the sound descriptor", [](dsp_days_desc &) {});
    days(true, ch, 1, "K = 1", [](dsp_days_desc &) {});
    days(true, ch, DSP_DAYS_MAX_K, "K = 64", [](dsp_days_desc &) {});
    days(true, ch, 3, "B == 0", [](dsp_days_desc &d) { d.B = 0; });
    days(true, ch, 3, "no filter", [](dsp_days_desc &d) { d.filter = 0; });
    days(true, ch, 3, "the most points", [](dsp_days_desc &d) { d.B = 32767, d.days = 65536; });
    for (int32_t K : {0, -1, DSP_DAYS_MAX_K + 1, imax, imin}) days(false, ch, K, "K", [](dsp_days_desc &) {});
    all_three(nullptr, 3, false, "NULL descriptor");
    DAYS_REFUSED(ch, d.profile = nullptr);
    DAYS_REFUSED(ch, d.p_min = nullptr);
    DAYS_REFUSED(ch, d.p_max = nullptr);
    DAYS_REFUSED(ch, d.B = -1);
    DAYS_REFUSED(ch, d.B = imin);
    DAYS_REFUSED(ch, d.B = DSP_DAYS_MAX_PLANTS + 1);
    DAYS_REFUSED(ch, d.B = imax);
    DAYS_REFUSED(ch, d.days = 0);
    DAYS_REFUSED(ch, d.days = -1);
    DAYS_REFUSED(ch, d.days = imin);
    DAYS_REFUSED(ch, d.days = DSP_DAYS_MAX_DAYS + 1);
    DAYS_REFUSED(ch, d.days = imax);
    DAYS_REFUSED(ch, (d.B = 32768, d.days = 65536));              // 2^31 points: one more than DSP_DAYS_MAX_POINTS
    DAYS_REFUSED(ch, (d.B = DSP_DAYS_MAX_PLANTS, d.days = DSP_DAYS_MAX_DAYS));
    DAYS_REFUSED(ch, d.channels = 0);
    DAYS_REFUSED(ch, d.channels = 3);
    DAYS_REFUSED(ch, d.channels = -1);
    DAYS_REFUSED(ch, d.channels = imax);
    DAYS_REFUSED(ch, d.channels = imin);
    DAYS_REFUSED(ch, d.filter = 2);
    DAYS_REFUSED(ch, d.filter = -1);
    DAYS_REFUSED(ch, d.filter = imin);
    for (int q = 0; q < 4; ++q) days(false, ch, 3, "reserved", [q](dsp_days_desc &d) { d.reserved[q] = -1; });
  }
  DAYS_REFUSED(2, d.cf_series = nullptr);
  DAYS_REFUSED(2, d.start = nullptr);
  DAYS_REFUSED(2, d.N = 0);
  DAYS_REFUSED(2, d.N = -1);
  DAYS_REFUSED(2, d.N = lmin);
  days(true, 1, 3, "one channel ignores the series", [](dsp_days_desc &d) { d.cf_series = nullptr, d.start = nullptr, d.N = -5; });

  // the array arguments, one at a time
  const dsp_days_desc d = sound_days(2);
  const int64_t need = dsp::days_work_doubles(8, 3, 2);
  check(need == 1 * (3 * 48 + 3 + 2), true, "work size of one chunk");
  check(dsp::days_work_doubles(DSP_DAYS_CHUNK + 1, 64, 2) == 2 * (64 * 48 + 64 + 2), true, "work size of two chunks");
  check(dsp::days_work_doubles(-1, 3, 1) == -1 && dsp::days_work_doubles(8, 0, 1) == -1 && dsp::days_work_doubles(8, 3, 3) == -1 &&
            dsp::days_work_doubles((int64_t)DSP_DAYS_MAX_POINTS + 1, 3, 1) == -1, true, "work size refusals");
  check(dsp::days_assign_ok(&d, nullptr, 3, labels, buffer), false, "assign: NULL centres");
  check(dsp::days_assign_ok(&d, buffer, 3, nullptr, buffer), false, "assign: NULL label");
  check(dsp::days_assign_ok(&d, buffer, 3, labels, nullptr), false, "assign: NULL dist2");
  check(dsp::days_update_ok(&d, labels, buffer, 3, buffer, counts, buffer, buffer, need), true, "update: sound");
  check(dsp::days_update_ok(&d, nullptr, buffer, 3, buffer, counts, buffer, buffer, need), false, "update: NULL label");
  check(dsp::days_update_ok(&d, labels, nullptr, 3, buffer, counts, buffer, buffer, need), false, "update: NULL dist2");
  check(dsp::days_update_ok(&d, labels, buffer, 3, nullptr, counts, buffer, buffer, need), false, "update: NULL centres");
  check(dsp::days_update_ok(&d, labels, buffer, 3, buffer, nullptr, buffer, buffer, need), false, "update: NULL count");
  check(dsp::days_update_ok(&d, labels, buffer, 3, buffer, counts, nullptr, buffer, need), false, "update: NULL inertia");
  check(dsp::days_update_ok(&d, labels, buffer, 3, buffer, counts, buffer, nullptr, need), false, "update: NULL work");
  check(dsp::days_update_ok(&d, labels, buffer, 3, buffer, counts, buffer, buffer, need - 1), false, "update: work one double short");
  check(dsp::days_update_ok(&d, labels, buffer, 3, buffer, counts, buffer, buffer, lmin), false, "update: negative work size");
  check(dsp::days_frequency_ok(&d, nullptr, 3, buffer), false, "frequency: NULL label");
  check(dsp::days_frequency_ok(&d, labels, 3, nullptr), false, "frequency: NULL freq");
  std::printf(failures ? "%d checks failed\n" : "all descriptors judged as the header states (%d failures)\n", failures);
  return failures ? 1 : 0;
}
