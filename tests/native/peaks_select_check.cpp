// Host-only check of the find_peaks rule of csrc/rhmc_select.hpp (Op::Peaks,
// select_peaks): which configurations take the one-launch descent kernel
// (Family::RegWin1) and which the stepwise path (Family::None).  Built with a
// host compiler alone by tests/test_peaks_host.py.
#include <cstdio>
#include <initializer_list>

#include "rhmc_select.hpp"

using namespace rhmc;

static int g_fail = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                         \
    }                                                                   \
  } while (0)

static SelectIn image(int side, bool f32, int kernel = RHMC_KERNEL_AUTO) {
  SelectIn s;
  s.rows = s.cols = side;
  s.img_f32 = f32;
  s.max_lds = 160 * 1024;
  s.n_cu = 256;
  s.kernel = kernel;
  return s;
}

static double inv_two_sig2(double sigma) { return 1.0 / (2.0 * sigma * sigma); }

int main() {
  const double ref = inv_two_sig2(3.5 / 2.354);  // the reference PSF, sigma = 1.487 px
  const double wide = inv_two_sig2(1.6);         // too wide for the 28-px window
  CHECK(reg_window_ok(28, ref) && !reg_window_ok(28, wide));
  auto plan = [&](const SelectIn& s, double c, int64_t n = 64) {
    return select(s, false, c, Op::Peaks, 1, n);
  };
  // sides 32 / 48 / 64 under the 28-px test: the fused kernel, at every batch
  // size (no lane-group descent), with the pixel cache the image allows
  for (int side : {32, 48, 64})
    for (int64_t n : {(int64_t)1, (int64_t)4096, (int64_t)65536, (int64_t)1 << 20}) {
      Plan p = plan(image(side, true), ref, n);
      CHECK(p.family == Family::RegWin1 && p.f32);
      p = plan(image(side, false), ref, n);
      CHECK(p.family == Family::RegWin1 && !p.f32);
    }
  // other sides: stepwise
  for (int side : {40, 96, 128, 256}) CHECK(plan(image(side, true), ref).family == Family::None);
  // a wide PSF: stepwise
  for (int side : {32, 48, 64}) CHECK(plan(image(side, true), wide).family == Family::None);
  // a forced per-wave family: stepwise; the one-star forcing options keep the kernel
  CHECK(plan(image(48, true, RHMC_KERNEL_GENERIC), ref).family == Family::None);
  CHECK(plan(image(48, true, RHMC_KERNEL_WINDOWED), ref).family == Family::None);
  CHECK(plan(image(48, true, RHMC_KERNEL_REGWIN), ref).family == Family::RegWin1);
  CHECK(plan(image(48, true, RHMC_KERNEL_LANE1), ref).family == Family::RegWin1);
  // RHMC_OPT_PEAKS_FUSED = 0: stepwise
  {
    SelectIn s = image(48, true);
    CHECK(s.peaks_fused == 1);
    s.peaks_fused = 0;
    CHECK(plan(s, ref).family == Family::None);
  }
  // a non-square image never reaches the kernel
  {
    SelectIn s = image(48, true);
    s.cols = 32;
    CHECK(plan(s, ref).family == Family::None);
  }
  // the stepwise path's launches exist for those configurations
  CHECK(select(image(40, true), false, ref, Op::Gradient, 1, 64).family == Family::LdsImage);
  CHECK(select(image(40, true), false, ref, Op::Energy, 1, 64).family == Family::LdsImage);
  CHECK(select(image(256, true), false, ref, Op::Gradient, 1, 64).family == Family::Slotted);
  CHECK(select(image(32, true), false, wide, Op::Energy, 1, 64).family == Family::LdsImage);
  // the status values share a word with the step's bits without colliding
  constexpr unsigned step_bits = RHMC_STATUS_NONFINITE | RHMC_STATUS_PLOOP_CAP |
                                 RHMC_STATUS_QLOOP_CAP | RHMC_STATUS_REFLECT_F |
                                 RHMC_STATUS_REFLECT_XY | RHMC_STATUS_NEAR_WALL;
  CHECK(((RHMC_PEAK_CONVERGED | RHMC_PEAK_FAINT | RHMC_PEAK_CAP) & step_bits) == 0);
  CHECK((RHMC_PEAK_CONVERGED & RHMC_PEAK_FAINT) == 0 && (RHMC_PEAK_FAINT & RHMC_PEAK_CAP) == 0 &&
        (RHMC_PEAK_CONVERGED & RHMC_PEAK_CAP) == 0);
  if (g_fail) return 1;
  std::printf("peaks select ok\n");
  return 0;
}
