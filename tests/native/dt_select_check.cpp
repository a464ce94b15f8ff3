// Host-only check of select_dt() of csrc/rhmc_select.hpp: lanes per task and
// pixels per lane of the trial kernel of HMC_find_best_dt's search
// (rhmc_dt.hpp) for every kind of image side.  Built with a host compiler
// alone by tests/test_dt_host.py.
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

static SelectIn image(int side, int lanes = 0) {
  SelectIn s;
  s.rows = s.cols = side;
  s.max_lds = 160 * 1024;
  s.n_cu = 256;
  s.dt_lanes = lanes;
  return s;
}

int main() {
  // the register-resident sides: every pixel has a register, in an instantiated size
  for (int side = 16; side <= 64; ++side) {
    const DtPlan p = select_dt(image(side));
    CHECK(!p.message && p.lanes == 256);
    CHECK(p.ppl == 4 || p.ppl == 9 || p.ppl == 16);
    CHECK(p.lanes * p.ppl >= side * side);
    CHECK(p.blocks_cap >= 1);
    const DtPlan q = select_dt(image(side, 256));
    CHECK(q.lanes == p.lanes && q.ppl == p.ppl);
    const DtPlan n = select_dt(image(side, 64));
    CHECK(!n.message && n.lanes == 64);
    if (side <= 32) CHECK(n.ppl == 16 && 64 * n.ppl >= side * side);
    else CHECK(n.ppl == 0);                        // 36 pixels of D and M per lane spill
  }
  CHECK(select_dt(image(16)).ppl == 4 && select_dt(image(32)).ppl == 4);
  CHECK(select_dt(image(33)).ppl == 9 && select_dt(image(48)).ppl == 9);
  CHECK(select_dt(image(49)).ppl == 16 && select_dt(image(64)).ppl == 16);
  // every other side: the same body on global memory
  for (int side : {1, 2, 15, 65, 96, 128, 1024, 8192})
    for (int lanes : {0, 64, 256}) {
      const DtPlan p = select_dt(image(side, lanes));
      CHECK(!p.message && p.ppl == 0 && p.lanes == (lanes == 64 ? 64 : 256));
      CHECK(p.blocks_cap >= 1 && p.blocks_cap <= 4096);
    }
  // a non-square image is an error, not another kernel
  {
    SelectIn s = image(48);
    s.cols = 32;
    CHECK(select_dt(s).message != nullptr);
  }
  // the other options do not reach the rule
  {
    SelectIn s = image(48);
    s.kernel = RHMC_KERNEL_GENERIC;
    s.peaks_fused = 0;
    CHECK(select_dt(s).ppl == 9 && select_dt(s).lanes == 256);
  }
  CHECK(RHMC_DT_GRAD_REFERENCE == 0 && RHMC_DT_GRAD_FULL == 1);
  if (g_fail) return 1;
  std::printf("dt select ok\n");
  return 0;
}
