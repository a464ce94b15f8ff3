// select_hess() (csrc/rhmc_select.hpp) with a host compiler alone: which
// (K, side) the Hessian-metric kernels serve, with how many waves per workgroup
// and how much LDS.  tests/test_hess_host.py builds and runs it.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rhmc_select.hpp"

using namespace rhmc;

static int g_fail = 0;
#define CHECK(cond)                                                         \
  do {                                                                      \
    if (!(cond)) {                                                          \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++g_fail;                                                             \
    }                                                                       \
  } while (0)

static SelectIn image(int rows, int cols, int max_lds = 160 * 1024) {
  SelectIn s;
  s.rows = rows;
  s.cols = cols;
  s.max_lds = max_lds;
  s.n_cu = 256;
  return s;
}

int main() {
  // every (K, side) of the scope is served within gfx950's 160 KB
  for (int side : {16, 32, 48})
    for (int K = 1; K <= 16; ++K) {
      const HessPlan pl = select_hess(image(side, side), K);
      CHECK(pl.message == nullptr);
      CHECK(pl.waves == 4 || pl.waves == 2 || pl.waves == 1);
      CHECK(pl.lds_bytes <= 160 * 1024);
      // the image once, per wave four tables, the 1 / Lambda image, the fluxes
      const size_t wave = (size_t)4 * K * side + (size_t)side * side + 16;
      CHECK(pl.lds_bytes == ((size_t)side * side + pl.waves * wave) * sizeof(double));
      CHECK(hess_wave_doubles(K, side) == wave);
      // the largest workgroup that fits
      if (pl.waves < 4)
        CHECK(((size_t)side * side + 2 * pl.waves * wave) * sizeof(double) > 160 * 1024);
    }
  CHECK(select_hess(image(48, 48), 11).waves == 4);
  CHECK(select_hess(image(48, 48), 11).lds_bytes == 160256);
  CHECK(select_hess(image(48, 48), 12).waves == 2);
  CHECK(select_hess(image(48, 48), 16).lds_bytes == 104704);
  CHECK(select_hess(image(32, 32), 16).waves == 4);
  // the sides in between are served too
  CHECK(select_hess(image(17, 17), 3).message == nullptr);
  CHECK(select_hess(image(47, 47), 16).message == nullptr);
  // refused: K = 17 and more, K < 1, sides outside 16..48, a non-square image
  for (int K : {17, 64, 1024, 0, -1}) {
    const HessPlan pl = select_hess(image(32, 32), K);
    CHECK(pl.message != nullptr && std::strstr(pl.message, "1 <= K <= 16"));
    CHECK(pl.waves == 0);
  }
  for (int side : {15, 1, 49, 64, 100}) {
    const HessPlan pl = select_hess(image(side, side), 1);
    CHECK(pl.message != nullptr && std::strstr(pl.message, "side 16..48"));
  }
  CHECK(select_hess(image(32, 48), 1).message != nullptr);
  // a device with less LDS gets fewer waves, then the refusal
  CHECK(select_hess(image(48, 48, 64 * 1024), 1).waves == 2);
  CHECK(select_hess(image(48, 48, 64 * 1024), 16).waves == 1);
  CHECK(select_hess(image(48, 48, 48 * 1024), 16).message != nullptr);
  CHECK(select_hess(image(48, 48, 0), 1).message != nullptr);
  // RHMC_OPT_KERNEL does not enter
  for (int kern : {RHMC_KERNEL_GENERIC, RHMC_KERNEL_WINDOWED, RHMC_KERNEL_DENSE}) {
    SelectIn s = image(48, 48);
    s.kernel = kern;
    const HessPlan a = select_hess(s, 3), b = select_hess(image(48, 48), 3);
    CHECK(a.message == nullptr && a.waves == b.waves && a.lds_bytes == b.lds_bytes);
  }
  if (g_fail) return 1;
  std::printf("hess select ok\n");
  return 0;
}
