// select_check.cpp — host-only check of csrc/rhmc_select.hpp: the plan for the
// configurations the project's documents name (README workloads, DESIGN.md
// section 4, include/rhmc.h's RHMC_KERNEL_* list, the ragged families).  The
// expected values are written from those documents, not from the header.
// Built by tests/test_select.py with a host compiler alone; exits non-zero
// with the failed rows listed.
#include <cstdio>
#include <initializer_list>

#include "rhmc_select.hpp"

using namespace rhmc;

static int g_failed = 0;
#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond);            \
      ++g_failed;                                                        \
    }                                                                    \
  } while (0)

// MI355X: 160 KB of LDS per workgroup, 256 compute units.
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
  const double wide = inv_two_sig2(1.6);         // past the 32-px window's 1.574 px
  const bool noVc = false;
  auto plan = [&](const SelectIn& s, Op op, int K, int64_t n) {
    return select(s, noVc, ref, op, K, n);
  };

  for (int side : {32, 48}) {
    // C1 / C2: one star, 4096 chains, Poisson counts (fp32-exact)
    Plan p = plan(image(side, true), Op::Step, 1, 4096);
    CHECK(p.family == Family::RegWin1 && p.window == 28 && p.f32);
    // the same from 16 Ki / 64 Ki chains: the lane-group kernel, 4 / 1 lanes per chain
    p = plan(image(side, true), Op::Step, 1, 16384);
    CHECK(p.family == Family::Lane && p.lpc == 4 && p.f32);
    p = plan(image(side, true), Op::Step, 1, 65536);
    CHECK(p.family == Family::Lane && p.lpc == 1 && p.f32);
    // the explicit integrators, HMC_random and the energy ignore the lane threshold
    for (Op op : {Op::Integrate, Op::HmcRandom, Op::Energy}) {
      p = plan(image(side, true), op, 1, 65536);
      CHECK(p.family == Family::RegWin1 && p.window == 28 && p.f32);
    }
    // the fused MH gives way to the lane-group kernel
    CHECK(plan(image(side, true), Op::MhFused, 1, 4096).family == Family::RegWin1);
    CHECK(plan(image(side, true), Op::MhFused, 1, 16384).family == Family::None);

    // C3: ten stars, fp32-exact -> pixel-major; else multi-star register-window
    // with LDS factor tables
    for (Op op : {Op::Step, Op::Integrate, Op::HmcRandom, Op::MhFused})
      CHECK(plan(image(side, true), op, 10, 4096).family == Family::PixMajor);
    p = plan(image(side, false), Op::Step, 10, 4096);
    CHECK(p.family == Family::MultiWin && p.tables && p.slots == 1 && !p.f32);
    CHECK(plan(image(side, false), Op::MhFused, 10, 4096).family == Family::None);
    // ... and their energy / gradient come from the LDS-image kernels
    CHECK(plan(image(side, true), Op::Energy, 10, 4096).family == Family::LdsImage);
    CHECK(plan(image(side, true), Op::Gradient, 10, 4096).family == Family::LdsImage);
    // ... with as many register accumulators as the next power of two of K
    const int accumulators[][2] = {{1, 1}, {2, 2}, {3, 4}, {4, 4},
                                   {5, 8}, {8, 8}, {9, 16}, {16, 16}};
    for (const auto& ka : accumulators) {
      p = plan(image(side, true, RHMC_KERNEL_GENERIC), Op::Step, ka[0], 4096);
      CHECK(p.family == Family::LdsImage && p.maxk == ka[1]);
      for (Op op : {Op::Energy, Op::Gradient})
        CHECK(plan(image(side, true, RHMC_KERNEL_GENERIC), op, ka[0], 4096).maxk == ka[1]);
    }

    // dense from 11 stars: B4 (K = 51) one slot, K = 100 two
    for (Op op : {Op::Step, Op::Integrate, Op::HmcRandom, Op::Energy, Op::Gradient}) {
      p = plan(image(side, true), op, 51, 4096);
      CHECK(p.family == Family::Slotted && p.policy == Policy::DenseG && p.path == side &&
            p.slots == 1);
      p = plan(image(side, true), op, 100, 4096);
      CHECK(p.family == Family::Slotted && p.policy == Policy::DenseG && p.slots == 2);
      p = plan(image(side, true), op, 11, 4096);
      CHECK(p.family == Family::Slotted && p.policy == Policy::DenseG && p.slots == 1);
    }
    // past 256 stars the dense kernel has no slots: global tables, 8 slots at K = 300
    p = plan(image(side, true), Op::Step, 300, 1024);
    CHECK(p.family == Family::Slotted && p.policy == Policy::WinGG && p.path == 0 && p.slots == 8);
  }

  {  // 96 px, one star: the implicit step only
    const SelectIn s = image(96, true);
    Plan p = plan(s, Op::Step, 1, 4096);
    CHECK(p.family == Family::RegWin1 && p.f32);
    CHECK(plan(s, Op::Integrate, 1, 4096).family != Family::RegWin1);
    CHECK(plan(s, Op::HmcRandom, 1, 4096).family != Family::RegWin1);
    CHECK(plan(s, Op::Energy, 1, 4096).family != Family::RegWin1);
    CHECK(plan(s, Op::MhFused, 1, 4096).family == Family::None);
    // no lane-group kernel above 64 px
    CHECK(plan(s, Op::Step, 1, 65536).family == Family::RegWin1);
  }

  {  // C5: 256 px, 64 stars: two slots, no tables; the split by batch size
    // (WS 4 at 1024 and 4096 chains, 2 at 8192, 1 at 16384)
    const SelectIn s = image(256, true);
    Plan p = plan(s, Op::Step, 64, 8192);
    CHECK(p.family == Family::MultiWin && p.slots == 2 && !p.tables && p.f32);
    CHECK(plan(s, Op::Step, 64, 1024).split == 4);
    CHECK(plan(s, Op::Step, 64, 2048).split == 4);
    CHECK(plan(s, Op::Step, 64, 4096).split == 4);
    CHECK(plan(s, Op::Step, 64, 8192).split == 2);
    CHECK(plan(s, Op::Step, 64, 16384).split == 1);
    SelectIn forced = s;  // RHMC_OPT_WINDOW_SPLIT
    forced.window_split = 2;
    CHECK(select(forced, noVc, ref, Op::Step, 64, 1024).split == 2);
    // the explicit solvers and HMC_random keep one wave per pair
    CHECK(plan(s, Op::Integrate, 64, 1024).split == 1);
    CHECK(plan(s, Op::HmcRandom, 64, 1024).split == 1);
    // K <= 32 without tables: one slot
    p = plan(s, Op::Step, 24, 8192);
    CHECK(p.family == Family::MultiWin && p.slots == 1 && !p.tables);
  }

  {  // 64 px: no dense kernel; K = 100 on the global tables with two slots,
    // K = 40 energy on column tables (WinEG), gradient on full tables (WinG)
    const SelectIn s = image(64, true);
    Plan p = plan(s, Op::Step, 100, 1024);
    CHECK(p.family == Family::Slotted && p.policy == Policy::WinGG && p.slots == 2 && p.path == 0);
    p = plan(s, Op::Energy, 40, 1024);
    CHECK(p.family == Family::Slotted && p.policy == Policy::WinEG && p.slots == 1);
    p = plan(s, Op::Gradient, 40, 1024);
    CHECK(p.family == Family::Slotted && p.policy == Policy::WinG && p.slots == 1);
    CHECK(plan(s, Op::Step, 40, 1024).family == Family::MultiWin);
  }

  {  // sigma above 1.574 px where only the windowed kernels would serve
    const SelectIn s = image(64, true);
    for (Op op : {Op::Step, Op::Integrate, Op::HmcRandom, Op::Energy, Op::Gradient}) {
      const Plan p = select(s, noVc, wide, op, 40, 1024);
      CHECK(p.family == Family::Unsupported && p.message != nullptr);
    }
    // the dense kernel and the LDS-image kernels take any PSF width
    CHECK(select(image(32, true), noVc, wide, Op::Step, 51, 1024).family == Family::Slotted);
    CHECK(select(image(32, true), noVc, wide, Op::Gradient, 10, 1024).family == Family::LdsImage);
    // one star: the 32-px register window reaches to sigma = 1.726 px (rhmc_tiledr.hpp)
    const Plan p1 = select(image(32, true), noVc, wide, Op::Step, 1, 1024);
    CHECK(p1.family == Family::RegWin1 && p1.window == 32);
    CHECK(select(image(32, true), noVc, wide, Op::Step, 10, 1024).family == Family::PixMajor);
  }

  {  // RHMC_KERNEL_* (include/rhmc.h), on C2's and C3's geometry
    auto forced = [&](int kernel, Op op, int K, int64_t n, bool f32 = true, int side = 48) {
      return plan(image(side, f32, kernel), op, K, n);
    };
    // GENERIC: image in LDS (K <= 16 and it fits), else WINDOWED; explicit
    // integrators and HMC_random take WINDOWED; MH runs the four-kernel loop
    CHECK(forced(RHMC_KERNEL_GENERIC, Op::Step, 1, 4096).family == Family::LdsImage);
    CHECK(forced(RHMC_KERNEL_GENERIC, Op::Step, 10, 4096).family == Family::LdsImage);
    CHECK(forced(RHMC_KERNEL_GENERIC, Op::Energy, 1, 4096).family == Family::LdsImage);
    Plan p = forced(RHMC_KERNEL_GENERIC, Op::Step, 51, 4096);
    CHECK(p.family == Family::Slotted && p.policy == Policy::WinG && p.path == 0);
    p = forced(RHMC_KERNEL_GENERIC, Op::Step, 2, 1024, true, 256);
    CHECK(p.family == Family::Slotted && p.policy == Policy::WinG);
    for (Op op : {Op::Integrate, Op::HmcRandom}) {
      p = forced(RHMC_KERNEL_GENERIC, op, 1, 4096);
      CHECK(p.family == Family::Slotted && p.policy == Policy::WinG && p.path == 0);
    }
    CHECK(forced(RHMC_KERNEL_GENERIC, Op::MhFused, 1, 4096).family == Family::None);
    CHECK(forced(RHMC_KERNEL_GENERIC, Op::MhFused, 10, 4096).family == Family::None);
    // WINDOWED: the windowed slotted kernel for every call
    for (Op op : {Op::Step, Op::Integrate, Op::HmcRandom, Op::Energy, Op::Gradient})
      for (int K : {1, 10, 51}) {
        p = forced(RHMC_KERNEL_WINDOWED, op, K, 4096);
        CHECK(p.family == Family::Slotted && p.path == 0 &&
              p.policy == (op == Op::Energy ? Policy::WinEG : Policy::WinG));
      }
    // REGWIN at every batch size; REGWIN32 the 32-px window; REGWIN_F64 the fp64 cache
    p = forced(RHMC_KERNEL_REGWIN, Op::Step, 1, 65536);
    CHECK(p.family == Family::RegWin1 && p.window == 28 && p.f32);
    CHECK(forced(RHMC_KERNEL_REGWIN, Op::MhFused, 1, 65536).family == Family::RegWin1);
    p = forced(RHMC_KERNEL_REGWIN32, Op::Step, 1, 65536);
    CHECK(p.family == Family::RegWin1 && p.window == 32 && p.f32);
    p = forced(RHMC_KERNEL_REGWIN_F64, Op::Step, 1, 65536);
    CHECK(p.family == Family::RegWin1 && p.window == 28 && !p.f32);
    // LANE1 / LANE4 at every batch size; LANE1_F64 the fp64 image
    p = forced(RHMC_KERNEL_LANE1, Op::Step, 1, 64);
    CHECK(p.family == Family::Lane && p.lpc == 1 && p.f32);
    p = forced(RHMC_KERNEL_LANE4, Op::Step, 1, 65536);
    CHECK(p.family == Family::Lane && p.lpc == 4 && p.f32);
    p = forced(RHMC_KERNEL_LANE1_F64, Op::Step, 1, 64);
    CHECK(p.family == Family::Lane && p.lpc == 1 && !p.f32);
    // PIXMAJOR is the AUTO choice where it serves; MULTIWIN takes those K too,
    // MULTIWIN_NOTAB without the LDS factor tables
    CHECK(forced(RHMC_KERNEL_PIXMAJOR, Op::Step, 10, 4096).family == Family::PixMajor);
    CHECK(forced(RHMC_KERNEL_PIXMAJOR, Op::MhFused, 10, 4096).family == Family::PixMajor);
    p = forced(RHMC_KERNEL_MULTIWIN, Op::Step, 10, 4096);
    CHECK(p.family == Family::MultiWin && p.tables && p.f32);
    CHECK(forced(RHMC_KERNEL_MULTIWIN, Op::MhFused, 10, 4096).family == Family::None);
    p = forced(RHMC_KERNEL_MULTIWIN_NOTAB, Op::Step, 10, 4096);
    CHECK(p.family == Family::MultiWin && !p.tables && p.slots == 1);
    p = forced(RHMC_KERNEL_MULTIWIN, Op::Step, 24, 4096);  // instead of the dense kernel
    CHECK(p.family == Family::MultiWin && !p.tables);
    // DENSE at any K on 32/48 px; a family that does not serve leaves AUTO
    for (int K : {1, 10, 256}) {
      p = forced(RHMC_KERNEL_DENSE, Op::Step, K, 4096);
      CHECK(p.family == Family::Slotted && p.policy == Policy::DenseG && p.path == 48);
    }
    p = forced(RHMC_KERNEL_DENSE, Op::Step, 51, 4096, true, 64);
    CHECK(p.family == Family::MultiWin);
    p = forced(RHMC_KERNEL_LANE1, Op::Step, 10, 4096);
    CHECK(p.family == Family::PixMajor);
  }

  // the MH loop's begin / end and the chain turn: a wave per chain from 8 stars
  CHECK(!mh_wave(1) && !mh_wave(7) && mh_wave(8) && mh_wave(1024));

  {  // ragged families: 1 dense, 2 windowed, 3 pixel-major, 0 fixed K per launch
    const SelectIn s48 = image(48, true), s48d = image(48, false), s64 = image(64, true);
    CHECK(ragged_family(s48, noVc, ref, 11) == 1 && ragged_family(s48, noVc, ref, 256) == 1);
    CHECK(ragged_family(s48, noVc, ref, 2) == 3 && ragged_family(s48, noVc, ref, 10) == 3);
    CHECK(ragged_family(s48, noVc, ref, 1) == 0);
    CHECK(ragged_family(s48d, noVc, ref, 5) == 0);   // multi-star register-window
    CHECK(ragged_family(s64, noVc, ref, 40) == 0);   // multi-star register-window
    CHECK(ragged_family(s64, noVc, ref, 65) == 2 && ragged_family(s64, noVc, ref, 1024) == 2);
    CHECK(ragged_family(s48, noVc, ref, 300) == 2);  // past the dense kernel's 256
    CHECK(ragged_family(s64, noVc, wide, 65) == 0);  // unsupported PSF
    CHECK(ragged_family(s48, noVc, ref, 0) == 0 && ragged_family(s48, noVc, ref, 1025) == 0);
  }

  if (g_failed) {
    std::fprintf(stderr, "%d selection rows failed\n", g_failed);
    return 1;
  }
  std::puts("select ok");
  return 0;
}
