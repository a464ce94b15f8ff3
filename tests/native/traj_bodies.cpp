// traj_bodies.cpp — which kernel body serves a call, asked of the library's own
// dispatch.  Host-only, csrc/rhmc_select.hpp and csrc/rhmc_dispatch.hpp alone:
// select() gives the plan, and the switch of rhmc_dispatch.hpp that the
// operation's launcher (csrc/rhmc_launch.hpp) calls for the plan's family turns
// it into template arguments; here its functor names the tags where the
// launcher's enqueues the kernel.  What this program knows of the launchers is
// which switch serves which (operation, family): family_key() and mh_key().
//
// The operation is the leading word; none: a random-length trajectory
// (rhmc_hmc_random, rhmc_diag_random; launch_hmc_random_t), `integrate`: an
// explicit integrator (launch_integrate, each body built once per solver):
//   regwin1/IMG/DT          (diag_)hmc_random_k1_tiledr<IMG, DT>
//                           integrate_k1_tiledr<IMG, 28, DT, SOLVER>
//   pixmajor/IMG            leapfrog_pk<IMG, 10, SOLVER>
//   multiwin/DT/SLOTS/TAB   leapfrog_kr<DT, SLOTS, TAB, SOLVER, 1>
//   slotted/POLICY/SLOTS    (diag_)hmc_random_win_kernel<G, SLOTS>
//                           integrate_win_kernel<G, SOLVER, SLOTS>
// Built and run by tests/test_traj_bodies.py and tests/test_integrate_bodies.py.
//   traj_bodies [integrate] sweep                                  the distinct keys
//   traj_bodies [integrate] side K img_f32 kernel n_chains [...]   one key per group of five
//
// `step`: the implicit generalized-leapfrog step (rhmc_leapfrog,
// launch_leapfrog), whose body also depends on the chain count (the lane-group
// kernel, the window split), on RHMC_OPT_WINDOW_SPLIT and on the PSF width
// (the 32-px one-star window by rule):
//   regwin1/IMG/WIN/DT            leapfrog_k1_tiledr<IMG, WIN, DT>
//   lane/IMG/DT/LPC               leapfrog_k1_tiledl<IMG, 28, DT, LPC>
//   pixmajor/IMG                  leapfrog_pk<IMG, 10, IMPLICIT>
//   multiwin/DT/1/tab             leapfrog_kr<DT, 1, true, IMPLICIT, 1>
//   multiwin/DT/SLOTS/notab/WS    leapfrog_kr<DT, SLOTS, false, IMPLICIT, WS>
//   ldsimage/MAXK                 leapfrog_kernel<MAXK>
//   slotted/POLICY/SLOTS          leapfrog_win_kernel<G, SLOTS>
// Built and run by tests/test_step_bodies.py.
//   traj_bodies step sweep                                                    the distinct keys
//   traj_bodies step side K img_f32 kernel n_chains window_split fwhm [...]   one key per seven
//
// `energy`, `gradient`, `mh`: rhmc_energy (launch_energy), rhmc_gradient
// (launch_gradient) and the Metropolis-Hastings loop rhmc_mh (run_mh:
// Op::MhFused, then the four-kernel loop).  The pair potential changes the
// energy's body (one star with it leaves the register window), so use_Vc is
// an input; rhmc_mh takes RHMC_OPT_MH_FUSED in its place:
//   regwin1/IMG/DT                energy_k1_tiledr<IMG, DT>
//   ldsimage/MAXK                 energy_ / gradient_win_kernel<LdsG<MAXK>, 1>
//   slotted/WinEG/1               energy_win_kernel<WinEG, 1>
//   slotted/WinG/1                gradient_win_kernel<WinG, 1>
//   slotted/WinGG/SLOTS           energy_ / gradient_win_kernel<WinGG, SLOTS>
//   slotted/DenseIMG/SLOTS        energy_ / gradient_win_kernel<DenseG<IMG>, SLOTS>
//   mh/regwin1/IMG/DT             mh_k1_tiledr<IMG, 28, DT>
//   mh/pixmajor/IMG               mh_pk_v0<IMG, 10> and mh_pk_iter<IMG, 10>
//   mh/loop/thread                mh_begin_kernel, mh_end_kernel
//   mh/loop/wave                  mh_begin_wave_kernel, mh_end_wave_kernel
// Built and run by tests/test_energy_bodies.py.
//   traj_bodies energy|gradient sweep                                          the distinct keys
//   traj_bodies energy|gradient side K img_f32 kernel n_chains use_Vc fwhm [...]   one per seven
//   traj_bodies mh sweep
//   traj_bodies mh side K img_f32 kernel n_chains mh_fused fwhm [...]
//
// `ragged`: a ragged chain set (rhmc_leapfrog_ragged_device, launch_leapfrog_ragged;
// rhmc_energy_ragged_device, launch_energy_ragged).  K is the launch's K_max,
// whose plans the two launchers take; `none` where ragged_family() is 0, else
// the step's body and the energy's, STEP|ENERGY:
//   pixmajor/IMG/ragged           leapfrog_pk<IMG, 10, IMPLICIT, true>
//   slotted/POLICY/SLOTS          leapfrog_win_kernel<G, SLOTS>
//   ldsimage/MAXK | slotted/...   energy_win_kernel<G, SLOTS>
// Built and run by tests/test_ragged_bodies.py.
//   traj_bodies ragged sweep                                          the distinct pairs
//   traj_bodies ragged side K img_f32 kernel n_chains use_Vc fwhm [...]   one pair per seven
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "rhmc_dispatch.hpp"

using namespace rhmc;

// The tags' names in a key.
static std::string str(TypeTag<float>) { return "float"; }
static std::string str(TypeTag<double>) { return "double"; }
static std::string str(TypeTag<WinG>) { return "WinG"; }
static std::string str(TypeTag<WinEG>) { return "WinEG"; }
static std::string str(TypeTag<WinGG>) { return "WinGG"; }
template <int N> static std::string str(IntTag<N>) { return std::to_string(N); }
template <int IMG> static std::string str(TypeTag<DenseG<IMG>>) {
  return "Dense" + std::to_string(IMG);
}
template <int MAXK> static std::string str(TypeTag<LdsG<MAXK>>) { return std::to_string(MAXK); }

// The body that the launcher of `op` runs for a plan of a kernel family on an
// image of `side` px.  A tag IMG other than the side is no kernel of that image.
static std::string family_key(Op op, const Plan& pl, int side) {
  const bool step = op == Op::Step;
  auto sided = [&](const char* family, int img, const std::string& rest) {
    return family + (img == side ? "/" + std::to_string(img) + rest : "/no-such-side");
  };
  switch (pl.family) {
    case Family::Unsupported: return "Unsupported";
    case Family::RegWin1:
      if (step)  // launch_tiledr
        return with_regwin1(pl, side, [&](auto img, auto win, auto dt) {
          return sided("regwin1", img.value, "/" + str(win) + "/" + str(dt));
        });
      return with_k1_w28(pl, side, [&](auto img, auto dt) {  // launch_k1_w28
        return sided("regwin1", img.value, "/" + str(dt));
      });
    case Family::Lane:  // launch_tiledl
      return with_lane(pl, side, [&](auto img, auto dt, auto lpc) {
        return sided("lane", img.value, "/" + str(dt) + "/" + str(lpc));
      });
    case Family::PixMajor:  // launch_multi, launch_mh_pk
      return with_side2(side, [&](auto img) { return sided("pixmajor", img.value, ""); });
    case Family::MultiWin: {  // launch_kr: the split belongs to the implicit step's key
      auto name = [&](auto dt, auto slots, auto tab, auto ws) {
        const std::string k = "multiwin/" + str(dt) + "/" + str(slots);
        if (tab.value) return k + "/tab";
        return k + (step ? "/notab/" + str(ws) : "/notab");
      };
      return step ? with_multiwin<true>(pl, name) : with_multiwin<false>(pl, name);
    }
    case Family::LdsImage: {  // launch_leapfrog; launch_energy_slotted, launch_gradient
      auto name = [](auto g, auto) { return "ldsimage/" + str(g); };
      if (op == Op::Step) return with_maxk(pl, [](auto maxk) { return "ldsimage/" + str(maxk); });
      if (op == Op::Energy) return with_perwave_energy_policy(pl, name);
      if (op == Op::Gradient) return with_perwave_policy(pl, name);
      return std::string("ldsimage/no-such-kernel");  // no other operation has one
    }
    default: break;
  }
  auto name = [](auto g, auto slots) { return "slotted/" + str(g) + "/" + str(slots); };
  if (op == Op::Energy) return with_perwave_energy_policy(pl, name);  // launch_energy_slotted
  return op == Op::Gradient ? with_perwave_policy(pl, name) : with_policy(pl, name);
}

static double inv_two_sig2_of(double fwhm) {
  const double sigma = fwhm / 2.354;
  return 1.0 / (2.0 * sigma * sigma);
}

// run_mh: a fused plan (launch_mh_k1, launch_mh_pk), else the four-kernel
// loop, whose step and energy must have a plan.  The fused kernels do not
// serve the pair potential, so use_Vc is off.
static std::string mh_key(const SelectIn& s, int K, int64_t n, double its) {
  const Plan fused = select(s, false, its, Op::MhFused, K, n);
  if (fused.family != Family::None) return "mh/" + family_key(Op::MhFused, fused, s.rows);
  if (select(s, false, its, Op::Step, K, n).family == Family::Unsupported ||
      select(s, false, its, Op::Energy, K, n).family == Family::Unsupported)
    return "Unsupported";
  return with_mh_wave(mh_wave(K), [](auto wave) {  // launch_mh_turn
    return std::string(wave.value ? "mh/loop/wave" : "mh/loop/thread");
  });
}

// launch_leapfrog_ragged: with_side2 for a pixel-major plan (the RAGGED
// instantiation), else launch_leap_slotted's with_policy; launch_energy_ragged:
// launch_energy_slotted's with_perwave_energy_policy.
static std::string ragged_key(const SelectIn& s, bool use_Vc, double its, int K, int64_t n) {
  if (!ragged_family(s, use_Vc, its, K)) return "none";
  const Plan st = select(s, use_Vc, its, Op::Step, K, n);
  const Plan en = select(s, use_Vc, its, Op::Energy, K, n);
  if (st.family == Family::Unsupported || en.family == Family::Unsupported) return "Unsupported";
  const std::string step =
      st.family == Family::PixMajor ? family_key(Op::Step, st, s.rows) + "/ragged"
      : st.family == Family::Slotted ? family_key(Op::Step, st, s.rows)
                                     : std::string("no-ragged-step");
  const std::string energy = en.family == Family::Slotted || en.family == Family::LdsImage
                                 ? family_key(Op::Energy, en, s.rows)
                                 : std::string("no-ragged-energy");
  return step + "|" + energy;
}

// A mode of the command line: its operation, the sweep's values and what the
// sixth argument of a point sets (none: five arguments, the reference PSF).
enum class Flag { None, WindowSplit, UseVc, MhFused };
struct Mode {
  const char* word;
  Op op;
  Flag flag;
  std::vector<int> sides;
  std::vector<int64_t> chains;
  std::vector<int> flags;
  std::vector<double> fwhms;
  bool ragged = false;   // a ragged set: ragged_key() of the step's and the energy's plans
};
// The reference PSF, FWHM 3.5 px, and 3.8 px, inside (3.555, 4.06]:
// reg_window_ok(32) holds, reg_window_ok(28) does not, and the 32-px windows of
// the slotted kernels are not exact (window_exact), so a shape only they could
// serve is unsupported by rule.
static const std::vector<double> kRefFwhm = {3.5}, kBothFwhm = {3.5, 3.8};
static const std::vector<int> kOpSides = {32, 40, 48, 64, 96, 256};
static const Mode kModes[] = {
    {"integrate", Op::Integrate, Flag::None, {32, 48, 64, 96}, {4, 65536}, {0}, kRefFwhm},
    {"step", Op::Step, Flag::WindowSplit, {32, 40, 48, 64, 96, 128, 256}, {4, 16384, 65536},
     {0, 1, 2, 4}, kBothFwhm},
    {"energy", Op::Energy, Flag::UseVc, kOpSides, {4, 65536}, {0, 1}, kBothFwhm},
    {"gradient", Op::Gradient, Flag::UseVc, kOpSides, {4, 65536}, {0, 1}, kBothFwhm},
    {"mh", Op::MhFused, Flag::MhFused, kOpSides, {4, 65536}, {0, 1}, kBothFwhm},
    // 24 px: below the register kernels' 32, the windowed kernel by rule from 17 stars
    {"ragged", Op::Step, Flag::UseVc, {24, 32, 40, 48, 64, 96, 256}, {4, 65536}, {0, 1}, kBothFwhm,
     true},
    {nullptr, Op::HmcRandom, Flag::None, {32, 48, 64, 96}, {4, 65536}, {0}, kRefFwhm},
};

// MI355X: 160 KB of LDS per workgroup, 256 compute units.
static std::string point_key(const Mode& m, int side, int K, bool f32, int kernel, int64_t n,
                             int flag, double fwhm) {
  SelectIn s;
  s.rows = s.cols = side;
  s.img_f32 = f32;
  s.max_lds = 160 * 1024;
  s.n_cu = 256;
  s.kernel = kernel;
  if (m.flag == Flag::WindowSplit) s.window_split = flag;
  if (m.flag == Flag::MhFused) s.mh_fused = flag;
  const double its = inv_two_sig2_of(fwhm);
  if (m.op == Op::MhFused) return mh_key(s, K, n, its);
  if (m.ragged) return ragged_key(s, flag != 0, its, K, n);
  return family_key(m.op, select(s, m.flag == Flag::UseVc && flag, its, m.op, K, n), side);
}

int main(int argc, char** argv) {
  const char* prog = argv[0];
  const Mode* m = kModes;
  while (m->word && !(argc > 1 && !std::strcmp(argv[1], m->word))) ++m;
  if (m->word) {
    --argc;
    ++argv;
  }
  const bool flagged = m->flag != Flag::None;
  if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
    std::set<std::string> keys;
    for (int side : m->sides)
      for (int K = 1; K <= kMaxK; ++K)
        for (int f32 = 0; f32 < 2; ++f32)
          for (int kernel = RHMC_KERNEL_AUTO; kernel <= RHMC_KERNEL_DENSE; ++kernel)
            for (int64_t n : m->chains)
              for (int flag : m->flags)
                for (double fwhm : m->fwhms) {
                  const std::string k = point_key(*m, side, K, f32 != 0, kernel, n, flag, fwhm);
                  if (k == "Unsupported" && !window_exact(inv_two_sig2_of(fwhm))) continue;
                  if (k == "none") continue;  // no ragged family: one packed call per K
                  keys.insert(k);
                }
    for (const std::string& k : keys) std::puts(k.c_str());
    return 0;
  }
  const int per = flagged ? 7 : 5;
  if (argc < per + 1 || (argc - 1) % per != 0) {
    std::fprintf(stderr, "usage: %s [integrate|step|energy|gradient|mh|ragged] sweep | side K img_f32 "
                         "kernel n_chains [window_split|use_Vc|mh_fused fwhm] [...]\n", prog);
    return 2;
  }
  for (int i = 1; i + per - 1 < argc; i += per)
    std::puts(point_key(*m, std::atoi(argv[i]), std::atoi(argv[i + 1]), std::atoi(argv[i + 2]) != 0,
                        std::atoi(argv[i + 3]), std::atoll(argv[i + 4]),
                        flagged ? std::atoi(argv[i + 5]) : 0,
                        flagged ? std::atof(argv[i + 6]) : 3.5).c_str());
  return 0;
}
