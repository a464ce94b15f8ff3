// traj_bodies.cpp — which kernel body serves a random-length trajectory
// (rhmc_hmc_random, rhmc_diag_random) or, with the leading word `integrate`,
// an explicit integrator (rhmc_integrate with RHMC_SOLVER_HMC, _RHMC_NAIVE or
// _RHMC_LEAPFROG).  Host-only, csrc/rhmc_select.hpp alone: select(...,
// Op::HmcRandom or Op::Integrate, ...) gives the plan, and body_key() names the
// instantiation that csrc/rhmc_launch.hpp's switches (launch_hmc_random_t or
// launch_integrate, then launch_k1_w28, launch_multi, launch_kr, with_path)
// launch for it; the integrators build each body once per solver:
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
// With the leading word `step`, the implicit generalized-leapfrog step
// (rhmc_leapfrog, Op::Step), whose body also depends on the chain count (the
// lane-group kernel by kLaneChains*, kr_window_split), on
// RHMC_OPT_WINDOW_SPLIT and on the PSF width (the 32-px one-star window by
// rule).  step_key() follows launch_leapfrog (launch_tiledr, launch_tiledl,
// launch_multi, launch_kr_t, launch_leap_slotted, launch_lds_image):
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
// With the leading word `energy`, `gradient` or `mh`: rhmc_energy (Op::Energy),
// rhmc_gradient (Op::Gradient) and the Metropolis-Hastings loop rhmc_mh
// (Op::MhFused, then the four-kernel loop).  The pair potential changes the
// energy's body (one star with it leaves the register window), so use_Vc is
// an input; rhmc_mh takes RHMC_OPT_MH_FUSED in its place.  energy_key() follows
// launch_energy (launch_k1_w28, launch_energy_slotted, with_energy_win,
// launch_energy_lds_image), gradient_key() launch_gradient (launch_lds_image,
// with_path), mh_key() run_mh (launch_mh_k1, launch_mh_pk, else the loop):
//   regwin1/IMG/DT                energy_k1_tiledr<IMG, DT>
//   ldsimage/MAXK                 energy_kernel<MAXK>, gradient_kernel<MAXK>
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
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

#include "rhmc_select.hpp"

using namespace rhmc;

// MI355X: 160 KB of LDS per workgroup, 256 compute units.
static SelectIn image(int side, bool f32, int kernel) {
  SelectIn s;
  s.rows = s.cols = side;
  s.img_f32 = f32;
  s.max_lds = 160 * 1024;
  s.n_cu = 256;
  s.kernel = kernel;
  return s;
}

static std::string body_key(Op op, const SelectIn& s, int K, int64_t n) {
  const double sigma = 3.5 / 2.354;  // the reference PSF, FWHM 3.5 px
  const Plan pl = select(s, /*use_Vc*/ false, 1.0 / (2.0 * sigma * sigma), op, K, n);
  const std::string side = std::to_string(s.rows);
  switch (pl.family) {
    case Family::Unsupported: return "Unsupported";
    case Family::RegWin1:  // launch_k1_w28: with_side3, the 28-px window
      if (s.rows != 32 && s.rows != 48 && s.rows != 64) return "regwin1/no-such-side";
      return "regwin1/" + side + (pl.f32 ? "/float" : "/double");
    case Family::PixMajor:  // launch_multi: with_side2
      if (s.rows != 32 && s.rows != 48) return "pixmajor/no-such-side";
      return "pixmajor/" + side;
    case Family::MultiWin: {  // launch_kr, one wave per chain pair
      const char* dt = pl.f32 ? "float" : "double";
      if (pl.split != 1) return "multiwin/split";
      if (pl.tables) return std::string("multiwin/") + dt + "/1/tab";
      return std::string("multiwin/") + dt + (pl.slots == 1 ? "/1/notab" : "/2/notab");
    }
    default: break;  // launch_hmc_random_t, launch_integrate: everything else goes with_path
  }
  if (pl.path == 32 || pl.path == 48) {  // with_slots: 1, 2, else 4
    const int sl = win_slots(K);
    return "slotted/Dense" + std::to_string(pl.path) + "/" + std::to_string(sl <= 2 ? sl : 4);
  }
  if (K >= kWinGlobalFromK) {  // with_big
    const int sl = K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
    return "slotted/WinGG/" + std::to_string(sl);
  }
  return "slotted/WinG/1";
}

static double inv_two_sig2_of(double fwhm) {
  const double sigma = fwhm / 2.354;
  return 1.0 / (2.0 * sigma * sigma);
}

static std::string step_key(const SelectIn& s, int K, int64_t n, double fwhm) {
  const Plan pl = select(s, /*use_Vc*/ false, inv_two_sig2_of(fwhm), Op::Step, K, n);
  const std::string side = std::to_string(s.rows);
  const char* dt = pl.f32 ? "float" : "double";
  switch (pl.family) {
    case Family::Unsupported: return "Unsupported";
    case Family::RegWin1:  // with_side5, launch_tiledr: the plan's window and pixel cache
      if (s.rows != 32 && s.rows != 48 && s.rows != 64 && s.rows != 96 && s.rows != 128)
        return "regwin1/no-such-side";
      if (pl.window != 28 && pl.window != 32) return "regwin1/no-such-window";
      return "regwin1/" + side + "/" + std::to_string(pl.window) + "/" + dt;
    case Family::Lane:  // with_side3, launch_tiledl
      if (s.rows != 32 && s.rows != 48 && s.rows != 64) return "lane/no-such-side";
      if (pl.lpc != 1 && pl.lpc != 4) return "lane/no-such-lpc";
      return "lane/" + side + "/" + dt + "/" + std::to_string(pl.lpc);
    case Family::PixMajor:  // launch_multi: with_side2
      if (s.rows != 32 && s.rows != 48) return "pixmajor/no-such-side";
      return "pixmajor/" + side;
    case Family::MultiWin: {  // launch_kr, launch_kr_t: the split only without LDS tables
      if (pl.tables) return std::string("multiwin/") + dt + "/1/tab";
      const int ws = pl.split == 2 || pl.split == 4 ? pl.split : 1;
      return std::string("multiwin/") + dt + (pl.slots == 1 ? "/1" : "/2") + "/notab/" +
             std::to_string(ws);
    }
    case Family::LdsImage:  // launch_lds_image: the next power of two
      return "ldsimage/" + std::to_string(K == 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16);
    case Family::Slotted: break;  // launch_leap_slotted: with_path
    default: return "no-such-family";
  }
  if (pl.path == 32 || pl.path == 48) {  // with_slots: 1, 2, else 4
    const int sl = win_slots(K);
    return "slotted/Dense" + std::to_string(pl.path) + "/" + std::to_string(sl <= 2 ? sl : 4);
  }
  if (K >= kWinGlobalFromK) {  // with_big
    const int sl = K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
    return "slotted/WinGG/" + std::to_string(sl);
  }
  return "slotted/WinG/1";
}

// A PSF inside (3.555, 4.06] px FWHM: reg_window_ok(32) holds, reg_window_ok(28)
// does not, and the 32-px windows of the slotted kernels are not exact
// (window_exact), so a shape only they could serve is unsupported by rule.
static const double kWideFwhm = 3.8;

static int step_main(int argc, char** argv, const char* prog) {
  if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
    std::set<std::string> keys;
    for (int side : {32, 40, 48, 64, 96, 128, 256})
      for (int K = 1; K <= kMaxK; ++K)
        for (int f32 = 0; f32 < 2; ++f32)
          for (int kernel = RHMC_KERNEL_AUTO; kernel <= RHMC_KERNEL_DENSE; ++kernel)
            for (int64_t n : {(int64_t)4, (int64_t)16384, (int64_t)65536})
              for (int ws : {0, 1, 2, 4})
                for (double fwhm : {3.5, kWideFwhm}) {
                  SelectIn s = image(side, f32 != 0, kernel);
                  s.window_split = ws;
                  const std::string k = step_key(s, K, n, fwhm);
                  if (k == "Unsupported" && !window_exact(inv_two_sig2_of(fwhm))) continue;
                  keys.insert(k);
                }
    for (const std::string& k : keys) std::puts(k.c_str());
    return 0;
  }
  if (argc < 8 || (argc - 1) % 7 != 0) {
    std::fprintf(stderr,
                 "usage: %s step sweep | side K img_f32 kernel n_chains window_split fwhm [...]\n",
                 prog);
    return 2;
  }
  for (int i = 1; i + 6 < argc; i += 7) {
    SelectIn s = image(std::atoi(argv[i]), std::atoi(argv[i + 2]) != 0, std::atoi(argv[i + 3]));
    s.window_split = std::atoi(argv[i + 5]);
    std::puts(step_key(s, std::atoi(argv[i + 1]), std::atoll(argv[i + 4]),
                       std::atof(argv[i + 6])).c_str());
  }
  return 0;
}

// The slotted launchers' switch (with_path; with_energy_win for the windowed
// energy, whose one-slot policy is WinEG): `one_slot` names that policy.
static std::string slotted_key(const Plan& pl, int K, const char* one_slot) {
  if (pl.path == 32 || pl.path == 48) {  // with_slots: 1, 2, else 4
    const int sl = win_slots(K);
    return "slotted/Dense" + std::to_string(pl.path) + "/" + std::to_string(sl <= 2 ? sl : 4);
  }
  if (K >= kWinGlobalFromK) {  // with_big
    const int sl = K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
    return "slotted/WinGG/" + std::to_string(sl);
  }
  return std::string("slotted/") + one_slot + "/1";
}

static std::string lds_image_key(int K) {  // launch_lds_image: the next power of two
  return "ldsimage/" + std::to_string(K == 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16);
}

static std::string energy_key(const SelectIn& s, int K, int64_t n, bool use_Vc, double fwhm) {
  const Plan pl = select(s, use_Vc, inv_two_sig2_of(fwhm), Op::Energy, K, n);
  switch (pl.family) {
    case Family::Unsupported: return "Unsupported";
    case Family::RegWin1:  // launch_k1_w28: with_side3, the 28-px window
      if (s.rows != 32 && s.rows != 48 && s.rows != 64) return "regwin1/no-such-side";
      return "regwin1/" + std::to_string(s.rows) + (pl.f32 ? "/float" : "/double");
    case Family::Slotted:  // launch_energy_slotted: with_path, or with_energy_win
      return slotted_key(pl, K, "WinEG");
    default: return lds_image_key(K);  // launch_energy's default: launch_energy_lds_image
  }
}

static std::string gradient_key(const SelectIn& s, int K, int64_t n, bool use_Vc, double fwhm) {
  const Plan pl = select(s, use_Vc, inv_two_sig2_of(fwhm), Op::Gradient, K, n);
  if (pl.family == Family::Unsupported) return "Unsupported";
  if (pl.family != Family::Slotted) return lds_image_key(K);  // launch_gradient's first branch
  return slotted_key(pl, K, "WinG");                          // with_path
}

// s.mh_fused holds RHMC_OPT_MH_FUSED; run_mh has no pair-potential argument of
// its own here (the fused kernels do not serve it), so use_Vc is off.
static std::string mh_key(const SelectIn& s, int K, int64_t n, double fwhm) {
  const double its = inv_two_sig2_of(fwhm);
  const Plan fused = select(s, /*use_Vc*/ false, its, Op::MhFused, K, n);
  if (fused.family == Family::RegWin1) {  // launch_mh_k1: launch_k1_w28
    if (s.rows != 32 && s.rows != 48 && s.rows != 64) return "mh/regwin1/no-such-side";
    return "mh/regwin1/" + std::to_string(s.rows) + (fused.f32 ? "/float" : "/double");
  }
  if (fused.family == Family::PixMajor) {  // launch_mh_pk: with_side2
    if (s.rows != 32 && s.rows != 48) return "mh/pixmajor/no-such-side";
    return "mh/pixmajor/" + std::to_string(s.rows);
  }
  if (fused.family != Family::None) return "mh/no-such-family";
  // the four-kernel loop: its step and its energy must have a plan
  if (select(s, false, its, Op::Step, K, n).family == Family::Unsupported ||
      select(s, false, its, Op::Energy, K, n).family == Family::Unsupported)
    return "Unsupported";
  // run_mh: `const bool wave_mh = K >= 8;` (one thread per chain below, one
  // wave per chain from 8 stars); the switch lives there, not in rhmc_select.hpp
  return K >= 8 ? "mh/loop/wave" : "mh/loop/thread";
}

// mode 0 energy, 1 gradient, 2 mh; `flag` is use_Vc (mh: RHMC_OPT_MH_FUSED)
static std::string op_key(int mode, SelectIn s, int K, int64_t n, int flag, double fwhm) {
  if (mode == 0) return energy_key(s, K, n, flag != 0, fwhm);
  if (mode == 1) return gradient_key(s, K, n, flag != 0, fwhm);
  s.mh_fused = flag;
  return mh_key(s, K, n, fwhm);
}

static int op_main(int mode, int argc, char** argv, const char* prog) {
  if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
    std::set<std::string> keys;
    for (int side : {32, 40, 48, 64, 96, 256})
      for (int K = 1; K <= kMaxK; ++K)
        for (int f32 = 0; f32 < 2; ++f32)
          for (int kernel = RHMC_KERNEL_AUTO; kernel <= RHMC_KERNEL_DENSE; ++kernel)
            for (int64_t n : {(int64_t)4, (int64_t)65536})
              for (int flag = 0; flag < 2; ++flag)
                for (double fwhm : {3.5, kWideFwhm}) {
                  const std::string k =
                      op_key(mode, image(side, f32 != 0, kernel), K, n, flag, fwhm);
                  if (k == "Unsupported" && !window_exact(inv_two_sig2_of(fwhm))) continue;
                  keys.insert(k);
                }
    for (const std::string& k : keys) std::puts(k.c_str());
    return 0;
  }
  if (argc < 8 || (argc - 1) % 7 != 0) {
    std::fprintf(stderr, "usage: %s %s sweep | side K img_f32 kernel n_chains %s fwhm [...]\n",
                 prog, mode == 0 ? "energy" : mode == 1 ? "gradient" : "mh",
                 mode == 2 ? "mh_fused" : "use_Vc");
    return 2;
  }
  for (int i = 1; i + 6 < argc; i += 7)
    std::puts(op_key(mode, image(std::atoi(argv[i]), std::atoi(argv[i + 2]) != 0,
                                 std::atoi(argv[i + 3])),
                     std::atoi(argv[i + 1]), std::atoll(argv[i + 4]), std::atoi(argv[i + 5]),
                     std::atof(argv[i + 6])).c_str());
  return 0;
}

int main(int argc, char** argv) {
  const char* prog = argv[0];
  if (argc > 1 && !std::strcmp(argv[1], "step")) return step_main(argc - 1, argv + 1, prog);
  for (int mode = 0; mode < 3; ++mode)
    if (argc > 1 && !std::strcmp(argv[1], mode == 0 ? "energy" : mode == 1 ? "gradient" : "mh"))
      return op_main(mode, argc - 1, argv + 1, prog);
  Op op = Op::HmcRandom;
  if (argc > 1 && !std::strcmp(argv[1], "integrate")) {
    op = Op::Integrate;
    --argc;
    ++argv;
  }
  if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
    std::set<std::string> keys;
    for (int side : {32, 48, 64, 96})
      for (int K = 1; K <= kMaxK; ++K)
        for (int f32 = 0; f32 < 2; ++f32)
          for (int kernel = RHMC_KERNEL_AUTO; kernel <= RHMC_KERNEL_DENSE; ++kernel)
            for (int64_t n : {(int64_t)4, (int64_t)65536})
              keys.insert(body_key(op, image(side, f32 != 0, kernel), K, n));
    for (const std::string& k : keys) std::puts(k.c_str());
    return 0;
  }
  if (argc < 6 || (argc - 1) % 5 != 0) {
    std::fprintf(stderr, "usage: %s [integrate] sweep | side K img_f32 kernel n_chains [...]\n",
                 prog);
    return 2;
  }
  for (int i = 1; i + 4 < argc; i += 5) {
    const int side = std::atoi(argv[i]), K = std::atoi(argv[i + 1]);
    const bool f32 = std::atoi(argv[i + 2]) != 0;
    const int kernel = std::atoi(argv[i + 3]);
    const int64_t n = std::atoll(argv[i + 4]);
    std::puts(body_key(op, image(side, f32, kernel), K, n).c_str());
  }
  return 0;
}
