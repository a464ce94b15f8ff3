// rhmc_select.hpp — which kernel family serves a call: the one place that
// holds the rule for (operation, K, image, PSF, batch size, RHMC_OPT_KERNEL).
// Plain C++17 with no HIP header, so a host compiler alone builds it (and its
// test, tests/native/select_check.cpp).  select() returns a Plan, which holds
// every value a kernel's template arguments depend on; rhmc_dispatch.hpp turns
// it into those arguments, and the launchers (rhmc_launch.hpp) add only launch
// mechanics (workgroup, LDS bytes, grid).  The operations differ on purpose;
// every difference is a commented row of op_rules() below, nowhere else.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rhmc.h"

namespace rhmc {

// ---- the pure arithmetic the rules read -----------------------------------

// exp(-(WIN/2)^2 / (2 sigma^2)) <= 2^-62 (62 ln 2 = 42.975)?
constexpr bool reg_window_ok(int win, double inv_two_sig2) {
  return (0.5 * win) * (0.5 * win) * inv_two_sig2 >= 42.98;
}

// The 32-pixel windows (rhmc_windowed.hpp) drop pixel
// centres >= 15.5 px from a star; exact to fp64 only while their PSF factor
// exp(-15.5^2 / (2 sigma^2)) <= 2^-70, i.e. sigma <= 1.574 px (reference: 1.487).
constexpr bool window_exact(double inv_two_sig2) { return 15.5 * 15.5 * inv_two_sig2 >= 48.5; }

constexpr const char* kWindowUnsupported =
    "PSF wider than the 32-pixel window allows (sigma > 1.574 px) for a configuration "
    "that needs the windowed kernels (K > 16 or image larger than LDS)";

// Doubles of one wave's separable PSF tables in the LDS-image kernels.
constexpr size_t table_doubles(int K, int rows, int cols) {
  return (size_t)2 * K * (rows + cols);
}

constexpr int kMaxKGeneric = 16;   // register accumulators of the LDS-image kernels
constexpr int kMaxKLds = 256;      // slotted kernels, LDS tables: 64 lanes x 4 star slots
constexpr int kMaxK = 1024;        // slotted kernels, global tables (WinGG): 8 / 16 slots
// The windowed path's first star count on the global-table policy (WinGG)
// instead of LDS tables (WinG, whose 2 K 33 doubles per wave cap a CU at one
// or two waves past 64 stars)
constexpr int kWinGlobalFromK = 65;

// Star slots per lane of the slotted kernels for K stars.
constexpr int win_slots(int K) {
  return K <= 64 ? 1 : K <= 128 ? 2 : K <= 256 ? 4 : K <= 512 ? 8 : 16;
}

// The dense many-star kernel (rhmc_dense.hpp) by default from kDenseMinK stars
// on 32/48-px square images (where every star's window covers most of the
// image).  Measured (4096 chains, 100 steps, chain-steps/s, profiles/r04_dense/):
// against the multi-star register-window kernel 32 px K = 12 1.15e8 vs 7.4e7,
// K = 24 8.1e7 vs 1.6e7; 48 px K = 12 5.6e7 vs 4.5e7, K = 24 3.6e7 vs 1.6e7,
// K = 40 2.3e7 vs 6.4e6; big-sim4 (32 px, K = 51) 5.1e7 vs 3.8e6, big-sim3
// (K = 100) 2.7e7 vs 1.7e5 for the windowed kernel.  At K <= 10 the
// pixel-major kernel stays (48 px K = 10: 2.2e8 vs 4.2e7).
constexpr int kDenseMinK = 11;

// Register accumulators of the LDS-image kernel for K stars: the next power of two.
constexpr int lds_image_maxk(int K) {
  return K == 1 ? 1 : K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : kMaxKGeneric;
}

// The MH loop's begin / end kernels and the chain turn: one thread per chain
// for few stars, one wave per chain (lanes over the coordinates) from 8 stars.
constexpr int kMhWaveFromK = 8;
constexpr bool mh_wave(int K) { return K >= kMhWaveFromK; }

// Lanes per chain of the lane-group kernel for a K = 1 batch of n chains, or 0
// for the register-window kernel.
// Measured (C2 geometry, 500 steps, chain-steps/s): 16384 chains tiledr
// 1.99e9 / LPC 4 2.25e9; 65536: 2.28e9 / LPC 1 3.06e9; 131072: 2.31e9 / 3.59e9.
constexpr int64_t kLaneChains1 = 65536;   // >= one 64-chain wave per SIMD
constexpr int64_t kLaneChains4 = 16384;   // >= one 16-chain wave per SIMD

// ---- inputs and result -----------------------------------------------------

// The context's part in the choice (rhmc_ctx: image, device, options).
struct SelectIn {
  int rows = 0, cols = 0;
  bool img_f32 = false;            // every pixel of D is exactly representable in fp32
  int max_lds = 0, n_cu = 0;
  int kernel = RHMC_KERNEL_AUTO;   // RHMC_OPT_KERNEL
  int mh_fused = 1;                // RHMC_OPT_MH_FUSED
  int window_split = 0;            // RHMC_OPT_WINDOW_SPLIT (0: by batch size)
  int peaks_fused = 1;             // RHMC_OPT_PEAKS_FUSED
  int dt_lanes = 0;                // RHMC_OPT_DT_LANES (0: the rule's choice)
};

enum class Op { Step, Integrate, HmcRandom, Energy, Gradient, MhFused, Peaks };

enum class Family {
  RegWin1,      // one-star register-window (rhmc_tiledr.hpp, rhmc_mhk1.hpp)
  Lane,         // one-star lane-group (rhmc_tiledl.hpp)
  PixMajor,     // pixel-major, 2-10 stars (rhmc_pixk.hpp, rhmc_mhpk.hpp)
  MultiWin,     // multi-star register-window (rhmc_tiledrk.hpp)
  Slotted,      // one wave per chain, a gradient policy (*_win_kernel)
  LdsImage,     // one wave per chain, image in LDS (K <= 16)
  None,         // MhFused: no fused kernel, the four-kernel loop runs;
                // Peaks: the stepwise path (gradient / update / energy launches)
  Unsupported   // message holds the error text (RHMC_ERR_UNSUPPORTED)
};

// The slotted kernels' gradient policy (rhmc_windowed.hpp, rhmc_dense.hpp).
enum class Policy { WinG, WinEG, WinGG, DenseG };

struct Plan {
  Family family = Family::LdsImage;
  // Slotted: 0 = windowed tables, 32 / 48 = the dense kernel at that side
  int path = 0;
  Policy policy = Policy::WinG;
  int slots = 1;         // Slotted, MultiWin: star slots per lane
  int maxk = kMaxKGeneric;  // LdsImage: register accumulators (1, 2, 4, 8, 16)
  int window = 28;       // RegWin1: 28- or 32-px window
  bool f32 = false;      // RegWin1, Lane, MultiWin: fp32 pixel cache
  int lpc = 0;           // Lane: lanes per chain (1 or 4)
  bool tables = false;   // MultiWin: PSF factor tables in LDS
  int split = 1;         // MultiWin: waves per chain pair (1, 2, 4)
  const char* message = nullptr;
};

// ---- the predicates --------------------------------------------------------

// GENERIC / WINDOWED force the one-wave-per-chain kernels for every call.
constexpr bool per_wave_forced(const SelectIn& s) {
  return s.kernel == RHMC_KERNEL_GENERIC || s.kernel == RHMC_KERNEL_WINDOWED;
}

// The LDS-image kernels need D and the per-wave tables in LDS and K <= 16;
// everything else one wave per chain goes windowed.
inline bool use_windowed(const SelectIn& s, int K) {
  if (K > kMaxKGeneric) return true;
  const size_t need =
      ((size_t)s.rows * s.cols + table_doubles(K, s.rows, s.cols)) * sizeof(double);
  return need > (size_t)s.max_lds || s.kernel == RHMC_KERNEL_WINDOWED;
}

// Multi-star register-window kernel (rhmc_tiledrk.hpp): K in [1, 64], square
// image of side >= 32, PSF narrow enough for the 28-row window.  The default
// wherever it applies (C3 with LDS factor tables: 18.0 ms per 100 steps
// against 20.3 for the full-image tiled kernel; C5: 3.2x the windowed kernel).
inline bool tiledrk_ok(const SelectIn& s, int K, double inv_two_sig2) {
  return K >= 1 && K <= 64 && s.rows == s.cols && s.rows >= 32 && reg_window_ok(28, inv_two_sig2);
}
inline bool use_tiledrk(const SelectIn& s, int K, double inv_two_sig2) {
  return !per_wave_forced(s) && tiledrk_ok(s, K, inv_two_sig2);
}

// Pixel-major multi-star kernel (rhmc_pixk.hpp): the default for 2 <= K <= 10
// on a 32/48-px fp32-exact image (C3: 1.23e8 chain-steps/s against 1.05e8 for
// the window-major kernel with LDS tables, measured A/B on one box).
// RHMC_KERNEL_MULTIWIN* force the window-major kernel, GENERIC / WINDOWED the
// per-wave ones.
inline bool use_pixk(const SelectIn& s, int K, bool use_Vc) {
  const int k = s.kernel;
  const bool want = !per_wave_forced(s) && k != RHMC_KERNEL_MULTIWIN &&
                    k != RHMC_KERNEL_MULTIWIN_NOTAB && k != RHMC_KERNEL_DENSE;
  return want && K >= 2 && K <= 10 && !use_Vc && s.img_f32 && s.rows == s.cols &&
         (s.rows == 32 || s.rows == 48);
}

// The dense kernel's side (32 / 48) for (K, image), or 0.  RHMC_KERNEL_DENSE
// forces it on those images at any K, GENERIC / WINDOWED keep the per-wave
// families, MULTIWIN(_NOTAB) keeps the multi-star register-window kernel where
// it applies (K <= 64).
inline int dense_path(const SelectIn& s, int K, double inv_two_sig2) {
  if (K > kMaxKLds) return 0;  // four register slots at most
  if (s.rows != s.cols || (s.rows != 32 && s.rows != 48)) return 0;
  if (per_wave_forced(s)) return 0;
  if (s.kernel != RHMC_KERNEL_DENSE) {
    if (K < kDenseMinK) return 0;
    if ((s.kernel == RHMC_KERNEL_MULTIWIN || s.kernel == RHMC_KERNEL_MULTIWIN_NOTAB) &&
        tiledrk_ok(s, K, inv_two_sig2))
      return 0;
  }
  return s.rows;
}

// RHMC_KERNEL_LANE1 / _LANE4 / _LANE1_F64 force the lane-group kernel,
// RHMC_KERNEL_REGWIN* turn it off; else by batch size (kLaneChains*).
inline int tiledl_lpc(int64_t n, int kern) {
  if (kern == RHMC_KERNEL_LANE1 || kern == RHMC_KERNEL_LANE1_F64) return 1;
  if (kern == RHMC_KERNEL_LANE4) return 4;
  if (kern == RHMC_KERNEL_REGWIN || kern == RHMC_KERNEL_REGWIN32 || kern == RHMC_KERNEL_REGWIN_F64)
    return 0;
  return n >= kLaneChains1 ? 1 : n >= kLaneChains4 ? 4 : 0;
}

// Factor tables in LDS (TiledRK<..., TAB>) for images up to 64 px with K <= 16,
// where every window overlaps (nearly) every star; RHMC_KERNEL_MULTIWIN_NOTAB
// forces the exp path there.
inline bool kr_tables(const SelectIn& s, int K) {
  return s.kernel != RHMC_KERNEL_MULTIWIN_NOTAB && s.rows <= 64 && K <= 16;
}

// Waves per chain pair for the implicit window-major kernel: the option, or
// the least of 1, 2, 4 that gives the launch eight waves per SIMD (four rounds
// of the kernel's two resident waves: finer rounds even out the waves' unequal
// neighbour work).  C5 sweep (profiles/r03_ws/, chain-steps/s, WS 1 / 2 / 4):
// 1024 chains 5.19e6 / 1.01e7 / 1.29e7, 2048 1.03e7 / 1.39e7 / 1.38e7,
// 4096 1.42e7 / 1.48e7 / 1.48e7, 8192 1.50e7 / 1.53e7 / 1.52e7,
// 16384 1.58e7 / 1.58e7 / 1.55e7.
inline int kr_window_split(const SelectIn& s, int64_t n_chains) {
  if (s.window_split) return s.window_split;
  const int64_t pairs = (n_chains + 1) / 2, target = 32 * (int64_t)(s.n_cu > 0 ? s.n_cu : 256);
  int ws = 1;
  while (ws < 4 && pairs * ws < target) ws *= 2;
  return ws;
}

// ---- what the operations do differently ------------------------------------

struct OpRules {
  bool k1_wide;     // one star: sides 96/128 too, and the 32-px window test
  bool lane;        // one star: the lane-group kernel by batch size / option
  bool k1_forcing;  // one star: REGWIN32 / REGWIN_F64 / LANE1_F64 are honoured
  bool k1;          // one star takes the register-window family at all
  bool multi;       // 2+ stars: the pixel-major / multi-star register-window kernels
  bool lds_image;   // falls back to the LDS-image kernels (else always slotted)
  Policy win_lds;   // windowed policy below kWinGlobalFromK stars
};

constexpr OpRules op_rules(Op op) {
  switch (op) {
    // The implicit step: the one-star register-window kernel on sides
    // 32/48/64/96/128 under the 32-px window test (the kernel then takes the
    // 28-px window where that is exact too), the lane-group kernel by batch
    // size on sides <= 64; every one-star forcing option applies.
    case Op::Step: return {true, true, true, true, true, true, Policy::WinG};
    // The explicit integrators and HMC_random: one star only on 32/48/64 px
    // under the 28-px test (only those instantiations exist), no lane-group
    // kernel whatever the batch, fp32 cache whenever the image allows; and
    // never the LDS-image kernels (there is no such integrator): what the
    // register kernels do not serve goes slotted.
    case Op::Integrate:
    case Op::HmcRandom: return {false, false, false, true, true, false, Policy::WinG};
    // Energy: one star as the integrators (energy_k1_tiledr); 2+ stars have
    // no register-kernel energy, so the per-wave kernels serve them, and the
    // windowed one needs only column tables (WinEG) below kWinGlobalFromK.
    case Op::Energy: return {false, false, false, true, false, true, Policy::WinEG};
    // Gradient (a host-buffer diagnostic): per-wave kernels only, full tables.
    case Op::Gradient: return {false, false, false, false, false, true, Policy::WinG};
    // Fused MH: see select_mh_fused.
    case Op::MhFused: break;
    // The seed descent of find_peaks: see select_peaks.
    case Op::Peaks: break;
  }
  return {false, false, false, false, false, false, Policy::WinG};
}

// One launch for the whole MH loop (K = 1, rhmc_mhk1.hpp) or one per iteration
// (2 <= K <= 10, rhmc_mhpk.hpp) where the step takes the register-window /
// pixel-major kernel: sides 32/48/64 under the 28-px test like the
// integrators, but unlike them it gives way to the lane-group kernel
// (tiledl_lpc must be 0).  RHMC_OPT_MH_FUSED = 0, or a forced kernel other
// than REGWIN (K = 1) / PIXMAJOR (K >= 2), keeps the four-kernel loop.
inline Plan select_mh_fused(const SelectIn& s, bool use_Vc, double inv_two_sig2, int K,
                            int64_t n) {
  Plan pl;
  pl.family = Family::None;
  if (!s.mh_fused) return pl;
  const int side = s.rows;
  if (K == 1) {
    if (s.kernel != RHMC_KERNEL_AUTO && s.kernel != RHMC_KERNEL_REGWIN) return pl;
    if (!use_Vc && s.rows == s.cols && (side == 32 || side == 48 || side == 64) &&
        reg_window_ok(28, inv_two_sig2) && tiledl_lpc(n, s.kernel) == 0) {
      pl.family = Family::RegWin1;
      pl.f32 = s.img_f32;
    }
    return pl;
  }
  if (s.kernel != RHMC_KERNEL_AUTO && s.kernel != RHMC_KERNEL_PIXMAJOR) return pl;
  if (use_pixk(s, K, use_Vc)) pl.family = Family::PixMajor;
  return pl;
}

// find_peaks' seed descent (rhmc_peaks.hpp), always one star per seed: the
// one-launch kernel on sides 32/48/64 under the 28-px test like the
// integrators (only those instantiations exist) and, like them, at every
// batch size (there is no lane-group descent).  RHMC_OPT_PEAKS_FUSED = 0, a
// forced per-wave family (GENERIC / WINDOWED) or any other configuration
// takes the stepwise path (Family::None): the K = 1 gradient and energy
// launches of this header's Gradient / Energy rows around peaks_update_kernel.
inline Plan select_peaks(const SelectIn& s, double inv_two_sig2) {
  Plan pl;
  pl.family = Family::None;
  if (!s.peaks_fused || per_wave_forced(s)) return pl;
  const int side = s.rows;
  if (s.rows == s.cols && (side == 32 || side == 48 || side == 64) &&
      reg_window_ok(28, inv_two_sig2)) {
    pl.family = Family::RegWin1;
    pl.f32 = s.img_f32;
  }
  return pl;
}

// The trial kernel of HMC_find_best_dt's search (rhmc_dt.hpp,
// dt_trials_kernel<lanes, ppl>): one task per workgroup of `lanes` lanes over
// the whole image.  Square sides 16..64 keep the lane's pixels of D and M in
// registers, ppl of each: ceil(side^2 / lanes) rounded up to an instantiated
// size (256 lanes: 4 / 9 / 16 for sides <= 32 / 48 / 64; 64 lanes: 16 for sides
// <= 32 only, the 36 pixels of D and of M per lane of a 48-px image spill: 276
// bytes of scratch per lane in the build that tried).  Every other side reads
// the pixels from global memory (ppl = 0) with factor tables in a global
// buffer, `blocks_cap` workgroups at most.  Lanes per task: 256
// unless RHMC_OPT_DT_LANES says 64 (the A/B of DESIGN.md section 4e); the
// calls that matter have one task per star and are bound by the serial chain
// of gradients, which 256 lanes make shorter.
struct DtPlan {
  int lanes = 256;
  int ppl = 0;           // pixels per lane in registers, 0: global memory
  int blocks_cap = 0;    // most workgroups of one launch
  const char* message = nullptr;   // set: RHMC_ERR_UNSUPPORTED
};

inline DtPlan select_dt(const SelectIn& s) {
  DtPlan pl;
  if (s.rows != s.cols || s.rows < 1) {
    pl.message = "dt_trials needs a square image";
    return pl;
  }
  const int side = s.rows;
  pl.lanes = s.dt_lanes == 64 ? 64 : 256;
  if (side >= 16 && side <= 64) {
    if (pl.lanes == 256) pl.ppl = side <= 32 ? 4 : (side <= 48 ? 9 : 16);
    else pl.ppl = side <= 32 ? 16 : 0;
  }
  pl.blocks_cap = pl.ppl ? 65536 : 4096;
  return pl;
}

// The Hessian-metric kernels (rhmc_hess.hpp: hess_derivs_kernel,
// hess_random_kernel): one wave per chain, pixel-major over the full image.
// LDS: the fp64 image once per workgroup, and per wave the four factor tables
// of rhmc_perwave.hpp (2 K (rows + cols) doubles), the 1 / Lambda image
// (side^2 doubles) and the stars' fluxes (kMaxKGeneric doubles).  Served:
// 1 <= K <= 16 on square images of side 16..48; `waves` is the largest of 4, 2,
// 1 waves per workgroup that fits the device's LDS (48 px: four waves up to 11
// stars, 160,256 B there; two from 12 stars, 104,704 B at 16).  RHMC_OPT_KERNEL
// does not enter.
constexpr int kHessMinSide = 16, kHessMaxSide = 48;

constexpr size_t hess_wave_doubles(int K, int side) {
  return table_doubles(K, side, side) + (size_t)side * side + kMaxKGeneric;
}

struct HessPlan {
  int waves = 0;                   // waves (chains) per workgroup
  size_t lds_bytes = 0;
  const char* message = nullptr;   // set: RHMC_ERR_UNSUPPORTED
};

inline HessPlan select_hess(const SelectIn& s, int K) {
  HessPlan pl;
  if (s.rows != s.cols || s.rows < kHessMinSide || s.rows > kHessMaxSide) {
    pl.message = "the Hessian-metric kernels serve square images of side 16..48";
    return pl;
  }
  if (K < 1 || K > kMaxKGeneric) {
    pl.message = "the Hessian-metric kernels serve 1 <= K <= 16";
    return pl;
  }
  const size_t img = (size_t)s.rows * s.cols;
  for (int W = 4; W >= 1; W >>= 1) {
    const size_t need = (img + W * hess_wave_doubles(K, s.rows)) * sizeof(double);
    if (need <= (size_t)s.max_lds) {
      pl.waves = W;
      pl.lds_bytes = need;
      return pl;
    }
  }
  pl.message = "the Hessian-metric kernels' image and tables exceed the device's LDS";
  return pl;
}

// The kernel family and its compile-time choices for one call.
inline Plan select(const SelectIn& s, bool use_Vc, double inv_two_sig2, Op op, int K,
                   int64_t n_chains) {
  if (op == Op::MhFused) return select_mh_fused(s, use_Vc, inv_two_sig2, K, n_chains);
  if (op == Op::Peaks) return select_peaks(s, inv_two_sig2);
  const OpRules r = op_rules(op);
  Plan pl;
  const int side = s.rows;
  // one star: the register-window kernel (C1, C2) or, from 16 Ki chains, the
  // lane-group kernel (C4 shards); wider PSFs and other image sides go on
  if (r.k1 && K == 1 && !use_Vc && s.rows == s.cols && !per_wave_forced(s) &&
      s.kernel != RHMC_KERNEL_DENSE) {
    const bool small = side == 32 || side == 48 || side == 64;
    const bool img_ok = small || (r.k1_wide && (side == 96 || side == 128));
    const bool w28 = reg_window_ok(28, inv_two_sig2);
    if (img_ok && (r.k1_wide ? reg_window_ok(32, inv_two_sig2) : w28)) {
      const int lpc = r.lane ? tiledl_lpc(n_chains, s.kernel) : 0;
      if (lpc && small && w28) {
        pl.family = Family::Lane;
        pl.lpc = lpc;
        pl.f32 = s.img_f32 && s.kernel != RHMC_KERNEL_LANE1_F64;
        return pl;
      }
      pl.family = Family::RegWin1;
      pl.window = w28 && !(r.k1_forcing && s.kernel == RHMC_KERNEL_REGWIN32) ? 28 : 32;
      pl.f32 = s.img_f32 && !(r.k1_forcing && s.kernel == RHMC_KERNEL_REGWIN_F64);
      return pl;
    }
  }
  pl.path = dense_path(s, K, inv_two_sig2);
  if (r.multi && !pl.path) {
    if (use_pixk(s, K, use_Vc)) {
      pl.family = Family::PixMajor;
      return pl;
    }
    if (use_tiledrk(s, K, inv_two_sig2)) {
      pl.family = Family::MultiWin;
      pl.f32 = s.img_f32;
      pl.tables = kr_tables(s, K);
      pl.slots = pl.tables || K <= 32 ? 1 : 2;
      // only the implicit step without LDS tables is built with a split
      pl.split = op == Op::Step && !pl.tables ? kr_window_split(s, n_chains) : 1;
      return pl;
    }
  }
  if (!pl.path && r.lds_image && !use_windowed(s, K)) {
    pl.family = Family::LdsImage;
    pl.maxk = lds_image_maxk(K);
    return pl;
  }
  if (!pl.path && !window_exact(inv_two_sig2)) {
    pl.family = Family::Unsupported;
    pl.message = kWindowUnsupported;
    return pl;
  }
  pl.family = Family::Slotted;
  pl.policy = pl.path ? Policy::DenseG : K >= kWinGlobalFromK ? Policy::WinGG : r.win_lds;
  pl.slots = win_slots(K);
  return pl;
}

// Ragged chain sets (rhmc.h: rhmc_leapfrog_ragged_device & co.; the
// reversible-jump driver).  Which star counts the automatic dispatch serves
// with a slotted one-wave-per-chain kernel — for both the step and the
// energy — where chains of different K can share a launch: 1 = the dense
// kernel (32/48-px images, from 11 stars), 2 = the windowed kernel, 3 = the
// pixel-major kernel (2-10 stars on 32/48-px fp32-exact images) with the
// LDS-image energy kernel; 0 = a kernel with a fixed K per launch (one-star,
// multi-star register-window).  A function of the two plans: the step and the
// energy of one K agree by construction.
inline int ragged_family(const SelectIn& s, bool use_Vc, double inv_two_sig2, int K) {
  if (K < 1 || K > kMaxK) return 0;
  const Plan step = select(s, use_Vc, inv_two_sig2, Op::Step, K, 1);
  const Plan en = select(s, use_Vc, inv_two_sig2, Op::Energy, K, 1);
  if (step.family == Family::Slotted && en.family == Family::Slotted && step.path == en.path) {
    if (step.path) return 1;
    return K == 1 ? 0 : 2;  // one star off the dense path: never a ragged set
  }
  if (step.family == Family::PixMajor && en.family == Family::LdsImage) return 3;
  return 0;
}

}  // namespace rhmc
