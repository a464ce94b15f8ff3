// rhmc_dispatch.hpp — from a Plan (rhmc_select.hpp) to the template arguments
// of the kernel that serves it: every run-time value -> template argument
// switch of the library, written once.  Plain C++17 with no HIP header; the
// launchers (rhmc_launch.hpp) pass functors that enqueue the kernel,
// tests/native/traj_bodies.cpp passes functors that name the tags, so the body
// tests ask the dispatch the library runs.  A switch reads the Plan (and the
// image side, which the plan does not hold), never K: what select() decided is
// not decided again here.  f's result is the switch's result.
#pragma once
#include "rhmc_select.hpp"

namespace rhmc {

// The slotted kernels' gradient policies (rhmc_perwave.hpp, rhmc_windowed.hpp,
// rhmc_dense.hpp); a tag of an incomplete type is enough for a switch.
template <int MAXK> struct LdsG;
struct WinG;
struct WinEG;
struct WinGG;
template <int IMG> struct DenseG;

template <class T> struct TypeTag { using type = T; };
template <int N> struct IntTag { static constexpr int value = N; };
template <bool B> struct BoolTag { static constexpr bool value = B; };

// The explicit integrators (launch_integrate has checked the range).
template <class F>
auto with_solver(int32_t solver, F&& f) {
  if (solver == RHMC_SOLVER_HMC) return f(IntTag<RHMC_SOLVER_HMC>{});
  if (solver == RHMC_SOLVER_RHMC_NAIVE) return f(IntTag<RHMC_SOLVER_RHMC_NAIVE>{});
  return f(IntTag<RHMC_SOLVER_RHMC_LEAPFROG>{});
}

// Image sides: the pixel-major and dense kernels are built for 32/48 px, the
// one-star kernels for 32/48/64, the implicit one-star step for 96/128 too.
// The plan has checked that the side is one of them.
template <class F>
auto with_side2(int side, F&& f) {
  return side == 32 ? f(IntTag<32>{}) : f(IntTag<48>{});
}
template <class F>
auto with_side3(int side, F&& f) {
  switch (side) {
    case 32: return f(IntTag<32>{});
    case 48: return f(IntTag<48>{});
    default: return f(IntTag<64>{});
  }
}
template <class F>
auto with_side5(int side, F&& f) {
  switch (side) {
    case 96: return f(IntTag<96>{});
    case 128: return f(IntTag<128>{});
    default: return with_side3(side, f);
  }
}

// The pixel cache of the register kernels: fp32 when the plan says so.
template <class F>
auto with_dt(const Plan& pl, F&& f) {
  return pl.f32 ? f(TypeTag<float>{}) : f(TypeTag<double>{});
}

// LDS-image plans, f(IntTag<MAXK>): the plan's register accumulators (the
// step's leapfrog_kernel<MAXK>).
template <class F>
auto with_maxk(const Plan& pl, F&& f) {
  switch (pl.maxk) {
    case 1: return f(IntTag<1>{});
    case 2: return f(IntTag<2>{});
    case 4: return f(IntTag<4>{});
    case 8: return f(IntTag<8>{});
    default: return f(IntTag<16>{});
  }
}

// The slotted one-wave-per-chain kernels, f(TypeTag<G>, IntTag<SLOTS>).
// An LDS-image plan's energy and gradient: the policy LdsG<MAXK> in one slot.
template <class F>
auto with_lds_policy(const Plan& pl, F&& f) {
  return with_maxk(pl, [&](auto mk) {
    return f(TypeTag<LdsG<decltype(mk)::value>>{}, IntTag<1>{});
  });
}
// A slotted plan: the dense policy DenseG<32 / 48> in 1, 2 or 4 slots
// (dense_path: K <= 256), the global-table policy WinGG in 2, 4, 8 or 16 (the
// only policy instantiated past 256 stars), else one slot of LDS tables: G1,
// WinG or the energy's WinEG.
template <class G, class F>
auto with_dense_slots(const Plan& pl, F&& f) {
  switch (pl.slots) {
    case 1: return f(TypeTag<G>{}, IntTag<1>{});
    case 2: return f(TypeTag<G>{}, IntTag<2>{});
    default: return f(TypeTag<G>{}, IntTag<4>{});
  }
}
static_assert(win_slots(kWinGlobalFromK - 1) == 1 && win_slots(kWinGlobalFromK) == 2,
              "below WinGG one slot (64 stars) of LDS tables");
template <class G1, class F>
auto with_policy_from(const Plan& pl, F&& f) {
  if (pl.path == 32) return with_dense_slots<DenseG<32>>(pl, f);
  if (pl.path == 48) return with_dense_slots<DenseG<48>>(pl, f);
  if (pl.policy == Policy::WinGG) {
    switch (pl.slots) {
      case 2: return f(TypeTag<WinGG>{}, IntTag<2>{});
      case 4: return f(TypeTag<WinGG>{}, IntTag<4>{});
      case 8: return f(TypeTag<WinGG>{}, IntTag<8>{});
      default: return f(TypeTag<WinGG>{}, IntTag<16>{});
    }
  }
  return f(TypeTag<G1>{}, IntTag<1>{});
}
// Step, integrators, trajectories, gradient: full tables (WinG).
template <class F>
auto with_policy(const Plan& pl, F&& f) {
  return with_policy_from<WinG>(pl, f);
}
// The energy: column tables only (WinEG).  Its dense path goes through
// with_policy, whose one-slot WinG branch a dense plan never takes: that
// instantiates energy_win_kernel<WinG, 1>, which is in the library and never
// launched.
template <class F>
auto with_energy_policy(const Plan& pl, F&& f) {
  return pl.path ? with_policy(pl, f) : with_policy_from<WinEG>(pl, f);
}
// Gradient and energy, whose plan may be an LDS-image one (the slotted step,
// the integrators and the trajectories never get one and call with_policy).
template <class F>
auto with_perwave_policy(const Plan& pl, F&& f) {
  return pl.family == Family::LdsImage ? with_lds_policy(pl, f) : with_policy(pl, f);
}
template <class F>
auto with_perwave_energy_policy(const Plan& pl, F&& f) {
  return pl.family == Family::LdsImage ? with_lds_policy(pl, f) : with_energy_policy(pl, f);
}

// The implicit one-star register-window step, f(IntTag<IMG>, IntTag<WIN>,
// TypeTag<DT>): the plan's window (28 px when the PSF allows it) and pixel cache.
template <class F>
auto with_regwin1(const Plan& pl, int side, F&& f) {
  return with_side5(side, [&](auto img) {
    return with_dt(pl, [&](auto dt) {
      return pl.window == 28 ? f(img, IntTag<28>{}, dt) : f(img, IntTag<32>{}, dt);
    });
  });
}

// The other one-star register-window kernels (explicit integrators,
// HMC_random, energy, fused MH, find_peaks), f(IntTag<IMG>, TypeTag<DT>):
// always the 28-px window, on a 32/48/64-px image.
template <class F>
auto with_k1_w28(const Plan& pl, int side, F&& f) {
  return with_side3(side, [&](auto img) {
    return with_dt(pl, [&](auto dt) { return f(img, dt); });
  });
}

// The one-star lane-group step, f(IntTag<IMG>, TypeTag<DT>, IntTag<LPC>).
template <class F>
auto with_lane(const Plan& pl, int side, F&& f) {
  return with_side3(side, [&](auto img) {
    return with_dt(pl, [&](auto dt) {
      return pl.lpc == 4 ? f(img, dt, IntTag<4>{}) : f(img, dt, IntTag<1>{});
    });
  });
}

// The multi-star register-window kernel, f(TypeTag<DT>, IntTag<SLOTS>,
// BoolTag<TAB>, IntTag<WS>): LDS factor tables in one slot, else one or two
// slots.  The window split WS (waves per chain pair) is built for the implicit
// step (IMPLICIT) without tables only; everything else runs WS = 1.
template <bool IMPLICIT, class F>
auto with_multiwin(const Plan& pl, F&& f) {
  auto no_tables = [&](auto slots) {
    return with_dt(pl, [&](auto dt) {
      if constexpr (IMPLICIT) {
        if (pl.split == 2) return f(dt, slots, BoolTag<false>{}, IntTag<2>{});
        if (pl.split == 4) return f(dt, slots, BoolTag<false>{}, IntTag<4>{});
      }
      return f(dt, slots, BoolTag<false>{}, IntTag<1>{});
    });
  };
  if (pl.tables)
    return with_dt(pl, [&](auto dt) { return f(dt, IntTag<1>{}, BoolTag<true>{}, IntTag<1>{}); });
  return pl.slots == 1 ? no_tables(IntTag<1>{}) : no_tables(IntTag<2>{});
}

// The MH loop's begin / end and the chain turn, f(BoolTag<WAVE>): one thread
// per chain, or one wave per chain (mh_wave(K), rhmc_select.hpp).
template <class F>
auto with_mh_wave(bool wave, F&& f) {
  return wave ? f(BoolTag<true>{}) : f(BoolTag<false>{});
}

}  // namespace rhmc
