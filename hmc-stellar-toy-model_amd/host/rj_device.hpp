// rj_device.hpp — rhmc_rj_run's loop: the chains live in HBM for the whole
// run (librhmc.so's ragged-set entry points, rhmc.h ABI 4).  Per pipe: padded
// [n][W] rows (W = 3 N_max, zeros past a chain's 3 K) of
//   Q0   the chains' states (the iteration's starting point; the q_chain rows)
//   Q, P the working trajectory state
// and per iteration only these cross PCIe:
//   H2D  the host-drawn normals z (3 K per chain: the NumPy-stream draws stay
//        on the host, bit for bit), the star counts, index lists, and the
//        jumping chains' proposed rows
//   D2H  T0, V / T at the end (one double each per chain), the jumping chains'
//        rows before their proposal, and — when the caller records them — the
//        q_chain / p_chain rows (on a second stream, overlapping the trajectory)
// The momentum p = z sqrt(H(q)) and both kinetic energies run on the device
// (rhmc_kinetic_rows_device, the reference's operation order); every phase is
// one ragged launch for the star counts the slotted kernels serve (dense /
// windowed, rhmc_ragged_ok) plus one packed launch per remaining star count
// (the one-star, pixel-major and multi-star register-window kernels), the
// packed ones spread over the pipe's two streams.
// A section of rhmc_rj.cpp's translation unit.
#pragma once

#include <mutex>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "rj_iteration.hpp"
#include "rj_pool.hpp"

namespace {

constexpr int kStreamsPerPipe = 2;  // main (in order) + aux (records, packed groups)

#define RJ_HIP(expr)                                                                   \
  do {                                                                                 \
    const hipError_t e_ = (expr);                                                      \
    if (e_ != hipSuccess) return fail(RHMC_ERR_HIP, std::string(#expr) + ": " +        \
                                                        hipGetErrorString(e_));        \
  } while (0)

#define RJ_TRY(expr)                        \
  do {                                      \
    if (int rc_ = (expr)) return rc_;       \
  } while (0)

// Index lists of an iteration, one region each (the launches read them from
// mapped host memory when they execute, so no region is rewritten before a
// wait on its readers).
enum { kIdxV0, kIdxSteps1, kIdxJump, kIdxSteps2, kIdxV1, kIdxCommit, kIdxRegions };

// One pipe's buffers: device rows and pinned staging, grown as needed and kept
// until rhmc_rj_release (a run of 4,096 chains at N_max 120 holds ~90 MB of HBM
// and ~60 MB of pinned memory per pipe).  `mu` is held for a whole run, so two
// concurrent rhmc_rj_run calls on one device serialise pipe by pipe.  Owned
// by the registry (rj_registry.hpp) and the runs that lease it.
struct Work {
  std::mutex mu;
  int dev = -1;
  // the pipe's per-chain host state, kept between runs with its vectors'
  // capacity (freeing and reallocating it per run cost ~2 ms at 1,024 chains)
  std::vector<Chain> chains;
  hipStream_t s[kStreamsPerPipe] = {};
  hipEvent_t ev[4] = {};

  int64_t cap_n = 0, cap_W = 0;
  // Device rows: Q, P (the trajectories' state), Q0 (each iteration's start),
  // pack (the fixed-K launches' gathered batches).
  double *Q = nullptr, *P = nullptr, *Q0 = nullptr, *pack = nullptr;
  // Everything that crosses PCIe lives in coherent pinned host memory mapped
  // into the device's address space, and the kernels read or write it there
  // (their *_d addresses): the iteration's draws `up` = [zoff (N int64) | K
  // (N int32, in N int64 slots) | Z (M doubles)], the index lists, T0 | V(q),
  // V(q') | T', the record rows' live columns and the jumping rows.  No copy
  // engine and no copy call: SDMA copies stalled a pipe 7-8 ms at its first
  // large copy of a direction (profiles/r06_rj/, RHMC_RJ_TIMING build), and
  // each one added a queue hand-off to the iteration's critical path.
  void *up_h = nullptr, *vt_h = nullptr;
  double *Zh = nullptr, *Jh = nullptr, *recq = nullptr, *recp = nullptr;
  double *T0h = nullptr, *T1h = nullptr, *Vh = nullptr;
  int32_t* Kh = nullptr;
  int64_t *zoffh = nullptr, *idxh = nullptr;
  // their device addresses
  double *Zd = nullptr, *Jd = nullptr, *recqd = nullptr, *recpd = nullptr;
  double *T0d = nullptr, *T1d = nullptr, *Vd = nullptr;
  int32_t* Kd = nullptr;
  int64_t *zoffd = nullptr, *idxd = nullptr;

  Work() = default;
  Work(const Work&) = delete;
  // a payload the registry has let go of is freed with its last lease
  ~Work() { destroy(); }

  void release() {
    for (double* d : {Q, P, Q0, pack}) (void)hipFree(d);
    for (double* h : {Jh, recq, recp, T0h}) (void)hipHostFree(h);
    for (void* h : {up_h, vt_h}) (void)hipHostFree(h);
    (void)hipHostFree(idxh);
    Q = P = Q0 = pack = nullptr;
    up_h = vt_h = nullptr;
    Zh = Jh = recq = recp = T0h = T1h = Vh = nullptr;
    Zd = Jd = recqd = recpd = T0d = T1d = Vd = nullptr;
    Kh = Kd = nullptr;
    zoffh = idxh = zoffd = idxd = nullptr;
    cap_n = cap_W = 0;
  }

  // everything, streams and events included (rhmc_rj_release; `mu` held).
  // Leaves dev == -1: ensure() sets the pipe up again
  void destroy() {
    std::vector<Chain>().swap(chains);
    if (dev < 0) return;
    (void)hipSetDevice(dev);
    for (auto& st : s)
      if (st) (void)hipStreamSynchronize(st);
    release();
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& st : s)
      if (st) (void)hipStreamDestroy(st);
    for (auto& e : ev) e = nullptr;
    for (auto& st : s) st = nullptr;
    dev = -1;
  }

  // streams and events on `device` once; buffers for n chains of W doubles
  int ensure(int device, int64_t n, int64_t W) {
    if (dev < 0) {
      dev = device;
      for (auto& st : s) RJ_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      for (auto& e : ev) RJ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (n <= cap_n && W <= cap_W) return 0;
    for (auto& st : s) RJ_HIP(hipStreamSynchronize(st));
    release();
    const int64_t N = std::max<int64_t>(n, 1), M = N * W;
    auto dmal = [](auto** p, size_t count) {
      return hipMalloc((void**)p, count * sizeof(**p)) == hipSuccess;
    };
    // coherent, mapped: the kernels read / write it at its device address
    auto hmap = [](auto** p, auto** d, size_t count) {
      return hipHostMalloc((void**)p, count * sizeof(**p),
                           hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
             hipHostGetDevicePointer((void**)d, *p, 0) == hipSuccess;
    };
    double *uph = nullptr, *upd = nullptr, *vth = nullptr, *vtd = nullptr;
    const bool ok = dmal(&Q, M) && dmal(&P, M) && dmal(&Q0, M) && dmal(&pack, 4 * M) &&
                    hmap(&uph, &upd, 2 * N + M) && hmap(&Jh, &Jd, 2 * M) &&
                    hmap(&recq, &recqd, M) && hmap(&recp, &recpd, M) &&
                    hmap(&T0h, &T0d, 2 * N) && hmap(&vth, &vtd, 2 * N) &&
                    hmap(&idxh, &idxd, kIdxRegions * N);
    up_h = uph;
    vt_h = vth;
    if (ok) {
      zoffh = (int64_t*)uph;
      Kh = (int32_t*)(uph + N);
      Zh = uph + 2 * N;
      zoffd = (int64_t*)upd;
      Kd = (int32_t*)(upd + N);
      Zd = upd + 2 * N;
      Vh = vth;
      T1h = vth + N;
      Vd = vtd;
      T1d = vtd + N;
    }
    if (!ok) {
      release();
      return fail(RHMC_ERR_NOMEM, "reversible-jump device buffers: allocation failed");
    }
    cap_n = N;
    cap_W = W;
    return 0;
  }
};

// The caller's current device, restored when a run returns.
struct DeviceGuard {
  int prev = -1;
  DeviceGuard() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

struct DevRun {
  rhmc_ctx* ctx;
  Work* w;
  int64_t n, W;
  std::vector<int32_t>& K;  // host star counts (what the kernels read: set_K)
  const std::vector<char>& ragged_ok;

  // the star counts as the kernels read them (mapped host memory; no kernel
  // reading them is in flight when the host rewrites them)
  void set_K() { std::copy(K.begin(), K.end(), w->Kh); }
  int64_t* idx_h(int region) { return w->idxh + region * w->cap_n; }
  int64_t* idx_d(int region) { return w->idxd + region * w->cap_n; }
  // the plan's chain order as the launches' index list.  Each region is
  // rewritten only after a wait on the launches that read it (or, for the
  // commit list, behind them in stream order)
  void set_order(const Plan& pl, int region) {
    std::copy(pl.order.begin(), pl.order.end(), idx_h(region));
  }
  // the host waits until stream i is done.  (A blocking-sync event instead of
  // the runtime's spinning wait measured 0.87-0.93x at B4: the wake-up latency
  // costs more than the CPU the spin takes from the pool threads.)
  // While the stream runs, the waiting pipe thread takes host chunks of the
  // other pipes' phases.
  Pool* pool;
  template <class Query>
  int wait_for(const char* what, Query query) {
    for (;;) {
      const hipError_t e = query();
      if (e == hipSuccess) return 0;
      if (e != hipErrorNotReady)
        return fail(RHMC_ERR_HIP,
                    std::string("reversible-jump ") + what + ": " + hipGetErrorString(e));
      if (!pool->help()) std::this_thread::yield();
    }
  }
  int wait(int i) { return wait_for("stream", [&] { return hipStreamQuery(w->s[i]); }); }
  // the host waits for event e (recorded on a stream), taking pool chunks
  int wait_event(int e) { return wait_for("event", [&] { return hipEventQuery(w->ev[e]); }); }
  // rows of src (width sw; rows si, or all n in order) -> rows of dst: d columns each
  int copy_rows(const char* what, const double* src, int64_t sw, const int64_t* si, double* dst,
                int64_t dw, const int64_t* di, int64_t m, int64_t d, hipStream_t st) {
    const int rc = rhmc_rows_copy_device(ctx, src, sw, si, dst, dw, di, m, (int32_t)d, st);
    return rc ? engine_fail(rc, what) : 0;
  }
  // aux waits for main, or main for aux
  int join(int from, int to, int e) {
    RJ_HIP(hipEventRecord(w->ev[e], w->s[from]));
    RJ_HIP(hipStreamWaitEvent(w->s[to], w->ev[e], 0));
    return 0;
  }

  // n_steps steps on chains idx (rows of Q, P)
  int trajectories(const rhmc_params* P, const std::vector<int64_t>& idx, int32_t n_steps,
                   int region) {
    if (idx.empty()) return 0;
    const Plan pl = make_plan(idx, K, ragged_ok);
    set_order(pl, region);
    bool aux_used = false;
    int packed = 0;
    for (const Call& c : pl.calls) {
      const int64_t* rows = idx_d(region) + c.off;
      if (c.ragged) {
        if (int rc = timed_launch("steps", c, [&] {
              return rhmc_leapfrog_ragged_device(ctx, P, w->Q, w->P, W, rows, w->Kd, c.n, c.Kmin,
                                                 c.Kmax, n_steps, w->s[0]);
            }))
          return engine_fail(rc, "ragged steps");
        continue;
      }
      // packed: gather, fixed-K steps, scatter — alternate groups onto aux
      const int si = (packed++ % 2);
      if (si == 1 && !aux_used) {
        RJ_TRY(join(0, 1, 0));
        aux_used = true;
      }
      hipStream_t st = w->s[si];
      const int64_t d = 3 * (int64_t)c.Kmin;
      double* pq = w->pack + (si ? 2 * n * W : 0);
      double* pp = pq + c.n * d;
      RJ_TRY(copy_rows("gather", w->Q, W, rows, pq, d, nullptr, c.n, d, st));
      RJ_TRY(copy_rows("gather", w->P, W, rows, pp, d, nullptr, c.n, d, st));
      if (int rc = rhmc_leapfrog_device(ctx, P, pq, pp, c.n, c.Kmin, n_steps, nullptr, nullptr, st))
        return engine_fail(rc, "steps");
      RJ_TRY(copy_rows("scatter", pq, d, nullptr, w->Q, W, rows, c.n, d, st));
      RJ_TRY(copy_rows("scatter", pp, d, nullptr, w->P, W, rows, c.n, d, st));
    }
    if (aux_used) RJ_TRY(join(1, 0, 1));
    return 0;
  }

  // V of chains idx (rows of Q) -> V_out[j] for chain order[j] (a device
  // address: the mapped host buffer the host reads after a wait)
  int energies(const rhmc_params* P, const std::vector<int64_t>& idx, int32_t f_pos,
               std::vector<int64_t>& order, int region, double* V_out) {
    order.clear();
    if (idx.empty()) return 0;
    const Plan pl = make_plan(idx, K, ragged_ok);
    order = pl.order;
    set_order(pl, region);
    for (const Call& c : pl.calls) {
      const int64_t* rows = idx_d(region) + c.off;
      if (c.ragged) {
        if (int rc = timed_launch("energy", c, [&] {
              return rhmc_energy_ragged_device(ctx, P, w->Q, W, rows, w->Kd, c.n, c.Kmin, c.Kmax,
                                               f_pos, V_out + c.off, w->s[0]);
            }))
          return engine_fail(rc, "ragged energy");
        continue;
      }
      const int64_t d = 3 * (int64_t)c.Kmin;
      RJ_TRY(copy_rows("gather", w->Q, W, rows, w->pack, d, nullptr, c.n, d, w->s[0]));
      if (int rc = rhmc_energy_device(ctx, P, w->pack, nullptr, V_out + c.off, nullptr, c.n, c.Kmin,
                                      f_pos, w->s[0]))
        return engine_fail(rc, "energy");
    }
    return 0;
  }
};

// The device-resident run of chains [0, n) of one pipe (q, K, seeds point at
// its first chain; record row l of chain c is l * rec_stride + rec_off + c).
int run_device(rhmc_ctx* ctx, int dev, Work* w, const rhmc_params* P0,
               const rhmc_rj_config* cfg, double* q, int32_t* K, const uint32_t* seeds, int64_t n,
               const rhmc_rj_record* rec, int64_t rec_stride, int64_t rec_off, Pool* pool,
               double* phase_out) {
  const Stopwatch sw;  // diagnostic build: setup / iterations / teardown of a pipe
  const int64_t W = 3 * (int64_t)cfg->N_max;
  RJ_TRY(w->ensure(dev, n, W));
  hipStream_t s0 = w->s[0];
  Moves mv(P0, cfg);
  std::vector<Chain>& ch = w->chains;  // the pipe's, kept with their capacity
  ch.resize((size_t)n);
  std::vector<int32_t> Kc((size_t)n);
  const std::vector<int32_t> K_in(K, K + n);  // the rows' widths on entry (ZP_STARTS)
  std::vector<int64_t> all((size_t)n);
  int32_t kin = 1;
  for (int64_t c = 0; c < n; ++c) {
    all[c] = c;
    kin = std::max(kin, K[c]);
  }
  // each chain's stream (MT19937 seeding: ~2 us a chain) and the caller's
  // rows' live columns (3 K_max, zeros past 3 K) -> Q0, on the pool; the
  // rest of Q0 is zeroed on the device
  const int64_t w0 = 3 * (int64_t)kin;
  parallel(pool, all, [&](int64_t c) {
    Chain& h = ch[c];
    start_stream(h, cfg, seeds, rec_off, c);
    h.K = K[c];
    h.pre = false;
    Kc[c] = K[c];
    double* row = w->Zh + c * w0;
    std::copy(q + c * W, q + c * W + 3 * (int64_t)K[c], row);
    std::fill(row + 3 * (int64_t)K[c], row + w0, 0.);
  });
  RJ_HIP(hipMemsetAsync(w->Q0, 0, (size_t)(n * W) * 8, s0));
  std::vector<char> ragged_ok((size_t)cfg->N_max + 1, 0);
  DevRun D{ctx, w, n, W, Kc, ragged_ok, pool};
  RJ_TRY(D.copy_rows("start rows", w->Zd, w0, nullptr, w->Q0, W, nullptr, n, w0, s0));
  RJ_HIP(hipStreamSynchronize(s0));  // Zh is the draws' staging next
  for (int k = 1; k <= cfg->N_max; ++k) {
    int32_t ok = 0;
    if (int rc = rhmc_ragged_ok(ctx, P0, k, &ok)) return rc;
    ragged_ok[k] = (char)ok;
  }
  const int64_t rows_n = (int64_t)cfg->n_iter + 1;
  std::vector<double> V0((size_t)n), V1((size_t)n);
  RecordedV V_end(n);
  const bool rec_q = rec && rec->q_chain, rec_p = rec && rec->p_chain;
  PhaseClock clock;
  std::vector<int64_t> order, order0, jump, live, scored, acc_rows;
  [[maybe_unused]] const double ms_setup = sw.ms();
  for (int64_t l = 0; l < rows_n; ++l) {
    clock.l = l;
    apply_schedules(cfg, l, mv.P);
    const Metric M = mv.metric();
    // 1. host draws: z = randn(3K) (the momentum, :1021-1022), move type, grow / shrink
    int64_t zt = 0;
    for (int64_t c = 0; c < n; ++c) {
      w->zoffh[c] = zt;
      zt += 3 * (int64_t)Kc[c];
    }
    parallel(pool, all, [&](int64_t c) {
      Chain& h = ch[c];
      double* z = w->Zh + w->zoffh[c];
      if (h.pre) {  // drawn during the previous iteration's V(q') wait
        std::copy(h.znext.begin(), h.znext.end(), z);
        h.move = h.move_next;
        h.grow = h.grow_next;
        h.pre = false;
      } else {
        draw_start(h, cfg, z);
      }
      h.K0 = h.K;
      h.dead = false;
    });
    clock.lap(0);
    // 2. device: Q = Q0, p = z sqrt(H(q)), T0; record rows; V(q) unless reused.
    // Rows are zero past 3 K in Q0; Q may hold a rejected birth's or split's
    // extra star past it (3 entries), so Q = Q0 covers 3 K_max + 3 columns and
    // every other copy only the columns a row can use (not the 3 N_max width)
    const int32_t kmax = *std::max_element(Kc.begin(), Kc.end());
    const int64_t wq = std::min<int64_t>(W, 3 * (int64_t)kmax + 3);
    const int64_t wr = 3 * (int64_t)kmax;  // the record rows' live columns
    D.set_K();  // [zoff | K | Z] are read by the kernels where the host wrote them
    RJ_HIP(hipMemcpy2DAsync(w->Q, (size_t)W * 8, w->Q0, (size_t)W * 8, (size_t)wq * 8, (size_t)n,
                            hipMemcpyDeviceToDevice, s0));
    if (int rc = rhmc_kinetic_rows_device(ctx, &mv.P, w->Q, w->P, W, w->Kd, w->Zd, w->zoffd, n,
                                          w->T0d, s0))
      return engine_fail(rc, "momentum");
    // the record rows' live columns, before the trajectory moves P
    const char* rr = "record rows";
    if (rec_q) RJ_TRY(D.copy_rows(rr, w->Q0, W, nullptr, w->recqd, W, nullptr, n, wr, s0));
    if (rec_p) RJ_TRY(D.copy_rows(rr, w->P, W, nullptr, w->recpd, W, nullptr, n, wr, s0));
    const bool reuse = V_end.valid(mv.P);
    // V(q) when not reused, [T0 | V(q)] read at the accept step
    double* V0h = w->T0h + w->cap_n;
    if (!reuse) RJ_TRY(D.energies(&mv.P, all, cfg->f_pos, order0, kIdxV0, w->T0d + w->cap_n));
    // the jumping chains (their rows go to the host after the trajectory)
    jump.clear();
    for (int64_t c = 0; c < n; ++c)
      if (ch[c].move != 0) jump.push_back(c);
    std::copy(jump.begin(), jump.end(), D.idx_h(kIdxJump));
    // 3. the trajectory of every chain (queued behind the above).  The host
    // needs T0, V(q) and the record rows only at the accept step: no wait here
    RJ_HIP(hipEventRecord(w->ev[2], s0));  // T0, V(q) and the record rows are in
                                           // (events 0 and 1: join())
    RJ_TRY(D.trajectories(&mv.P, all, cfg->n_steps, kIdxSteps1));
    clock.lap(1);
    // while the trajectories run: the iteration's record rows (row l: its
    // starting state; none of it depends on the accept step)
    RJ_TRY(D.wait_event(2));
    if (!reuse)
      for (size_t j = 0; j < order0.size(); ++j) V0[order0[j]] = V0h[j];
    else
      V0 = V_end.V;
    parallel(pool, all, [&](int64_t c) {
      Chain& h = ch[c];
      h.E0 = V0[c] + w->T0h[c];
      // the rows are zero past 3 K0 on the device: copy the 3 K0, write the zeros
      record_start(cfg, rec, l * rec_stride + rec_off + c, W, w->recq + c * W, w->recp + c * W,
                   h.K0, V0[c], w->T0h[c], h.E0, h.move, h.grow);
    });
    clock.lap(6);
    // 4. the jumping chains' rows to the host, their proposals on (q, -p), back
    const int64_t nj = (int64_t)jump.size();
    // a jumping row's columns: its 3 K stars and the one a birth / split adds
    int32_t kj = 1;
    for (int64_t c : jump) kj = std::max(kj, Kc[c]);
    const int64_t dj = std::min<int64_t>(W, 3 * (int64_t)kj + 3);
    double* Jq = w->Jd;             // [nj][dj] q rows, then [nj][dj] p rows (host, mapped)
    double* Jp = w->Jd + nj * dj;
    int64_t* jd = D.idx_d(kIdxJump);
    if (nj > 0) {
      RJ_TRY(D.copy_rows("gather", w->Q, W, jd, Jq, dj, nullptr, nj, dj, s0));
      RJ_TRY(D.copy_rows("gather", w->P, W, jd, Jp, dj, nullptr, nj, dj, s0));
    }
    RJ_TRY(D.wait(0));
    clock.lap(2);
    std::vector<int64_t> jpos(jump.size());
    for (int64_t j = 0; j < nj; ++j) jpos[j] = j;
    parallel(pool, jpos, [&](int64_t j) {
      Chain& h = ch[jump[j]];
      double* rq = w->Jh + j * dj;
      double* rp = w->Jh + nj * dj + j * dj;
      const int64_t d = 3 * (int64_t)h.K;
      h.q.assign(rq, rq + d);
      h.p.resize((size_t)d);
      for (int64_t i = 0; i < d; ++i) h.p[i] = -rp[i];
      if (!mv.propose(h, M)) {
        h.dead = true;
        h.K = h.K0;
        return;  // its rows are restored from Q0 at the accept step
      }
      std::fill(std::copy(h.q.begin(), h.q.end(), rq), rq + dj, 0.);
      std::fill(std::copy(h.p.begin(), h.p.end(), rp), rp + dj, 0.);
    });
    live.clear();
    for (int64_t c : jump)
      if (!ch[c].dead) live.push_back(c);
    for (int64_t c : live) Kc[c] = ch[c].K;
    clock.lap(3);
    if (nj > 0) {  // every jumping row back (a dead end's rows are restored later)
      RJ_TRY(D.copy_rows("scatter", Jq, dj, nullptr, w->Q, W, jd, nj, dj, s0));
      RJ_TRY(D.copy_rows("scatter", Jp, dj, nullptr, w->P, W, jd, nj, dj, s0));
      D.set_K();
    }
    // 5. the trajectory after the jump
    RJ_TRY(D.trajectories(&mv.P, live, cfg->n_steps, kIdxSteps2));
    clock.lap(4);
    // 6. V(q') and T(p', H(q')) of every chain that was not a dead end
    scored.clear();
    for (int64_t c = 0; c < n; ++c)
      if (!ch[c].dead) scored.push_back(c);
    RJ_TRY(D.energies(&mv.P, scored, cfg->f_pos, order, kIdxV1, w->Vd));
    if (int rc = rhmc_kinetic_rows_device(ctx, &mv.P, w->Q, w->P, W, w->Kd, nullptr, nullptr, n,
                                          w->T1d, s0))
      return engine_fail(rc, "kinetic");
    clock.lap(4);
    // while they run: each scored chain's accept uniform (:1072, :1120), and
    // for a chain whose star count cannot change the next iteration's draws
    const bool next = l + 1 < rows_n;
    parallel(pool, all, [&](int64_t c) {
      Chain& h = ch[c];
      if (h.dead) {
        h.K = h.K0;
      } else {
        h.u = std::log(h.rng.random_sample());
        if (h.move != 0) return;
      }
      if (!next) return;
      const int mv_now = h.move;  // this iteration's, for its accept step
      const bool gr = h.grow;
      h.znext.resize(3 * (size_t)h.K);
      draw_start(h, cfg, h.znext.data());
      h.move_next = h.move;
      h.grow_next = h.grow;
      h.move = mv_now;
      h.grow = gr;
      h.pre = true;
    });
    clock.lap(0);
    RJ_TRY(D.wait(0));  // V(q') and T'
    for (size_t j = 0; j < order.size(); ++j) V1[order[j]] = w->Vh[j];
    clock.lap(5);
    // 7. accept / reject (:1072-1083, :1120-1131); accepted rows become Q0
    std::vector<char> acc((size_t)n, 0);
    parallel(pool, all, [&](int64_t c) {
      Chain& h = ch[c];
      const bool a = !h.dead && accepts(h.move, h.E0, V1[c] + w->T1h[c], h.u, h.factor);
      if (!a) h.K = h.K0;
      acc[c] = a;
      V_end.V[c] = a ? V1[c] : V0[c];
      record_accept(rec, l * rec_stride + rec_off + c, a, h.dead);
    });
    acc_rows.clear();
    int32_t kacc = 1;  // an accepted row's columns: its old and new stars
    for (int64_t c = 0; c < n; ++c) {
      if (acc[c]) {
        acc_rows.push_back(c);
        kacc = std::max(kacc, std::max(ch[c].K0, ch[c].K));
      }
      Kc[c] = ch[c].K;
    }
    if (!acc_rows.empty()) {
      const int64_t dc = std::min<int64_t>(W, 3 * (int64_t)kacc);
      int64_t* cd = D.idx_d(kIdxCommit);
      std::copy(acc_rows.begin(), acc_rows.end(), D.idx_h(kIdxCommit));
      RJ_TRY(D.copy_rows("commit", w->Q, W, cd, w->Q0, W, cd, (int64_t)acc_rows.size(), dc, s0));
    }
    clock.lap(6);
    V_end.store(mv.P);
  }
  [[maybe_unused]] const double ms_loop = sw.ms();
  // the final states: the live columns (3 K_max) back, zeros past 3 K
  int32_t kout = 1;
  for (int64_t c = 0; c < n; ++c) kout = std::max(kout, ch[c].K);
  const int64_t w1 = 3 * (int64_t)kout;
  RJ_TRY(D.copy_rows("final rows", w->Q0, W, nullptr, w->Zd, w1, nullptr, n, w1, s0));
  RJ_HIP(hipStreamSynchronize(s0));
  const bool zp_starts = cfg->records_zero_padded & RHMC_RJ_ZP_STARTS;
  parallel(pool, all, [&](int64_t c) {
    // ZP_STARTS: the caller's row is zero past 3 K_in, so the zeros stop there
    const int64_t d = 3 * (int64_t)ch[c].K;
    finish_chain(ch[c], cfg, rec_off, c, w->Zh + c * w1,
                 zp_starts ? std::max(d, 3 * (int64_t)K_in[c]) : W, W, q, K);
  });
  clock.add_to(phase_out);
  RJ_TRACE("rj pipe n=%lld setup %.3f ms iterations %.3f ms teardown %.3f ms\n", (long long)n,
           ms_setup, ms_loop - ms_setup, sw.ms() - ms_loop);
  return 0;
}

}  // namespace
