// rj_registry_check.cpp — the owner of the reversible-jump driver's per-pipe
// buffers (hmc-stellar-toy-model_amd/host/rj_registry.hpp) with a stand-in
// payload, run under the thread and the address sanitizer
// (`make -C hmc-stellar-toy-model_amd/host registry_check`,
// tests/test_rj_registry_host.py): four threads lease pipes 0..k-1 of device 0
// over and over while a fifth releases device 0 and every device.  A lock-order
// mistake hangs (the test's timeout), a lifetime mistake is a sanitizer report,
// and the counters below catch a payload used while or after it is destroyed.
#include <atomic>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "rj_registry.hpp"

namespace {

std::atomic<long> g_made{0}, g_freed{0};      // objects constructed / destructed
std::atomic<long> g_lives{0}, g_destroyed{0}; // set-ups (dev -1 -> 0) / destroy()s of a live one
std::atomic<long> g_bad{0};                   // a lease saw a payload being destroyed

// Work's shape: a mutex, a device (-1: destroyed, to be set up again by the
// next run that holds it), something a run touches, destroy().
struct Payload {
  std::mutex mu;
  int dev = -1;
  long counter = 0;
  bool destroying = false;  // set only inside destroy(), under mu
  Payload() { g_made.fetch_add(1); }
  Payload(const Payload&) = delete;
  ~Payload() {
    destroy();
    g_freed.fetch_add(1);
  }
  void ensure() {  // mu held
    if (dev >= 0) return;
    dev = 0;
    g_lives.fetch_add(1);
  }
  void destroy() {  // mu held (or the last reference)
    destroying = true;
    if (dev >= 0) {
      dev = -1;
      counter = 0;
      g_destroyed.fetch_add(1);
    }
    destroying = false;
  }
};

}  // namespace

int main() {
  rj::Registry<Payload> reg;
  constexpr int kThreads = 4, kRounds = 2000;
  std::atomic<int> running{kThreads};
  std::vector<std::thread> ts;
  for (int t = 0; t < kThreads; ++t)
    ts.emplace_back([&, t] {
      for (int r = 0; r < kRounds; ++r) {
        const int k = 1 + (r + t) % 3;
        auto lease = reg.acquire(0, k);
        for (int i = 0; i < k; ++i) {
          Payload& p = lease[i];
          p.ensure();
          if (p.destroying || p.dev != 0) g_bad.fetch_add(1);
          p.counter += 1;
          if (p.destroying || p.dev != 0 || p.counter < 1) g_bad.fetch_add(1);
        }
      }
      running.fetch_sub(1);
    });
  std::thread releaser([&] {
    while (running.load() > 0) {
      reg.release(0);
      reg.release(-1);
      std::this_thread::yield();
    }
  });
  for (auto& t : ts) t.join();
  releaser.join();
  reg.release(-1);
  int rc = 0;
  auto expect = [&](bool ok, const char* what) {
    if (!ok) {
      std::fprintf(stderr, "rj registry: %s (made %ld freed %ld lives %ld destroyed %ld bad %ld)\n",
                   what, g_made.load(), g_freed.load(), g_lives.load(), g_destroyed.load(),
                   g_bad.load());
      rc = 1;
    }
  };
  expect(reg.size() == 0, "the map is not empty after release(-1)");
  expect(g_made.load() > 0 && g_made.load() == g_freed.load(),
         "a payload outlived its last reference, or was freed twice");
  expect(g_lives.load() == g_destroyed.load(), "a set-up payload was not destroyed exactly once");
  expect(g_bad.load() == 0, "a lease held a payload that was being destroyed");
  if (rc == 0) std::printf("rj registry ok\n");
  return rc;
}
