// rj_pool.hpp — the fork-join thread pool of the driver's host phases and the
// process's pools by size.  A section of rhmc_rj.cpp's translation unit.
#pragma once

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <exception>
#include <functional>
#include <iterator>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include <emmintrin.h>

namespace {

// Fork-join pool shared by every pipe of a run (and kept between runs: spawning
// threads per phase cost ~3 ms per iteration at 16 threads, per run ~1 ms).
// Several callers may run jobs at once: a worker takes chunks of whichever job
// has some left, so while one pipe waits for its GPU phase its share of the
// host threads works on the other pipes' host phases (round 5's per-pipe
// pools left them idle), and a pipe thread waiting for its stream takes chunks
// too (help()).  Each chain's work is its own, so results do not depend on
// which thread runs it.
class Pool {
 public:
  explicit Pool(int workers) {
    try {
      for (int t = 0; t < workers; ++t) th_.emplace_back([this] { worker(); });
    } catch (...) {  // a thread could not start: stop and join the ones that did
      shutdown();
      throw;
    }
  }
  ~Pool() { shutdown(); }
  int size() const { return (int)th_.size() + 1; }
  // body(i) for i in [0, n), in chunks, the caller works too.  An exception
  // from body (any thread) is rethrown here once no thread is left in it.
  void run(int64_t n, const std::function<void(int64_t)>& body) {
    Job j;
    j.body = &body;
    j.n = n;
    {
      std::lock_guard<std::mutex> l(mu_);
      jobs_.push_back(&j);
      pending_.fetch_add(1);
    }
    cv_.notify_all();
    while (take(j)) {
    }
    {
      std::lock_guard<std::mutex> l(mu_);
      jobs_.erase(std::find(jobs_.begin(), jobs_.end(), &j));
      pending_.fetch_sub(1);
    }
    // every chunk is taken; wait for the ones still running elsewhere (no
    // worker picks the job up once it is off the list)
    while (j.done.load() != n || j.users.load() != 0) std::this_thread::yield();
    if (j.exc) std::rethrow_exception(j.exc);
  }
  // one chunk of any caller's job, if one is left: false if none
  bool help() {
    Job* j = nullptr;
    {
      std::lock_guard<std::mutex> l(mu_);
      j = pick();
      if (j) j->users.fetch_add(1);
    }
    if (!j) return false;
    const bool did = take(*j);
    j->users.fetch_sub(1);
    return did;
  }

 private:
  static constexpr int64_t kChunk = 16;
  struct Job {
    const std::function<void(int64_t)>* body = nullptr;
    int64_t n = 0;
    std::atomic<int64_t> next{0}, done{0};
    std::atomic<int> users{0};
    std::atomic<bool> failed{false};
    std::mutex emu;
    std::exception_ptr exc;
  };
  Job* pick() {  // mu_ held
    for (Job* j : jobs_)
      if (j->next.load() < j->n) return j;
    return nullptr;
  }
  // one chunk of j; false when none was left.  After a failure the remaining
  // chunks are counted without running (the first exception is kept)
  bool take(Job& j) {
    const int64_t b = j.next.fetch_add(kChunk);
    if (b >= j.n) return false;
    const int64_t e = std::min(j.n, b + kChunk);
    if (!j.failed.load()) {
      try {
        for (int64_t i = b; i < e; ++i) (*j.body)(i);
      } catch (...) {
        std::lock_guard<std::mutex> l(j.emu);
        if (!j.exc) j.exc = std::current_exception();
        j.failed.store(true);
      }
    }
    j.done.fetch_add(e - b);
    return true;
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> l(mu_);
      stop_ = true;
      stop_flag_.store(true);
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
    th_.clear();
  }
  void worker() {
    for (;;) {
      Job* j = nullptr;
      // spin a little before sleeping: the pipes' phases follow each other
      // within tens of microseconds, and a futex wake-up costs about that
      const auto t0 = std::chrono::steady_clock::now();
      for (int k = 0; pending_.load(std::memory_order_relaxed) == 0 && !stop_flag_.load(); ++k) {
        _mm_pause();
        if ((k & 255) == 255 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kSpinUs))
          break;
      }
      {
        std::unique_lock<std::mutex> l(mu_);
        cv_.wait(l, [&] { return stop_ || (j = pick()) != nullptr; });
        if (stop_) return;
        j->users.fetch_add(1);
      }
      while (take(*j)) {
      }
      j->users.fetch_sub(1);
    }
  }
  std::vector<std::thread> th_;
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<Job*> jobs_;
  bool stop_ = false;
  std::atomic<bool> stop_flag_{false};
  std::atomic<int> pending_{0};  // jobs on the list (the spin's hint)
  static constexpr int kSpinUs = 50;
};

// The process's pools by worker count: a run takes the one of its size (runs
// on other threads may share it) and it stays for the next run, until
// rhmc_rj_release drops the ones no run holds.
struct Pools {
  std::mutex mu;
  std::map<int, std::shared_ptr<Pool>> by_size;
};
Pools& pools() {
  static Pools p;
  return p;
}

std::shared_ptr<Pool> shared_pool(int workers) {
  Pools& ps = pools();
  std::lock_guard<std::mutex> l(ps.mu);
  auto& p = ps.by_size[workers];
  if (!p) p = std::make_shared<Pool>(workers);
  return p;
}

// a pool only the map refers to has no run on it (a run holds its own
// reference from start to end, taken under the same mutex); its workers join
void drop_idle_pools() {
  Pools& ps = pools();
  std::lock_guard<std::mutex> l(ps.mu);
  for (auto it = ps.by_size.begin(); it != ps.by_size.end();)
    it = it->second.use_count() == 1 ? ps.by_size.erase(it) : std::next(it);
}

// f(idx[i]) for every i, on the pool when there is one and enough to share
template <class F>
void parallel(Pool* pool, const std::vector<int64_t>& idx, F f) {
  const int64_t n = (int64_t)idx.size();
  if (!pool || pool->size() <= 1 || n < 32) {
    for (int64_t i = 0; i < n; ++i) f(idx[i]);
    return;
  }
  const std::function<void(int64_t)> body = [&](int64_t i) { f(idx[i]); };
  pool->run(n, body);
}

}  // namespace
