// rj_registry.hpp — the owner of what rhmc_rj_run keeps between runs: one
// payload per (device, pipe), shared between the map and the runs that lease
// it.  Plain C++ (no HIP): tests/native/rj_registry_check.cpp runs it under the
// thread and address sanitizers with a stand-in payload.
//
// Payload needs `std::mutex mu` and `void destroy()` (called with mu held; it
// must leave the payload usable again, as after construction).
//
// Lock order: the registry mutex guards the map alone and is never held
// while a payload mutex is taken; payload mutexes are taken in ascending pipe
// index.  A run that copied a payload's pointer before a release and locks it
// after finds it destroyed but alive, sets it up again and frees it with its
// lease (the map no longer holds it).
#pragma once

#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

namespace rj {

template <class Payload>
class Registry {
 public:
  // The payloads of pipes 0 .. n-1, locked; unlocked in reverse order.
  class Leases {
   public:
    Leases() = default;
    Leases(Leases&&) = default;
    Leases& operator=(Leases&&) = delete;
    ~Leases() {
      while (!held_.empty()) held_.pop_back();
    }
    Payload& operator[](int pipe) { return *held_[(size_t)pipe].payload; }
    int size() const { return (int)held_.size(); }

   private:
    friend class Registry;
    struct Lease {  // members are destroyed in reverse: unlock, then drop
      std::shared_ptr<Payload> payload;
      std::unique_lock<std::mutex> lock;
    };
    std::vector<Lease> held_;
  };

  Leases acquire(int device, int pipes) {
    Leases out;
    out.held_.reserve((size_t)pipes);
    {
      std::lock_guard<std::mutex> l(mu_);
      for (int i = 0; i < pipes; ++i) {
        auto& p = map_[{device, i}];
        if (!p) p = std::make_shared<Payload>();
        out.held_.push_back({p, {}});
      }
    }
    for (auto& h : out.held_) h.lock = std::unique_lock<std::mutex>(h.payload->mu);
    return out;
  }

  // destroy() every payload of `device` (every device when device < 0),
  // waiting for a run that holds one
  void release(int device) {
    std::vector<std::shared_ptr<Payload>> gone;
    {
      std::lock_guard<std::mutex> l(mu_);
      for (auto it = map_.begin(); it != map_.end();) {
        if (device >= 0 && it->first.first != device) {
          ++it;
          continue;
        }
        gone.push_back(std::move(it->second));
        it = map_.erase(it);
      }
    }
    for (auto& p : gone) {
      {
        std::lock_guard<std::mutex> l(p->mu);
        p->destroy();
      }
      p.reset();  // freed here, or with the lease of a run that still refers to it
    }
  }

  size_t size() {
    std::lock_guard<std::mutex> l(mu_);
    return map_.size();
  }

 private:
  std::mutex mu_;
  std::map<std::pair<int, int>, std::shared_ptr<Payload>> map_;
};

}  // namespace rj
