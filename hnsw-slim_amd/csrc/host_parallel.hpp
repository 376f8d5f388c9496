// host_parallel.hpp -- the one worker pool of the host code (builders, converters, quantiser).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstddef>
#include <exception>
#include <mutex>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace hs {

// fn(i, tid) once for every i in [0, n), on `threads` workers (threads < 1: one) that claim [i, i + grain) with fetch_add(grain);
// tid < threads names the worker, so per-thread state is a vector the caller owns.  The caller is worker 0.  The first
// std::exception thrown by fn stops further claims and is rethrown here, after the join, as a std::runtime_error with its message.
template <class Fn>
void parallel_for(size_t n, int threads, size_t grain, Fn fn) {
  if (threads < 1) threads = 1;
  if (grain < 1) grain = 1;
  std::atomic<size_t> next(0);
  std::atomic<bool> failed(false);
  std::string err;
  std::mutex err_mu;
  auto work = [&](int tid) {
    for (size_t i0; !failed && (i0 = next.fetch_add(grain)) < n;) {
      try {
        for (size_t i = i0; i < std::min(n, i0 + grain); i++) fn(i, tid);
      } catch (std::exception &e) {
        std::lock_guard<std::mutex> g(err_mu);
        if (!failed) err = e.what();
        failed = true;
      }
    }
  };
  std::vector<std::thread> pool;
  for (int t = 1; t < threads; t++) pool.emplace_back(work, t);
  work(0);
  for (auto &th : pool) th.join();
  if (failed) throw std::runtime_error(err);
}

}  // namespace hs
