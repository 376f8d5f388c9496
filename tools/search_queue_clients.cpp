// search_queue_clients.cpp -- leg 2 of tools/search_queue_bench.py: the reference's caller loop (one searchKnn per query,
// include/strategy/hnsw_slim_strategy.h:112-114; the HTTP demo server's one query per request) from `threads` client threads,
// through the facade (hnsw-slim_amd/hnswlib/hnswlib_amd.h).
//   queue: every thread calls SearchQueue<float>::searchKnn(q, k) on one shared queue (submit + wait: queries of threads that
//          arrive together share a launch)
//   plain: every thread calls the index's own searchKnn(q, k), one at a time (the entry serves one caller: a mutex around it)
// usage: search_queue_clients <hnsw|slim> <index.bin> <dim> <queries.f32> <nq> <k> <ef> <threads> <calls per thread> <queue|plain>
// Output: one JSON line -- q/s over the whole run (wall clock from the first call to the last return) and the p50 / p99 latency
// of a call.  The first 10 % of every thread's calls are warm-up and not counted.
// Build: g++ -std=c++17 -O2 -pthread tools/search_queue_clients.cpp -o <out> -Lhnsw-slim_amd -lhnsw_slim_amd -Wl,-rpath,'$ORIGIN/../hnsw-slim_amd'
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

using Clock = std::chrono::steady_clock;

template <class Index>
static int run(Index &ix, const std::vector<float> &Q, size_t dim, size_t nq, size_t k, size_t ef, size_t threads, size_t calls, bool use_queue) {
  ix.setEf(ef);
  hnswlib::SearchQueue<float> queue(ix, k, 4096, 2);
  std::mutex one_at_a_time;
  const size_t warm = calls / 10;
  std::vector<std::vector<double>> lat(threads);
  std::atomic<size_t> ready{0}, found{0};
  std::atomic<bool> go{false};
  std::vector<Clock::time_point> t_begin(threads), t_end(threads);
  std::vector<std::thread> ts;
  for (size_t t = 0; t < threads; t++)
    ts.emplace_back([&, t] {
      lat[t].reserve(calls);
      ready++;
      while (!go.load()) std::this_thread::yield();
      size_t hits = 0;
      for (size_t i = 0; i < calls; i++) {
        if (i == warm) t_begin[t] = Clock::now();
        const float *q = Q.data() + ((t * 7919 + i) % nq) * dim;
        const Clock::time_point a = Clock::now();
        if (use_queue) {
          hits += queue.searchKnn(q, k).size();
        } else {
          std::lock_guard<std::mutex> g(one_at_a_time);
          hits += ix.searchKnn(q, k).size();
        }
        if (i >= warm) lat[t].push_back(std::chrono::duration<double, std::micro>(Clock::now() - a).count());
      }
      t_end[t] = Clock::now();
      found += hits;
    });
  while (ready.load() < threads) std::this_thread::yield();
  go = true;
  for (auto &t : ts) t.join();
  std::vector<double> all;
  for (auto &l : lat) all.insert(all.end(), l.begin(), l.end());
  std::sort(all.begin(), all.end());
  const double secs = std::chrono::duration<double>(*std::max_element(t_end.begin(), t_end.end()) - *std::min_element(t_begin.begin(), t_begin.end())).count();
  const struct hs_queue_info info = queue.info();
  printf("{\"mode\": \"%s\", \"threads\": %zu, \"queries\": %zu, \"seconds\": %.4f, \"qps\": %.1f, \"p50_us\": %.1f, \"p99_us\": %.1f, "
         "\"launches\": %llu, \"largest_launch\": %llu, \"results\": %zu}\n",
         use_queue ? "queue" : "plain", threads, all.size(), secs, all.size() / secs, all[all.size() / 2], all[all.size() * 99 / 100],
         (unsigned long long)info.launches, (unsigned long long)info.largest_launch, found.load());
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 11) return 2;
  const std::string kind = argv[1], mode = argv[10];
  const size_t dim = atoi(argv[3]), nq = atoi(argv[5]), k = atoi(argv[6]), ef = atoi(argv[7]), threads = atoi(argv[8]), calls = atoi(argv[9]);
  if (threads < 1 || calls < 10 || nq < 1) return 2;
  std::vector<float> Q(nq * dim);
  std::ifstream(argv[4], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space space(dim);
  try {
    if (kind == "slim") {
      hnswlib::HierarchicalNSWSlim<float> ix(&space, argv[2]);
      return run(ix, Q, dim, nq, k, ef, threads, calls, mode == "queue");
    }
    hnswlib::HierarchicalNSW<float> ix(&space, argv[2]);
    return run(ix, Q, dim, nq, k, ef, threads, calls, mode == "queue");
  } catch (const std::exception &e) {
    fprintf(stderr, "search_queue_clients: %s\n", e.what());
    return 1;
  }
}
