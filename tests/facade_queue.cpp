// tests/facade_queue.cpp -- a server's worker threads through the facade's SearchQueue (hnsw-slim_amd/hnswlib/hnswlib_amd.h, hs_queue_*).
// Part A: the first half of the queries handed in as submissions of 1, 2, 3, 1, 2, 3, ... rows, then ONE wait on the first ticket
//         (which flushes: one launch), then the other waits.
// Part B: `threads` threads, each calling the queue's thread-safe searchKnn(q, k) for its share of the second half, one query a call.
// usage: facade_queue <hnsw|slim> <index.bin> <dim> <queries.f32> <nq> <k> <ef> <threads> <out.bin>
//   out.bin: u64 launches after part A, u64 largest launch after part A,
//            part A: nA x k u64 labels, nA x k f32 dists, nA u32 counts (as searchKnnBatch writes them),
//            part B, per query: u32 count, count x {f32 dist, u64 label} in the priority_queue's pop order (farthest first)
#include <atomic>
#include <cstdio>
#include <fstream>
#include <string>
#include <thread>
#include <vector>

#include "../hnsw-slim_amd/hnswlib/hnswlib_amd.h"

template <class Index>
static int run(Index &ix, const std::vector<float> &Q, size_t dim, size_t nq, size_t k, size_t ef, size_t threads, std::ofstream &out) {
  ix.setEf(ef);
  hnswlib::SearchQueue<float> queue(ix, k, 4096, 2);
  const size_t nA = nq / 2, nB = nq - nA;
  std::vector<uint64_t> labels(nA * k);
  std::vector<float> dists(nA * k);
  std::vector<uint32_t> counts(nA);
  std::vector<hnswlib::SearchQueue<float>::ticket_t> tickets;
  for (size_t at = 0, i = 0; at < nA; i++) {
    const size_t m = std::min(nA - at, i % 3 + 1);
    tickets.push_back(queue.submit(Q.data() + at * dim, m, labels.data() + at * k, dists.data() + at * k, counts.data() + at));
    at += m;
  }
  queue.wait(tickets[0]);
  const struct hs_queue_info info = queue.info();
  for (size_t i = 1; i < tickets.size(); i++) queue.wait(tickets[i]);
  out.write((const char *)&info.launches, 8);
  out.write((const char *)&info.largest_launch, 8);
  out.write((const char *)labels.data(), labels.size() * 8);
  out.write((const char *)dists.data(), dists.size() * 4);
  out.write((const char *)counts.data(), counts.size() * 4);

  std::vector<std::vector<std::pair<float, uint64_t>>> got(nB);
  std::vector<std::thread> ts;
  std::atomic<int> failed{0};
  for (size_t t = 0; t < threads; t++)
    ts.emplace_back([&, t] {
      try {
        for (size_t i = t; i < nB; i += threads) {
          auto r = queue.searchKnn(Q.data() + (nA + i) * dim, k);
          while (!r.empty()) { got[i].emplace_back(r.top().first, (uint64_t)r.top().second); r.pop(); }
        }
      } catch (const std::exception &e) {
        fprintf(stderr, "facade_queue: %s\n", e.what());
        failed = 1;
      }
    });
  for (auto &t : ts) t.join();
  for (auto &g : got) {
    const uint32_t c = (uint32_t)g.size();
    out.write((const char *)&c, 4);
    for (auto &p : g) { out.write((const char *)&p.first, 4); out.write((const char *)&p.second, 8); }
  }
  return failed;
}

int main(int argc, char **argv) {
  if (argc < 10) return 2;
  const std::string mode = argv[1];
  const size_t dim = atoi(argv[3]), nq = atoi(argv[5]), k = atoi(argv[6]), ef = atoi(argv[7]), threads = atoi(argv[8]);
  std::vector<float> Q(nq * dim);
  std::ifstream(argv[4], std::ios::binary).read((char *)Q.data(), Q.size() * 4);
  hnswlib::L2Space space(dim);
  std::ofstream out(argv[9], std::ios::binary);
  try {
    if (mode == "slim") {
      hnswlib::HierarchicalNSWSlim<float> ix(&space, argv[2]);
      return run(ix, Q, dim, nq, k, ef, threads, out);
    }
    hnswlib::HierarchicalNSW<float> ix(&space, argv[2]);
    return run(ix, Q, dim, nq, k, ef, threads, out);
  } catch (const std::exception &e) {
    fprintf(stderr, "facade_queue: %s\n", e.what());
    return 1;
  }
}
