// Second host-runtime self-test for sanitizer builds: KVBlockManager::truncate, the way a
// speculative verify step gives back the cache slots of rejected draft tokens. Built by
// tests/test_spec_cpu.py with
//   g++ -fsanitize=address,undefined -fno-omit-frame-pointer selftest_spec.cpp  (no Python headers)
// and run as a plain executable. It drives randomised allocate / speculative step (append_slot,
// extend by the drafts, truncate to the accepted length) / bare truncate / fork / free streams,
// with and without prefix-cache registration of the prompt pages, against a model that knows
// every sequence's length and page list, and checks after every operation that
//   * length and page count of every sequence are the model's, and a truncate keeps the pages
//     it does not release, in order;
//   * pages are conserved: free == total - (pages some live sequence lists);
//   * the slots a speculative step writes lie in pages no other sequence lists;
//   * a truncate past the length throws and changes nothing;
//   * registered prompt pages survive truncation and are found again by match_prefix.
// Exit code 0 = pass; a failed check prints and aborts (and ASan/UBSan abort on memory / UB).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#define BFLY_RT_NO_PYTHON
#include "../kv_manager.h"

using namespace bfly_rt;

#define CHECK(c)                                                               \
  do {                                                                         \
    if (!(c)) {                                                                \
      std::fprintf(stderr, "CHECK failed %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::abort();                                                            \
    }                                                                          \
  } while (0)

static void test_truncate_basics() {
  KVBlockManager kv(8, 4);
  kv.allocate(1, 6);                               // 2 pages
  kv.extend(1, 7);                                 // 13 tokens: 4 pages
  CHECK(kv.length(1) == 13 && kv.num_free() == 4);
  const auto before = kv.block_table(1);
  kv.truncate(1, 13);                              // no-op
  CHECK(kv.length(1) == 13 && kv.num_free() == 4);
  kv.truncate(1, 9);                               // page 4 wholly beyond: released
  CHECK(kv.length(1) == 9 && kv.num_free() == 5 && kv.block_table(1).size() == 3);
  kv.truncate(1, 8);                               // exactly two full pages
  CHECK(kv.length(1) == 8 && kv.num_free() == 6 && kv.block_table(1).size() == 2);
  CHECK(kv.block_table(1)[0] == before[0] && kv.block_table(1)[1] == before[1]);
  bool threw = false;
  try {
    kv.truncate(1, 9);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw && kv.length(1) == 8 && kv.num_free() == 6);
  threw = false;
  try {
    kv.truncate(1, -1);
  } catch (const std::invalid_argument&) {
    threw = true;
  }
  CHECK(threw);
  // shared pages: the child's truncate only drops its references
  kv.extend(1, 4);                                 // 12 tokens, 3 pages
  kv.fork(1, 2);
  CHECK(kv.num_free() == 5);
  kv.truncate(2, 5);                               // child keeps 2 pages; page 3 still the parent's
  CHECK(kv.num_free() == 5 && kv.block_table(1).size() == 3 && kv.length(1) == 12);
  kv.truncate(1, 5);                               // now nobody holds page 3
  CHECK(kv.num_free() == 6);
  kv.free(1);
  CHECK(kv.num_free() == 6);
  kv.free(2);
  CHECK(kv.num_free() == 8 && kv.num_seqs() == 0);
}

struct Model {
  int64_t prompt = 0, len = 0;
  std::vector<int32_t> pages;
};

static void run_stream(unsigned seed, bool prefix_cache) {
  std::mt19937 rng(seed);
  const int kPages = 40, kBS = 8;
  KVBlockManager kv(kPages, kBS);
  std::map<int64_t, Model> seqs;
  int64_t next_id = 0;
  long spec_steps = 0, truncs = 0, released = 0;
  // prompts drawn from 2 shared heads (prefix-cache registrations collide on purpose)
  std::vector<std::vector<int32_t>> heads(2);
  for (auto& h : heads)
    for (int i = 0; i < 32; ++i) h.push_back((int32_t)(rng() % 1000));

  auto check_all = [&]() {
    std::set<int32_t> live;
    for (auto& kvp : seqs) {
      const Model& m = kvp.second;
      CHECK(kv.length(kvp.first) == m.len);
      const auto bt = kv.block_table(kvp.first);
      CHECK((int)bt.size() == kv.blocks_needed(m.len));
      CHECK(bt == m.pages);
      for (int32_t p : bt) {
        CHECK(p >= 0 && p < kPages);
        live.insert(p);
      }
    }
    CHECK(kv.num_free() == kPages - (int)live.size());
    CHECK(kv.num_seqs() == (int)seqs.size());
  };
  auto holders = [&](int32_t page) {
    int n = 0;
    for (auto& kvp : seqs)
      for (int32_t p : kvp.second.pages) n += p == page;
    return n;
  };
  auto pick = [&]() {
    auto it = seqs.begin();
    std::advance(it, rng() % seqs.size());
    return it->first;
  };

  for (int step = 0; step < 4000; ++step) {
    const unsigned op = rng() % 16;
    if (seqs.empty() || op == 0) {                                   // new sequence
      const int64_t prompt = (int64_t)(rng() % 30) + 1;
      if (!kv.can_allocate(prompt) || seqs.size() >= 10) continue;
      const int64_t sid = next_id++;
      std::vector<int32_t> toks;
      const auto& h = heads[rng() % 2];
      for (int64_t i = 0; i < prompt; ++i) toks.push_back(i < 32 && rng() % 16 ? h[i] : (int32_t)(rng() % 1000));
      const auto slots = kv.allocate(sid, prompt);
      CHECK((int64_t)slots.size() == prompt);
      if (prefix_cache) kv.register_blocks(sid, kv.block_hashes(toks));
      Model m;
      m.prompt = m.len = prompt;
      m.pages = kv.block_table(sid);
      seqs[sid] = m;
    } else if (op <= 8) {                                            // speculative step
      const int64_t sid = pick();
      Model& m = seqs.at(sid);
      if (!kv.can_append({sid})) continue;
      const auto [slot, src, dst] = kv.append_slot(sid);
      CHECK((src < 0) == (dst < 0));
      m.len += 1;
      m.pages = kv.block_table(sid);
      CHECK(slot / kBS == m.pages.back() && holders(m.pages.back()) == 1);
      const int64_t d = (int64_t)(rng() % 12);
      if (d > 0 && kv.extend_blocks(sid, d) <= kv.num_free()) {
        const auto slots = kv.extend(sid, d);
        CHECK((int64_t)slots.size() == d);
        m.pages = kv.block_table(sid);
        for (int64_t t = 0; t < d; ++t) {
          CHECK(slots[t] == m.pages[(m.len + t) / kBS] * kBS + (m.len + t) % kBS);
          CHECK(holders(slots[t] / kBS) == 1);                      // nobody else lists a draft page
        }
        const int64_t a = (int64_t)(rng() % (d + 1));                // accepted drafts
        const int before = kv.num_free();
        const auto kept = kv.block_table(sid);
        kv.truncate(sid, m.len + a);
        m.len += a;
        m.pages.resize(kv.blocks_needed(m.len));
        CHECK(std::equal(m.pages.begin(), m.pages.end(), kept.begin()));
        released += kv.num_free() - before;
        ++spec_steps;
      }
    } else if (op <= 10) {                                           // bare truncate, never below the prompt
      const int64_t sid = pick();
      Model& m = seqs.at(sid);
      const int64_t nl = m.prompt + (int64_t)(rng() % (m.len - m.prompt + 1));
      kv.truncate(sid, nl);
      m.len = nl;
      m.pages.resize(kv.blocks_needed(nl));
      ++truncs;
      bool threw = false;
      try {
        kv.truncate(sid, m.len + 1 + (int64_t)(rng() % 5));
      } catch (const std::invalid_argument&) {
        threw = true;
      }
      CHECK(threw);
    } else if (op <= 12) {                                           // fork
      if (seqs.size() >= 10) continue;
      const int64_t sid = pick(), child = next_id++;
      kv.fork(sid, child);
      seqs[child] = seqs.at(sid);
    } else {                                                         // free
      const int64_t sid = pick();
      kv.free(sid);
      seqs.erase(sid);
    }
    check_all();
  }
  for (auto& kvp : seqs) kv.free(kvp.first);
  seqs.clear();
  CHECK(kv.num_free() == kPages && kv.num_seqs() == 0);
  std::printf("spec stream prefix_cache=%d seed=%u: %ld verify steps, %ld bare truncates, %ld pages given back, %d cached\n",
              (int)prefix_cache, seed, spec_steps, truncs, released, kv.num_cached_blocks());
}

// registered full prompt pages stay registered and matchable through a truncate above the prompt
static void test_truncate_keeps_prefix_cache() {
  KVBlockManager kv(8, 4);
  std::vector<int32_t> t = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  const auto hs = kv.block_hashes(t);              // 2 full blocks
  kv.allocate(1, 9);
  kv.register_blocks(1, hs);
  kv.append_slot(1);
  kv.extend(1, 6);                                 // 16 tokens, 4 pages
  kv.truncate(1, 10);
  CHECK(kv.length(1) == 10 && kv.num_cached_blocks() == 2 && kv.match_prefix(hs, 2) == 2 && kv.num_free() == 5);
  kv.free(1);
  CHECK(kv.num_free() == 8 && kv.match_prefix(hs, 2) == 2);
}

int main() {
  test_truncate_basics();
  test_truncate_keeps_prefix_cache();
  for (unsigned seed = 1; seed <= 12; ++seed) {
    run_stream(seed, false);
    run_stream(seed, true);
  }
  std::printf("runtime spec selftest: PASS\n");
  return 0;
}
