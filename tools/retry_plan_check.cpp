// Host driver for ksql_amd/csrc/khip_retry.hpp (tests/test_retry_plan.py).  Reads commands from
// stdin, one per line, and prints one JSON line per result:
//   item P SBITS SUB             encode, then decode: {"w", "p", "sbits", "sub"}
//   plan N K  l[N]  f[K][N]      retry_begin on the learned bits l, then retry_next for each of the
//                                K fail vectors (stopping at the first that reports an error), then
//                                retry_learn: one line per step, then {"learned": [...]}
#include <cstdio>
#include <iostream>
#include <vector>

#include "../ksql_amd/csrc/khip_retry.hpp"

using namespace khip;

template <class V>
static void print_list(const char* name, const V& v, const char* end) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); i++) printf("%s%lld", i ? ", " : "", (long long)v[i]);
  printf("]%s", end);
}

static void print_plan(const RetryPlan& r, bool ok) {
  printf("{\"ok\": %s, \"grow\": %s, ", ok ? "true" : "false", r.grow ? "true" : "false");
  print_list("sbits", r.sbits, ", ");
  print_list("work", r.work, ", ");
  std::vector<uint32_t> dec;
  for (const uint32_t w : r.work) {
    dec.push_back(work_part(w));
    dec.push_back((uint32_t)work_sbits(w));
    dec.push_back(work_sub(w));
  }
  print_list("decoded", dec, ", ");
  print_list("plist", r.plist, ", ");
  print_list("image", r.image, "}\n");
}

int main() {
  std::string cmd;
  while (std::cin >> cmd) {
    if (cmd == "item") {
      long long p, sbits, sub;
      std::cin >> p >> sbits >> sub;
      const uint32_t w = work_item((uint32_t)p, (int)sbits, (uint32_t)sub);
      printf("{\"w\": %u, \"p\": %u, \"sbits\": %d, \"sub\": %u}\n", w, work_part(w), work_sbits(w), work_sub(w));
    } else if (cmd == "plan") {
      int n, k;
      std::cin >> n >> k;
      std::vector<uint8_t> learned(n), fail(n);
      for (int i = 0; i < n; i++) {
        int v;
        std::cin >> v;
        learned[i] = (uint8_t)v;
      }
      RetryPlan r;
      retry_begin(r, learned);
      print_plan(r, true);
      bool ok = true;
      for (int j = 0; j < k; j++) {
        for (int i = 0; i < n; i++) {
          int v;
          std::cin >> v;
          fail[i] = (uint8_t)v;
        }
        if (!ok) continue;
        ok = retry_next(r, fail.data(), n);
        print_plan(r, ok);
      }
      retry_learn(learned, r);
      printf("{");
      print_list("learned", learned, "}\n");
    } else {
      fprintf(stderr, "unknown command %s\n", cmd.c_str());
      return 2;
    }
  }
  return 0;
}
