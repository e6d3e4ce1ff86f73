// CPU check of ksql_amd/csrc/khip_correlation.hpp (test infrastructure): reads lines
// "<bigint 0|1> <n> <sx0> <sx1> <sy0> <sy1> <sxx0..3> <syy0..3> <sxy0..3>" (18 numbers, the words
// unsigned decimal; an INT state's unused words are 0) and prints the bits of correlation_result as
// an unsigned decimal.
#include <cstdio>
#include <cstring>
#include "../ksql_amd/csrc/khip_correlation.hpp"
int main() {
  for (;;) {
    int bigint;
    unsigned long long v[17];
    if (std::scanf("%d", &bigint) != 1) break;
    bool ok = true;
    for (int i = 0; i < 17 && ok; i++) ok = std::scanf("%llu", &v[i]) == 1;
    if (!ok) return 1;
    uint64_t w[17];
    for (int i = 0; i < 17; i++) w[i] = v[i];
    const double d = khip::correlation_result(bigint != 0, w[0], &w[1], &w[3], &w[5], &w[9], &w[13]);
    uint64_t b;
    memcpy(&b, &d, 8);
    std::printf("%llu\n", (unsigned long long)b);
  }
  return 0;
}
