// CPU check of ksql_amd/csrc/khip_variance.hpp (test infrastructure): reads lines
// "<sample 0|1> <bigint 0|1> <n> <sum> <hi> <sq0> <sq1> <sq2> <sq3>" (n signed, the words unsigned
// decimal) and prints the bits of variance_result as an unsigned decimal.
#include <cstdio>
#include <cstring>
#include "../ksql_amd/csrc/khip_variance.hpp"
int main() {
  int sample, bigint;
  long long n;
  unsigned long long sum, hi, sq[4];
  while (std::scanf("%d %d %lld %llu %llu %llu %llu %llu %llu", &sample, &bigint, &n, &sum, &hi, &sq[0], &sq[1], &sq[2],
                    &sq[3]) == 9) {
    const uint64_t w[4] = {sq[0], sq[1], sq[2], sq[3]};
    const double d = khip::variance_result(sample != 0, bigint != 0, (int64_t)n, sum, hi, w, bigint ? 4 : 2);
    uint64_t b;
    memcpy(&b, &d, 8);
    std::printf("%llu\n", (unsigned long long)b);
  }
  return 0;
}
