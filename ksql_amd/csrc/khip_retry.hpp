// khip_retry.hpp — the partitioned engine's retry protocol on the host: work items,
// and what one pass's fail[] bytes make of the next pass.  Shared by part_push (khip_agg_part.hip)
// and c1_push (khip_agg_c1.hip); no HIP, no ABI: tools/retry_plan_check.cpp builds it alone.
#pragma once

#include <cstdint>
#include <vector>

namespace khip {

// fail[p] bits a merge / aggregate kernel sets for partition p
enum { FAIL_TABLE = 1, FAIL_REGION = 2, FAIL_FATAL = 4 };
constexpr int RETRY_MAX_SBITS = 12;  // at most 4096 sub-passes per partition

// A work item: sub-pass `sub` of the 2^sbits of partition p (p < 2^16, sbits <= 12).
inline uint32_t work_item(uint32_t p, int sbits, uint32_t sub) { return p | ((uint32_t)sbits << 16) | (sub << 20); }
inline uint32_t work_part(uint32_t w) { return w & 0xFFFFu; }
inline int work_sbits(uint32_t w) { return (int)((w >> 16) & 0xFu); }
inline uint32_t work_sub(uint32_t w) { return w >> 20; }

// One push's retry state.
struct RetryPlan {
  std::vector<int> sbits;       // sub-pass bits per partition as of the next pass
  std::vector<uint32_t> work;   // the next pass's items (pass 0: empty = one item per partition)
  std::vector<uint32_t> plist;  // the partitions the next pass re-runs (k_part_commit's list)
  std::vector<uint32_t> image;  // work ++ plist: what the device's work buffer holds for that pass
  bool grow = false;            // some partition's region overflowed: regrow before the next pass
};

inline void retry_queue(RetryPlan& r, int p) {
  for (uint32_t k = 0; k < (1u << r.sbits[p]); k++) r.work.push_back(work_item((uint32_t)p, r.sbits[p], k));
}

// Pass 0 from the learned bits: every partition's 2^sbits items in partition order, or no list at
// all when no partition has sub-passes (the kernels then take one item per partition).
inline void retry_begin(RetryPlan& r, const std::vector<uint8_t>& learned) {
  r.sbits.assign(learned.begin(), learned.end());
  r.work.clear();
  r.plist.clear();
  r.grow = false;
  bool subs = false;
  for (const uint8_t b : learned) subs = subs || b > 0;
  for (int p = 0; subs && p < (int)learned.size(); p++) retry_queue(r, p);
  r.image = r.work;
}

// The next pass from this one's fail[]: a failed partition re-runs ALL its items (one more
// sub-pass bit after a table overflow).  False: a partition would need more than 4096 sub-passes.
inline bool retry_next(RetryPlan& r, const uint8_t* fail, int P) {
  r.grow = false;
  r.plist.clear();
  r.work.clear();
  for (int p = 0; p < P; p++) {
    if (!fail[p]) continue;
    if (fail[p] & FAIL_TABLE) r.sbits[p]++;
    if (fail[p] & FAIL_REGION) r.grow = true;
    if (r.sbits[p] > RETRY_MAX_SBITS) return false;
    r.plist.push_back((uint32_t)p);
    retry_queue(r, p);
  }
  r.image = r.work;
  r.image.insert(r.image.end(), r.plist.begin(), r.plist.end());
  return true;
}

// End of the push: a partition keeps the sub-passes it needed.
inline void retry_learn(std::vector<uint8_t>& learned, const RetryPlan& r) {
  for (size_t p = 0; p < learned.size(); p++)
    if (r.sbits[p] > learned[p]) learned[p] = (uint8_t)r.sbits[p];
}

}  // namespace khip
