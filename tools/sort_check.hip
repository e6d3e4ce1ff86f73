// sort_check.hip — test-only entry points for the primitives of csrc/khip_sort.hpp (sort_pairs /
// sort_run, scan_excl, rle_sorted), built into ksql_amd/libkhip_sortcheck.so (make sortcheck) and
// driven by tests/test_gpu_sort.py.  The header lives in an anonymous namespace and has no entry
// in the ABI; this file gives it one, for host arrays.
//
// Every entry allocates its own device buffers.  A buffer a primitive writes is allocated with
// GUARD bytes in front of and behind it, the whole allocation filled with FILL; afterwards the
// guards are compared on the host and SC_E_GUARD is returned if one changed (khip_last_error names
// the buffer), so a store just past either end fails a test instead of passing unseen.  The
// payload keeps FILL wherever the primitive did not write.  No kernels of its own, no
// environment knobs.
#include <string.h>

#include <vector>

#include "../ksql_amd/csrc/khip_sort.hpp"

using namespace khip;

namespace {

constexpr size_t GUARD = 256;
constexpr int FILL = 0xA5;
constexpr int SC_E_GUARD = 100;  // a guard byte changed
constexpr int SC_E_INPUT = 101;  // a read-only input changed

struct Guarded {
  char* base = nullptr;
  size_t bytes = 0;
  const char* name = "";
  Guarded() = default;
  Guarded(const Guarded&) = delete;
  Guarded& operator=(const Guarded&) = delete;
  ~Guarded() {
    if (base) hipFree(base);
  }
  khip_status alloc(size_t b, const char* nm) {
    bytes = b;
    name = nm;
    if (hipMalloc((void**)&base, b + 2 * GUARD) != hipSuccess) {
      base = nullptr;
      return fail(KHIP_E_NOMEM, std::string("hipMalloc failed for ") + nm);
    }
    KHIP_TRY_HIP(hipMemset(base, FILL, b + 2 * GUARD));
    KHIP_TRY_HIP(hipDeviceSynchronize());
    return KHIP_OK;
  }
  template <class T>
  T* p() const { return reinterpret_cast<T*>(base + GUARD); }
  khip_status put(const void* src, size_t b) {
    if (b) KHIP_TRY_HIP(hipMemcpy(base + GUARD, src, b, hipMemcpyHostToDevice));
    return KHIP_OK;
  }
  // The payload's first dst_bytes to dst (may be null); SC_E_GUARD when a guard byte changed.
  int finish(void* dst, size_t dst_bytes) {
    std::vector<unsigned char> h(bytes + 2 * GUARD);
    KHIP_TRY_HIP(hipMemcpy(h.data(), base, h.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < GUARD; i++) {
      if (h[i] != FILL || h[GUARD + bytes + i] != FILL) {
        const bool front = h[i] != FILL;
        set_error(std::string("guard ") + (front ? "before " : "after ") + name + " touched at byte " +
                  std::to_string(front ? (long long)i - (long long)GUARD : (long long)i));
        return SC_E_GUARD;
      }
    }
    if (dst && dst_bytes) memcpy(dst, h.data() + GUARD, dst_bytes);
    return KHIP_OK;
  }
  // SC_E_INPUT when the payload differs from src (a read-only input).
  int unchanged(const void* src) {
    std::vector<unsigned char> h(bytes);
    if (bytes) KHIP_TRY_HIP(hipMemcpy(h.data(), base + GUARD, bytes, hipMemcpyDeviceToHost));
    if (bytes && memcmp(h.data(), src, bytes)) {
      set_error(std::string("input ") + name + " was modified");
      return SC_E_INPUT;
    }
    return KHIP_OK;
  }
};

struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) hipStreamDestroy(s);
  }
  khip_status create() {
    KHIP_TRY_HIP(hipStreamCreate(&s));
    return KHIP_OK;
  }
};

#define SC_TRY(expr)           \
  do {                         \
    int _r = (int)(expr);      \
    if (_r != KHIP_OK) return _r; \
  } while (0)

template <class V>
int sort_case(int cfg, const uint64_t* keys, const V* vals, int64_t n, int end_bit, uint64_t* keys_out, V* vals_out,
              int64_t* info) {
  Stream st;
  SC_TRY(st.create());
  Guarded kin, kout, vin, vout;
  SC_TRY(kin.alloc((size_t)n * 8, "k_in"));
  SC_TRY(kout.alloc((size_t)n * 8, "k_out"));
  SC_TRY(vin.alloc((size_t)n * sizeof(V), "v_in"));
  SC_TRY(vout.alloc((size_t)n * sizeof(V), "v_out"));
  SC_TRY(kin.put(keys, (size_t)n * 8));
  SC_TRY(vin.put(vals, (size_t)n * sizeof(V)));
  DevBuf tmp, alt;
  if (cfg == 0) {
    SC_TRY(ksort::sort_pairs<V>(st.s, tmp, alt, kin.p<uint64_t>(), kout.p<uint64_t>(), vin.p<V>(), vout.p<V>(), n,
                                end_bit));
  } else {  // sort_pairs' pass count, the tile shape it takes only under the tuning build's knob
    const int passes = std::min(8, std::max(1, (end_bit + 7) / 8));
    SC_TRY((ksort::sort_run<512, 16, V>(st.s, tmp, alt, kin.p<uint64_t>(), kout.p<uint64_t>(), vin.p<V>(),
                                        vout.p<V>(), n, passes)));
  }
  KHIP_TRY_HIP(hipStreamSynchronize(st.s));
  info[0] = (int64_t)tmp.bytes;  // histograms + tickets + one status block per pass
  info[1] = (int64_t)alt.bytes;  // the third buffer: allocated only for an even pass count
  SC_TRY(kin.finish(nullptr, 0));
  SC_TRY(vin.finish(nullptr, 0));
  SC_TRY(kout.finish(keys_out, (size_t)n * 8));
  SC_TRY(vout.finish(vals_out, (size_t)n * sizeof(V)));
  return KHIP_OK;
}

template <class I, class O>
int scan_case(const I* in, int64_t n, bool with_total, bool alias, bool want_host, O* out, int64_t* total_host) {
  static_assert(sizeof(I) == sizeof(O), "aliasing needs equal widths");
  Stream st;
  SC_TRY(st.create());
  const size_t nout = (size_t)n + (with_total ? 1 : 0);
  Guarded din, dout;
  SC_TRY(dout.alloc(nout * sizeof(O), alias ? "in/out" : "out"));
  if (alias) {
    SC_TRY(dout.put(in, (size_t)n * sizeof(I)));
  } else {
    SC_TRY(din.alloc((size_t)n * sizeof(I), "in"));
    SC_TRY(din.put(in, (size_t)n * sizeof(I)));
  }
  DevBuf tmp;
  const I* src = alias ? dout.p<I>() : din.p<I>();
  SC_TRY((ksort::scan_excl<I, O>(st.s, tmp, src, dout.p<O>(), n, with_total, want_host ? total_host : nullptr)));
  KHIP_TRY_HIP(hipStreamSynchronize(st.s));
  if (!alias) {
    SC_TRY(din.finish(nullptr, 0));
    SC_TRY(din.unchanged(in));
  }
  SC_TRY(dout.finish(out, nout * sizeof(O)));
  return KHIP_OK;
}

}  // namespace

extern "C" {

// cfg 0: sort_pairs (tiles of 1024 x 8); 1: sort_run<512, 16, V>.  vbytes: 4 or 8.
// info[0] / info[1]: the bytes of the sort's scratch and of its third buffer after the call.
int khip_sortcheck_sort(int cfg, int vbytes, const uint64_t* keys, const void* vals, int64_t n, int end_bit,
                        uint64_t* keys_out, void* vals_out, int64_t* info) {
  clear_error();
  if ((cfg != 0 && cfg != 1) || n < 1 || end_bit < 1 || end_bit > 64) return fail(KHIP_E_INVALID, "sort: bad argument");
  if (vbytes == 4) return sort_case<uint32_t>(cfg, keys, (const uint32_t*)vals, n, end_bit, keys_out, (uint32_t*)vals_out, info);
  if (vbytes == 8) return sort_case<uint64_t>(cfg, keys, (const uint64_t*)vals, n, end_bit, keys_out, (uint64_t*)vals_out, info);
  return fail(KHIP_E_INVALID, "sort: value width");
}

// types 0: <int64, int64>, 1: <int, int>, 2: <uint32, uint32>.  out holds n (+ 1 with_total).
int khip_sortcheck_scan(int types, const void* in, int64_t n, int with_total, int alias, int want_host, void* out,
                        int64_t* total_host) {
  clear_error();
  if (n < 0) return fail(KHIP_E_INVALID, "scan: bad argument");
  if (types == 0) return scan_case<int64_t, int64_t>((const int64_t*)in, n, with_total, alias, want_host, (int64_t*)out, total_host);
  if (types == 1) return scan_case<int, int>((const int*)in, n, with_total, alias, want_host, (int*)out, total_host);
  if (types == 2) return scan_case<uint32_t, uint32_t>((const uint32_t*)in, n, with_total, alias, want_host, (uint32_t*)out, total_host);
  return fail(KHIP_E_INVALID, "scan: type pair");
}

// ukeys / cnt hold n entries, start n + 1 (entries the call did not write keep the fill byte 0xA5).
int khip_sortcheck_rle(const uint64_t* keys, int64_t n, uint64_t* ukeys, int32_t* cnt, int64_t* start,
                       int32_t* nseg_dev, int64_t* nseg_host) {
  clear_error();
  if (n < 1) return fail(KHIP_E_INVALID, "rle: bad argument");
  Stream st;
  SC_TRY(st.create());
  Guarded dk, du, dc, ds, dn;
  SC_TRY(dk.alloc((size_t)n * 8, "key"));
  SC_TRY(du.alloc((size_t)n * 8, "ukeys"));
  SC_TRY(dc.alloc((size_t)n * 4, "cnt"));
  SC_TRY(ds.alloc((size_t)(n + 1) * 8, "start"));
  SC_TRY(dn.alloc(4, "nseg"));
  SC_TRY(dk.put(keys, (size_t)n * 8));
  DevBuf tmp;
  SC_TRY(ksort::rle_sorted(st.s, tmp, dk.p<uint64_t>(), n, du.p<uint64_t>(), dc.p<int>(), ds.p<int64_t>(), dn.p<int>(),
                           nseg_host));
  KHIP_TRY_HIP(hipStreamSynchronize(st.s));
  SC_TRY(dk.finish(nullptr, 0));
  SC_TRY(dk.unchanged(keys));
  SC_TRY(du.finish(ukeys, (size_t)n * 8));
  SC_TRY(dc.finish(cnt, (size_t)n * 4));
  SC_TRY(ds.finish(start, (size_t)(n + 1) * 8));
  SC_TRY(dn.finish(nseg_dev, 4));
  return KHIP_OK;
}

}  // extern "C"
