// qn_kf_buf.h - the host plumbing every translation unit around a qn_kf_store shares: one error macro, one owned buffer with three ways to grow, one
// get-or-create of a unit's per-store state, one pair of result sets for the units whose results belong to the map slot.  Header only.  Rule of the buffers: a call that fails leaves nothing stale behind - a buffer that could not
// be grown is empty, a slot array that could not be moved is the old one, and the HIP runtime's sticky error is cleared (a hipGetLastError() behind a later
// launch on this thread would otherwise report the old out-of-memory as its own).
#pragma once
#include <hip/hip_runtime.h>
#include <cmath>
#include <new>
#include <string>
#include <utility>
#include "qn_kf_internal.h"

#define QN_KFCHK(s, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { (void)hipGetLastError(); qn_kf_int_set_error((s), (std::string(#call) + " -> " + hipGetErrorString(e_)).c_str()); return QN_ERR_HIP; } } while (0)
inline int qn_kf_fail(qn_kf_store* s, const char* msg) { qn_kf_int_set_error(s, msg); return QN_ERR_HIP; }
inline size_t qn_up16(size_t b) { return (b + 15) & ~(size_t)15; }
// `bytes` of device memory to the host on the store's stream, there when it returns: the one synchronisation of a getter that copies one buffer
inline int qn_kf_download(qn_kf_store* s, void* dst, const void* src, size_t bytes) {
  QN_KFCHK(s, hipSetDevice(qn_kf_int_device(s)));
  const hipStream_t stream = qn_kf_int_stream(s);
  QN_KFCHK(s, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream));
  QN_KFCHK(s, hipStreamSynchronize(stream));
  return QN_OK;
}

// `cap` elements of device (DevBuf) or pinned host (PinBuf) memory, freed with their owner.  Move-only.
template <typename T, bool kPinned> struct KfBuf {
  T* p = nullptr; size_t cap = 0;
  KfBuf() = default;
  KfBuf(KfBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  KfBuf& operator=(KfBuf&& o) noexcept { swap(o); return *this; }      // (o takes the old buffer and frees it)
  ~KfBuf() { reset(); }
  void swap(KfBuf& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); }
  void reset() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; cap = 0;
  }
  // at least `need` elements, the old contents dead: nothing when they fit, else freed first and allocated half again as large (exact: just `need`).
  // false: the buffer is empty and last_error says why (the caller returns QN_ERR_HIP).
  bool grow(qn_kf_store* s, size_t need, bool exact = false) {
    if (need <= cap) return true;
    reset();
    const size_t n = exact ? need : need + need / 2;
    if (!(p = alloc(s, n))) return false;
    cap = n;
    return true;
  }
  // results that must outlive a failed call: room for `need` elements with this buffer untouched - nothing when they fit, else `fresh` is allocated beside
  // it (false: nothing changed).  Once everything the call needs is there, adopt(fresh) makes the larger one this buffer and the old one goes with `fresh`.
  bool grow_beside(qn_kf_store* s, size_t need, KfBuf& fresh) const { return need <= cap || fresh.grow(s, need); }
  void adopt(KfBuf& fresh) noexcept { if (fresh.p) swap(fresh); }
  // slot arrays: new_cap elements whose first `cap` are the old ones, copied on `stream` and synchronised before the old buffer goes.
  // false: the buffer is as it was.
  bool grow_keep(qn_kf_store* s, size_t new_cap, hipStream_t stream) {
    static_assert(!kPinned, "device buffers only");
    KfBuf g;
    if (!(g.p = alloc(s, new_cap))) return false;
    g.cap = new_cap;
    if (cap) {
      hipError_t e = hipMemcpyAsync(g.p, p, sizeof(T) * cap, hipMemcpyDeviceToDevice, stream);
      if (e == hipSuccess) e = hipStreamSynchronize(stream);
      if (e != hipSuccess) return failed(s, "moving a slot array -> ", e);
    }
    swap(g);
    return true;
  }
  // exactly the n elements at `host`, copied before it returns (tables)
  bool assign(qn_kf_store* s, const T* host, size_t n) {
    static_assert(!kPinned, "device buffers only");
    reset();
    if (!(p = alloc(s, n))) return false;
    cap = n;
    const hipError_t e = hipMemcpy(p, host, sizeof(T) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) return true;
    reset();
    return failed(s, "hipMemcpy -> ", e);
  }

 private:
  static T* alloc(qn_kf_store* s, size_t n) {
    void* q = nullptr;
    const hipError_t e = kPinned ? hipHostMalloc(&q, sizeof(T) * n, hipHostMallocDefault) : hipMalloc(&q, sizeof(T) * n);
    if (e != hipSuccess) failed(s, kPinned ? "hipHostMalloc -> " : "hipMalloc -> ", e);
    return e == hipSuccess ? (T*)q : nullptr;
  }
  // every failure of a buffer ends here: the sticky error cleared, last_error set
  static bool failed(qn_kf_store* s, const char* what, hipError_t e) {
    (void)hipGetLastError();
    qn_kf_int_set_error(s, (std::string(what) + hipGetErrorString(e)).c_str());
    return false;
  }
};

// the state a translation unit keeps in extension slot `slot`, made on first use (first_use(st): QN_OK, or a status with which nothing is registered) and
// deleted by the store once its stream has drained
template <typename St, typename FirstUse> int qn_kf_ext_state(qn_kf_store* s, int slot, St** out, FirstUse first_use) {
  St* st = (St*)qn_kf_int_ext(s, slot);
  if (!st) {
    st = new (std::nothrow) St();
    if (!st) return qn_kf_fail(s, "qn_kf: out of memory");
    const int rc = first_use(st);
    if (rc != QN_OK) { delete st; return rc; }
    qn_kf_int_set_ext(s, slot, st, [](void* p) { delete (St*)p; });
  }
  *out = st;
  return QN_OK;
}
template <typename St> int qn_kf_ext_state(qn_kf_store* s, int slot, St** out) {
  return qn_kf_ext_state(s, slot, out, [](St*) { return QN_OK; });
}

// The per-store state of a unit whose results belong to the map slot as it stood at one generation (qn_mapnormals.hip, qn_mapoutliers.hip, qn_mapground.hip):
// two result sets, the live one holding what the latest successful call computed for the map of generation `gen` with its n points.  A call writes spare()
// and commits on success, so a refused call leaves the previous results as they were.
template <typename Set> struct KfMapResults {
  bool live = false; uint64_t gen = 0; uint32_t n = 0; int cur = 0;
  Set set[2];
  Set& spare() { return set[live ? 1 - cur : cur]; }
  void commit(uint64_t map_gen, uint32_t map_n) { if (live) cur = 1 - cur; live = true; gen = map_gen; n = map_n; }
  // the live set of the state in extension slot `slot` if it is that of the map slot as it stands (*map its records, *n their number), else nullptr
  static const Set* lookup(qn_kf_store* s, int slot, const float4** map, uint32_t* n) {
    const KfMapResults* st = (const KfMapResults*)qn_kf_int_ext(s, slot);
    uint64_t map_gen = 0;
    *map = qn_kf_int_map(s, n, &map_gen);
    return st ? st->current(s, map, n) : nullptr;
  }
  // the same for a state that is reached another way than as a slot of its own
  const Set* current(qn_kf_store* s, const float4** map, uint32_t* map_n) const {
    uint64_t map_gen = 0;
    *map = qn_kf_int_map(s, map_n, &map_gen);
    return live && *map && gen == map_gen && n == *map_n ? &set[cur] : nullptr;
  }
};

// the largest e with x 2^e <= 2^bits, within the exponents of normal f32 powers of two (the twins' quant_exponent): the scale 2^e of a unit's integers
inline int qn_quant_exponent(double x, int bits) {
  int ex = 0;
  const double m = std::frexp(x, &ex);                   // x = m 2^ex, 0.5 <= m < 1
  const int e = (m == 0.5 ? bits + 1 : bits) - ex;
  return e < -126 ? -126 : e > 127 ? 127 : e;
}
