// What every qn_map header writes the same way, once: the text of a refused library call, the check that throws it, and "the caller's parameters or the
// library's defaults".  The next helper over the C-ABI starts from here, not from a copy of another header's lines: its own std::invalid_argument checks first,
// then params_or, the library call and check.  Header-only, everything inline; uses nothing from Eigen or PCL.
#pragma once
#include <stdexcept>
#include <string>
#include "qn_engine.h"

namespace qn_map {
namespace detail {

// "[qn_map] call: status", then the store's last error when there is a store
inline std::string why(const char* call, int rc, qn_kf_store* store) {
  return std::string("[qn_map] ") + call + ": " + qn_status_str(rc) + (store ? std::string(" ") + qn_kf_last_error(store) : std::string());
}

// throws why(call, rc, store) as a std::runtime_error unless rc is QN_OK - or also_ok: QN_ERR_CAPACITY for the first call of a size probe.  A null store is
// named too ("... null store"): the library refuses it, and its last-error text says why.
inline void check(qn_kf_store* store, int rc, const char* call, int also_ok = QN_OK) {
  if (rc != QN_OK && rc != also_ok) throw std::runtime_error(why(call, rc, nullptr) + " " + qn_kf_last_error(store));
}

// the caller's parameter record, or the library's defaults for a null pointer: params_or(params, qn_route_default_params)
template <typename P>
inline P params_or(const P* params, void (*defaults)(P*)) {
  P p;
  if (params) p = *params; else defaults(&p);
  return p;
}

}  // namespace detail
}  // namespace qn_map
