// The scratch that skeleton.hip and separators.hip each keep an instance of (DESIGN.md "Shared line machinery"): it
// carries the seeds and directions of the lanes from the counting half of a call to its filling half.
#pragma once

#include "common.hpp"

namespace ndsm {
namespace {

// Scratch of a file's calls, kept between calls and grown on demand (no result depends on its size): `lead` 8-byte
// slots of the file's own, then the seed (3 doubles) and the direction (1 double) of every lane, written by the
// counting half and read again by the filling half.  Each file keeps one instance and hands at_reset a function that
// calls its release().
struct LineScratch {
  size_t lead;                 // leading 8-byte slots
  void (*on_reset)();          // calls release() of this instance
  double *buf = nullptr;
  size_t cap = 0;              // lanes the buffer holds
  size_t lanes = 0;            // lanes the last counting half wrote
  bool registered = false;     // on_reset is queued for the next reset

  double *seeds() const { return buf + lead; }
  double *sgns(size_t nl) const { return buf + lead + 3 * nl; }

  void release() {
    if (buf) (void)hipFree(buf);
    buf = nullptr;
    cap = lanes = 0;
    registered = false;
  }

  int grow(size_t nl) {
    if (!registered) {
      ndsm::at_reset(on_reset);
      registered = true;
    }
    lanes = 0;
    if (nl <= cap) return 0;
    if (buf) {
      const int rc = ndsmk_free(buf);      // (drains the streams first)
      buf = nullptr;
      cap = 0;
      if (rc != 0) return rc;
    }
    void *q = nullptr;
    const int rc = ndsmk_alloc(&q, sizeof(double) * (lead + 4 * nl));
    if (rc != 0) return rc;
    buf = (double *)q;
    cap = nl;
    return 0;
  }
};

}  // namespace
}  // namespace ndsm
