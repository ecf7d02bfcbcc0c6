// entry.hpp -- the host side every stateless entry point of the appearance chain shares: HIP status ->
// MPMHIP code, the early return, the device argument, the grid size of a one-lane-per-item launch.  Nothing here launches.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mpmhip.h"

namespace entry {

inline int check(hipError_t e) { return e == hipSuccess ? MPMHIP_OK : MPMHIP_ERR_HIP; }

// return the MPMHIP code of a failed HIP call from the enclosing function
#define ENTRY_CHECK(expr) do { if (int rc_ = entry::check(expr)) return rc_; } while (0)

// MPMHIP_ERR_NO_DEVICE unless `device` names a visible device: the half of select_device that an entry point with an
// empty-work return runs before that return, so that nothing is selected for a call that launches nothing
inline int device_in_range(int32_t device) {
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev == 0 || device < 0 || device >= n_dev) return MPMHIP_ERR_NO_DEVICE;
  return MPMHIP_OK;
}

// `device` stays the calling thread's current device on return
inline int select_device(int32_t device) {
  if (int rc = device_in_range(device)) return rc;
  return check(hipSetDevice(device));
}

inline unsigned blocks(int64_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

}  // namespace entry
