// The launch layout (mpmavatar_amd/csrc/launch_layout.hpp) compiled for the host (tests/test_launch_layout_host.py; the stand-in for
// <hip/hip_runtime.h> is tests/hostmath/stub): the layout the host makes from the five counts, and the role the kernels' own decode
// gives every blockIdx of the launch.
#include <hip/hip_runtime.h>

#include "launch_layout.hpp"

#include <cstdint>

using namespace mpm;

extern "C" int32_t hl_xcd_run() { return XCD_RUN; }

// out = {n_riders, z_first, pack_first, n_scatter, n_clear, grid}
extern "C" void hl_layout(int32_t n_fbins, int32_t n_joint, int32_t n_chunks, int32_t n_clear, int32_t n_pack, int32_t *out) {
  const LaunchLayout L = launch_layout(n_fbins, n_joint, n_chunks, n_clear, n_pack);
  out[0] = L.n_riders; out[1] = L.z_first; out[2] = L.pack_first; out[3] = L.n_scatter(); out[4] = L.n_clear(); out[5] = (int32_t)L.grid();
}

// kind[bid], index[bid] for bid in [0, grid); both arrays hold `cap` entries.  Returns the grid size, or -1 if it exceeds cap.
extern "C" int32_t hl_walk(int32_t n_fbins, int32_t n_joint, int32_t n_chunks, int32_t n_clear, int32_t n_pack, int32_t cap, int32_t *kind,
                           int32_t *index) {
  const LaunchLayout L = launch_layout(n_fbins, n_joint, n_chunks, n_clear, n_pack);
  const int32_t grid = (int32_t)L.grid();
  if (grid > cap) return -1;
  for (int32_t bid = 0; bid < grid; ++bid) {
    const WgRole r = wg_role(bid, L);
    kind[bid] = r.kind; index[bid] = r.index;
  }
  return grid;
}

extern "C" void hl_kinds(int32_t *out) {
  out[0] = WG_FACE; out[1] = WG_JOINT; out[2] = WG_PAD; out[3] = WG_CHUNK; out[4] = WG_CLEAR; out[5] = WG_PACK;
}
