// launch_layout.hpp -- which workgroup of a substep launch does what: the XCD remap of the work items and the layout of the
// workgroups that ride in the chunk launches.  Plain integer arithmetic, no HIP beyond __host__ / __device__ (the includer brings
// those): the host lays a launch out with it, the kernels decode blockIdx with it, tests/hostlayout/ walks it with g++.
#pragma once

namespace mpm {
inline namespace fk {

// XCD-aware remap: consecutive workgroup ids land on different XCDs (observed: id % 8).  Work items are sorted by
// grid block, so runs of XCD_RUN consecutive items (neighbouring tiles) are given to the same XCD to share its L2,
// while successive runs rotate over the 8 XCDs so that a spatially concentrated load (e.g. the blocks around the
// body collider) is spread over the whole chip instead of landing on one or two XCDs.
#ifndef MPM_XCD_RUN
#define MPM_XCD_RUN 16  // (experiment switch; 8 and 32 measured in round 5)
#endif
constexpr int XCD_RUN = MPM_XCD_RUN;
__device__ __forceinline__ int xcd_slice(int w, int n) {
  int xcd = w & 7, idx = w >> 3;
  int i = ((idx / XCD_RUN) * 8 + xcd) * XCD_RUN + (idx % XCD_RUN);
  return i < n ? i : -1;
}
__host__ __device__ inline unsigned xcd_grid(int n) { return (unsigned)(((n + 8 * XCD_RUN - 1) / (8 * XCD_RUN)) * (8 * XCD_RUN)); }

// The p2g launch (and k_g2p2g) carries up to five kinds of workgroup besides its chunks' own, in blockIdx order:
//   [0, n_fbins)                    body-face splat bins, one each
//   [n_fbins, n_fbins + n_joint)    joint splats
//   [.., n_riders)                  padding: the riders are rounded up to a multiple of 8, which keeps the XCD mapping of the chunks
//   [n_riders, z_first)             chunk slots on the XCD-remapped grid (xcd_grid(n_chunks) of them; slots past the list are holes)
//   [z_first, pack_first)           clearing of the other accumulator buffer: the tail of the launch
//   [pack_first, grid)              (sharded runs) halo pack, once everything in front of the clearing workgroups has scattered
// The riders go in front: the longest workgroups of the launch start first.  A launch of riders alone (a phase of a profiling run;
// the splat pass in front of the stress launch, k_stress_elem_splat) is the same layout with no chunks.
struct LaunchLayout {
  int n_fbins, n_joint, n_riders, n_chunks, z_first, pack_first, n_pack;
  __host__ __device__ int n_clear() const { return pack_first - z_first; }
  // the workgroups that scatter -- riders, padding, chunk slots, holes: each counts itself done for the pack workgroups (PackArgs)
  __host__ __device__ int n_scatter() const { return z_first; }
  __host__ __device__ unsigned grid() const { return (unsigned)(pack_first + n_pack); }
};
__host__ __device__ inline LaunchLayout launch_layout(int n_fbins, int n_joint, int n_chunks, int n_clear, int n_pack) {
  LaunchLayout L;
  L.n_fbins = n_fbins; L.n_joint = n_joint; L.n_chunks = n_chunks; L.n_pack = n_pack;
  L.n_riders = (n_fbins + n_joint + 7) & ~7;
  L.z_first = L.n_riders + (int)xcd_grid(n_chunks);
  L.pack_first = L.z_first + n_clear;
  return L;
}

enum WgKind { WG_FACE, WG_JOINT, WG_PAD, WG_CHUNK, WG_CLEAR, WG_PACK };
// index: within the role (the bin, the joint / clearing / pack workgroup); WG_CHUNK: into the chunk list, -1 for a hole; WG_PAD: 0
struct WgRole { int kind, index; };
// The chunk slots by themselves, for the kernels whose chunk workgroups are the launch: they ask wg_is_chunk first and take wg_role
// only for the others.  (Taken from wg_role's value alone, hipcc keeps `kind` in a register and dispatches on it a second time at
// the head of every chunk workgroup: profiles/rider_layout_ab.md.)
__device__ __forceinline__ bool wg_is_chunk(int bid, const LaunchLayout &L) { return bid >= L.n_riders && bid < L.z_first; }
__device__ __forceinline__ int wg_chunk(int bid, const LaunchLayout &L) { return xcd_slice(bid - L.n_riders, L.n_chunks); }
__device__ __forceinline__ WgRole wg_role(int bid, const LaunchLayout &L) {
  if (wg_is_chunk(bid, L)) return WgRole{WG_CHUNK, wg_chunk(bid, L)};
  if (bid < L.n_riders) {
    if (bid < L.n_fbins) return WgRole{WG_FACE, bid};
    if (bid < L.n_fbins + L.n_joint) return WgRole{WG_JOINT, bid - L.n_fbins};
    return WgRole{WG_PAD, 0};
  }
  if (L.n_pack && bid >= L.pack_first) return WgRole{WG_PACK, bid - L.pack_first};
  return WgRole{WG_CLEAR, bid - L.z_first};
}

}  // namespace fk
}  // namespace mpm
