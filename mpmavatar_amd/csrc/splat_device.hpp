// splat_device.hpp -- the two splats that ride in the p2g launches as extra workgroups: the body-face collider splat (compute_mesh,
// mpm_solver.py:829-880) and the joint splat (add_velocity_{traditional,verts,faces}, mpm_solver.py:677-788).
// Included by p2g_device.hpp below its DPP pre-reduction (SegMask, seg_masks, seg_scan4), which the large-bin form shares.
//
// Body faces are binned by grid block at each face sort (k_face_keys: key = block and cell of the centroid, face_centroid below).
// Per substep one workgroup per non-empty bin on the active list (FaceBin) evaluates its faces -- centroid, mean vertex velocity, unit
// normal, with the caller's mesh advection applied: face_eval -- and accumulates weight, weight * velocity (collider channels 0-3,
// "pass 0", PASSES bit 0) and weight * normal (channels 4-6, "pass 1", PASSES bit 1) in an fp64 LDS tile of 8 x 8 x 8 nodes, which
// col_splat_flush adds to the block-major collider channels.  Faces in blocks off the active list cannot reach a node that carries mass
// and have no workgroup; a face that left its bin's tile margin since the face sort adds its nodes with global atomics
// (col_add_global) and raises CNT_FACE, which makes the next re-sort bin the faces again.  col_splat_wg picks one of three forms:
//   col_splat_small_onepass   bins of <= SPLAT_SMALL faces, both passes: lane = (face, stencil node), ONE pass through a seven-channel
//                             tile (SplatTile7)
//   col_splat_small<PASSES>   the same lanes, one of the two passes through the four-channel tile of p2g (SplatTile4)
//   col_splat_large<PASSES>   larger bins: lane = face with the segmented DPP pre-reduction, one or both passes through the
//                             four-channel tile, PT faces at a time
// Launches: k_stress_elem_splat runs col_splat_wg<1> and k_p2g col_splat_wg<2> where the two passes ride in different launches (cloth
// scenes, SplatArgs::splat_passes == 2); otherwise k_p2g, and always k_g2p2g, run col_splat_wg<3>.
// (Tried and dropped: gathering the faces per node block inside the grid stage -- no atomics at all, but the few wavefronts next to the
// body serialise ~50 faces x 60 dependent instructions each and set the kernel's tail.)
#pragma once
#include "fast_device.hpp"

namespace mpm {
inline namespace fk {

__device__ __forceinline__ bool splat_ok(int G, const Stencil &s) {
  return s.bx >= 0 && s.bx < G - 3 && s.by >= 0 && s.by < G - 3 && s.bz >= 0 && s.bz < G - 3;
}
// does a stencil whose base node is (lx, ly, lz) in tile coordinates fit the tile?
__device__ __forceinline__ bool in_margin(int lx, int ly, int lz) { return !((unsigned)lx > 5u || (unsigned)ly > 5u || (unsigned)lz > 5u); }

// ---- face evaluation: the kernel that bins a face (k_face_keys) and the kernels that splat it share this text
__device__ __forceinline__ void load_face(const int32_t *idx, int f, int &i0, int &i1, int &i2) {
  i0 = idx[3 * f]; i1 = idx[3 * f + 1]; i2 = idx[3 * f + 2];
}
__device__ __forceinline__ V3 face_centroid(const float *pts, const float *vel, float adv, int i0, int i1, int i2, V3 &p0, V3 &p1, V3 &p2) {
  p0 = mesh_point(pts, vel, adv, i0); p1 = mesh_point(pts, vel, adv, i1); p2 = mesh_point(pts, vel, adv, i2);
  return v3((p0.x + p1.x + p2.x) / 3.0f, (p0.y + p1.y + p2.y) / 3.0f, (p0.z + p1.z + p2.z) / 3.0f);
}
// mean vertex velocity a, unit normal fn and the stencil of the centroid of face (i0, i1, i2).  (Vertex indices, not a face number:
// the one-pass form requests its first indices ahead of everything else.)
__device__ __forceinline__ void face_eval(const float *pts, const float *vel, float adv, int i0, int i1, int i2, float inv_dx, V3 &a,
                                          V3 &fn, Stencil &s) {
  V3 p0, p1, p2;
  V3 fp = face_centroid(pts, vel, adv, i0, i1, i2, p0, p1, p2);
  V3 u0 = load_v3(vel + 3 * i0), u1 = load_v3(vel + 3 * i1), u2 = load_v3(vel + 3 * i2);
  a = v3((u0.x + u1.x + u2.x) / 3.0f, (u0.y + u1.y + u2.y) / 3.0f, (u0.z + u1.z + u2.z) / 3.0f);
  fn = normalize(cross(p1 - p0, p2 - p0));  // wp.mesh_eval_face_normal
  s = make_stencil(fp, inv_dx);
}

// non-empty face bins that lie on the active list (order irrelevant), as self-contained records
struct FaceBin { int blk, start, cnt, pad; };

// ---- joint splat (add_velocity_{traditional,verts,faces}, mpm_solver.py:677-788) as ONE launch: 32 lanes per joint
// particle, lane = stencil node (27 used), so every thread has a single short dependency chain instead of a 27-trip
// loop of dependent loads.  Group 0: the last n_t traditional particles, group 1: the first n_v vertices, group 2:
// the first n_f elements (caller-order indices; inv[] maps them to sorted slots).
struct JointSplatArgs {
  const float *vel_t, *vel_v, *vel_f;
  int n_t, n_v, n_f;
  int off_t, off_v;  // caller-order index of the first particle of group 0 / group 1 (group 2 starts at 0)
  const int *inv;    // caller order -> sorted slot
  const int *perm;   // sorted slot -> caller order
  int t_in_tile;     // 1: group 0 is splatted by the p2g chunks themselves (second tile pass), not by mover_splat_wg
};
// (weight, weight * joint velocity) of one node into the mover channels with global atomics
__device__ __forceinline__ void mov_add_global(const GridPtrs &g, const Dims &d, int x, int y, int z, float w, V3 pv) {
  int blk = blk_of(x, y, z, d.NB);
  if (!g.ab_flag[blk]) { atomicAdd(g.counters + CNT_DROPPED, 1); return; }
  float *p = g.mov + ((size_t)blk * GCH_MOV) * 64 + loc_of(x, y, z);
  atomicAdd(p, w);
  atomicAdd(p + 64, w * pv.x); atomicAdd(p + 128, w * pv.y); atomicAdd(p + 192, w * pv.z);
}
__device__ __forceinline__ void mover_splat_wg(const Bufs &b, const JointSplatArgs &js, int wg, const Dims &d,
                                               const GridPtrs &g) {
  const int *inv = js.inv;
  int t = wg * PT + (int)threadIdx.x;
  int q = (t >> 5) + (js.t_in_tile ? js.n_t : 0), nn = t & 31;
  if (nn >= 27 || q >= js.n_t + js.n_v + js.n_f) return;
  const float *vel;
  int orig;
  if (q < js.n_t) { vel = js.vel_t + 3 * (size_t)q; orig = js.off_t + q; }
  else if (q < js.n_t + js.n_v) { vel = js.vel_v + 3 * (size_t)(q - js.n_t); orig = js.off_v + (q - js.n_t); }
  else { vel = js.vel_f + 3 * (size_t)(q - js.n_t - js.n_v); orig = q - js.n_t - js.n_v; }
  Stencil s = make_stencil(ld3(b.all, A_X, inv[orig]), d.inv_dx);
  if (!splat_ok(d.G, s)) return;  // mpm_solver.py:692,730,767
  int i = nn / 9, j = (nn / 3) % 3, k = nn % 3;
  mov_add_global(g, d, s.bx + i, s.by + j, s.bz + k, stencil_w(s, i, j, k), load_v3(vel));
}
// joint splat of one out-of-margin particle (second tile pass of k_p2g<.., JT = true>)
__device__ __forceinline__ void mover_escaped(V3 x, V3 pv, const Dims &d, const GridPtrs &g) {
  Stencil s = make_stencil(x, d.inv_dx);
#pragma unroll 1
  for (int n = 0; n < 27; ++n) {
    int i = n / 9, j = (n / 3) % 3, k = n % 3;
    mov_add_global(g, d, s.bx + i, s.by + j, s.bz + k, stencil_w(s, i, j, k), pv);
  }
}

// The two splats are small, latency-bound and independent of the particle transfer, so they ride along in the p2g
// LAUNCH as extra workgroups (k_p2g: wg_role, launch_layout.hpp) instead of being kernels of their own: as separate launches
// they either sit on the critical path (17 us) or, on a side stream, cost two cross-queue barrier packets per
// substep (~6 us of idle GPU each, measured with rocprofv3 --kernel-trace).
struct SplatArgs {
  const float *pts, *vel;  // body mesh at this substep: pts + adv * vel
  float adv;
  const int *fidx;         // [n_f][3] vertex ids in bin order
  const FaceBin *fbins;
  int n_fbins;             // workgroups [0, n_fbins): one face bin each
  int splat_passes;        // 3: both passes of the body-face splat here; 2: only the normal pass (pass 0 rode in the stress launch)
  JointSplatArgs js;       // workgroups [n_fbins, n_fbins + n_mov_wg): joints
  int n_mov_wg;
  int n_extra;             // LaunchLayout::n_riders
  ZeroArgs z;              // workgroups [z_first, z_first + z.n_wg), after the chunk workgroups: clear the other
  int z_first;             // accumulator buffer
  PackArgs pack;           // workgroups [pack.first, ...) after those: multi-GPU halo pack (see PackArgs)
};
// Where each kind of workgroup begins is LaunchLayout's arithmetic (launch_layout.hpp) and nobody else's: the host copies a layout in,
// the kernels read it back for wg_role.  (z.n_wg and pack.n_wg are the host's inputs to the layout and stay the caller's.)
inline void set_layout(SplatArgs &sa, const LaunchLayout &L) {
  sa.n_fbins = L.n_fbins; sa.n_mov_wg = L.n_joint; sa.n_extra = L.n_riders;
  sa.z_first = L.z_first; sa.pack.first = L.pack_first;
}
__device__ __forceinline__ LaunchLayout layout_of(const SplatArgs &sa, int n_chunks) {
  return LaunchLayout{sa.n_fbins, sa.n_mov_wg, sa.n_extra, n_chunks, sa.z_first, sa.pack.first, sa.pack.n_wg};
}

// ---- body-face splat: the pieces the three forms share ----
// The two tile layouts: node (i, j, k) of channel c at c * CS + i * SI + j * SJ + k.
// Seven channels at once (weight, weight * velocity, weight * normal) at strides (67, 8, 1) -- 2 * (67 i + 8 j + k) mod 64 puts 25 of a
// face's 27 nodes into different bank pairs -- so that a small bin costs one clearing, one scatter and one flush instead of two of each
// with five barriers in between.  The workgroup tile is 7 * 536 doubles = 30 KB instead of 24.6 KB: still five workgroups per CU
// (VGPR-bound at five).  The experiment that sent small bins through the four-channel tile in two passes instead (the LDS cut alone)
// is recorded in profiles/r05_experiments.md: slower.
constexpr int SPLAT7_SI = 67, SPLAT7_SJ = 8, SPLAT7_S = 536;  // 7*67 + 7*8 + 7 = 532 < 536
struct SplatTile7 { static constexpr int SI = SPLAT7_SI, SJ = SPLAT7_SJ, CS = SPLAT7_S; };
struct SplatTile4 { static constexpr int SI = TS_I, SJ = TS_J, CS = TILE_PAD; };  // the chunk tile of p2g (tile_idx)
constexpr int P2G_TILE_DOUBLES = 7 * SPLAT7_S > 4 * TILE_PAD ? 7 * SPLAT7_S : 4 * TILE_PAD;  // LDS tile of the launches that run col_splat_wg<3>
static_assert(7 * SPLAT7_S <= P2G_TILE_DOUBLES && 4 * TILE_PAD <= P2G_TILE_DOUBLES, "the seven-channel tile and the chunk tile share it");
constexpr int SPLAT_SMALL = 32;  // faces per bin up to which the splat workgroup maps lanes to (face, node) pairs

// block, tile origin of a bin
struct BinTile { int bx, by, bz, ox, oy, oz; };

__device__ __forceinline__ float *col_node(const GridPtrs &g, int nb, int x, int y, int z) {  // channel c of the node at [64 * c]
  return g.col + ((size_t)nb * GCH_COL) * 64 + loc_of(x, y, z);
}
// One node of a face that left its bin's tile margin, with global atomics: (w, w a) into channels 0-3 (PASSES bit 0; sets col_flag),
// w fn into channels 4-6 (bit 1).  A node in a block off the active list is never read by g2p and gets nothing.
template <int PASSES>
__device__ __forceinline__ void col_add_global(const GridPtrs &g, const Dims &d, int x, int y, int z, float w, V3 a, V3 fn) {
  int nb = blk_of(x, y, z, d.NB);
  if (!g.ab_flag[nb]) return;
  float *p = col_node(g, nb, x, y, z);
  if (PASSES & 1) {
    __hip_atomic_store(&g.col_flag[nb], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(p, w);
    atomicAdd(p + 64, w * a.x); atomicAdd(p + 128, w * a.y); atomicAdd(p + 192, w * a.z);
  }
  if (PASSES & 2) { atomicAdd(p + 256, w * fn.x); atomicAdd(p + 320, w * fn.y); atomicAdd(p + 384, w * fn.z); }
}
// Tile -> collider channels.  PASSES 1: tile channels 0-3 -> collider channels 0-3, 2: tile channels 0-2 -> collider channels 4-6,
// 3: the seven of SplatTile7.  A node without weight got nothing at all (pass 1 alone has no weight channel: all three components
// zero); nodes outside the grid or in a block off the active list (act_mask: bit n = neighbour block n of the bin's) are skipped.
template <int PASSES, class T>
__device__ __forceinline__ void col_splat_flush(const double *tile, const BinTile &bt, unsigned long long act_mask, const Dims &d,
                                                const GridPtrs &g) {
  constexpr int NCH = PASSES == 3 ? 7 : (PASSES == 1 ? 4 : 3);
  for (int t = threadIdx.x; t < TILE3; t += PT) {
    int ti = t >> 6, tj = (t >> 3) & 7, tk = t & 7;
    const double *q = tile + (ti * T::SI + tj * T::SJ + tk);
    float c0 = (float)q[0];
    if (PASSES & 1 ? c0 == 0.0f : (c0 == 0.0f && (float)q[T::CS] == 0.0f && (float)q[2 * T::CS] == 0.0f)) continue;
    int x = bt.ox + ti, y = bt.oy + tj, z = bt.oz + tk;
    if (!in_grid(x, y, z, d.G)) continue;
    int nb = blk_of(x, y, z, d.NB);
    int nidx = (((x >> 2) - bt.bx + 1) * 3 + ((y >> 2) - bt.by + 1)) * 3 + ((z >> 2) - bt.bz + 1);
    if (!((act_mask >> nidx) & 1ull)) continue;  // inactive block: never read by g2p, never re-zeroed
    float *p = col_node(g, nb, x, y, z) + (PASSES == 2 ? 256 : 0);
    atomicAdd(p, c0);
#pragma unroll
    for (int c = 1; c < NCH; ++c) atomicAdd(p + 64 * c, (float)q[c * T::CS]);
    if (PASSES & 1) __hip_atomic_store(&g.col_flag[nb], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---- small bins (the common case once the cloth has draped: ~740 bins of ~27 faces): lane = (face, stencil node), 8 faces x 32 lanes
// (27 used) per step, <= 4 steps -- instead of lane = face with a 27-trip node loop of dependent DPP scans that 230 of the 256 lanes
// sit out.  Such a workgroup used to live 10-17 us (two 3 us scatter passes, profiles/r03_wg_timeline.md); what is left is its chain
// of loads and the flush.
// both passes, one pass through the seven-channel tile
__device__ __forceinline__ void col_splat_small_onepass(double *tile, const SplatArgs &sa, const FaceBin &fb, const BinTile &bt,
                                                        bool nb_act, const Dims &d, const GridPtrs &g) {
  const int l = threadIdx.x, fi = l >> 5, n = l & 31;
  const int ni = n / 9, nj = (n / 3) % 3, nk = n % 3;
  // the first pair's face indices are requested together with the block flags, BEFORE the tile is cleared: behind the barrier they
  // were a memory level of their own (record -> flags -> [clear, barrier] -> indices -> vertices; now record -> flags + indices -> vertices)
  int pre_i[2][3];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = u * 8 + fi;
    load_face(sa.fidx, q < fb.cnt ? fb.start + q : fb.start, pre_i[u][0], pre_i[u][1], pre_i[u][2]);
  }
  for (int t = l; t < 7 * SPLAT7_S; t += PT) tile[t] = 0.0;
  __syncthreads();
  WGT(g, 0, 2);  // (debug build: bin record, block flags, tile cleared)
  // this lane's (face, node) of step `it`: node weight, face velocity, normal and stencil; false = no face, or one outside the grid
  auto lane_face = [&](int it, bool pre, float &w, V3 &a, V3 &fn, Stencil &s) -> bool {
    const int q = it * 8 + fi;
    int i0, i1, i2;
    if (pre) { i0 = pre_i[it & 1][0]; i1 = pre_i[it & 1][1]; i2 = pre_i[it & 1][2]; }  // (it < 2 only)
    else load_face(sa.fidx, q < fb.cnt ? fb.start + q : fb.start, i0, i1, i2);
    face_eval(sa.pts, sa.vel, sa.adv, i0, i1, i2, d.inv_dx, a, fn, s);
    w = stencil_w(s, ni, nj, nk);
    return q < fb.cnt && n < 27 && splat_ok(d.G, s);  // mpm_solver.py:858
  };
  // Two steps' loads in flight at a time, then their LDS atomics; the global atomics of the out-of-margin lanes wait until all
  // steps are through.  With those inside the load loop (they may alias the vertex arrays) the compiler kept the four steps in
  // order and a bin paid index -> vertex latency four times: 5.3 us of the workgroup's 11 (profiles/r04_experiments.md 15); all
  // four steps' loads at once are 84 registers of raw vertex data and cost the whole kernel a wavefront per SIMD.
  unsigned esc_mask = 0;  // steps whose face left the tile margin since the faces were binned
#pragma unroll
  for (int h = 0; h < SPLAT_SMALL / 8; h += 2) {
    if (h * 8 >= fb.cnt) break;  // (workgroup-uniform: a bin of at most 16 faces -- the average is 13 -- is done after the first pair)
    float w[2];
    V3 a[2], fn[2];
    int off[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      Stencil s;
      const bool ok = lane_face(h + u, h == 0, w[u], a[u], fn[u], s);
      const int lx = s.bx - bt.ox, ly = s.by - bt.oy, lz = s.bz - bt.oz;
      const bool in_tile = in_margin(lx, ly, lz);
      off[u] = (ok && in_tile) ? (lx + ni) * SPLAT7_SI + (ly + nj) * SPLAT7_SJ + (lz + nk) : -1;
      if (ok && !in_tile) esc_mask |= 1u << (h + u);
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (off[u] >= 0) {
        double *p = tile + off[u];
        atomicAdd(p, (double)w[u]);
        atomicAdd(p + SPLAT7_S, (double)(w[u] * a[u].x)); atomicAdd(p + 2 * SPLAT7_S, (double)(w[u] * a[u].y));
        atomicAdd(p + 3 * SPLAT7_S, (double)(w[u] * a[u].z));
        atomicAdd(p + 4 * SPLAT7_S, (double)(w[u] * fn[u].x)); atomicAdd(p + 5 * SPLAT7_S, (double)(w[u] * fn[u].y));
        atomicAdd(p + 6 * SPLAT7_S, (double)(w[u] * fn[u].z));
      }
    asm volatile("" : "+v"(esc_mask)::"memory");  // (the next pair's loads stay behind this pair's)
  }
  if (esc_mask) {  // rare: this lane's node through global atomics; the flag makes the next re-sort bin the faces again
    raise_drift(g.counters, g.step_id);
    raise_face(g.counters, g.step_id);
#pragma unroll 1
    for (int it = 0; it < SPLAT_SMALL / 8; ++it) {
      if (!((esc_mask >> it) & 1u)) continue;
      float w;
      V3 a, fn;
      Stencil s;
      (void)lane_face(it, false, w, a, fn, s);
      col_add_global<3>(g, d, s.bx + ni, s.by + nj, s.bz + nk, w, a, fn);
    }
  }
  WGT(g, 0, 3);  // faces loaded, LDS atomics of wavefront 0 out
  // (the ballot -- i.e. the wait for the block flags -- right before the flush: in front of the tile clearing it was one more dependent
  // memory level at the head of the workgroup)
  const unsigned long long act_mask = __ballot(nb_act);
  __syncthreads();
  WGT(g, 0, 4);
  col_splat_flush<3, SplatTile7>(tile, bt, act_mask, d, g);
}

// one of the two passes (they ride in different launches) through the four-channel tile
template <int PASSES>
__device__ __forceinline__ void col_splat_small(double *tile, const SplatArgs &sa, const FaceBin &fb, const BinTile &bt, bool nb_act,
                                                const Dims &d, const GridPtrs &g) {
  static_assert(PASSES == 1 || PASSES == 2, "both passes in one workgroup: col_splat_small_onepass");
  const unsigned long long act_mask = __ballot(nb_act);
  const int l = threadIdx.x, fi = l >> 5, n = l & 31;
  const int ni = n / 9, nj = (n / 3) % 3, nk = n % 3;
  for (int t = l; t < 4 * TILE_PAD; t += PT) tile[t] = 0.0;
  __syncthreads();
#pragma unroll
  for (int it = 0; it < SPLAT_SMALL / 8; ++it) {
    if (it * 8 >= fb.cnt) break;  // (workgroup-uniform: no face left for this step)
    const int q = it * 8 + fi;
    int i0, i1, i2;
    load_face(sa.fidx, q < fb.cnt ? fb.start + q : fb.start, i0, i1, i2);
    V3 a, fn;
    Stencil s;
    face_eval(sa.pts, sa.vel, sa.adv, i0, i1, i2, d.inv_dx, a, fn, s);
    const bool ok = q < fb.cnt && n < 27 && splat_ok(d.G, s);  // mpm_solver.py:858
    const int lx = s.bx - bt.ox, ly = s.by - bt.oy, lz = s.bz - bt.oz;
    const float w = stencil_w(s, ni, nj, nk);
    if (ok && in_margin(lx, ly, lz)) {
      double *p = tile + tile_idx(lx + ni, ly + nj, lz + nk);
      if (PASSES == 1) {
        atomicAdd(p, (double)w);
        atomicAdd(p + TILE_PAD, (double)(w * a.x)); atomicAdd(p + 2 * TILE_PAD, (double)(w * a.y)); atomicAdd(p + 3 * TILE_PAD, (double)(w * a.z));
      } else {
        atomicAdd(p, (double)(w * fn.x)); atomicAdd(p + TILE_PAD, (double)(w * fn.y)); atomicAdd(p + 2 * TILE_PAD, (double)(w * fn.z));
      }
    } else if (ok) {  // drifted out of the tile margin since the faces were binned: this lane's node through global atomics
      raise_drift(g.counters, g.step_id);
      raise_face(g.counters, g.step_id);
      col_add_global<PASSES>(g, d, s.bx + ni, s.by + nj, s.bz + nk, w, a, fn);
    }
  }
  __syncthreads();
  col_splat_flush<PASSES, SplatTile4>(tile, bt, act_mask, d, g);
}

// ---- large bins: lane = face.  Faces are sorted by (block, cell of the centroid) at the face sort, so neighbouring lanes mostly hold faces
// of the same cell and add into the same 27 tile nodes: the same segmented DPP pre-reduction as the particle scatter (p2g_scatter)
// leaves one lane per run issuing the LDS atomics.  DBG 4096 switches the pre-reduction off (every lane issues).
// Two passes through the four-channel tile per batch of faces -- (weight, weight * velocity), then weight * normal -- with the face, its
// stencil and the scan masks loaded / computed once for both.
template <int PASS>
__device__ __forceinline__ void col_splat_scatter(double *tile, const Stencil &s, float on, V3 c, SegMask sm, bool do_add, int base) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float wx = sel3(i, s.w0.x, s.w1.x, s.w2.x) * on;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      float wxy = wx * sel3(j, s.w0.y, s.w1.y, s.w2.y);
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        float w = wxy * sel3(k, s.w0.z, s.w1.z, s.w2.z);
        float r0 = w * c.x, r1 = w * c.y, r2 = w * c.z, r3 = w;
        seg_scan4<3>(r0, r1, r2, r3, sm);
        if (do_add) {
          double *p = tile + base + tile_idx(i, j, k);
          if (PASS == 0) {
            atomicAdd(p, (double)r3);
            atomicAdd(p + TILE_PAD, (double)r0); atomicAdd(p + 2 * TILE_PAD, (double)r1); atomicAdd(p + 3 * TILE_PAD, (double)r2);
          } else {
            atomicAdd(p, (double)r0); atomicAdd(p + TILE_PAD, (double)r1); atomicAdd(p + 2 * TILE_PAD, (double)r2);
          }
        }
      }
    }
  }
}
template <int PASSES>
__device__ __forceinline__ void col_splat_large(double *tile, const SplatArgs &sa, const FaceBin &fb, const BinTile &bt, bool nb_act,
                                                const Dims &d, const GridPtrs &g) {
  const unsigned long long act_mask = __ballot(nb_act);
  const int l = threadIdx.x, end = fb.start + fb.cnt;
  for (int j0 = fb.start; j0 < end; j0 += PT) {  // workgroup-uniform trip count: barriers and DPP need converged lanes
    for (int t = l; t < 4 * TILE_PAD; t += PT) tile[t] = 0.0;
    int jj = j0 + l;
    bool have = jj < end;
    int i0, i1, i2;
    load_face(sa.fidx, have ? jj : fb.start, i0, i1, i2);
    V3 a, fn;
    Stencil s;
    face_eval(sa.pts, sa.vel, sa.adv, i0, i1, i2, d.inv_dx, a, fn, s);
    bool ok = have && splat_ok(d.G, s);  // mpm_solver.py:858
    int lx = s.bx - bt.ox, ly = s.by - bt.oy, lz = s.bz - bt.oz;
    bool tile_ok = ok && in_margin(lx, ly, lz);
    // lanes without a face in the tile carry a unique key (never merged, never issue) and a zero contribution
    int key = tile_ok ? (lx * TILE + ly) * TILE + lz : -2 - (l & 63);
    int base = tile_ok ? tile_idx(lx, ly, lz) : 0;
    float on = tile_ok ? 1.0f : 0.0f;
    bool any = __any(tile_ok);
    SegMask sm = seg_masks(key);
    unsigned long long tails = __ballot(sm.tail);
    int dist = __ffsll((unsigned long long)(tails >> (l & 63))) - 1;
    bool do_add = tile_ok && (dist & 7) == 0;
    if (DBG(g, 4096)) { sm.m1 = sm.m2 = sm.m4 = sm.m8 = 0.0f; do_add = tile_ok; }
    __syncthreads();
    if (any && (PASSES & 1)) col_splat_scatter<0>(tile, s, on, a, sm, do_add, base);
    if (ok && !tile_ok) {  // drifted out of the tile margin since the faces were binned
      raise_drift(g.counters, g.step_id);
      raise_face(g.counters, g.step_id);  // ... which is what makes the next re-sort bin the faces again (rebin)
#pragma unroll 1
      for (int n = 0; n < 27; ++n) {
        int i = n / 9, j = (n / 3) % 3, k = n % 3;
        col_add_global<PASSES>(g, d, s.bx + i, s.by + j, s.bz + k, stencil_w(s, i, j, k), a, fn);
      }
    }
    if (PASSES & 1) {
      __syncthreads();
      col_splat_flush<1, SplatTile4>(tile, bt, act_mask, d, g);
    }
    if (PASSES == 3) {
      __syncthreads();
      for (int t = l; t < 3 * TILE_PAD; t += PT) tile[t] = 0.0;
    }
    if (PASSES & 2) {
      __syncthreads();
      if (any) col_splat_scatter<1>(tile, s, on, fn, sm, do_add, base);
      __syncthreads();
      col_splat_flush<2, SplatTile4>(tile, bt, act_mask, d, g);
    }
    __syncthreads();
  }
}

// One bin.  In cloth scenes the two passes ride in DIFFERENT launches -- pass 0 in front of the stress kernel, pass 1 in the p2g launch --
// because a two-pass splat workgroup lives 10-17 us and set the length of the p2g launch in scenes that fit one round of workgroups
// (garment-120k: p2g 18 us for 10 us chunk workgroups), while the stress launch before it has room (9 us of streaming work, no LDS, one
// round).  Nothing reads the collider channels before g2p; the buffer they go into was cleared by the p2g launch of the substep before.
template <int PASSES>
__device__ __forceinline__ void col_splat_wg(double *tile, const SplatArgs &sa, int bin, const Dims &d, const GridPtrs &g) {
  const FaceBin fb = sa.fbins[bin];
  BinTile bt;
  bt.bz = fb.blk % d.NB; bt.by = (fb.blk / d.NB) % d.NB; bt.bx = fb.blk / (d.NB * d.NB);
  bt.ox = 4 * bt.bx - 1; bt.oy = 4 * bt.by - 1; bt.oz = 4 * bt.bz - 1;
  // active flags of the 27 blocks the tile overlaps (lane n < 27 of every wavefront -> neighbour n); the forms ballot them
  bool nb_act = false;
  if ((threadIdx.x & 63) < 27) {
    int n = threadIdx.x & 63;
    int x = bt.bx + n / 9 - 1, y = bt.by + (n / 3) % 3 - 1, z = bt.bz + n % 3 - 1;
    if ((unsigned)x < (unsigned)d.NB && (unsigned)y < (unsigned)d.NB && (unsigned)z < (unsigned)d.NB)
      nb_act = g.ab_flag[(x * d.NB + y) * d.NB + z] != 0;
  }
  if (fb.cnt > SPLAT_SMALL) col_splat_large<PASSES>(tile, sa, fb, bt, nb_act, d, g);
  else if constexpr (PASSES == 3) col_splat_small_onepass(tile, sa, fb, bt, nb_act, d, g);
  else col_splat_small<PASSES>(tile, sa, fb, bt, nb_act, d, g);
}

}  // namespace fk
}  // namespace mpm
