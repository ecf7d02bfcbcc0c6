/*
 * mpmhip.h -- C ABI of libmpmhip.so, the MI355X (gfx950) MPM substep solver.
 *
 * Drop-in boundary for the hot path of KAISTChangmin/MPMAvatar: one MPM substep,
 * `MPMWARP.p2g2p` (/root/reference/warp_mpm/mpm_solver.py:229-536) and the solver
 * state it advances.  The reference has no FFI for this path (it is NVIDIA-Warp DSL
 * called from Python); the entry points below are what a ctypes
 * binding of `warp_mpm/mpm_solver.py` + `mpm_data_structure.py` needs, one group per
 * reference interface.  The Python shim `mpmavatar_amd/warp_mpm/` is that binding.
 *
 * Conventions
 *   - every pointer marked [dev] is a device pointer on `config.device` (e.g.
 *     torch.Tensor.data_ptr() of a ROCm tensor); [host] pointers are read during the
 *     call and not retained.  No torch types cross this boundary.
 *   - particle arrays use the reference's layout: AoS fp32, vec3 = 3 floats,
 *     mat33 = 9 floats row-major; index classes [0,n_elements) elements,
 *     [n_elements,n_nv) traditional, [n_nv,n_particles) vertices,
 *     n_nv = n_particles - n_vertices (mpm_solver.py:19-26, SURVEY.md 8 layout).
 *   - calls are asynchronous on the context's stream unless stated; every function
 *     returns MPMHIP_OK (0) or a negative error code, mpmhip_last_error() has the text.
 *   - a context is bound to one GPU and is not thread-safe; distinct contexts are
 *     independent (one per rank in multi-GPU runs).
 */
#ifndef MPMHIP_H
#define MPMHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPMHIP_VERSION 100

enum {
  MPMHIP_OK = 0,
  MPMHIP_ERR_INVALID = -1,   /* bad argument / inconsistent sizes  (reference: assert / RuntimeError) */
  MPMHIP_ERR_NO_DEVICE = -2, /* no HIP device visible: the solver never falls back to a CPU path */
  MPMHIP_ERR_HIP = -3,       /* a HIP runtime call failed */
  MPMHIP_ERR_STATE = -4,     /* called before the state/model were bound */
  MPMHIP_ERR_LIMIT = -5      /* too many colliders / boundary conditions */
};

enum { MPMHIP_MODE_FAST = 0,      /* cell-sorted SoA particles + block-sparse grid + LDS-tiled transfers */
       MPMHIP_MODE_BASELINE = 1   /* reference-structured kernels on the caller's AoS arrays, dense grid */ };

typedef struct mpmhip_ctx mpmhip_ctx;

/* MPMWARP.__init__/initialize arguments, mpm_solver.py:14-26 */
typedef struct {
  int32_t n_particles, n_elements, n_vertices;
  int32_t n_grid;
  float grid_lim;
  int32_t num_joint_t, num_joint_v, num_joint_f;
  int32_t device;         /* HIP device ordinal */
  int32_t mode;           /* MPMHIP_MODE_* */
  int32_t rebin_interval; /* fast mode: max substeps between particle re-sorts (a device-side drift flag triggers
                             earlier ones); 0 = default (256); < 0 = exactly every -n substeps, drift flag ignored */
  int32_t own_stream;     /* 1: create a private non-blocking stream and ignore `stream` */
  void *stream;           /* own_stream == 0: hipStream_t to launch on (NULL = the HIP null stream), e.g.
                             torch.cuda.current_stream().cuda_stream so that solver work is ordered with the
                             caller's tensor ops the way Warp's stream is with torch's */
  int32_t p2g_tile;       /* fast mode, the one setting that changes NUMERICS: accumulator of p2g's chunk tile.
                             MPMHIP_P2G_TILE_AUTO (0): packed fixed point, or fp64 when the particle masses of the scene span more
                             than 1e5 (decided at every import of the state); MPMHIP_P2G_TILE_FIXED (1); MPMHIP_P2G_TILE_F64 (2).
                             (The environment variable MPMHIP_P2G_TILE=fx|f64 overrides it for experiments.) */
  int32_t reserved_;      /* must be 0 */
} mpmhip_config;
#define MPMHIP_P2G_TILE_AUTO 0
#define MPMHIP_P2G_TILE_FIXED 1
#define MPMHIP_P2G_TILE_F64 2

/* MPMStateStruct fields the substep touches, mpm_data_structure.py:13-49.  All [dev]. */
typedef struct {
  float *particle_x;        /* [n_particles*3] */
  float *particle_v;        /* [n_particles*3] */
  float *particle_C;        /* [n_particles*9] */
  float *particle_F;        /* [n_nv*9] */
  float *particle_F_trial;  /* [n_nv*9] */
  float *particle_stress;   /* [n_nv*9] */
  float *particle_d;        /* [n_elements*9] */
  float *particle_R_inv;    /* [n_elements*3] */
  const float *faces;       /* [n_elements*3] float-encoded vertex ids (quirk Q8) */
  float *vertex_force;      /* [n_vertices*3] */
  const float *particle_vol;  /* [n_particles] */
  const float *particle_mass; /* [n_particles] */
  const int32_t *particle_selection; /* [n_particles], 0 = simulate, anything else = not simulated (mpm_utils.py:492); the
                                        value 2 marks a ghost copy, but only after mpmhip_dist_enable */
} mpmhip_state_ptrs;

/* MPMModelStruct arrays, mpm_data_structure.py:621-630.  All [dev], [n_particles]. */
typedef struct {
  float *mu, *lam, *gamma, *kappa, *yield_stress;
} mpmhip_model_ptrs;

/* MPMModelStruct scalars, mpm_data_structure.py:627-645 + init_other_params :686-715 */
typedef struct {
  int32_t material; /* 0 jelly 1 metal 2 sand 3 foam 4 snow 5 plasticine 6 neo-hookean 7 cloth */
  float friction_coeff, alpha;
  float g[3];
  float hardening, xi, plastic_viscosity, softening;
  float rpic_damping, grid_v_damping_scale;
} mpmhip_model_scalars;

typedef struct {
  int64_t substeps;        /* p2g2p calls since creation */
  int64_t rebins;          /* particle re-sorts (fast mode) */
  int32_t n_active_blocks; /* 4x4x4-node grid blocks currently swept (fast mode) */
  int32_t n_active_nodes;  /* nodes with mass > 0 after the last p2g (filled by mpmhip_measure) */
  int32_t n_collider_nodes;
  int32_t n_mover_nodes;
  int32_t n_fallback_particles; /* particles that left their tile margin since the last re-sort */
  int32_t n_dropped;            /* fast mode: scatter contributions that fell outside the active blocks (cumulative).
                                   Must stay 0: non-zero means particles outran the re-sorts (fixed-interval mode
                                   with an interval too long for their speed) and the results are not valid */
  int64_t g2p2g_launches;       /* fast mode, scenes of traditional particles only: substep boundaries that ran as ONE launch
                                   (g2p of substep n + stress and p2g of substep n + 1, csrc/g2p.hip k_g2p2g) */
  int32_t p2g_tile_in_use;      /* fast mode: the accumulator p2g's chunk tile runs on NOW -- MPMHIP_P2G_TILE_FIXED or MPMHIP_P2G_TILE_F64
                                   (what MPMHIP_P2G_TILE_AUTO resolved to at the last import; 0 in baseline mode) */
  int32_t kept_collider_substeps; /* fast mode: substeps of mpmhip_steps calls whose body was at rest (mesh_v == 0 for every vertex) that
                                     ran WITHOUT body-face splat workgroups: the collider field is splatted once per accumulator buffer
                                     and kept until the particle order changes or the call ends (csrc/fast.hip fast_body_at_rest_begin) */
} mpmhip_stats;

/* ---- lifetime ----------------------------------------------------------------- */
int mpmhip_version(void);
int mpmhip_device_count(void); /* 0 when no GPU is visible (never an error) */
/* MPMWARP(...) constructor, mpm_solver.py:14-51 */
int mpmhip_create(const mpmhip_config *cfg, mpmhip_ctx **out);
void mpmhip_destroy(mpmhip_ctx *ctx);
/* text of the last error on ctx (ctx may be NULL for mpmhip_create failures) */
const char *mpmhip_last_error(const mpmhip_ctx *ctx);

/* ---- state / model binding ------------------------------------------------------ */
/* MPMStateStruct.from_torch / reset_state / continue_from_torch rebind arrays
 * (mpm_data_structure.py:158-419): call again whenever any pointer changes.  The caller's
 * arrays are taken as the authoritative state at the next step. */
int mpmhip_bind_state(mpmhip_ctx *ctx, const mpmhip_state_ptrs *p);
/* MPMModelStruct.init + set_E_nu + prepare_mu_lam results, mpm_solver.py:128-227 */
int mpmhip_bind_model(mpmhip_ctx *ctx, const mpmhip_model_ptrs *p);
/* MPMWARP.set_parameters_dict scalars, mpm_solver.py:57-126 */
int mpmhip_set_model_scalars(mpmhip_ctx *ctx, const mpmhip_model_scalars *s);
/* The caller changed bound arrays in place (particle or model): re-import before the next step. */
int mpmhip_push_state(mpmhip_ctx *ctx);
/* Make the caller's particle_x/v/C/F/F_trial/stress/d/vertex_force current (the equivalent of the
 * zero-copy wp.to_torch(mpm_state.particle_x) read, run_demo.py:532).  No-op in baseline mode. */
int mpmhip_pull_state(mpmhip_ctx *ctx);

/* ---- body mesh, colliders, boundary conditions ----------------------------------- */
/* wp.Mesh(points, velocities=0, indices), mpm_solver.py:45-51.  verts/faces are [host]. */
int mpmhip_set_body_mesh(mpmhip_ctx *ctx, int32_t n_verts, int32_t n_faces, const float *verts,
                         const int32_t *faces);
/* MPMWARP.add_mesh_collider, mpm_solver.py:805-919 */
int mpmhip_add_mesh_collider(mpmhip_ctx *ctx, float friction);
/* MPMWARP.add_particle_mover, mpm_solver.py:661-802 */
int mpmhip_add_particle_mover(mpmhip_ctx *ctx);
/* MPMWARP.add_surface_collider, mpm_solver.py:564-658; normal already normalised,
 * surface_type 0 sticky / 1 slip / 11 cut / 2 other */
int mpmhip_add_surface_collider(mpmhip_ctx *ctx, const float point[3], const float normal[3],
                                int32_t surface_type, float friction, float start_time, float end_time);
/* MPMWARP.set_velocity_on_cuboid, mpm_solver.py:929-984 (the host-side `modify` is applied inside step) */
int mpmhip_add_velocity_cuboid(mpmhip_ctx *ctx, const float point[3], const float size[3],
                               const float velocity[3], float start_time, float end_time, int32_t reset);
/* MPMWARP.add_bounding_box, mpm_solver.py:986-1053 */
int mpmhip_add_bounding_box(mpmhip_ctx *ctx, float start_time, float end_time);
/* MPMWARP.enforce_grid_velocity_by_mask, mpm_solver.py:1330-1355; mask [dev] int32 [n_grid^3] */
int mpmhip_add_grid_mask(mpmhip_ctx *ctx, const int32_t *mask);

/* ---- pre-p2g particle operations (mpm_solver.py:1058-1417) ------------------------ */
/* selection kernels, mpm_utils.py:1198-1248: write 0/1 into mask [dev] int32 [n_particles] */
int mpmhip_select_box(mpmhip_ctx *ctx, const float point[3], const float size[3], int32_t *mask);
int mpmhip_select_cylinder(mpmhip_ctx *ctx, const float point[3], const float normal[3],
                           float half_height, float radius, int32_t *mask);
/* add_impulse_on_particles (per_mass=1: v += force/mass*dt where mask==1, :1093-1104) and
 * add_impulse_on_particles_with_mask (per_mass=0: v += force*dt where mask>=1, :1399-1415) */
int mpmhip_add_impulse(mpmhip_ctx *ctx, const float force[3], const int32_t *mask, int32_t per_mass,
                       float start_time, float end_time);
/* enforce_particle_velocity_translation / _by_mask, :1138-1149, :1315-1326 */
int mpmhip_add_velocity_set(mpmhip_ctx *ctx, const float velocity[3], const int32_t *mask,
                            float start_time, float end_time);
/* enforce_particle_velocity_rotation, :1156-1257 */
int mpmhip_add_velocity_rotation(mpmhip_ctx *ctx, const float point[3], const float normal[3],
                                 const float axis1[3], const float axis2[3], float rotation_scale,
                                 float translation_scale, const int32_t *mask, float start_time,
                                 float end_time);

/* ---- the substep --------------------------------------------------------------------- */
/* MPMWARP.p2g2p, mpm_solver.py:229-536.  mesh_x, mesh_v [dev][num_mesh_v*3]; joint_traditional_v
 * [dev][n_joint_t*3]; joint_verts_v [dev][num_joint_v*3]; joint_faces_v [dev][num_joint_f*3];
 * NULL = the Python argument None. */
int mpmhip_step(mpmhip_ctx *ctx, float dt, const float *mesh_x, const float *mesh_v,
                const float *joint_traditional_v, int32_t n_joint_t, const float *joint_verts_v,
                const float *joint_faces_v);
/* n substeps with the caller's per-substep mesh advection mesh_x + k*dt*mesh_v fused on the device
 * (the loop at train_material_params.py:622-626 / run_demo.py:526-530) */
int mpmhip_steps(mpmhip_ctx *ctx, float dt, int32_t n, const float *mesh_x, const float *mesh_v,
                 const float *joint_traditional_v, int32_t n_joint_t, const float *joint_verts_v,
                 const float *joint_faces_v);
int mpmhip_synchronize(mpmhip_ctx *ctx);
/* MPMWARP.time (never reset by reset_state, quirk Q3) */
double mpmhip_get_time(const mpmhip_ctx *ctx);
int mpmhip_set_time(mpmhip_ctx *ctx, double t);
/* mpm_solver.py:536: `self.time = self.time + dt` adds the caller's Python float (a double) while the kernels receive dt as
 * fp32.  Tell the library that double once (and whenever dt changes); steps whose fp32 dt equals (float)dt_host then advance
 * MPMWARP.time by dt_host exactly as the reference does.  Without it time advances by (double)(float)dt. */
int mpmhip_set_host_dt(mpmhip_ctx *ctx, double dt_host);

/* ---- multi-GPU (one process and one context per GPU; not in the reference) --------------------
 * Particles are sharded across ranks by the caller (mpmavatar_amd/dist.py: spatial x-slabs, re-cut at the particles' current positions when more than a
 * tenth of them have left their slab); every rank runs
 * its own context on its particles plus ghost copies (particle_selection == 2: stress yes, transfers no).  The
 * substep is split in three so that the caller can run its two neighbour exchanges (RCCL send/recv through
 * torch.distributed) between the phases:
 *   begin: [stress, p2g] + pack halo_send      -> exchange halo   (sum of the grid blocks both ranks touch)
 *   mid  : add halo_recv, [grid, g2p] + pack ghost_send -> exchange ghosts (x, v of vertices; d3 of elements)
 *   end  : unpack ghost_recv, [element finalise]
 * All ranks must re-sort at the same substep: mpmhip_dist_rebin() replaces the context's own re-sort policy.
 * With mpmhip_dist_set_ghost_mode(ctx, 1) the ghost copies gather for themselves (g2p yes, p2g no): their grid
 * neighbourhood is on both ranks' active lists and therefore complete after the halo sum, so the per-substep ghost
 * exchange disappears (mid / end no longer pack / unpack); owners and copies differ only by the rounding order of the
 * halo sums, and mpmhip_dist_ghost_pack / _unpack re-synchronise them around an exchange at each collective re-sort. */
typedef struct {
  int32_t n_blocks;          /* grid blocks on both ranks' active lists */
  const int32_t *blocks;     /* [dev] their ids in ascending order (identical on both ranks) */
  float *halo_send, *halo_recv; /* [dev] n_blocks * CH * 64 floats; CH = 8 when a particle mover exists, else 4 */
  int32_t n_send_p, n_recv_p, n_send_e, n_recv_e;
  const int32_t *send_p, *recv_p; /* [dev] caller-order indices of vertices/traditional particles sent / received */
  const int32_t *send_e, *recv_e; /* [dev] caller-order indices of elements whose d3 is sent / received */
  float *ghost_send, *ghost_recv; /* [dev] 6*n_p + 3*n_e floats */
} mpmhip_dist_peer;
int mpmhip_dist_enable(mpmhip_ctx *ctx);
/* 0 (default): ghost copies are overwritten by their owners' values every substep; 1: they gather for themselves.
 * Call before the first mpmhip_dist_rebin. */
int mpmhip_dist_set_ghost_mode(mpmhip_ctx *ctx, int32_t ghosts_gather);
int mpmhip_dist_ghost_pack(mpmhip_ctx *ctx);   /* fill every peer's ghost_send */
int mpmhip_dist_ghost_unpack(mpmhip_ctx *ctx); /* apply every peer's ghost_recv */
int mpmhip_dist_num_blocks(const mpmhip_ctx *ctx); /* size of the active-block byte map */
/* MPMHIP_P2G_TILE_AUTO in a sharded run: the smallest positive and the largest mass over the simulated particles of ALL ranks (the
 * caller all-reduces them).  The tile decision of every later import is taken from max(this rank's span, max_mass / min_mass), so
 * every rank switches to the fp64 tile together -- ranks that share halo blocks must not run different accumulator numerics -- and
 * from the masses actually bound (reset_density(update_mass) after the build included), never from a description of the scene.
 * AUTO is only ever widened to fp64 this way, never forced to the fixed-point tile.  min_mass <= 0: forget the global span. */
int mpmhip_dist_set_mass_span(mpmhip_ctx *ctx, float min_mass, float max_mass);
/* this rank's early-warning drift flag (1: some particle is about to leave the tile margin of the block it was sorted
 * into; cleared by the next re-sort).  Synchronous.  A sharded driver max-reduces it over the ranks to decide on a
 * collective re-sort -- the single-GPU adaptive policy (mpmhip_config.rebin_interval = 0) made collective. */
int mpmhip_dist_drift_flag(mpmhip_ctx *ctx, int32_t *flag);
/* import the bound state if needed, re-sort, and write this rank's active-block map (1 byte per block) [dev] */
int mpmhip_dist_rebin(mpmhip_ctx *ctx, uint8_t *active_map);
int mpmhip_dist_set_peers(mpmhip_ctx *ctx, int32_t n_peers, const mpmhip_dist_peer *peers);
int mpmhip_dist_step_begin(mpmhip_ctx *ctx, float dt, const float *mesh_x, const float *mesh_v, float mesh_advect,
                           const float *joint_traditional_v, int32_t n_joint_t, const float *joint_verts_v,
                           const float *joint_faces_v);
int mpmhip_dist_step_mid(mpmhip_ctx *ctx);
int mpmhip_dist_step_end(mpmhip_ctx *ctx);

/* RCCL transport inside the library (no Python in the substep loop): the communicator is created from a
 * ncclUniqueId that rank 0 obtains with mpmhip_rccl_unique_id() and the caller broadcasts (torch.distributed).
 * librccl.so.1 is dlopen'ed on first use (the copy torch has already loaded, if any). */
int mpmhip_rccl_unique_id(char id[128]);
int mpmhip_rccl_init(mpmhip_ctx *ctx, int32_t rank, int32_t world, const char id[128]);
/* static ghost lists per peer rank ([host] int arrays of caller-order particle indices, see mpmhip_dist_peer) */
int mpmhip_rccl_set_ghosts(mpmhip_ctx *ctx, int32_t n_peers, const int32_t *peer_ranks, const int32_t *n_send_p,
                           const int32_t *const *send_p, const int32_t *n_recv_p, const int32_t *const *recv_p,
                           const int32_t *n_send_e, const int32_t *const *send_e, const int32_t *n_recv_e,
                           const int32_t *const *recv_e);
/* n substeps (collective): re-sort + shared-block lists every rebin_interval substeps (counted from step_index) if
 * rebin_interval > 0; if <= 0, when the max-reduced drift flag of the ranks (ncclAllReduce of one int every 16
 * substeps, read 4 substeps later so that all ranks act at the same substep) asks for it, at the latest every 256
 * (or -rebin_interval) substeps.  Halo (and, in ghost mode 0, ghost) exchanges with ncclSend/ncclRecv groups on the context's stream; in ghost mode 1
 * the ghosts are re-synchronised before every re-sort instead.  Mesh advection factor of substep k is
 * (step_index + k) * dt.  joint_traditional_v: velocities of the LAST n_joint_t traditional particles this rank owns (the
 * staged release of run_demo.py:524; a rank's share of the held particles is a suffix of its owned ones), or NULL */
/* bytes this rank sends per substep in the halo exchange with the current shared-block lists (measurement) */
int mpmhip_dist_halo_bytes(mpmhip_ctx *ctx, int64_t *out);
/* how mpmhip_rccl_steps moves the halos: 1 = peer-mapped buffers (each pair of neighbouring ranks maps the other's
 * fine-grained receive arena with HIP IPC at the first collective re-sort; the pack kernel stores into it and raises a flag
 * there, the add kernel waits for its own flag -- no RCCL kernel in the substep), 0 = ncclSend/ncclRecv groups.  Peer
 * mapping is the default and is used only if a four-round handshake over every link of every rank succeeded (max-reduced);
 * MPMHIP_DIST_HALO=rccl keeps send/recv.  No counterpart in the reference (single GPU). */
int mpmhip_dist_halo_transport(mpmhip_ctx *ctx, int32_t *out);
/* substeps of mpmhip_rccl_steps so far that had NO halo kernels: with peer-mapped halos the pack rides in the p2g launch as
 * trailing workgroups (they wait until every scattering workgroup of that launch has counted itself done) and g2p adds the
 * neighbour's share to the shared blocks while it stages its tile.  Falls back to the pack / add kernels for an interval in
 * which a block is shared with more than one neighbour, a pair's arena is too small, or profiling brackets the launches;
 * MPMHIP_DIST_FUSED_HALO=0 switches it off. */
int mpmhip_dist_fused_halo_steps(mpmhip_ctx *ctx, int64_t *out);
int mpmhip_rccl_steps(mpmhip_ctx *ctx, float dt, int32_t n, int64_t step_index, int32_t rebin_interval,
                      const float *mesh_x, const float *mesh_v, const float *joint_traditional_v, int32_t n_joint_t,
                      const float *joint_verts_v, const float *joint_faces_v);

/* ---- after the solver: per-face frames and bound Gaussians --------------------------------
 * Stand-alone maps on [dev] arrays (no solver context; `stream` is a hipStream_t, NULL = default stream).
 * mpmhip_face_frames = MeshGaussianModel.set_mesh_by_verts (scene/mesh_gaussian_model.py:137-146) with
 * compute_face_orientation(return_scale=True) (utils/graphics_utils.py:88-106):
 *   face_center [n_f*3] = mean of the three vertices, face_orien_mat [n_f*9] row-major with columns a0 a1 a2,
 *   face_orien_quat [n_f*4] WXYZ = quat_xyzw_to_wxyz(rotmat_to_unitquat(mat)) (roma), face_scaling [n_f]. */
int mpmhip_face_frames(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces,
                       float *face_center, float *face_orien_mat, float *face_orien_quat, float *face_scaling);
/* GaussianModel.get_xyz / get_rotation / get_scaling with a face binding (scene/gaussian_model.py:112-151):
 *   xyz [n_g*3] = mat[b] xyz_local * scaling[b] + center[b];  rotation [n_g*4] WXYZ = normalize(quat[b]) (x)
 *   normalize(rotation_raw);  scaling [n_g*3] = exp(scaling_raw) * face_scaling[b].  Any output may be NULL. */
int mpmhip_bind_gaussians(int32_t device, void *stream, int32_t n_gaussians, const int32_t *binding, const float *xyz_local,
                          const float *rotation_raw, const float *scaling_raw, const float *face_center,
                          const float *face_orien_mat, const float *face_orien_quat, const float *face_scaling, float *xyz,
                          float *rotation, float *scaling);

/* The rasteriser's inputs, SURVEY.md 8(f) N4: what gaussian_renderer/__init__.py:52-103 hands to GaussianRasterizer for a mesh-bound
 * model plus the caller's `extra` primitives (run_demo.py:578-604: sand and chair), assembled in one launch into buffers of
 * n_gaussians + n_extra rows: means3D [*3] = get_xyz (scene/gaussian_model.py:141-151) | extra_xyz; means2D [*3] = 0 (:27);
 * opacities [*1] = sigmoid(opacity_raw) (:158-160) | extra_opacity; scales [*3] = get_scaling (:112-122) | extra_scales;
 * rotations [*4] WXYZ = get_rotation (:124-138) | extra_rotations -- the five torch.cat of :84-91.  Colours (shs or
 * colors_precomp) are the caller's tensors unchanged.  With frames taken from the solver's particle_x on the device this replaces
 * the per-frame OBJ write / re-read of train_material_params.py:819-845 for everything but the Blender AO bake. */
int mpmhip_render_inputs(int32_t device, void *stream, int32_t n_gaussians, int32_t n_extra, const int32_t *binding,
                         const float *xyz_local, const float *rotation_raw, const float *scaling_raw, const float *opacity_raw,
                         const float *face_center, const float *face_orien_mat, const float *face_orien_quat,
                         const float *face_scaling, const float *extra_xyz, const float *extra_opacity, const float *extra_scales,
                         const float *extra_rotations, float *means3D, float *means2D, float *opacities, float *scales,
                         float *rotations);

/* ---- gradients through the two steps above (the appearance loop, train_appearance.py: parameters and vertices -> frames ->
 * binding -> rasteriser -> loss -> backward) --------------------------------------------------------------------------------------
 * The exact derivative of the forward kernels' expressions with every discrete decision held fixed: the quaternion branch, the
 * sign inside |a2 . e2| (sign(0) = 0), and the clamps of length() (1e-20) and normalize (1e-12), which pass zero slope where they
 * bind.  fp32, no atomics: the two reductions walk a CSR segment in ascending index, so two runs give the same bits.
 *
 * mpmhip_render_inputs_backward: g_means3D / g_opacities / g_scales / g_rotations are the upstream gradients of the first
 * n_gaussians rows of mpmhip_render_inputs' outputs (or of mpmhip_bind_gaussians' xyz / scaling / rotation); a NULL one counts
 * as zero and the raw inputs only it needs may then be NULL too.  d_xyz [n_g*3], d_rotation [n_g*4], d_scaling [n_g*3],
 * d_opacity [n_g]: written in full, NULL = not wanted.  d_face_center [n_f*3], d_face_orien_mat [n_f*9], d_face_orien_quat
 * [n_f*4], d_face_scaling [n_f]: all four or none; they need the face -> Gaussian table face_start [n_f+1] (ascending, face_start[0]
 * = 0, face_start[n_f] = n_g) and face_items [n_g] (the Gaussians of face f, ascending, at face_start[f] .. face_start[f+1]); a face
 * without Gaussians gets zeros.  The rows of `extra` primitives need no kernel: their gradients are the upstream rows. */
int mpmhip_render_inputs_backward(int32_t device, void *stream, int32_t n_gaussians, int32_t n_faces, const int32_t *binding,
                                  const float *xyz_local, const float *rotation_raw, const float *scaling_raw, const float *opacity_raw,
                                  const float *face_orien_mat, const float *face_orien_quat, const float *face_scaling,
                                  const float *g_means3D, const float *g_opacities, const float *g_scales, const float *g_rotations,
                                  float *d_xyz, float *d_rotation, float *d_scaling, float *d_opacity, const int32_t *face_start,
                                  const int32_t *face_items, float *d_face_center, float *d_face_orien_mat, float *d_face_orien_quat,
                                  float *d_face_scaling);
/* mpmhip_face_frames_backward: from the upstream gradients of mpmhip_face_frames' four outputs (a NULL one counts as zero) to
 * d_verts [n_v*3].  face_orien_mat / face_orien_quat are the forward's own outputs (the quaternion branch is chosen from those
 * floats); d_corners [n_f*9] is scratch (the gradient of each face's three corners); vert_start [n_v+1] / vert_corners [3*n_f] is
 * the vertex -> corner table (corner = 3 * face + position, ascending within a vertex); a vertex in no face gets exactly 0. */
int mpmhip_face_frames_backward(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, int32_t n_verts,
                                const float *face_orien_mat, const float *face_orien_quat, const float *g_face_center,
                                const float *g_face_orien_mat, const float *g_face_orien_quat, const float *g_face_scaling,
                                const int32_t *vert_start, const int32_t *vert_corners, float *d_corners, float *d_verts);

/* ---- the colours handed to the render call (train_appearance.py:120-123 and convert_SH, :31-47) ---------------------------------
 *   out_colors [n*3] = shadow[binding[i]] * clamp_min(eval_sh(sh_degree, features[i], normalize(means3D[i] - campos)) + 0.5, 0)
 *   shadow[f] = grid_sample(shadow_map [map_h*map_w], face_uv[f], bilinear, align_corners = False, zeros padding)
 * features_dc [n*1*3] and features_rest [n*(n_sh_coeffs-1)*3] are GaussianModel's two tensors, read through two pointers (no cat);
 * only the (sh_degree+1)^2 coefficients in use are read.  campos [3] and face_uv [n_faces*2] (in [-1, 1], v flipped,
 * scene/mesh_gaussian_model.py:109-111) are device arrays.  shadow_map == NULL: shadow = 1, plain convert_SH; face_uv and binding
 * may then be NULL.  features_dc == NULL: the colour before the shadow is (1, 1, 1), the shadow.repeat(1, 3) renders of
 * train_appearance.py:215-226.  Both NULL is invalid.  A binding entry outside [0, n_faces) gives NaN and reads nothing.
 * MPMHIP_ERR_INVALID, nothing launched: a negative count, sh_degree outside 0..3, n_sh_coeffs < (sh_degree+1)^2, a map size <= 0
 * with a map, a required pointer NULL.  n == 0: MPMHIP_OK, no launch. */
int mpmhip_shade_colors(int32_t device, void *stream, int32_t n, int32_t n_faces, const int32_t *binding, const float *means3D,
                        const float *campos, int32_t sh_degree, int32_t n_sh_coeffs, const float *features_dc, const float *features_rest,
                        const float *shadow_map, int32_t map_h, int32_t map_w, const float *face_uv, float *out_colors);
/* mpmhip_shade_colors_backward: from g_colors [n*3] (NULL counts as zero) to d_features_dc, d_features_rest (zero above the active
 * degree), d_means3D [n*3] and d_shadow_map [map_h*map_w]; each is written in full, NULL = not wanted.  The exact derivative with
 * every discrete decision held fixed: the bilinear cell, a tap outside the map, and the SH clamp (zero slope where it binds); face_uv
 * gets no gradient, as in train_appearance.py:120-123, where it is a constant.  fp32, no atomics, the same bits on every run:
 * d_shadow_map walks two tables, needed only for it -- face_start [n_faces+1] / face_items [n] (the Gaussians of a face, ascending)
 * and texel_start [map_h*map_w+1] / texel_items (4 * face + corner of every tap inside the map that lands on the texel, ascending;
 * corner 0..3 = north-west, north-east, south-west, south-east) -- and scratch [n + n_faces] floats.  n == 0 still writes zeros
 * to d_shadow_map. */
int mpmhip_shade_colors_backward(int32_t device, void *stream, int32_t n, int32_t n_faces, const int32_t *binding, const float *means3D,
                                 const float *campos, int32_t sh_degree, int32_t n_sh_coeffs, const float *features_dc,
                                 const float *features_rest, const float *shadow_map, int32_t map_h, int32_t map_w, const float *face_uv,
                                 const float *g_colors, float *d_features_dc, float *d_features_rest, float *d_means3D,
                                 const int32_t *face_start, const int32_t *face_items, const int32_t *texel_start,
                                 const int32_t *texel_items, float *d_shadow_map, float *scratch);

/* ---- the shadow network in front of the colours (scene/shadow.py:14-181, called at train_appearance.py:120 and :201) --------------
 * ShadowUNet over scene/network.py (Conv2dUB :277-329, weight_norm_wrapper :158-266, Conv2dWN / Conv2dWNUB :471-473), for
 * interp_mode = "bilinear" and a constant ao_mean, forward and backward.  With S = shadow_size, U = uv_size,
 * C = n_dims (4 or 8) and level sizes s_i = S >> i:
 *   x = nearest(ao_map [n, in_h, in_w] -> S x S) - ao_mean [S*S]               (F.interpolate(size=), legacy nearest; shadow.py:138-141)
 *   layers 0..3 (encoder i, at s_i): lrelu(conv3x3 + untied bias), the input of i > 0 read bilinearly (align_corners) from s_{i-1}
 *   layers 4..7 (decoder j, at s_{3-j}): the same over [up(decoder j-1), encoder 3-j] (j = 0: encoder 3 alone)
 *   layer 8 (shadow_pred, C -> 1): lowres = sigmoid(conv3x3 + bias + beta); the bias is [1] (Conv2dWN, biases = False) or [S*S]
 *   shadow_map [n, U, U] = bilinear(lowres, align_corners = False); with U == S a bit-exact copy
 * Weights of layer L: weight_v [cout, cin, 3, 3], weight_g [cout], w[o] = v[o] g[o] / ||v||_F with one norm over the whole of v;
 * bias [cout, s, s].  Channels (cin, cout): (1, C), three times (C, C), (C, C), three times (2C, C), (C, 1).
 * Every discrete decision and weight of a resampling is read from `tables`, a DEVICE copy of the blob that
 * mpmhip_shadow_workspace_bytes fills on the host for (in_h, in_w, shadow_size, uv_size); forward and backward share it, the
 * adjoint of a resampling is a gather over its inverse lists, and nothing uses a floating-point atomic: the same input gives the same
 * bits.  d_weight_v / d_weight_g / d_bias are read by mpmhip_shadow_backward alone: written in full where given, NULL = not wanted. */
#define MPMHIP_SHADOW_LAYERS 9
typedef struct {
  int32_t n, in_h, in_w, shadow_size, uv_size, n_dims;
  int32_t untied_head_bias; /* 0: the head's bias is [1] (biases = False); 1: [shadow_size^2] */
  int32_t reserved_;
  float lrelu_slope, beta;
  const float *ao_mean;
  const void *tables;
  const float *weight_v[MPMHIP_SHADOW_LAYERS];
  const float *weight_g[MPMHIP_SHADOW_LAYERS];
  const float *bias[MPMHIP_SHADOW_LAYERS];
  float *d_weight_v[MPMHIP_SHADOW_LAYERS];
  float *d_weight_g[MPMHIP_SHADOW_LAYERS];
  float *d_bias[MPMHIP_SHADOW_LAYERS];
} mpmhip_shadow_desc;
/* The sizes for desc's n, in_h, in_w, shadow_size, uv_size and n_dims (its pointers are not read): the workspace both passes take
 * and the table blob; host_tables != NULL: table_bytes bytes of HOST memory are filled with the blob, for the caller to copy to the
 * device once.  Host arithmetic: the outputs are written whenever the arguments are valid, and the return is then that of the
 * device check.  MPMHIP_ERR_INVALID: n < 0 or > 65535, a size < 1 or > 8192, shadow_size < 8, n_dims not 4 or 8, a NULL output. */
int mpmhip_shadow_workspace_bytes(int32_t device, void *stream, const mpmhip_shadow_desc *desc, int64_t *out_workspace_bytes,
                                  int64_t *out_table_bytes, void *host_tables);
/* shadow.py:135-181.  ao_map [n*in_h*in_w]; out_lowres [n*S*S], out_shadow_map [n*U*U]; out_ao_map [n*S*S], the resized input the
 * reference returns beside them, or NULL.  The workspace keeps the normalised weights and the eight activations for the backward
 * pass; a caller that wants no gradient may reuse it at once.  10 launches, 11 where U != S.  MPMHIP_ERR_INVALID also: a negative
 * or non-finite lrelu_slope, a NULL input, parameter or output, a workspace that is too small.  n == 0: MPMHIP_OK, no launch. */
int mpmhip_shadow_forward(int32_t device, void *stream, const mpmhip_shadow_desc *desc, const float *ao_map, void *workspace,
                          int64_t workspace_bytes, float *out_ao_map, float *out_lowres, float *out_shadow_map);
/* The gradients of every parameter desc names, from g_shadow_map [n*U*U] and g_lowres [n*S*S] (either may be NULL = zero), over the
 * workspace mpmhip_shadow_forward left and the lowres it wrote.  The derivative of LeakyReLU at exactly 0 is the slope, as in torch;
 * an untied bias gradient is the pre-activation gradient itself, summed over n.  12 launches.  ao_map and ao_mean are constants, as
 * in the reference.  Nothing wanted: MPMHIP_OK, no launch. */
int mpmhip_shadow_backward(int32_t device, void *stream, const mpmhip_shadow_desc *desc, const float *ao_map, const float *lowres,
                           const float *g_shadow_map, const float *g_lowres, void *workspace, int64_t workspace_bytes);

/* ---- LPIPS, the third term of the image loss (lpipsPyTorch/modules/{lpips,networks,utils}.py, net_type 'vgg', version 0.1; called at
 * train_appearance.py:133 and :231, eval.py:59) ---------------------------------------------------------------------------------------
 * x, y [n, 3, h, w] -> out [1]: z-score with mean / std, torchvision's vgg16().features[0:30] (thirteen conv3x3 + bias + ReLU with
 * channels 3-64, 64 | 128, 128 | 256 x3 | 512 x3 | 512 x3, MaxPool2d(2, 2) at the bars), at each of the five taps the channel-normalised
 * squared difference weighted by tap_weight [C] and averaged over the pixels, summed over the taps AND over the n images (the
 * reference's sum over the batch it concatenated).  weight [L]: [cout, cin, 3, 3]; bias [L]: [cout]; weight_bwd [L]: cout*cin*9 floats
 * that mpmhip_lpips_prepare_weights fills ([cin, cout, 3, 3], flipped), read by the backward pass alone.  fp32 on the f32-input MFMA,
 * every sum in a fixed order, no floating-point atomics: the same input gives the same bits. */
#define MPMHIP_LPIPS_LAYERS 13
#define MPMHIP_LPIPS_TAPS 5
typedef struct {
  int32_t n, h, w;
  int32_t reserved_;
  const float *weight[MPMHIP_LPIPS_LAYERS];
  const float *bias[MPMHIP_LPIPS_LAYERS];
  float *weight_bwd[MPMHIP_LPIPS_LAYERS];
  const float *tap_weight[MPMHIP_LPIPS_TAPS];
  float mean[3], std[3];
} mpmhip_lpips_desc;
/* One launch that fills every weight_bwd [L] from weight [L]; to be repeated when a weight changes.  Sizes are not read. */
int mpmhip_lpips_prepare_weights(int32_t device, void *stream, const mpmhip_lpips_desc *desc);
/* The workspace for desc's n, h, w (its pointers are not read).  keep = 1: a forward pass whose backward pass will follow (the
 * thirteen maps of x, the five tap maps of y, the tap gradients and two gradient buffers); keep = 0: a forward pass alone (the taps and
 * two alternating buffers per image).  Host arithmetic: written whenever the arguments are valid, and the return is then that of the
 * device check.  MPMHIP_ERR_INVALID: n < 0 or > 1024, h or w < 16 (four poolings must leave 1 x 1) or > 8192, keep not 0 or 1. */
int mpmhip_lpips_workspace_bytes(int32_t device, void *stream, const mpmhip_lpips_desc *desc, int32_t keep, int64_t *out_workspace_bytes);
/* out [1].  19 launches.  keep as above; weight_bwd may be NULL with keep = 0.  MPMHIP_ERR_INVALID also: a NULL weight, bias, input or
 * output, a zero or non-finite std, a workspace that is too small.  n == 0: out = 0. */
int mpmhip_lpips_forward(int32_t device, void *stream, const mpmhip_lpips_desc *desc, const float *x, const float *y, int32_t keep,
                         void *workspace, int64_t workspace_bytes, float *out);
/* dx [n, 3, h, w] = g_out [1] * d out / d x over the workspace a forward pass with keep = 1 left (same desc, x and y no longer needed).
 * 18 launches.  ReLU's derivative is read off the saved output (> 0); a pooling window's gradient goes to its first maximum in
 * row-major order; a tap pixel whose feature vector is all zero contributes nothing (the reference yields NaN there).  There is no
 * gradient to y or to a weight: the network is frozen. */
int mpmhip_lpips_backward(int32_t device, void *stream, const mpmhip_lpips_desc *desc, const float *g_out, void *workspace,
                          int64_t workspace_bytes, float *dx);

/* ---- the regularisation terms of the appearance loop (train_appearance.py:136-150) ------------------------------------------------
 * What the reference computes between render(...) and loss.backward() besides the image loss, as two fused ops with exact backward
 * passes.  Stand-alone maps on [dev] arrays; nothing allocates or synchronises; fp32 data, sums in fp64 in a fixed order, no
 * floating-point atomics: the same input gives the same bits.  The weights of train_appearance.py:87 are the caller's.
 *
 * Mesh terms (scene/mesh_gaussian_model.py:203-246), K = MPMHIP_REG_K = 3 neighbours per face:
 *   out_terms[0] normal = mean_f | mean_k(n_f . n_nb[f,k]) - 1 |,  n_f = d3 / |d3|, d3 = (v2 - v1) x (v3 - v1)      (normal_loss)
 *   out_terms[1] iso    = mean_fk sqrt((sqrt(|c_nb[f,k] - c_f|^2 + 1e-20) - nd[f,k])^2 nw[f,k] + 1e-20)              (iso_loss)
 *   out_terms[2] area   = mean_f | a_f - mean(a) |, a_f = |d3| / 2           (area_loss, the loop's "eq_faces_weight")
 * face_neighbors [n_faces*3] is the array of find_adjacent_faces (utils/general_utils.py:286-316); a row may name its own face, as
 * the reference pads boundary faces (:309-311): such a slot adds n_f . n_f to the mean and sqrt(1e-20 nw + 1e-20) to iso, and its
 * gradient is exactly zero.  The array need not be symmetric.  neighbor_dist / neighbor_weight [n_faces*3] are the set-up of
 * scene/mesh_gaussian_model.py:88-98; out_sq_dist [n_faces*3] or NULL receives |c_nb - c_f|^2 of every slot, from which that set-up
 * is sqrt(.) and exp(-2000 .) (call once on verts_orig[0]; the two inputs play no part in it).  A zero-area face gives NaN in normal,
 * as in the reference; an index outside its range gives NaN and reads nothing.  out_stats [2] = mean(a), mean(sign(a - mean(a))),
 * which the backward pass reads.  scratch [MPMHIP_MESH_REG_SCRATCH(n_faces)] doubles.  n_faces == 0: MPMHIP_OK, nothing written.
 * MPMHIP_ERR_INVALID, nothing launched: a negative count, 36 * n_faces > 2^31 - 1, a required pointer NULL. */
#define MPMHIP_REG_K 3
#define MPMHIP_REG_TPB 256
#define MPMHIP_MESH_REG_SCRATCH(n_faces) (3 * (((int64_t)(n_faces) + MPMHIP_REG_TPB - 1) / MPMHIP_REG_TPB) + ((int64_t)(n_faces) + 1) / 2)
int mpmhip_mesh_reg_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                            const int32_t *face_neighbors, const float *neighbor_dist, const float *neighbor_weight, double *scratch,
                            float *out_terms, float *out_stats, float *out_sq_dist);
/* mpmhip_mesh_reg_backward: from g_terms [3] on the device (the upstream gradients of normal, iso, area; no value passes through
 * the host) to d_verts [n_verts*3], written in full; NULL = not wanted, nothing launched.  The exact derivative with every discrete
 * decision held fixed (sign(0) = 0 inside the absolute values); d area / d a_f = (sign(a_f - mean) - stats[1]) / n_faces.  Row f of
 * the loss touches a stencil of 1 + K faces x 3 corners, S[f, s, c] = faces[nbx[f, s], c] with nbx[f, 0] = f, nbx[f, 1 + k] =
 * face_neighbors[f, k]: d_stencil [n_faces*36] is scratch for the gradient of each of those corners, and vert_start [n_verts+1] /
 * vert_items [12*n_faces] is the vertex -> stencil item table (item = 12 f + 3 s + c, ascending within a vertex), which a vertex
 * walks serially.  A vertex in no face gets exactly 0.  stats [2]: the forward's, for the same verts. */
int mpmhip_mesh_reg_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                             const int32_t *face_neighbors, const float *neighbor_dist, const float *neighbor_weight, const float *stats,
                             const float *g_terms, const int32_t *vert_start, const int32_t *vert_items, float *d_stencil, float *d_verts);
/* Gaussian terms (train_appearance.py:138,147,148; opacity_loss is scene/mesh_gaussian_model.py:222-223 over get_opacity,
 * scene/gaussian_model.py:158), visible = radii[i] > 0 (the rasteriser's int32 radii) or visible[i] != 0 (a byte mask): exactly one
 * of the two pointers is given.
 *   out_terms[0] opacity = mean(1 - sigmoid(opacity [n]))
 *   out_terms[1] xyz     = mean over visible of relu(|xyz[i]| - threshold_xyz)                      xyz, scaling [n*3]
 *   out_terms[2] scale   = mean over visible of | relu(exp(scaling[i]) - threshold_scale) |_2
 * out_n_visible [1]: the count, kept on the device for the backward pass.  No visible row: NaN for xyz and scale (0 / 0, the
 * reference's mean of an empty tensor).  scratch [MPMHIP_GAUSS_REG_SCRATCH(n)] doubles.  n == 0: MPMHIP_OK, nothing written. */
#define MPMHIP_GAUSS_REG_SCRATCH(n) (4 * (((int64_t)(n) + MPMHIP_REG_TPB - 1) / MPMHIP_REG_TPB))
int mpmhip_gauss_reg_forward(int32_t device, void *stream, int32_t n, const float *opacity, const float *xyz, const float *scaling,
                             const int32_t *radii, const uint8_t *visible, float threshold_xyz, float threshold_scale, double *scratch,
                             float *out_terms, int32_t *out_n_visible);
/* mpmhip_gauss_reg_backward: from g_terms [3] on the device to d_opacity [n], d_xyz [n*3], d_scaling [n*3], each written in full,
 * NULL = not wanted.  A relu that binds has zero slope, the norm of an all-zero row has zero slope, a row outside the visible set
 * gets exact zeros for xyz and scale (so with no visible row every such gradient is zero). */
int mpmhip_gauss_reg_backward(int32_t device, void *stream, int32_t n, const float *opacity, const float *xyz, const float *scaling,
                              const int32_t *radii, const uint8_t *visible, float threshold_xyz, float threshold_scale,
                              const int32_t *n_visible, const float *g_terms, float *d_opacity, float *d_xyz, float *d_scaling);

/* ---- densification of the bound Gaussians (scene/gaussian_model.py:378-526, train_appearance.py:245-257) ----------------------------
 * The last block of the appearance loop: the statistics of every iteration, densify_and_prune (clone, split, prune, the face rule
 * of prune_points :379-385) and reset_opacity (:284-287).  Stand-alone maps on [dev] arrays; nothing allocates or synchronises;
 * fp32; integer atomics only: the same input gives the same bits.
 *
 * mpmhip_densify_stats_add (add_densification_stats :524-526 and train_appearance.py:248), in place, one launch: for rows with
 * radii[i] > 0 (the rasteriser's int32 radii) or visible[i] != 0 (a byte mask, counted as radius 1; exactly one of the two pointers
 * is given)  xyz_gradient_accum[i] += sqrt(gx^2 + gy^2) of viewspace_grad [n*3],  denom[i] += 1,  max_radii2D[i] = max(., radii[i]). */
int mpmhip_densify_stats_add(int32_t device, void *stream, int32_t n, const float *viewspace_grad, const int32_t *radii,
                             const uint8_t *visible, float *xyz_gradient_accum, float *denom, float *max_radii2D);
/* densify_and_prune (:508-522 with densify_and_clone :488-506, densify_and_split :453-486, prune_points :378-405) in two calls with
 * the caller's one read-back between them.  With g = accum / denom (NaN -> 0) and gs = exp(scaling[i]) * face_scaling[binding[i]]:
 * clone when g >= max_grad and max(gs) <= dense_limit, split when g >= max_grad and max(gs) > dense_limit (two children, the source
 * leaves); then, over the enlarged set, a row is flagged when sigmoid(opacity) < min_opacity or, with prune_big != 0, when its
 * max world scale > world_limit (the reference's screen-size test is dead: densification_postfix zeroes max_radii2D before it is
 * read, so a screen size only switches the world-size test on); flagged rows leave unless that empties their face.
 * mpmhip_densify_plan decides and leaves out_counts [MPMHIP_DENSIFY_COUNTS] int32 on the device: n_out, n_cloned, n_split (selected),
 * n_pruned (rows the last prune removed), an error flag (a binding outside [0, n_faces); such a row reads nothing), and the rows at
 * which the clones, the first children and the second children begin.  scratch: mpmhip_densify_scratch_bytes(n, n_faces) bytes,
 * handed unchanged to mpmhip_densify_emit.  MPMHIP_ERR_INVALID: a negative count, 3 n + 1 > 2^31 - 1, a required pointer NULL, a
 * scratch that is too small. */
#define MPMHIP_DENSIFY_COUNTS 8
#define MPMHIP_DENSIFY_MAX_TENSORS 24
int mpmhip_densify_scratch_bytes(int32_t device, int32_t n, int32_t n_faces, int64_t *out_bytes);
int mpmhip_densify_plan(int32_t device, void *stream, int32_t n, int32_t n_faces, const float *scaling, const float *opacity,
                        const int32_t *binding, const float *face_scaling, const float *xyz_gradient_accum, const float *denom,
                        float max_grad, float dense_limit, float min_opacity, float world_limit, int32_t prune_big, void *scratch,
                        int64_t scratch_bytes, int32_t *out_counts);
/* mpmhip_densify_emit writes the n_out rows the plan counted, in the reference's order [kept originals | clones | first children |
 * second children], each block in source order: out_src (the source row), out_kind (0 kept, 1 clone, 2 split child), out_binding,
 * out_binding_counter [n_faces] (the new per-face count), and the n_tensors <= MPMHIP_DENSIFY_MAX_TENSORS row-aligned fp32 tensors
 * named by the HOST arrays in / out / widths (floats per row, > 0) / modes: 0 copied, 1 copied for kept rows and zero for new ones
 * (Adam moments), 2 the _xyz and 3 the _scaling of the model (width 3), which a child computes as
 *   xyz = R(rotation[i] / |rotation[i]|) (gs * noise[i, c]) + xyz[i],   scaling = log((gs / face_scaling) / 1.6)
 * with noise [n*2*3] standard normals (build_rotation: utils/general_utils.py:116-137).  One gather launch for all tensors. */
int mpmhip_densify_emit(int32_t device, void *stream, int32_t n, int32_t n_faces, int32_t n_out, const float *xyz, const float *scaling,
                        const float *rotation, const int32_t *binding, const float *face_scaling, const float *noise, const void *scratch,
                        int64_t scratch_bytes, int32_t n_tensors, const float *const *in, float *const *out, const int32_t *widths,
                        const int32_t *modes, int32_t *out_src, int32_t *out_kind, int32_t *out_binding, int32_t *out_binding_counter);
/* reset_opacity (:284-287): out[i] = log(x / (1 - x)), x = min(sigmoid(opacity[i]), 0.01). */
int mpmhip_reset_opacity(int32_t device, void *stream, int64_t n, const float *opacity, float *out);

/* ---- the optimiser step of the appearance loop --------------------------------------------
 * gaussians.optimizer.step() (train_appearance.py:260-261) for the torch.optim.Adam(l, lr=0.0, eps=1e-15) that
 * scene/gaussian_model.py:207-234 and scene/mesh_gaussian_model.py:148-170 set up: no amsgrad, no weight decay.  One call updates
 * n_tensors fp32 tensors in place, in one launch per MPMHIP_ADAM_MAX_TENSORS of them (the table of a launch is its kernel
 * argument); a tensor is worked on in chunks of MPMHIP_ADAM_CHUNK elements.  Every array is a HOST array of length n_tensors; the
 * pointers in params / grads / exp_avg / exp_avg_sq are device pointers to counts[i] floats.  Per element
 *   m' = m + w1 (g - m),   v' = v beta2 + w2 g g,   p' = p - step_size (m' / (sqrt(v') / bc2_sqrt + eps))
 * in fp32 without contraction and in this order, with the caller's scalars: w1 = 1 - beta1, w2 = 1 - beta2, bc2_sqrt =
 * sqrt(1 - beta2^step), step_size = lr / (1 - beta1^step), computed in double and rounded once.  update_param[i] == 0 (a group
 * with lr == 0): params[i] is neither read nor written, the moments still move.  Nothing is allocated, copied or synchronised.
 * MPMHIP_ERR_INVALID: a negative n_tensors or count, a NULL array with n_tensors > 0, a NULL tensor pointer with a positive
 * count, a count above what a launch can index (2^31 / MPMHIP_ADAM_MAX_TENSORS chunks).  Tensors without elements are skipped. */
#define MPMHIP_ADAM_CHUNK 4096
#define MPMHIP_ADAM_MAX_TENSORS 48
int mpmhip_adam_step(int32_t device, void *stream, int32_t n_tensors, void *const *params, const void *const *grads,
                     void *const *exp_avg, void *const *exp_avg_sq, const int64_t *counts, const float *step_size,
                     const float *bc2_sqrt, const float *w1, const float *beta2, const float *w2, const float *eps,
                     const uint8_t *update_param);

/* MPMWARP.export_particle_cov_to_torch (warp_mpm/mpm_solver.py:543-561) = kernel compute_cov_from_F
 * (warp_mpm/mpm_utils.py:1108-1132): new_cov[6p..] = upper triangle (xx xy xz yy yz zz) of F_trial[p] * sym(particle_cov[6p..])
 * * F_trial[p]^T for p < n (= n_particles - n_vertices).  Stand-alone map on [dev] arrays in the reference's AoS layout. */
int mpmhip_cov_from_F(int32_t device, void *stream, const float *particle_F_trial, const float *particle_cov, int32_t n,
                      float *new_cov);

/* ---- after the solver: geometry evaluation --------------------------------------------------
 * What every run of the reference ends with: eval.py:30-56 calls metric.all_mesh_metrics (metric.py:56-63) per frame --
 * 100,000 area-weighted surface samples on each mesh (metric.py:4-8, trimesh's sample_surface), nearest neighbours in
 * both directions (metric.py:18-21, SciPy's cKDTree there; exact brute force here), Chamfer distance (metric.py:23-32)
 * and F-score at tau = 1e-3 (metric.py:34-54).  Stand-alone maps on [dev] arrays (no solver context; `stream` is a
 * hipStream_t, NULL = default stream); nothing here allocates or synchronises, every buffer is the caller's.
 * All four return MPMHIP_ERR_INVALID for a count <= 0, a NULL required pointer or slices < 0.
 *
 * mpmhip_face_areas: area [n_f] = 0.5 |(v1 - v0) x (v2 - v0)| in fp32.  The caller accumulates them (float64, inclusive)
 * into area_cdf [n_f] for mpmhip_mesh_sample. */
int mpmhip_face_areas(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, float *area);
/* metric.py:4-8 without the normals: uniforms [n_samples*3] in [0, 1); sample i lies on the first face f with
 * area_cdf[f] >= (double)u0 * area_cdf[n_f-1] (numpy.searchsorted, side "left": zero-area faces are never picked) at
 * v0 + u1 (v1 - v0) + u2 (v2 - v0), (u1, u2) folded back into the triangle when u1 + u2 > 1.
 * points [n_samples*3]; face_index [n_samples] may be NULL. */
int mpmhip_mesh_sample(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces,
                       const double *area_cdf, const float *uniforms, int32_t n_samples, float *points,
                       int32_t *face_index);
/* metric.py:18-21 squared: dist2 [n_src] = min_j |src_i - dst_j|^2 in the direct form (within 8 * 2^-24 relative of the
 * exact value), index [n_src] (may be NULL) the lowest j that attains it.  src [n_src*3], dst [n_dst*3].
 * best_scratch [n_src] 64-bit words.  slices: in how many parts the targets are cut so that few queries still fill the
 * device (0 = chosen from the sizes; larger than n_dst is clamped); the result does not depend on it, bit for bit.
 * Non-finite coordinates give unspecified values, never an access outside the arrays. */
int mpmhip_nn_dist2(int32_t device, void *stream, const float *src, int32_t n_src, const float *dst, int32_t n_dst,
                    int32_t slices, uint64_t *best_scratch, float *dist2, int32_t *index);
/* metric.py:31 and :34-41 from the two dist2 arrays: out [4] doubles on the device = F-score, Chamfer distance
 * (1000 * (mean12 + mean21)), precision, recall (percent of dist2 <= tau: the reference compares the SQUARED distance
 * with its threshold, metric.py:35).  Sums in fp64 in a fixed order (no floating-point atomics): bitwise reproducible.
 * scratch [MPMHIP_GEO_REDUCE_SCRATCH] doubles.  No host synchronisation: the reference's .item() (eval.py:50-51) is the
 * caller's choice. */
#define MPMHIP_GEO_REDUCE_SCRATCH 256
int mpmhip_geo_reduce(int32_t device, void *stream, const float *dist2_12, int32_t n1, const float *dist2_21, int32_t n2,
                      double tau, double *scratch, double *out);

/* ---- after the solver: the ambient-occlusion bake ---------------------------------------------------------------------
 * What the reference runs as a Blender subprocess per frame (train_material_params.py:819-822 calls blender/bake.py, which bakes
 * type AO with Cycles into aomap/NNN.png, bake.py:37-78): the [map_h*map_w] AO map of the UV mesh, from vertices that are already
 * on the device.  The definition (coverage, texel frame, direction table, any-hit occlusion, margin) is csrc/ao_math.hpp and
 * DESIGN.md section 19; Cycles' own sampling cannot be inspected, so that definition is this project's.  Stand-alone maps on [dev]
 * arrays; nothing here allocates or synchronises.  Scratch is the caller's: the arrays then live and die with the caller's tensors
 * under its allocator's stream rules, and the library keeps no state to destroy.  All arithmetic per frame is fp32, no
 * floating-point atomics, integer atomics only in the grid's count and fill: the same input gives the same bits.
 * All return MPMHIP_ERR_INVALID, with nothing launched, for a negative count, a non-positive map size, map_h * map_w > 2^31 - 1,
 * samples outside [1, 4096], a scratch that is too small or a NULL required pointer.  Indices are the caller's to check.
 *
 * mpmhip_ao_coverage (once per mesh; replaces the UV rasterisation inside bake.py:73): cov_face [map_h*map_w] = the lowest face
 * whose UV triangle (vt [n_vt*2] through ft [n_faces*3], the 'vt' and 'f v/vt' lines) contains the texel centre
 * u = (x + 0.5) / W, v = 1 - (y + 0.5) / H, edges inclusive, both windings, -1 = none; cov_bary [map_h*map_w*2] = the weights of
 * the face's second and third corner, float64 rounded once.  A face without UV area or with a repeated vertex covers nothing. */
int mpmhip_ao_coverage(int32_t device, void *stream, const int32_t *faces, const int32_t *ft, int32_t n_faces, const float *vt,
                       int32_t n_vt, int32_t map_h, int32_t map_w, int32_t *cov_face, float *cov_bary);
/* bytes of scratch that mpmhip_ao_build_grid and mpmhip_ao_trace share for a mesh of n_faces faces, a grid of at most cap_cells
 * cells and at most cap_entries (cell, face) entries. */
int mpmhip_ao_scratch_bytes(int32_t device, int32_t n_faces, int32_t cap_cells, int32_t cap_entries, int64_t *out_bytes);
/* The per-texel frame the rays leave from (inspection; the trace computes the same values itself): origin, normal, tangent
 * [map_h*map_w*3] each, zeros on texels that no face covers or whose face has no area in this frame.  rot [map_h*map_w*2] is the
 * per-texel (cos, sin) table. */
int mpmhip_ao_texel_frames(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, int32_t map_h,
                           int32_t map_w, const int32_t *cov_face, const float *cov_bary, const float *rot, float *origin,
                           float *normal, float *tangent);
/* Per frame, stage 1 (bake.py:50, the import of uvmesh/NNN.obj, and Cycles' own BVH build): one 48-byte record (v0, e1, e2) per
 * face, the mesh's bounding box, and a uniform grid over it (cells of about twice the mean edge, at most cap_cells) as
 * count / exclusive scan / fill, all in scratch. */
int mpmhip_ao_build_grid(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, int32_t cap_cells,
                         int32_t cap_entries, void *scratch, int64_t scratch_bytes);
/* Per frame, stage 2 (bake.py:73, bpy.ops.object.bake(type='AO')): ao [map_h*map_w] = 1 - occluded / samples on the n_cov texels
 * of cov_list (the covered ones, compacted once); other texels are not written.  dirs [samples*3] is the direction table.  A ray
 * is occluded when it meets any face but the texel's own with bias < t <= max_distance.  If the frame's grid needed more than
 * cap_entries entries every texel of cov_list is NaN: loud in the image, no access out of bounds. */
int mpmhip_ao_trace(int32_t device, void *stream, const float *verts, const int32_t *faces, int32_t n_faces, const int32_t *cov_face,
                    const float *cov_bary, const int32_t *cov_list, int32_t n_cov, const float *rot, const float *dirs,
                    int32_t samples, float bias, float max_distance, int32_t cap_cells, int32_t cap_entries, void *scratch,
                    int64_t scratch_bytes, float *ao);
/* Per frame, stage 3, one margin pixel (bake.py:37, bake.margin = ao_res // 256): a texel with in_mask = 0 and covered texels
 * among its 8 neighbours takes their mean (row-major order) and out_mask = 1; in and out must not overlap. */
int mpmhip_ao_margin(int32_t device, void *stream, int32_t map_h, int32_t map_w, const float *in_val, const uint8_t *in_mask,
                     float *out_val, uint8_t *out_mask);

/* ---- after the solver: the Gaussian rasteriser ----------------------------------------------------------------------
 * What the reference calls as diff_gauss.GaussianRasterizer (gaussian_renderer/__init__.py:14,36-103; the extension is not
 * vendored there, README.md:51): the published 3D Gaussian splatting forward pass, as the eval loop
 * (train_material_params.py:857-872) and the demo (run_demo.py:540-604) use it; the backward pass follows below.  All arithmetic fp32, no floating-point
 * atomics: the same input gives the same bits.
 *
 * GaussianRasterizationSettings, gaussian_renderer/__init__.py:36-49 (prefiltered and debug have no meaning here).
 * viewmatrix / projmatrix are the reference's world_view_transform / full_proj_transform (scene/cameras.py:26-39): row-major,
 * points multiply from the left as row vectors. */
typedef struct {
  int32_t image_height, image_width;
  float tanfovx, tanfovy;
  float bg[3];
  float scale_modifier;
  int32_t sh_degree;       /* 0..3, read only when shs is given */
  const float *viewmatrix; /* [dev] [16] */
  const float *projmatrix; /* [dev] [16] */
  const float *campos;     /* [dev] [3] */
} mpmhip_raster_settings;

/* of the newest mpmhip_raster_forward of a handle */
typedef struct {
  int64_t n_entries;        /* (tile, Gaussian) pairs that were sorted */
  int32_t max_tile_entries; /* the longest tile list */
  int32_t n_visible;        /* Gaussians with radius > 0 */
  int64_t scratch_bytes;    /* device memory the handle holds */
} mpmhip_raster_stats_t;

typedef struct mpmhip_raster mpmhip_raster;

/* A handle owns the scratch of the pipeline (records, sort keys, sort temporaries, tile ranges) on `device` and launches on
 * `stream` (hipStream_t, NULL = default stream).  The scratch grows geometrically when a frame needs more and is reused
 * otherwise: no allocation in steady state.  Not thread-safe; distinct handles are independent. */
int mpmhip_raster_create(int32_t device, void *stream, mpmhip_raster **out);
void mpmhip_raster_destroy(mpmhip_raster *r);
/* The rasterizer(...) call of gaussian_renderer/__init__.py:95-103 on [dev] arrays: means3D [n*3]; shs [n*n_sh_coeffs*3]
 * (coefficient-major, GaussianModel.get_features) evaluated as utils/sh_utils.py:57-100 does at degree sh_degree, OR
 * colors_precomp [n*3]; opacities [n]; scales [n*3] and rotations [n*4] WXYZ, OR cov3D_precomp [n*6] (xx xy xz yy yz zz).
 * Outputs: out_color [3*H*W] (= colour + T * bg), out_alpha [H*W] (= 1 - T, the reference's mask), radii [n] (0 = culled).
 * Blocks the host once per call: the number of (tile, Gaussian) entries is read back to size the sort, as in the CUDA
 * original; everything else is asynchronous on the handle's stream.
 * MPMHIP_ERR_INVALID: n < 0, a non-positive image size, both or neither of shs / colors_precomp, both or neither of
 * (scales, rotations) / cov3D_precomp, sh_degree outside 0..3 or n_sh_coeffs < (sh_degree + 1)^2; nothing is launched then.
 * n == 0 renders the background.  MPMHIP_ERR_LIMIT: more than 2^31 - 1 entries. */
int mpmhip_raster_forward(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                          int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                          const float *rotations, const float *cov3D_precomp, float *out_color, float *out_alpha,
                          int32_t *radii);
/* ---- the rasteriser's backward pass: what train_appearance.py:123-155 needs ---------------------------------------------
 * There the render call (gaussian_renderer/__init__.py:95-103 with override_color, scales and rotations) is followed by
 * image * mask, the loss (L1 + SSIM: mpmhip_image_loss_* below; LPIPS: the caller's) and loss.backward()
 * (train_appearance.py:123-155), and viewspace_point_tensor.grad -- the
 * gradient of means2D -- feeds the densification statistics (train_appearance.py:245-253).  The gradient is the exact
 * derivative of the forward function above with every discrete decision held fixed (culling, radius, tile rectangle, depth
 * order, power > 0, alpha < 1/255, the T < 1e-4 finish); the clamps -- alpha = min(0.99, .), the frustum clamp inside the
 * Jacobian, max(0, sh + 0.5) -- have zero slope where they bind.  No floating-point atomics: the same input gives the same bits.
 *
 * A handle's scratch is overwritten by its next forward call, so a frame that will be differentiated is copied out:
 *   mpmhip_raster_forward_grad  mpmhip_raster_forward (same arguments, same image / alpha / radii bits) that also records, per
 *                               pixel, the final T and the position in its tile's list at which it stopped, and the map from a
 *                               Gaussian's entries to their sorted positions
 *   mpmhip_raster_saved_bytes   size of that frame's state and its number of (tile, Gaussian) entries; MPMHIP_ERR_STATE when the
 *                               handle's newest frame was not a forward_grad
 *   mpmhip_raster_save          asynchronous device-to-device copy of the state, on the handle's stream, into the caller's [dev]
 *                               buffer of exactly that size (16-byte aligned): packed records and colours, sorted Gaussian
 *                               indices, tile ranges, offsets, rectangles, the inverse map, per-pixel T and position
 *   mpmhip_raster_backward      the settings and inputs of the forward call, the saved buffer with its two sizes, dL_dimage
 *                               [3*H*W] and dL_dalpha [H*W] (either may be NULL = zeros), and the [dev] outputs: d_means3D [n*3]
 *                               (projection + Jacobian of the 2D covariance + SH view direction), d_means2D [n*3] (dL/dpx * W/2,
 *                               dL/dpy * H/2, 0: the gradient with respect to an additive NDC offset of the pixel centre),
 *                               d_shs [n*n_sh_coeffs*3] OR d_colors_precomp [n*3], d_opacities [n], d_scales [n*3] and
 *                               d_rotations [n*4] (through the normalisation of the quaternion) OR d_cov3D_precomp [n*6] (an
 *                               off-diagonal value gets the sum of both positions it fills).  Every element is written, zeros
 *                               for a culled Gaussian.  Any handle of the same device may run it (its own temporaries, 36 B per
 *                               entry, live in the handle); asynchronous on that handle's stream.
 * MPMHIP_ERR_INVALID and nothing launched: the conditions of mpmhip_raster_forward, a NULL saved buffer or required output, or
 * saved_bytes that is not the size of a frame of this n, image size and n_entries. */
int mpmhip_raster_forward_grad(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                               int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                               const float *rotations, const float *cov3D_precomp, float *out_color, float *out_alpha,
                               int32_t *radii);
int mpmhip_raster_saved_bytes(const mpmhip_raster *r, int64_t *bytes, int64_t *n_entries);
int mpmhip_raster_save(mpmhip_raster *r, void *dst, int64_t bytes);
int mpmhip_raster_backward(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                           int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                           const float *rotations, const float *cov3D_precomp, const void *saved, int64_t saved_bytes,
                           int64_t n_entries, const float *dL_dimage, const float *dL_dalpha, float *d_means3D, float *d_means2D,
                           float *d_shs, float *d_colors_precomp, float *d_opacities, float *d_scales, float *d_rotations,
                           float *d_cov3D_precomp);
/* ---- extra attribute channels: what the 4D-DRESS tracking script needs of the render call -----------------------------------
 * preprocess/train_mesh_lbs_4ddress.py:260-277 hands the rasteriser 'extra_attrs': variables['cloth_mask'], an [N, 2] table
 * (upper and lower garment, 0 / 1), :299 reads the blended channels back as the sixth value of the call, and :306 compares them
 * with the data's garment mask (l1_loss_v1, weight 2).  Per pixel, with alpha_k, T_k and the finishing rule of the colour,
 *   extra_e = sum_k a_ke alpha_k T_k,  e = 0 .. E-1,  1 <= E <= 8,  no background term
 * (UNCONFIRMED against the CUDA original, whose source is not at hand: DESIGN.md).  The gradient is the exact derivative with the
 * decisions held fixed, as above; the extras' share of the geometry and opacity gradients adds to that of image and alpha.
 *
 *   mpmhip_raster_extra_forward   train_mesh_lbs_4ddress.py:260-277, :299 (what :306 then compares).  One more walk over the tile lists of the frame that
 *                                 mpmhip_raster_forward_grad has just rendered on this handle, each pixel up to where its colour
 *                                 walk stopped: extra [dev] [n*E] -> out_extra [dev] [E*H*W], every element written (zeros where
 *                                 nothing contributes, and for n == 0).  Valid only directly after a forward_grad of the same n
 *                                 and image size on the handle: MPMHIP_ERR_STATE otherwise.  Asynchronous on the handle's stream.
 *   mpmhip_raster_backward_extra  train_mesh_lbs_4ddress.py:306 and its loss.backward(), back through the call of :299 to the
 *                                 table of :260-277.  mpmhip_raster_backward (same arguments,
 *                                 same stages) with the extras' tile pass in between: extra [n*E] as in the forward call, g_extra
 *                                 [E*H*W] = dL/dextra (NULL = zeros), d_extra [n*E] = dL/dextra_attrs, every element written.
 *                                 Its temporaries (the 36 B per entry of mpmhip_raster_backward and 4 E more) live in the handle.
 * MPMHIP_ERR_INVALID and nothing launched: E < 1 or E > 8, a NULL extra, out_extra or d_extra (n > 0), and the conditions of
 * mpmhip_raster_backward. */
int mpmhip_raster_extra_forward(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *extra, int32_t E,
                                float *out_extra);
int mpmhip_raster_backward_extra(mpmhip_raster *r, const mpmhip_raster_settings *s, int32_t n, const float *means3D, const float *shs,
                                 int32_t n_sh_coeffs, const float *colors_precomp, const float *opacities, const float *scales,
                                 const float *rotations, const float *cov3D_precomp, const void *saved, int64_t saved_bytes,
                                 int64_t n_entries, const float *dL_dimage, const float *dL_dalpha, float *d_means3D,
                                 float *d_means2D, float *d_shs, float *d_colors_precomp, float *d_opacities, float *d_scales,
                                 float *d_rotations, float *d_cov3D_precomp, const float *extra, int32_t E, const float *g_extra,
                                 float *d_extra);
/* counts of the newest frame; synchronous, runs one small count kernel */
int mpmhip_raster_stats(const mpmhip_raster *r, mpmhip_raster_stats_t *out);
/* Measurement only (tools/raster_bench.py; the counterpart of mpmhip_profile_enable for this pipeline): while on, every
 * frame is bracketed by hipEvents between its stages -- preprocess, scan + read-back, duplicate, sort, ranges, render -- and
 * waits for its last one.  The call first copies out what was accumulated so far (stage_ms [MPMHIP_RASTER_STAGES] milliseconds
 * summed over `frames` frames; either may be NULL); switching from off to on then resets the sums. */
#define MPMHIP_RASTER_STAGES 6
int mpmhip_raster_profile(mpmhip_raster *r, int32_t on, double *stage_ms, int64_t *frames);

/* ---- after the rasteriser: the image loss and the image metrics ----------------------------------------------------------
 * What stands between the render call and loss.backward() in train_appearance.py:132-134 -- (1 - lambda) l1_loss(image, gt)
 * + lambda (1 - ssim(image, gt)), utils/loss_utils.py:18-64 -- and what eval.py:89-91 closes every run with: psnr
 * (utils/image_utils.py:17-19) and ssim.  LPIPS (train_appearance.py:133, eval.py:89) needs network weights and stays the
 * caller's.  Stand-alone maps on [dev] arrays (no context; `stream` is a hipStream_t, NULL = default stream); nothing here
 * allocates or synchronises, every buffer is the caller's.  A "plane" is one (batch, channel) image of H x W floats;
 * planes = N * C, planes stored one after the other.  Both return MPMHIP_ERR_INVALID, with nothing launched, for a NULL
 * required pointer, planes, H or W <= 0, or planes * H * W > 2^31 - 1.  All arithmetic fp32 with the sums in fp64 in a fixed
 * order, no floating-point atomics: the same input gives the same bits.
 *
 * mpmhip_image_loss_forward: torch.abs(img - gt).mean() (loss_utils.py:18-19), ((img - gt) ** 2).mean() (the mse of
 * image_utils.py:18) and _ssim(...).mean() (loss_utils.py:44-62: the 11-tap Gaussian window of :24-32, sigma 1.5, zero padding
 * of 5, C1 = 0.01^2, C2 = 0.03^2, variances as E[x^2] - mu^2 in fp32 as there), each PER PLANE:
 * out_means [planes*3] = mean |d|, mean d^2, mean SSIM map of plane 0, then of plane 1, ...  The reference's means over
 * planes, 1 - ssim, the lambda mix and 20 log10(1 / sqrt(mse)) are the caller's few scalar operations.
 * maps [planes*3*H*W] or NULL: per plane three H x W planes, the partial derivatives of the SSIM map value with respect to
 * mu1 (in total), sigma1^2 and sigma12 at every pixel, which the backward pass convolves; NULL (evaluation) stores nothing.
 * scratch [MPMHIP_IMAGE_LOSS_SCRATCH(planes, H, W)] doubles: one triple per 16 x 16 tile. */
#define MPMHIP_IMAGE_LOSS_SCRATCH(planes, H, W) ((int64_t)(planes) * (((H) + 15) / 16) * (((W) + 15) / 16) * 3)
int mpmhip_image_loss_forward(int32_t device, void *stream, const float *img, const float *gt, int32_t planes, int32_t H, int32_t W,
                              float *maps, double *scratch, float *out_means);
/* What autograd does for loss.backward() through the expressions above (train_appearance.py:155), for img alone (gt gets no
 * gradient): with the upstream gradients of the three per-plane means, g_l1, g_mse, g_ssim [planes] on the device (no value
 * passes through the host),
 *   d_img(q) = (g_l1[p] sign(x - y) + g_mse[p] 2 (x - y) + g_ssim[p] dSSIM(q)) / (H W),   sign(0) = 0 as torch's abs backward,
 *   dSSIM(q) = (w * d_mu)(q) + 2 x(q) (w * d_s1)(q) + y(q) (w * d_s12)(q),   w * . the zero-padded window convolution of the
 * maps that mpmhip_image_loss_forward stored for the same img and gt.  d_img [planes*H*W]: every element is written. */
int mpmhip_image_loss_backward(int32_t device, void *stream, const float *img, const float *gt, int32_t planes, int32_t H, int32_t W,
                               const float *maps, const float *g_l1, const float *g_mse, const float *g_ssim, float *d_img);

/* ---- between the rasteriser and the loss: the image head -------------------------------------------------------------------
 * The expression between the render call and the loss of train_appearance.py:126-127 (again at :206-207 and in
 * train_material_params.py:865-870),
 *   image = render * exp(cam_m[camera_idx])[:, None, None] + cam_c[camera_idx][:, None, None]
 *   image = (image * mask).clip(0., 1.)
 * with its gradient, and the forward-only maps of the evaluation side.  Stand-alone maps on [dev] arrays (no context; `stream`
 * is a hipStream_t, NULL = default stream); nothing here allocates or synchronises, every buffer is the caller's.  render
 * [3*H*W] (CHW), mask [H*W] (the rasteriser's alpha), cam_m and cam_c [n_cam*3]; `cam` is the camera's row, read on the device.
 * All return MPMHIP_ERR_INVALID, with nothing launched, for a NULL required pointer, H or W <= 0, H * W > 2^31 - 1, n_cam <= 0
 * or cam outside [0, n_cam).  All arithmetic fp32 with every operation rounded on its own as torch rounds them, no
 * floating-point atomics: the same input gives the same bits.  A lane takes four consecutive pixels; planes that are 16-byte
 * aligned with H * W % 4 == 0 are read and written 16 bytes at a time, anything else pixel by pixel, with the same results.
 *
 * mpmhip_image_head_forward: out_image [3*H*W], v = (render[c] * exp(cam_m[cam][c]) + cam_c[cam][c]) * mask,
 * image = min(max(v, 0), 1), NaN propagating as in torch.  One launch.
 *
 * Workgroups of the forward and backward launches and doubles of the backward scratch, pure functions of H * W: one
 * workgroup of 256 lanes per 1024 pixels, at most 1024 (beyond 1024 x 1024 pixels they stride over the image), six sums each. */
#define MPMHIP_IMAGE_HEAD_WORKGROUPS(H, W) \
  ((((int64_t)(H) * (W) + 1023) / 1024) < 1024 ? (((int64_t)(H) * (W) + 1023) / 1024) : (int64_t)1024)
#define MPMHIP_IMAGE_HEAD_SCRATCH(H, W) (MPMHIP_IMAGE_HEAD_WORKGROUPS(H, W) * 6)
int mpmhip_image_head_forward(int32_t device, void *stream, const float *render, const float *mask, const float *cam_m, const float *cam_c,
                              int32_t n_cam, int32_t cam, int32_t H, int32_t W, float *out_image);
/* What autograd does for loss.backward() through those two lines (train_appearance.py:155): from g_image [3*H*W] (NULL counts
 * as zeros) to the four gradients, each wanted on its own (NULL = not wanted; every wanted output is written in full).  The
 * clip has TORCH's slope: with v recomputed by the forward's own function, g_v = g_image where 0 <= v <= 1, both ends
 * included, and 0 elsewhere -- a pixel with mask == 0 has v == 0 exactly and still hands a gradient to mask.  a_c =
 * exp(cam_m[cam][c]):
 *   d_render [3*H*W]    g_v * mask * a_c
 *   d_mask [H*W]        sum_c g_v[c] * (render[c] * a_c + cam_c[cam][c])
 *   d_cam_c [n_cam*3]   row cam: sum_pixels g_v[c] * mask; every other row zero
 *   d_cam_m [n_cam*3]   row cam: a_c * sum_pixels g_v[c] * mask * render[c]; every other row zero
 * the dense tensors torch's index backward hands to the optimiser.  The pixel sums have fp32 terms and fp64 additions in an
 * order that depends on H * W alone: per-workgroup partials in scratch [MPMHIP_IMAGE_HEAD_SCRATCH(H, W)] doubles (required
 * when d_cam_m or d_cam_c is wanted), folded in index order by one workgroup that also writes both [n_cam*3] outputs.  Two
 * launches, one when neither d_cam_m nor d_cam_c is wanted, none when nothing is. */
int mpmhip_image_head_backward(int32_t device, void *stream, const float *render, const float *mask, const float *cam_m, const float *cam_c,
                               int32_t n_cam, int32_t cam, int32_t H, int32_t W, const float *g_image, double *scratch, float *d_render,
                               float *d_mask, float *d_cam_m, float *d_cam_c);
/* The evaluation side, forward only: what replaces the PNG, OpenCV and host detour of train_material_params.py:865-876 and
 * eval.py:68-87.  One launch each.
 * mpmhip_image_head_bytes (train_material_params.py:865-870): r = (render * exp(cam_m[cam]) + cam_c[cam]) * mask, plus
 * (1 - mask) if white != 0, then (clamp(r, 0, 1) * 255.f) truncated toward zero, stored HWC in out_u8 [H*W*3].  cam_m and
 * cam_c both NULL: the identity (n_cam and cam are not looked at), which makes the ground-truth frame of :847-849 and :874
 * from (gt_rgb, gt_msk); one of them NULL alone is MPMHIP_ERR_INVALID.
 * mpmhip_image_compose (train_appearance.py:108-110): out [3*H*W] = rgb * msk, plus (1 - msk) if white != 0; not clipped.
 * mpmhip_eval_pair (eval.py:68-87): from the two byte frames pred_u8, gt_u8 [H*W*3] (HWC) and the float mask [H*W] to
 * out_pred, out_gt [3*H*W] (CHW): byte / 255 as a true fp32 division; with remove_white != 0 (the actorshq branch, :73-76) a
 * pixel whose three bytes sum to >= 689 -- for bytes exactly mean(axis=0) > 0.90 -- is zero in that image, each image on its
 * own; then both times the mask. */
int mpmhip_image_head_bytes(int32_t device, void *stream, const float *render, const float *mask, const float *cam_m, const float *cam_c,
                            int32_t n_cam, int32_t cam, int32_t white, int32_t H, int32_t W, uint8_t *out_u8);
int mpmhip_image_compose(int32_t device, void *stream, const float *rgb, const float *msk, int32_t white, int32_t H, int32_t W, float *out);
int mpmhip_eval_pair(int32_t device, void *stream, const uint8_t *pred_u8, const uint8_t *gt_u8, const float *mask, int32_t remove_white,
                     int32_t H, int32_t W, float *out_pred, float *out_gt);

/* ---- the mesh tracking step (preprocess/train_mesh_lbs_actorshq.py:209-279) ---------------------------------------------------------
 * What the tracking loop computes between the trained vertices and the rasteriser's argument list, and the loss terms the
 * appearance loop does not have.  Stand-alone maps on [dev] arrays; nothing allocates or synchronises; fp32 data, sums in fp64 in a
 * fixed order, no floating-point atomics: the same input gives the same bits.  faces [n_faces*3] index verts [n_verts*3]; an index
 * outside [0, n_verts) reads nothing and gives NaN.  A zero-area face gives NaN, as in the reference.  MPMHIP_ERR_INVALID, nothing
 * launched: a negative count, 3 * n_faces > 2^31 - 1, a required pointer NULL.  n_faces == 0: MPMHIP_OK.
 *
 * mpmhip_track_render_vars (params2rendervar :209-225), one Gaussian per face, one launch:
 *   out_means3D [n_faces*3]  (v1 + v2 + v3) / 3                                  compute_face_barycenters (utils/geo_utils.py:32-38)
 *   out_rotations [n_faces*4] WXYZ, the quaternion of the matrix with columns x, y, z: x the longest of e1 = v2 - v1, e2 = v3 - v2,
 *                 e3 = v1 - v3 (the first of the longest), normalised; z the normal of compute_face_normals (:21-30) normalised
 *                 again; y = z x x, normalised                                   compute_q_from_faces (:40-75)
 *   out_scales [n_faces*3] exp(log_scales);  out_opacities [n_faces] sigmoid(logit_opacities)
 * The matrix -> quaternion map restates pytorch3d.transforms.matrix_to_quaternion (roots sqrt(max(0, 1 +- m00 +- m11 +- m22)), rows
 * divided by 2 max(root, 0.1), the row of the largest root, then w >= 0) and is UNCONFIRMED against pytorch3d itself; q and -q are
 * the same rotation. */
#define MPMHIP_TRACK_TPB 256
int mpmhip_track_render_vars(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                             const float *log_scales, const float *logit_opacities, float *out_means3D, float *out_rotations,
                             float *out_scales, float *out_opacities);
/* mpmhip_track_render_vars_backward: from the four upstream gradients (each may be NULL = zeros) to d_verts [n_verts*3],
 * d_log_scales [n_faces*3], d_logit_opacities [n_faces], each written in full, NULL = not wanted.  The exact derivative with the
 * longest edge and the quaternion's branch and sign held fixed.  d_stencil [n_faces*9] is scratch for the gradient of each corner;
 * vert_start [n_verts+1] / vert_items [3*n_faces] is the vertex -> corner table (item = 3 f + c, ascending within a vertex), which a
 * vertex walks serially: a vertex in no face gets exactly 0.  The table and d_stencil are needed only with d_verts. */
int mpmhip_track_render_vars_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                      const float *log_scales, const float *logit_opacities, const float *g_means3D, const float *g_rotations,
                                      const float *g_scales, const float *g_opacities, const int32_t *vert_start, const int32_t *vert_items,
                                      float *d_stencil, float *d_verts, float *d_log_scales, float *d_logit_opacities);
/* compute_face_normals and compute_face_areas (utils/geo_utils.py:21-30, :77-85): out_normals [n_faces*3], out_areas [n_faces], either
 * may be NULL.  Forward only. */
int mpmhip_track_face_geometry(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                               float *out_normals, float *out_areas);
/* The loss terms of :242, :254, :263-268:
 *   out_terms[0] area    = mean_f | |e1 x e2| / 2 - pi s0 s1 |,  s = exp(log_scales)
 *   out_terms[1] scale   = mean_f s2
 *   out_terms[2] opacity = mean_f (1 - sigmoid(logit_opacities))
 * scratch [MPMHIP_TRACK_TERMS_SCRATCH(n_faces)] doubles.  n_faces == 0: nothing written. */
#define MPMHIP_TRACK_TERMS_SCRATCH(n_faces) (3 * (((int64_t)(n_faces) + MPMHIP_TRACK_TPB - 1) / MPMHIP_TRACK_TPB))
int mpmhip_track_terms_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                               const float *log_scales, const float *logit_opacities, double *scratch, float *out_terms);
/* from g_terms [3] on the device to d_verts, d_log_scales, d_logit_opacities as above; sign(0) = 0 inside the absolute value */
int mpmhip_track_terms_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                const float *log_scales, const float *logit_opacities, const float *g_terms, const int32_t *vert_start,
                                const int32_t *vert_items, float *d_stencil, float *d_verts, float *d_log_scales, float *d_logit_opacities);
/* compute_vertex_normals (utils/geo_utils.py:8-19): out_normals [n_verts*3] = the sum over the vertex's faces, in ascending face order
 * through the table above, of (v0 - v1) x (v2 - v1), normalised.  A vertex in no face gives NaN (0 / 0), as in the reference.
 * Forward only. */
int mpmhip_track_vertex_normals(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                const int32_t *vert_start, const int32_t *vert_items, float *out_normals);
/* collision_penalty (preprocess/losses/physics.py:6-20) without the [n, n_body] distance matrix: out_index [n] = the nearest of
 * vb [n_body*3] to va[i] by the kernel of mpmhip_nn_dist2 (the exact minimum of the direct-form squared distance, the lowest index on
 * a tie); with nb [n_body*3] given, out_distance [n] = -nb[j] . (va[i] - vb[j]) and, by mode,
 *   MPMHIP_TRACK_DISTANCE nothing more;  MPMHIP_TRACK_AVERAGE out_value[0] = sum_i max(eps - d_i, 0) / n;
 *   MPMHIP_TRACK_CUBED out_value[0] = sum_i max(eps - d_i, 0)^3.
 * nb == NULL: the index alone (NearestNeighbour of preprocess/losses/layers.py).  best_scratch [n] uint64; scratch
 * [MPMHIP_TRACK_COLLISION_SCRATCH(n)] doubles (the two penalty modes).  n == 0: MPMHIP_OK, nothing written.  n_body must be positive. */
#define MPMHIP_TRACK_DISTANCE 0
#define MPMHIP_TRACK_AVERAGE 1
#define MPMHIP_TRACK_CUBED 2
#define MPMHIP_TRACK_COLLISION_SCRATCH(n) (((int64_t)(n) + MPMHIP_TRACK_TPB - 1) / MPMHIP_TRACK_TPB)
int mpmhip_track_collision_forward(int32_t device, void *stream, const float *va, int32_t n, const float *vb, const float *nb, int32_t n_body,
                                   float eps, int32_t mode, uint64_t *best_scratch, double *scratch, int32_t *out_index, float *out_distance,
                                   float *out_value);
/* d_va [n*3] from the forward's index and distance: -g[i] nb[j] in the distance mode (g [n]); g[0] slope nb[j] / n and
 * g[0] 3 pen^2 nb[j] in the penalty modes (g [1]), slope = 1 where eps - d > 0, 0 where < 0 and exactly 1/2 where equal, as
 * torch.maximum.  The body receives no gradient.  d_va == NULL: nothing launched. */
int mpmhip_track_collision_backward(int32_t device, void *stream, int32_t n, const float *nb, int32_t n_body, const int32_t *index,
                                    const float *distance, float eps, int32_t mode, const float *g, float *d_va);

/* ---- the 4D-DRESS tracking script's two further terms (preprocess/train_mesh_lbs_4ddress.py:279-292, :361, :363) ---------------------
 * Stateless like the entry points above, and under the same rules: fp32 data, sums in fp64 in a fixed order, no floating-point
 * atomics, workgroups of MPMHIP_TRACK_TPB.  MPMHIP_ERR_INVALID, nothing launched: a count that is not positive, a required pointer
 * NULL, a scratch shorter than its macro says.
 *
 * mpmhip_track4d_laplacian_forward replaces variables['laplacian_matrix'].mm(vertices).norm(dim=1).mean() (:363) and the dense
 * [V, V] matrix of :212-214 (Meshes(...).laplacian_packed().to_dense()) by a gather over the vertex adjacency: nbr_start
 * [n_verts+1] / nbr [n_nbr] is the CSR table of the undirected edges in both directions, ascending within a row.
 *   out_lv [n_verts*3]   (Lv)_i = (sum_{j in N(i)} v_j) / deg(i) - v_i; -v_i for a vertex with no neighbour
 *   out_value [1]        mean_i |(Lv)_i| over all n_verts rows
 * The sum is divided by the degree (pytorch3d stores 1 / deg in the matrix: a difference at rounding level), so neighbours that sum
 * to exactly deg * v_i give exactly 0.  The uniform Laplacian restates pytorch3d's and is UNCONFIRMED against pytorch3d itself.
 * Either output may be NULL; scratch [n_scratch >= MPMHIP_TRACK4D_LAPLACIAN_SCRATCH(n_verts)] doubles is needed with out_value. */
#define MPMHIP_TRACK4D_LAPLACIAN_SCRATCH(n_verts) (((int64_t)(n_verts) + MPMHIP_TRACK_TPB - 1) / MPMHIP_TRACK_TPB)
int mpmhip_track4d_laplacian_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *nbr_start,
                                     const int32_t *nbr, int32_t n_nbr, double *scratch, int32_t n_scratch, float *out_lv, float *out_value);
/* d_verts [n_verts*3] of :363 from the forward's lv and the upstream scalar g [1] on the device:
 * u_i = (g / n_verts) lv_i / |lv_i| (0 where the norm is 0, torch's subgradient), d_verts_j = sum_{i in N(j)} u_i / deg(i) - u_j.
 * A gather over the same table; the vertices are not read.  d_verts == NULL: nothing launched. */
int mpmhip_track4d_laplacian_backward(int32_t device, void *stream, const float *lv, int32_t n_verts, const int32_t *nbr_start,
                                      const int32_t *nbr, int32_t n_nbr, const float *g, float *d_verts);
/* scale_ratio_loss (:279-292, called at :361 with the thresholds 5.0 and 1.0) on scales [n_faces*3], the `scales` entry of the
 * render variables.  Per face m = the longest of |v_k - v_{(k+1) mod 3}|, a = max(s0, s1), b = min(s0, s1), r = a / (b + 1e-8),
 * q = a / (m + 1e-8):
 *   out_terms[0] scale_ratio          = mean(max(r, th_ratio) - th_ratio)
 *   out_terms[1] scale_edge_ratio     = mean(max(q, th_edge) - th_edge)
 *   out_terms[2] scale_edge_ratio_var = the unbiased variance of q (NaN for n_faces == 1, as torch.var)
 *   out_terms[3] the mean of q, which the backward reads
 * scratch [n_scratch >= MPMHIP_TRACK4D_SCALE_RATIO_SCRATCH(n_faces)] doubles. */
#define MPMHIP_TRACK4D_SCALE_RATIO_SCRATCH(n_faces) (4 * (((int64_t)(n_faces) + MPMHIP_TRACK_TPB - 1) / MPMHIP_TRACK_TPB))
int mpmhip_track4d_scale_ratio_forward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces, int32_t n_faces,
                                       const float *scales, float th_ratio, float th_edge, double *scratch, int32_t n_scratch,
                                       float *out_terms);
/* from terms (the forward's four) and g_terms [3] on the device to d_verts [n_verts*3] and d_scales [n_faces*3] (column 2 exactly 0),
 * each written in full, NULL = not wanted.  Decisions as torch takes them on the CPU: the first of equal maxima and of equal minima,
 * slope 1 at r == th_ratio and q == th_edge, no gradient through a longest edge of length zero.  A g_terms entry that is exactly zero
 * leaves no trace.  d_stencil [n_faces*9] and the vertex -> corner table (above) are needed only with d_verts. */
int mpmhip_track4d_scale_ratio_backward(int32_t device, void *stream, const float *verts, int32_t n_verts, const int32_t *faces,
                                        int32_t n_faces, const float *scales, float th_ratio, float th_edge, const float *terms,
                                        const float *g_terms, const int32_t *vert_start, const int32_t *vert_items, float *d_stencil,
                                        float *d_verts, float *d_scales);

/* ---- re-posing: k nearest neighbours and linear-blend skinning (utils/smplx_deformer.py:164-337) ------------------------------------
 * What the reference's drivers do with SmplxDeformer between a tracked mesh and the solver's input (train_material_params.py:335-349,
 * preprocess/train_mesh_lbs_actorshq.py:495-516), without pytorch3d or open3d.  Stand-alone maps on [dev] arrays; nothing allocates
 * or synchronises; fp32, no atomics, fixed summation orders: the same input gives the same bits.  The SMPL-X forward is the caller's:
 * A is smplx_output.transform_mat.
 *
 * mpmhip_knn (find_k_closest_verts :164-185 = pytorch3d's knn_points; o3d_knn of preprocess/helpers.py:84-94; knn_points(K=1) of
 * lbs_weights_inpainting_*.py:60): for every query [n*dim] the k targets [m*dim] of smallest direct-form squared distance
 * sum_d (q_d - t_d)^2 (ascending d), brute force and exact, ordered ascending by (distance, index): equal distances go to the lower
 * index.  dim is 3 or 6, 1 <= k <= min(m, 16).  out_dists [n*k], out_idx [n*k].  The targets are cut into `slices` parts (0: chosen by
 * the library) that are searched by different workgroups and merged by the total order of the keys (bits of d2) << 32 | index, so
 * the result does not depend on `slices`.  scratch [scratch_len] uint64 with scratch_len >= what mpmhip_knn_scratch reports for the
 * same n, m, dim, k and slices (it needs no device).  Non-finite input: unspecified values, indices in [0, m).  n == 0: MPMHIP_OK. */
int mpmhip_knn_scratch(int32_t n, int32_t m, int32_t dim, int32_t k, int32_t slices, int64_t *out_len);
int mpmhip_knn(int32_t device, void *stream, const float *queries, int32_t n, const float *targets, int32_t m, int32_t dim, int32_t k,
               int32_t slices, uint64_t *scratch, int64_t scratch_len, float *out_dists, int32_t *out_idx);
/* weights_from_k_closest_verts (:187-205) and the gather of transform_to_t_pose (:235-241) in one launch, from the output of
 * mpmhip_knn: w_k = clamp(dists[p, k], 1e-8)^-power / sum_k, out_w[p, :] = sum_k w_k lbs_weights[idx[p, k], :], both sums in ascending
 * k.  lbs_weights [n_verts*n_joints], out_w [n*n_joints]; power >= 0 (the reference uses 2); an index outside [0, n_verts) is clamped.
 * lbs_weights == NULL: out_w [n*k] = the weights w themselves (what weights_from_k_closest_verts returns); idx, n_verts and n_joints
 * are then not used. */
int mpmhip_shepard_weights(int32_t device, void *stream, const float *dists, const int32_t *idx, int32_t n, int32_t k, int32_t power,
                           const float *lbs_weights, int32_t n_verts, int32_t n_joints, float *out_w);
/* Linear-blend skinning.  For frame b and point p: T = sum_j w[p, j] A[b, j] (all 16 entries, ascending j).
 *   mpmhip_skin_to_pose  (transform_to_pose :290-337)    out = (T (v, 1))[:3], then + transl[b], then * scale, each only if given
 *   mpmhip_skin_to_tpose (transform_to_t_pose :262-286)  v' = v / scale - transl[b], out = (T^-1 (v', 1))[:3]; T^-1 is the general
 *                        4 x 4 inverse by cofactors (the last row of T is (0, 0, 0, sum_j w_j), not (0, 0, 0, 1)); a singular T
 *                        gives non-finite output
 * verts [n_points*3], or [n_frames*n_points*3] with verts_batched; w [n_points*n_joints], or one such block per frame with w_batched
 * (the reference's lbs_w.repeat is never needed); A [n_frames*n_joints*16]; transl [n_frames*3] or NULL; scale [1], or [n_frames]
 * with scale_batched, or NULL, on the device.  out_points [n_frames*n_points*3]; out_T [n_frames*n_points*16] (T, or T^-1 on the way
 * to the T-pose, which is what the reference returns) or NULL = not written.  1 <= n_joints <= MPMHIP_SKIN_MAX_JOINTS.
 * n_frames == 0 or n_points == 0: MPMHIP_OK. */
#define MPMHIP_SKIN_MAX_JOINTS 127
int mpmhip_skin_to_pose(int32_t device, void *stream, const float *verts, int32_t verts_batched, const float *w, int32_t w_batched,
                        const float *A, int32_t n_frames, int32_t n_points, int32_t n_joints, const float *transl, const float *scale,
                        int32_t scale_batched, float *out_points, float *out_T);
int mpmhip_skin_to_tpose(int32_t device, void *stream, const float *verts, int32_t verts_batched, const float *w, int32_t w_batched,
                         const float *A, int32_t n_frames, int32_t n_points, int32_t n_joints, const float *transl, const float *scale,
                         int32_t scale_batched, float *out_points, float *out_T);

/* ---- introspection ---------------------------------------------------------------------- */
/* dense reference-layout copies of grid_m [G^3], grid_v_in [G^3*3], grid_v_out [G^3*3] as they
 * stand after the last substep's grid stage ([dev] outputs, any may be NULL).  Synchronous. */
int mpmhip_export_grid(mpmhip_ctx *ctx, float *grid_m, float *grid_v_in, float *grid_v_out);
/* performance experiments only (kernel ablations, MPMHIP_DBG bit mask of csrc/fast_device.hpp; most bits make the results wrong).
 * The kernel switches exist only in -DMPMHIP_DEBUG=1 builds; the production build accepts bit 64 (host-side) alone. */
int mpmhip_set_debug_flags(mpmhip_ctx *ctx, int32_t flags);
int mpmhip_debug_counter(mpmhip_ctx *ctx, int32_t index, int64_t *out); /* device-side experiment counters, synchronous */
/* per-workgroup timeline of the newest p2g (kernel 0) / g2p (kernel 1) launch: out[wg * 8 + slot] in ticks of the 100 MHz
 * constant clock, slot 7 = (XCC_ID << 32) | HW_ID.  out == NULL starts recording.  Only libraries built with
 * -DMPMHIP_DEBUG=1 carry the stamps (and the kernel switches of mpmhip_set_debug_flags); the production build returns
 * MPMHIP_ERR_INVALID.  tools/gpu/wgtrace.py. */
int mpmhip_debug_wgtrace(mpmhip_ctx *ctx, int32_t kernel, uint64_t *out, int32_t max_wg);
/* the sort of the re-sort on its own (tests/test_gpu_sort.py): stable sort of n 32-bit keys by their low `bits` bits
 * ([dev] keys_in; bits above `bits` must be zero) -> [dev] keys_out (sorted), order_out (source index of each sorted key).
 * Uses the path the context's re-sorts use (csrc/resort.hip k_rs_*; rocPRIM with MPMHIP_SORT=rocprim or n > 2^21).
 * Synchronous; fast mode only. */
int mpmhip_debug_sort(mpmhip_ctx *ctx, const uint32_t *keys_in, int32_t n, int32_t bits, uint32_t *keys_out, int32_t *order_out);
/* counts for the algorithmic-bytes formula; synchronous, runs small count kernels */
int mpmhip_get_stats(mpmhip_ctx *ctx, mpmhip_stats *out);
/* MPMWARP.time_profile / print_time_profile, mpm_solver.py:16,538-541: when enabled every phase is
 * bracketed by hipEvents (forces a sync per substep, like ScopedTimer(synchronize=True)).
 * on = 1: every reference phase is its own launch (the reference's keys; un-fused kernels);
 * on = 2: event pairs around the launches of the production loop -- the same (fused) kernels an unprofiled run
 *         executes, keys compute_stress_from_F_trial / p2g / g2p_v / rebin (what bench.py's roofline uses);
 * on = 0: off (no events, no syncs). */
int mpmhip_profile_enable(mpmhip_ctx *ctx, int32_t on);
int mpmhip_profile_count(const mpmhip_ctx *ctx);
/* i-th phase: name, accumulated milliseconds, number of samples */
int mpmhip_profile_get(const mpmhip_ctx *ctx, int32_t i, const char **name, double *total_ms,
                       int64_t *samples);
/* on = 2 only: the i-th phase's launch timed by its OWN start / stop timestamps (the kernel duration a profiler's kernel trace
 * reports), without what the event bracket adds around it; samples = 0 for phases that are not a single hot launch.
 * (No reference counterpart: the reference's ScopedTimer only has the synchronised wall time, mpm_solver.py:16.) */
int mpmhip_profile_get_kernel(const mpmhip_ctx *ctx, int32_t i, double *kernel_ms, int64_t *samples);
int mpmhip_profile_reset(mpmhip_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MPMHIP_H */
