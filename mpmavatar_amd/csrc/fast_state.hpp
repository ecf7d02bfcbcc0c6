// fast_state.hpp -- host-side state of the fast back end (FastState and what hangs on it) and the functions its translation
// units share.
#pragma once
#include "g2p_device.hpp"

namespace mpm {

// ================================================================================================
// host side
// ================================================================================================
// Pinned host scratch (FastState::h_pin): where the read-backs behind the host's waits land.  One name per slot; a block is
// [first, first + its _N).  The slots are laid out one after the other, so no two can share a word; the assert keeps that true
// if one is ever placed by hand.
constexpr int PIN_STATS_N = CNT_STATS_N, PIN_RCNT_N = RC_N, PIN_MASS_N = 3;
enum {
  PIN_STATS = 0,                         // fast_stats: the first CNT_STATS_N device counters
  PIN_ADJ_K = PIN_STATS + PIN_STATS_N,   // do_import: width of the vertex adjacency
  PIN_DIST_DRIFT,                        // fast_dist_drift_flag: this rank's CNT_DRIFT
  PIN_LINK_VOTE,                         // rccl_link_setup: CNT_LINK_VOTE_ALL
  PIN_LINK_TIMEOUT,                      // fast_rccl_steps: CNT_LINK_TIMEOUT
  PIN_HALO_MULTI,                        // rccl_rebin: a block shared with more than one peer (no fused halo)
  PIN_BODY_MOVES,                        // fast_body_at_rest_begin: CNT_BODY_MOVES
  PIN_RCNT,                              // rebin, compact_shared_blocks: the counts of the re-sort (RC_*)
  PIN_MASS = PIN_RCNT + PIN_RCNT_N,      // rebin: CNT_MMIN, CNT_MMAX, CNT_NSEL
  PIN_N = PIN_MASS + PIN_MASS_N
};
static_assert(PIN_STATS + PIN_STATS_N <= PIN_ADJ_K && PIN_ADJ_K < PIN_DIST_DRIFT &&
              PIN_BODY_MOVES < PIN_RCNT && PIN_RCNT + PIN_RCNT_N <= PIN_MASS && PIN_MASS + PIN_MASS_N <= PIN_N,
              "blocks of the pinned scratch overlap");

// The grid accumulators and everything the host knows about their contents.  There are two buffers (three for scenes that can run
// the fused g2p -> p2g launch, k_g2p2g: read / write / clear); GridPtrs' {mv, col, mov, m_flag, col_flag} point at the current one.
// A fused substep leaves the accumulators of the active blocks LOADED (g2p only read them): the next substep scatters into the
// other buffer and clears the loaded one with extra workgroups of its own launches (the ZeroArgs handed out here), and whoever
// is about to change the active list clears first.
// A body AT REST inside one mpmhip_steps call (mesh_v == 0 for every vertex: checked once per call, fast_body_at_rest_begin): its
// collider field -- weight, weight * velocity, weight * normal per node -- is the same in every substep, so it is splatted ONCE into
// each of the two buffers and then KEPT: no splat workgroups, no clearing of the collider channels, until the particle order (the
// face bins, the active list) changes, the body may move again, or the call ends (invalidate_kept_fields).
// All of that state is private: callers say what happens to the buffers, and the active list the clearing runs over can only be
// replaced through begin_relist(), which drops the kept fields and hands back the pending clearing first.
class AccumRing {
 public:
  // begin_relist()'s receipt: the clearing the caller's next launch has to carry, and the only key to end_relist()
  class Relist {
    friend class AccumRing;
    explicit Relist(const ZeroArgs &z_) : z(z_) {}
   public:
    const ZeroArgs z;
  };
  int allocate(mpmhip_ctx *c, GridPtrs *g, size_t nblocks, bool three);
  // (weight: channel 0 of buffer 0, for the context's bookkeeping)
  int add_collider_channels(mpmhip_ctx *c, float **weight) { return add_channels(c, col, GCH_COL, weight); }
  int add_mover_channels(mpmhip_ctx *c, float **weight) { return add_channels(c, mov, GCH_MOV, weight); }
  int n_buffers() const { return nbuf; }
  bool loaded() const { return is_loaded; }  // the current buffer holds the last fused substep's accumulators
  bool body_at_rest() const { return at_rest; }
  void set_body_at_rest(bool r) { at_rest = r; }
  // Head of a substep: the clearing its launches carry for what the last one left loaded.  With something to clear the ring
  // advances to the other buffer; clear_now (one launch per phase: profiling) clears with a launch of its own and stays instead.
  ZeroArgs begin_substep(hipStream_t s, bool clear_now);
  // Head of a substep whose launch also runs the deferred g2p of the last one (k_g2p2g): that reads the current buffer, p2g
  // scatters into the next, and the clearing handed back is of the buffer the fused launch BEFORE this one read.
  ZeroArgs begin_fused_substep();
  void clear_fused_read(hipStream_t s);  // the sequence of fused launches ends: clear what the last one read now
  // This substep has a collider field.  true: the current buffer already holds the field of the body at rest, no splat
  // workgroups.  Otherwise the launch splats it; `keep` (the body is at rest and the run may keep fields) keeps it from now on.
  bool collider_substep(bool keep);
  void mark_loaded(int has_col, int has_mov);  // a fused substep has been issued into the current buffer
  // kept collider fields are no longer valid: clear them now, over the active list as it stands
  void invalidate_kept_fields(hipStream_t s);
  // The active list (or the face bins) is about to change: kept fields are dropped and the pending clearing of the old list
  // is handed back; end_relist() installs the new list.
  Relist begin_relist(hipStream_t s);
  void end_relist(const Relist &, const int *alist, int n_A) { list = alist; n_list = n_A; }

 private:
  enum ColField { COL_CLEAN, COL_SPLAT, COL_KEPT };  // SPLAT: this substep's, cleared by the next launch's clearing workgroups as ever
  int clear_wgs() const { return (n_list + PT / 64 - 1) / (PT / 64); }
  ZeroArgs zero_args(int k, int has_col, int has_mov) const;
  ZeroArgs take_loaded();
  int add_channels(mpmhip_ctx *c, float *(&ch)[3], int per_block, float **weight);
  void point_at(int k);
  GridPtrs *g = nullptr;
  size_t nblocks = 0;
  float *mv[3] = {nullptr, nullptr, nullptr}, *col[3] = {nullptr, nullptr, nullptr}, *mov[3] = {nullptr, nullptr, nullptr};
  int *mflag[3] = {nullptr, nullptr, nullptr}, *cflag[3] = {nullptr, nullptr, nullptr};
  int *zero_flags = nullptr;  // [blocks] zeros: stands in for the mass flags where only the collider channels are cleared
  int nbuf = 2, cur = 0;
  const int *list = nullptr;  // the active list the contents of the buffers live on
  int n_list = 0;
  bool is_loaded = false;
  int loaded_col = 0, loaded_mov = 0;  // ... with collider / mover channels
  bool at_rest = false;                // this mpmhip_steps call's body does not move
  ColField col_field[3] = {COL_CLEAN, COL_CLEAN, COL_CLEAN};
  int fused_read = -1, fused_col = 0, fused_mov = 0;  // buffer the last fused launch read: cleared by the next one (or clear_fused_read)
};

struct ResortState;
struct DistState;

struct FastState {
  // ---- multi-GPU: the state of the exchange -- communicator, peer list, links, sequence numbers, the collective re-sort's
  // bookkeeping -- is DistState, defined and owned by dist.hip (dist_alloc / dist_free below).  Four things stay here:
  DistState *ds = nullptr;
  bool dist = false;              // the policy switch the substep and the re-sort read: re-sorts only on request (all ranks re-sort
                                  // together), no kept collider fields, no G2P2G, no split splat
  bool ghost_g2p = false;         // read by the re-sort (k_keys: which copies go on the g2p list): ghost copies (selection == 2)
                                  // gather for themselves
  float global_mass_span = 0.0f;  // read by the re-sort's tile decision: the span over ALL ranks' simulated particles
                                  // (mpmhip_dist_set_mass_span); 0: not set
  // (and g.halo below, a device argument: the launcher of g2p picks the kernel by its slot table)
  Dims d{};
  bool g2p_two_pass = false;   // k_g2p<., true, .>: see there (default: scenes without traditional particles)
  bool p2g_fixed = true;       // p2g's chunk tile in packed fixed point (k_p2g<.., FX = true>); MPMHIP_P2G_TILE=f64: the fp64 tile
  bool p2g_fixed_forced = false;  // ... whatever the mass span (MPMHIP_P2G_TILE=fx)
  int blk_bits = 0, key_bits = 0;  // blk_bits: packed key format kf (field widths) as the kernels take it
  int blk_bits_plain = 0;          // bits of a block id (face-bin sort)
  float lead_steps = 12.0f;        // predictive sort: look this many substeps ahead (half the expected re-sort interval)
  float last_dt = 0.0f;
  int true_since_rebin = 0;        // substeps since the last re-sort (steps_since_rebin is overwritten to force one)
  size_t nblocks = 0;
  F3 *eforce = nullptr;  // [3][n_e] + zero slot
  VAdj va() const { return VAdj{adj_s, eforce, adj_K, d.n_v, d.n_e}; }
  // ---- what a re-sort leaves for the substep: written by resort.hip (do_import, rebin), read by everyone.  What only the re-sort
  // itself touches -- sort buffers, block flags, tables and their capacities, face sort, original-index adjacency -- is ResortState
  ResortState *rs = nullptr;
  Bufs buf[2]{};  // the particles in sorted order; the re-sort gathers from buf[cur] into the other and flips cur
  int cur = 0;
  int *perm[2] = {nullptr, nullptr}, *inv = nullptr;   // sorted slot -> caller's index (of buf[i]) and back
  SortKey *keys[2] = {nullptr, nullptr};               // keys[1]: the sorted keys
  int *face_slot = nullptr, *adj_s = nullptr;          // cloth topology in sorted slots: [3][n_e] corners, [adj_K][n_v] (element, corner) of a vertex
  int adj_K = 0;
  int *alist = nullptr, *ab_flag = nullptr;            // active blocks: the list and [nblocks] flags
  int n_P = 0, n_A = 0;                                // particle blocks, active blocks
  ChunkRec *chunks = nullptr, *chunks_g = nullptr;     // p2g list, g2p list (= p2g list unless there are ghost copies)
  int n_chunks = 0, n_chunks_g = 0;
  FaceBin *fbins = nullptr;                            // body-face bins (collider gather) on the active list
  int *fidx = nullptr;                                 // [n_f][3] face vertex ids in bin order
  int n_fbins = 0;
  bool face_flag_seen = false;    // some ring entry since the last face sort had the face bit set (poll_drift_flags; the face sort clears it)
  // the mass span of the import, read back by the next re-sort: decides the chunk tile of p2g (read_mass_span, resort.hip)
  bool mass_span_pending = false, p2g_fixed_now = true;
  float mass_span = 1.0f;
  bool all_simulated = false;     // no particle with selection != 0 (counted at every import with the mass span)
  // ---- (end of the re-sort's block)
  bool sort_rocprim = false;   // MPMHIP_SORT=rocprim: the library's sort instead (same permutation)
  GridPtrs g{};
  int64_t stat_steps = 0;
  int *h_pin = nullptr;  // pinned host scratch, PIN_N ints (PIN_*)
  bool elem_pending = false;  // element finalise of the last substep still to be done (fused into the next stress)
  int steps_since_rebin = 0;
  volatile int *h_sig = nullptr;  // pinned, host-mapped, written by the kernels (GridPtrs::host_sig)
  unsigned sig_seq = 0;           // step_id of the last p2g launch issued (wraps)
  unsigned sig_at_rebin = 0;      // sig_seq when the last re-sort finished: ring entries up to it speak about the old order
  int host_lead = 6;              // substeps the host may run ahead of the GPU (MPMHIP_HOST_LEAD)
  bool have_order = false;
  int64_t rebins = 0;
  int rebin_interval = 32;
  bool adaptive_rebin = true;
  // fused grid stage (no grid kernel: g2p evaluates the nodes, the accumulators stay loaded, see AccumRing); fused stress of
  // the traditional particles (in front of p2g)
  bool fuse_grid = true, fuse_trad = true;
  AccumRing acc;
  int64_t n_col_kept = 0;        // substeps that ran without splat workgroups because the field was kept (statistics)
  bool col_keep = true;        // MPMHIP_COL_KEEP=0: splat the body every substep whether it moves or not (A/B)
  bool g2p2g = true;           // MPMHIP_G2P2G=0: two launches per substep for traditional-only scenes as before
  int g2p2g_max_chunks = 512;  // MPMHIP_G2P2G_MAX
  int stagger_auto = 2;        // p2g first-round stagger units for chunk lists of at least two rounds; -1: forced by MPMHIP_P2G_STAGGER
  int split_splat_max_chunks = 1024;  // MPMHIP_SPLIT_SPLAT_MAX
  bool split_splat = true;     // body-face splat: pass 0 in the stress launch, pass 1 in the p2g launch (MPMHIP_SPLIT_SPLAT=0: both in p2g)
  int64_t n_g2p2g = 0;         // fused launches so far (mpmhip_stats)
  // G2P2G: the g2p of the last substep has not been launched yet -- the next substep's launch does it in front of its own p2g
  // (k_g2p2g), or flush_g2p() does with a plain k_g2p when anything else needs the particles first
  bool g2p_pending = false;
  GridParams pend_gp{};
  BCList pend_bcl{};
  float pend_dt = 0.0f;
  GridParams last_gp{};  // grid-stage parameters of the last fused substep (materialize_grid)
  BCList last_bcl{};
  std::vector<void *> allocs;
};

template <class T>
int dalloc(mpmhip_ctx *c, T **p, size_t count, bool zero = true) {
  size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
  MPM_HIP_CHECK(c, hipMalloc((void **)p, bytes));
  c->fast->allocs.push_back((void *)*p);
  if (zero) MPM_HIP_CHECK(c, hipMemsetAsync(*p, 0, bytes, c->stream));
  return MPMHIP_OK;
}

#ifndef P2G_STEPS
#define P2G_STEPS 3  // DPP scan steps of the fixed-point instantiations (experiment switch)
#endif
// the hot launches: in prof_fused mode they carry the context's kernel-stamp events (ctx.hpp kev0 / kev1); otherwise a plain launch
template <class K, class... A>
inline void kstamp_launch(mpmhip_ctx *c, K kernel, unsigned grid, unsigned block, A &&...args) {
  if (c->prof_fused) {
    hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, c->stream, c->kev0, c->kev1, 0, args...);
    c->kev_pending = true;
  } else {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, c->stream, args...);
  }
}

// ---- functions shared by the translation units of the fast back end ------------------------------------------------------
// resort.hip
int alloc_bufs(mpmhip_ctx *c, Bufs &b);
int resort_alloc(mpmhip_ctx *c);                  // ResortState and the buffers of FastState's re-sort block (fast_init)
int resort_alloc_face_sort(mpmhip_ctx *c, int nf);  // ... the arrays of the body-face sort (first mesh collider)
void resort_free(FastState *f);                     // (device memory goes with FastState::allocs)
int do_import(mpmhip_ctx *c);
int rebin(mpmhip_ctx *c);
int compact_shared_blocks(mpmhip_ctx *c, const int *flag, int n, int *index, int *list, int cap, int *total);
// dist.hip: all that fast.hip asks of the multi-GPU side
int dist_alloc(mpmhip_ctx *c);     // DistState and the pack counter (fast_init); reads MPMHIP_DIST_FUSED_HALO and MPMHIP_DIST_HALO
void dist_free(FastState *f);      // peer links, link arenas, communicator, DistState: BEFORE the sweep of FastState::allocs
bool dist_fused_halo_now(const mpmhip_ctx *c);  // the fused halo is in force for this substep: no pack / add kernels
// What of the halo rides in this p2g launch: the pack table and pk.n_wg (0: nothing).  Once the launch is laid out, the second call
// sets count / done / target and advances the running target by the workgroups that scatter.
void dist_pack_riders(mpmhip_ctx *c, PackArgs &pk);
void dist_pack_placed(mpmhip_ctx *c, const LaunchLayout &lay, PackArgs &pk);
// fast.hip
int flush_elements(mpmhip_ctx *c);
int flush_g2p(mpmhip_ctx *c);  // launches the deferred g2p of a G2P2G sequence
void launch_zero_blocks(hipStream_t s, const ZeroArgs &z);
void materialize_grid(mpmhip_ctx *c, bool count);
int step_phase_a(mpmhip_ctx *c, const StepArgs &a);
int step_phase_b(mpmhip_ctx *c, const StepArgs &a);
int step_phase_c(mpmhip_ctx *c, const StepArgs &a);
// p2g.hip / g2p.hip: the only places that name the template instantiations of the substep's kernels
void launch_p2g(mpmhip_ctx *c, bool trad, bool jt, unsigned grid, int n_chunks, float dt, const SplatArgs &sa, const TradParams &tp);
void launch_stress_elem(mpmhip_ctx *c, int mode, const SplatArgs &sa);
void launch_stress_trad(mpmhip_ctx *c, float dt);
void launch_g2p(mpmhip_ctx *c, bool fused, bool two, float dt, const GridParams &gp, const BCList &bcl);
void launch_g2p2g(mpmhip_ctx *c, unsigned grid, float dt, const GridRead &rd, const SplatArgs &sa, const TradParams &tp, const GridParams &gp,
                  const BCList &bcl);

}  // namespace mpm
