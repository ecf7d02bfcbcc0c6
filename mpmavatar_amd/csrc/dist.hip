// dist.hip -- multi-GPU: halo / ghost kernels, peer links (HIP IPC), the RCCL binding and the in-library sharded loop.
// (shared device code: fast_device.hpp; the per-peer tables the kernels take and their builders: halo_tables.hpp)
// The state of all this is DistState, below: defined here, allocated and freed here (dist_alloc / dist_free), and FastState holds a
// pointer to it that no other translation unit looks behind.  fast.hip asks three things of it, by name (fast_state.hpp): alloc / free,
// "is the fused halo in force for this substep?", and "what of the halo rides in this p2g launch?".
#include "fast_state.hpp"

namespace mpm {

struct Rccl {  // entry points resolved with dlsym: libmpmhip.so itself does not link librccl
  void *h = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  bool load(std::string &err) {
    if (h) return true;
    // MPMHIP_RCCL_LIB: another library with the same ten entry points (tests/mock_rccl: shared-memory stand-in that lets
    // 2-3 ranks share the one GPU of a test box, which RCCL itself refuses)
    const char *over = getenv("MPMHIP_RCCL_LIB");
    if (over && *over) {
      h = dlopen(over, RTLD_NOW | RTLD_LOCAL);
      if (!h) { err = std::string("dlopen MPMHIP_RCCL_LIB=") + over + ": " + dlerror(); return false; }
      // never silently: the collective library of a production run must be RCCL
      fprintf(stderr, "[mpmhip] WARNING: MPMHIP_RCCL_LIB is set -- the multi-GPU exchange uses %s INSTEAD OF librccl.so (test hook)\n", over);
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) { err = std::string("dlopen librccl.so.1: ") + dlerror(); return false; }
    auto sym = [&](const char *n) { void *p = dlsym(h, n); if (!p) err = std::string("dlsym ") + n; return p; };
    *(void **)&GetUniqueId = sym("ncclGetUniqueId"); *(void **)&CommInitRank = sym("ncclCommInitRank");
    *(void **)&CommDestroy = sym("ncclCommDestroy"); *(void **)&GroupStart = sym("ncclGroupStart");
    *(void **)&GroupEnd = sym("ncclGroupEnd"); *(void **)&Send = sym("ncclSend"); *(void **)&Recv = sym("ncclRecv");
    *(void **)&AllGather = sym("ncclAllGather"); *(void **)&GetErrorString = sym("ncclGetErrorString");
    *(void **)&AllReduce = sym("ncclAllReduce");
    return GetUniqueId && CommInitRank && CommDestroy && GroupStart && GroupEnd && Send && Recv && AllGather && AllReduce &&
           GetErrorString;
  }
};

// One neighbour rank: the record the launches and the exchange read (DistPeer: shared blocks, halo and ghost buffers, the link) plus
// what only the in-library loop keeps of it, all buffers owned here.  A peer that came through the ABI (mpmhip_dist_set_peers: the
// Python-driven transport) is the DistPeer part alone: no rank, no link, nothing owned.
struct RcclPeer : DistPeer {
  RcclPeer() = default;
  explicit RcclPeer(const mpmhip_dist_peer &p) : DistPeer(p) {}
  int rank = -1;
  int *flag = nullptr, *index = nullptr;  // [nblocks] shared with this rank / position in blocks[] (per collective re-sort)
  int cap_blocks = 0;                     // capacity of blocks[], halo_send, halo_recv
  unsigned char *hbuf = nullptr;          // device staging of the two IPC handles (mine at 0, theirs at 128)
  // (the ABI's record points at its lists as const; the loop's own blocks[] is an allocation of this file, which the re-sort fills)
  int *own_blocks() const { return const_cast<int *>(blocks); }
};

struct DistState {
  Rccl rccl;
  // THE peer list, of either transport: filled by mpmhip_rccl_set_ghosts + every collective re-sort (in-library loop) or replaced by
  // mpmhip_dist_set_peers (Python-driven).  The tables are built from it and the exchange walks it: one list, nothing to keep paired.
  std::vector<RcclPeer> peers;
  unsigned char *map_all = nullptr;  // [world][nblocks] active-block byte maps
  StepArgs dist_args{};              // the substep in flight (phase 0 stores them for phases 1 and 2)
  bool link_want = true, link_decided = false, link_on = false;  // peer-mapped halos: asked for / decided collectively / in use
  // fused halo (peer-mapped halos only): pack workgroups ride in the p2g launch, g2p adds the neighbour's share while it
  // stages its tile (PackArgs, HaloIn) -- no pack / add kernels in the substep.  Decided per collective re-sort (local decision:
  // what goes over the links is the same either way).  MPMHIP_DIST_FUSED_HALO=0: keep the two kernels.
  bool fused_want = true, fused_halo = false;
  int *halo_slot = nullptr, *halo_multi = nullptr;
  unsigned *pack_done = nullptr, pack_target = 0;
  int64_t fused_halo_steps = 0;  // substeps that ran without pack / add kernels (mpmhip_dist_fused_halo_steps)
  unsigned halo_seq = 0;         // substeps exchanged so far (+ handshake rounds): flag value and buffer parity (wraps: the
                                 // kernels compare (int)(flag - seq), long trainings run billions of substeps)
  bool dist_keep_cur = false;    // re-sort inside mpmhip_rccl_steps: the caller's mesh pointers are valid
  // adaptive collective re-sorts (mpmhip_rccl_steps with rebin_interval <= 0): the ranks' drift flags are max-reduced
  // every DIST_POLL substeps and read DIST_LAG substeps later, so every rank takes the same decision at the same substep
  int dist_since = 0;
  bool dist_resort = false, dflag_in_flight = false, rccl_sorted = false;
  int64_t dflag_check_at = 0;
  unsigned dflag_seq = 0;  // sequence number of the last reduction posted to host memory (k_post_flag; wraps)
};

namespace {

__global__ void k_link_ping(unsigned *data, int n, int *cnt, int *flag, int seq) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) data[i] = link_pattern(seq, i);
  link_signal(cnt, gridDim.x, flag, seq);
}

__global__ void k_link_check(const unsigned *data, int n, const int *flag, int seq, int *counters) {
  link_wait(flag, seq, counters + CNT_LINK_TIMEOUT, LINK_HANDSHAKE_TICKS);
  int bad = 0;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) bad += data[i] != link_pattern(seq, i);
  if (bad) atomicAdd(counters + CNT_LINK_BAD, bad);
}


// the all-reduced drift flag of the sharded loop -> pinned host memory: value first, then its sequence number
__global__ void k_post_flag(const int *value, int *host_sig, int seq) {
  __hip_atomic_store(host_sig + SIG_DFLAG, *value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __threadfence_system();
  __hip_atomic_store(host_sig + SIG_DSEQ, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ void k_link_verdict(int *counters) { counters[CNT_LINK_VOTE] = (counters[CNT_LINK_TIMEOUT] != 0 || counters[CNT_LINK_BAD] != 0) ? 1 : 0; }


__global__ void k_halo_pack(HaloTab tb, GridPtrs g) { halo_pack_wg<false>(tb, g, (int)blockIdx.x); }

// a block can be shared with more than one peer (slabs thinner than two blocks): atomic adds
__global__ void k_halo_add(HaloTab tb, GridPtrs g) {
  int p = tab_peer(tb, blockIdx.x);
  int t = ((int)blockIdx.x - tb.wg_off[p]) * blockDim.x + threadIdx.x;
  int CH = tb.with_mov ? 8 : 4;
  if (tb.sig[p]) link_wait(tb.sig[p], tb.seq, g.counters + CNT_LINK_TIMEOUT);
  if (t >= tb.n_blocks[p] * CH * 64) return;
  int l = t & 63, ch = (t >> 6) % CH, i = t / (CH * 64);
  int blk = tb.blocks[p][i];
  float v = tb.buf[p][t];
  if (v == 0.0f) return;
  if (ch < 4) { atomicAdd(g.mv + ((size_t)blk * GCH_MV + ch) * 64 + l, v); g.m_flag[blk] = 1; }
  else atomicAdd(g.mov + ((size_t)blk * GCH_MOV + (ch - 4)) * 64 + l, v);
}

// ghosts: x, v of vertices / traditional particles (6 floats) and the director d3 of elements (3 floats);
// ids are the caller-order particle indices of this rank's solver, inv[] maps them to sorted slots
__global__ void k_ghost_pack(GhostTab tb, const int *inv, Bufs b) {
  int p = tab_peer(tb, blockIdx.x);
  int t = ((int)blockIdx.x - tb.wg_off[p]) * blockDim.x + threadIdx.x;
  int n_p_ids = tb.n_p[p], n_e_ids = tb.n_e[p];
  float *out = tb.buf[p];
  if (t < n_p_ids) {
    int s = inv[tb.ids_p[p][t]];
    V3 x = ld3(b.all, A_X, s), v = ld3(b.all, A_V, s);
    float *o = out + 6 * (size_t)t;
    o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = v.x; o[4] = v.y; o[5] = v.z;
  } else if (t < n_p_ids + n_e_ids) {
    int i = t - n_p_ids, s = inv[tb.ids_e[p][i]];
    float *o = out + 6 * (size_t)n_p_ids + 3 * (size_t)i;
    o[0] = b.el.at(E_D + 2, s); o[1] = b.el.at(E_D + 5, s); o[2] = b.el.at(E_D + 8, s);
  }
}

__global__ void k_ghost_unpack(GhostTab tb, const int *inv, Bufs b) {
  int p = tab_peer(tb, blockIdx.x);
  int t = ((int)blockIdx.x - tb.wg_off[p]) * blockDim.x + threadIdx.x;
  int n_p_ids = tb.n_p[p], n_e_ids = tb.n_e[p];
  const float *in = tb.buf[p];
  if (t < n_p_ids) {
    int s = inv[tb.ids_p[p][t]];
    const float *o = in + 6 * (size_t)t;
    st3(b.all, A_X, s, v3(o[0], o[1], o[2]));
    st3(b.all, A_V, s, v3(o[3], o[4], o[5]));
  } else if (t < n_p_ids + n_e_ids) {
    int i = t - n_p_ids, s = inv[tb.ids_e[p][i]];
    const float *o = in + 6 * (size_t)n_p_ids + 3 * (size_t)i;
    b.el.at(E_D + 2, s) = o[0]; b.el.at(E_D + 5, s) = o[1]; b.el.at(E_D + 8, s) = o[2];
  }
}

// halo_slot[b] = (peer << 24) | index of block b in that peer's shared-block list; *multi = 1 if a block is shared with
// more than one peer (slabs thinner than two blocks: those intervals keep the separate add kernel with its atomics)
__global__ void k_halo_slots(const int *flag, const int *index, int n, int peer, int *slot, int *multi) {
  int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n || !flag[b]) return;
  if (slot[b] != -1) *multi = 1;
  else slot[b] = (peer << 24) | index[b];
}

__global__ void k_shared_flags(const unsigned char *a, const unsigned char *b, int n, int *flag) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = (a[i] && b[i]) ? 1 : 0;
}

__global__ void k_flags_to_bytes(const int *flag, int n, unsigned char *out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = flag[i] ? 1 : 0;
}

}  // namespace


// ---- DistState's lifetime and what fast.hip asks of it (fast_state.hpp) --------------------------------------
int dist_alloc(mpmhip_ctx *c) {
  FastState *f = c->fast;
  DistState *ds = f->ds = new DistState();
  if (const char *e = getenv("MPMHIP_DIST_FUSED_HALO")) ds->fused_want = atoi(e) != 0;
  const char *hm = getenv("MPMHIP_DIST_HALO");  // "rccl": keep the halos on ncclSend/ncclRecv; default: peer-mapped buffers
  ds->link_want = !(hm && !strcmp(hm, "rccl"));
  return dalloc(c, &ds->pack_done, (size_t)DONE_SHARDS * DONE_STRIDE);
}
void dist_free(FastState *f) {
  DistState *ds = f->ds;
  if (!ds) return;
  for (auto &p : ds->peers) {
    if (p.link_remote) (void)hipIpcCloseMemHandle(p.link_remote);
    if (p.link_local) (void)hipFree(p.link_local);
  }
  if (ds->rccl.comm) (void)ds->rccl.CommDestroy(ds->rccl.comm);
  delete ds;
  f->ds = nullptr;
}
bool dist_fused_halo_now(const mpmhip_ctx *c) {
  return c->fast->dist && c->fast->ds->fused_halo && !c->profiling && !c->prof_fused;
}
// (the fused halo is decided only where every peer that shares blocks is linked and all fit one table, rccl_rebin: the send table
// addresses the neighbours' arenas alone)
void dist_pack_riders(mpmhip_ctx *c, PackArgs &pk) {
  if (!dist_fused_halo_now(c)) return;
  const DistState *ds = c->fast->ds;
  pk.tb = halo_tab(ds->peers.data(), ds->peers.size(), 0, true, !c->movers.empty(), ds->halo_seq, ds->link_on);
  pk.n_wg = pk.tb.wg_off[pk.tb.n];
}
void dist_pack_placed(mpmhip_ctx *c, const LaunchLayout &lay, PackArgs &pk) {
  if (!dist_fused_halo_now(c)) return;
  DistState *ds = c->fast->ds;
  pk.count = 1;
  pk.done = ds->pack_done;
  ds->pack_target += (unsigned)lay.n_scatter();
  pk.target = ds->pack_target;
}

// ---- multi-GPU entry points --------------------------------------------------------------------------------
// a context becomes one rank of a sharded run (either transport): the drift look-ahead gets its multi-GPU default
static void enter_dist_mode(FastState *f) {
  f->dist = true;
  if (!getenv("MPMHIP_DRIFT_LOOKAHEAD")) f->g.lookahead = DRIFT_LOOKAHEAD_DIST;
}
int fast_dist_enable(mpmhip_ctx *c) {
  enter_dist_mode(c->fast);
  return MPMHIP_OK;
}
int fast_dist_set_ghost_mode(mpmhip_ctx *c, int ghosts_gather) {
  c->fast->ghost_g2p = ghosts_gather != 0;
  c->fast->steps_since_rebin = 1 << 30;
  return MPMHIP_OK;
}
// the mass span of the whole sharded scene (all ranks): see mpmhip_dist_set_mass_span
int fast_dist_set_mass_span(mpmhip_ctx *c, float min_mass, float max_mass) {
  FastState *f = c->fast;
  f->global_mass_span = min_mass > 0.0f ? max_mass / min_mass : 0.0f;
  // (an import whose own span has already been read decides again; a pending one decides in rebin with the value just stored)
  if (!f->mass_span_pending)
    f->p2g_fixed_now = f->p2g_fixed && (f->p2g_fixed_forced || std::max(f->mass_span, f->global_mass_span) <= 1.0e5f);
  return MPMHIP_OK;
}
int fast_dist_num_blocks(const mpmhip_ctx *c) { return (int)c->fast->nblocks; }
int64_t fast_dist_halo_bytes(const mpmhip_ctx *c) {  // bytes this rank sends per substep in the halo exchange (all peers)
  int CH = halo_channels(!c->movers.empty());
  int64_t n = 0;
  for (auto &p : c->fast->ds->peers) n += (int64_t)(halo_floats(p.n_blocks, CH) * sizeof(float));
  return n;
}

int fast_dist_rebin(mpmhip_ctx *c, unsigned char *active_map) {
  FastState *f = c->fast;
  int rc;
  if (!c->st_bound || !c->md_bound) return fail(c, MPMHIP_ERR_STATE, "dist_rebin: state/model not bound");
  if (c->caller_dirty && (rc = do_import(c))) return rc;
  // between substeps the caller's mesh tensors may be gone: bin the body faces from the context's own copy
  if (!f->ds->dist_keep_cur) set_body_view(c, nullptr, nullptr, 0.0f);
  if ((rc = rebin(c))) return rc;
  if (active_map)
    hipLaunchKernelGGL(k_flags_to_bytes, nblk(f->nblocks), TPB, 0, c->stream, f->ab_flag, (int)f->nblocks, active_map);
  return MPMHIP_OK;
}

int fast_dist_set_peers(mpmhip_ctx *c, int n, const mpmhip_dist_peer *peers) {
  FastState *f = c->fast;
  if (n < 0 || n > 64 || (n > 0 && !peers)) return fail(c, MPMHIP_ERR_INVALID, "dist_set_peers: bad peer list");
  f->ds->peers.clear();
  for (int i = 0; i < n; ++i) f->ds->peers.push_back(RcclPeer(peers[i]));
  return MPMHIP_OK;
}

// halo (send = true: pack into halo_send, false: add halo_recv) for all peers, PEER_TAB per launch
static void launch_halo(mpmhip_ctx *c, bool send) {
  FastState *f = c->fast;
  const DistState *ds = f->ds;
  for (size_t i0 = 0; i0 < ds->peers.size(); i0 += PEER_TAB) {
    const HaloTab tb = halo_tab(ds->peers.data(), ds->peers.size(), i0, send, !c->movers.empty(), ds->halo_seq, ds->link_on);
    if (!tb.n) continue;
    if (send) hipLaunchKernelGGL(k_halo_pack, (unsigned)tb.wg_off[tb.n], TPB, 0, c->stream, tb, f->g);
    else hipLaunchKernelGGL(k_halo_add, (unsigned)tb.wg_off[tb.n], TPB, 0, c->stream, tb, f->g);
  }
}
static void launch_ghosts(mpmhip_ctx *c, bool send) {
  FastState *f = c->fast;
  const DistState *ds = f->ds;
  for (size_t i0 = 0; i0 < ds->peers.size(); i0 += PEER_TAB) {
    const GhostTab tb = ghost_tab(ds->peers.data(), ds->peers.size(), i0, send);
    if (!tb.n) continue;
    if (send) hipLaunchKernelGGL(k_ghost_pack, (unsigned)tb.wg_off[tb.n], TPB, 0, c->stream, tb, f->inv, f->buf[f->cur]);
    else hipLaunchKernelGGL(k_ghost_unpack, (unsigned)tb.wg_off[tb.n], TPB, 0, c->stream, tb, f->inv, f->buf[f->cur]);
  }
}

int fast_dist_phase(mpmhip_ctx *c, int phase, const StepArgs &a) {
  FastState *f = c->fast;
  DistState *ds = f->ds;
  int rc;
  if (phase == 0) {
    ds->dist_args = a;
    if ((rc = step_phase_a(c, a))) return rc;
    if (!dist_fused_halo_now(c)) {     // (else the pack rode in the p2g launch)
      ScopedPhase ph(c, "halo_pack");  // (profiling only) with peer links: the stores into the neighbour's memory + its flag
      launch_halo(c, true);
    }
  } else if (phase == 1) {
    if (!dist_fused_halo_now(c)) {
      ScopedPhase ph(c, "halo_add");   // (profiling only) with peer links: includes the wait for the neighbour's flag
      launch_halo(c, false);
    } else {  // g2p adds the neighbours' shares itself: this substep's receive buffers and flags
      ds->fused_halo_steps += 1;
      f->g.halo = halo_in(ds->peers.data(), ds->peers.size(), ds->halo_slot, !c->movers.empty(), ds->halo_seq);
    }
    rc = step_phase_b(c, ds->dist_args);
    f->g.halo.slot = nullptr;
    if (rc) return rc;
    if (!f->ghost_g2p) launch_ghosts(c, true);
  } else {
    if (!f->ghost_g2p) launch_ghosts(c, false);
    if ((rc = step_phase_c(c, ds->dist_args))) return rc;
  }
  MPM_HIP_CHECK(c, hipGetLastError());
  return MPMHIP_OK;
}
// re-synchronisation of the ghost copies around an exchange (ghost mode 1: at every collective re-sort)
int fast_dist_ghosts(mpmhip_ctx *c, int send) {
  if (!c->fast->have_order) return MPMHIP_OK;  // nothing sorted yet: the copies are still the caller's exact values
  if (!send) flush_elements(c);                // finished elements first: the unpack overwrites their d3
  launch_ghosts(c, send != 0);
  MPM_HIP_CHECK(c, hipGetLastError());
  return MPMHIP_OK;
}

// ---- RCCL transport inside the library ----------------------------------------------------------------------
#define MPM_NCCL_CHECK(c, r, expr)                                                                                \
  do {                                                                                                            \
    ncclResult_t e_ = (expr);                                                                                     \
    if (e_ != ncclSuccess) return fail(c, MPMHIP_ERR_HIP, std::string(#expr) + ": " + (r).GetErrorString(e_));   \
  } while (0)

int fast_rccl_unique_id(char id[128], std::string &err) {
  Rccl r;
  if (!r.load(err)) return MPMHIP_ERR_HIP;
  ncclUniqueId uid;
  ncclResult_t e = r.GetUniqueId(&uid);
  if (e != ncclSuccess) { err = std::string("ncclGetUniqueId: ") + r.GetErrorString(e); return MPMHIP_ERR_HIP; }
  static_assert(sizeof(uid) == 128, "ncclUniqueId size");
  memcpy(id, &uid, 128);
  return MPMHIP_OK;
}

int fast_rccl_init(mpmhip_ctx *c, int rank, int world, const char id[128]) {
  FastState *f = c->fast;
  Rccl &r = f->ds->rccl;
  if (world < 1 || rank < 0 || rank >= world) return fail(c, MPMHIP_ERR_INVALID, "rccl_init: bad rank/world");
  if (!r.load(c->err)) return MPMHIP_ERR_HIP;
  ncclUniqueId uid;
  memcpy(&uid, id, 128);
  MPM_NCCL_CHECK(c, r, r.CommInitRank(&r.comm, world, uid, rank));
  r.rank = rank;
  r.world = world;
  enter_dist_mode(f);
  return dalloc(c, &f->ds->map_all, (size_t)world * f->nblocks);
}

int fast_rccl_set_ghosts(mpmhip_ctx *c, int n, const int32_t *ranks, const int32_t *nsp, const int32_t *const *sp,
                         const int32_t *nrp, const int32_t *const *rp, const int32_t *nse, const int32_t *const *se,
                         const int32_t *nre, const int32_t *const *re) {
  FastState *f = c->fast;
  DistState *ds = f->ds;
  if (!ds->rccl.comm) return fail(c, MPMHIP_ERR_STATE, "rccl_set_ghosts: call mpmhip_rccl_init first");
  // one peer slot per other rank (shared blocks may exist without ghosts, e.g. traditional particles only)
  ds->peers.clear();
  for (int q = 0; q < ds->rccl.world; ++q) {
    if (q == ds->rccl.rank) continue;
    RcclPeer p;
    p.rank = q;
    int rc;
    if ((rc = dalloc(c, &p.flag, f->nblocks))) return rc;
    if ((rc = dalloc(c, &p.index, f->nblocks))) return rc;
    ds->peers.push_back(p);
  }
  auto up = [&](const int32_t **dst, const int32_t *src, int cnt) -> int {
    int *dev = nullptr;
    int rc = dalloc(c, &dev, (size_t)std::max(cnt, 1), false);
    if (rc) return rc;
    if (cnt) MPM_HIP_CHECK(c, hipMemcpy(dev, src, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice));
    *dst = dev;
    return MPMHIP_OK;
  };
  for (int i = 0; i < n; ++i) {
    RcclPeer *p = nullptr;
    for (auto &q : ds->peers) if (q.rank == ranks[i]) p = &q;
    if (!p) return fail(c, MPMHIP_ERR_INVALID, "rccl_set_ghosts: bad peer rank");
    int rc;
    p->n_send_p = nsp[i]; p->n_recv_p = nrp[i]; p->n_send_e = nse[i]; p->n_recv_e = nre[i];
    if ((rc = up(&p->send_p, sp[i], nsp[i])) || (rc = up(&p->recv_p, rp[i], nrp[i])) || (rc = up(&p->send_e, se[i], nse[i])) ||
        (rc = up(&p->recv_e, re[i], nre[i])))
      return rc;
    if ((rc = dalloc(c, &p->ghost_send, ghost_floats(nsp[i], nse[i]) + 1))) return rc;
    if ((rc = dalloc(c, &p->ghost_recv, ghost_floats(nrp[i], nre[i]) + 1))) return rc;
  }
  return MPMHIP_OK;
}

// max over the ranks of CNT_LINK_VOTE (1: some link of this rank does not work), read back into h_pin[PIN_LINK_VOTE]
static int reduce_vote(mpmhip_ctx *c) {
  FastState *f = c->fast;
  Rccl &r = f->ds->rccl;
  int *vote = f->g.counters + CNT_LINK_VOTE, *vote_all = f->g.counters + CNT_LINK_VOTE_ALL;
  MPM_NCCL_CHECK(c, r, r.AllReduce(vote, vote_all, 1, ncclInt32, ncclMax, r.comm, c->stream));
  MPM_HIP_CHECK(c, hipMemcpyAsync(f->h_pin + PIN_LINK_VOTE, vote_all, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MPM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  return MPMHIP_OK;
}

// Peer-mapped halo buffers.  At the first collective re-sort every pair of ranks that shares grid blocks allocates a
// fine-grained receive arena each, swaps the HIP IPC handles (64 bytes through ncclSend/ncclRecv), maps the other side's
// arena and pushes four rounds of a test pattern through both buffer parities with the same signal / wait primitives the
// substep uses.  The outcome is max-reduced over all ranks: only if every link of every rank works do the halos go
// through the links (k_halo_pack stores into the neighbour's memory and raises its flag, k_halo_add waits for the
// flag: no RCCL kernel in the substep); otherwise every rank stays on ncclSend/ncclRecv.  Pairs that start sharing
// blocks only later, or share more than link_cap of them, use send/recv for that interval (both sides see the same count).
static int rccl_link_setup(mpmhip_ctx *c) {
  FastState *f = c->fast;
  DistState *ds = f->ds;
  Rccl &r = ds->rccl;
  hipStream_t s = c->stream;
  int rc, bad = 0;
  ds->link_decided = true;
  std::vector<hipIpcMemHandle_t> mine(ds->peers.size()), theirs(ds->peers.size());
  for (size_t i = 0; i < ds->peers.size(); ++i) {
    RcclPeer &p = ds->peers[i];
    memset(&mine[i], 0, sizeof(hipIpcMemHandle_t));
    if (!p.n_blocks) continue;
    if ((rc = dalloc(c, &p.link_cnt, 1))) return rc;
    if ((rc = dalloc(c, &p.hbuf, 256))) return rc;  // [0, 96): my IPC handle + PCI bus id, [128, 224): the peer's
    p.link_cap = std::max(4 * p.n_blocks, 1024);
    size_t bytes = link_arena_floats(p.link_cap) * sizeof(float);
    if (hipExtMallocWithFlags((void **)&p.link_local, bytes, hipDeviceMallocFinegrained) != hipSuccess) { p.link_local = nullptr; bad = 1; continue; }
    if (hipMemsetAsync(p.link_local, 0, bytes, s) != hipSuccess || hipIpcGetMemHandle(&mine[i], p.link_local) != hipSuccess) {
      memset(&mine[i], 0, sizeof(hipIpcMemHandle_t));
      bad = 1;
    }
  }
  (void)hipGetLastError();
  // ... and with the handle this rank's PCI bus id: the receiver asks hipDeviceCanAccessPeer before it maps the arena
  char my_bus[32] = {0};
  int my_dev = 0;
  (void)hipGetDevice(&my_dev);
  if (hipDeviceGetPCIBusId(my_bus, (int)sizeof my_bus, my_dev) != hipSuccess) my_bus[0] = 0;
  (void)hipGetLastError();
  std::vector<std::array<char, 96>> msg_out(ds->peers.size()), msg_in(ds->peers.size());
  for (size_t i = 0; i < ds->peers.size(); ++i) {
    memcpy(msg_out[i].data(), &mine[i], 64);
    memcpy(msg_out[i].data() + 64, my_bus, 32);
    if (ds->peers[i].n_blocks) MPM_HIP_CHECK(c, hipMemcpyAsync(ds->peers[i].hbuf, msg_out[i].data(), 96, hipMemcpyHostToDevice, s));
  }
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "HIP IPC handle size");
  MPM_NCCL_CHECK(c, r, r.GroupStart());
  for (auto &p : ds->peers) {
    if (!p.n_blocks) continue;
    MPM_NCCL_CHECK(c, r, r.Send(p.hbuf, 96, ncclUint8, p.rank, r.comm, s));
    MPM_NCCL_CHECK(c, r, r.Recv(p.hbuf + 128, 96, ncclUint8, p.rank, r.comm, s));
  }
  MPM_NCCL_CHECK(c, r, r.GroupEnd());
  for (size_t i = 0; i < ds->peers.size(); ++i)
    if (ds->peers[i].n_blocks) MPM_HIP_CHECK(c, hipMemcpyAsync(msg_in[i].data(), ds->peers[i].hbuf + 128, 96, hipMemcpyDeviceToHost, s));
  MPM_HIP_CHECK(c, hipStreamSynchronize(s));
  const bool verbose = getenv("MPMHIP_VERBOSE") != nullptr;
  for (size_t i = 0; i < ds->peers.size(); ++i) {
    RcclPeer &p = ds->peers[i];
    if (!p.n_blocks) continue;
    static const hipIpcMemHandle_t none{};
    memcpy(&theirs[i], msg_in[i].data(), 64);
    char peer_bus[33] = {0};
    memcpy(peer_bus, msg_in[i].data() + 64, 32);
    // Can this GPU reach the peer's memory at all?  Asked BEFORE the arena is mapped (round 4): a pair without peer access (another
    // PCIe root without xGMI, an IOMMU setting) is refused here with a reason, instead of failing inside hipIpcOpenMemHandle or --
    // worse -- passing it and faulting in the first substep.  The same GPU (ranks sharing a device in tests) needs no peer access; a
    // peer device this process cannot see (masked by HIP_VISIBLE_DEVICES) cannot be asked, and the mapping is attempted.
    int peer_dev = -1, can = 1;
    const char *why = "same device";
    if (peer_bus[0] && hipDeviceGetByPCIBusId(&peer_dev, peer_bus) == hipSuccess) {
      if (peer_dev != my_dev) {
        if (hipDeviceCanAccessPeer(&can, my_dev, peer_dev) != hipSuccess) can = 0;
        why = can ? "hipDeviceCanAccessPeer: yes" : "hipDeviceCanAccessPeer: NO";
      }
    } else {
      why = "peer device not visible to this process: not asked";
    }
    (void)hipGetLastError();
    bool mapped = false;
    if (can && memcmp(&theirs[i], &none, 64) &&
        hipIpcOpenMemHandle((void **)&p.link_remote, theirs[i], hipIpcMemLazyEnablePeerAccess) == hipSuccess)
      mapped = true;
    if (!mapped) {
      p.link_remote = nullptr;
      bad = 1;
    }
    if (verbose || !mapped)
      fprintf(stderr, "[mpmhip] rank %d (%s) <- rank %d (%s): %s; halo arena %s\n", r.rank, my_bus[0] ? my_bus : "?", p.rank,
              peer_bus[0] ? peer_bus : "?", why, mapped ? "mapped (HIP IPC)" : "NOT mapped: every rank falls back to ncclSend / ncclRecv");
  }
  (void)hipGetLastError();
  const char *fault = getenv("MPMHIP_LINK_FAULT");  // tests: this rank pretends its links failed
  if (fault && *fault && atoi(fault) == r.rank) bad = 1;
  // agree before the handshake: a rank without its links would leave its neighbours waiting for pings
  MPM_HIP_CHECK(c, hipMemcpyAsync(f->g.counters + CNT_LINK_VOTE, &bad, sizeof(int), hipMemcpyHostToDevice, s));
  if ((rc = reduce_vote(c))) return rc;
  if (f->h_pin[PIN_LINK_VOTE] == 0) {
    MPM_HIP_CHECK(c, hipMemsetAsync(f->g.counters + CNT_LINK_TIMEOUT, 0, 2 * sizeof(int), s));  // (TIMEOUT and BAD)
    for (int round = 0; round < 4; ++round) {
      const int seq = (int)++ds->halo_seq, par = halo_parity(ds->halo_seq);
      auto n_test = [](const RcclPeer &p) { return (int)std::min<size_t>(halo_floats(p.link_cap, HALO_CHANNELS_MAX), (size_t)1 << 16); };
      for (auto &p : ds->peers) {
        if (!p.link_remote) continue;
        hipLaunchKernelGGL(k_link_ping, 16, TPB, 0, s, (unsigned *)link_data(p.link_remote, par, p.link_cap), n_test(p), p.link_cnt,
                           link_flag(p.link_remote, par), seq);
      }
      for (auto &p : ds->peers) {
        if (!p.link_remote) continue;
        hipLaunchKernelGGL(k_link_check, 16, TPB, 0, s, (const unsigned *)link_data(p.link_local, par, p.link_cap), n_test(p),
                           (const int *)link_flag(p.link_local, par), seq, f->g.counters);
      }
    }
    hipLaunchKernelGGL(k_link_verdict, 1, 1, 0, s, f->g.counters);
    if ((rc = reduce_vote(c))) return rc;
    MPM_HIP_CHECK(c, hipMemsetAsync(f->g.counters + CNT_LINK_TIMEOUT, 0, 2 * sizeof(int), s));
  }
  ds->link_on = f->h_pin[PIN_LINK_VOTE] == 0;
  if (getenv("MPMHIP_VERBOSE"))
    fprintf(stderr, "[mpmhip] rank %d: halo transport %s\n", r.rank, ds->link_on ? "peer-mapped buffers" : "ncclSend/ncclRecv");
  return MPMHIP_OK;
}

static int rccl_rebin(mpmhip_ctx *c) {
  FastState *f = c->fast;
  DistState *ds = f->ds;
  Rccl &r = ds->rccl;
  hipStream_t s = c->stream;
  int rc, nb = (int)f->nblocks;
  unsigned char *mine = ds->map_all + (size_t)r.rank * f->nblocks;
  if ((rc = fast_dist_rebin(c, mine))) return rc;
  MPM_NCCL_CHECK(c, r, r.AllGather(mine, ds->map_all, f->nblocks, ncclUint8, r.comm, s));
  for (auto &p : ds->peers) {
    hipLaunchKernelGGL(k_shared_flags, nblk(nb), TPB, 0, s, mine, ds->map_all + (size_t)p.rank * f->nblocks, nb, p.flag);
    // index[] and blocks[] in one go (the re-sort's flag compaction), total read back; too many for blocks[]: grown, and again
    if ((rc = compact_shared_blocks(c, p.flag, nb, p.index, p.own_blocks(), p.cap_blocks, &p.n_blocks))) return rc;
    if (p.n_blocks > p.cap_blocks) {
      int cap = std::max(p.n_blocks + p.n_blocks / 2, 256), *grown = nullptr;
      if ((rc = dalloc(c, &grown, (size_t)cap, false))) return rc;
      p.blocks = grown;
      if ((rc = dalloc(c, &p.halo_send, halo_floats(cap, HALO_CHANNELS_MAX), false))) return rc;   // (sized for the wider record)
      if ((rc = dalloc(c, &p.halo_recv, halo_floats(cap, HALO_CHANNELS_MAX), false))) return rc;
      p.cap_blocks = cap;
      if ((rc = compact_shared_blocks(c, p.flag, nb, p.index, p.own_blocks(), p.cap_blocks, nullptr))) return rc;
    }
  }
  if (ds->link_want && !ds->link_decided && (rc = rccl_link_setup(c))) return rc;   // (first re-sort: the links come up here)
  // fused halo for this interval?
  ds->fused_halo = false;
  if (ds->fused_want && ds->link_on && f->fuse_grid && ds->peers.size() <= (size_t)PEER_TAB) {
    bool all = true, any = false;
    for (auto &q : ds->peers)
      if (q.n_blocks) { any = true; all = all && peer_linked(ds->link_on, q); }
    if (all && any) {
      if (!ds->halo_slot) {
        if ((rc = dalloc(c, &ds->halo_slot, f->nblocks + 1, false))) return rc;
        ds->halo_multi = ds->halo_slot + f->nblocks;
      }
      MPM_HIP_CHECK(c, hipMemsetAsync(ds->halo_slot, 0xff, f->nblocks * sizeof(int), s));
      MPM_HIP_CHECK(c, hipMemsetAsync(ds->halo_multi, 0, sizeof(int), s));
      for (size_t i = 0; i < ds->peers.size(); ++i)
        if (ds->peers[i].n_blocks)
          hipLaunchKernelGGL(k_halo_slots, nblk(nb), TPB, 0, s, ds->peers[i].flag, ds->peers[i].index, nb, (int)i, ds->halo_slot, ds->halo_multi);
      MPM_HIP_CHECK(c, hipMemcpyAsync(f->h_pin + PIN_HALO_MULTI, ds->halo_multi, sizeof(int), hipMemcpyDeviceToHost, s));
      MPM_HIP_CHECK(c, hipStreamSynchronize(s));
      ds->fused_halo = f->h_pin[PIN_HALO_MULTI] == 0;
    }
  }
  return MPMHIP_OK;
}

static int rccl_exchange(mpmhip_ctx *c, bool halo) {
  const DistState *ds = c->fast->ds;
  const Rccl &r = ds->rccl;
  int CH = halo_channels(!c->movers.empty());
  bool open = false;
  for (const RcclPeer &p : ds->peers) {
    const int peer = p.rank;
    if (halo && peer_linked(ds->link_on, p)) continue;  // went through the pair's link (k_halo_pack / k_halo_add)
    size_t ns = halo ? halo_floats(p.n_blocks, CH) : ghost_floats(p.n_send_p, p.n_send_e);
    size_t nr = halo ? halo_floats(p.n_blocks, CH) : ghost_floats(p.n_recv_p, p.n_recv_e);
    if ((ns || nr) && !open) { MPM_NCCL_CHECK(c, r, r.GroupStart()); open = true; }
    if (ns) MPM_NCCL_CHECK(c, r, r.Send(halo ? p.halo_send : p.ghost_send, ns, ncclFloat, peer, r.comm, c->stream));
    if (nr) MPM_NCCL_CHECK(c, r, r.Recv(halo ? p.halo_recv : p.ghost_recv, nr, ncclFloat, peer, r.comm, c->stream));
  }
  if (open) MPM_NCCL_CHECK(c, r, r.GroupEnd());
  return MPMHIP_OK;
}

int fast_rccl_steps(mpmhip_ctx *c, float dt, int n, int64_t step_index, int rebin_interval, const float *mesh_x,
                    const float *mesh_v, const float *jt, int n_jt, const float *jv, const float *jf) {
  FastState *f = c->fast;
  DistState *ds = f->ds;
  if (!ds->rccl.comm) return fail(c, MPMHIP_ERR_STATE, "rccl_steps: call mpmhip_rccl_init first");
  // rebin_interval > 0: every rank re-sorts at substeps that are multiples of it.  <= 0: when any rank's early-warning
  // drift flag is up (the single-GPU policy made collective), at the latest every 256 (or -rebin_interval) substeps.
  const bool adaptive = rebin_interval <= 0;
  const int cap = rebin_interval < 0 ? -rebin_interval : (rebin_interval == 0 ? 256 : rebin_interval);
  constexpr int DIST_POLL = 16, DIST_LAG = 4;
  int rc;
  for (int k = 0; k < n; ++k) {
    int64_t idx = step_index + k;
    StepArgs a{dt, mesh_x, mesh_v, (float)((double)dt * (double)idx), true, jt, jt ? n_jt : 0, jv, jf};
    set_body_view(c, a.mesh_x, a.mesh_v, a.mesh_f);
    if (adaptive && ds->dflag_in_flight && idx >= ds->dflag_check_at) {
      // posted by k_post_flag: wait for THIS reduction's sequence number, then read its value
      for (long spins = 0; (unsigned)f->h_sig[SIG_DSEQ] != ds->dflag_seq; ++spins) {
        if ((spins & 0x3ff) == 0x3ff) {
          hipError_t e = hipStreamQuery(c->stream);
          if (e == hipSuccess && (unsigned)f->h_sig[SIG_DSEQ] != ds->dflag_seq)
            return fail(c, MPMHIP_ERR_HIP, "rccl_steps: the reduced drift flag never reached host memory");
          if (e != hipSuccess && e != hipErrorNotReady) MPM_HIP_CHECK(c, e);
        }
        std::this_thread::yield();
      }
      std::atomic_thread_fence(std::memory_order_acquire);
      if (f->h_sig[SIG_DFLAG]) ds->dist_resort = true;
      ds->dflag_in_flight = false;
    }
    bool due = adaptive ? (ds->dist_resort || ds->dist_since >= cap || !ds->rccl_sorted) : (idx % cap == 0);
    if (due || c->caller_dirty) {
      // owners -> copies, then re-sort (not before the first collective re-sort: the peers have their ghost lists, no order yet)
      if (f->ghost_g2p && f->have_order && !c->caller_dirty && ds->rccl_sorted && !ds->peers.empty()) {
        if ((rc = fast_dist_ghosts(c, 1))) return rc;
        if ((rc = rccl_exchange(c, false))) return rc;
        if ((rc = fast_dist_ghosts(c, 0))) return rc;
      }
      if (adaptive && f->true_since_rebin > 0)  // predictive sort: aim at the middle of the next interval
        f->lead_steps = std::min(std::max(0.5f * (float)f->true_since_rebin, 4.0f), 48.0f);
      ds->dist_keep_cur = true;
      rc = rccl_rebin(c);
      ds->dist_keep_cur = false;
      if (rc) return rc;
      f->true_since_rebin = 0;
      ds->dist_since = 0;
      ds->dist_resort = false;
      ds->rccl_sorted = true;
      // a reduction issued before this re-sort speaks about the old order: drop it (every rank does; the next poll waits for a
      // newer sequence number)
      ds->dflag_in_flight = false;
    }
    ds->halo_seq += 1;
    if ((rc = fast_dist_phase(c, 0, a))) return rc;
    {
      ScopedPhase ph(c, "halo_exchange");  // (profiling only: the ncclSend/ncclRecv group between the pack and the add kernel)
      if ((rc = rccl_exchange(c, true))) return rc;
    }
    if ((rc = fast_dist_phase(c, 1, a))) return rc;
    if (!f->ghost_g2p && (rc = rccl_exchange(c, false))) return rc;
    if ((rc = fast_dist_phase(c, 2, a))) return rc;
    advance_time(c, dt);
    ds->dist_since += 1;
    if (adaptive && !ds->dflag_in_flight && ds->dist_since % DIST_POLL == 0) {
      MPM_NCCL_CHECK(c, ds->rccl, ds->rccl.AllReduce(f->g.counters + CNT_DRIFT, f->g.counters + CNT_DRIFT_ALL, 1, ncclInt32, ncclMax,
                                                   ds->rccl.comm, c->stream));
      // no copy + event on the stream (each costs an idle queue, see fast_step): one thread posts the result
      hipLaunchKernelGGL(k_post_flag, 1, 1, 0, c->stream, f->g.counters + CNT_DRIFT_ALL, f->g.host_sig, (int)++ds->dflag_seq);
      ds->dflag_in_flight = true;
      ds->dflag_check_at = idx + 1 + DIST_LAG;
    }
  }
  if (ds->link_on) {  // a wait that ran into its wall-clock bound computed with an incomplete halo: fail the call
    MPM_HIP_CHECK(c, hipMemcpyAsync(f->h_pin + PIN_LINK_TIMEOUT, f->g.counters + CNT_LINK_TIMEOUT, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    MPM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    if (f->h_pin[PIN_LINK_TIMEOUT]) return fail(c, MPMHIP_ERR_HIP, "rccl_steps: a peer-mapped halo never arrived (flag wait timed out)");
  }
  return MPMHIP_OK;
}
int fast_dist_halo_transport(const mpmhip_ctx *c) { return c->fast->ds->link_on ? 1 : 0; }
int64_t fast_dist_fused_halo_steps(const mpmhip_ctx *c) { return c->fast->ds->fused_halo_steps; }

// the drift flag of this rank (set by the kernels when a particle is about to leave its tile margin); synchronous
int fast_dist_drift_flag(mpmhip_ctx *c, int32_t *out) {
  FastState *f = c->fast;
  MPM_HIP_CHECK(c, hipMemcpyAsync(f->h_pin + PIN_DIST_DRIFT, f->g.counters + CNT_DRIFT, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  MPM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
  *out = f->h_pin[PIN_DIST_DRIFT];
  return MPMHIP_OK;
}

}  // namespace mpm
