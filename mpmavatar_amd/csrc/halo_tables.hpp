// halo_tables.hpp -- the per-peer tables of the multi-GPU exchange: what the kernels are handed (HaloTab, GhostTab, HaloIn), the
// record sizes, the layout of a peer-link arena, and the ONE place each table is filled from a peer list.  Plain structs and integer /
// pointer arithmetic, no HIP: the host fills the tables with it (dist.hip), the kernels read them (fast_device.hpp),
// tests/hostdist/ checks the builders with g++ on fabricated peer lists.
#pragma once
#include <cstddef>

#include "../../include/mpmhip.h"

namespace mpm {
inline namespace fk {

// Fused halo add (multi-GPU, peer-mapped halos): k_g2p<.., HALO = true> adds the neighbour rank's contribution to a shared
// block while it stages its tile -- own accumulator + the value the neighbour's pack stored into this rank's arena -- instead
// of a separate add kernel between p2g and g2p.  slot == nullptr: off.
constexpr int PEER_TAB = 8;
struct HaloIn {
  const int *slot;             // [blocks] -1, or (peer << 24) | index of the block in that peer's shared-block list
  const float *buf[PEER_TAB];  // this substep's receive buffer of each peer (arena of parity halo_seq & 1)
  const int *sig[PEER_TAB];    // its flag: reaches `seq` when the neighbour's pack of this substep has landed
  int n_peers, seq, ch;        // ch = 4 (m, momentum) or 8 (+ mover channels)
};

// ---- multi-GPU exchange helpers (mpmavatar_amd/dist.py drives them) ---------------------------------------
// halo: the (m, momentum) and mover channels of the grid blocks two ranks both have on their active lists
// One launch serves up to PEER_TAB neighbours: workgroups [wg_off[p], wg_off[p+1]) belong to peer p.
struct HaloTab {
  int n, with_mov;
  int wg_off[PEER_TAB + 1];
  const int *blocks[PEER_TAB];
  int n_blocks[PEER_TAB];
  float *buf[PEER_TAB];
  // peer-mapped halos ("peer links", fast_device.hpp): pack stores straight into the neighbour's receive buffer and the last
  // workgroup raises sig (a flag in the neighbour's memory) to seq; add waits for its own flag to reach seq.  null: none
  int *sig[PEER_TAB];
  int *cnt[PEER_TAB];
  int seq;
};
struct GhostTab {
  int n;
  int wg_off[PEER_TAB + 1];
  const int *ids_p[PEER_TAB], *ids_e[PEER_TAB];
  int n_p[PEER_TAB], n_e[PEER_TAB];
  float *buf[PEER_TAB];
};

}  // namespace fk

struct DistPeer : mpmhip_dist_peer {  // the ABI's peer record (shared blocks, halo buffers, ghost lists) plus the pair's link
  DistPeer() : mpmhip_dist_peer{} {}
  explicit DistPeer(const mpmhip_dist_peer &p) : mpmhip_dist_peer(p) {}
  // peer link (in-library loop only; see rccl_link_setup): arena = [flag parity 0 | flag parity 1 | data parity 0 | data parity 1],
  // flags 64 B apart, data from word 32, link_cap blocks x 8 channels x 64 nodes per parity.  link_local is fine-grained memory of
  // this rank that the neighbour writes; link_remote is the neighbour's arena for this rank (hipIpcOpenMemHandle)
  float *link_local = nullptr, *link_remote = nullptr;
  int link_cap = 0;
  int *link_cnt = nullptr;
};

// Record sizes of the two exchanges, in floats (mpmavatar_amd/dist.py has the same two functions; include/mpmhip.h states them
// at mpmhip_dist_peer).  Halo: 64 nodes per channel of a shared block, (m, momentum) = 4 channels, 8 with a particle mover.
// Ghosts: x, v of a vertex / traditional particle, the director d3 of an element.
constexpr int HALO_CHANNELS_MAX = 8;  // the in-library loop sizes its halo buffers and link arenas for the wider record
inline int halo_channels(bool movers) { return movers ? 8 : 4; }
constexpr size_t halo_floats(size_t n_blocks, int channels) { return n_blocks * (size_t)channels * 64; }
constexpr size_t ghost_floats(size_t n_p, size_t n_e) { return 6 * n_p + 3 * n_e; }
// the peer-link arena (layout at DistPeer): where parity `par`'s data and flag sit
constexpr int LINK_DATA0 = 32, LINK_FLAG_STRIDE = 16;
constexpr size_t link_arena_floats(int cap) { return (size_t)LINK_DATA0 + 2 * halo_floats((size_t)cap, HALO_CHANNELS_MAX); }
inline float *link_data(float *arena, int par, int cap) { return arena + LINK_DATA0 + (size_t)par * halo_floats((size_t)cap, HALO_CHANNELS_MAX); }
inline int *link_flag(float *arena, int par) { return (int *)arena + par * LINK_FLAG_STRIDE; }

// ---- the rules, once each ----------------------------------------------------------------------------------
// A table's workgroups have TAB_WG threads, one per float of a halo record / per ghost id (the kernels' TPB and PT: asserted
// in fast_device.hpp, where both names are defined).
constexpr int TAB_WG = 256;
inline int tab_wgs(size_t items) { return (int)((items + TAB_WG - 1) / TAB_WG); }
// The sequence number of a substep's exchange is its flag value and, by its lowest bit, its buffer parity (unsigned: it wraps).
inline int halo_parity(unsigned seq) { return (int)(seq & 1u); }
// This pair's halo goes through its link: the links are in use, this one is mapped, and the shared blocks fit its arena.
inline bool peer_linked(bool link_on, const DistPeer &p) { return link_on && p.link_remote && p.n_blocks <= p.link_cap; }

// ---- the builders: Peer is DistPeer or a record derived from it ------------------------------------------
// Halo table of the peers [i0, i0 + PEER_TAB) of a list; send: pack (into halo_send, or the neighbour's arena), else add (from
// halo_recv, or this rank's arena).  Peers that share no block get no slot.
template <class Peer>
inline HaloTab halo_tab(const Peer *peers, size_t n, size_t i0, bool send, bool movers, unsigned seq, bool link_on) {
  HaloTab tb{};
  tb.with_mov = movers ? 1 : 0;
  tb.seq = (int)seq;
  const int CH = halo_channels(movers), par = halo_parity(seq);
  for (size_t i = i0; i < n && i < i0 + PEER_TAB; ++i) {
    const DistPeer &p = peers[i];
    if (!p.n_blocks) continue;
    const int k = tb.n++;
    tb.blocks[k] = p.blocks; tb.n_blocks[k] = p.n_blocks; tb.buf[k] = send ? p.halo_send : p.halo_recv;
    if (peer_linked(link_on, p)) {  // store into / read from the receive arena of this pair instead, flag in the same memory
      float *arena = send ? p.link_remote : p.link_local;
      tb.buf[k] = link_data(arena, par, p.link_cap);
      tb.sig[k] = link_flag(arena, par);
      tb.cnt[k] = p.link_cnt;
    }
    tb.wg_off[k + 1] = tb.wg_off[k] + tab_wgs(halo_floats(p.n_blocks, CH));
  }
  return tb;
}
// What g2p adds for itself (fused halo): this substep's receive buffers and flags.  Indexed by the peer's POSITION in the list, not
// compacted -- `slot` stores that position (k_halo_slots); a peer without blocks or without a mapped arena leaves its entry null.
template <class Peer>
inline HaloIn halo_in(const Peer *peers, size_t n, const int *slot, bool movers, unsigned seq) {
  HaloIn h{};
  h.slot = slot;
  h.n_peers = (int)n;
  h.seq = (int)seq;
  h.ch = halo_channels(movers);
  for (size_t i = 0; i < n && i < (size_t)PEER_TAB; ++i) {
    const DistPeer &q = peers[i];
    if (!q.n_blocks || !q.link_local) continue;
    h.buf[i] = link_data(q.link_local, halo_parity(seq), q.link_cap);
    h.sig[i] = link_flag(q.link_local, halo_parity(seq));
  }
  return h;
}
// Ghost table of the peers [i0, i0 + PEER_TAB): the send or the receive lists; peers without ghosts get no slot.
template <class Peer>
inline GhostTab ghost_tab(const Peer *peers, size_t n, size_t i0, bool send) {
  GhostTab tb{};
  for (size_t i = i0; i < n && i < i0 + PEER_TAB; ++i) {
    const DistPeer &p = peers[i];
    const int np = send ? p.n_send_p : p.n_recv_p, ne = send ? p.n_send_e : p.n_recv_e;
    if (np + ne == 0) continue;
    const int k = tb.n++;
    tb.ids_p[k] = send ? p.send_p : p.recv_p; tb.ids_e[k] = send ? p.send_e : p.recv_e;
    tb.n_p[k] = np; tb.n_e[k] = ne; tb.buf[k] = send ? p.ghost_send : p.ghost_recv;
    tb.wg_off[k + 1] = tb.wg_off[k] + tab_wgs((size_t)(np + ne));
  }
  return tb;
}

}  // namespace mpm
