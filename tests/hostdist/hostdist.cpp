// The per-peer tables of the multi-GPU exchange (mpmavatar_amd/csrc/halo_tables.hpp) compiled for the host
// (tests/test_halo_tables_host.py): the builders are handed fabricated peer lists -- every pointer a made-up address that nothing
// dereferences -- and the tables they fill come back as flat arrays of 64-bit words.  The header needs nothing of HIP.
#include "halo_tables.hpp"

#include <cstdint>
#include <vector>

using namespace mpm;

namespace {

// a peer as P_WORDS 64-bit words, in this order (the test's PEER_FIELDS)
enum {
  P_N_BLOCKS, P_BLOCKS, P_HALO_SEND, P_HALO_RECV, P_N_SEND_P, P_N_RECV_P, P_N_SEND_E, P_N_RECV_E, P_SEND_P, P_RECV_P, P_SEND_E, P_RECV_E,
  P_GHOST_SEND, P_GHOST_RECV, P_LINK_LOCAL, P_LINK_REMOTE, P_LINK_CAP, P_LINK_CNT, P_WORDS
};
template <class T>
T *ptr(int64_t a) { return reinterpret_cast<T *>(static_cast<uintptr_t>(a)); }
int64_t word(const void *p) { return static_cast<int64_t>(reinterpret_cast<uintptr_t>(p)); }

// a record derived from DistPeer with members of its own behind it, like the one the in-library loop keeps: the builders must
// step through a list of these by ITS size
struct WidePeer : DistPeer {
  int64_t own[3] = {-1, -1, -1};
};

template <class Peer>
std::vector<Peer> peers_of(const int64_t *w, int n) {
  std::vector<Peer> v(n);
  for (int i = 0; i < n; ++i, w += P_WORDS) {
    Peer &p = v[i];
    p.n_blocks = (int32_t)w[P_N_BLOCKS]; p.blocks = ptr<const int32_t>(w[P_BLOCKS]);
    p.halo_send = ptr<float>(w[P_HALO_SEND]); p.halo_recv = ptr<float>(w[P_HALO_RECV]);
    p.n_send_p = (int32_t)w[P_N_SEND_P]; p.n_recv_p = (int32_t)w[P_N_RECV_P];
    p.n_send_e = (int32_t)w[P_N_SEND_E]; p.n_recv_e = (int32_t)w[P_N_RECV_E];
    p.send_p = ptr<const int32_t>(w[P_SEND_P]); p.recv_p = ptr<const int32_t>(w[P_RECV_P]);
    p.send_e = ptr<const int32_t>(w[P_SEND_E]); p.recv_e = ptr<const int32_t>(w[P_RECV_E]);
    p.ghost_send = ptr<float>(w[P_GHOST_SEND]); p.ghost_recv = ptr<float>(w[P_GHOST_RECV]);
    p.link_local = ptr<float>(w[P_LINK_LOCAL]); p.link_remote = ptr<float>(w[P_LINK_REMOTE]);
    p.link_cap = (int)w[P_LINK_CAP]; p.link_cnt = ptr<int>(w[P_LINK_CNT]);
  }
  return v;
}

// out = {n, with_mov, seq, wg_off[PEER_TAB + 1], blocks[], n_blocks[], buf[], sig[], cnt[]}
void put(const HaloTab &tb, int64_t *out) {
  *out++ = tb.n; *out++ = tb.with_mov; *out++ = tb.seq;
  for (int k = 0; k <= PEER_TAB; ++k) *out++ = tb.wg_off[k];
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.blocks[k]);
  for (int k = 0; k < PEER_TAB; ++k) *out++ = tb.n_blocks[k];
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.buf[k]);
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.sig[k]);
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.cnt[k]);
}
// out = {slot, n_peers, seq, ch, buf[], sig[]}
void put(const HaloIn &h, int64_t *out) {
  *out++ = word(h.slot); *out++ = h.n_peers; *out++ = h.seq; *out++ = h.ch;
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(h.buf[k]);
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(h.sig[k]);
}
// out = {n, wg_off[PEER_TAB + 1], ids_p[], ids_e[], n_p[], n_e[], buf[]}
void put(const GhostTab &tb, int64_t *out) {
  *out++ = tb.n;
  for (int k = 0; k <= PEER_TAB; ++k) *out++ = tb.wg_off[k];
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.ids_p[k]);
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.ids_e[k]);
  for (int k = 0; k < PEER_TAB; ++k) *out++ = tb.n_p[k];
  for (int k = 0; k < PEER_TAB; ++k) *out++ = tb.n_e[k];
  for (int k = 0; k < PEER_TAB; ++k) *out++ = word(tb.buf[k]);
}

}  // namespace

// out = {PEER_TAB, TAB_WG, LINK_DATA0, LINK_FLAG_STRIDE, HALO_CHANNELS_MAX, words of a peer}
extern "C" void hd_consts(int32_t *out) {
  out[0] = PEER_TAB; out[1] = TAB_WG; out[2] = LINK_DATA0; out[3] = LINK_FLAG_STRIDE; out[4] = HALO_CHANNELS_MAX; out[5] = P_WORDS;
}
extern "C" int64_t hd_link_arena_floats(int32_t cap) { return (int64_t)link_arena_floats(cap); }
extern "C" int64_t hd_halo_floats(int64_t n_blocks, int32_t movers) { return (int64_t)halo_floats((size_t)n_blocks, halo_channels(movers != 0)); }
extern "C" int64_t hd_ghost_floats(int64_t n_p, int64_t n_e) { return (int64_t)ghost_floats((size_t)n_p, (size_t)n_e); }

// wide != 0: the list is of WidePeer records
extern "C" void hd_halo_tab(const int64_t *peers, int32_t n, int32_t i0, int32_t send, int32_t movers, uint32_t seq, int32_t link_on,
                            int32_t wide, int64_t *out) {
  if (wide) {
    const auto v = peers_of<WidePeer>(peers, n);
    put(halo_tab(v.data(), v.size(), (size_t)i0, send != 0, movers != 0, seq, link_on != 0), out);
  } else {
    const auto v = peers_of<DistPeer>(peers, n);
    put(halo_tab(v.data(), v.size(), (size_t)i0, send != 0, movers != 0, seq, link_on != 0), out);
  }
}
extern "C" void hd_halo_in(const int64_t *peers, int32_t n, int64_t slot, int32_t movers, uint32_t seq, int32_t wide, int64_t *out) {
  if (wide) {
    const auto v = peers_of<WidePeer>(peers, n);
    put(halo_in(v.data(), v.size(), ptr<const int>(slot), movers != 0, seq), out);
  } else {
    const auto v = peers_of<DistPeer>(peers, n);
    put(halo_in(v.data(), v.size(), ptr<const int>(slot), movers != 0, seq), out);
  }
}
extern "C" void hd_ghost_tab(const int64_t *peers, int32_t n, int32_t i0, int32_t send, int32_t wide, int64_t *out) {
  if (wide) {
    const auto v = peers_of<WidePeer>(peers, n);
    put(ghost_tab(v.data(), v.size(), (size_t)i0, send != 0), out);
  } else {
    const auto v = peers_of<DistPeer>(peers, n);
    put(ghost_tab(v.data(), v.size(), (size_t)i0, send != 0), out);
  }
}
