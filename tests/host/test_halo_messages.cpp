// CPU check of the per-peer message list of the halo layer (lammps-spherharm_amd/csrc/halo_plan.hpp halo_peer_blocks),
// compiled with halo_plan.cpp and run by tests/test_halo_messages.py.  For every rank of a few processor grids, with
// seeded per-direction send counts that include zeros, the forward and the reverse list must be what the layout of
// shhalo_plan_layout says, leave out empty blocks, cover every row that is not the rank's own image, fit the buffers at
// every row width in use, and meet their counterpart on the peer.  Prints "ok <lists checked>" or the first failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "halo_plan.hpp"

using namespace shp;

#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                              \
      std::printf("\n");                                     \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

static unsigned lcg(unsigned& s) { return (s = s * 1664525u + 1013904223u) >> 8; }

struct Rank {
  shhalo_geometry geo;
  int send_cnt[27], recv_cnt[27];
  shhalo_layout lay;
  HaloPeerBlocks fwd, rev;
};

// n blocks against the layout's per-peer offsets and counts: one per peer with rows, none empty, in peer_rank order
static void check_blocks(const char* what, int rank, const shhalo_layout& L, const HaloRowBlock* blk, int n, const int* off, const int* cnt,
                         int nrows, int self_rows)
{
  int k = 0, rows = 0;
  for (int j = 0; j < n; ++j) {
    CHECK(blk[j].count > 0, "%s of rank %d: entry %d is empty", what, rank, j);
    CHECK(blk[j].peer != rank, "%s of rank %d: entry %d goes to the rank itself", what, rank, j);
    while (k < L.npeers && L.peer_rank[k] != blk[j].peer) {   // peers passed over have nothing to move
      CHECK(cnt[k] == 0, "%s of rank %d: peer %d with %d rows has no entry", what, rank, L.peer_rank[k], cnt[k]);
      ++k;
    }
    CHECK(k < L.npeers, "%s of rank %d: entry %d names rank %d: not a peer, a second entry for one, or out of order", what, rank, j,
          blk[j].peer);
    CHECK(blk[j].first == off[k] && blk[j].count == cnt[k], "%s of rank %d, peer %d: rows %d + %d, the layout has %d + %d", what, rank,
          blk[j].peer, blk[j].first, blk[j].count, off[k], cnt[k]);
    rows += blk[j].count;
    ++k;
  }
  for (; k < L.npeers; ++k) CHECK(cnt[k] == 0, "%s of rank %d: peer %d with %d rows has no entry", what, rank, L.peer_rank[k], cnt[k]);
  CHECK(rows + self_rows == nrows, "%s of rank %d: %d rows to peers + %d of its own images, the layout has %d", what, rank, rows,
        self_rows, nrows);
  // at every row width in use the messages are disjoint pieces of a buffer of nrows rows
  for (int W : {6, 7, 9, 13}) {
    std::vector<char> used((size_t)nrows * W, 0);
    for (int j = 0; j < n; ++j) {
      const long long a = (long long)blk[j].first * W, b = a + (long long)blk[j].count * W;
      CHECK(a >= 0 && b <= (long long)nrows * W, "%s of rank %d, W = %d: doubles [%lld, %lld) outside a buffer of %d rows", what, rank, W,
            a, b, nrows);
      for (long long q = a; q < b; ++q) {
        CHECK(!used[q], "%s of rank %d, W = %d: two messages share double %lld", what, rank, W, q);
        used[q] = 1;
      }
    }
  }
}

static void check_same(const char* what, int rank, const HaloRowBlock* a, int na, const HaloRowBlock* b, int nb)
{
  CHECK(na == nb, "%s of rank %d: %d entries against %d", what, rank, na, nb);
  for (int j = 0; j < na; ++j)
    CHECK(a[j].peer == b[j].peer && a[j].first == b[j].first && a[j].count == b[j].count, "%s of rank %d: entry %d differs", what, rank, j);
}

static int check_grid(const int grid[3], const int periodic[3], unsigned seed)
{
  const double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {10.0, 12.0, 14.0};
  const int nranks = grid[0] * grid[1] * grid[2];
  std::vector<Rank> R(nranks);
  for (int r = 0; r < nranks; ++r) {
    CHECK(shhalo_plan_geometry(grid, lo, hi, periodic, 1.0, r, &R[r].geo) == SHPAIR_OK, "geometry of rank %d", r);
    for (int c = 0; c < 27; ++c) {
      const unsigned u = lcg(seed);
      R[r].send_cnt[c] = (c == 13 || R[r].geo.peer[c] < 0 || u % 3 == 0) ? 0 : 1 + (int)(u % 17);
    }
  }
  for (int r = 0; r < nranks; ++r) {
    Rank& me = R[r];
    for (int c = 0; c < 27; ++c) {
      const int p = me.geo.peer[c];
      // what arrives through my direction c was sent with the sender's code 26 - c
      me.recv_cnt[c] = (c == 13 || p < 0) ? 0 : R[p].send_cnt[26 - c];
    }
    CHECK(shhalo_plan_layout(&me.geo, me.send_cnt, me.recv_cnt, &me.lay) == SHPAIR_OK, "layout of rank %d", r);
    me.fwd = halo_peer_blocks(me.lay, false);
    me.rev = halo_peer_blocks(me.lay, true);
    const shhalo_layout& L = me.lay;
    int self_send = 0, self_recv = 0;
    for (int c = 0; c < 27; ++c)
      if (c != 13 && me.geo.peer[c] == r) {
        self_send += L.send_cnt[c];
        self_recv += L.recv_cnt[c];
      }
    check_blocks("forward send", r, L, me.fwd.send, me.fwd.nsend, L.peer_send_off, L.peer_send_cnt, L.nsend, self_send);
    check_blocks("forward receive", r, L, me.fwd.recv, me.fwd.nrecv, L.peer_recv_off, L.peer_recv_cnt, L.nghost, self_recv);
    check_blocks("reverse send", r, L, me.rev.send, me.rev.nsend, L.peer_recv_off, L.peer_recv_cnt, L.nghost, self_recv);
    check_blocks("reverse receive", r, L, me.rev.recv, me.rev.nrecv, L.peer_send_off, L.peer_send_cnt, L.nsend, self_send);
    check_same("reverse send against forward receive", r, me.rev.send, me.rev.nsend, me.fwd.recv, me.fwd.nrecv);
    check_same("reverse receive against forward send", r, me.rev.recv, me.rev.nrecv, me.fwd.send, me.fwd.nsend);
    if (nranks == 1) CHECK(me.fwd.nsend == 0 && me.fwd.nrecv == 0 && L.npeers == 0, "one rank has no remote peer");
  }
  // every forward send A -> B of n rows meets a forward receive of n rows from A on B, and nothing is received unsent
  for (int a = 0; a < nranks; ++a) {
    for (int j = 0; j < R[a].fwd.nsend; ++j) {
      const HaloRowBlock& s = R[a].fwd.send[j];
      CHECK(s.peer >= 0 && s.peer < nranks, "rank %d sends to rank %d", a, s.peer);
      int met = 0;
      for (int k = 0; k < R[s.peer].fwd.nrecv; ++k)
        if (R[s.peer].fwd.recv[k].peer == a) {
          ++met;
          CHECK(R[s.peer].fwd.recv[k].count == s.count, "rank %d sends %d rows to rank %d, which expects %d", a, s.count, s.peer,
                R[s.peer].fwd.recv[k].count);
        }
      CHECK(met == 1, "the send of rank %d to rank %d meets %d receives", a, s.peer, met);
    }
    for (int j = 0; j < R[a].fwd.nrecv; ++j) {
      const HaloRowBlock& g = R[a].fwd.recv[j];
      CHECK(g.peer >= 0 && g.peer < nranks, "rank %d receives from rank %d", a, g.peer);
      int met = 0;
      for (int k = 0; k < R[g.peer].fwd.nsend; ++k) met += R[g.peer].fwd.send[k].peer == a;
      CHECK(met == 1, "the receive of rank %d from rank %d meets %d sends", a, g.peer, met);
    }
  }
  return 2 * nranks;
}

int main()
{
  const int cases[4][6] = {{2, 1, 1, 1, 1, 1}, {2, 2, 1, 1, 1, 0}, {2, 2, 2, 1, 1, 0}, {1, 1, 1, 1, 1, 1}};
  int lists = 0;
  for (const auto& c : cases)
    for (unsigned seed = 1; seed <= 8; ++seed) lists += check_grid(c, c + 3, 20241019u * seed);
  std::printf("ok %d\n", lists);
  return 0;
}
