#include "deep_halo.hpp"

#include <algorithm>

namespace wave3d {

ShellSplit split_shells(const Box& c, const Box& in) {
    ShellSplit s;
    auto add = [&](Box b) {
        if (!b.empty()) s.shell.push_back(b);
    };
    if (in.empty()) {
        add(c);
        s.nx = int(s.shell.size());
        return s;
    }
    add({c.i0, in.i0 - 1, c.j0, c.j1, c.k0, c.k1});
    add({in.i1 + 1, c.i1, c.j0, c.j1, c.k0, c.k1});
    s.nx = int(s.shell.size());
    add({in.i0, in.i1, c.j0, in.j0 - 1, c.k0, c.k1});
    add({in.i0, in.i1, in.j1 + 1, c.j1, c.k0, c.k1});
    add({in.i0, in.i1, in.j0, in.j1, c.k0, in.k0 - 1});
    add({in.i0, in.i1, in.j0, in.j1, in.k1 + 1, c.k1});
    return s;
}

namespace {

struct Planner {
    const Topology& t;
    const bool self_x;
    const int dA, dB, G;  // depth of the next A level, of the next B level, ghost depth
    DeepHaloPlan P;

    int X() const { return t.X(); }
    int Y() const { return t.Y(); }
    int Z() const { return t.Z(); }

    // ---- x: whole planes (contiguous, sent in place) --------------------------------------
    // depth dA of the newest level (next A), dB = dA - 1 of the one before (next B); the
    // periodic duplicate plane x = N is skipped (mpi_new.cpp:186-187) and shipped to the other
    // end of the ring as the seam alias plane instead (tags 12/14, 22/24).
    // Sends are listed up then down, receives from-down then from-up: per-peer FIFO order
    // matches on both ends also when up == down (dims[0] == 2).
    void x_planes(HaloRound& r) {
        using M = PlaneMsg;
        W3D_REQUIRE(X() >= 2 * dA, "temporal blocking needs >= 2 x depth planes per rank");
        // one x rank messaging itself (--x-self-transport): the seam partner planes are
        // its own planes X and 1 (see sweep), no alias messages
        const bool first = t.first(0) && t.dims[0] > 1, last = t.last(0) && t.dims[0] > 1;
        const bool lastx = t.last(0), firstx = t.first(0);
        const int up = t.nbr[0][1], dn = t.nbr[0][0], n = X();
        const bool aliasB = dA >= 3;
        r.sends.push_back(M{up, 11, 0, lastx ? n - dA : n - dA + 1, dA});
        if (last) r.sends.push_back(M{up, 12, 0, n, 1});
        r.sends.push_back(M{up, 13, 1, lastx ? n - dB : n - dB + 1, dB});
        if (last && aliasB) r.sends.push_back(M{up, 14, 1, n, 1});
        r.sends.push_back(M{dn, 21, 0, firstx ? 2 : 1, dA});
        if (first) r.sends.push_back(M{dn, 22, 0, 1, 1});
        r.sends.push_back(M{dn, 23, 1, firstx ? 2 : 1, dB});
        if (first && aliasB) r.sends.push_back(M{dn, 24, 1, 1, 1});
        r.recvs.push_back(M{dn, 11, 0, 1 - dA, dA});
        if (first) r.recvs.push_back(M{dn, 12, 0, kAliasPlane, 1});
        r.recvs.push_back(M{dn, 13, 1, 1 - dB, dB});
        if (first && aliasB) r.recvs.push_back(M{dn, 14, 1, kAliasPlane, 1});
        r.recvs.push_back(M{up, 21, 0, n + 1, dA});
        if (last) r.recvs.push_back(M{up, 22, 0, kAliasPlane, 1});
        r.recvs.push_back(M{up, 23, 1, n + 1, dB});
        if (last && aliasB) r.recvs.push_back(M{up, 24, 1, kAliasPlane, 1});
        P.alias[0] = first || last;
        P.alias[1] = P.alias[0] && aliasB;
    }

    // ---- y (round 1) and z (round 2): rows / columns of depth dA (A) and dB (B), each over the
    // full extent of the axes exchanged before (ghosts included); one buffer per message
    void yz_round(HaloRound& r, int ax) {
        if (t.dims[ax] == 1) return;
        const int n = ax == 1 ? Y() : Z();
        auto box = [&](int lo, int hi) {
            Box b{1 - G, X() + G, 1, Y(), 1, Z()};
            if (ax == 1) b.j0 = lo, b.j1 = hi;
            else b.j0 = 1 - G, b.j1 = Y() + G, b.k0 = lo, b.k1 = hi;
            return b;
        };
        auto add = [&](bool send, int peer, int tag, int level, Box b) {
            const int id = int(P.bufs.size());
            P.bufs.push_back(HaloBuf{peer, tag, size_t(b.count())});
            (send ? r.bsends : r.brecvs).push_back(BoxMsg{peer, tag, level, b, 0, id, 0});
            (send ? r.sbufs : r.rbufs).push_back(id);
        };
        const int base = ax == 1 ? 30 : 50;
        const int dn = t.nbr[ax][0], up = t.nbr[ax][1];
        const bool S = true, V = false;
        // sends: down (to dn) then up; receives: from down then from up — the same
        // per-peer order on both sides (tag-less RCCL matching)
        W3D_REQUIRE(n >= 2 * dA, "temporal blocking needs >= 2 x depth nodes per rank on split axes");
        if (dn >= 0) add(S, dn, base + 1, 0, box(1, dA)), add(S, dn, base + 2, 1, box(1, dB));
        if (up >= 0) add(S, up, base + 11, 0, box(n - dA + 1, n)), add(S, up, base + 12, 1, box(n - dB + 1, n));
        if (dn >= 0) add(V, dn, base + 11, 0, box(1 - dA, 0)), add(V, dn, base + 12, 1, box(1 - dB, 0));
        if (up >= 0) add(V, up, base + 1, 0, box(n + 1, n + dA)), add(V, up, base + 2, 1, box(n + 1, n + dB));
        // three-layer sweeps also evaluate C on the seam alias plane (k_seam_c), whose
        // j/k neighbours at the subdomain edge are ghosts: the alias planes of the y/z
        // neighbours (same x coordinate, so they hold the same global plane) supply them
        if (dA < 3 || !P.alias[0]) return;
        auto abox = [&](int lo, int hi) {
            Box b = box(lo, hi);
            b.i0 = b.i1 = 0;
            return b;
        };
        if (dn >= 0) add(S, dn, base + 3, 2, abox(1, dA));
        if (up >= 0) add(S, up, base + 13, 2, abox(n - dA + 1, n));
        if (dn >= 0) add(V, dn, base + 13, 2, abox(1 - dA, 0));
        if (up >= 0) add(V, up, base + 3, 2, abox(n + 1, n + dA));
        // ... and the B alias plane (level 3, depth dB): the seam stages read B there on
        // their rings, whose y/z ghosts the x round delivered stale (round 6: tb4 on 2x2x2
        // with --halo rounds was wrong from the third sweep on; --halo direct sends them)
        if (!P.alias[1]) return;
        if (dn >= 0) add(S, dn, base + 4, 3, abox(1, dB));
        if (up >= 0) add(S, up, base + 14, 3, abox(n - dB + 1, n));
        if (dn >= 0) add(V, dn, base + 14, 3, abox(1 - dB, 0));
        if (up >= 0) add(V, up, base + 4, 3, abox(n + 1, n + dB));
    }

    // Single-round plan (--halo direct, the default). On a fully connected xGMI node every
    // diagonal neighbour has its own link, so every ghost region — faces, edges, corners, of A
    // (depth dA) and B (depth dB), and of the seam alias planes — comes straight from the rank
    // that owns it, all in one transport group: one latency instead of three, all links busy at
    // once (2x2x2: 7 peers, one link each). Region rules per axis a, receiver R, sender
    // S = R + d: d_a = -1 -> R's ghosts 1-D..0 from S's top D owned nodes, +1 -> R's ghosts
    // E+1..E+D from S's bottom D, 0 -> the owned range (and the x ghosts as well when x wraps
    // inside the rank: the fused wrap fills them). Across the periodic seam the duplicate plane is
    // skipped (mpi_new.cpp:186-187): the last x-rank sends X-D..X-1, the first 2..D+1, and the
    // planes x = N / x = 0 themselves travel as the alias planes. Messages are listed by (level,
    // direction) on both ends, so per-peer FIFO order matches for tag-less RCCL.
    void direct_boxes(HaloRound& r) {
        const int E[3] = {X(), Y(), Z()};
        const bool seam = t.dims[0] > 1;  // alias planes exist (first / last x-rank)
        auto peer = [&](const int d[3]) -> int {  // rank at coords + d, -1 outside y/z
            int c[3];
            for (int a = 0; a < 3; ++a) {
                c[a] = t.coords[a] + d[a];
                if (a == 0) c[a] = ((c[a] % t.dims[0]) + t.dims[0]) % t.dims[0];
                else if (c[a] < 0 || c[a] >= t.dims[a]) return -1;
            }
            return t.rank_of(c[0], c[1], c[2]);
        };
        // receive box of R for direction d (ghost region), depth D
        auto rbox = [&](const int d[3], int D, bool alias) {
            int lo[3], hi[3];
            for (int a = 0; a < 3; ++a) {
                if (d[a] < 0) lo[a] = 1 - D, hi[a] = 0;
                else if (d[a] > 0) lo[a] = E[a] + 1, hi[a] = E[a] + D;
                else if (a == 0 && self_x) lo[a] = 1 - D, hi[a] = E[a] + D;
                else lo[a] = 1, hi[a] = E[a];
            }
            if (alias) lo[0] = hi[0] = 0;  // the alias buffer's one plane (logical i = 0)
            return Box{lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]};
        };
        // source box of R for a receiver Q = R - d (R fills Q's ghosts in direction d)
        auto sbox = [&](const int d[3], int D, bool alias) {
            int lo[3], hi[3];
            for (int a = 0; a < 3; ++a) {
                // crossing the periodic seam from Q to R: Q first and R last x-rank (d = -1),
                // or Q last and R first (d = +1); with one x rank messaging itself both hold
                const int tw = a == 0 && ((d[a] < 0 && t.last(0)) || (d[a] > 0 && t.first(0))) ? 1 : 0;
                if (d[a] < 0) lo[a] = E[a] - D + 1 - tw, hi[a] = E[a] - tw;
                else if (d[a] > 0) lo[a] = 1 + tw, hi[a] = D + tw;
                else if (a == 0 && self_x) lo[a] = 1 - D, hi[a] = E[a] + D;
                else lo[a] = 1, hi[a] = E[a];
            }
            if (alias) lo[0] = hi[0] = d[0] < 0 ? E[0] : 1;  // plane x = N (last) / x = 0 (first)
            return Box{lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]};
        };
        for (int level = 0; level < (dA >= 3 ? 4 : 3); ++level) {
            const bool alias = level >= 2;
            if (alias && !seam) continue;
            const int D = (level == 0 || level == 2) ? dA : dB;
            int q = 0;
            for (int dx = -1; dx <= 1; ++dx)
                for (int dy = -1; dy <= 1; ++dy)
                    for (int dz = -1; dz <= 1; ++dz, ++q) {
                        if (!dx && !dy && !dz) continue;
                        if (self_x && dx) continue;  // x ghosts: fused wrap
                        if (alias && !dx) continue;  // alias planes cross the x seam only
                        if (!dy && !dz) continue;    // x faces: whole planes in place (x list)
                        const int tag = 200 + q * 4 + level;
                        const int d[3] = {dx, dy, dz}, md[3] = {-dx, -dy, -dz};
                        // receive: from S = R + d into R's ghosts (alias: R first x-rank <- last
                        // for d_x = -1, R last <- first for d_x = +1)
                        const int S = peer(d);
                        const bool ra = !alias || (dx < 0 ? t.first(0) : t.last(0));
                        if (S >= 0 && ra) r.brecvs.push_back(BoxMsg{S, tag, level, rbox(d, D, alias), dx, -1, 0});
                        // send: to Q = R - d from R's own nodes (alias: R last x-rank -> first
                        // for d_x = -1, R first -> last for d_x = +1)
                        const int Q = peer(md);
                        const bool sa = !alias || (dx < 0 ? t.last(0) : t.first(0));
                        if (Q >= 0 && sa) r.bsends.push_back(BoxMsg{Q, tag, level, sbox(d, D, alias), dx, -1, 0});
                    }
        }
        pack_per_peer(r);
    }

    // one buffer per peer: its boxes back to back in (level, direction) order — the order in
    // which both ends list them, so the packed messages have the same layout
    void pack_per_peer(HaloRound& r) {
        auto pack = [&](std::vector<BoxMsg>& v, std::vector<int>& ids) {
            std::vector<int> peers;
            for (auto& m : v)
                if (std::find(peers.begin(), peers.end(), m.peer) == peers.end()) peers.push_back(m.peer);
            std::sort(peers.begin(), peers.end());
            for (int pr : peers) {
                const int id = int(P.bufs.size());
                size_t off = 0;
                for (auto& m : v)
                    if (m.peer == pr) m.buf = id, m.off = off, off += size_t(m.box.count());
                P.bufs.push_back(HaloBuf{pr, kPeerTag, off});
                ids.push_back(id);
            }
        };
        pack(r.bsends, r.sbufs);
        pack(r.brecvs, r.rbufs);
    }

    // The last layer within dA nodes of a received ghost depends on it (through the rings).
    // The j/k shells are widened to whole tiles — tile_rows rows from the compute box's edge, k on
    // the global 64-column tile grid — so the shell launch runs no partially filled tiles
    // (a 2-column z shell used 2 of 64 lanes per tile and cost ~20 % of a sweep); the
    // interior shrinks by the same nodes, so the total work is that of one full sweep. x
    // shells stay dA planes thin: the march along i handles thin boxes at a small prologue.
    // The shells also contain every plane / row / column the next exchange sends (the first
    // and last x-ranks send one plane deeper, skipping the periodic duplicate plane), so the
    // exchange can start as soon as the shells are done, while the interior still runs.
    void shells(int TJ) {
        const Box c = t.compute_box();
        Box in = c;
        const int TK = kShellTileK;
        if (!self_x) {
            const int xs = t.dims[0] > 1 ? 1 : 0;  // one x rank messaging itself: both ends
            in.i0 = std::max(in.i0, 1 + dA + ((t.first(0) || !xs) ? 1 : 0));
            in.i1 = std::min(in.i1, X() - dA - ((t.last(0) || !xs) ? 1 : 0));
        }
        if (t.nbr[1][0] >= 0) in.j0 = std::max(in.j0, std::max(1 + dA, c.j0 + TJ));
        if (t.nbr[1][1] >= 0) in.j1 = std::min(in.j1, std::min(Y() - dA, c.j1 - TJ));
        if (t.nbr[2][0] >= 0) in.k0 = std::max(in.k0, 1 + TK * ((dA + TK - 1) / TK));
        if (t.nbr[2][1] >= 0) in.k1 = std::min(in.k1, TK * ((Z() - dA) / TK));
        P.interior = in;
        P.shell = split_shells(c, in).shell;
    }

    // --overlap pipe: slab j of a deep sweep covers planes xs(j) .. xs(j+1)-1 of 1..X (the same
    // cut on every rank of an x coordinate, so y/z neighbours cut their messages alike). Group j
    // holds what slab j computes: the x faces and the dx != 0 boxes of the direct plan go with the
    // end slab that holds their source planes (dx < 0 / the x+ faces: slab C-1; dx > 0 / the x-
    // faces: slab 0; each slab is >= depth + 1 planes thick, pipe_slabs()), the dx == 0 boxes are
    // cut along x. Both ends derive the groups from plans that already match message for message,
    // and cut them the same way, so every group's packed per-peer messages match too.
    void pipe(int C) {
        auto xs = [&](int j) { return 1 + int(i64(j) * X() / C); };
        auto cut = [&](Box b, int j) {
            if (j > 0) b.i0 = std::max(b.i0, xs(j));
            if (j < C - 1) b.i1 = std::min(b.i1, xs(j + 1) - 1);
            return b;
        };
        for (int j = 0; j < C; ++j) P.slabs.push_back(cut(t.compute_box(), j));
        P.pipe.assign(size_t(C), HaloRound{});
        const HaloRound& W = P.rounds[0];
        // x faces: tags 11-14 travel up from the top planes, 21-24 down from the bottom ones
        for (auto& m : W.sends) P.pipe[m.tag < 20 ? C - 1 : 0].sends.push_back(m);
        for (auto& m : W.recvs) P.pipe[m.tag < 20 ? C - 1 : 0].recvs.push_back(m);
        auto split = [&](const std::vector<BoxMsg>& v, std::vector<BoxMsg> HaloRound::*dst) {
            for (const auto& m : v) {
                if (m.dx) {
                    (P.pipe[m.dx < 0 ? C - 1 : 0].*dst).push_back(m);
                    continue;
                }
                for (int j = 0; j < C; ++j) {
                    BoxMsg p = m;
                    p.box = cut(m.box, j);
                    if (p.box.i0 <= p.box.i1) (P.pipe[j].*dst).push_back(p);
                }
            }
        };
        split(W.bsends, &HaloRound::bsends);
        split(W.brecvs, &HaloRound::brecvs);
        for (auto& g : P.pipe) pack_per_peer(g);
    }
};

}  // namespace

DeepHaloPlan plan_deep_halo(const Topology& t, bool self_x, int depth, int ghost, bool direct, int tile_rows,
                            int slabs) {
    Planner p{t, self_x, depth, depth - 1, ghost, {}};
    p.P.interior = t.compute_box();
    if (self_x && t.dims[1] == 1 && t.dims[2] == 1) return p.P;  // one rank: nothing to exchange
    p.P.rounds.resize(direct ? 1 : 3);
    if (!self_x) p.x_planes(p.P.rounds[0]);
    if (direct) p.direct_boxes(p.P.rounds[0]);
    else p.yz_round(p.P.rounds[1], 1), p.yz_round(p.P.rounds[2], 2);
    p.shells(tile_rows);
    if (slabs > 0 && direct) p.pipe(slabs);
    return p.P;
}

}  // namespace wave3d
