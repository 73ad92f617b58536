// Deep-halo plan of the temporal-blocking sweeps (host only: no HIP, no device pointers).
//
// Which rank sends which planes and boxes to whom after a sweep of `depth` layers, with which
// tags and in which order — a pure function of the topology, planned here so that it runs (and
// is tested) without a GPU. The solver allocates one device buffer per entry of `bufs` and
// resolves every box message as buffer base + offset.
//
// One transport round (HaloRound) moves x planes in place plus staged boxes:
//   --halo rounds: three dependent rounds — the x planes, then the y boxes over the full x
//                  extent (ghosts included), then the z boxes over both, so edges and corners
//                  arrive without diagonal messages; every box is a message of its own tag;
//   --halo direct: one round — every face, edge and corner region straight from the rank that
//                  owns it, the boxes of one peer packed back to back into one message (tag
//                  kPeerTag on both ends);
//   --overlap pipe: the direct round cut into one group per x slab of the sweep.
// Every send meets exactly one receive of the same (peer, tag) and size, in the same per-peer
// order on both ends: tag-less RCCL matches messages by that order.
#pragma once

#include <vector>

#include "common.hpp"
#include "topology.hpp"

namespace wave3d {

constexpr int kAliasPlane = -1000;  // PlaneMsg::plane of a seam alias buffer
constexpr int kPeerTag = 199;       // one packed message per peer and direction of travel
constexpr int kShellTileK = 64;     // k tile of the sweeps (hip_kernels.hpp kTileK)

struct PlaneMsg {
    int peer, tag;
    int level;      // 0 = A level (D of the sweep), 1 = B level (C of the sweep)
    int plane;      // first logical plane; kAliasPlane = the alias buffer
    int nplanes;
};

// A region staged through a buffer. level: 0 = next A level, 1 = next B level, 2 / 3 = the seam
// alias plane of A / B (one plane at logical i = 0 wherever the alias buffer is the grid). box =
// source region on sends, ghost region on receives.
struct BoxMsg {
    int peer, tag;
    int level;
    Box box;
    int dx;         // x direction of travel as the receiver sees it (direct plan; 0 in y/z rounds)
    int buf;        // index into DeepHaloPlan::bufs ...
    size_t off;     // ... and the element offset of this box in it
};

// One transport message staged through a device buffer of `count` elements.
struct HaloBuf {
    int peer, tag;
    size_t count;
};

struct HaloRound {
    std::vector<PlaneMsg> sends, recvs;    // x planes, sent and received in place
    std::vector<BoxMsg> bsends, brecvs;    // packed before / unpacked after the transport
    std::vector<int> sbufs, rbufs;         // the buffers (bufs indices) that travel, in order
    bool empty() const { return sends.empty() && recvs.empty() && sbufs.empty() && rbufs.empty(); }
};

struct DeepHaloPlan {
    std::vector<HaloRound> rounds;  // direct: one; rounds: x, y, z (none: no deep halo at all)
    std::vector<HaloRound> pipe;    // --overlap pipe: one group per x slab
    std::vector<Box> slabs;         // the compute box cut into the sweep's x slabs
    std::vector<HaloBuf> bufs;      // every staging buffer of the rank
    bool alias[2] = {false, false}; // the rank holds seam alias planes of the A / the B level
    Box interior;                   // compute box minus what depends on a received ghost
    std::vector<Box> shell;
    bool any() const {
        for (const auto& r : rounds)
            if (!r.empty()) return true;
        return false;
    }
};

// The compute box `c` minus `in`, as up to six boxes: the x shells (full j/k extent) first, then
// y (full k extent), then z; nx = how many are x shells. An empty interior gives `c` itself.
struct ShellSplit {
    std::vector<Box> shell;
    int nx = 0;
};
ShellSplit split_shells(const Box& c, const Box& in);

// self_x: the face plan's (the periodic x neighbour is this rank and wraps locally); depth: layers
// per sweep (3 or 4); ghost: ghost depth of the storage; tile_rows: rows of the sweep's tile (the
// j shells are whole tiles); slabs: x slabs of the pipelined sweep (0 = no pipe; direct only).
DeepHaloPlan plan_deep_halo(const Topology& t, bool self_x, int depth, int ghost, bool direct, int tile_rows,
                            int slabs);

}  // namespace wave3d
