"""Deep-halo plan of the temporal-blocking sweeps (csrc/deep_halo.hpp), on the CPU.

The property the exchange relies on — every send meets exactly one receive of the same size, in
the same per-peer order (tag-less RCCL matches by that order) — plus the layout of what arrives:
packed peer buffers, alias planes, ghost coverage of the direct plan, shells and pipe groups.
"""
import itertools

import numpy as np
import pytest

TILE_ROWS = 16
# (N, dims, x_self)
CASES = [(40, (4, 1, 1), False), (47, (2, 1, 1), False), (47, (2, 2, 2), False), (40, (1, 2, 2), False),
         (40, (1, 1, 2), False), (40, (3, 1, 2), False), (40, (1, 1, 1), True)]


def count(b):
    return max(0, b[1] - b[0] + 1) * max(0, b[3] - b[2] + 1) * max(0, b[5] - b[4] + 1)


@pytest.fixture(scope="module")
def plans(C):
    cache = {}

    def get(N, dims, x_self, depth, direct):
        key = (N, dims, x_self, depth, direct)
        if key not in cache:
            P = dims[0] * dims[1] * dims[2]
            slabs = 4 if N == 47 and direct else 0  # 24 planes per x rank >= 4 x (depth + 1)
            cache[key] = [C.deep_halo_plan(N, P, r, list(dims), depth, direct, x_self, TILE_ROWS, slabs)
                          for r in range(P)]
        return cache[key]

    return get


def params():
    for (N, dims, xs), depth, direct in itertools.product(CASES, (3, 4), (True, False)):
        yield pytest.param(N, dims, xs, depth, direct,
                           id=f"N{N}-{'x'.join(map(str, dims))}{'-xself' if xs else ''}-d{depth}-"
                              f"{'direct' if direct else 'rounds'}")


def messages(plan, rnd, send):
    """The three message kinds of one round of one rank as {kind: [(peer, tag, elements)]}, in
    list order; a plane message counts its planes times the rank's (Y, Z) plane."""
    yz = (plan["ext"][1], plan["ext"][2])
    return {
        "planes": [(m[0], m[1], (m[4],) + yz) for m in rnd["sends" if send else "recvs"]],
        "boxes": [(m[0], m[1], count(m[3])) for m in rnd["bsends" if send else "brecvs"]],
        "bufs": [plan["bufs"][i] for i in rnd["sbufs" if send else "rbufs"]],
    }


def check_matching_and_order(ps, rounds_of):
    """rounds_of(plan) -> the rounds to check; every round is checked across all ranks."""
    for q in range(len(rounds_of(ps[0]))):
        snd = [messages(p, rounds_of(p)[q], True) for p in ps]
        rcv = [messages(p, rounds_of(p)[q], False) for p in ps]
        for kind in ("planes", "boxes", "bufs"):
            for r in range(len(ps)):
                for (peer, tag, n) in snd[r][kind]:
                    match = [m for m in rcv[peer][kind] if m[0] == r and m[1] == tag]
                    assert len(match) == 1 and match[0][2] == n, (kind, q, r, peer, tag)
                for (peer, tag, n) in rcv[r][kind]:  # and no receive waits for nothing
                    assert sum(1 for m in snd[peer][kind] if m[0] == r and m[1] == tag) == 1, (kind, q, r, tag)
                for peer in range(len(ps)):
                    s_tags = [m[1] for m in snd[r][kind] if m[0] == peer]
                    r_tags = [m[1] for m in rcv[peer][kind] if m[0] == r]
                    assert s_tags == r_tags, (kind, q, r, peer)


def check_packing(ps, rounds_of):
    for q in range(len(rounds_of(ps[0]))):
        for r, p in enumerate(ps):
            rnd = rounds_of(p)[q]
            for lst, ids in ((rnd["bsends"], rnd["sbufs"]), (rnd["brecvs"], rnd["rbufs"])):
                assert sorted({m[5] for m in lst}) == sorted(ids)  # every box in a buffer that travels
                for i in ids:
                    off = 0
                    for m in (m for m in lst if m[5] == i):
                        assert m[0] == p["bufs"][i][0] and m[6] == off  # its peer's buffer, back to back
                        off += count(m[3])
                    assert off == p["bufs"][i][2] and off > 0
            for i in rnd["sbufs"]:
                peer, tag, _ = p["bufs"][i]
                prnd = rounds_of(ps[peer])[q]
                there = [j for j in prnd["rbufs"] if ps[peer]["bufs"][j][:2] == (r, tag)]
                assert len(there) == 1
                mine = [count(m[3]) for m in rnd["bsends"] if m[5] == i]
                theirs = [count(m[3]) for m in prnd["brecvs"] if m[5] == there[0]]
                assert mine == theirs


@pytest.mark.parametrize("N,dims,x_self,depth,direct", params())
def test_sends_meet_receives(plans, N, dims, x_self, depth, direct):
    ps = plans(N, dims, x_self, depth, direct)
    assert all(len(p["rounds"]) == (1 if direct else 3) for p in ps)
    assert any(rnd[k] for p in ps for rnd in p["rounds"] for k in ("sends", "bsends"))  # not vacuous
    check_matching_and_order(ps, lambda p: p["rounds"])
    check_packing(ps, lambda p: p["rounds"])
    for p in ps:
        tags = {b[1] for rnd in p["rounds"] for b in (p["bufs"][i] for i in rnd["sbufs"] + rnd["rbufs"])}
        assert tags <= {p["peer_tag"]} if direct else p["peer_tag"] not in tags
        if direct:  # tag = 200 + 4 * direction + level, direction = 9 (dx + 1) + 3 (dy + 1) + (dz + 1)
            assert all(m[4] == (m[1] - 200) // 36 - 1 and m[2] == (m[1] - 200) % 4
                       for rnd in p["rounds"] for key in ("bsends", "brecvs") for m in rnd[key])


@pytest.mark.parametrize("N,dims,x_self,depth,direct", params())
def test_alias_boxes_lie_in_the_alias_plane(plans, N, dims, x_self, depth, direct):
    for p in plans(N, dims, x_self, depth, direct):
        for rnd in p["rounds"] + p["pipe"]:
            for m in rnd["brecvs"]:
                if m[2] >= 2:
                    assert p["alias"][m[2] - 2] and m[3][0] == 0 and m[3][1] == 0
            for m in rnd["recvs"]:
                if m[3] == p["alias_plane"]:
                    assert p["alias"][m[2]] and m[4] == 1


@pytest.mark.parametrize("N,dims,x_self,depth", [pytest.param(*c, d, id=f"N{c[0]}-{'x'.join(map(str, c[1]))}-d{d}")
                                                 for c in CASES for d in (3, 4)])
def test_direct_receives_tile_the_ghosts(plans, N, dims, x_self, depth):
    """Direct plan: the receive boxes of a level are pairwise disjoint and, with the x planes on
    owned (j,k), cover exactly the ghost cells of that level's depth that have a neighbour — but
    for the x ghosts at owned (j,k) of a rank that wraps x itself (the kernels' fused wrap)."""
    for p in plans(N, dims, x_self, depth, True):
        rnd = p["rounds"][0] if p["rounds"] else {"recvs": [], "brecvs": []}
        X, Y, Z = p["ext"]
        for level in (0, 1, 2, 3):
            D = depth if level % 2 == 0 else depth - 1
            got = np.zeros((X + 2 * D, Y + 2 * D, Z + 2 * D), dtype=np.int32)  # index = logical + D - 1

            def add(b):
                assert b[0] >= 1 - D and b[1] <= X + D and b[2] >= 1 - D and b[3] <= Y + D and b[4] >= 1 - D \
                    and b[5] <= Z + D and count(b) > 0, b
                got[b[0] + D - 1:b[1] + D, b[2] + D - 1:b[3] + D, b[4] + D - 1:b[5] + D] += 1

            for m in rnd["brecvs"]:
                if m[2] == level:
                    add(m[3])
            if level >= 2:
                assert got.max(initial=0) <= 1  # alias boxes: disjoint
                continue
            for m in rnd["recvs"]:
                if m[2] == level and m[3] != p["alias_plane"]:
                    add([m[3], m[3] + m[4] - 1, 1, Y, 1, Z])
            want = np.zeros_like(got)
            for d in itertools.product((-1, 0, 1), repeat=3):
                if d == (0, 0, 0) or any(d[a] and p["nbr"][a][(d[a] + 1) // 2] < 0 for a in (1, 2)):
                    continue
                if p["self_x"] and d[0] and not d[1] and not d[2]:
                    continue
                sl = tuple(slice(0, D) if d[a] < 0 else slice(D + p["ext"][a], 2 * D + p["ext"][a]) if d[a] > 0
                           else slice(D, D + p["ext"][a]) for a in range(3))
                want[sl] = 1
            assert np.array_equal(got, want), (level, np.argwhere(got != want)[:4] - D + 1)


@pytest.mark.parametrize("N,dims,x_self,depth,direct", params())
def test_shells_partition_the_compute_box(plans, N, dims, x_self, depth, direct):
    for p in plans(N, dims, x_self, depth, direct):
        c = p["compute_box"]
        got = np.zeros((p["ext"][0] + 2, p["ext"][1] + 2, p["ext"][2] + 2), dtype=np.int32)
        for b in p["shell"] + ([p["interior"]] if count(p["interior"]) else []):
            assert count(b) > 0
            got[b[0]:b[1] + 1, b[2]:b[3] + 1, b[4]:b[5] + 1] += 1
        want = np.zeros_like(got)
        want[c[0]:c[1] + 1, c[2]:c[3] + 1, c[4]:c[5] + 1] = 1
        assert np.array_equal(got, want)


@pytest.mark.parametrize("dims", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("depth", [3, 4])
def test_pipe_groups(plans, dims, depth):
    ps = plans(47, dims, False, depth, True)
    for p in ps:
        c, slabs = p["compute_box"], p["slabs"]
        assert len(slabs) == 4 == len(p["pipe"])
        assert slabs[0][0] == c[0] and slabs[-1][1] == c[1]
        for a, b in zip(slabs, slabs[1:]):
            assert b[0] == a[1] + 1
        assert all(s[2:] == c[2:] and s[1] - s[0] + 1 >= depth + 1 for s in slabs)
        whole = p["rounds"][0]
        for key in ("sends", "recvs"):  # every plane message in exactly one group
            assert sorted(m for g in p["pipe"] for m in g[key]) == sorted(whole[key])
        # a message goes with the slab that computes its source planes: what travels up (x faces of
        # tags 11-14, boxes with dx < 0) comes from the top planes = the last slab, what travels down
        # (tags 21-24, dx > 0) from the bottom planes = slab 0
        for j, g in enumerate(p["pipe"]):
            assert all(j == (3 if m[1] < 20 else 0) for key in ("sends", "recvs") for m in g[key])
            assert all(j == (3 if m[4] < 0 else 0) for key in ("bsends", "brecvs") for m in g[key] if m[4])
        assert all(10 < m[1] < 15 or 20 < m[1] < 25 for key in ("sends", "recvs") for m in whole[key])
        assert not dims[1] * dims[2] > 1 or any(m[4] for m in whole["bsends"])  # 2x2x2: dx != 0 boxes exist
        for key in ("bsends", "brecvs"):
            for m in whole[key]:
                parts = sorted(q[3] for g in p["pipe"] for q in g[key] if q[:3] == m[:3])
                assert parts and sum(count(b) for b in parts) == count(m[3])
                assert parts[0][0] == m[3][0] and parts[-1][1] == m[3][1]
                assert all(b[2:] == m[3][2:] for b in parts)
                assert all(b[0] == a[1] + 1 for a, b in zip(parts, parts[1:]))  # disjoint, no gap
            assert sum(len(g[key]) for g in p["pipe"]) >= len(whole[key])
            assert {q[:3] for g in p["pipe"] for q in g[key]} == {m[:3] for m in whole[key]}
    check_matching_and_order(ps, lambda p: p["pipe"])
    check_packing(ps, lambda p: p["pipe"])
