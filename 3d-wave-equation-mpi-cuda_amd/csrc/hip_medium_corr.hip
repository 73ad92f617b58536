// Face correlation of two fields, the accumulation of the density gradient dJ/drho of the medium
// solver's adjoint pass (interface: hip_medium.hpp, launch_face_corr).
//
//  * k_face_corr: acc = acc + C(a, v) at the box nodes, C the sum over a node's six faces of the
//    products of the two fields' differences across the face, each axis divided by its h^2. It is
//    k_march_mb's skeleton (hip_medium.hip; the shared pieces are in march_tile.hpp) with other
//    streams: both fields need their six neighbours, so both roll through registers and LDS the way
//    u1 and b do there, and acc is the one read-modify-write stream at the lane's own nodes. No u2,
//    m, taper, statistic or wrap.
//
// FP contraction is off (-ffp-contract=off + the pragmas in stencil_math.hpp): every operation is
// rounded on its own in the order of ops/reference.py face_correlation, so fp64 results are bitwise
// those of the PyTorch oracle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_common.hpp"
#include "hip_medium.hpp"
#include "march_tile.hpp"

namespace wave3d {
namespace {

template <class T>
struct CorrParams : TileParams<T> {
    const T* a;
    const T* v;
    T* acc;
};

// One axis of C(a, v): the two faces' products of differences, summed; ops/reference.py
// face_correlation has the same operations in the same order. Symmetric in (a, v) bit for bit.
template <class T>
__device__ __forceinline__ T face_pair(T ac, T am, T ap, T vc, T vm, T vp) {
#pragma clang fp contract(off)
    const T pp = (ap - ac) * (vp - vc);
    const T pm = (ac - am) * (vc - vm);
    return pp + pm;
}

// R = rows (j) per lane; the workgroup tile is (4R) x 64, marched along i in chunks. a and v at the
// lane's own nodes roll through 4-slot register rings (planes i-1, i, i+1 and the prefetch slot,
// the phase a template constant: no in-flight load is copied); plane i of each is staged in its
// own double-buffered LDS tile with the one-node j / k halo, every halo lane loading its one cell of
// each field per plane with the same offset; the plane's one barrier covers both tiles. The j
// neighbours of a lane's inner rows come from registers. acc is loaded non-temporally at the lane's
// own nodes one plane ahead (two-slot ring) and stored non-temporally; lanes outside the box carry
// kOOB (the load gives 0, the store is dropped), so nothing outside the boxes is written. A masked
// a or v reads 0: it only enters nodes whose stores are masked too. 32 B per node in fp64 (16 B in
// fp32): a, v, and acc read and written.
template <class T, int R>
__global__ void __launch_bounds__(kThreads) k_face_corr(const CorrParams<T> p) {
    constexpr int kTJ = kWaves * R;
    __shared__ T lda[2][kTJ + 2][kLW];
    __shared__ T ldv[2][kTJ + 2][kLW];
    const Tile<T, R> t(p);
    const int lane = t.lane, w = t.w, ib = t.ib;

    unsigned oa[R], os[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = t.row(r);
        oa[r] = t.boff(j, t.k, t.kload && j <= p.jmax);  // a and v
        os[r] = t.boff(j, t.k, t.owns(j));               // acc: loads and stores
    }
    const HaloCell h = halo_cell(t);  // one cell per plane and tile
    constexpr int kNt = 2;            // non-temporal: acc is read once and written once per call

    T aa[4][R], vv[4][R], cc[2][R];
    T ha[2], hv[2];
    {
        const auto a0 = t.prs(p.a, ib - 1), a1 = t.prs(p.a, ib), a2 = t.prs(p.a, ib + 1);
        const auto v0 = t.prs(p.v, ib - 1), v1 = t.prs(p.v, ib), v2 = t.prs(p.v, ib + 1);
        const auto c0 = t.prs(p.acc, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            aa[0][r] = bld<T>(a0, oa[r]);
            aa[1][r] = bld<T>(a1, oa[r]);
            aa[2][r] = bld<T>(a2, oa[r]);
            aa[3][r] = T(0);
            vv[0][r] = bld<T>(v0, oa[r]);
            vv[1][r] = bld<T>(v1, oa[r]);
            vv[2][r] = bld<T>(v2, oa[r]);
            vv[3][r] = T(0);
            cc[0][r] = bld<T, kNt>(c0, os[r]);
            cc[1][r] = T(0);
        }
        ha[0] = bld<T>(a1, h.hoff);
        hv[0] = bld<T>(v1, h.hoff);
        ha[1] = hv[1] = T(0);
    }

    auto plane = [&](auto phase, const int i) {
        constexpr int P = decltype(phase)::value;
        constexpr int S0 = P & 3, S1 = (P + 1) & 3, S2 = (P + 2) & 3, S3 = (P + 3) & 3;
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        // prefetch a, v (i+2, own rows), a, v (i+1, halo), acc(i+1)
        {
            const bool more = i < t.ie;
            const auto aN = t.next_rsrc(p.a, i, 2, more), aH = t.next_rsrc(p.a, i, 1, more);
            const auto vN = t.next_rsrc(p.v, i, 2, more), vH = t.next_rsrc(p.v, i, 1, more);
            const auto cN = t.next_rsrc(p.acc, i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                aa[S3][r] = bld<T>(aN, oa[r]);
                vv[S3][r] = bld<T>(vN, oa[r]);
                cc[H1][r] = bld<T, kNt>(cN, os[r]);
            }
            ha[H1] = bld<T>(aH, h.hoff);
            hv[H1] = bld<T>(vH, h.hoff);
        }

        // stage plane i of a and v: one barrier for both tiles
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lda[H0][1 + w * R + r][1 + lane] = aa[S1][r];
            ldv[H0][1 + w * R + r][1 + lane] = vv[S1][r];
        }
        if (h.hon) {
            lda[H0][h.hrow][h.hcol] = ha[H0];
            ldv[H0][h.hrow][h.hcol] = hv[H0];
        }
        __syncthreads();

        T out[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma clang fp contract(off)
            const int lr = 1 + w * R + r;
            const T ac = aa[S1][r], vc = vv[S1][r];
            const T ajm = r == 0 ? lda[H0][lr - 1][1 + lane] : aa[S1][r - 1];
            const T ajp = r == R - 1 ? lda[H0][lr + 1][1 + lane] : aa[S1][r + 1];
            const T vjm = r == 0 ? ldv[H0][lr - 1][1 + lane] : vv[S1][r - 1];
            const T vjp = r == R - 1 ? ldv[H0][lr + 1][1 + lane] : vv[S1][r + 1];
            const T tx = face_pair(ac, aa[S0][r], aa[S2][r], vc, vv[S0][r], vv[S2][r]);
            const T ty = face_pair(ac, ajm, ajp, vc, vjm, vjp);
            const T tz = face_pair(ac, lda[H0][lr][lane], lda[H0][lr][lane + 2], vc, ldv[H0][lr][lane],
                                   ldv[H0][lr][lane + 2]);
            out[r] = cc[H0][r] + sum_div<T>(tx, ty, tz, p);
        }
        {
            const auto rs = t.prs(p.acc, i);
#pragma unroll
            for (int r = 0; r < R; ++r) bst<kNt>(out[r], rs, os[r]);
        }
    };
    march_planes<4>(ib, t.ie, plane);
}

// rows per lane (`make resources`: no scratch in fp64 or fp32). Two rows in fp32 (66 VGPRs, 7 waves
// per SIMD instead of 108 and 4) measured slower on MI355X at N = 512: 0.453 against 0.438 ms
// (profiles/medium_density_gradient.txt)
constexpr int kCorrRows = 4;

}  // namespace

template <class T>
void launch_face_corr(const T* a, const T* v, T* acc, const GridView& gv, const Box* boxes, int nbox,
                      const double h2[3], int chunk, hipStream_t s) {
    W3D_REQUIRE(a && v && acc, "face correlation: null grid");
    W3D_REQUIRE(nbox >= 1 && nbox <= kMaxBoxes, "bad box count");
    W3D_REQUIRE(gv.G == 1 && gv.poff == 0, "face correlation: one ghost layer in the grid view");
    W3D_REQUIRE(gv.X >= 1 && gv.Y >= 1 && gv.Z >= 1, "grid needs at least one owned node per axis");
    W3D_REQUIRE(gv.si > 0 && gv.si * i64(sizeof(T)) < (1ll << 31), "plane larger than a buffer descriptor's range");
    W3D_REQUIRE(gv.sj >= gv.Z + 2 && gv.si >= i64(gv.Y + 2) * gv.sj, "strides smaller than the grid");
    W3D_REQUIRE(h2[0] > 0 && h2[1] > 0 && h2[2] > 0, "h2 = (hx2, hy2, hz2), all > 0");
    // acc is read and written while a and v are read: it must not share memory with either
    const i64 span = i64(gv.X + 1) * gv.si + i64(gv.Y + 1) * gv.sj + gv.Z + 2;  // elements a grid covers
    W3D_REQUIRE(!overlaps<T>(acc, a, span) && !overlaps<T>(acc, v, span),
                "face correlation: acc shares memory with a or v");
    CorrParams<T> p{};
    fill_tile_params(p, gv, h2);
    p.a = a;
    p.v = v;
    p.acc = acc;
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
        // k_march_m's box contract: every box node has its six neighbours inside the storage
        W3D_REQUIRE(bx.i0 >= 1 && bx.i1 <= gv.X && bx.j0 >= 1 && bx.j1 <= gv.Y && bx.k0 >= 1 && bx.k1 <= gv.Z,
                    "face correlation: box outside the owned region (it touches a storage edge)");
    }
    const int total = plan_boxes(p, boxes, nbox, kWaves * kCorrRows, chunk);
    if (p.nbox == 0) return;
    hipLaunchKernelGGL((k_face_corr<T, kCorrRows>), dim3(total), dim3(kThreads), 0, s, p);
    HIP_OK(hipGetLastError());
}

template void launch_face_corr<double>(const double*, const double*, double*, const GridView&, const Box*, int,
                                       const double[3], int, hipStream_t);
template void launch_face_corr<float>(const float*, const float*, float*, const GridView&, const Box*, int,
                                      const double[3], int, hipStream_t);

}  // namespace wave3d
