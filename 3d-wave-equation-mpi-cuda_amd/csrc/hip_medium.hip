// Heterogeneous-medium kernels: the 2.5-D marching step with a per-node coefficient field,
// point-source injection and receiver sampling (interface: hip_medium.hpp).
//
//  * k_march_m: k_march's design (hip_kernels.hip) — a 256-thread workgroup owns a (4R) x 64
//    tile of the (j,k) plane and marches along i, u^{n-1} rolling through four register slots,
//    the current plane staged in a double-buffered LDS tile (one barrier per plane), u^{n-2}
//    prefetched one plane ahead, non-temporal stores with the periodic self-wrap fused in — plus
//    a fourth stream: m = c^2 tau^2 at the lane's own nodes, prefetched one plane ahead in a
//    two-slot register ring like u^{n-2} (no LDS: only the centre node's m enters the update).
//    No analytic tables and no fused halo packing; the per-step statistic is max |u|.
//    TAPER: the damped leapfrog of an absorbing sponge, u = G ((2 u1 - G u2) + m lap) with the
//    separable G = gx[i] (gy[j] gz[k]): gy gz is one register per lane row, formed before the
//    march, gx[i] a wave-uniform scalar load fetched one plane ahead. No further stream.
//  * k_march_mh: the same march with a star stencil of half-width M = 2 or 4 per axis (space
//    orders 4 and 8): a (2M + 2)-slot u^{n-1} ring, an M-deep LDS halo and odd reflection at the
//    Dirichlet faces (described at the kernel).
//  * k_march_mb: k_march_m with a variable density: the operator div(b grad u) with the buoyancy
//    b = 1 / rho as a fifth stream that rolls through registers and LDS like u^{n-1} (described at
//    the kernel). It alone has the scatter and Born-add modes of Born modelling with a density
//    perturbation.
//  * all three march kernels have the save, image and Born modes of the adjoint-state gradient and
//    of Born modelling and the two illumination modes (MarchMode; hip_medium.hpp describes them), and
//    are built from the tile skeleton of march_tile.hpp and the per-mode pieces below, each written once.
//    The launcher checks a step against one table of per-mode rules (kMediumModes).
//  * k_inject / k_record: one thread per source entry / receiver.
//
// FP contraction is off (-ffp-contract=off + the pragmas in stencil_math.hpp and in every helper
// here that does arithmetic: the pragma is lexical): every operation is rounded on its own in the
// order of ops/reference.py step_medium, so fp64 results are bitwise those of the PyTorch oracle,
// and a uniform m == coef gives k_march's bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include <algorithm>

#include "device_common.hpp"
#include "hip_medium.hpp"
#include "march_tile.hpp"

namespace wave3d {
namespace {

template <class T>
struct MediumParams : TileParams<T> {
    const T* u1;
    const T* u2;
    const T* m;
    T* u;
    int ei0, ei1;
    int w_lo[2], w_hi[2], w_sh[2];  // wrap_ranges
    u64* err;
    const T *gx, *gy, *gz;  // TAPER: sponge factors per axis, storage indexing (X+2, Y+2, Z+2 values)
    T* lap_out;             // kSave: receives lap(u1) at the box nodes (strides of u)
    const T* q;             // kImage: the grid multiplied with the centre value of u1 ... (kScatter: db, below)
    T* acc;                 // ... and the grid the product is added to, at the box nodes
    const T* dm;            // kBorn: the coefficient perturbation; u receives + dm * q (q as above)
                            // kScatter (k_march_mb): lap_out receives dm * lap + m * r, r = D_db u1 with the
                            // buoyancy perturbation db, a level like b, in q; kBornAdd: u receives + q
    T* illum;               // kIllum, kSaveIllum: h = h + lap * lap at the box nodes (strides of u)
};

// The streams of a MODE (MarchMode; hip_medium.hpp describes the modes) other than kPlain (FIRST = false
// only), each behind `if constexpr`, at the lane's own nodes, masked like the stores of u and without the
// periodic wrap: one write-once stream (kSave: lap_out); a read-once stream (q) and a read-modify-write one
// (kImage: acc); two read-once streams (kBorn: q and dm, no store beside u's); a read-once stream dm, a
// write-once stream lap_out = s_out, and db handled like b, described at the kernel (kScatter); one
// read-once stream, q = s (kBornAdd); one more read-modify-write stream, like image mode's acc without its
// q (kIllum, kSaveIllum: illum).
constexpr bool saves_lap(int mode) { return mode == kSave || mode == kSaveIllum; }
constexpr bool illuminates(int mode) { return mode == kIllum || mode == kSaveIllum; }

constexpr int kNt = 2;  // cache policy of the read-once and write-once streams: non-temporal

// The extra read streams of image mode (q and acc), Born mode (q and dm), scatter mode (dm alone),
// Born-add mode (q = s alone) and the illumination modes (h alone, in the `a` ring), at the lane's own
// nodes: two-slot register rings prefetched one plane ahead like m; plane x in slot (x - ib) & 1.
template <class T, int R, int MODE>
struct AuxRings {
    static constexpr bool kQ = MODE == kImage || MODE == kBorn || MODE == kBornAdd;
    static constexpr bool kA = MODE == kImage || MODE == kBorn || MODE == kScatter || illuminates(MODE);
    T q[kQ ? 2 : 1][kQ ? R : 1], a[kA ? 2 : 1][kA ? R : 1];

    static __device__ __forceinline__ const T* second(const MediumParams<T>& p) {
        return MODE == kImage ? p.acc : illuminates(MODE) ? p.illum : p.dm;
    }
    // plane ib into slot 0
    __device__ __forceinline__ void prime(const Tile<T, R>& t, const MediumParams<T>& p, const unsigned (&os)[R]) {
        if constexpr (kQ && kA) {
            const auto rQ = t.prs(p.q, t.ib), rA = t.prs(second(p), t.ib);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                q[0][r] = bld<T, kNt>(rQ, os[r]);
                a[0][r] = bld<T, kNt>(rA, os[r]);
                q[1][r] = a[1][r] = T(0);
            }
        } else if constexpr (kQ) {
            const auto rQ = t.prs(p.q, t.ib);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                q[0][r] = bld<T, kNt>(rQ, os[r]);
                q[1][r] = T(0);
            }
        } else if constexpr (kA) {
            const auto rA = t.prs(second(p), t.ib);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a[0][r] = bld<T, kNt>(rA, os[r]);
                a[1][r] = T(0);
            }
        }
    }
    // plane i + 1 into slot H1
    template <int H1>
    __device__ __forceinline__ void prefetch(Ph<H1>, const Tile<T, R>& t, const MediumParams<T>& p, int i,
                                             bool more, const unsigned (&os)[R]) {
        if constexpr (kQ && kA) {
            const auto rQ = t.next_rsrc(p.q, i, 1, more), rA = t.next_rsrc(second(p), i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                q[H1][r] = bld<T, kNt>(rQ, os[r]);
                a[H1][r] = bld<T, kNt>(rA, os[r]);
            }
        } else if constexpr (kQ) {
            const auto rQ = t.next_rsrc(p.q, i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) q[H1][r] = bld<T, kNt>(rQ, os[r]);
        } else if constexpr (kA) {
            const auto rA = t.next_rsrc(second(p), i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) a[H1][r] = bld<T, kNt>(rA, os[r]);
        }
    }
    // the values of the current plane (slot H0) at row r; 0, and unused, in the other modes
    template <int H0>
    __device__ __forceinline__ T qv(Ph<H0>, int r) const {
        if constexpr (kQ) return q[H0][r];
        else return T(0);
    }
    template <int H0>
    __device__ __forceinline__ T av(Ph<H0>, int r) const {
        if constexpr (kA) return a[H0][r];
        else return T(0);
    }
};

// Sponge: gyz[r] = gy[j] gz[k] (rounded) of the lane's rows; lanes and rows past the grid read
// the last table entry (their stores are masked). gxn = gx of the next plane to compute:
// i + 1 <= X + 1 is always inside the table. TAPER = false: no table is touched, factors of 1
// that medium_update never uses.
template <class T, int R, bool TAPER>
struct Sponge {
    T gyz[TAPER ? R : 1];
    T gxn = T(1);

    __device__ __forceinline__ Sponge(const Tile<T, R>& t, const MediumParams<T>& p) {
        if constexpr (TAPER) {
#pragma clang fp contract(off)
            const T gzk = p.gz[min(t.k, p.kmax)];
#pragma unroll
            for (int r = 0; r < R; ++r) gyz[r] = ldconst(p.gy, min(t.row(r), p.jmax)) * gzk;
            gxn = ldconst(p.gx, t.ib);
        }
    }
    // gx of plane i; fetches plane i + 1's
    __device__ __forceinline__ T next(const MediumParams<T>& p, int i) {
        const T gxi = gxn;
        if constexpr (TAPER) gxn = ldconst(p.gx, i + 1);
        return gxi;
    }
    __device__ __forceinline__ T yz(int r) const {
        if constexpr (TAPER) return gyz[r];
        else return T(1);
    }
};

// The new value of a node: centre c = u1, u2, the (density-weighted) Laplacian, m; sponge factors
// gxi, gyz (TAPER); Born mode's a = dm and q; Born-add mode's q = s, the scattering term as stored.
template <class T, bool FIRST, bool TAPER, int MODE>
__device__ __forceinline__ T medium_update(T c, T u2, T lap, T m, T gxi, T gyz, T a, T q) {
#pragma clang fp contract(off)
    static_assert(MODE == kPlain || !FIRST, "save / image / Born modes: leapfrog steps only");
    if constexpr (FIRST) {
        const T half_m = T(0.5) * m;  // exact
        const T v = taylor_first(c, lap, half_m);
        if constexpr (TAPER) return (gxi * gyz) * v;
        else return v;
    } else if constexpr (MODE == kBorn || MODE == kBornAdd) {
        const T pr = MODE == kBorn ? a * q : q;  // dm q, rounded before the add; or s itself
        if constexpr (TAPER) {
            const T g = gxi * gyz;
            return g * (leapfrog(c, g * u2, lap, m) + pr);
        } else {
            return leapfrog(c, u2, lap, m) + pr;
        }
    } else if constexpr (TAPER) {
        const T g = gxi * gyz;
        return g * leapfrog(c, g * u2, lap, m);
    } else {
        return leapfrog(c, u2, lap, m);
    }
}

// What a mode stores beside u: kSave the Laplacian, kImage the new acc = a + c q (a = acc), kScatter
// the scattering term a lap + m q (a = dm, q = r = D_db u1), both products rounded before the add
template <class T, int MODE>
__device__ __forceinline__ T side_value(T c, T lap, T a, T q, T m = T(0)) {
#pragma clang fp contract(off)
    if constexpr (saves_lap(MODE)) {
        return lap;
    } else if constexpr (MODE == kImage) {
        const T pr = c * q;
        return a + pr;
    } else if constexpr (MODE == kScatter) {
        const T p1 = a * lap, p2 = m * q;
        return p1 + p2;
    } else {
        return T(0);
    }
}

// The new illumination of a node, a + lap lap (a = h), the product rounded before the add; 0, and
// unused, in the other modes
template <class T, int MODE>
__device__ __forceinline__ T illum_value(T lap, T a) {
#pragma clang fp contract(off)
    if constexpr (illuminates(MODE)) {
        const T pr = lap * lap;
        return a + pr;
    } else {
        return T(0);
    }
}

// stores of plane i: own plane + fused periodic wrap (buffer stores, masked lanes dropped), the
// mode's side stream xv (side_value) and the illumination modes' hx (illum_value)
template <int MODE, class T, int R>
__device__ __forceinline__ void store_plane(const Tile<T, R>& t, const MediumParams<T>& p, int i, const T (&vv)[R],
                                            const T (&xv)[R], const T (&hx)[R], const unsigned (&os)[R]) {
    const auto rs = t.prs(p.u, i);
#pragma unroll
    for (int r = 0; r < R; ++r) bst<kNt>(vv[r], rs, os[r]);
#pragma unroll
    for (int g = 0; g < 2; ++g)
        if (i >= p.w_lo[g] && i <= p.w_hi[g]) {
            const auto rw = t.prs(p.u, i + p.w_sh[g]);
#pragma unroll
            for (int r = 0; r < R; ++r) bst<kNt>(vv[r], rw, os[r]);
        }
    if constexpr (saves_lap(MODE) || MODE == kImage || MODE == kScatter) {
        const auto rx = t.prs(MODE == kImage ? p.acc : p.lap_out, i);
#pragma unroll
        for (int r = 0; r < R; ++r) bst<kNt>(xv[r], rx, os[r]);
    }
    if constexpr (illuminates(MODE)) {
        const auto rh = t.prs(p.illum, i);
#pragma unroll
        for (int r = 0; r < R; ++r) bst<kNt>(hx[r], rh, os[r]);
    }
}

// the step's statistic over the box nodes of plane i: ma = max |u| on the planes [ei0, ei1], chk =
// the sum of the values (commit_errors: nonfinite flag)
template <class T, int R>
__device__ __forceinline__ void plane_stats(const MediumParams<T>& p, int i, const T (&vv)[R],
                                            const bool (&valid)[R], T& chk, T& ma) {
#pragma clang fp contract(off)
    const bool erow = i >= p.ei0 && i <= p.ei1;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (!valid[r]) continue;
        chk += vv[r];
        if (erow) ma = max_abs(ma, vv[r]);
    }
}

// R = rows (j) per lane; the workgroup tile is (4R) x 64. NTM = non-temporal loads of m.
// Register slots as in k_march: u1(x) -> (x - ib + 1) & 3; u2(x), m(x), halo(x) and the LDS
// buffer -> (x - ib) & 1; the i loop is unrolled by 4 with the phase as a constant.
// TAPER = false compiles to the undamped kernel (every use of the tables is `if constexpr`).
template <class T, bool FIRST, int R, bool NTM, bool TAPER, int MODE = kPlain>
__global__ void __launch_bounds__(kThreads) k_march_m(const MediumParams<T> p) {
    constexpr int kTJ = kWaves * R;
    __shared__ T lds[2][kTJ + 2][kLW];
    const Tile<T, R> t(p);
    const int lane = t.lane, w = t.w, ib = t.ib;

    unsigned oa[R], ou2[R], os[R];
    bool valid[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = t.row(r);
        valid[r] = t.owns(j);
        oa[r] = t.boff(j, t.k, t.kload && j <= p.jmax);
        ou2[r] = t.boff(j, t.k, !FIRST && valid[r]);
        os[r] = t.boff(j, t.k, valid[r]);  // stores, and the loads of m
    }
    const HaloCell h = halo_cell(t);
    constexpr int kMAux = NTM ? kNt : 0;

    T u1[4][R], u2[2][R], mm[2][R];
    T hv[2];
    AuxRings<T, R, MODE> aux;
    aux.prime(t, p, os);
    {
        const auto r0 = t.prs(p.u1, ib - 1), r1 = t.prs(p.u1, ib), r2 = t.prs(p.u1, ib + 1);
        const auto q0 = t.prs(p.u2, ib), m0 = t.prs(p.m, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u1[0][r] = bld<T>(r0, oa[r]);
            u1[1][r] = bld<T>(r1, oa[r]);
            u1[2][r] = bld<T>(r2, oa[r]);
            u1[3][r] = T(0);
            u2[0][r] = FIRST ? T(0) : bld<T>(q0, ou2[r]);
            u2[1][r] = T(0);
            mm[0][r] = bld<T, kMAux>(m0, os[r]);
            mm[1][r] = T(0);
        }
        hv[0] = bld<T>(r1, h.hoff);
        hv[1] = T(0);
    }
    Sponge<T, R, TAPER> sponge(t, p);
    T ma = T(kErrInit), chk = T(0);

    auto plane = [&](auto phase, const int i) {
        constexpr int P = decltype(phase)::value;
        constexpr int S0 = P & 3, S1 = (P + 1) & 3, S2 = (P + 2) & 3, S3 = (P + 3) & 3;
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        // prefetch u1(i+2) (own rows), u1(i+1) (halo), u2(i+1), m(i+1)
        {
            const bool more = i < t.ie;
            const auto rN = t.next_rsrc(p.u1, i, 2, more), rH = t.next_rsrc(p.u1, i, 1, more);
            const auto rU = t.next_rsrc(p.u2, i, 1, more), rM = t.next_rsrc(p.m, i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u1[S3][r] = bld<T>(rN, oa[r]);
                if (!FIRST) u2[H1][r] = bld<T>(rU, ou2[r]);
                mm[H1][r] = bld<T, kMAux>(rM, os[r]);
            }
            hv[H1] = bld<T>(rH, h.hoff);
            aux.prefetch(Ph<H1>{}, t, p, i, more, os);
        }

        // stage plane i
#pragma unroll
        for (int r = 0; r < R; ++r) lds[H0][1 + w * R + r][1 + lane] = u1[S1][r];
        if (h.hon) lds[H0][h.hrow][h.hcol] = hv[H0];
        __syncthreads();

        const T gxi = sponge.next(p, i);
        T vv[R], xv[R], hx[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int lr = 1 + w * R + r;
            const T c = u1[S1][r];
            const T jm = r == 0 ? lds[H0][lr - 1][1 + lane] : u1[S1][r - 1];
            const T jp = r == R - 1 ? lds[H0][lr + 1][1 + lane] : u1[S1][r + 1];
            const T km = lds[H0][lr][lane];
            const T kp = lds[H0][lr][lane + 2];
            const T lap =
                laplace7_cr(c, u1[S0][r], u1[S2][r], jm, jp, km, kp, p.hx2, p.hy2, p.hz2, p.yx2, p.yy2, p.yz2);
            const T a = aux.av(Ph<H0>{}, r), q = aux.qv(Ph<H0>{}, r);
            xv[r] = side_value<T, MODE>(c, lap, a, q);
            hx[r] = illum_value<T, MODE>(lap, a);
            vv[r] = medium_update<T, FIRST, TAPER, MODE>(c, u2[H0][r], lap, mm[H0][r], gxi, sponge.yz(r), a, q);
        }
        store_plane<MODE>(t, p, i, vv, xv, hx, os);
        plane_stats(p, i, vv, valid, chk, ma);
    };
    march_planes<4>(ib, t.ie, plane);
    // slot 1 keeps its initial key: atomicMax with that same key
    commit_errors(ma, T(kErrInit), chk, p.err);
}

// ---- space orders 4 and 8: k_march_mh ------------------------------------------------------
// Central second-derivative weights of the star stencil of half-width M: double quotients of
// integers, cast to T by the kernel (ops/reference.py star_weights forms the same values).
constexpr double star_weight(int M, int d) {
    return M == 1   ? (d == 0 ? -2.0 : 1.0)
           : M == 2 ? (d == 0 ? -5.0 / 2.0 : d == 1 ? 4.0 / 3.0 : -1.0 / 12.0)
                    : (d == 0   ? -205.0 / 72.0
                       : d == 1 ? 8.0 / 5.0
                       : d == 2 ? -1.0 / 5.0
                       : d == 3 ? 8.0 / 315.0
                                : -1.0 / 560.0);
}

template <class T>
struct MediumParamsH : MediumParams<T> {
    int mj0, mj1, mk0, mk1;  // reflecting faces (storage indices); -+2^29 = none on that side
};

// k_march_m's design with a star stencil of half-width M (2 or 4) per axis: the same tile, march,
// streams, stores, statistic and masking. What differs:
//  * the u1 ring holds the planes i-M .. i+M and the prefetch slot, NS = 2M + 2 register slots per
//    row; plane x lives in slot (x - ib + M) % NS, and the i loop is unrolled by NS so that every
//    slot index is a constant (no in-flight load is ever copied);
//  * the LDS tile carries an M-deep halo in j and k, (4R + 2M) x (64 + 2M) per buffer, no corners;
//    its 2M 64 + 4R 2M halo cells are dealt to the 256 threads, NH cells each, prefetched one plane
//    ahead like k_march_m's single cell;
//  * every load of u1, own node or halo, goes through `src`: a node beyond a reflecting face f is
//    read at 2f - j and negated when it is staged (odd reflection, an exact negation); a node with
//    no source in the plane gets kOOB (reads 0). The host has checked that each node a box node
//    reaches has a source, so 0 never enters a stored value. The x neighbours of the lane's own
//    nodes come from the ring unreflected: only box nodes use them, and those lie inside the faces.
// Per node and axis: t = c_0 v, t = t + c_d (p_-d + p_+d) for d = 1 .. M; the j neighbours of a
// lane's own rows come from its registers, the rest and all k neighbours from LDS.
template <class T, int M, bool FIRST, int R, bool TAPER, int MODE = kPlain>
__global__ void __launch_bounds__(kThreads) k_march_mh(const MediumParamsH<T> p) {
    constexpr int kTJ = kWaves * R;
    constexpr int NS = 2 * M + 2;
    constexpr int LR = kTJ + 2 * M, LC = kTK + 2 * M;
    constexpr int kHaloJ = 2 * M * kTK, kHaloK = kTJ * 2 * M;
    constexpr int NH = (kHaloJ + kHaloK + kThreads - 1) / kThreads;
    static_assert(M == 2 || M == 4, "orders 4 and 8");
    __shared__ T lds[2][LR][LC];
    const Tile<T, R> t(p);
    const int lane = t.lane, w = t.w, ib = t.ib, kb = t.kb, jt = t.jt;

    // byte offset of the source of u1(j, kk) in a plane block and whether it is negated
    auto src = [&](int j, int kk, bool& neg) {
        neg = false;
        if (j < p.mj0) j = 2 * p.mj0 - j, neg = !neg;
        else if (j > p.mj1) j = 2 * p.mj1 - j, neg = !neg;
        if (kk < p.mk0) kk = 2 * p.mk0 - kk, neg = !neg;
        else if (kk > p.mk1) kk = 2 * p.mk1 - kk, neg = !neg;
        return t.boff(j, kk, j >= 0 && j <= p.jmax && kk >= 0 && kk <= p.kmax);
    };

    unsigned oa[R], ou2[R], os[R];
    bool valid[R], ng[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = t.row(r);
        valid[r] = t.owns(j);
        oa[r] = src(j, t.k, ng[r]);
        ou2[r] = t.boff(j, t.k, !FIRST && valid[r]);
        os[r] = t.boff(j, t.k, valid[r]);  // stores, and the loads of m
    }

    // halo cells of this thread: cell c = h 256 + tid; the first 2M 64 are the rows jt-M .. jt-1 and
    // jt+TJ .. jt+TJ+M-1, the next TJ 2M the columns kb-M .. kb-1 and kb+64 .. kb+64+M-1
    unsigned hoff[NH];
    int hidx[NH];  // LDS cell (element index in a buffer), -1 = none
    bool hng[NH];
#pragma unroll
    for (int h = 0; h < NH; ++h) {
        const int c = h * kThreads + int(threadIdx.x);
        int j = 0, kk = 0;
        hidx[h] = -1;
        hng[h] = false;
        hoff[h] = kOOB;
        if (c < kHaloJ) {
            const int hr = c / kTK, col = c % kTK;
            j = hr < M ? jt - M + hr : jt + kTJ + hr - M;
            kk = kb + col;
            hidx[h] = (hr < M ? hr : kTJ + hr) * LC + M + col;
        } else if (c < kHaloJ + kHaloK) {
            const int c2 = c - kHaloJ;
            const int rr = c2 / (2 * M), hc = c2 % (2 * M);
            j = jt + rr;
            kk = hc < M ? kb - M + hc : kb + kTK + hc - M;
            hidx[h] = (M + rr) * LC + (hc < M ? hc : kTK + hc);
        }
        if (hidx[h] >= 0) hoff[h] = src(j, kk, hng[h]);
    }

    T u1[NS][R], u2[2][R], mm[2][R];
    T hv[2][NH];
    AuxRings<T, R, MODE> aux;
    aux.prime(t, p, os);
    {
        // planes ib-M .. ib+M into slots 0 .. 2M (the host keeps the boxes M planes inside)
#pragma unroll
        for (int s = 0; s <= 2 * M; ++s) {
            const auto rp = t.prs(p.u1, ib - M + s);
#pragma unroll
            for (int r = 0; r < R; ++r) u1[s][r] = bld<T>(rp, oa[r]);
            if (s == M) {
#pragma unroll
                for (int h = 0; h < NH; ++h) {
                    hv[0][h] = bld<T>(rp, hoff[h]);
                    hv[1][h] = T(0);
                }
            }
        }
        const auto q0 = t.prs(p.u2, ib), m0 = t.prs(p.m, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u1[NS - 1][r] = T(0);
            u2[0][r] = FIRST ? T(0) : bld<T>(q0, ou2[r]);
            u2[1][r] = T(0);
            mm[0][r] = bld<T, kNt>(m0, os[r]);
            mm[1][r] = T(0);
        }
    }
    Sponge<T, R, TAPER> sponge(t, p);
    T ma = T(kErrInit), chk = T(0);
    T* const lds0 = &lds[0][0][0];

    auto plane = [&](auto phase, const int i) {
#pragma clang fp contract(off)
        constexpr int P = decltype(phase)::value;
        constexpr int SC = (P + M) % NS;          // plane i
        constexpr int SN = (P + 2 * M + 1) % NS;  // plane i+M+1, prefetched here
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        {
            const bool more = i < t.ie;
            const auto rN = t.next_rsrc(p.u1, i, M + 1, more), rH = t.next_rsrc(p.u1, i, 1, more);
            const auto rU = t.next_rsrc(p.u2, i, 1, more), rM = t.next_rsrc(p.m, i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u1[SN][r] = bld<T>(rN, oa[r]);
                if (!FIRST) u2[H1][r] = bld<T>(rU, ou2[r]);
                mm[H1][r] = bld<T, kNt>(rM, os[r]);
            }
#pragma unroll
            for (int h = 0; h < NH; ++h) hv[H1][h] = bld<T>(rH, hoff[h]);
            aux.prefetch(Ph<H1>{}, t, p, i, more, os);
        }

        // stage plane i, reflected nodes negated
        T cs[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            cs[r] = ng[r] ? -u1[SC][r] : u1[SC][r];
            lds[H0][M + w * R + r][M + lane] = cs[r];
        }
#pragma unroll
        for (int h = 0; h < NH; ++h)
            if (hidx[h] >= 0) lds0[H0 * (LR * LC) + hidx[h]] = hng[h] ? -hv[H0][h] : hv[H0][h];
        __syncthreads();

        const T gxi = sponge.next(p, i);
        T vv[R], xv[R], hx[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int lr = M + w * R + r;
            const T c = u1[SC][r];
            T tx = T(star_weight(M, 0)) * c, ty = tx, tz = tx;
#pragma unroll
            for (int d = 1; d <= M; ++d) {
                const T wd = T(star_weight(M, d));
                tx = tx + wd * (u1[(SC + NS - d) % NS][r] + u1[(SC + d) % NS][r]);
                const T jm = r - d >= 0 ? cs[r - d >= 0 ? r - d : 0] : lds[H0][lr - d][M + lane];
                const T jp = r + d < R ? cs[r + d < R ? r + d : 0] : lds[H0][lr + d][M + lane];
                ty = ty + wd * (jm + jp);
                tz = tz + wd * (lds[H0][lr][M + lane - d] + lds[H0][lr][M + lane + d]);
            }
            const T lap = sum_div<T>(tx, ty, tz, p);
            const T a = aux.av(Ph<H0>{}, r), q = aux.qv(Ph<H0>{}, r);
            xv[r] = side_value<T, MODE>(c, lap, a, q);
            hx[r] = illum_value<T, MODE>(lap, a);
            vv[r] = medium_update<T, FIRST, TAPER, MODE>(c, u2[H0][r], lap, mm[H0][r], gxi, sponge.yz(r), a, q);
        }
        store_plane<MODE>(t, p, i, vv, xv, hx, os);
        plane_stats(p, i, vv, valid, chk, ma);
    };
    march_planes<NS>(ib, t.ie, plane);
    commit_errors(ma, T(kErrInit), chk, p.err);
}

// ---- variable density: k_march_mb ----------------------------------------------------------
template <class T>
struct MediumParamsB : MediumParams<T> {
    const T* b;  // buoyancy 1 / rho, a level with the strides of u1 (x ghost planes filled)
};

// One axis of div(b grad u): the difference of the two face fluxes, a face buoyancy being the
// arithmetic mean of its two nodes' (the product with 0.5 is exact); ops/reference.py
// laplace_density has the same operations in the same order.
template <class T>
__device__ __forceinline__ T flux_diff(T c, T um, T up, T bc, T bm, T bp) {
#pragma clang fp contract(off)
    const T fp = (T(0.5) * (bc + bp)) * (up - c);
    const T fm = (T(0.5) * (bc + bm)) * (c - um);
    return fp - fm;
}

// k_march_m (non-temporal m, R rows per lane) with lap(u1) replaced by
// D_b u1 = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2, t = flux_diff per axis: the same tile, march,
// streams, sponge, modes (kSave stores D_b u1), stores, statistic and masking. The fifth stream b
// needs its six neighbours, so it is handled exactly like u1: b at the lane's own nodes rolls
// through a 4-slot register ring (planes i-1, i, i+1 and the prefetch slot, the phase a template
// constant), plane i of b is staged in a second double-buffered LDS tile of the same shape, and
// each halo lane loads its one b cell per plane beside its u1 cell, with the same offset and the
// same kOOB masking. The plane's one barrier covers both tiles. The j neighbours of a lane's inner
// rows come from registers for b as for u1. The loads of b are ordinary temporal loads (the halo
// lines are reused across tiles through L2); m stays non-temporal. A masked b reads 0: it only
// enters nodes whose stores are masked too. 40 B per node in fp64 (20 B in fp32).
// Scatter mode (kScatter) also evaluates r = D_db u1 with the same operations, db's values in b's
// place, and stores s = dm D_b u1 + m r where save mode stores D_b u1. db needs its six neighbours
// too, so it is a third copy of b's machinery: a 4-slot register ring, a third LDS tile of the same
// shape under the same barrier, one more halo cell per lane and plane with b's offset and masking,
// temporal loads. dm is a read-once stream (AuxRings). u and the statistic are the plain step's.
// 64 B per node in fp64: u1, u2, m, b, db, dm read, u and s written. Born-add mode (kBornAdd) reads
// the stored s back: 48 B.
template <class T, bool FIRST, int R, bool TAPER, int MODE = kPlain>
__global__ void __launch_bounds__(kThreads) k_march_mb(const MediumParamsB<T> p) {
    constexpr int kTJ = kWaves * R;
    constexpr bool SC = MODE == kScatter;
    __shared__ T lds[2][kTJ + 2][kLW];
    __shared__ T ldb[2][kTJ + 2][kLW];
    __shared__ T ldd[SC ? 2 : 1][SC ? kTJ + 2 : 1][SC ? kLW : 1];  // db's tile, scatter mode only
    const Tile<T, R> t(p);
    const int lane = t.lane, w = t.w, ib = t.ib;

    unsigned oa[R], ou2[R], os[R];
    bool valid[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = t.row(r);
        valid[r] = t.owns(j);
        oa[r] = t.boff(j, t.k, t.kload && j <= p.jmax);  // u1 and b
        ou2[r] = t.boff(j, t.k, !FIRST && valid[r]);
        os[r] = t.boff(j, t.k, valid[r]);  // stores, and the loads of m
    }
    const HaloCell h = halo_cell(t);  // one cell per plane and tile

    T u1[4][R], bb[4][R], u2[2][R], mm[2][R];
    T hv[2], hb[2];
    T dd[SC ? 4 : 1][SC ? R : 1], hd[2];  // db's ring and halo cell
    AuxRings<T, R, MODE> aux;
    aux.prime(t, p, os);
    if constexpr (SC) {  // db travels in p.q (MediumParams)
        const auto d0 = t.prs(p.q, ib - 1), d1 = t.prs(p.q, ib), d2 = t.prs(p.q, ib + 1);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            dd[0][r] = bld<T>(d0, oa[r]);
            dd[1][r] = bld<T>(d1, oa[r]);
            dd[2][r] = bld<T>(d2, oa[r]);
            dd[3][r] = T(0);
        }
        hd[0] = bld<T>(d1, h.hoff);
        hd[1] = T(0);
    }
    {
        const auto r0 = t.prs(p.u1, ib - 1), r1 = t.prs(p.u1, ib), r2 = t.prs(p.u1, ib + 1);
        const auto b0 = t.prs(p.b, ib - 1), b1 = t.prs(p.b, ib), b2 = t.prs(p.b, ib + 1);
        const auto q0 = t.prs(p.u2, ib), m0 = t.prs(p.m, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u1[0][r] = bld<T>(r0, oa[r]);
            u1[1][r] = bld<T>(r1, oa[r]);
            u1[2][r] = bld<T>(r2, oa[r]);
            u1[3][r] = T(0);
            bb[0][r] = bld<T>(b0, oa[r]);
            bb[1][r] = bld<T>(b1, oa[r]);
            bb[2][r] = bld<T>(b2, oa[r]);
            bb[3][r] = T(0);
            u2[0][r] = FIRST ? T(0) : bld<T>(q0, ou2[r]);
            u2[1][r] = T(0);
            mm[0][r] = bld<T, kNt>(m0, os[r]);
            mm[1][r] = T(0);
        }
        hv[0] = bld<T>(r1, h.hoff);
        hb[0] = bld<T>(b1, h.hoff);
        hv[1] = hb[1] = T(0);
    }
    Sponge<T, R, TAPER> sponge(t, p);
    T ma = T(kErrInit), chk = T(0);

    auto plane = [&](auto phase, const int i) {
        constexpr int P = decltype(phase)::value;
        constexpr int S0 = P & 3, S1 = (P + 1) & 3, S2 = (P + 2) & 3, S3 = (P + 3) & 3;
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        // prefetch u1, b (i+2, own rows), u1, b (i+1, halo), u2(i+1), m(i+1)
        {
            const bool more = i < t.ie;
            const auto rN = t.next_rsrc(p.u1, i, 2, more), rH = t.next_rsrc(p.u1, i, 1, more);
            const auto bN = t.next_rsrc(p.b, i, 2, more), bH = t.next_rsrc(p.b, i, 1, more);
            const auto rU = t.next_rsrc(p.u2, i, 1, more), rM = t.next_rsrc(p.m, i, 1, more);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u1[S3][r] = bld<T>(rN, oa[r]);
                bb[S3][r] = bld<T>(bN, oa[r]);
                if (!FIRST) u2[H1][r] = bld<T>(rU, ou2[r]);
                mm[H1][r] = bld<T, kNt>(rM, os[r]);
            }
            hv[H1] = bld<T>(rH, h.hoff);
            hb[H1] = bld<T>(bH, h.hoff);
            if constexpr (SC) {
                const auto dN = t.next_rsrc(p.q, i, 2, more), dH = t.next_rsrc(p.q, i, 1, more);
#pragma unroll
                for (int r = 0; r < R; ++r) dd[S3][r] = bld<T>(dN, oa[r]);
                hd[H1] = bld<T>(dH, h.hoff);
            }
            aux.prefetch(Ph<H1>{}, t, p, i, more, os);
        }

        // stage plane i of u1 and b (and db): one barrier for all tiles
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lds[H0][1 + w * R + r][1 + lane] = u1[S1][r];
            ldb[H0][1 + w * R + r][1 + lane] = bb[S1][r];
            if constexpr (SC) ldd[H0][1 + w * R + r][1 + lane] = dd[S1][r];
        }
        if (h.hon) {
            lds[H0][h.hrow][h.hcol] = hv[H0];
            ldb[H0][h.hrow][h.hcol] = hb[H0];
            if constexpr (SC) ldd[H0][h.hrow][h.hcol] = hd[H0];
        }
        __syncthreads();

        const T gxi = sponge.next(p, i);
        T vv[R], xv[R], hx[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int lr = 1 + w * R + r;
            const T c = u1[S1][r], bc = bb[S1][r];
            const T jm = r == 0 ? lds[H0][lr - 1][1 + lane] : u1[S1][r - 1];
            const T jp = r == R - 1 ? lds[H0][lr + 1][1 + lane] : u1[S1][r + 1];
            const T bjm = r == 0 ? ldb[H0][lr - 1][1 + lane] : bb[S1][r - 1];
            const T bjp = r == R - 1 ? ldb[H0][lr + 1][1 + lane] : bb[S1][r + 1];
            const T tx = flux_diff(c, u1[S0][r], u1[S2][r], bc, bb[S0][r], bb[S2][r]);
            const T ty = flux_diff(c, jm, jp, bc, bjm, bjp);
            const T tz = flux_diff(c, lds[H0][lr][lane], lds[H0][lr][lane + 2], bc, ldb[H0][lr][lane],
                                   ldb[H0][lr][lane + 2]);
            const T lap = sum_div<T>(tx, ty, tz, p);
            const T a = aux.av(Ph<H0>{}, r);
            T q = aux.qv(Ph<H0>{}, r);
            if constexpr (SC) {  // q = r = D_db u1
                const T dc = dd[S1][r];
                const T djm = r == 0 ? ldd[H0][lr - 1][1 + lane] : dd[S1][r - 1];
                const T djp = r == R - 1 ? ldd[H0][lr + 1][1 + lane] : dd[S1][r + 1];
                const T rx = flux_diff(c, u1[S0][r], u1[S2][r], dc, dd[S0][r], dd[S2][r]);
                const T ry = flux_diff(c, jm, jp, dc, djm, djp);
                const T rz = flux_diff(c, lds[H0][lr][lane], lds[H0][lr][lane + 2], dc, ldd[H0][lr][lane],
                                       ldd[H0][lr][lane + 2]);
                q = sum_div<T>(rx, ry, rz, p);
            }
            xv[r] = side_value<T, MODE>(c, lap, a, q, mm[H0][r]);
            hx[r] = illum_value<T, MODE>(lap, a);
            vv[r] = medium_update<T, FIRST, TAPER, MODE>(c, u2[H0][r], lap, mm[H0][r], gxi, sponge.yz(r), a, q);
        }
        store_plane<MODE>(t, p, i, vv, xv, hx, os);
        plane_stats(p, i, vv, valid, chk, ma);
    };
    march_planes<4>(ib, t.ie, plane);
    commit_errors(ma, T(kErrInit), chk, p.err);
}

// The runtime (first, taper, mode) of a launch as template arguments: pick(FIRST, TAPER, MODE),
// three integral constants, returns the kernel of one family for them. The modes exist for the
// leapfrog step only. Every instantiation has 4 rows per lane unless a variant asks for 2
// (`make resources`: no scratch in any of them).
template <class F>
auto select_march(bool first, bool taper, int mode, F pick) {
    auto with_taper = [&](auto fi, auto mo) {
        return taper ? pick(fi, std::true_type{}, mo) : pick(fi, std::false_type{}, mo);
    };
    switch (mode) {
        case kSave: return with_taper(std::false_type{}, Ph<kSave>{});
        case kImage: return with_taper(std::false_type{}, Ph<kImage>{});
        case kBorn: return with_taper(std::false_type{}, Ph<kBorn>{});
        case kScatter: return with_taper(std::false_type{}, Ph<kScatter>{});
        case kBornAdd: return with_taper(std::false_type{}, Ph<kBornAdd>{});
        case kIllum: return with_taper(std::false_type{}, Ph<kIllum>{});
        case kSaveIllum: return with_taper(std::false_type{}, Ph<kSaveIllum>{});
        default: break;
    }
    return first ? with_taper(std::true_type{}, Ph<kPlain>{}) : with_taper(std::false_type{}, Ph<kPlain>{});
}

__device__ __forceinline__ bool node_offset(const NodeGrid& g, const int* nodes, int e, int& i, i64& row) {
    i = nodes[3 * e];
    const int j = nodes[3 * e + 1], k = nodes[3 * e + 2];
    row = i64(j) * g.sj + k;
    // the host validates the lists; a node outside the storage is skipped, never dereferenced
    return i >= 0 && i < g.nx && j >= 0 && j < g.ny && k >= 0 && k < g.nz;
}

template <class T>
__global__ void k_inject(T* u, const T* m, NodeGrid gr, const int* nodes, const T* g, int n, Wrap wrap) {
#pragma clang fp contract(off)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    int i;
    i64 row;
    if (!node_offset(gr, nodes, e, i, row)) return;
    const i64 o = i64(i) * gr.si + row;
    const T add = m[o] * g[e];
    const T v = u[o] + add;
    u[o] = v;
#pragma unroll
    for (int q = 0; q < kMaxWrap; ++q)
        if (wrap.src[q] >= 1 && i == wrap.src[q] && wrap.dst[q] >= 0 && wrap.dst[q] < gr.nx)
            u[i64(wrap.dst[q]) * gr.si + row] = v;
}

template <class T>
__global__ void k_record(const T* u, NodeGrid gr, const int* nodes, T* out, int n) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    int i;
    i64 row;
    if (!node_offset(gr, nodes, e, i, row)) return;
    out[e] = u[i64(i) * gr.si + row];
}

// k_march_m: the plain step exists in four variants (R, NTM); the modes for the default one only
template <class T>
void (*march_m_kernel(bool first, bool taper, int mode, int variant))(const MediumParams<T>) {
    return select_march(first, taper, mode, [&](auto fi, auto ta, auto mo) -> void (*)(const MediumParams<T>) {
        constexpr bool FIRST = decltype(fi)::value, TAPER = decltype(ta)::value;
        constexpr int MODE = decltype(mo)::value;
        constexpr int RD = 4;  // march_rows_per_thread()
        if constexpr (MODE == kScatter || MODE == kBornAdd) return nullptr;  // k_march_mb only (kMediumModes rejects the call)
        else if constexpr (MODE != kPlain) return k_march_m<T, FIRST, RD, true, TAPER, MODE>;
        else switch (variant & 3) {
                case 1: return k_march_m<T, FIRST, RD, true, TAPER>;
                case 2: return k_march_m<T, FIRST, 2, false, TAPER>;
                case 3: return k_march_m<T, FIRST, 2, true, TAPER>;
                default: return k_march_m<T, FIRST, RD, false, TAPER>;
            }
    });
}

template <class T, int M>
void (*march_mh_kernel(bool first, bool taper, int mode))(const MediumParamsH<T>) {
    return select_march(first, taper, mode, [](auto fi, auto ta, auto mo) -> void (*)(const MediumParamsH<T>) {
        constexpr int MODE = decltype(mo)::value;
        if constexpr (MODE == kScatter || MODE == kBornAdd) return nullptr;  // k_march_mb only (kMediumModes rejects the call)
        else return k_march_mh<T, M, decltype(fi)::value, 4, decltype(ta)::value, MODE>;
    });
}

template <class T>
void (*march_mb_kernel(bool first, bool taper, int mode))(const MediumParamsB<T>) {
    return select_march(first, taper, mode, [](auto fi, auto ta, auto mo) -> void (*)(const MediumParamsB<T>) {
        return k_march_mb<T, decltype(fi)::value, 4, decltype(ta)::value, decltype(mo)::value>;
    });
}

}  // namespace

int medium_variant() {
    static const int v = [] {
        const char* e = std::getenv("WAVE3D_MEDIUM_VARIANT");
        const std::string s = e ? e : "";
        if (s == "plain") return 0;
        if (s == "r2") return 2;
        if (s == "r2nt") return 3;
        W3D_REQUIRE(s.empty() || s == "nt", "WAVE3D_MEDIUM_VARIANT must be nt, plain, r2 or r2nt, not " + s);
        // non-temporal m loads, 4 rows per lane: the fastest of the four on MI355X at N = 512
        // (profiles/medium_march.txt)
        return 1;
    }();
    return v;
}

double medium_weight(int order, int d) {
    W3D_REQUIRE((order == 2 || order == 4 || order == 8) && d >= 0 && d <= order / 2, "no such stencil weight");
    return star_weight(order / 2, d);
}

namespace {

// The rules of the modes, one row each, in MarchMode's order: all that launch_step_medium checks of a
// step's mode. The grids of a step, as bits: the levels a mode grid may have to stay clear of, then the
// mode grids in MediumStep's order.
enum : unsigned {
    gU = 1u << 0, gU1 = 1u << 1, gU2 = 1u << 2, gM = 1u << 3, gB = 1u << 4,
    gLapOut = 1u << 5, gQ = 1u << 6, gAcc = 1u << 7, gDm = 1u << 8, gDb = 1u << 9, gSOut = 1u << 10,
    gSAdd = 1u << 11, gIllum = 1u << 12
};
constexpr int kFirstModeGrid = 5, kStepGrids = 13;
constexpr const char* kGridNames[kStepGrids] = {"u", "u1", "u2", "m", "b", "lap_out", "q", "acc", "dm", "db",
                                                "s_out", "sadd", "illum"};
enum : unsigned { kFamM = 1, kFamMH = 2, kFamMB = 4, kFamAll = 7 };  // k_march_m, k_march_mh, k_march_mb
struct ModeRule {
    const char* name;
    unsigned grids;        // the mode grids it takes: each of them non-null, every other mode grid null
    bool on_first;         // runs on the Taylor start
    unsigned families;     // the kernel families that have it
    bool default_variant;  // at order 2: instantiated for variant 1 alone (nt, 4 rows per lane)
    // a grid (one bit) that the step writes, and the grids read or written beside it (its own plane and, for u,
    // the wrap planes) that it must not share memory with; a null one does not count. 0: no such rule
    unsigned apart, from;
};
constexpr unsigned kLevels = gU | gU1 | gU2 | gM | gB;
constexpr ModeRule kMediumModes[kMarchModes] = {
    {"plain", 0, true, kFamAll, false, 0, 0},
    {"save", gLapOut, false, kFamAll, true, 0, 0},
    {"image", gQ | gAcc, false, kFamAll, true, 0, 0},
    {"born", gQ | gDm, false, kFamAll, true, gU, gQ | gDm},
    {"scatter", gSOut | gDm | gDb, false, kFamMB, true, gSOut, kLevels | gDm | gDb},
    {"born_add", gSAdd, false, kFamMB, true, gU, gSAdd},
    {"illum", gIllum, false, kFamAll, true, gIllum, kLevels},
    {"save_illum", gLapOut | gIllum, false, kFamAll, true, gIllum, kLevels | gLapOut},
};

// The mode checks of a step that runs in kernel family `family` with the (resolved) variant; span: the
// elements a grid covers.
template <class T>
void check_mode(const MediumStep<T>& st, unsigned family, int variant, i64 span) {
    W3D_REQUIRE(st.mode >= kPlain && st.mode < kMarchModes, "no such mode: " + std::to_string(int(st.mode)));
    const ModeRule& r = kMediumModes[st.mode];
    const std::string mode = std::string(r.name) + " mode";
    const T* grid[kStepGrids] = {st.u,  st.u1, st.u2, st.m,     st.b,    st.lap_out, st.q,
                                 st.acc, st.dm, st.db, st.s_out, st.sadd, st.illum};
    for (int g = kFirstModeGrid; g < kStepGrids; ++g) {
        const bool takes = r.grids >> g & 1;
        W3D_REQUIRE(takes == (grid[g] != nullptr),
                    mode + (takes ? " needs " : " cannot be combined with ") + kGridNames[g]);
    }
    W3D_REQUIRE(r.on_first || !st.first, mode + ": not on the Taylor start (first)");
    W3D_REQUIRE(r.families & family, mode + (family == kFamMH ? " exists for space order 2 only"
                                                              : " needs the buoyancy b (variable density)"));
    W3D_REQUIRE(!r.default_variant || variant == 1 || st.order != 2,
                mode + " is instantiated for the default variant only (nt, 4 rows per lane)");
    const int g = r.apart ? __builtin_ctz(r.apart) : 0;
    for (int o = 0; o < kStepGrids; ++o)
        W3D_REQUIRE(!(r.from >> o & 1) || !grid[o] || !overlaps<T>(grid[g], grid[o], span),
                    mode + ": " + kGridNames[g] + " shares memory with " + kGridNames[o]);
}

}  // namespace

const char* march_mode_name(int mode) {
    W3D_REQUIRE(mode >= kPlain && mode < kMarchModes, "no such mode: " + std::to_string(mode));
    return kMediumModes[mode].name;
}

template <class T>
void launch_step_medium(const MediumStep<T>& st, hipStream_t s) {
    const bool first = st.first;
    const GridView& gv = st.gv;
    const Box* boxes = st.boxes;
    const int nbox = st.nbox, order = st.order;
    const int* mirror = st.mirror;
    const T* b = st.b;
    W3D_REQUIRE(order == 2 || order == 4 || order == 8, "space order must be 2, 4 or 8, not " + std::to_string(order));
    W3D_REQUIRE(!b || order == 2, "variable density (b) exists for space order 2 only");
    const int M = order / 2;
    const bool taper = st.gx || st.gy || st.gz;
    W3D_REQUIRE(!taper || (st.gx && st.gy && st.gz), "the sponge needs all three tables");
    W3D_REQUIRE(!taper || gv.G == 1, "sponge tables: one ghost layer");
    W3D_REQUIRE(nbox >= 1 && nbox <= kMaxBoxes, "bad box count");
    W3D_REQUIRE(march_rows_per_thread() == 4, "k_march_m is instantiated for 4 rows per lane");
    W3D_REQUIRE(gv.si > 0 && gv.si * i64(sizeof(T)) < (1ll << 31), "plane larger than a buffer descriptor's range");
    W3D_REQUIRE(gv.sj >= gv.Z + 2 * gv.G && gv.si >= i64(gv.Y + 2 * gv.G) * gv.sj, "strides smaller than the grid");
    const int variant = st.variant < 0 ? medium_variant() : st.variant;
    W3D_REQUIRE(!b || variant == 1, "variable density (b) is instantiated for the default variant only (nt, 4 rows per lane)");
    const i64 span = i64(gv.X + 2 * gv.G - 1) * gv.si + i64(gv.Y + 2 * gv.G - 1) * gv.sj + gv.Z + 2 * gv.G;
    check_mode(st, M > 1 ? kFamMH : b ? kFamMB : kFamM, variant, span);
    const int mode = st.mode;
    // reflecting faces of k_march_mh: (j_lo, j_hi, k_lo, k_hi), +-2^29 where there is none
    int mir[4] = {kNoMirror, -kNoMirror, kNoMirror, -kNoMirror};
    bool has[4] = {false, false, false, false};
    if (M > 1) {
        W3D_REQUIRE(gv.G == 1 && gv.poff == 0, "orders 4 and 8: one ghost layer in the grid view");
        for (int f = 0; f < 4; ++f) {
            if (!mirror || mirror[f] == kNoMirror) continue;
            const int top = f < 2 ? gv.jmax() : gv.kmax();
            W3D_REQUIRE(mirror[f] >= 0 && mirror[f] <= top, "mirror face outside the storage");
            // the farthest reflected index, M - 1 nodes inside the face, must exist
            W3D_REQUIRE((f & 1) ? mirror[f] - (M - 1) >= 0 : mirror[f] + (M - 1) <= top,
                        "a node reflected at a mirror face would leave the storage");
            mir[f] = mirror[f];
            has[f] = true;
        }
        for (int a = 0; a < 2; ++a)
            W3D_REQUIRE(!(has[2 * a] && has[2 * a + 1]) || mir[2 * a + 1] - mir[2 * a] >= M,
                        "mirror faces nearer than the stencil's half-width");
    }
    MediumParams<T> p{};
    fill_tile_params(p, gv, st.h2);
    p.u1 = st.u1;
    p.u2 = st.u2;
    p.m = st.m;
    p.u = st.u;
    p.ei0 = st.ei0;
    p.ei1 = st.ei1;
    const Wrap& wrap = st.wrap;
    for (int q = 0; q < kMaxWrap; ++q)
        W3D_REQUIRE(wrap.src[q] < 1 || (wrap.src[q] <= gv.X && wrap.dst[q] >= 1 - gv.G && wrap.dst[q] <= gv.X + gv.G),
                    "wrap plane outside the grid");
    wrap_ranges(wrap, p.w_lo, p.w_hi, p.w_sh);
    p.err = st.err;
    p.gx = st.gx;
    p.gy = st.gy;
    p.gz = st.gz;
    // the kernels' slots: lap_out doubles as kScatter's s_out, q as kScatter's db and kBornAdd's s
    p.lap_out = mode == kScatter ? st.s_out : st.lap_out;
    p.q = mode == kBornAdd ? st.sadd : mode == kScatter ? st.db : st.q;
    p.acc = st.acc;
    p.dm = st.dm;
    p.illum = st.illum;
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
        W3D_REQUIRE(bx.i0 >= 1 && bx.i1 <= gv.X && bx.j0 >= 1 && bx.j1 <= gv.Y && bx.k0 >= 1 && bx.k1 <= gv.Z,
                    "step box outside the owned region");
        if (M > 1) {
            W3D_REQUIRE(bx.i0 >= M && bx.i1 <= gv.X + 1 - M, "step box nearer than order / 2 to the storage edge in x");
            const int lo[2] = {bx.j0, bx.k0}, hi[2] = {bx.j1, bx.k1}, top[2] = {gv.jmax(), gv.kmax()};
            for (int a = 0; a < 2; ++a) {
                W3D_REQUIRE(has[2 * a] ? lo[a] > mir[2 * a] : lo[a] >= M,
                            has[2 * a] ? "step box not strictly inside its mirror faces"
                                       : "step box nearer than order / 2 to an unmirrored storage edge");
                W3D_REQUIRE(has[2 * a + 1] ? hi[a] < mir[2 * a + 1] : hi[a] <= top[a] - M,
                            has[2 * a + 1] ? "step box not strictly inside its mirror faces"
                                           : "step box nearer than order / 2 to an unmirrored storage edge");
            }
        }
    }
    // 4 rows per lane in every kernel but k_march_m's two-row variants
    const int tj_rows = kWaves * (M == 1 && (variant & 2) ? 2 : 4);
    const int total = plan_boxes(p, boxes, nbox, tj_rows, st.chunk);
    if (p.nbox == 0) return;
    if (M > 1) {
        MediumParamsH<T> ph{};
        static_cast<MediumParams<T>&>(ph) = p;
        ph.mj0 = mir[0], ph.mj1 = mir[1], ph.mk0 = mir[2], ph.mk1 = mir[3];
        auto kh = M == 2 ? march_mh_kernel<T, 2>(first, taper, mode) : march_mh_kernel<T, 4>(first, taper, mode);
        hipLaunchKernelGGL(kh, dim3(total), dim3(kThreads), 0, s, ph);
        HIP_OK(hipGetLastError());
        return;
    }
    if (b) {
        MediumParamsB<T> pb{};
        static_cast<MediumParams<T>&>(pb) = p;
        pb.b = b;
        hipLaunchKernelGGL(march_mb_kernel<T>(first, taper, mode), dim3(total), dim3(kThreads), 0, s, pb);
        HIP_OK(hipGetLastError());
        return;
    }
    hipLaunchKernelGGL(march_m_kernel<T>(first, taper, mode, variant), dim3(total), dim3(kThreads), 0, s, p);
    HIP_OK(hipGetLastError());
}

template <class T>
void launch_inject(T* u, const T* m, const GridView& gv, const int* nodes, const T* g, int n,
                   const Wrap& wrap, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_inject<T>, dim3(cdiv(n, 64)), dim3(64), 0, s, u, m, node_grid(gv), nodes, g, n, wrap);
    HIP_OK(hipGetLastError());
}

template <class T>
void launch_record(const T* u, const GridView& gv, const int* nodes, T* out, int n, hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_record<T>, dim3(cdiv(n, 64)), dim3(64), 0, s, u, node_grid(gv), nodes, out, n);
    HIP_OK(hipGetLastError());
}

#define W3D_MEDIUM_INST(T)                                                                             \
    template void launch_step_medium<T>(const MediumStep<T>&, hipStream_t);                            \
    template void launch_inject<T>(T*, const T*, const GridView&, const int*, const T*, int,           \
                                   const Wrap&, hipStream_t);                                          \
    template void launch_record<T>(const T*, const GridView&, const int*, T*, int, hipStream_t);
W3D_MEDIUM_INST(double)
W3D_MEDIUM_INST(float)

}  // namespace wave3d
