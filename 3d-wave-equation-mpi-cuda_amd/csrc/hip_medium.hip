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
//    the kernel).
//  * all three march kernels have the save, image and Born modes of the adjoint-state gradient and
//    of Born modelling (MarchMode below; hip_medium.hpp has the contract).
//  * k_inject / k_record: one thread per source entry / receiver.
//
// FP contraction is off (-ffp-contract=off + the pragmas in stencil_math.hpp): every operation
// is rounded on its own in the order of ops/reference.py step_medium, so fp64 results are
// bitwise those of the PyTorch oracle, and a uniform m == coef gives k_march's bits.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include <algorithm>

#include "device_common.hpp"
#include "hip_medium.hpp"

namespace wave3d {
namespace {

template <class T>
struct MediumParams {
    int xcd;  // XCD-aware tile order (xcd_swizzle)
    const T* u1;
    const T* u2;
    const T* m;
    T* u;
    i64 si;
    int sj;
    int poff;        // see GridView::poff
    int jmax, kmax;  // largest valid j / k index in storage
    int nbox;
    BoxLaunch box[kMaxBoxes];
    int ei0, ei1;
    int w_lo[2], w_hi[2], w_sh[2];  // wrap_ranges
    T hx2, hy2, hz2;
    T yx2, yy2, yz2;  // RN(1/h^2) in T for the correctly rounded constant division
    u64* err;
    const T *gx, *gy, *gz;  // TAPER: sponge factors per axis, storage indexing (X+2, Y+2, Z+2 values)
    T* lap_out;             // kSave: receives lap(u1) at the box nodes (strides of u)
    const T* q;             // kImage: the grid multiplied with the centre value of u1 ...
    T* acc;                 // ... and the grid the product is added to, at the box nodes
    const T* dm;            // kBorn: the coefficient perturbation; u receives + dm * q (q as above)
};

// k_march_m modes: the plain step; kSave also stores the Laplacian that entered the update; kImage
// also accumulates acc = acc + u1 * q (the imaging condition of the adjoint-state gradient); kBorn
// adds the scattering term dm * q to the update itself (Born / linearised modelling, image mode's
// transpose): u = G (((2 u1 - G u2) + m lap) + dm q).
enum MarchMode { kPlain = 0, kSave = 1, kImage = 2, kBorn = 3 };

// R = rows (j) per lane; the workgroup tile is (4R) x 64. NTM = non-temporal loads of m.
// Register slots as in k_march: u1(x) -> (x - ib + 1) & 3; u2(x), m(x), halo(x) and the LDS
// buffer -> (x - ib) & 1; the i loop is unrolled by 4 with the phase as a constant.
// TAPER = false compiles to the undamped kernel (every use of the tables is `if constexpr`).
// MODE (kSave / kImage: FIRST = false only) adds, likewise behind `if constexpr`, one write-once
// stream (lap_out), or a read-once stream (q) and a read-modify-write one (acc), both prefetched
// one plane ahead in two-slot rings like m; all at the lane's own nodes, masked like the stores
// of u and without the periodic wrap. kBorn (FIRST = false only) has two read-once streams in the
// same two rings, q and dm in acc's place, and no store beside u's.
template <class T, bool FIRST, int R, bool NTM, bool TAPER, int MODE = kPlain>
__global__ void __launch_bounds__(kThreads) k_march_m(const MediumParams<T> p) {
    constexpr int kTJ = kWaves * R;
    constexpr unsigned ES = sizeof(T);
    __shared__ T lds[2][kTJ + 2][kLW];

    const int bid = xcd_swizzle(blockIdx.x, gridDim.x, p.xcd);
    const int b = find_box(p, bid);
    const BoxLaunch B = p.box[b];
    int local = bid - B.block_begin;
    const int tk = local % B.tiles_k;
    local /= B.tiles_k;
    const int tj = local % B.tiles_j;
    const int ci = local / B.tiles_j;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kb = B.kbase + tk * kTK;
    const int k = kb + lane;
    const int jt = B.j0 + tj * kTJ;
    const int ib = B.i0 + ci * B.chunk;
    const int ie = min(B.i1, ib + B.chunk - 1);

    const bool kload = k <= p.kmax;
    const bool kin = k >= B.k0 && k <= B.k1;
    const i64 si = p.si;
    const unsigned pbytes = unsigned(si) * ES;
    // byte offset of (j,k) in a plane block (kOOB = masked: loads give 0, stores dropped)
    auto boff = [&](int j, int kk, bool ok) { return ok ? unsigned(j * p.sj + kk + p.poff) * ES : kOOB; };
    auto prs = [&](const T* base, int i) { return plane_rsrc(base + (i64(i) * si - p.poff), pbytes); };

    unsigned oa[R], ou2[R], os[R];
    bool valid[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = jt + w * R + r;
        valid[r] = kin && j <= B.j1;
        oa[r] = boff(j, k, kload && j <= p.jmax);
        ou2[r] = boff(j, k, !FIRST && valid[r]);
        os[r] = boff(j, k, valid[r]);  // stores, and the loads of m
    }

    // halo role of this lane: one LDS cell per plane
    int hrow = 0, hcol = 0;
    unsigned hoff = kOOB;
    bool hon = false;
    if (w == 0) {  // row jt-1
        hon = true;
        hoff = boff(jt - 1, k, kload);
        hrow = 0;
        hcol = 1 + lane;
    } else if (w == kWaves - 1) {  // row jt+TJ
        const int j = jt + kTJ;
        hon = true;
        hoff = boff(j, k, kload && j <= p.jmax);
        hrow = kTJ + 1;
        hcol = 1 + lane;
    } else if (w == 1) {  // columns kb-1 (lanes 0..TJ-1) and kb+64 (lanes 32..32+TJ-1)
        const int side = lane >> 5, rr = lane & 31;
        const int j = jt + rr;
        const int kk = side ? kb + kTK : kb - 1;
        hon = rr < kTJ;
        hoff = boff(j, kk, hon && j <= p.jmax && kk <= p.kmax);
        hrow = 1 + rr;
        hcol = side ? kTK + 1 : 0;
    }
    constexpr int kMAux = NTM ? 2 : 0;  // non-temporal m (read once per step)
    constexpr int kStAux = 2;           // non-temporal stores (write-once stream)

    static_assert(MODE == kPlain || !FIRST, "save / image / Born modes: leapfrog steps only");
    constexpr bool kImg = MODE == kImage, kBrn = MODE == kBorn;
    constexpr bool kTwo = kImg || kBrn;  // the two extra rings: q and acc (image) or q and dm (Born)
    T u1[4][R], u2[2][R], mm[2][R];
    T qq[kTwo ? 2 : 1][kTwo ? R : 1], aa[kTwo ? 2 : 1][kTwo ? R : 1];
    T hv[2];
    if constexpr (kTwo) {
        const auto rQ = prs(p.q, ib), rA = prs(kBrn ? p.dm : p.acc, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            qq[0][r] = bld<T, 2>(rQ, os[r]);
            aa[0][r] = bld<T, 2>(rA, os[r]);
            qq[1][r] = aa[1][r] = T(0);
        }
    }
    {
        const auto r0 = prs(p.u1, ib - 1), r1 = prs(p.u1, ib), r2 = prs(p.u1, ib + 1);
        const auto q0 = prs(p.u2, ib), m0 = prs(p.m, ib);
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
        hv[0] = bld<T>(r1, hoff);
        hv[1] = T(0);
    }
    const T hx2 = p.hx2, hy2 = p.hy2, hz2 = p.hz2;
    const T yx2 = p.yx2, yy2 = p.yy2, yz2 = p.yz2;

    // sponge: gyz[r] = gy[j] gz[k] (rounded) of the lane's rows; lanes and rows past the grid read
    // the last table entry (their stores are masked). gxn = gx of the next plane to compute:
    // i + 1 <= X + 1 is always inside the table.
    T gyz[TAPER ? R : 1];
    T gxn = T(1);
    if constexpr (TAPER) {
#pragma clang fp contract(off)
        const T gzk = p.gz[min(k, p.kmax)];
#pragma unroll
        for (int r = 0; r < R; ++r) gyz[r] = ldconst(p.gy, min(jt + w * R + r, p.jmax)) * gzk;
        gxn = ldconst(p.gx, ib);
    }

    T ma = T(kErrInit);
    T chk = T(0);  // sum of the values (commit_errors: nonfinite flag)

    auto plane = [&](auto phase, const int i) {
        constexpr int P = decltype(phase)::value;
        constexpr int S0 = P & 3, S1 = (P + 1) & 3, S2 = (P + 2) & 3, S3 = (P + 3) & 3;
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        // prefetch u1(i+2) (own rows), u1(i+1) (halo), u2(i+1), m(i+1); 0-record descriptors on
        // the last plane (loads return 0 without touching memory)
        {
            const bool more = i < ie;
            const unsigned nb = more ? pbytes : 0u;
            const int d2 = more ? 2 : 0, d1 = more ? 1 : 0;
            const auto rN = plane_rsrc(p.u1 + (i64(i + d2) * si - p.poff), nb);
            const auto rH = plane_rsrc(p.u1 + (i64(i + d1) * si - p.poff), nb);
            const auto rU = plane_rsrc(p.u2 + (i64(i + d1) * si - p.poff), nb);
            const auto rM = plane_rsrc(p.m + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u1[S3][r] = bld<T>(rN, oa[r]);
                if (!FIRST) u2[H1][r] = bld<T>(rU, ou2[r]);
                mm[H1][r] = bld<T, kMAux>(rM, os[r]);
            }
            hv[H1] = bld<T>(rH, hoff);
            if constexpr (kTwo) {
                const auto rQ = plane_rsrc(p.q + (i64(i + d1) * si - p.poff), nb);
                const auto rA = plane_rsrc((kBrn ? p.dm : p.acc) + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    qq[H1][r] = bld<T, 2>(rQ, os[r]);
                    aa[H1][r] = bld<T, 2>(rA, os[r]);
                }
            }
        }

        // stage plane i
#pragma unroll
        for (int r = 0; r < R; ++r) lds[H0][1 + w * R + r][1 + lane] = u1[S1][r];
        if (hon) lds[H0][hrow][hcol] = hv[H0];
        __syncthreads();

        const bool erow = i >= p.ei0 && i <= p.ei1;
        const T gxi = gxn;
        if constexpr (TAPER) gxn = ldconst(p.gx, i + 1);
        T vv[R];
        T xv[MODE == kSave || kImg ? R : 1];  // kSave: lap; kImage: the new acc
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int lr = 1 + w * R + r;
            const T c = u1[S1][r];
            const T jm = r == 0 ? lds[H0][lr - 1][1 + lane] : u1[S1][r - 1];
            const T jp = r == R - 1 ? lds[H0][lr + 1][1 + lane] : u1[S1][r + 1];
            const T km = lds[H0][lr][lane];
            const T kp = lds[H0][lr][lane + 2];
            const T lap = laplace7_cr(c, u1[S0][r], u1[S2][r], jm, jp, km, kp, hx2, hy2, hz2, yx2, yy2, yz2);
            if constexpr (MODE == kSave) xv[r] = lap;
            if constexpr (kImg) {
#pragma clang fp contract(off)
                const T pr = c * qq[H0][r];
                xv[r] = aa[H0][r] + pr;
            }
            if constexpr (FIRST) {
#pragma clang fp contract(off)
                const T half_m = T(0.5) * mm[H0][r];  // exact
                vv[r] = taylor_first(c, lap, half_m);
                if constexpr (TAPER) vv[r] = (gxi * gyz[r]) * vv[r];
            } else if constexpr (kBrn) {
#pragma clang fp contract(off)
                const T pr = aa[H0][r] * qq[H0][r];  // dm q, rounded before the add
                if constexpr (TAPER) {
                    const T g = gxi * gyz[r];
                    vv[r] = g * (leapfrog(c, g * u2[H0][r], lap, mm[H0][r]) + pr);
                } else {
                    vv[r] = leapfrog(c, u2[H0][r], lap, mm[H0][r]) + pr;
                }
            } else if constexpr (TAPER) {
#pragma clang fp contract(off)
                const T g = gxi * gyz[r];
                vv[r] = g * leapfrog(c, g * u2[H0][r], lap, mm[H0][r]);
            } else {
                vv[r] = leapfrog(c, u2[H0][r], lap, mm[H0][r]);
            }
        }
        // stores: own plane + fused periodic wrap (buffer stores, masked lanes dropped)
        {
            const auto rs = prs(p.u, i);
#pragma unroll
            for (int r = 0; r < R; ++r) bst<kStAux>(vv[r], rs, os[r]);
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (i >= p.w_lo[g] && i <= p.w_hi[g]) {
                    const auto rw = prs(p.u, i + p.w_sh[g]);
#pragma unroll
                    for (int r = 0; r < R; ++r) bst<kStAux>(vv[r], rw, os[r]);
                }
            if constexpr (MODE == kSave || kImg) {
                const auto rx = prs(MODE == kSave ? p.lap_out : p.acc, i);
#pragma unroll
                for (int r = 0; r < R; ++r) bst<kStAux>(xv[r], rx, os[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!valid[r]) continue;
            chk += vv[r];
            if (erow) ma = max_abs(ma, vv[r]);
        }
    };

    for (int i = ib;;) {
        plane(Ph<0>{}, i);
        if (++i > ie) break;
        plane(Ph<1>{}, i);
        if (++i > ie) break;
        plane(Ph<2>{}, i);
        if (++i > ie) break;
        plane(Ph<3>{}, i);
        if (++i > ie) break;
    }
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
    constexpr unsigned ES = sizeof(T);
    __shared__ T lds[2][LR][LC];

    const int bid = xcd_swizzle(blockIdx.x, gridDim.x, p.xcd);
    const int b = find_box(p, bid);
    const BoxLaunch B = p.box[b];
    int local = bid - B.block_begin;
    const int tk = local % B.tiles_k;
    local /= B.tiles_k;
    const int tj = local % B.tiles_j;
    const int ci = local / B.tiles_j;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kb = B.kbase + tk * kTK;
    const int k = kb + lane;
    const int jt = B.j0 + tj * kTJ;
    const int ib = B.i0 + ci * B.chunk;
    const int ie = min(B.i1, ib + B.chunk - 1);

    const bool kin = k >= B.k0 && k <= B.k1;
    const i64 si = p.si;
    const unsigned pbytes = unsigned(si) * ES;
    auto boff = [&](int j, int kk, bool ok) { return ok ? unsigned(j * p.sj + kk + p.poff) * ES : kOOB; };
    auto prs = [&](const T* base, int i) { return plane_rsrc(base + (i64(i) * si - p.poff), pbytes); };
    // byte offset of the source of u1(j, kk) in a plane block and whether it is negated
    auto src = [&](int j, int kk, bool& neg) {
        neg = false;
        if (j < p.mj0) j = 2 * p.mj0 - j, neg = !neg;
        else if (j > p.mj1) j = 2 * p.mj1 - j, neg = !neg;
        if (kk < p.mk0) kk = 2 * p.mk0 - kk, neg = !neg;
        else if (kk > p.mk1) kk = 2 * p.mk1 - kk, neg = !neg;
        return boff(j, kk, j >= 0 && j <= p.jmax && kk >= 0 && kk <= p.kmax);
    };

    unsigned oa[R], ou2[R], os[R];
    bool valid[R], ng[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = jt + w * R + r;
        valid[r] = kin && j <= B.j1;
        oa[r] = src(j, k, ng[r]);
        ou2[r] = boff(j, k, !FIRST && valid[r]);
        os[r] = boff(j, k, valid[r]);  // stores, and the loads of m
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
    constexpr int kMAux = 2;   // non-temporal m (read once per step)
    constexpr int kStAux = 2;  // non-temporal stores (write-once stream)

    static_assert(MODE == kPlain || !FIRST, "save / image / Born modes: leapfrog steps only");
    static_assert(M == 2 || M == 4, "orders 4 and 8");
    constexpr bool kImg = MODE == kImage, kBrn = MODE == kBorn;
    constexpr bool kTwo = kImg || kBrn;  // the two extra rings: q and acc (image) or q and dm (Born)
    T u1[NS][R], u2[2][R], mm[2][R];
    T qq[kTwo ? 2 : 1][kTwo ? R : 1], aa[kTwo ? 2 : 1][kTwo ? R : 1];
    T hv[2][NH];
    if constexpr (kTwo) {
        const auto rQ = prs(p.q, ib), rA = prs(kBrn ? p.dm : p.acc, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            qq[0][r] = bld<T, 2>(rQ, os[r]);
            aa[0][r] = bld<T, 2>(rA, os[r]);
            qq[1][r] = aa[1][r] = T(0);
        }
    }
    {
        // planes ib-M .. ib+M into slots 0 .. 2M (the host keeps the boxes M planes inside)
#pragma unroll
        for (int s = 0; s <= 2 * M; ++s) {
            const auto rp = prs(p.u1, ib - M + s);
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
        const auto q0 = prs(p.u2, ib), m0 = prs(p.m, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            u1[NS - 1][r] = T(0);
            u2[0][r] = FIRST ? T(0) : bld<T>(q0, ou2[r]);
            u2[1][r] = T(0);
            mm[0][r] = bld<T, kMAux>(m0, os[r]);
            mm[1][r] = T(0);
        }
    }
    const T hx2 = p.hx2, hy2 = p.hy2, hz2 = p.hz2;
    const T yx2 = p.yx2, yy2 = p.yy2, yz2 = p.yz2;

    T gyz[TAPER ? R : 1];
    T gxn = T(1);
    if constexpr (TAPER) {
#pragma clang fp contract(off)
        const T gzk = p.gz[min(k, p.kmax)];
#pragma unroll
        for (int r = 0; r < R; ++r) gyz[r] = ldconst(p.gy, min(jt + w * R + r, p.jmax)) * gzk;
        gxn = ldconst(p.gx, ib);
    }

    T ma = T(kErrInit);
    T chk = T(0);
    T* const lds0 = &lds[0][0][0];

    auto plane = [&](auto phase, const int i) {
#pragma clang fp contract(off)
        constexpr int P = decltype(phase)::value;
        constexpr int SC = (P + M) % NS;          // plane i
        constexpr int SN = (P + 2 * M + 1) % NS;  // plane i+M+1, prefetched here
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        {
            const bool more = i < ie;
            const unsigned nb = more ? pbytes : 0u;
            const int dn = more ? M + 1 : 0, d1 = more ? 1 : 0;
            const auto rN = plane_rsrc(p.u1 + (i64(i + dn) * si - p.poff), nb);
            const auto rH = plane_rsrc(p.u1 + (i64(i + d1) * si - p.poff), nb);
            const auto rU = plane_rsrc(p.u2 + (i64(i + d1) * si - p.poff), nb);
            const auto rM = plane_rsrc(p.m + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u1[SN][r] = bld<T>(rN, oa[r]);
                if (!FIRST) u2[H1][r] = bld<T>(rU, ou2[r]);
                mm[H1][r] = bld<T, kMAux>(rM, os[r]);
            }
#pragma unroll
            for (int h = 0; h < NH; ++h) hv[H1][h] = bld<T>(rH, hoff[h]);
            if constexpr (kTwo) {
                const auto rQ = plane_rsrc(p.q + (i64(i + d1) * si - p.poff), nb);
                const auto rA = plane_rsrc((kBrn ? p.dm : p.acc) + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    qq[H1][r] = bld<T, 2>(rQ, os[r]);
                    aa[H1][r] = bld<T, 2>(rA, os[r]);
                }
            }
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

        const bool erow = i >= p.ei0 && i <= p.ei1;
        const T gxi = gxn;
        if constexpr (TAPER) gxn = ldconst(p.gx, i + 1);
        T vv[R];
        T xv[MODE == kSave || kImg ? R : 1];  // kSave: lap; kImage: the new acc
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
            T lap = T(0);
            lap = lap + div_const(tx, hx2, yx2);
            lap = lap + div_const(ty, hy2, yy2);
            lap = lap + div_const(tz, hz2, yz2);
            if constexpr (MODE == kSave) xv[r] = lap;
            if constexpr (kImg) {
                const T pr = c * qq[H0][r];
                xv[r] = aa[H0][r] + pr;
            }
            if constexpr (FIRST) {
                const T half_m = T(0.5) * mm[H0][r];  // exact
                vv[r] = taylor_first(c, lap, half_m);
                if constexpr (TAPER) vv[r] = (gxi * gyz[r]) * vv[r];
            } else if constexpr (kBrn) {
                const T pr = aa[H0][r] * qq[H0][r];  // dm q, rounded before the add
                if constexpr (TAPER) {
                    const T g = gxi * gyz[r];
                    vv[r] = g * (leapfrog(c, g * u2[H0][r], lap, mm[H0][r]) + pr);
                } else {
                    vv[r] = leapfrog(c, u2[H0][r], lap, mm[H0][r]) + pr;
                }
            } else if constexpr (TAPER) {
                const T g = gxi * gyz[r];
                vv[r] = g * leapfrog(c, g * u2[H0][r], lap, mm[H0][r]);
            } else {
                vv[r] = leapfrog(c, u2[H0][r], lap, mm[H0][r]);
            }
        }
        {
            const auto rs = prs(p.u, i);
#pragma unroll
            for (int r = 0; r < R; ++r) bst<kStAux>(vv[r], rs, os[r]);
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (i >= p.w_lo[g] && i <= p.w_hi[g]) {
                    const auto rw = prs(p.u, i + p.w_sh[g]);
#pragma unroll
                    for (int r = 0; r < R; ++r) bst<kStAux>(vv[r], rw, os[r]);
                }
            if constexpr (MODE == kSave || kImg) {
                const auto rx = prs(MODE == kSave ? p.lap_out : p.acc, i);
#pragma unroll
                for (int r = 0; r < R; ++r) bst<kStAux>(xv[r], rx, os[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!valid[r]) continue;
            chk += vv[r];
            if (erow) ma = max_abs(ma, vv[r]);
        }
    };

    for (int i = ib;;) {
        plane(Ph<0>{}, i);
        if (++i > ie) break;
        plane(Ph<1>{}, i);
        if (++i > ie) break;
        plane(Ph<2>{}, i);
        if (++i > ie) break;
        plane(Ph<3>{}, i);
        if (++i > ie) break;
        plane(Ph<4>{}, i);
        if (++i > ie) break;
        plane(Ph<5>{}, i);
        if (++i > ie) break;
        if constexpr (NS > 6) {
            plane(Ph<6>{}, i);
            if (++i > ie) break;
            plane(Ph<7>{}, i);
            if (++i > ie) break;
            plane(Ph<8>{}, i);
            if (++i > ie) break;
            plane(Ph<9>{}, i);
            if (++i > ie) break;
        }
    }
    commit_errors(ma, T(kErrInit), chk, p.err);
}

// rows per lane of the k_march_mh instantiations (`make resources`: no scratch in any of them)
template <class T, int M, int MODE>
constexpr int mh_rows() {
    return 4;
}

template <class T, int M>
void (*march_mh_kernel(bool first, bool taper, int mode))(const MediumParamsH<T>) {
    if (mode == kSave)
        return taper ? k_march_mh<T, M, false, mh_rows<T, M, kSave>(), true, kSave>
                     : k_march_mh<T, M, false, mh_rows<T, M, kSave>(), false, kSave>;
    if (mode == kImage)
        return taper ? k_march_mh<T, M, false, mh_rows<T, M, kImage>(), true, kImage>
                     : k_march_mh<T, M, false, mh_rows<T, M, kImage>(), false, kImage>;
    if (mode == kBorn)
        return taper ? k_march_mh<T, M, false, mh_rows<T, M, kBorn>(), true, kBorn>
                     : k_march_mh<T, M, false, mh_rows<T, M, kBorn>(), false, kBorn>;
    constexpr int RP = mh_rows<T, M, kPlain>();
    if (first) return taper ? k_march_mh<T, M, true, RP, true> : k_march_mh<T, M, true, RP, false>;
    return taper ? k_march_mh<T, M, false, RP, true> : k_march_mh<T, M, false, RP, false>;
}

template <class T, int M>
int march_mh_rows(int mode) {
    return mode == kSave    ? mh_rows<T, M, kSave>()
           : mode == kImage ? mh_rows<T, M, kImage>()
           : mode == kBorn  ? mh_rows<T, M, kBorn>()
                            : mh_rows<T, M, kPlain>();
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
template <class T, bool FIRST, int R, bool TAPER, int MODE = kPlain>
__global__ void __launch_bounds__(kThreads) k_march_mb(const MediumParamsB<T> p) {
    constexpr int kTJ = kWaves * R;
    constexpr unsigned ES = sizeof(T);
    __shared__ T lds[2][kTJ + 2][kLW];
    __shared__ T ldb[2][kTJ + 2][kLW];

    const int bid = xcd_swizzle(blockIdx.x, gridDim.x, p.xcd);
    const int b = find_box(p, bid);
    const BoxLaunch B = p.box[b];
    int local = bid - B.block_begin;
    const int tk = local % B.tiles_k;
    local /= B.tiles_k;
    const int tj = local % B.tiles_j;
    const int ci = local / B.tiles_j;

    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int kb = B.kbase + tk * kTK;
    const int k = kb + lane;
    const int jt = B.j0 + tj * kTJ;
    const int ib = B.i0 + ci * B.chunk;
    const int ie = min(B.i1, ib + B.chunk - 1);

    const bool kload = k <= p.kmax;
    const bool kin = k >= B.k0 && k <= B.k1;
    const i64 si = p.si;
    const unsigned pbytes = unsigned(si) * ES;
    auto boff = [&](int j, int kk, bool ok) { return ok ? unsigned(j * p.sj + kk + p.poff) * ES : kOOB; };
    auto prs = [&](const T* base, int i) { return plane_rsrc(base + (i64(i) * si - p.poff), pbytes); };

    unsigned oa[R], ou2[R], os[R];
    bool valid[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = jt + w * R + r;
        valid[r] = kin && j <= B.j1;
        oa[r] = boff(j, k, kload && j <= p.jmax);  // u1 and b
        ou2[r] = boff(j, k, !FIRST && valid[r]);
        os[r] = boff(j, k, valid[r]);  // stores, and the loads of m
    }

    // halo role of this lane (k_march_m's): one LDS cell per plane and tile
    int hrow = 0, hcol = 0;
    unsigned hoff = kOOB;
    bool hon = false;
    if (w == 0) {  // row jt-1
        hon = true;
        hoff = boff(jt - 1, k, kload);
        hrow = 0;
        hcol = 1 + lane;
    } else if (w == kWaves - 1) {  // row jt+TJ
        const int j = jt + kTJ;
        hon = true;
        hoff = boff(j, k, kload && j <= p.jmax);
        hrow = kTJ + 1;
        hcol = 1 + lane;
    } else if (w == 1) {  // columns kb-1 (lanes 0..TJ-1) and kb+64 (lanes 32..32+TJ-1)
        const int side = lane >> 5, rr = lane & 31;
        const int j = jt + rr;
        const int kk = side ? kb + kTK : kb - 1;
        hon = rr < kTJ;
        hoff = boff(j, kk, hon && j <= p.jmax && kk <= p.kmax);
        hrow = 1 + rr;
        hcol = side ? kTK + 1 : 0;
    }
    constexpr int kMAux = 2;   // non-temporal m (read once per step)
    constexpr int kStAux = 2;  // non-temporal stores (write-once stream)

    static_assert(MODE == kPlain || !FIRST, "save / image / Born modes: leapfrog steps only");
    constexpr bool kImg = MODE == kImage, kBrn = MODE == kBorn;
    constexpr bool kTwo = kImg || kBrn;  // the two extra rings: q and acc (image) or q and dm (Born)
    T u1[4][R], bb[4][R], u2[2][R], mm[2][R];
    T qq[kTwo ? 2 : 1][kTwo ? R : 1], aa[kTwo ? 2 : 1][kTwo ? R : 1];
    T hv[2], hb[2];
    if constexpr (kTwo) {
        const auto rQ = prs(p.q, ib), rA = prs(kBrn ? p.dm : p.acc, ib);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            qq[0][r] = bld<T, 2>(rQ, os[r]);
            aa[0][r] = bld<T, 2>(rA, os[r]);
            qq[1][r] = aa[1][r] = T(0);
        }
    }
    {
        const auto r0 = prs(p.u1, ib - 1), r1 = prs(p.u1, ib), r2 = prs(p.u1, ib + 1);
        const auto b0 = prs(p.b, ib - 1), b1 = prs(p.b, ib), b2 = prs(p.b, ib + 1);
        const auto q0 = prs(p.u2, ib), m0 = prs(p.m, ib);
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
            mm[0][r] = bld<T, kMAux>(m0, os[r]);
            mm[1][r] = T(0);
        }
        hv[0] = bld<T>(r1, hoff);
        hb[0] = bld<T>(b1, hoff);
        hv[1] = hb[1] = T(0);
    }
    const T hx2 = p.hx2, hy2 = p.hy2, hz2 = p.hz2;
    const T yx2 = p.yx2, yy2 = p.yy2, yz2 = p.yz2;

    T gyz[TAPER ? R : 1];
    T gxn = T(1);
    if constexpr (TAPER) {
#pragma clang fp contract(off)
        const T gzk = p.gz[min(k, p.kmax)];
#pragma unroll
        for (int r = 0; r < R; ++r) gyz[r] = ldconst(p.gy, min(jt + w * R + r, p.jmax)) * gzk;
        gxn = ldconst(p.gx, ib);
    }

    T ma = T(kErrInit);
    T chk = T(0);

    auto plane = [&](auto phase, const int i) {
        constexpr int P = decltype(phase)::value;
        constexpr int S0 = P & 3, S1 = (P + 1) & 3, S2 = (P + 2) & 3, S3 = (P + 3) & 3;
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        // prefetch u1, b (i+2, own rows), u1, b (i+1, halo), u2(i+1), m(i+1); 0-record descriptors
        // on the last plane (loads return 0 without touching memory)
        {
            const bool more = i < ie;
            const unsigned nb = more ? pbytes : 0u;
            const int d2 = more ? 2 : 0, d1 = more ? 1 : 0;
            const auto rN = plane_rsrc(p.u1 + (i64(i + d2) * si - p.poff), nb);
            const auto rH = plane_rsrc(p.u1 + (i64(i + d1) * si - p.poff), nb);
            const auto bN = plane_rsrc(p.b + (i64(i + d2) * si - p.poff), nb);
            const auto bH = plane_rsrc(p.b + (i64(i + d1) * si - p.poff), nb);
            const auto rU = plane_rsrc(p.u2 + (i64(i + d1) * si - p.poff), nb);
            const auto rM = plane_rsrc(p.m + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u1[S3][r] = bld<T>(rN, oa[r]);
                bb[S3][r] = bld<T>(bN, oa[r]);
                if (!FIRST) u2[H1][r] = bld<T>(rU, ou2[r]);
                mm[H1][r] = bld<T, kMAux>(rM, os[r]);
            }
            hv[H1] = bld<T>(rH, hoff);
            hb[H1] = bld<T>(bH, hoff);
            if constexpr (kTwo) {
                const auto rQ = plane_rsrc(p.q + (i64(i + d1) * si - p.poff), nb);
                const auto rA = plane_rsrc((kBrn ? p.dm : p.acc) + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    qq[H1][r] = bld<T, 2>(rQ, os[r]);
                    aa[H1][r] = bld<T, 2>(rA, os[r]);
                }
            }
        }

        // stage plane i of u1 and b: one barrier for both tiles
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lds[H0][1 + w * R + r][1 + lane] = u1[S1][r];
            ldb[H0][1 + w * R + r][1 + lane] = bb[S1][r];
        }
        if (hon) {
            lds[H0][hrow][hcol] = hv[H0];
            ldb[H0][hrow][hcol] = hb[H0];
        }
        __syncthreads();

        const bool erow = i >= p.ei0 && i <= p.ei1;
        const T gxi = gxn;
        if constexpr (TAPER) gxn = ldconst(p.gx, i + 1);
        T vv[R];
        T xv[MODE == kSave || kImg ? R : 1];  // kSave: D_b u1; kImage: the new acc
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma clang fp contract(off)
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
            T lap = T(0);
            lap = lap + div_const(tx, hx2, yx2);
            lap = lap + div_const(ty, hy2, yy2);
            lap = lap + div_const(tz, hz2, yz2);
            if constexpr (MODE == kSave) xv[r] = lap;
            if constexpr (kImg) {
                const T pr = c * qq[H0][r];
                xv[r] = aa[H0][r] + pr;
            }
            if constexpr (FIRST) {
                const T half_m = T(0.5) * mm[H0][r];  // exact
                vv[r] = taylor_first(c, lap, half_m);
                if constexpr (TAPER) vv[r] = (gxi * gyz[r]) * vv[r];
            } else if constexpr (kBrn) {
                const T pr = aa[H0][r] * qq[H0][r];  // dm q, rounded before the add
                if constexpr (TAPER) {
                    const T g = gxi * gyz[r];
                    vv[r] = g * (leapfrog(c, g * u2[H0][r], lap, mm[H0][r]) + pr);
                } else {
                    vv[r] = leapfrog(c, u2[H0][r], lap, mm[H0][r]) + pr;
                }
            } else if constexpr (TAPER) {
                const T g = gxi * gyz[r];
                vv[r] = g * leapfrog(c, g * u2[H0][r], lap, mm[H0][r]);
            } else {
                vv[r] = leapfrog(c, u2[H0][r], lap, mm[H0][r]);
            }
        }
        // stores: own plane + fused periodic wrap (buffer stores, masked lanes dropped)
        {
            const auto rs = prs(p.u, i);
#pragma unroll
            for (int r = 0; r < R; ++r) bst<kStAux>(vv[r], rs, os[r]);
#pragma unroll
            for (int g = 0; g < 2; ++g)
                if (i >= p.w_lo[g] && i <= p.w_hi[g]) {
                    const auto rw = prs(p.u, i + p.w_sh[g]);
#pragma unroll
                    for (int r = 0; r < R; ++r) bst<kStAux>(vv[r], rw, os[r]);
                }
            if constexpr (MODE == kSave || kImg) {
                const auto rx = prs(MODE == kSave ? p.lap_out : p.acc, i);
#pragma unroll
                for (int r = 0; r < R; ++r) bst<kStAux>(xv[r], rx, os[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (!valid[r]) continue;
            chk += vv[r];
            if (erow) ma = max_abs(ma, vv[r]);
        }
    };

    for (int i = ib;;) {
        plane(Ph<0>{}, i);
        if (++i > ie) break;
        plane(Ph<1>{}, i);
        if (++i > ie) break;
        plane(Ph<2>{}, i);
        if (++i > ie) break;
        plane(Ph<3>{}, i);
        if (++i > ie) break;
    }
    commit_errors(ma, T(kErrInit), chk, p.err);
}

// the k_march_mb instantiations: 4 rows per lane (`make resources`: no scratch in any of them)
template <class T>
void (*march_mb_kernel(bool first, bool taper, int mode))(const MediumParamsB<T>) {
    if (mode == kSave) return taper ? k_march_mb<T, false, 4, true, kSave> : k_march_mb<T, false, 4, false, kSave>;
    if (mode == kImage) return taper ? k_march_mb<T, false, 4, true, kImage> : k_march_mb<T, false, 4, false, kImage>;
    if (mode == kBorn) return taper ? k_march_mb<T, false, 4, true, kBorn> : k_march_mb<T, false, 4, false, kBorn>;
    if (first) return taper ? k_march_mb<T, true, 4, true> : k_march_mb<T, true, 4, false>;
    return taper ? k_march_mb<T, false, 4, true> : k_march_mb<T, false, 4, false>;
}

struct NodeGrid {
    i64 si;
    int sj;
    int nx, ny, nz;  // storage extents: indices 0 .. n-1 exist
};

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

NodeGrid node_grid(const GridView& gv) {
    W3D_REQUIRE(gv.G == 1 && gv.poff == 0, "medium kernels: one ghost layer");
    return NodeGrid{gv.si, gv.sj, gv.X + 2, gv.Y + 2, gv.Z + 2};
}

template <class T, bool FIRST, bool TAPER>
void (*march_m_kernel(int variant))(const MediumParams<T>) {
    constexpr int RD = 4;  // march_rows_per_thread()
    switch (variant & 3) {
        case 1: return k_march_m<T, FIRST, RD, true, TAPER>;
        case 2: return k_march_m<T, FIRST, 2, false, TAPER>;
        case 3: return k_march_m<T, FIRST, 2, true, TAPER>;
        default: return k_march_m<T, FIRST, RD, false, TAPER>;
    }
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

template <class T>
void launch_step_medium(bool first, const T* u1, const T* u2, const T* m, T* u, const GridView& gv,
                        const Box* boxes, int nbox, int ei0, int ei1, const Wrap& wrap,
                        const double h2[3], u64* err, int chunk, hipStream_t s, int variant, const T* gx,
                        const T* gy, const T* gz, T* lap_out, const T* q, T* acc, int order, const int* mirror,
                        const T* b, const T* dm) {
    W3D_REQUIRE(order == 2 || order == 4 || order == 8, "space order must be 2, 4 or 8, not " + std::to_string(order));
    W3D_REQUIRE(!b || order == 2, "variable density (b) exists for space order 2 only");
    const int M = order / 2;
    const bool taper = gx || gy || gz;
    W3D_REQUIRE(!taper || (gx && gy && gz), "the sponge needs all three tables");
    W3D_REQUIRE(!taper || gv.G == 1, "sponge tables: one ghost layer");
    W3D_REQUIRE(nbox >= 1 && nbox <= kMaxBoxes, "bad box count");
    W3D_REQUIRE(march_rows_per_thread() == 4, "k_march_m is instantiated for 4 rows per lane");
    W3D_REQUIRE(gv.si > 0 && gv.si * i64(sizeof(T)) < (1ll << 31), "plane larger than a buffer descriptor's range");
    W3D_REQUIRE(gv.sj >= gv.Z + 2 * gv.G && gv.si >= i64(gv.Y + 2 * gv.G) * gv.sj, "strides smaller than the grid");
    if (variant < 0) variant = medium_variant();
    W3D_REQUIRE(!b || variant == 1, "variable density (b) is instantiated for the default variant only (nt, 4 rows per lane)");
    // Born mode: q and dm without acc; q with neither acc nor dm stays an incomplete image mode
    const bool born = dm != nullptr;
    W3D_REQUIRE(!born || q, "Born mode needs q beside dm");
    W3D_REQUIRE(!born || (!lap_out && !acc), "Born mode (q, dm) cannot be combined with save or image mode");
    const bool save = lap_out != nullptr, image = !born && (q || acc);
    W3D_REQUIRE(!image || (q && acc), "image mode needs both q and acc");
    W3D_REQUIRE(!(save && image), "save mode (lap_out) and image mode (q, acc) cannot be combined");
    W3D_REQUIRE(!(save || image || born) || !first, "save / image / Born modes: not on the Taylor start (first)");
    W3D_REQUIRE(!(save || image || born) || variant == 1 || M > 1,
                "save / image / Born modes are instantiated for the default variant only (nt, 4 rows per lane)");
    if (born) {
        // q and dm are read while u is written (own plane and wrap planes): no shared memory
        const i64 span = i64(gv.X + 2 * gv.G - 1) * gv.si + i64(gv.Y + 2 * gv.G - 1) * gv.sj + gv.Z + 2 * gv.G;
        auto overlaps = [&](const T* x) {
            const std::uintptr_t u0 = std::uintptr_t(u), x0 = std::uintptr_t(x), n = std::uintptr_t(span) * sizeof(T);
            return u0 < x0 + n && x0 < u0 + n;
        };
        W3D_REQUIRE(!overlaps(q) && !overlaps(dm), "Born mode: q or dm shares memory with u");
    }
    const int mode = save ? kSave : image ? kImage : born ? kBorn : kPlain;
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
    p.xcd = xcd_swizzle_enabled();
    p.u1 = u1;
    p.u2 = u2;
    p.m = m;
    p.u = u;
    p.si = gv.si;
    p.sj = gv.sj;
    p.poff = gv.poff;
    p.jmax = gv.jmax();
    p.kmax = gv.kmax();
    p.ei0 = ei0;
    p.ei1 = ei1;
    for (int q = 0; q < kMaxWrap; ++q)
        W3D_REQUIRE(wrap.src[q] < 1 || (wrap.src[q] <= gv.X && wrap.dst[q] >= 1 - gv.G && wrap.dst[q] <= gv.X + gv.G),
                    "wrap plane outside the grid");
    wrap_ranges(wrap, p.w_lo, p.w_hi, p.w_sh);
    p.hx2 = T(h2[0]);
    p.hy2 = T(h2[1]);
    p.hz2 = T(h2[2]);
    p.yx2 = T(1) / T(h2[0]);
    p.yy2 = T(1) / T(h2[1]);
    p.yz2 = T(1) / T(h2[2]);
    p.err = err;
    p.gx = gx;
    p.gy = gy;
    p.gz = gz;
    p.lap_out = lap_out;
    p.q = q;
    p.acc = acc;
    p.dm = dm;
    const int tj_rows = kWaves * (M == 2   ? march_mh_rows<T, 2>(mode)
                                  : M == 4 ? march_mh_rows<T, 4>(mode)
                                  : (variant & 2) ? 2
                                                  : 4);
    int btiles[kMaxBoxes], bplanes[kMaxBoxes], nbt = 0;
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
        btiles[nbt] = ((bx.k1 - 1) / kTK - (bx.k0 - 1) / kTK + 1) * cdiv(bx.j1 - bx.j0 + 1, tj_rows);
        bplanes[nbt++] = bx.i1 - bx.i0 + 1;
    }
    // launch_step's march path: 32-plane work items, shorter on small grids
    const int achunk = auto_chunk_boxes(32, btiles, bplanes, nbt);
    int nb = 0, total = 0;
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
        BoxLaunch& L = p.box[nb];
        L.i0 = bx.i0, L.i1 = bx.i1, L.j0 = bx.j0, L.j1 = bx.j1, L.k0 = bx.k0, L.k1 = bx.k1;
        const int t0 = (bx.k0 - 1) / kTK, t1 = (bx.k1 - 1) / kTK;
        L.kbase = 1 + t0 * kTK;
        L.tiles_k = t1 - t0 + 1;
        L.tiles_j = cdiv(bx.j1 - bx.j0 + 1, tj_rows);
        const int planes = bx.i1 - bx.i0 + 1;
        int ch = std::min(chunk > 0 ? chunk : achunk, planes);
        ch = cdiv(planes, cdiv(planes, ch));  // equal work items (no short tail chunk)
        L.chunk = ch;
        L.block_begin = total;
        total += L.tiles_k * L.tiles_j * cdiv(planes, ch);
        ++nb;
    }
    p.nbox = nb;
    if (nb == 0) return;
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
    void (*kern)(const MediumParams<T>) =
        taper ? (first ? march_m_kernel<T, true, true>(variant) : march_m_kernel<T, false, true>(variant))
              : (first ? march_m_kernel<T, true, false>(variant) : march_m_kernel<T, false, false>(variant));
    if (save) kern = taper ? k_march_m<T, false, 4, true, true, kSave> : k_march_m<T, false, 4, true, false, kSave>;
    if (image) kern = taper ? k_march_m<T, false, 4, true, true, kImage> : k_march_m<T, false, 4, true, false, kImage>;
    if (born) kern = taper ? k_march_m<T, false, 4, true, true, kBorn> : k_march_m<T, false, 4, true, false, kBorn>;
    hipLaunchKernelGGL(kern, dim3(total), dim3(kThreads), 0, s, p);
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

#define W3D_MEDIUM_INST(T)                                                                              \
    template void launch_step_medium<T>(bool, const T*, const T*, const T*, T*, const GridView&,       \
                                        const Box*, int, int, int, const Wrap&, const double[3], u64*, \
                                        int, hipStream_t, int, const T*, const T*, const T*, T*,       \
                                        const T*, T*, int, const int*, const T*, const T*);            \
    template void launch_inject<T>(T*, const T*, const GridView&, const int*, const T*, int,           \
                                   const Wrap&, hipStream_t);                                          \
    template void launch_record<T>(const T*, const GridView&, const int*, T*, int, hipStream_t);
W3D_MEDIUM_INST(double)
W3D_MEDIUM_INST(float)

}  // namespace wave3d
