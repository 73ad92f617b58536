// Face correlation of two fields, the accumulation of the density gradient dJ/drho of the medium
// solver's adjoint pass (interface: hip_medium.hpp, launch_face_corr).
//
//  * k_face_corr: acc = acc + C(a, v) at the box nodes, C the sum over a node's six faces of the
//    products of the two fields' differences across the face, each axis divided by its h^2. It is
//    k_march_mb's skeleton (hip_medium.hip) with other streams: both fields need their six
//    neighbours, so both roll through registers and LDS the way u1 and b do there, and acc is the
//    one read-modify-write stream at the lane's own nodes. No u2, m, taper, statistic or wrap.
//
// FP contraction is off (-ffp-contract=off + the pragmas in stencil_math.hpp): every operation is
// rounded on its own in the order of ops/reference.py face_correlation, so fp64 results are bitwise
// those of the PyTorch oracle.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_common.hpp"
#include "hip_medium.hpp"

namespace wave3d {
namespace {

template <class T>
struct CorrParams {
    int xcd;  // XCD-aware tile order (xcd_swizzle)
    const T* a;
    const T* v;
    T* acc;
    i64 si;
    int sj;
    int poff;        // see GridView::poff
    int jmax, kmax;  // largest valid j / k index in storage
    int nbox;
    BoxLaunch box[kMaxBoxes];
    T hx2, hy2, hz2;
    T yx2, yy2, yz2;  // RN(1/h^2) in T for the correctly rounded constant division
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
    constexpr unsigned ES = sizeof(T);
    __shared__ T lda[2][kTJ + 2][kLW];
    __shared__ T ldv[2][kTJ + 2][kLW];

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

    unsigned oa[R], os[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = jt + w * R + r;
        oa[r] = boff(j, k, kload && j <= p.jmax);  // a and v
        os[r] = boff(j, k, kin && j <= B.j1);      // acc: loads and stores
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
    constexpr int kNt = 2;  // non-temporal: acc is read once and written once per call

    T aa[4][R], vv[4][R], cc[2][R];
    T ha[2], hv[2];
    {
        const auto a0 = prs(p.a, ib - 1), a1 = prs(p.a, ib), a2 = prs(p.a, ib + 1);
        const auto v0 = prs(p.v, ib - 1), v1 = prs(p.v, ib), v2 = prs(p.v, ib + 1);
        const auto c0 = prs(p.acc, ib);
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
        ha[0] = bld<T>(a1, hoff);
        hv[0] = bld<T>(v1, hoff);
        ha[1] = hv[1] = T(0);
    }
    const T hx2 = p.hx2, hy2 = p.hy2, hz2 = p.hz2;
    const T yx2 = p.yx2, yy2 = p.yy2, yz2 = p.yz2;

    auto plane = [&](auto phase, const int i) {
        constexpr int P = decltype(phase)::value;
        constexpr int S0 = P & 3, S1 = (P + 1) & 3, S2 = (P + 2) & 3, S3 = (P + 3) & 3;
        constexpr int H0 = P & 1, H1 = (P + 1) & 1;
        // prefetch a, v (i+2, own rows), a, v (i+1, halo), acc(i+1); 0-record descriptors on the
        // last plane (loads return 0 without touching memory)
        {
            const bool more = i < ie;
            const unsigned nb = more ? pbytes : 0u;
            const int d2 = more ? 2 : 0, d1 = more ? 1 : 0;
            const auto aN = plane_rsrc(p.a + (i64(i + d2) * si - p.poff), nb);
            const auto aH = plane_rsrc(p.a + (i64(i + d1) * si - p.poff), nb);
            const auto vN = plane_rsrc(p.v + (i64(i + d2) * si - p.poff), nb);
            const auto vH = plane_rsrc(p.v + (i64(i + d1) * si - p.poff), nb);
            const auto cN = plane_rsrc(p.acc + (i64(i + d1) * si - p.poff), nb);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                aa[S3][r] = bld<T>(aN, oa[r]);
                vv[S3][r] = bld<T>(vN, oa[r]);
                cc[H1][r] = bld<T, kNt>(cN, os[r]);
            }
            ha[H1] = bld<T>(aH, hoff);
            hv[H1] = bld<T>(vH, hoff);
        }

        // stage plane i of a and v: one barrier for both tiles
#pragma unroll
        for (int r = 0; r < R; ++r) {
            lda[H0][1 + w * R + r][1 + lane] = aa[S1][r];
            ldv[H0][1 + w * R + r][1 + lane] = vv[S1][r];
        }
        if (hon) {
            lda[H0][hrow][hcol] = ha[H0];
            ldv[H0][hrow][hcol] = hv[H0];
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
            T c = T(0);
            c = c + div_const(tx, hx2, yx2);
            c = c + div_const(ty, hy2, yy2);
            c = c + div_const(tz, hz2, yz2);
            out[r] = cc[H0][r] + c;
        }
        {
            const auto rs = prs(p.acc, i);
#pragma unroll
            for (int r = 0; r < R; ++r) bst<kNt>(out[r], rs, os[r]);
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
    auto overlaps = [&](const T* x) {
        const std::uintptr_t c0 = std::uintptr_t(acc), x0 = std::uintptr_t(x), n = std::uintptr_t(span) * sizeof(T);
        return c0 < x0 + n && x0 < c0 + n;
    };
    W3D_REQUIRE(!overlaps(a) && !overlaps(v), "face correlation: acc shares memory with a or v");
    CorrParams<T> p{};
    p.xcd = xcd_swizzle_enabled();
    p.a = a;
    p.v = v;
    p.acc = acc;
    p.si = gv.si;
    p.sj = gv.sj;
    p.poff = gv.poff;
    p.jmax = gv.jmax();
    p.kmax = gv.kmax();
    p.hx2 = T(h2[0]);
    p.hy2 = T(h2[1]);
    p.hz2 = T(h2[2]);
    p.yx2 = T(1) / T(h2[0]);
    p.yy2 = T(1) / T(h2[1]);
    p.yz2 = T(1) / T(h2[2]);
    constexpr int tj_rows = kWaves * kCorrRows;
    int btiles[kMaxBoxes], bplanes[kMaxBoxes], nbt = 0;
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
        // k_march_m's box contract: every box node has its six neighbours inside the storage
        W3D_REQUIRE(bx.i0 >= 1 && bx.i1 <= gv.X && bx.j0 >= 1 && bx.j1 <= gv.Y && bx.k0 >= 1 && bx.k1 <= gv.Z,
                    "face correlation: box outside the owned region (it touches a storage edge)");
        btiles[nbt] = ((bx.k1 - 1) / kTK - (bx.k0 - 1) / kTK + 1) * cdiv(bx.j1 - bx.j0 + 1, tj_rows);
        bplanes[nbt++] = bx.i1 - bx.i0 + 1;
    }
    // launch_step_medium's work items: 32 planes, shorter on small grids
    const int achunk = auto_chunk_boxes(32, btiles, bplanes, nbt);
    int nb = 0, total = 0;
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
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
    hipLaunchKernelGGL((k_face_corr<T, kCorrRows>), dim3(total), dim3(kThreads), 0, s, p);
    HIP_OK(hipGetLastError());
}

template void launch_face_corr<double>(const double*, const double*, double*, const GridView&, const Box*, int,
                                       const double[3], int, hipStream_t);
template void launch_face_corr<float>(const float*, const float*, float*, const GridView&, const Box*, int,
                                      const double[3], int, hipStream_t);

}  // namespace wave3d
