// The skeleton shared by the medium solver's marching kernels (hip_medium.hip: k_march_m,
// k_march_mh, k_march_mb; hip_medium_corr.hip: k_face_corr): a 256-thread workgroup owns a
// (4R) x 64 tile of the (j,k) plane of one box and marches along i over one chunk of planes.
// Here: the parameters every such kernel takes, the decode of a workgroup into its tile, the
// plane descriptors, the one-cell halo role, the unrolled march loop, the division sum, and the
// host's planning of the boxes into work items. Internal to those two translation units.
#pragma once

#include <cstdint>
#include <utility>

#include "device_common.hpp"
#include "hip_medium.hpp"

namespace wave3d {
namespace {

// What every marching kernel's parameter struct begins with (find_box reads nbox and box).
template <class T>
struct TileParams {
    int xcd;  // XCD-aware tile order (xcd_swizzle)
    i64 si;
    int sj;
    int poff;        // see GridView::poff
    int jmax, kmax;  // largest valid j / k index in storage
    int nbox;
    BoxLaunch box[kMaxBoxes];
    T hx2, hy2, hz2;
    T yx2, yy2, yz2;  // RN(1/h^2) in T for the constant division (div_const)
};

template <class T>
void fill_tile_params(TileParams<T>& p, const GridView& gv, const double h2[3]) {
    p.xcd = xcd_swizzle_enabled();
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
}

// The workgroup's box, tile and chunk: R = rows (j) per lane, wave w owns the rows
// jt + w R .. jt + w R + R - 1 and lane l the column k = kb + l; the planes ib .. ie.
template <class T, int R>
struct Tile {
    static constexpr int kTJ = kWaves * R;
    static constexpr unsigned ES = sizeof(T);
    const TileParams<T>& p;
    BoxLaunch B;
    int lane, w, kb, k, jt, ib, ie;
    bool kload, kin;  // k inside the storage / inside the box
    i64 si;
    unsigned pbytes;

    __device__ __forceinline__ explicit Tile(const TileParams<T>& p_) : p(p_) {
        const int bid = xcd_swizzle(blockIdx.x, gridDim.x, p.xcd);
        B = p.box[find_box(p, bid)];
        int local = bid - B.block_begin;
        const int tk = local % B.tiles_k;
        local /= B.tiles_k;
        const int tj = local % B.tiles_j;
        const int ci = local / B.tiles_j;

        lane = threadIdx.x & 63;
        w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        kb = B.kbase + tk * kTK;
        k = kb + lane;
        jt = B.j0 + tj * kTJ;
        ib = B.i0 + ci * B.chunk;
        ie = min(B.i1, ib + B.chunk - 1);

        kload = k <= p.kmax;
        kin = k >= B.k0 && k <= B.k1;
        si = p.si;
        pbytes = unsigned(si) * ES;
    }
    // row r of this lane, and whether (j, k) is a box node of this lane
    __device__ __forceinline__ int row(int r) const { return jt + w * R + r; }
    __device__ __forceinline__ bool owns(int j) const { return kin && j <= B.j1; }
    // byte offset of (j,k) in a plane block (kOOB = masked: loads give 0, stores dropped)
    __device__ __forceinline__ unsigned boff(int j, int kk, bool ok) const {
        return ok ? unsigned(j * p.sj + kk + p.poff) * ES : kOOB;
    }
    // descriptor of plane i of a level
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t prs(const T* base, int i) const {
        return plane_rsrc(base + (i64(i) * si - p.poff), pbytes);
    }
    // descriptor of plane i + d for a prefetch issued while plane i is computed; on the chunk's
    // last plane (!more) a 0-record descriptor: the loads return 0 without touching memory
    __device__ __forceinline__ __amdgpu_buffer_rsrc_t next_rsrc(const T* base, int i, int d, bool more) const {
        return plane_rsrc(base + (i64(i + (more ? d : 0)) * si - p.poff), more ? pbytes : 0u);
    }
};

// One-cell halo role of a lane in the (4R + 2) x 66 LDS tile of a 7-point kernel: wave 0 loads the
// row jt-1, the last wave the row jt+TJ, wave 1 the columns kb-1 (lanes 0..TJ-1) and kb+64 (lanes
// 32..32+TJ-1); one cell per plane, at byte offset hoff of the plane, stored to lds[hrow][hcol].
struct HaloCell {
    bool hon;
    unsigned hoff;
    int hrow, hcol;
};

template <class T, int R>
__device__ __forceinline__ HaloCell halo_cell(const Tile<T, R>& t) {
    constexpr int kTJ = kWaves * R;
    HaloCell h{false, kOOB, 0, 0};
    if (t.w == 0) {  // row jt-1
        h.hon = true;
        h.hoff = t.boff(t.jt - 1, t.k, t.kload);
        h.hrow = 0;
        h.hcol = 1 + t.lane;
    } else if (t.w == kWaves - 1) {  // row jt+TJ
        const int j = t.jt + kTJ;
        h.hon = true;
        h.hoff = t.boff(j, t.k, t.kload && j <= t.p.jmax);
        h.hrow = kTJ + 1;
        h.hcol = 1 + t.lane;
    } else if (t.w == 1) {  // columns kb-1 and kb+64
        const int side = t.lane >> 5, rr = t.lane & 31;
        const int j = t.jt + rr;
        const int kk = side ? t.kb + kTK : t.kb - 1;
        h.hon = rr < kTJ;
        h.hoff = t.boff(j, kk, h.hon && j <= t.p.jmax && kk <= t.p.kmax);
        h.hrow = 1 + rr;
        h.hcol = side ? kTK + 1 : 0;
    }
    return h;
}

// The march over the planes ib .. ie, unrolled by N so that the phase (plane - ib) mod N, and with
// it every register-ring slot, is a compile-time constant: plane(Ph<phase>{}, i).
template <class F, int... I>
__device__ __forceinline__ void march_planes(int ib, int ie, F& plane, std::integer_sequence<int, I...>) {
    for (int i = ib;;)
        if (((plane(Ph<I>{}, i), ++i > ie) || ...)) break;
}
template <int N, class F>
__device__ __forceinline__ void march_planes(int ib, int ie, F& plane) {
    march_planes(ib, ie, plane, std::make_integer_sequence<int, N>{});
}

// ((0 + tx / hx2) + ty / hy2) + tz / hz2, the divisions by div_const: correctly rounded for numerators
// that are zero or in 2^(emin + p + 1) <= |t| <= 2^(emax - ceil(log2 (1 / h2))), within D = 1 ulp of the
// true quotient below that range, NaN above it and for t = +-inf (stencil_math.hpp)
template <class T>
__device__ __forceinline__ T sum_div(T tx, T ty, T tz, const TileParams<T>& p) {
#pragma clang fp contract(off)
    T s = T(0);
    s = s + div_const(tx, p.hx2, p.yx2);
    s = s + div_const(ty, p.hy2, p.yy2);
    s = s + div_const(tz, p.hz2, p.yz2);
    return s;
}

// ---- host ------------------------------------------------------------------------------------
// The non-empty boxes as work items of a (tj_rows x 64)-tile kernel into p.box / p.nbox; returns
// the number of workgroups. chunk > 0 fixes the planes per work item; otherwise 32 planes (the
// march path of launch_step), shorter on small grids, decided for the launch as a whole.
template <class T>
int plan_boxes(TileParams<T>& p, const Box* boxes, int nbox, int tj_rows, int chunk) {
    int btiles[kMaxBoxes], bplanes[kMaxBoxes], nbt = 0;
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
        btiles[nbt] = ((bx.k1 - 1) / kTK - (bx.k0 - 1) / kTK + 1) * cdiv(bx.j1 - bx.j0 + 1, tj_rows);
        bplanes[nbt++] = bx.i1 - bx.i0 + 1;
    }
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
    return total;
}

// whether two grids of `span` elements each share memory
template <class T>
bool overlaps(const T* a, const T* b, i64 span) {
    const std::uintptr_t a0 = std::uintptr_t(a), b0 = std::uintptr_t(b), n = std::uintptr_t(span) * sizeof(T);
    return a0 < b0 + n && b0 < a0 + n;
}

}  // namespace
}  // namespace wave3d
