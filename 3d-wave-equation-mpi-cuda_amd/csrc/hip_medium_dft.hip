// On-the-fly discrete Fourier transform of a field: the accumulation behind the medium solver's
// frequency-domain wavefields and its checkpoint-free spectral gradient (interface: hip_medium.hpp,
// launch_dft_acc).
//
//  * k_dft_acc: re_f = re_f + u c_f, im_f = im_f + u s_f at the box nodes for the NF frequencies of a
//    launch, (c_f, s_f) one row of a twiddle table in device memory. It takes k_face_corr's
//    decomposition (march_tile.hpp: the same tiles, boxes and chunks, 64 lanes along k, plane
//    descriptors with kOOB masking) and none of its staging: a node needs no neighbour, so there is no
//    LDS, no barrier, no halo and no statistic.
//
// FP contraction is off (-ffp-contract=off + the pragmas in stencil_math.hpp): every product is rounded
// before its add, so fp64 and fp32 results are bitwise those of ops/reference.py dft_accumulate.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "device_common.hpp"
#include "hip_medium.hpp"
#include "march_tile.hpp"

namespace wave3d {
namespace {

template <class T>
struct DftParams : TileParams<T> {
    const T* u;
    const T* c;  // the launch's part of the twiddle row: NF cosines
    const T* s;  // and NF negated sines
    T* re[kDftNF];
    T* im[kDftNF];
};

// R = rows (j) per lane; the workgroup tile is (4R) x 64, marched along i over one chunk. Per plane a
// lane loads u at its R nodes once, then the 2 NF accumulators at the same offsets non-temporally
// (each is read once and written once per call), and only then computes and stores: all of a plane's
// (1 + 2 NF) R loads are in flight together, and the other waves of the SIMD cover their latency. The
// twiddles are wave-uniform scalar loads ahead of the march. Lanes outside the box carry kOOB (the
// load gives 0, the store is dropped), so nothing outside the boxes is read into a sum or written.
// 8 + 32 NF B per node in fp64, 4 + 16 NF B in fp32.
template <class T, int NF, int R>
__global__ void __launch_bounds__(kThreads) k_dft_acc(const DftParams<T> p) {
    const Tile<T, R> t(p);
    unsigned os[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int j = t.row(r);
        os[r] = t.boff(j, t.k, t.owns(j));
    }
    T cf[NF], sf[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        cf[f] = ldconst(p.c, f);
        sf[f] = ldconst(p.s, f);
    }
    constexpr int kNt = 2;  // non-temporal

    for (int i = t.ib; i <= t.ie; ++i) {
        T uu[R], a[NF][R], b[NF][R];
        {
            const auto ru = t.prs(p.u, i);
#pragma unroll
            for (int r = 0; r < R; ++r) uu[r] = bld<T>(ru, os[r]);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const auto rr = t.prs(p.re[f], i), ri = t.prs(p.im[f], i);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                a[f][r] = bld<T, kNt>(rr, os[r]);
                b[f][r] = bld<T, kNt>(ri, os[r]);
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma clang fp contract(off)
            const auto rr = t.prs(p.re[f], i), ri = t.prs(p.im[f], i);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const T pc = uu[r] * cf[f];
                const T ps = uu[r] * sf[f];
                bst<kNt>(a[f][r] + pc, rr, os[r]);
                bst<kNt>(b[f][r] + ps, ri, os[r]);
            }
        }
    }
}

// Rows per lane. Two: a plane's loads are then 2 (1 + 2 NF) = 18 values per lane at NF = 4, which
// `make resources` shows far below the 64 VGPRs that still allow 8 waves per SIMD; no scratch.
constexpr int kDftRows = 2;

template <class T, int NF>
void launch_part(DftParams<T>& p, int total, hipStream_t s) {
    hipLaunchKernelGGL((k_dft_acc<T, NF, kDftRows>), dim3(total), dim3(kThreads), 0, s, p);
    HIP_OK(hipGetLastError());
}

}  // namespace

template <class T>
void launch_dft_acc(const T* u, T* const* re, T* const* im, int nf, const T* c_row, const T* s_row,
                    const GridView& gv, const Box* boxes, int nbox, int chunk, hipStream_t s) {
    W3D_REQUIRE(nf >= 1, "dft accumulation: needs at least one frequency");
    W3D_REQUIRE(u && re && im && c_row && s_row, "dft accumulation: null grid or twiddle row");
    W3D_REQUIRE(nbox >= 1 && nbox <= kMaxBoxes, "bad box count");
    W3D_REQUIRE(gv.G == 1 && gv.poff == 0, "dft accumulation: one ghost layer in the grid view");
    W3D_REQUIRE(gv.X >= 1 && gv.Y >= 1 && gv.Z >= 1, "grid needs at least one owned node per axis");
    W3D_REQUIRE(gv.si > 0 && gv.si * i64(sizeof(T)) < (1ll << 31), "plane larger than a buffer descriptor's range");
    W3D_REQUIRE(gv.sj >= gv.Z + 2 && gv.si >= i64(gv.Y + 2) * gv.sj, "strides smaller than the grid");
    // every accumulator is read and written while u is read: none may share memory with u or another
    const i64 span = i64(gv.X + 1) * gv.si + i64(gv.Y + 1) * gv.sj + gv.Z + 2;  // elements a grid covers
    for (int f = 0; f < nf; ++f) {
        W3D_REQUIRE(re[f] && im[f], "dft accumulation: null accumulator");
        W3D_REQUIRE(!overlaps<T>(re[f], u, span) && !overlaps<T>(im[f], u, span),
                    "dft accumulation: an accumulator shares memory with u");
        W3D_REQUIRE(!overlaps<T>(re[f], im[f], span), "dft accumulation: two accumulators share memory");
        for (int g = 0; g < f; ++g)
            W3D_REQUIRE(!overlaps<T>(re[f], re[g], span) && !overlaps<T>(re[f], im[g], span) &&
                            !overlaps<T>(im[f], re[g], span) && !overlaps<T>(im[f], im[g], span),
                        "dft accumulation: two accumulators share memory");
    }
    for (int q = 0; q < nbox; ++q) {
        const Box& bx = boxes[q];
        if (bx.empty()) continue;
        W3D_REQUIRE(bx.i0 >= 1 && bx.i1 <= gv.X && bx.j0 >= 1 && bx.j1 <= gv.Y && bx.k0 >= 1 && bx.k1 <= gv.Z,
                    "dft accumulation: box outside the owned region (it touches a storage edge)");
    }
    DftParams<T> p{};
    const double ones[3] = {1, 1, 1};  // no division here
    fill_tile_params(p, gv, ones);
    p.u = u;
    const int total = plan_boxes(p, boxes, nbox, kWaves * kDftRows, chunk);
    if (p.nbox == 0) return;
    for (int f0 = 0; f0 < nf; f0 += kDftNF) {  // whole launches of kDftNF, then the rest in one
        const int n = std::min(kDftNF, nf - f0);
        p.c = c_row + f0;
        p.s = s_row + f0;
        for (int f = 0; f < kDftNF; ++f) {
            p.re[f] = f < n ? re[f0 + f] : nullptr;
            p.im[f] = f < n ? im[f0 + f] : nullptr;
        }
        switch (n) {
            case 1: launch_part<T, 1>(p, total, s); break;
            case 2: launch_part<T, 2>(p, total, s); break;
            case 3: launch_part<T, 3>(p, total, s); break;
            default: launch_part<T, 4>(p, total, s); break;
        }
    }
}
static_assert(kDftNF == 4, "launch_dft_acc dispatches on 1 .. 4 frequencies per launch");

template void launch_dft_acc<double>(const double*, double* const*, double* const*, int, const double*, const double*,
                                     const GridView&, const Box*, int, int, hipStream_t);
template void launch_dft_acc<float>(const float*, float* const*, float* const*, int, const float*, const float*,
                                    const GridView&, const Box*, int, int, hipStream_t);

}  // namespace wave3d
