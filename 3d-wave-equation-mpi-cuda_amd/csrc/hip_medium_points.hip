// Off-grid sources and receivers of the medium solver: weighted gather and scatter on 8 x 8 x 8
// interpolation supports (interface: hip_medium.hpp, launch_record_w / launch_inject_rows /
// launch_rows_dot; ops/reference.py interp_tables, receiver_tables and point_rows build the tables).
//
//  * k_record_w: one wave64 per receiver. Lane l = 8a + b gathers its z column, s = s + wz[c] u[ix[a],
//    iy[b], iz[c]] for c = 0 .. 7, then t = (wx[a] wy[b]) s, and a fixed xor butterfly (32, 16, .. 1)
//    sums the 64 lanes; lane 0 stores. The 24 indices and 24 weights of the receiver are loaded once
//    per wave (lanes 0 .. 23) and handed round by wave shuffles. No LDS, no atomics.
//  * k_inject_rows: one lane per row (touched node) of a CSR list: val = val + w[e] g[col[e]] over
//    the row's entries in order, then u = u + m val and the ghost-plane copies of k_inject. A gather
//    per node: no atomics, no ordering hazard between overlapping supports.
//  * k_rows_dot (the DOT instantiation of the same kernel): sacc[row] = sacc[row] + u val, nothing
//    else is written.
//
// FP contraction is off: every product is rounded before its add, in the order of the oracle
// (ops/reference.py record_weighted, rows_values), so results are bitwise those of PyTorch on the
// CPU in fp64 and in fp32. The host validates every index; the kernels skip what lies outside the
// storage or the tables without dereferencing it.
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "hip_medium.hpp"

namespace wave3d {
namespace {

constexpr int kSlots = 8;              // interpolation slots per axis
constexpr int kTab = 3 * kSlots;       // indices (and weights) per receiver: x, y, z slots

template <class T>
__global__ void __launch_bounds__(64) k_record_w(const T* __restrict__ u, NodeGrid gr, const int* __restrict__ index,
                                                 const T* __restrict__ weight, T* __restrict__ out, int n) {
#pragma clang fp contract(off)
    const int r = blockIdx.x;  // uniform: the whole wave leaves or stays
    if (r >= n) return;
    const int l = threadIdx.x, a = l >> 3, b = l & 7;
    // the receiver's tables, once per wave
    int my_i = -1;
    T my_w = T(0);
    if (l < kTab) {
        my_i = index[i64(r) * kTab + l];
        my_w = weight[i64(r) * kTab + l];
    }
    const int i = __shfl(my_i, a, 64), j = __shfl(my_i, kSlots + b, 64);
    const T wx = __shfl(my_w, a, 64), wy = __shfl(my_w, kSlots + b, 64);
    const bool row_ok = i >= 0 && i < gr.nx && j >= 0 && j < gr.ny;
    const i64 row = i64(i) * gr.si + i64(j) * gr.sj;
    T s = T(0);
#pragma unroll
    for (int c = 0; c < kSlots; ++c) {
        const int k = __shfl(my_i, 2 * kSlots + c, 64);
        const T wz = __shfl(my_w, 2 * kSlots + c, 64);
        const T v = (row_ok && k >= 0 && k < gr.nz) ? u[row + k] : T(0);
        s = s + wz * v;
    }
    T t = (wx * wy) * s;
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) t = t + __shfl_xor(t, h, 64);
    if (l == 0) out[r] = t;
}

template <class T>
struct RowParams {
    const int* nodes;   // nrows x (i, j, k), storage indices
    const int* rowptr;  // nrows + 1
    const int* col;     // nnz, columns of g
    const T* w;         // nnz
    const T* g;         // ng values: one time row of the compact table
    int nrows, nnz, ng;
};

template <class T, bool DOT>
__global__ void __launch_bounds__(64) k_inject_rows(T* __restrict__ u, const T* __restrict__ m, NodeGrid gr,
                                                    RowParams<T> p, Wrap wrap, T* __restrict__ sacc) {
#pragma clang fp contract(off)
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= p.nrows) return;
    const int i = p.nodes[3 * i64(row)], j = p.nodes[3 * i64(row) + 1], k = p.nodes[3 * i64(row) + 2];
    if (!(i >= 0 && i < gr.nx && j >= 0 && j < gr.ny && k >= 0 && k < gr.nz)) return;
    const int e0 = p.rowptr[row], e1 = p.rowptr[row + 1];
    if (e0 < 0 || e1 > p.nnz || e0 > e1) return;
    T val = T(0);
    for (int e = e0; e < e1; ++e) {
        const int c = p.col[e];
        if (c < 0 || c >= p.ng) continue;
        val = val + p.w[e] * p.g[c];
    }
    const i64 rw = i64(j) * gr.sj + k;
    const i64 o = i64(i) * gr.si + rw;
    if constexpr (DOT) {
        sacc[row] = sacc[row] + u[o] * val;
    } else {
        const T v = u[o] + m[o] * val;
        u[o] = v;
#pragma unroll
        for (int q = 0; q < kMaxWrap; ++q)
            if (wrap.src[q] >= 1 && i == wrap.src[q] && wrap.dst[q] >= 0 && wrap.dst[q] < gr.nx)
                u[i64(wrap.dst[q]) * gr.si + rw] = v;
    }
}

template <class T>
RowParams<T> row_params(const int* nodes, const int* rowptr, const int* col, const T* w, const T* g, int nrows,
                        int nnz, int ng) {
    W3D_REQUIRE(nodes && rowptr, "row list: null rows");
    W3D_REQUIRE(nnz >= 0 && ng >= 0, "row list: negative counts");
    W3D_REQUIRE(nnz == 0 || (col && w && g), "row list: null entries");
    return RowParams<T>{nodes, rowptr, col, w, g, nrows, nnz, ng};
}

}  // namespace

template <class T>
void launch_record_w(const T* u, const GridView& gv, const int* index, const T* weight, T* out, int n,
                     hipStream_t s) {
    if (n <= 0) return;
    W3D_REQUIRE(u && index && weight && out, "weighted record: null argument");
    hipLaunchKernelGGL(k_record_w<T>, dim3(n), dim3(64), 0, s, u, node_grid(gv), index, weight, out, n);
    HIP_OK(hipGetLastError());
}

template <class T>
void launch_inject_rows(T* u, const T* m, const GridView& gv, const int* nodes, const int* rowptr, const int* col,
                        const T* w, const T* g, int nrows, int nnz, int ng, const Wrap& wrap, hipStream_t s) {
    if (nrows <= 0) return;
    W3D_REQUIRE(u && m, "row injection: null grid");
    const RowParams<T> p = row_params<T>(nodes, rowptr, col, w, g, nrows, nnz, ng);
    hipLaunchKernelGGL((k_inject_rows<T, false>), dim3(cdiv(nrows, 64)), dim3(64), 0, s, u, m, node_grid(gv), p, wrap,
                       static_cast<T*>(nullptr));
    HIP_OK(hipGetLastError());
}

template <class T>
void launch_rows_dot(const T* u, const GridView& gv, const int* nodes, const int* rowptr, const int* col, const T* w,
                     const T* g, int nrows, int nnz, int ng, T* sacc, hipStream_t s) {
    if (nrows <= 0) return;
    W3D_REQUIRE(u && sacc, "row dot: null argument");
    const RowParams<T> p = row_params<T>(nodes, rowptr, col, w, g, nrows, nnz, ng);
    // the DOT instantiation reads u and writes sacc alone
    hipLaunchKernelGGL((k_inject_rows<T, true>), dim3(cdiv(nrows, 64)), dim3(64), 0, s, const_cast<T*>(u),
                       static_cast<const T*>(nullptr), node_grid(gv), p, Wrap{}, sacc);
    HIP_OK(hipGetLastError());
}

#define W3D_POINTS_INST(T)                                                                                    \
    template void launch_record_w<T>(const T*, const GridView&, const int*, const T*, T*, int, hipStream_t);   \
    template void launch_inject_rows<T>(T*, const T*, const GridView&, const int*, const int*, const int*,     \
                                        const T*, const T*, int, int, int, const Wrap&, hipStream_t);         \
    template void launch_rows_dot<T>(const T*, const GridView&, const int*, const int*, const int*, const T*, \
                                     const T*, int, int, int, T*, hipStream_t);
W3D_POINTS_INST(double)
W3D_POINTS_INST(float)

}  // namespace wave3d
