// Heterogeneous-medium kernels (hip_medium.hip): u_tt = c(x,y,z)^2 (lap u + f) on the box, grid
// and boundary conditions of the constant-speed solver, with point sources and receivers.
//
// The per-node coefficient field m = c^2 tau^2 is stored like a time level (GridView, one ghost
// layer); a step reads u^{n-1}, u^{n-2} and m once and writes u^n once: 32 B per node in fp64.
#pragma once

#include "hip_kernels.hpp"

namespace wave3d {

// One time layer n >= 1 over `nbox` boxes (launch_step_medium, a MediumStep): u = (2 u1 - u2) + m lap(u1),
// or on the Taylor start (`first`) u = u1 + (0.5 m) lap(u1), rounded operation by operation in that order
// (a uniform m == coef reproduces launch_step's march kernel bit for bit). h2 = (hx*hx, hy*hy, hz*hz).
// err[0] = key of max |u| over the planes [ei0, ei1] (NaN ignored), err[1] untouched,
// err[2] = non-finite flag. variant: -1 = WAVE3D_MEDIUM_VARIANT or the default; bit 0 =
// non-temporal loads of m, bit 1 = 2 rows per lane instead of march_rows_per_thread().
//
// Absorbing sponge (gx, gy, gz all non-null; all null = none, the kernels above): device tables of
// X+2, Y+2, Z+2 factors in (0, 1] in storage indexing (gv.G == 1), G = gx[i] (gy[j] gz[k]) with
// each product rounded, and the damped leapfrog u = G ((2 u1 - G u2) + m lap(u1)), on the Taylor
// start u = G (u1 + (0.5 m) lap(u1)). Tables of ones give the undamped bits; err as above, of the
// damped values.
//
// Modes. A step runs in one MarchMode, named in MediumStep::mode; this is the one description of what
// each mode computes. A mode takes its own grids and no others (kMediumModes in hip_medium.hip has the
// set, and the rules below, one row per mode): every grid of the set non-null, every other mode grid
// null. All mode grids have the strides of u, are touched at the box nodes alone and never through the
// wrap, which applies to u alone. Every mode but kPlain is a leapfrog step (not `first`) and, at order 2,
// of variant 1 alone; every violation is rejected before the launch.
//
// kSave and kImage serve the adjoint-state gradient; u and err are those of the plain step bit for bit.
// kSave (lap_out) also stores lap(u1), the value that entered the update: one write-once stream.
// kImage (q, acc) also does acc = acc + u1 * q, the product rounded before the add (the imaging
// condition): a read-once stream and a read-modify-write one. Per node in fp64: 40 B (save), 56 B (image).
//
// kBorn (q, dm): the step of linearised (Born) modelling, image mode's transpose. u1 and u2 are
// levels of the perturbation field, q = lap of the background field (what save mode stored) and dm
// the perturbation of the coefficient, both read once and never written:
// u = ((2 u1 - u2) + m lap(u1)) + dm q, with the sponge
// u = G (((2 u1 - G u2) + m lap(u1)) + dm q), the product dm q rounded before its add. The wrap,
// err[0] and the non-finite flag are those of the plain step, of the Born-updated values; no store
// beside u's. q and dm must not share memory with u. Per node in fp64: 48 B (56 B with b).
//
// Space order (order = 2, 4 or 8; half-width M = order / 2). Order 2 is the 7-point kernel above
// and ignores `mirror`. Orders 4 and 8 run k_march_mh, a star stencil of 2M + 1 points per axis with
// the central second-derivative weights c_0 .. c_M (medium_weight): per axis t = c_0 v, then
// t = t + c_d (p_-d + p_+d) for d = 1 .. M, and lap = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2,
// every operation rounded on its own, the divisions correctly rounded on div_const's range (the
// paragraph "Division by h^2" below); the updates, the sponge and the save / image modes are those above (any variant is accepted and ignored). The x neighbours
// come from storage: the boxes keep M planes from both ends of the storage. mirror = (j_lo, j_hi,
// k_lo, k_hi), storage indices of reflecting (Dirichlet) faces, kNoMirror = none on that side
// (nullptr: none at all): a neighbour beyond a face f is read as -u1[2 f - j], the face itself as
// stored; the boxes lie strictly inside the faces, a pair of faces is at least M apart, and on a
// side without a face the boxes keep M nodes from the storage edge. Every violation is rejected
// before the launch, so no address outside a level's plane is formed.
//
// Variable density (b non-null; order 2 and the default variant 1 only, anything else is rejected
// before the launch): b = 1 / rho is a level like u1, x ghost planes filled, and m = rho c^2 tau^2.
// k_march_mb replaces lap(u1) in every form above (Taylor start, leapfrog, sponge, save, image) by
// D_b u1 = div(b grad u1): per axis, with centre c, neighbours u_-, u_+ and buoyancies b_c, b_-, b_+,
// f_+ = (0.5 (b_c + b_+)) (u_+ - c), f_- = (0.5 (b_c + b_-)) (c - u_-), t = f_+ - f_-, and
// D_b u1 = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2, every operation rounded on its own, the
// divisions correctly rounded on div_const's range ("Division by h^2" below; ops/reference.py
// laplace_density). Save mode stores D_b u1. b is read
// at the box nodes and their six neighbours, never written. Per node in fp64: 40 B (20 B in fp32).
//
// Born modelling with a density perturbation splits Born mode's work differently, in two modes that
// k_march_mb alone has (b non-null, so order 2 and variant 1).
// kScatter (s_out, dm, db): the background step that also stores the whole scattering term. db is the
// buoyancy perturbation, a level like b (x ghost planes filled), read at the box nodes and their six
// neighbours; r = D_db u1 is formed by D_b's operations with db's values in b's place, and
// s_out = dm D_b u1 + m r at the box nodes, both products rounded, then the add. u and err are those of
// the plain step bit for bit; s_out must not share memory with u, u1, u2, m, b, dm or db. Per node in
// fp64: 64 B.
// kBornAdd (sadd): the step of the perturbation field with the scattering term s = sadd read back,
// u = ((2 u1 - u2) + m D_b u1) + s, with the sponge u = G (((2 u1 - G u2) + m D_b u1) + s); s is read
// once and must not share memory with u. The wrap, err[0] and the non-finite flag are those of the
// updated values, as in Born mode. Per node in fp64: 48 B.
//
// Source illumination (the diagonal of the pseudo-Hessian; all three march kernels): kIllum (illum) is the
// plain step, kSaveIllum (lap_out, illum) the save step, that also does illum = illum + lap * lap, lap being
// the value that entered the update (D_b u1 with b), the product rounded before the add: one more
// read-modify-write stream. u, the wrap, err and lap_out are those of the plain step and of save mode
// bit for bit. illum must not share memory with u, u1, u2, m, b or lap_out. Per node in fp64: 48 B
// (illum), 56 B (save+illum); with b 56 B and 64 B.
//
// Division by h^2. All four march kernels and k_face_corr divide a numerator t by h^2 with div_const
// (stencil_math.hpp: three operations with y = RN(1 / h^2)), not with an IEEE division. The quotient is
// RN(t / h^2), the oracle's bits, for t = 0 and for 2^(emin + p + 1) <= |t| <= 2^(emax - ceil(log2 y)):
// in fp32 2^-101 = 3.9e-31 up to 2^120 for h^2 = 0.011, in fp64 2^-968 = 4.0e-292 up to 2^1016 (for
// h^2 >= 2 up to the largest finite value). Outside that range:
//   * a smaller numerator (down to the subnormals) gives a quotient at most D = 1 unit in the last place
//     from RN(t / h^2); measured by tests/test_div_const_cpu.py: up to 45 % of a binade's numerators
//     around 2^-131 (fp32) and 58 % around 2^-1026 (fp64), none found from 2^-108 (fp32) and 2^-1005
//     (fp64) on;
//   * a larger one, and t = +-inf, gives NaN where true division gives a finite quotient or +-inf: an
//     infinity in u1 makes its stencil neighbours NaN here and +-inf in the oracle, non-finite at the
//     same nodes (the non-finite flag is set either way; max |u| ignores a NaN but not an infinity);
//   * t = -0 gives +0; the 0 + ... in front of the sum hides it (true division's -0 ends as +0 too).
// So "hip equals cpu bit for bit" holds for fields whose numerators are zero or in range. The precursor
// ahead of a wave front decays through the lower bound; there the two backends may differ in the last
// place of a quotient (tests/test_gpu_medium_bits.py bounds it).
constexpr int kNoMirror = -(1 << 29);
// The modes of a step (above); the march kernels take one as their `int MODE` template argument.
enum MarchMode : int {
    kPlain = 0,
    kSave = 1,
    kImage = 2,
    kBorn = 3,
    kScatter = 4,
    kBornAdd = 5,
    kIllum = 6,
    kSaveIllum = 7
};
constexpr int kMarchModes = 8;
// its name in messages and in the Python binding: "plain", "save", "image", "born", "scatter", "born_add",
// "illum", "save_illum"
const char* march_mode_name(int mode);

// One step: what launch_step_medium runs. The mode's own grids are named members; the rest stay null.
template <class T>
struct MediumStep {
    bool first = false;
    const T *u1 = nullptr, *u2 = nullptr, *m = nullptr;
    T* u = nullptr;
    GridView gv;
    const Box* boxes = nullptr;
    int nbox = 0;
    int ei0 = 0, ei1 = 0;
    Wrap wrap;
    double h2[3] = {1, 1, 1};
    u64* err = nullptr;
    int chunk = 0;
    int variant = -1;
    int order = 2;
    const int* mirror = nullptr;                           // 4 entries, or null: no faces
    const T *gx = nullptr, *gy = nullptr, *gz = nullptr;   // the sponge tables
    const T* b = nullptr;                                  // the buoyancy 1 / rho
    MarchMode mode = kPlain;
    T* lap_out = nullptr;     // kSave, kSaveIllum
    const T* q = nullptr;     // kImage, kBorn
    T* acc = nullptr;         // kImage
    const T* dm = nullptr;    // kBorn, kScatter
    const T* db = nullptr;    // kScatter
    T* s_out = nullptr;       // kScatter
    const T* sadd = nullptr;  // kBornAdd
    T* illum = nullptr;       // kIllum, kSaveIllum
};
template <class T>
void launch_step_medium(const MediumStep<T>& st, hipStream_t s);

// Central second-derivative weight c_d of the star stencil of `order` (2, 4, 8), d = 0 .. order / 2:
// the double quotient of its two integers (order 4: -5/2, 4/3, -1/12; order 8: -205/72, 8/5, -1/5,
// 8/315, -1/560); the kernels cast it to the working type.
double medium_weight(int order, int d);

// Point sources: u(node[e]) += m(node[e]) * g[e] for e < n (the product rounded, then the add);
// an entry on a wrap source plane is also copied to its ghost plane. nodes = n x (i, j, k),
// logical indices; no two entries may name the same node (the caller checks).
template <class T>
void launch_inject(T* u, const T* m, const GridView& gv, const int* nodes, const T* g, int n,
                   const Wrap& wrap, hipStream_t s);

// Receivers: out[r] = u(node[r]) for r < n.
template <class T>
void launch_record(const T* u, const GridView& gv, const int* nodes, T* out, int n, hipStream_t s);

// Face correlation (hip_medium_corr.hip, k_face_corr): acc = acc + C(a, v) at the nodes of `nbox`
// boxes, the accumulation behind the density gradient dJ/drho of the adjoint pass (a = mu^{n+1},
// v = u^n). Per axis, with centre values a_c, v_c and neighbours a_-, a_+, v_-, v_+:
// p_+ = (a_+ - a_c) (v_+ - v_c), p_- = (a_c - a_-) (v_c - v_-), t = p_+ + p_-, and
// C = ((0 + t_x / hx2) + t_y / hy2) + t_z / hz2, every operation rounded on its own, the divisions
// correctly rounded on div_const's range ("Division by h^2" above; ops/reference.py face_correlation);
// C(a, v) == C(v, a) bit for bit. a, v and
// acc are levels with the strides of `gv` (one ghost layer, x ghost planes of a and v filled); the
// box contract is k_march_m's: boxes inside the owned region, so every box node has its six
// neighbours in storage. a and v are never written and acc only at the box nodes. Rejected before
// the launch: a box that touches a storage edge, strides smaller than the grid, and an acc that
// shares memory with a or v. Per node in fp64: 32 B (a, v, acc read and written), 16 B in fp32.
template <class T>
void launch_face_corr(const T* a, const T* v, T* acc, const GridView& gv, const Box* boxes, int nbox,
                      const double h2[3], int chunk, hipStream_t s);

// On-the-fly Fourier accumulation (hip_medium_dft.hip, k_dft_acc): for f = 0 .. nf - 1 in ascending order
// re[f] = re[f] + u c_row[f] and im[f] = im[f] + u s_row[f] at the nodes of `nbox` boxes, every product
// rounded before its add (ops/reference.py dft_accumulate; fp64 and fp32 results are bitwise equal to it).
// c_row / s_row: nf device values each, one row of the twiddle table cos(2 pi f p tau) / -sin(2 pi f p tau)
// uploaded once, so no host value travels with a step. u and the 2 nf accumulators are levels with the
// strides of `gv` (one ghost layer); the box contract is k_march_m's (boxes inside the owned region). u is
// never written, the accumulators only at the box nodes. A launch carries up to kDftNF frequencies on one
// read of u and a longer list is split into launches: with 4, u is 8 of a launch's 136 B per node in fp64,
// so 8 frequencies per launch would save 3 % of the traffic at most and need twice the registers in flight
// per lane. Rejected before any launch: nf < 1, a null pointer, a box that touches a storage edge, strides
// smaller than the grid, and an accumulator that shares memory with u or with another accumulator. Per
// node in fp64: 8 + 32 nf B for nf <= kDftNF (u read; re, im read and written), 4 + 16 nf B in fp32.
constexpr int kDftNF = 4;
template <class T>
void launch_dft_acc(const T* u, T* const* re, T* const* im, int nf, const T* c_row, const T* s_row,
                    const GridView& gv, const Box* boxes, int nbox, int chunk, hipStream_t s);

// Off-grid sources and receivers (hip_medium_points.hip): positions between the nodes act through
// 8 slots per axis (ops/reference.py interp_tables; the slots carry the periodic wrap in x and the odd
// reflection at the y/z faces already, as storage indices and signed weights).
//
// Weighted record (k_record_w): out[r] = sum over the 8 x 8 x 8 slots of receiver r, one wave64 per
// receiver. index / weight = n x 3 x 8 (x, y, z slots; storage indices). Lane 8a + b forms
// s = s + wz[c] u(ix[a], iy[b], iz[c]) for c = 0 .. 7 from s = 0, then t = (wx[a] wy[b]) s, and the wave
// sums t by the xor butterfly 32, 16, 8, 4, 2, 1; every product is rounded before its add. An index
// outside the storage contributes 0 and is never dereferenced.
template <class T>
void launch_record_w(const T* u, const GridView& gv, const int* index, const T* weight, T* out, int n,
                     hipStream_t s);

// Row injection (k_inject_rows): a CSR list of touched nodes, row = (i, j, k) storage indices with the
// entries rowptr[row] .. rowptr[row + 1] - 1, each a weight w[e] and a column col[e] of g (ng values:
// one time row of the compact source or residual table). Per row, one lane: val = val + w[e] g[col[e]]
// from val = 0 in entry order, then u = u + m val and the ghost-plane copies of launch_inject. The
// rows name distinct nodes (the caller checks); rows, entries and columns outside their tables are
// skipped.
template <class T>
void launch_inject_rows(T* u, const T* m, const GridView& gv, const int* nodes, const int* rowptr, const int* col,
                        const T* w, const T* g, int nrows, int nnz, int ng, const Wrap& wrap, hipStream_t s);

// Row dot (k_rows_dot, an instantiation of k_inject_rows): sacc[row] = sacc[row] + u(row) val with the
// val above, for the first `nrows` rows; nothing else is written. sacc must not share memory with u.
template <class T>
void launch_rows_dot(const T* u, const GridView& gv, const int* nodes, const int* rowptr, const int* col, const T* w,
                     const T* g, int nrows, int nnz, int ng, T* sacc, hipStream_t s);

// default variant of launch_step_medium: 1 ("nt"), or env WAVE3D_MEDIUM_VARIANT = "plain" (0),
// "r2" (2), "r2nt" (3) for ablation
int medium_variant();

}  // namespace wave3d
