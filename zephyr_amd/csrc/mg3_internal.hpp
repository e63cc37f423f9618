// What the units of the 3-D multigrid preconditioner share (mg3d.hip, mg3_keep.hip, mg3_coarse.hip, mg3_depth.hip: each says at its top what it
// holds): the structs of a hierarchy and the few functions that cross units.
#pragma once
#include "helm_internal.hpp"
#include "direct.hpp"
#include <algorithm>
#include <complex>
#include <memory>

struct Mg3Level {
    helm_op *op = nullptr;
    int nz = 0, ny = 0, nx = 0;
    long long N = 0;
    cplx *u = nullptr, *f = nullptr, *r = nullptr, *t = nullptr;      // [batch][N]
    size_t vbytes = 0;
};

struct Mg3Keep;
struct Mg3Precond {
    std::vector<Mg3Level> lv;
    Mg3Keep *keep = nullptr;      // layer-preserving hierarchy instead of the standard one
    int kept_levels = 0; double ppw_direct = 0.0;     // (layer-preserving) coarsenings above the directly solved level and its points per wavelength: the class its iteration counts are booked under
    cplx *cinvT = nullptr;        // transposed dense inverse of the coarsest operator
    int nc = 0, batch = 0;
    double omega_j = 0.8, beta = 0.6, cpml_m = 30.0;
    int nu1 = 1, nu2 = 1, min_n = 8;
    bool fine32 = false;          // (layer-preserving cycle) the finest level's work vectors u, t, r hold complex64 -- see cycle_keep
};

struct Ax3 {
    std::vector<double> x, gam;     // node coordinates, damping gamma at the nodes
    std::vector<char> lay;          // node belongs to an absorbing layer (never dropped)
    int n() const { return (int)x.size(); }
};
struct PTab { int c0, c1; double w0, w1; };         // fine node -> its two coarse nodes and weights (kept node: c0 = c1, w = 1, 0)
struct RTab { int f; double wl, wc, wr; };          // coarse node -> fine nodes f-1, f, f+1 with normalised weights

// shape of the plane-by-plane elimination of a level (mg3_bt_shape): bt_setup allocates by it and the depth decision budgets by it
struct BtShape {
    int axis = 0, np = 0, m = 0;    // sweep axis (the longest: the planes normal to it are the smallest), its np planes of m nodes
    bool own = true;                // k_bt_apply (memory-bound product) instead of the generic batched GEMM
    bool f32 = false;               // plane inverses kept in single precision (Tinv32) instead of Tinv
    int ksplit = 1, kc = 0, mpad = 0, ld32 = 0;
    size_t wbytes = 0, tbytes = 0, tbytes32 = 0;    // one double-precision plane; Tinv (f32: the set-up's four ping-pong planes); Tinv32
};
struct BtGeom { int axis, np, na, nb, m; long long ss, sa, sb, N; };
struct Bt3 : BtShape {              // direct solver of the coarsest level
    int na = 0, nb = 0, batch = 0, nparts = 1;
    int mid = 0;                    // twisted elimination: planes 0 .. mid-1 from the left, np-1 .. mid+1 from the right, plane mid last
    int device = 0;                 // Tinv comes from the size-keyed buffer pool (the next frequency takes it over without a hipMalloc)
    long long ss = 0, sa = 0, sb = 0, N = 0;      // node strides of the sweep axis / the two in-plane axes
    cplx *Tinv = nullptr;           // np x (mpad x m): inverse of the transposed Schur complement of plane k (rows >= m are zero)
    float2 *Tinv32 = nullptr;       // single-precision copy, np x (m x ld32), used INSTEAD of Tinv (f32 = true: Tinv is then not kept)
    cplx *Y[2] = {nullptr, nullptr};      // per chain: batch x mpad, packed right-hand side of one plane (columns >= m stay zero)
    cplx *Z = nullptr;                    // np x batch x m: forward-substituted planes, then the solution
    cplx *parts[2] = {nullptr, nullptr};  // per chain: ksplit x batch x m partial products of the split-K product
    helm_op *aux = nullptr;         // carries the stream (and the look-ahead stream) of the right-hand chain
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
};

// Nested-dissection alternative to Bt3 (helm_tuning.mg3_coarse): the multifrontal solver of the 2-D path (direct.hpp) run over the (ny, nx) grid of
// z-columns of the level -- a "cell" is a column of nz unknowns (NdPlan::dof = nz), its 27-point coupling to the nine neighbour columns a
// block-tridiagonal nz x nz block.  The top separator is one plane of the level (the size Bt3 inverts np times); below it the fronts shrink.
struct Nd3 {
    std::shared_ptr<NdPlanDev> pd;
    NdFactor *f = nullptr;
    cplx *ws = nullptr; size_t ws_bytes = 0;        // solve scratch (nd_solve_ws_elems), from the pool
    int device = 0, batch = 0;
    bool on() const { return f != nullptr; }
};
// what the column dissection of a level costs: flops of its factorisation, bytes of its factors and of the factorisation scratch, rows of its top separator
struct Nd3Cost { double flops = 0, fac_bytes = 0, ws_bytes = 0; int top = 0; };

struct Mg3Keep {
    std::vector<cplx *> dl1;                         // per level: l1-Jacobi inverse diagonal
    std::vector<size_t> dl1_bytes; int device = 0;   // (everything here comes from the size-keyed pool: hipMalloc / hipFree beside another handle's solve stall)
    std::vector<std::pair<void *, size_t>> tabs;     // the transfer tables' buffers
    std::vector<PTab *> pt[3]; std::vector<RTab *> rt[3];   // per transfer (level l -> l+1) and axis (z, y, x): device tables
    Bt3 bt;
    Nd3 nd;
    double omega_l1 = 1.6;
};

// `tune`: the options of the set-up in progress, read once by mg3_setup and passed down
// ---- mg3d.hip
bool mg3_trace();                                                     // HELM_MG3_TRACE=1 (a diagnostic: environment only, include/helm.h)
bool mg3_level_vectors(helm_op *op, Mg3Level &L, int batch);          // the level's four work vectors, from the pool
size_t mg3_available_bytes(int device, size_t *total);                // free device memory plus what the library's own pool holds idle
// ---- mg3_keep.hip
void mg3_keep_level_dims(const helm_op *op, int l, int out[3]);       // nodes per axis (z, y, x) of level l of the layer-preserving hierarchy
int mg3_keep_setup(helm_op *op, Mg3Precond *P, int batch, int ncoarsen, double tauM, const helm_tuning &tune);
void mg3_keep_free(Mg3Precond *P);
// ---- mg3_coarse.hip
BtShape mg3_bt_shape(const int dims[3], int batch, const helm_tuning &tune);
Nd3Cost mg3_nd_cost(int nz, int ny, int nx, int leaf);
bool mg3_coarse_is_nd(int nz, int ny, int nx, const helm_tuning &tune);
int mg3_coarse_setup(helm_op *op, Mg3Keep *K, const Mg3Level &L, int batch, const helm_tuning &tune);
int mg3_coarse_solve(helm_op *op, Mg3Keep *K, const Mg3Level &L, const cplx *f, cplx *u, int nrhs);       // u = A^-1 f on the last level (f, u: [nrhs][N])
void mg3_coarse_free(Mg3Keep *K);
// ---- mg3_depth.hip
int mg3_choose_depth(helm_op *op, int batch, double ppw, const helm_tuning &tune);      // layer-preserving coarsenings above the directly solved level
