// The two Hessian diagonals of the exact MiniZephyr derivatives (survey_frechet.hip) from stored columns, each kernel beside the C entry point that launches it:
// the pseudo-Hessian diagonal, and the exact diagonal of the Gauss-Newton Hessian (the autocorrelation planes of a set of columns and the per-cell trace), which
// is built from the coefficients of the first.  survey_internal.hpp holds what they share with the derivative kernels.  The last section holds the per-cell 2 x 2
// blocks of the joint (c, rho) Hessian under either of the two: the same walks and coefficient sets with three sums per cell, so they live beside what they extend.
#include "survey_internal.hpp"

// ------------------------------------------------------------------------------------------
// the pseudo-Hessian diagonal of the exact derivatives: H[i] += alpha W[i] sum_s || (d A / d p_i) u^_s ||^2
// ------------------------------------------------------------------------------------------
// A unit perturbation of cell i (of its velocity, or of its buoyancy) touches only the rows j of the 3 x 3 block around i, and in those only the lags that point
// back into the block (frechet.pseudoHessianDiagonal states the same).  Per cell that is a small matrix E_i, independent of the source:
//     row i             nine coefficients: mz_star on the differentiated row factors and d kappa_i / dc b_i (velocity), on the row itself with the averages
//                       1 / 2 and kappa_i (buoyancy)
//     row j = i - o     velocity: the one mass weight m_o d kappa_i / dc b_i at the lag o, which multiplies u[i] -- the eight rows together are
//                       |d kappa_i / dc b_i|^2 sum_j m_o^2 |u[i]|^2, one real weight S_i.
//                       buoyancy: m_o kappa_i + T_o(j) / 2 at the lag o and -T_o(j) / 2 at the centre, T the row's own stiffness factor (mz_stiffness); a corner
//                       row has +-tzx(j) / 2 at the two lags beside o as well.  2 coefficients per edge row, 4 per corner row: 9 + 8 + 16 = 33.
//     Gardner           velocity + chain_i x buoyancy, coefficient by coefficient (the mass weight of the velocity part joins the lag o of row j).
// The stored fields are conj(u^): the coefficients are conjugated once instead (|conj(E) conj(u)| = |E u|).
//
// The walk: a workgroup of PH_WAVES waves owns OP_TILE_X cells of one grid row, one lane per cell plus a halo lane at either end.  The lane's E_i stays in
// registers for the whole kernel; the columns go to the waves in groups of PH_UNROLL (group g to wave g mod PH_WAVES).  Per column a lane loads the three rows
// z - 1, z, z + 1 of its own x (3 PH_UNROLL loads in flight), takes the left and right neighbours from the adjacent lanes, forms the up to nine row sums and adds
// their squared moduli to one double.  The waves add their sums into one LDS row in wave order and wave 0 adds alpha W (.) sum to H: one writer per cell, a
// fixed order, no atomics -- the same bits on every run.  Rows z - 1 and z + 1 are the halo: the workgroups of the neighbouring rows load them at the same time.
// PACKED: E_i is read from an array [ph_ncoef(MODE)][N] that k_pseudo_hessian_coefficients wrote (the same function, one lane per cell) instead of being built
// by every wave of the workgroup.
enum { PH_VELOCITY = 0, PH_BUOYANCY = 1, PH_GARDNER = 2 };
constexpr int PH_WAVES = 4;         // waves per workgroup
constexpr int PH_UNROLL = 4;        // columns a wave loads together

// e[a]: the edge rows j = i - o, o = (-1, 0), (1, 0), (0, -1), (0, 1): {lag o, centre}.  k[a]: the corner rows, a = 2 [sz > 0] + [sx > 0]: {lag o, lag (0, sx) -> cell
// i - (sz, 0), lag (sz, 0) -> cell i - (0, sx), centre}.  S: the real weight of |u[i]|^2 (velocity alone).
struct PhCoef { cplx c[9]; cplx e[4][2]; cplx k[4][4]; double S; };
__host__ __device__ constexpr int ph_ncoef(int mode) { return mode == PH_VELOCITY ? 10 : 33; }

template <int MODE>
__device__ __forceinline__ void ph_coefficients(const MzParams &P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ chain,
                                                int iz, int ix, PhCoef &E) {
    const cplx zero = cmake(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < 9; ++k) E.c[k] = zero;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        E.e[a][0] = E.e[a][1] = zero;
        E.k[a][0] = E.k[a][1] = E.k[a][2] = E.k[a][3] = zero;
    }
    E.S = 0.0;
    const long long i = (long long)iz * P.nx + ix;
    const cplx ci = c[i];
    const cplx kap = mz_kappa(P, ci);
    const double ch = MODE == PH_GARDNER ? chain[i] : 1.0;
    const cplx w = MODE != PH_BUOYANCY ? cscale(mz_kappa_dc(P, ci), 1.0 / rho[i]) : zero;       // d K_i / d c_i at the density of the handle
    if (iz >= 1 && iz <= P.nz - 2 && ix >= 1 && ix <= P.nx - 2) {           // row i: the assembly's star on the unit perturbation
        double bn[9];
        cplx Kn[9];
        if (MODE != PH_BUOYANCY) {
            const double b0 = 1.0 / rho[i];
#pragma unroll
            for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
                for (int sx = -1; sx <= 1; ++sx) {
                    bn[mz_slot(sz, sx)] = (b0 + 1.0 / rho[i + (long long)sz * P.nx + sx]) / 2.0;
                    Kn[mz_slot(sz, sx)] = zero;
                }
            Kn[4] = w;
            mz_star(P, mz_row_dc_at(P, c, iz, ix), bn, Kn, E.c);
        }
        if (MODE != PH_VELOCITY) {
            cplx more[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { bn[k] = 0.5; Kn[k] = zero; }
            bn[4] = 1.0;
            Kn[4] = kap;
            mz_star(P, mz_row_at(P, c, iz, ix), bn, Kn, more);
#pragma unroll
            for (int k = 0; k < 9; ++k) E.c[k] = MODE == PH_GARDNER ? cadd(E.c[k], cscale(more[k], ch)) : more[k];
        }
    }
    double m2 = 0.0;
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            if (sz == 0 && sx == 0) continue;
            const int jz = iz - sz, jx = ix - sx;                 // row j sees cell i at the lag (sz, sx)
            if (jz < 1 || jz > P.nz - 2 || jx < 1 || jx > P.nx - 2) continue;
            const double m = (sz == 0 || sx == 0) ? MZ_WD : MZ_WE;
            if (MODE == PH_VELOCITY) { m2 += m * m; continue; }
            const MzStiff T = mz_stiffness<false>(P, mz_row_at(P, c, jz, jx));
            const cplx t = sx == 0 ? T.tv[(sz + 1) / 2] : (sz == 0 ? T.th[(sx + 1) / 2] : T.tc[(sz + 1) / 2][(sx + 1) / 2]);
            cplx lag = cscale(cadd(cscale(kap, m), cscale(t, 0.5)), ch);
            if (MODE == PH_GARDNER) lag = cadd(lag, cscale(w, m));
            const cplx ctr = cscale(t, -0.5 * ch);
            if (sz != 0 && sx != 0) {
                const int a = 2 * ((sz + 1) / 2) + (sx + 1) / 2;
                E.k[a][0] = lag;
                E.k[a][1] = cscale(T.tzx, -0.5 * ch);            // row j's lag (0, sx): the horizontal neighbours take -tzx
                E.k[a][2] = cscale(T.tzx, 0.5 * ch);             // row j's lag (sz, 0)
                E.k[a][3] = ctr;
            } else {
                const int a = sx == 0 ? (sz + 1) / 2 : 2 + (sx + 1) / 2;
                E.e[a][0] = lag;
                E.e[a][1] = ctr;
            }
        }
    if (MODE == PH_VELOCITY) E.S = m2 * (w.x * w.x + w.y * w.y);
#pragma unroll
    for (int k = 0; k < 9; ++k) E.c[k] = cconj(E.c[k]);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        E.e[a][0] = cconj(E.e[a][0]); E.e[a][1] = cconj(E.e[a][1]);
#pragma unroll
        for (int q = 0; q < 4; ++q) E.k[a][q] = cconj(E.k[a][q]);
    }
}

// the packed order of a cell's coefficients: c[0..8], then (velocity) S, or e[0..3][0..1], k[0..3][0..3]
template <int MODE, class FN>
__device__ __forceinline__ void ph_each(PhCoef &E, FN &&fn) {
#pragma unroll
    for (int k = 0; k < 9; ++k) fn(k, E.c[k]);
    if (MODE == PH_VELOCITY) {
        cplx s = cmake(E.S, 0.0);
        fn(9, s);
        E.S = s.x;
    } else {
#pragma unroll
        for (int a = 0; a < 4; ++a) { fn(9 + 2 * a, E.e[a][0]); fn(10 + 2 * a, E.e[a][1]); }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int q = 0; q < 4; ++q) fn(17 + 4 * a + q, E.k[a][q]);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void k_pseudo_hessian_coefficients(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho,
                                                                     const double *__restrict__ chain, cplx *__restrict__ Epk) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    PhCoef E;
    ph_coefficients<MODE>(P, c, rho, chain, (int)(i / P.nx), (int)(i % P.nx), E);
    ph_each<MODE>(E, [&](int q, cplx &v) { Epk[(long long)q * N + i] = v; });
}

template <class F, int MODE, bool PACKED>
__global__ __launch_bounds__(64 * PH_WAVES) void k_pseudo_hessian(F U, int nsrc, long long ld, MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho,
                                                                  const double *__restrict__ chain, const cplx *__restrict__ Epk, double alpha,
                                                                  const double *__restrict__ W, double *__restrict__ H) {
    __shared__ double part[64];
    const int nz = P.nz, nx = P.nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z = (int)(blockIdx.x / ntx);
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    const long long N = (long long)nz * nx, i = (long long)z * nx + x;
    PhCoef E;
    if (store) {
        if (PACKED) ph_each<MODE>(E, [&](int q, cplx &v) { v = Epk[(long long)q * N + i]; });
        else ph_coefficients<MODE>(P, c, rho, chain, z, x, E);
    } else {
        ph_each<MODE>(E, [&](int, cplx &v) { v = cmake(0.0, 0.0); });       // (a halo lane adds nothing)
    }
    double acc = 0.0;
    const int ngroups = (nsrc + PH_UNROLL - 1) / PH_UNROLL;
    for (int g = wave; g < ngroups; g += PH_WAVES) {          // (wave-uniform: the lane exchanges stay complete)
        const int s0 = g * PH_UNROLL, ncol = min(PH_UNROLL, nsrc - s0);
        typename F::raw raw[PH_UNROLL][3];
        double sc[PH_UNROLL];
#pragma unroll
        for (int j = 0; j < PH_UNROLL; ++j) {
            sc[j] = U.scale(s0 + min(j, ncol - 1));
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int zz = z - 1 + r;
                raw[j][r] = (xin && j < ncol && zz >= 0 && zz < nz) ? U.load((long long)(s0 + j) * ld + (long long)zz * nx + x) : typename F::raw{};
            }
        }
#pragma unroll
        for (int j = 0; j < PH_UNROLL; ++j) {
            cplx v[9];                                          // the 3 x 3 block around the lane's cell in the slot order of the operator
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                v[3 * r + 1] = U.scaled(raw[j][r], sc[j]);
                lane_left_right(v[3 * r + 1], v[3 * r], v[3 * r + 2]);
            }
            cplx r0 = cmake(0.0, 0.0);
#pragma unroll
            for (int k = 0; k < 9; ++k) cfma(r0, E.c[k], v[k]);
            double sum = cabs2(r0);
            if (MODE == PH_VELOCITY) sum += E.S * cabs2(v[4]);
            else {
#pragma unroll
                for (int a = 0; a < 4; ++a) {                   // the edge row j = i - o sits at the slot of -o
                    const int sz = a < 2 ? 2 * a - 1 : 0, sx = a < 2 ? 0 : 2 * (a - 2) - 1;
                    cplx r1 = cmul(E.e[a][0], v[4]);
                    cfma(r1, E.e[a][1], v[mz_slot(-sz, -sx)]);
                    sum += cabs2(r1);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    const int sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
                    cplx r2 = cmul(E.k[a][0], v[4]);
                    cfma(r2, E.k[a][1], v[mz_slot(-sz, 0)]);     // j + (0, sx) = i - (sz, 0)
                    cfma(r2, E.k[a][2], v[mz_slot(0, -sx)]);     // j + (sz, 0) = i - (0, sx)
                    cfma(r2, E.k[a][3], v[mz_slot(-sz, -sx)]);
                    sum += cabs2(r2);
                }
            }
            if (j < ncol) acc += sum;
        }
    }
    for (int w = 0; w < PH_WAVES; ++w) {
        if (wave == w) part[lane] = w == 0 ? acc : part[lane] + acc;
        __syncthreads();
    }
    if (wave == 0 && store) H[i] = H[i] + (W ? alpha * W[i] : alpha) * part[lane];
}

static int pseudo_hessian_launch(helm_op *op, HostField U, int nsrc, long long ld, int mode, const void *dChain, const void *dE, double alpha, const void *dW, void *dH) {
    helm_tuning_refresh();
    const char *what = U.c64 ? "helm_pseudo_hessian_accumulate_c64_device" : "helm_pseudo_hessian_accumulate_device";       // (each entry point refuses under its own name)
    if (!op || !U.ok() || !dH || nsrc < 1 || ld < op->N || !(alpha >= 0.0) || mode < PH_VELOCITY || mode > PH_GARDNER) return HELM_ERR_ARG;
    if ((mode == PH_GARDNER) != (dChain != nullptr) && !dE) return HELM_ERR_ARG;       // (the chain goes with the Gardner mode alone; packed coefficients carry it)
    if (int rc = mz_handle_args(op, what)) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dChain) | ((uintptr_t)dW) | ((uintptr_t)dH)) & 7) || (((uintptr_t)dE) & 15)) return HELM_ERR_ARG;
    const size_t hbytes = (size_t)op->N * 8;
    if (ranges_overlap(U.u, U.bytes(nsrc, ld), dH, hbytes) || (dW && ranges_overlap(dW, hbytes, dH, hbytes)) || (dChain && ranges_overlap(dChain, hbytes, dH, hbytes)) ||
        (dE && ranges_overlap(dE, (size_t)op->N * ph_ncoef(mode) * sizeof(cplx), dH, hbytes)))
        return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle holds no assembled operator", what);
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * op->nz)), block(64 * PH_WAVES);
    const cplx *c = (const cplx *)op->d_c, *E = (const cplx *)dE;
    const double *rho = (const double *)op->d_rho, *chain = (const double *)dChain, *W = (const double *)dW;
    double *H = (double *)dH;
#define PH_GO(MODE) do { \
        if (E) HELM_LAUNCH((k_pseudo_hessian<decltype(F), MODE, true>), grid, block, 0, op->stream, F, nsrc, ld, P, c, rho, chain, E, alpha, W, H); \
        else HELM_LAUNCH((k_pseudo_hessian<decltype(F), MODE, false>), grid, block, 0, op->stream, F, nsrc, ld, P, c, rho, chain, E, alpha, W, H); } while (0)
    return U.with([&](auto F) {
        if (mode == PH_VELOCITY) PH_GO(PH_VELOCITY);
        else if (mode == PH_BUOYANCY) PH_GO(PH_BUOYANCY);
        else PH_GO(PH_GARDNER);
        return launched(op);
    });
#undef PH_GO
}

// H[i] += alpha (W ? W[i] : 1) sum_{s<nsrc} sum_j |sum_n E_i[j][n] U[s ld + n]|^2 for i < N: U the stored (conjugated) fields, E_i the derivative of the operator the
// handle holds with respect to the velocity of cell i (mode 0, at the handle's density), to its buoyancy (mode 1), or to its velocity with the buoyancy following
// it by dChain (mode 2: dChain N float64, NULL otherwise).  dE NULL: the coefficients are built in the kernel; else the array of
// helm_pseudo_hessian_coefficients_device for the same mode and chain.  Returns when H is complete.
extern "C" int helm_pseudo_hessian_accumulate_packed_device(helm_op *op, const void *dU, int nsrc, long long ld, int mode, const void *dChain, const void *dE,
                                                            double alpha, const void *dW, void *dH) {
    return pseudo_hessian_launch(op, HostField::c128(dU), nsrc, ld, mode, dChain, dE, alpha, dW, dH);
}
extern "C" int helm_pseudo_hessian_accumulate_packed_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int mode, const void *dChain,
                                                                const void *dE, double alpha, const void *dW, void *dH) {
    return pseudo_hessian_launch(op, HostField::packed(dU32, dExp), nsrc, ld, mode, dChain, dE, alpha, dW, dH);
}
extern "C" int helm_pseudo_hessian_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, int mode, const void *dChain, double alpha, const void *dW,
                                                     void *dH) {
    return helm_pseudo_hessian_accumulate_packed_device(op, dU, nsrc, ld, mode, dChain, nullptr, alpha, dW, dH);
}
extern "C" int helm_pseudo_hessian_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int mode, const void *dChain,
                                                         double alpha, const void *dW, void *dH) {
    return helm_pseudo_hessian_accumulate_packed_c64_device(op, dU32, dExp, nsrc, ld, mode, dChain, nullptr, alpha, dW, dH);
}

// dE[ph_ncoef(mode)][N] complex128: the coefficients E_i of every cell, what the _packed entry points read (10 planes for mode 0, 33 otherwise)
extern "C" int helm_pseudo_hessian_coefficients_device(helm_op *op, int mode, const void *dChain, void *dE) {
    helm_tuning_refresh();
    if (!op || !dE || mode < PH_VELOCITY || mode > PH_GARDNER || (mode == PH_GARDNER) != (dChain != nullptr)) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_pseudo_hessian_coefficients_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dChain) & 7) || (((uintptr_t)dE) & 15)) return HELM_ERR_ARG;
    if (dChain && ranges_overlap(dChain, (size_t)op->N * 8, dE, (size_t)op->N * ph_ncoef(mode) * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_pseudo_hessian_coefficients_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    const cplx *c = (const cplx *)op->d_c;
    const double *rho = (const double *)op->d_rho, *chain = (const double *)dChain;
    if (mode == PH_VELOCITY) HELM_LAUNCH(k_pseudo_hessian_coefficients<PH_VELOCITY>, grid, dim3(256), 0, op->stream, P, c, rho, chain, (cplx *)dE);
    else if (mode == PH_BUOYANCY) HELM_LAUNCH(k_pseudo_hessian_coefficients<PH_BUOYANCY>, grid, dim3(256), 0, op->stream, P, c, rho, chain, (cplx *)dE);
    else HELM_LAUNCH(k_pseudo_hessian_coefficients<PH_GARDNER>, grid, dim3(256), 0, op->stream, P, c, rho, chain, (cplx *)dE);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the exact diagonal of the Gauss-Newton Hessian: H[i] += alpha W[i] sum_s sum_r |g_r^T (d A / d p_i) u^_s|^2
// ------------------------------------------------------------------------------------------
// With E_i the coefficients of the section above, Gamma_i[j, j'] = sum_r g_r[j] conj(g_r[j']) and Phi_i[n, n'] = sum_s u_s[n] conj(u_s[n']) over the cells of the
// 3 x 3 block around i, the double sum is Re sum conj(E[j', n']) Gamma[j, j'] E[j, n] Phi[n, n'] (frechet.gaussNewtonDiagonal states the same).  Two cells of a
// block are at most two steps apart in either direction, so Gamma and Phi are read off the autocorrelation planes at the 25 lags of (-2..2)^2, of which the
// half plane (0, 0), (0, 1), (0, 2), (1, -2..2), (2, -2..2) is stored; the other twelve are conjugates, read at the shifted cell.  k_lag_gram makes the 13 planes of
// a set of columns, k_gauss_newton_diagonal evaluates the trace per cell.
//
// k_lag_gram: C[l][i] += sum_s U[s ld + i] conj(U[s ld + i + off_l]) for the 13 lags l and every cell i whose partner i + off_l is inside the grid; the other
// entries are not touched.  The walk of k_lag_imaging with one field and a halo of two: a workgroup of LG_WAVES waves owns a tile of LG_TILE_X x LG_ROWS cells, one
// lane per cell of a row plus two halo lanes at either end.  Column s goes to wave s mod LG_WAVES, which keeps the 13 LG_ROWS sums of its lane's cells in REGISTERS
// over all its columns: per column it loads the rows z0 .. z0 + LG_ROWS + 1 of its own x (the half plane looks down only), gets the partners one and two cells
// to the left and right from the adjacent lanes and does 13 LG_ROWS complex FMAs.  Then the waves add their sums into ONE LDS tile in wave order and wave r adds
// row r to C: one writer per entry, a fixed order, no atomics -- the same bits on every run.  Per cell and column 16 (8) B times (1 + 2 / LG_ROWS)(1 + 4 / LG_TILE_X).
constexpr int LG_TILE_X = 60;       // output cells per wave along x: 64 lanes less two halo lanes at either end
constexpr int LG_ROWS = 4;          // output rows per workgroup: 104 accumulator doubles per lane
constexpr int LG_WAVES = 4;         // waves per workgroup
constexpr int LG_NLAG = 13;
static_assert(LG_ROWS <= LG_WAVES, "wave r finishes row r");
__host__ __device__ constexpr int lg_plane(int dz, int dx) { return dz == 0 ? dx : 3 + 5 * (dz - 1) + (dx + 2); }      // (dz, dx) of the stored half plane -> l

template <class F>
__global__ __launch_bounds__(64 * LG_WAVES) void k_lag_gram(F U, long long ld, int nsrc, cplx *__restrict__ C, int nz, int nx) {
    __shared__ cplx part[LG_ROWS][LG_NLAG][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + LG_TILE_X - 1) / LG_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * LG_TILE_X + lane - 2, z0 = (int)(blockIdx.x / ntx) * LG_ROWS;
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 2 && lane < 2 + LG_TILE_X && x < nx;
    const long long N = (long long)nz * nx;
    cplx acc[LG_ROWS][LG_NLAG];
#pragma unroll
    for (int r = 0; r < LG_ROWS; ++r)
#pragma unroll
        for (int l = 0; l < LG_NLAG; ++l) acc[r][l] = cmake(0.0, 0.0);
    for (int s = wave; s < nsrc; s += LG_WAVES) {               // (wave-uniform: the lane exchanges stay complete)
        const double sc = U.scale(s);
        typename F::raw raw[LG_ROWS + 2];
#pragma unroll
        for (int r = 0; r < LG_ROWS + 2; ++r) {
            const int z = z0 + r;
            raw[r] = (xin && z < nz) ? U.load((long long)s * ld + (long long)z * nx + x) : typename F::raw{};      // (zero outside the grid: such pairs are never stored)
        }
        cplx t[LG_ROWS + 2];
#pragma unroll
        for (int r = 0; r < LG_ROWS + 2; ++r) t[r] = U.scaled(raw[r], sc);
#pragma unroll
        for (int wr = 0; wr < LG_ROWS + 2; ++wr) {              // row z0 + wr is the partner row of the output rows wr (dz = 0), wr - 1 and wr - 2
            cplx sh[5];                                         // the row at x - 2 .. x + 2 (a halo lane's missing neighbours are its own value: never stored)
            sh[2] = t[wr];
            sh[0] = cmake(__shfl_up(t[wr].x, 2, 64), __shfl_up(t[wr].y, 2, 64));
            sh[1] = cmake(__shfl_up(t[wr].x, 1, 64), __shfl_up(t[wr].y, 1, 64));
            sh[3] = cmake(__shfl_down(t[wr].x, 1, 64), __shfl_down(t[wr].y, 1, 64));
            sh[4] = cmake(__shfl_down(t[wr].x, 2, 64), __shfl_down(t[wr].y, 2, 64));
#pragma unroll
            for (int dz = 0; dz <= 2; ++dz) {
                const int r = wr - dz;
                if (r < 0 || r >= LG_ROWS) continue;
#pragma unroll
                for (int dx = (dz == 0 ? 0 : -2); dx <= 2; ++dx) cfma_conj(acc[r][lg_plane(dz, dx)], sh[dx + 2], t[r]);      // += t[r] conj(partner)
            }
        }
    }
    for (int w = 0; w < LG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < LG_ROWS; ++r)
#pragma unroll
                for (int l = 0; l < LG_NLAG; ++l) part[r][l][lane] = w == 0 ? acc[r][l] : cadd(part[r][l][lane], acc[r][l]);
        }
        __syncthreads();
    }
    if (wave < LG_ROWS) {
        const int z = z0 + wave;
        if (store && z < nz) {
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int dz = 0; dz <= 2; ++dz)
#pragma unroll
                for (int dx = (dz == 0 ? 0 : -2); dx <= 2; ++dx) {
                    if (z + dz >= nz || x + dx < 0 || x + dx >= nx) continue;       // (the partner is outside the grid: the entry stays as it is)
                    cplx *p = C + (long long)lg_plane(dz, dx) * N + i;
                    *p = cadd(*p, part[wave][lg_plane(dz, dx)][lane]);
                }
        }
    }
}

// C[l][i] += sum_{s<nsrc} U[s ld + i] conj(U[s ld + i + off_l]) for the 13 lags l of the stored half plane and the cells i of the handle's grid whose partner is
// inside it: U [nsrc][ld], C [13][N] complex128.  C must not overlap U.  Returns when C is complete.
static int lag_gram_launch(helm_op *op, HostField U, int nsrc, long long ld, void *dC) {
    helm_tuning_refresh();
    if (!op || !U.u || !dC || nsrc < 1 || ld < op->N) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, U.c64 ? "helm_lag_gram_accumulate_c64_device" : "helm_lag_gram_accumulate_device")) return rc;       // (each under its own name)
    if (ranges_overlap(U.u, U.bytes(nsrc, ld), dC, (size_t)op->N * LG_NLAG * sizeof(cplx))) return HELM_ERR_ARG;
    if (!U.ok() || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;       // (the exponents and every alignment come after the handle)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)(((op->nx + LG_TILE_X - 1) / LG_TILE_X) * ((op->nz + LG_ROWS - 1) / LG_ROWS)));
    return U.with([&](auto F) {
        HELM_LAUNCH(k_lag_gram<decltype(F)>, grid, dim3(64 * LG_WAVES), 0, op->stream, F, ld, nsrc, (cplx *)dC, op->nz, op->nx);
        return launched(op);
    });
}
extern "C" int helm_lag_gram_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, void *dC) {
    return lag_gram_launch(op, HostField::c128(dU), nsrc, ld, dC);
}
extern "C" int helm_lag_gram_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, void *dC) {
    return lag_gram_launch(op, HostField::packed(dU32, dExp), nsrc, ld, dC);
}

// k_gauss_newton_diagonal: one lane per cell.  The lane's E_i is the coefficient set of ph_coefficients (conjugated once there: the planes it is fed are those
// of the stored conjugates, and conjugating E, Gamma and Phi together leaves the real trace as it is) as a flat list of GN_NCOEF (row, column) entries over the
// slots of the block.  Gamma now couples the rows of the block, so the velocity modes carry the eight mass rows with their complex factor m_o d kappa_i / dc b_i
// (gn_mass_rows) where k_pseudo_hessian has the one real weight S_i.  Per column n' of Phi the lane loads its nine entries and forms t = E Phi[:, n']; per row j'
// that has a coefficient in that column it adds Re conj(E[j', n']) sum_j Gamma[j, j'] t[j], the nine entries of Gamma loaded where they are used.  Both loops are
// real loops over wave-uniform indices: with the 45 entries of the Hermitian Gamma held in registers beside the 33 coefficients, or with the loops unrolled (the
// compiler then hoists every load of the planes to the top), the full modes spilt 164 to 842 registers to scratch.  About 600 complex multiply-adds and 380
// cached 16-byte loads per cell, every sum in the order of the code.  One writer per cell, no atomics, no LDS, no scratch.
enum { GN_VELOCITY = 0, GN_BUOYANCY = 1, GN_GARDNER = 2, GN_MASS = 3, GN_DIAGONAL = 4 };
constexpr int GN_NCOEF = 33;        // the packed order of ph_each: c[0..8], e[0..3][0..1], k[0..3][0..3]

// the slot of the block a coefficient's row and column are: row i has the nine lags; the edge row j = i - o sits at the slot of -o and holds {lag o -> i, centre};
// the corner row holds {lag o -> i, lag (0, sx) -> i - (sz, 0), lag (sz, 0) -> i - (0, sx), centre}
__host__ __device__ constexpr int gn_row(int q) {
    if (q < 9) return 4;
    if (q < 17) {
        const int a = (q - 9) / 2, sz = a < 2 ? 2 * a - 1 : 0, sx = a < 2 ? 0 : 2 * (a - 2) - 1;
        return 3 * (-sz + 1) + (-sx + 1);
    }
    const int a = (q - 17) / 4, sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
    return 3 * (-sz + 1) + (-sx + 1);
}
__host__ __device__ constexpr int gn_col(int q) {
    if (q < 9) return q;
    if (q < 17) return (q - 9) % 2 == 0 ? 4 : gn_row(q);
    const int a = (q - 17) / 4, t = (q - 17) % 4, sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
    return t == 0 ? 4 : (t == 1 ? 3 * (-sz + 1) + 1 : (t == 2 ? 3 + (-sx + 1) : gn_row(q)));
}
// the coefficients a mode can have: the velocity star at a fixed density has its own row and one mass weight per neighbouring row; the mass term alone one per row
__host__ __device__ constexpr bool gn_live(int mode, int q) {
    if (mode == GN_VELOCITY) return q < 9 || gn_col(q) == 4;
    if (mode == GN_MASS) return gn_col(q) == 4;
    return true;
}

// entry (p, q) of a cell's block from the planes of k_lag_gram, sum over the columns of u[i + o_p] conj(u[i + o_q]); zero where either cell is outside the grid
// (no coefficient is non-zero there: an interior row has every neighbour inside)
__device__ __forceinline__ cplx gn_gram(const cplx *__restrict__ C, long long N, int nz, int nx, int iz, int ix, int p, int q) {
    const int az = iz + p / 3 - 1, ax = ix + p % 3 - 1, bz = iz + q / 3 - 1, bx = ix + q % 3 - 1;
    if (az < 0 || az >= nz || ax < 0 || ax >= nx || bz < 0 || bz >= nz || bx < 0 || bx >= nx) return cmake(0.0, 0.0);
    const int dz = bz - az, dx = bx - ax;
    if (dz > 0 || (dz == 0 && dx >= 0)) return C[(long long)lg_plane(dz, dx) * N + (long long)az * nx + ax];
    return cconj(C[(long long)lg_plane(-dz, -dx) * N + (long long)bz * nx + bx]);
}

// the mass weight m_o w of cell i in the interior rows j = i - o around it (conjugated, as ph_coefficients leaves its own): entries 9 + 2 a and 17 + 4 a
__device__ __forceinline__ void gn_mass_rows(const MzParams &P, int iz, int ix, cplx w, cplx (&e)[GN_NCOEF]) {
    auto put = [&](int sz, int sx, double m, cplx &out) {
        const int jz = iz - sz, jx = ix - sx;
        if (jz >= 1 && jz <= P.nz - 2 && jx >= 1 && jx <= P.nx - 2) out = cconj(cscale(w, m));
    };
    put(-1, 0, MZ_WD, e[9]); put(1, 0, MZ_WD, e[11]); put(0, -1, MZ_WD, e[13]); put(0, 1, MZ_WD, e[15]);
    put(-1, -1, MZ_WE, e[17]); put(-1, 1, MZ_WE, e[21]); put(1, -1, MZ_WE, e[25]); put(1, 1, MZ_WE, e[29]);
}

// fn(std::integral_constant<int, 0>) .. fn(std::integral_constant<int, N - 1>) in order: a loop whose index is a constant expression in its body
template <class FN, int... I>
__device__ __forceinline__ void gn_for_each(FN &&fn, std::integer_sequence<int, I...>) { (fn(std::integral_constant<int, I>{}), ...); }
template <int N, class FN>
__device__ __forceinline__ void gn_for(FN &&fn) { gn_for_each(fn, std::make_integer_sequence<int, N>{}); }

template <int MODE>
__device__ __forceinline__ void gn_coefficients(const MzParams &P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ chain,
                                                int iz, int ix, cplx (&e)[GN_NCOEF]) {
#pragma unroll
    for (int q = 0; q < GN_NCOEF; ++q) e[q] = cmake(0.0, 0.0);
    const long long i = (long long)iz * P.nx + ix;
    if (MODE == GN_BUOYANCY || MODE == GN_GARDNER) {
        PhCoef E;
        ph_coefficients<MODE == GN_BUOYANCY ? PH_BUOYANCY : PH_GARDNER>(P, c, rho, chain, iz, ix, E);
        ph_each<PH_BUOYANCY>(E, [&](int q, cplx &v) { e[q] = v; });
        return;
    }
    const cplx w = cscale(mz_kappa_dc(P, c[i]), 1.0 / rho[i]);          // d K_i / d c_i at the density of the handle
    if (MODE == GN_VELOCITY) {
        PhCoef E;
        ph_coefficients<PH_VELOCITY>(P, c, rho, chain, iz, ix, E);
#pragma unroll
        for (int k = 0; k < 9; ++k) e[k] = E.c[k];
    } else if (iz >= 1 && iz <= P.nz - 2 && ix >= 1 && ix <= P.nx - 2) {
        e[4] = cconj(cscale(w, MZ_WC));
    }
    gn_mass_rows(P, iz, ix, w, e);
}

template <int MODE>
__global__ __launch_bounds__(64) void k_gauss_newton_diagonal(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ chain,
                                                              const cplx *__restrict__ Cu, const cplx *__restrict__ Cg, double alpha, const double *__restrict__ W,
                                                              double *__restrict__ H) {
    const int nz = P.nz, nx = P.nx;
    const long long N = (long long)nz * nx, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double wgt = W ? alpha * W[i] : alpha;
    if (MODE == GN_DIAGONAL) {                                  // the diagonal weight of 'scaler': the zero-lag planes alone, |w_i|^2 in W
        H[i] = H[i] + wgt * (Cg[i].x * Cu[i].x);
        return;
    }
    const int iz = (int)(i / nx), ix = (int)(i % nx);
    cplx e[GN_NCOEF];
    gn_coefficients<MODE>(P, c, rho, chain, iz, ix, e);
    double h = 0.0;
#pragma unroll 1
    for (int n2 = 0; n2 < 9; ++n2) {                            // (a real loop: unrolled, the compiler hoists every load of the planes to the top and spills)
        cplx phi[9], t[9];                                      // (compile-time indices inside: e, phi and t stay in registers)
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            phi[n] = gn_gram(Cu, N, nz, nx, iz, ix, n, n2);
            t[n] = cmake(0.0, 0.0);
        }
        gn_for<GN_NCOEF>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if constexpr (gn_live(MODE, q)) cfma(t[gn_row(q)], e[q], phi[gn_col(q)]);
        });
#pragma unroll 1
        for (int j2 = 0; j2 < 9; ++j2) {                        // (a real loop too: the entries of Gamma are loaded where they are used)
            cplx ec = cmake(0.0, 0.0);
            bool any = false;
            gn_for<GN_NCOEF>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                if (gn_live(MODE, q) && gn_row(q) == j2 && gn_col(q) == n2) { ec = e[q]; any = true; }      // (uniform over the wave; at most one q)
            });
            if (!any) continue;
            cplx s = cmake(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 9; ++j) cfma(s, gn_gram(Cg, N, nz, nx, iz, ix, j, j2), t[j]);
            h = fma(ec.x, s.x, h);
            h = fma(ec.y, s.y, h);                              // Re conj(e) s
        }
    }
    H[i] = H[i] + wgt * h;
}

// H[i] += alpha (W ? W[i] : 1) Re tr(E_i^H Gamma_i E_i Phi_i) for i < N: Phi from dCu and Gamma from dCg, two sets of 13 planes of helm_lag_gram_accumulate_device
// (of the stored forward fields and of the receiver columns solved with the transposed operator, as they are).  E_i the derivative of the operator the handle holds
// with respect to the velocity of cell i (mode 0, at the handle's density), to its buoyancy (mode 1), to its velocity with the buoyancy following it by dChain
// (mode 2: dChain N float64, NULL otherwise), its mass term alone (mode 3: linearisation='operator'), or the unit diagonal (mode 4: 'scaler', the weight |w_i|^2
// in dW; H[i] += alpha W[i] Gamma_i[i, i] Phi_i[i, i]).  dW, dH: N float64; alpha >= 0.  Returns when H is complete.
extern "C" int helm_gauss_newton_diagonal_device(helm_op *op, int mode, const void *dChain, const void *dW, const void *dCu, const void *dCg, double alpha, void *dH) {
    helm_tuning_refresh();
    if (!op || !dCu || !dCg || !dH || !(alpha >= 0.0) || mode < GN_VELOCITY || mode > GN_DIAGONAL || (mode == GN_GARDNER) != (dChain != nullptr)) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_gauss_newton_diagonal_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dChain) | ((uintptr_t)dW) | ((uintptr_t)dH)) & 7) || ((((uintptr_t)dCu) | ((uintptr_t)dCg)) & 15)) return HELM_ERR_ARG;
    const size_t hbytes = (size_t)op->N * 8, cbytes = (size_t)op->N * LG_NLAG * sizeof(cplx);
    if (ranges_overlap(dCu, cbytes, dH, hbytes) || ranges_overlap(dCg, cbytes, dH, hbytes) || (dW && ranges_overlap(dW, hbytes, dH, hbytes)) ||
        (dChain && ranges_overlap(dChain, hbytes, dH, hbytes)))
        return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_gauss_newton_diagonal_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 63) / 64)), block(64);
    const cplx *c = (const cplx *)op->d_c, *Cu = (const cplx *)dCu, *Cg = (const cplx *)dCg;
    const double *rho = (const double *)op->d_rho, *chain = (const double *)dChain, *W = (const double *)dW;
    double *H = (double *)dH;
#define GN_GO(MODE) HELM_LAUNCH(k_gauss_newton_diagonal<MODE>, grid, block, 0, op->stream, P, c, rho, chain, Cu, Cg, alpha, W, H)
    if (mode == GN_VELOCITY) GN_GO(GN_VELOCITY);
    else if (mode == GN_BUOYANCY) GN_GO(GN_BUOYANCY);
    else if (mode == GN_GARDNER) GN_GO(GN_GARDNER);
    else if (mode == GN_MASS) GN_GO(GN_MASS);
    else GN_GO(GN_DIAGONAL);
#undef GN_GO
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the per-cell 2 x 2 blocks of the joint (c, rho) Hessian: rows H_cc, H_crho, H_rhorho of H, ldH apart
// ------------------------------------------------------------------------------------------
// The pair (E^c_i, E^b_i) of a cell -- the velocity star at the density of the handle (STRETCH) or its mass term alone, and the buoyancy star -- has a 2 x 2 Gram
// matrix under either inner product of the sections above: (cc, cb, bb).  In density units, d b / d rho = -1 / rho^2:
//     H[0][i] += alpha cc,     H[1][i] += -alpha cb / rho_i^2,     H[2][i] += alpha bb / rho_i^4.
// Rows 0 and 2 are what the diagonal kernels give for the two parameters; the cross term is what is new, and it has either sign.

// what the three sums of a cell end in: one writer per cell
__device__ __forceinline__ void blocks_store(double *__restrict__ H, long long ldH, long long i, double alpha, double rho, double cc, double cb, double bb) {
    const double r2 = rho * rho;
    H[i] = H[i] + alpha * cc;
    H[ldH + i] = H[ldH + i] + (-alpha / r2) * cb;
    H[2 * ldH + i] = H[2 * ldH + i] + (alpha / (r2 * r2)) * bb;
}

// k_gauss_newton_blocks: the walk of k_gauss_newton_diagonal with both coefficient sets of the lane in registers -- 17 (STRETCH: the nine of its own row and the
// eight mass rows) or 9 (the mass term alone) live velocity coefficients beside the 33 of the buoyancy.  Per column n' of Phi the nine entries are loaded once and
// both t^c = E^c Phi[:, n'] and t^b = E^b Phi[:, n'] formed; per row j' the nine entries of Gamma are loaded once for s^c = Gamma^T t^c and s^b = Gamma^T t^b, and
// Re conj(e^c) s^c, Re conj(e^c) s^b, Re conj(e^b) s^b go to the three sums.  Both loops stay real loops, as there.  One writer per cell, every sum in the order of
// the code, no atomics, no LDS, no scratch.
template <bool STRETCH>
__global__ __launch_bounds__(64) void k_gauss_newton_blocks(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const cplx *__restrict__ Cu,
                                                            const cplx *__restrict__ Cg, double alpha, double *__restrict__ H, long long ldH) {
    constexpr int CM = STRETCH ? GN_VELOCITY : GN_MASS;
    const int nz = P.nz, nx = P.nx;
    const long long N = (long long)nz * nx, i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / nx), ix = (int)(i % nx);
    cplx ec[GN_NCOEF], eb[GN_NCOEF];
    gn_coefficients<CM>(P, c, rho, nullptr, iz, ix, ec);
    gn_coefficients<GN_BUOYANCY>(P, c, rho, nullptr, iz, ix, eb);
    double cc = 0.0, cb = 0.0, bb = 0.0;
#pragma unroll 1
    for (int n2 = 0; n2 < 9; ++n2) {
        cplx phi[9], tc[9], tb[9];
#pragma unroll
        for (int n = 0; n < 9; ++n) {
            phi[n] = gn_gram(Cu, N, nz, nx, iz, ix, n, n2);
            tc[n] = tb[n] = cmake(0.0, 0.0);
        }
        gn_for<GN_NCOEF>([&](auto qc) {
            constexpr int q = decltype(qc)::value;
            if constexpr (gn_live(CM, q)) cfma(tc[gn_row(q)], ec[q], phi[gn_col(q)]);
            cfma(tb[gn_row(q)], eb[q], phi[gn_col(q)]);
        });
#pragma unroll 1
        for (int j2 = 0; j2 < 9; ++j2) {
            cplx xc = cmake(0.0, 0.0), xb = cmake(0.0, 0.0);
            bool anyc = false, anyb = false;
            gn_for<GN_NCOEF>([&](auto qc) {
                constexpr int q = decltype(qc)::value;
                if (gn_row(q) == j2 && gn_col(q) == n2) {           // (uniform over the wave; at most one q)
                    xb = eb[q]; anyb = true;
                    if (gn_live(CM, q)) { xc = ec[q]; anyc = true; }
                }
            });
            if (!anyb) continue;                                    // (every live velocity entry is a buoyancy entry too)
            cplx sc = cmake(0.0, 0.0), sb = cmake(0.0, 0.0);
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                const cplx g = gn_gram(Cg, N, nz, nx, iz, ix, j, j2);
                cfma(sc, g, tc[j]);
                cfma(sb, g, tb[j]);
            }
            if (anyc) {
                cc = fma(xc.x, sc.x, cc); cc = fma(xc.y, sc.y, cc);      // Re conj(e^c) s^c
                cb = fma(xc.x, sb.x, cb); cb = fma(xc.y, sb.y, cb);      // Re conj(e^c) s^b
            }
            bb = fma(xb.x, sb.x, bb); bb = fma(xb.y, sb.y, bb);          // Re conj(e^b) s^b
        }
    }
    blocks_store(H, ldH, i, alpha, rho[i], cc, cb, bb);
}

// H[a][i] += alpha d_a(i) Re tr(E^a_i^H Gamma_i E^b_i Phi_i) for the three entries (c, c), (c, rho), (rho, rho) of the block of cell i < N, row a at dH + a ldH: Phi from
// dCu and Gamma from dCg as helm_gauss_newton_diagonal_device takes them; E^c the velocity star at the handle's density (stretch != 0) or its mass term alone,
// E^rho = -E^b / rho_i^2.  dH: float64, ldH >= N; alpha >= 0.  Returns when H is complete.
extern "C" int helm_gauss_newton_blocks_device(helm_op *op, int stretch, const void *dCu, const void *dCg, double alpha, void *dH, long long ldH) {
    helm_tuning_refresh();
    if (!op || !dCu || !dCg || !dH || !(alpha >= 0.0) || stretch < 0 || stretch > 1 || ldH < op->N) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_gauss_newton_blocks_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dH) & 7) || ((((uintptr_t)dCu) | ((uintptr_t)dCg)) & 15)) return HELM_ERR_ARG;
    const size_t hbytes = ((size_t)2 * ldH + op->N) * 8, cbytes = (size_t)op->N * LG_NLAG * sizeof(cplx);
    if (ranges_overlap(dCu, cbytes, dH, hbytes) || ranges_overlap(dCg, cbytes, dH, hbytes)) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_gauss_newton_blocks_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 63) / 64)), block(64);
    const cplx *c = (const cplx *)op->d_c, *Cu = (const cplx *)dCu, *Cg = (const cplx *)dCg;
    const double *rho = (const double *)op->d_rho;
    if (stretch) HELM_LAUNCH(k_gauss_newton_blocks<true>, grid, block, 0, op->stream, P, c, rho, Cu, Cg, alpha, (double *)dH, ldH);
    else HELM_LAUNCH(k_gauss_newton_blocks<false>, grid, block, 0, op->stream, P, c, rho, Cu, Cg, alpha, (double *)dH, ldH);
    return launched(op);
}

// k_pseudo_hessian_blocks: the walk of k_pseudo_hessian with three sums per lane.  Per column the lane forms the velocity row sum r^c_0 of its own row and the
// buoyancy row sums r^b_0 and r^b_j of the buoyancy mode.  The eight neighbouring velocity rows are conj(m_o w) v[4] (w = d kappa_i / dc b_i): their part of cc is
// the real weight S |v[4]|^2 of the velocity mode, their part of the cross term one weighted sum, Re[conj(conj(w) v[4]) sum_j m_o r^b_j] -- a row j outside the
// interior has no buoyancy coefficient, so r^b_j = 0 there and the weights are those of the lag alone.  !STRETCH: row i holds the centre mass weight alone.
template <class F, bool STRETCH>
__global__ __launch_bounds__(64 * PH_WAVES) void k_pseudo_hessian_blocks(F U, int nsrc, long long ld, MzParams P, const cplx *__restrict__ c,
                                                                         const double *__restrict__ rho, double alpha, double *__restrict__ H, long long ldH) {
    __shared__ double part[3][64];
    const int nz = P.nz, nx = P.nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z = (int)(blockIdx.x / ntx);
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    const long long i = (long long)z * nx + x;
    PhCoef Eb, Ec;
    cplx wc = cmake(0.0, 0.0);                                  // conj(w): the velocity coefficient of a neighbouring row without its mass weight
    if (store) {
        ph_coefficients<PH_BUOYANCY>(P, c, rho, nullptr, z, x, Eb);
        ph_coefficients<PH_VELOCITY>(P, c, rho, nullptr, z, x, Ec);
        wc = cconj(cscale(mz_kappa_dc(P, c[i]), 1.0 / rho[i]));
        if (!STRETCH) {
#pragma unroll
            for (int k = 0; k < 9; ++k) Ec.c[k] = cmake(0.0, 0.0);
            if (z >= 1 && z <= nz - 2 && x >= 1 && x <= nx - 2) Ec.c[4] = cscale(wc, MZ_WC);
        }
    } else {
        ph_each<PH_BUOYANCY>(Eb, [&](int, cplx &v) { v = cmake(0.0, 0.0); });       // (a halo lane adds nothing)
        ph_each<PH_VELOCITY>(Ec, [&](int, cplx &v) { v = cmake(0.0, 0.0); });
    }
    double acc_cc = 0.0, acc_cb = 0.0, acc_bb = 0.0;
    const int ngroups = (nsrc + PH_UNROLL - 1) / PH_UNROLL;
    for (int g = wave; g < ngroups; g += PH_WAVES) {          // (wave-uniform: the lane exchanges stay complete)
        const int s0 = g * PH_UNROLL, ncol = min(PH_UNROLL, nsrc - s0);
        typename F::raw raw[PH_UNROLL][3];
        double sc[PH_UNROLL];
#pragma unroll
        for (int j = 0; j < PH_UNROLL; ++j) {
            sc[j] = U.scale(s0 + min(j, ncol - 1));
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const int zz = z - 1 + r;
                raw[j][r] = (xin && j < ncol && zz >= 0 && zz < nz) ? U.load((long long)(s0 + j) * ld + (long long)zz * nx + x) : typename F::raw{};
            }
        }
#pragma unroll
        for (int j = 0; j < PH_UNROLL; ++j) {
            cplx v[9];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                v[3 * r + 1] = U.scaled(raw[j][r], sc[j]);
                lane_left_right(v[3 * r + 1], v[3 * r], v[3 * r + 2]);
            }
            cplx rc = cmake(0.0, 0.0), rb = cmake(0.0, 0.0);
            if (STRETCH) {
#pragma unroll
                for (int k = 0; k < 9; ++k) cfma(rc, Ec.c[k], v[k]);
            } else {
                rc = cmul(Ec.c[4], v[4]);
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) cfma(rb, Eb.c[k], v[k]);
            double scc = cabs2(rc) + Ec.S * cabs2(v[4]);
            double sbb = cabs2(rb);
            double scb = rc.x * rb.x + rc.y * rb.y;
            cplx medge = cmake(0.0, 0.0), mcorner = cmake(0.0, 0.0);
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int sz = a < 2 ? 2 * a - 1 : 0, sx = a < 2 ? 0 : 2 * (a - 2) - 1;
                cplx r1 = cmul(Eb.e[a][0], v[4]);
                cfma(r1, Eb.e[a][1], v[mz_slot(-sz, -sx)]);
                sbb += cabs2(r1);
                medge = cadd(medge, r1);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int sz = 2 * (a / 2) - 1, sx = 2 * (a % 2) - 1;
                cplx r2 = cmul(Eb.k[a][0], v[4]);
                cfma(r2, Eb.k[a][1], v[mz_slot(-sz, 0)]);
                cfma(r2, Eb.k[a][2], v[mz_slot(0, -sx)]);
                cfma(r2, Eb.k[a][3], v[mz_slot(-sz, -sx)]);
                sbb += cabs2(r2);
                mcorner = cadd(mcorner, r2);
            }
            const cplx msum = cadd(cscale(medge, MZ_WD), cscale(mcorner, MZ_WE));
            const cplx rn = cmul(wc, v[4]);
            scb += rn.x * msum.x + rn.y * msum.y;
            if (j < ncol) { acc_cc += scc; acc_cb += scb; acc_bb += sbb; }
        }
    }
    for (int w = 0; w < PH_WAVES; ++w) {
        if (wave == w) {
            part[0][lane] = w == 0 ? acc_cc : part[0][lane] + acc_cc;
            part[1][lane] = w == 0 ? acc_cb : part[1][lane] + acc_cb;
            part[2][lane] = w == 0 ? acc_bb : part[2][lane] + acc_bb;
        }
        __syncthreads();
    }
    if (wave == 0 && store) blocks_store(H, ldH, i, alpha, rho[i], part[0][lane], part[1][lane], part[2][lane]);
}

static int pseudo_hessian_blocks_launch(helm_op *op, HostField U, int nsrc, long long ld, int stretch, double alpha, void *dH, long long ldH) {
    helm_tuning_refresh();
    const char *what = U.c64 ? "helm_pseudo_hessian_blocks_c64_device" : "helm_pseudo_hessian_blocks_device";
    if (!op || !U.ok() || !dH || nsrc < 1 || ld < op->N || ldH < op->N || !(alpha >= 0.0) || stretch < 0 || stretch > 1) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, what)) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dH) & 7)) return HELM_ERR_ARG;
    if (ranges_overlap(U.u, U.bytes(nsrc, ld), dH, ((size_t)2 * ldH + op->N) * 8)) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle holds no assembled operator", what);
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * op->nz)), block(64 * PH_WAVES);
    const cplx *c = (const cplx *)op->d_c;
    const double *rho = (const double *)op->d_rho;
    return U.with([&](auto F) {
        if (stretch) HELM_LAUNCH((k_pseudo_hessian_blocks<decltype(F), true>), grid, block, 0, op->stream, F, nsrc, ld, P, c, rho, alpha, (double *)dH, ldH);
        else HELM_LAUNCH((k_pseudo_hessian_blocks<decltype(F), false>), grid, block, 0, op->stream, F, nsrc, ld, P, c, rho, alpha, (double *)dH, ldH);
        return launched(op);
    });
}

// H[a][i] += alpha d_a(i) sum_{s<nsrc} Re <E^a_i u^_s, E^b_i u^_s> for the three entries (c, c), (c, rho), (rho, rho) of the block of cell i < N, row a at dH + a ldH:
// U the stored (conjugated) fields as helm_pseudo_hessian_accumulate_device takes them, E^c and E^rho as helm_gauss_newton_blocks_device.  Returns when H is complete.
extern "C" int helm_pseudo_hessian_blocks_device(helm_op *op, const void *dU, int nsrc, long long ld, int stretch, double alpha, void *dH, long long ldH) {
    return pseudo_hessian_blocks_launch(op, HostField::c128(dU), nsrc, ld, stretch, alpha, dH, ldH);
}
extern "C" int helm_pseudo_hessian_blocks_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int stretch, double alpha, void *dH,
                                                     long long ldH) {
    return pseudo_hessian_blocks_launch(op, HostField::packed(dU32, dExp), nsrc, ld, stretch, alpha, dH, ldH);
}
