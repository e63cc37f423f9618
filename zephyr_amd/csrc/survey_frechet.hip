// The derivative kernels of the 2-D MiniZephyr operator on stored columns, each beside the C entry point that launches it: the mass stencil of the exact Frechet
// derivative fused into the virtual sources and into the imaging sum; the exact density derivative (the buoyancy map, its stencil on stored columns, the nine lag
// products and its transpose); the planes of the total velocity derivative and their transpose.  The walk they share, the readers of a stored field and the row
// factors at a cell are in survey_internal.hpp; the Hessian diagonals built on these derivatives are in survey_hessian.hip.
#include "survey_internal.hpp"

// ------------------------------------------------------------------------------------------
// the exact Frechet derivative of MiniZephyr: the mass stencil fused into the virtual sources and into the imaging sum
// ------------------------------------------------------------------------------------------
// MiniZephyr carries the velocity as K = (omega_d^2 / c^2 - ky^2) / rho of the NEIGHBOURING cell, spread over the nine slots of a row by the mass weights
// (assemble.hip: centre cc, edges dc, corners ec), and its four boundary lines are +-identity rows.  So (dA) u = mask_int (.) M0(dK (.) u): M0 the constant
// 9-point stencil of those weights (cells outside the grid contribute nothing), mask_int zero on the boundary lines.  HelmBaseProblem.JvecBorn /
// Jtvec(linearisation='operator') need M0 applied to k columns on the way to the solver (k_virtual_sources_op) and, transposed -- M0^T mask_int = M0 mask_int,
// the weights are symmetric -- to the back-propagated columns inside the imaging sum (k_imaging_op).
//
// Both kernels walk the grid the same way.  A wave takes a tile of OP_TILE_X output cells along x, one lane per cell, plus one halo lane at either end (lanes 0 and
// 63 load and never store), and OP_ROWS output rows, which it walks down with a rolling window of three rows per column held in registers: per row and column
// the value t of the lane's own cell and h = t(x - 1) + t(x + 1), fetched from the neighbouring lanes (no LDS, no barrier: waves run independently).  Row z is
//     mc t(z) + md ((t(z-1) + t(z+1)) + h(z)) + me (h(z-1) + h(z+1))
// OP_UNROLL columns are walked together, and the loads of the next row are issued before the arithmetic of the current one.  A field element is loaded once per
// kernel except for the halo: one lane in 32 and two rows in OP_ROWS + 2 are loaded by two waves (neighbours in the grid, hence in flight together).
// The order of every sum is fixed by the code: the same bits on every run.
constexpr double MZ_MC = 0.6248, MZ_MD = 0.09381, MZ_ME = 0.000001297;      // (assemble.hip cc, dc, ec)
__device__ __forceinline__ cplx mass_row(const MassRow &up, const MassRow &mid, const MassRow &dn) {
    const cplx e = cmake((up.t.x + dn.t.x) + mid.h.x, (up.t.y + dn.t.y) + mid.h.y);
    const cplx c = cmake(up.h.x + dn.h.x, up.h.y + dn.h.y);
    return cmake(MZ_MC * mid.t.x + MZ_MD * e.x + MZ_ME * c.x, MZ_MC * mid.t.y + MZ_MD * e.y + MZ_ME * c.y);
}

// R[s ldr + i] = coef mask_int[i] M0(W (.) (CONJ ? conj(U[s]) : U[s]))[i] for the nsrc columns, i over the nz x nx grid.  grid.y: groups of OP_UNROLL columns.
// Per cell and column 16 (8: complex64 store) bytes read and 16 written; W is read once per group of columns (16 B per cell against 4 x 32).
template <class F, bool CONJ>
__global__ __launch_bounds__(256) void k_virtual_sources_op(F U, int nsrc, long long ldu, const cplx *__restrict__ W, cplx coef, cplx *__restrict__ R, long long ldr,
                                                            int nz, int nx) {
    const OpJob job(nz, nx);
    if (!job.live) return;                                  // (a whole wave: the lane exchanges below stay complete)
    const int s0 = blockIdx.y * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
    const int x = job.x;
    typename F::raw raw[OP_UNROLL];
    cplx w;
    MassRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    double sc[OP_UNROLL];                                   // (the columns' scales, read once: not a dependent load per row)
#pragma unroll
    for (int j = 0; j < OP_UNROLL; ++j) sc[j] = U.scale(s0 + min(j, ncol - 1));

    // the loads of row z (nothing outside the grid); the products and the neighbour exchange of what was loaded
    auto fetch = [&](int z) {
        const bool in = job.xin && z >= 0 && z < nz;
        const long long i = (long long)z * nx + x;
        w = in ? W[i] : cmake(0.0, 0.0);
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) raw[j] = (in && j < ncol) ? U.load((long long)(s0 + j) * ldu + i) : typename F::raw{};
    };
    auto make = [&](MassRow *row) {
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) {
            cplx u = U.scaled(raw[j], sc[j]);
            if (CONJ) u = cconj(u);
            row[j].t = cmul(w, u);
            row[j].h = lane_neighbours(row[j].t);
        }
    };
    fetch(job.z0 - 1); make(up);
    fetch(job.z0); make(mid);
    fetch(job.z0 + 1);
    for (int z = job.z0; z < job.z1; ++z) {
        make(dn);
        if (z + 1 < job.z1) fetch(z + 2);                  // (wave-uniform)
        const bool inside = z >= 1 && z <= nz - 2 && x >= 1 && x <= nx - 2;
        if (job.store) {
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j)
                if (j < ncol) R[(long long)(s0 + j) * ldr + i] = inside ? cmul(coef, mass_row(up[j], mid[j], dn[j])) : cmake(0.0, 0.0);
        }
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
    }
}

// R[s][i] = coef mask_int[i] M0(W (.) U[s])[i] (conj != 0: M0(W (.) conj(U[s]))) for s < nsrc, i < N (the handle's nz x nx grid): U [nsrc][ldu] complex128, W N
// complex128, R [nsrc][ldr] complex128, ldu, ldr >= N.  R must not overlap U or W.  Returns when R is complete.
static int virtual_sources_op_launch(helm_op *op, HostField U, int nsrc, long long ldu, const void *dW, cplx coef, int conj, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !U.u || !dW || !dR || nsrc < 1 || nsrc > 65535 * OP_UNROLL || ldu < op->N || ldr < op->N || U.u == dR || dW == dR) return HELM_ERR_ARG;
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the mass stencil of the exact derivative is that of the 2-D MiniZephyr operator");
    if (!U.ok() || ((((uintptr_t)dW) | ((uintptr_t)dR)) & 15)) return HELM_ERR_ARG;       // (the exponents and every alignment come after the handle; 16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    return U.with([&](auto F) {
        if (conj) HELM_LAUNCH((k_virtual_sources_op<decltype(F), true>), grid, dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dW, coef, (cplx *)dR, ldr, op->nz, op->nx);
        else HELM_LAUNCH((k_virtual_sources_op<decltype(F), false>), grid, dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dW, coef, (cplx *)dR, ldr, op->nz, op->nx);
        return launched(op);
    });
}
extern "C" int helm_virtual_sources_op_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im, int conj,
                                              void *dR, long long ldr) {
    return virtual_sources_op_launch(op, HostField::c128(dU), nsrc, ldu, dW, cmake(coef_re, coef_im), conj, dR, ldr);
}
extern "C" int helm_virtual_sources_op_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im,
                                                  int conj, void *dR, long long ldr) {
    return virtual_sources_op_launch(op, HostField::packed(dU32, dExp), nsrc, ldu, dW, cmake(coef_re, coef_im), conj, dR, ldr);
}

// G[i] += W[i] sum_s UF[s ldf + i] M0(mask_int (.) UB[s])[i]: the stencil on the back-propagated field inside the imaging sum, no intermediate array.  A workgroup
// of IMG_WAVES waves owns a tile of OP_TILE_X x IMG_ROWS cells of G.  The columns go to its waves in groups of OP_UNROLL, group g to wave g mod IMG_WAVES; a wave walks
// the tile's rows once per group (the walk of the header comment) and keeps its sum per cell in an LDS slice of its own.  After one barrier wave r adds the slices
// of row r in wave order and then W (.) sum to G: one writer per cell and a fixed order, so no atomics and the same bits on every run.
// Per cell and column 16 (8: complex64 store) bytes of UF and 16 of UB, the latter times (1 + 2 / IMG_ROWS) (1 + 2 / OP_TILE_X) for the halo; W and G once per cell.
// Rows are short because the columns of a tile are spread over the waves of ONE workgroup: with a wave per 32 rows and every column, 512^2 cells gave 144 waves
// to 1024 SIMDs and the kernel ran at 0.7 TB/s.
constexpr int IMG_ROWS = 8;         // output rows per workgroup
constexpr int IMG_WAVES = 8;        // waves per workgroup: 64 KB of LDS
static_assert(IMG_ROWS <= IMG_WAVES, "wave r finishes row r");

template <class F>
__global__ __launch_bounds__(64 * IMG_WAVES) void k_imaging_op(F UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc, const cplx *__restrict__ W,
                                                               cplx *__restrict__ G, int nz, int nx) {
    __shared__ cplx part[IMG_WAVES][IMG_ROWS][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z0 = (int)(blockIdx.x / ntx) * IMG_ROWS;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    cplx rawb[OP_UNROLL];
    MassRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    const int ngroups = (nsrc + OP_UNROLL - 1) / OP_UNROLL;
    for (int g = wave; g < ngroups; g += IMG_WAVES) {          // (wave-uniform: the lane exchanges stay complete)
        const int s0 = g * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
        double sc[OP_UNROLL];                               // (the columns' scales, read once per group: not a dependent load per row)
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) sc[j] = UF.scale(s0 + min(j, ncol - 1));
        // the loads of row z of UB with mask_int applied: nothing outside the grid, nothing from its boundary lines
        auto fetch = [&](int z) {
            const bool in = z >= 1 && z <= nz - 2 && x >= 1 && x <= nx - 2;
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j) rawb[j] = (in && j < ncol) ? UB[(long long)(s0 + j) * ldb + i] : cmake(0.0, 0.0);
        };
        auto make = [&](MassRow *row) {
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j) { row[j].t = rawb[j]; row[j].h = lane_neighbours(rawb[j]); }
        };
        fetch(z0 - 1); make(up);
        fetch(z0); make(mid);
        fetch(z0 + 1);
#pragma unroll 1
        for (int r = 0; r < IMG_ROWS; ++r) {
            const int z = z0 + r;
            make(dn);
            if (r + 1 < IMG_ROWS) fetch(z + 2);
            cplx acc = cmake(0.0, 0.0);
            if (store && z < nz) {
                const long long i = (long long)z * nx + x;
                typename F::raw rawf[OP_UNROLL];
#pragma unroll
                for (int j = 0; j < OP_UNROLL; ++j) rawf[j] = j < ncol ? UF.load((long long)(s0 + j) * ldf + i) : typename F::raw{};
#pragma unroll
                for (int j = 0; j < OP_UNROLL; ++j)
                    if (j < ncol) cfma(acc, UF.scaled(rawf[j], sc[j]), mass_row(up[j], mid[j], dn[j]));
            }
            part[wave][r][lane] = g == wave ? acc : cadd(part[wave][r][lane], acc);      // (the wave's own slice: no other wave touches it before the barrier)
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
        }
    }
    __syncthreads();
    if (wave < IMG_ROWS && store && z0 + wave < nz) {
        cplx sum = part[0][wave][lane];                          // (nsrc >= 1: wave 0 has a group)
        for (int w = 1; w < min(IMG_WAVES, ngroups); ++w) sum = cadd(sum, part[w][wave][lane]);
        const long long i = (long long)(z0 + wave) * nx + x;
        cplx gv = G[i];
        cfma(gv, W[i], sum);
        G[i] = gv;
    }
}
static dim3 imaging_op_grid(const helm_op *op) {
    return dim3((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * ((op->nz + IMG_ROWS - 1) / IMG_ROWS)));
}

// G[i] += W[i] sum_s UF[s][i] M0(mask_int (.) UB[s])[i] for i < N: UF [nsrc][ldf], UB [nsrc][ldb], W and G N complex128.  G must not overlap the others.  Returns when G
// is complete.
static int imaging_op_launch(helm_op *op, HostField UF, long long ldf, const void *dUB, long long ldb, int nsrc, const void *dW, void *dG) {
    helm_tuning_refresh();
    if (!op || !UF.u || !dUB || !dW || !dG || nsrc < 1 || ldf < op->N || ldb < op->N || UF.u == dG || dUB == dG || dW == dG) return HELM_ERR_ARG;
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the mass stencil of the exact derivative is that of the 2-D MiniZephyr operator");
    if (!UF.ok() || ((((uintptr_t)dUB) | ((uintptr_t)dW) | ((uintptr_t)dG)) & 15)) return HELM_ERR_ARG;       // (the exponents and every alignment come after the handle)
    HIP_TRY(op, hipSetDevice(op->device));
    return UF.with([&](auto F) {
        HELM_LAUNCH(k_imaging_op<decltype(F)>, imaging_op_grid(op), dim3(64 * IMG_WAVES), 0, op->stream, F, ldf, (const cplx *)dUB, ldb, nsrc, (const cplx *)dW, (cplx *)dG,
                    op->nz, op->nx);
        return launched(op);
    });
}
extern "C" int helm_imaging_op_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, const void *dW, void *dG) {
    return imaging_op_launch(op, HostField::c128(dUF), ldf, dUB, ldb, nsrc, dW, dG);
}
extern "C" int helm_imaging_op_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc,
                                                     const void *dW, void *dG) {
    return imaging_op_launch(op, HostField::packed(dUF32, dExp), ldf, dUB, ldb, nsrc, dW, dG);
}

// ------------------------------------------------------------------------------------------
// the exact density derivative of MiniZephyr: the buoyancy map L, its stencil on stored columns, the nine lag products and L^T
// ------------------------------------------------------------------------------------------
// Every interior row of MiniZephyr is a linear, homogeneous function of the buoyancy field b = 1 / rho (mz_row.hpp mz_star: the mass terms carry
// kappa b of the neighbouring cell, kappa = omega_d^2 / c^2 - ky^2; every stiffness term is a row factor -- X, Z, px, pz of the row's own cell, which depend
// on c and the PML only -- times an average (b_i + b_(i+o)) / 2), and the four boundary lines are +-identity.  So the derivative of A along a perturbation
// db of the buoyancy is the nine planes dC = L[db], the assembly's own formulas evaluated on db with the boundary rows zero, and
//     (dA) u = sum_k dC_k (.) shift_k(u)                                  (k_buoyancy_planes, then k_stencil_sources on the stored columns)
//     sum_s z_s^T (dA) u_s = sum_k sum_i dC_k[i] P_k[i],   P_k[i] = sum_s z_s[i] u_s[i + off_k]     (k_lag_imaging: nine model-sized planes)
//     g_b = L^T P                                                         (k_buoyancy_adjoint: a gather over the 3 x 3 rows around a cell)
// HelmBaseProblem.JvecBorn / Jtvec(linearisation='operator', parameter='rho') put these together (device_survey.py); db = -v / rho^2 and g_rho = -g_b / rho^2
// are the caller's.  Planes are [9][N] with the slot order of the operator, k = 3 (dz + 1) + (dx + 1).

// dC = L[db]: one lane per cell, the assembly's star (mz_star) on the perturbation.  An interior row reads only cells inside the grid, so there is no padding.
__global__ __launch_bounds__(256) void k_buoyancy_planes(MzParams P, const cplx *__restrict__ c, const double *__restrict__ db, cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    cplx out[9];
    if (iz == 0 || iz == P.nz - 1 || ix == 0 || ix == P.nx - 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = cmake(0.0, 0.0);
    } else {
        const MzRow row = mz_row_at(P, c, iz, ix);
        double bn[9];
        cplx Kn[9];
        const double b0 = db[i];
#pragma unroll
        for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
            for (int sx = -1; sx <= 1; ++sx) {
                const long long j = i + (long long)sz * P.nx + sx;
                const double bj = db[j];
                const cplx k = mz_kappa(P, c[j]);
                bn[mz_slot(sz, sx)] = (b0 + bj) / 2.0;
                Kn[mz_slot(sz, sx)] = cmake(k.x * bj, k.y * bj);
            }
        mz_star(P, row, bn, Kn, out);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[(long long)k * N + i] = out[k];
}

// dC[9][N] = L[db] for the operator the handle holds (its c, PML and the frequency of its last assembly): db N float64, dC 9 N complex128, boundary rows zero.
// Returns when dC is complete.
extern "C" int helm_buoyancy_planes_device(helm_op *op, const void *dDb, void *dC) {
    helm_tuning_refresh();
    if (!op || !dDb || !dC) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_buoyancy_planes_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || (((uintptr_t)dDb) & 7) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dDb, (size_t)op->N * 8, dC, (size_t)op->N * 9 * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_buoyancy_planes_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_buoyancy_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)dDb, (cplx *)dC);
    return launched(op);
}

// R[s ldr + i] = coef sum_k C_k[i] (CONJ ? conj(U[s]) : U[s])[i + off_k] for the nsrc columns, cells outside the grid contributing nothing: the walk of
// k_virtual_sources_op (a tile of OP_TILE_X cells and OP_ROWS rows per wave, OP_UNROLL columns together, a rolling window of three rows in registers), with
// the left and right neighbours kept apart because their coefficients differ.  The nine planes are read once per group of columns: per cell and column 16 (8)
// bytes read and 16 written, plus 144 / OP_UNROLL.  The sum runs k = 0 .. 8: the same bits on every run.
template <class F, bool CONJ>
__global__ __launch_bounds__(256) void k_stencil_sources(F U, int nsrc, long long ldu, const cplx *__restrict__ C, cplx coef, cplx *__restrict__ R, long long ldr,
                                                         int nz, int nx) {
    const OpJob job(nz, nx);
    if (!job.live) return;                                  // (a whole wave: the lane exchanges below stay complete)
    const long long N = (long long)nz * nx;
    const int s0 = blockIdx.y * OP_UNROLL, ncol = min(OP_UNROLL, nsrc - s0);
    const int x = job.x;
    typename F::raw raw[OP_UNROLL];
    LagRow up[OP_UNROLL], mid[OP_UNROLL], dn[OP_UNROLL];
    double sc[OP_UNROLL];
#pragma unroll
    for (int j = 0; j < OP_UNROLL; ++j) sc[j] = U.scale(s0 + min(j, ncol - 1));
    auto fetch = [&](int z) {
        const bool in = job.xin && z >= 0 && z < nz;
        const long long i = (long long)z * nx + x;
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) raw[j] = (in && j < ncol) ? U.load((long long)(s0 + j) * ldu + i) : typename F::raw{};
    };
    auto make = [&](LagRow *row) {
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) {
            cplx u = U.scaled(raw[j], sc[j]);
            if (CONJ) u = cconj(u);
            row[j].t = u;
            lane_left_right(u, row[j].l, row[j].r);
        }
    };
    fetch(job.z0 - 1); make(up);
    fetch(job.z0); make(mid);
    fetch(job.z0 + 1);
    for (int z = job.z0; z < job.z1; ++z) {
        make(dn);
        if (z + 1 < job.z1) fetch(z + 2);                  // (wave-uniform)
        if (job.store) {
            const long long i = (long long)z * nx + x;
            cplx ck[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) ck[k] = C[(long long)k * N + i];
#pragma unroll
            for (int j = 0; j < OP_UNROLL; ++j)
                if (j < ncol) {
                    cplx acc = cmake(0.0, 0.0);
                    cfma(acc, ck[0], up[j].l); cfma(acc, ck[1], up[j].t); cfma(acc, ck[2], up[j].r);
                    cfma(acc, ck[3], mid[j].l); cfma(acc, ck[4], mid[j].t); cfma(acc, ck[5], mid[j].r);
                    cfma(acc, ck[6], dn[j].l); cfma(acc, ck[7], dn[j].t); cfma(acc, ck[8], dn[j].r);
                    R[(long long)(s0 + j) * ldr + i] = cmul(coef, acc);
                }
        }
#pragma unroll
        for (int j = 0; j < OP_UNROLL; ++j) { up[j] = mid[j]; mid[j] = dn[j]; }
    }
}

// R[s][i] = coef sum_k C_k[i] U[s][i + off_k] (conj != 0: conj(U[s])) for s < nsrc, i < N (the handle's nz x nx grid): U [nsrc][ldu] complex128, C [9][N]
// complex128 (helm_buoyancy_planes_device), R [nsrc][ldr] complex128, ldu, ldr >= N.  R must not overlap U or C.  Returns when R is complete.
static int stencil_sources_launch(helm_op *op, HostField U, int nsrc, long long ldu, const void *dC, cplx coef, int conj, void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !U.u || !dC || !dR || nsrc < 1 || nsrc > 65535 * OP_UNROLL || ldu < op->N || ldr < op->N) return HELM_ERR_ARG;
    if (int rc = planes_handle_args(op, "helm_stencil_sources_device")) return rc;       // (both entry points refuse under this name)
    const size_t rbytes = (size_t)nsrc * ldr * sizeof(cplx);
    if (ranges_overlap(U.u, U.bytes(nsrc, ldu), dR, rbytes) || ranges_overlap(dC, (size_t)op->N * 9 * sizeof(cplx), dR, rbytes)) return HELM_ERR_ARG;
    if (!U.ok() || ((((uintptr_t)dC) | ((uintptr_t)dR)) & 15)) return HELM_ERR_ARG;       // (the exponents and every alignment come after the handle; 16-byte loads and stores)
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid = op_grid(op, (nsrc + OP_UNROLL - 1) / OP_UNROLL);
    return U.with([&](auto F) {
        if (conj) HELM_LAUNCH((k_stencil_sources<decltype(F), true>), grid, dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dC, coef, (cplx *)dR, ldr, op->nz, op->nx);
        else HELM_LAUNCH((k_stencil_sources<decltype(F), false>), grid, dim3(256), 0, op->stream, F, nsrc, ldu, (const cplx *)dC, coef, (cplx *)dR, ldr, op->nz, op->nx);
        return launched(op);
    });
}
extern "C" int helm_stencil_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im, int conj,
                                           void *dR, long long ldr) {
    return stencil_sources_launch(op, HostField::c128(dU), nsrc, ldu, dC, cmake(coef_re, coef_im), conj, dR, ldr);
}
extern "C" int helm_stencil_sources_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im,
                                               int conj, void *dR, long long ldr) {
    return stencil_sources_launch(op, HostField::packed(dU32, dExp), nsrc, ldu, dC, cmake(coef_re, coef_im), conj, dR, ldr);
}

// P_k[i] += sum_s UB[s ldb + i] UF[s ldf + i + off_k] for the nine lags k and the interior cells i (the boundary lines of P are left as they are: the rows of
// dC are zero there; an interior cell has every neighbour inside the grid).  A workgroup of LAG_WAVES waves owns a tile of OP_TILE_X x LAG_ROWS cells.  Column s
// goes to wave s mod LAG_WAVES, which keeps the 9 LAG_ROWS sums of its lane's cells in REGISTERS over all its columns: per column it loads the LAG_ROWS + 2 rows
// of UF and the LAG_ROWS rows of UB at once (ten 16-byte loads in flight per lane), gets the left and right neighbours of UF from the adjacent lanes and
// does 9 LAG_ROWS complex FMAs.  Then the waves add their sums into ONE LDS tile in wave order (36 KiB; nine accumulators per cell and wave side by side, the
// scheme of k_imaging_op, would be 9 x 64 KiB), and wave r adds row r to P: one writer per entry, a fixed order, no atomics -- the same bits on every run.
// Per cell and column 16 B of UB and 16 (8) B of UF, the latter times (1 + 2 / LAG_ROWS)(1 + 2 / OP_TILE_X) for the halo, which neighbouring workgroups read at the
// same time; the nine planes of P once per call.
constexpr int LAG_ROWS = 4;         // output rows per workgroup: 72 accumulator doubles per lane
constexpr int LAG_WAVES = 4;        // waves per workgroup
static_assert(LAG_ROWS <= LAG_WAVES, "wave r finishes row r");

template <class F>
__global__ __launch_bounds__(64 * LAG_WAVES) void k_lag_imaging(F UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc, cplx *__restrict__ P,
                                                                int nz, int nx) {
    __shared__ cplx part[LAG_ROWS][9][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X;
    const int x = (int)(blockIdx.x % ntx) * OP_TILE_X + lane - 1, z0 = (int)(blockIdx.x / ntx) * LAG_ROWS;
    const bool xin = x >= 0 && x < nx;
    const bool store = lane >= 1 && lane <= OP_TILE_X && x >= 1 && x <= nx - 2;
    const long long N = (long long)nz * nx;
    cplx acc[LAG_ROWS][9];
#pragma unroll
    for (int r = 0; r < LAG_ROWS; ++r)
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[r][k] = cmake(0.0, 0.0);
    for (int s = wave; s < nsrc; s += LAG_WAVES) {             // (wave-uniform: the lane exchanges stay complete)
        const double sc = UF.scale(s);
        typename F::raw rf[LAG_ROWS + 2];
        cplx rb[LAG_ROWS];
#pragma unroll
        for (int r = 0; r < LAG_ROWS + 2; ++r) {
            const int z = z0 - 1 + r;
            rf[r] = (xin && z >= 0 && z < nz) ? UF.load((long long)s * ldf + (long long)z * nx + x) : typename F::raw{};
        }
#pragma unroll
        for (int r = 0; r < LAG_ROWS; ++r) {
            const int z = z0 + r;
            rb[r] = (store && z >= 1 && z <= nz - 2) ? UB[(long long)s * ldb + (long long)z * nx + x] : cmake(0.0, 0.0);      // (zero off the interior: nothing is added there)
        }
#pragma unroll
        for (int wr = 0; wr < LAG_ROWS + 2; ++wr) {            // row z0 - 1 + wr of UF serves the output rows wr - 2 (dz = +1), wr - 1 (dz = 0) and wr (dz = -1)
            LagRow w;
            w.t = UF.scaled(rf[wr], sc);
            lane_left_right(w.t, w.l, w.r);
#pragma unroll
            for (int dz = -1; dz <= 1; ++dz) {
                const int r = wr - 1 - dz;
                if (r >= 0 && r < LAG_ROWS) {
                    cfma(acc[r][3 * (dz + 1) + 0], rb[r], w.l);
                    cfma(acc[r][3 * (dz + 1) + 1], rb[r], w.t);
                    cfma(acc[r][3 * (dz + 1) + 2], rb[r], w.r);
                }
            }
        }
    }
    for (int w = 0; w < LAG_WAVES; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < LAG_ROWS; ++r)
#pragma unroll
                for (int k = 0; k < 9; ++k) part[r][k][lane] = w == 0 ? acc[r][k] : cadd(part[r][k][lane], acc[r][k]);
        }
        __syncthreads();
    }
    if (wave < LAG_ROWS) {
        const int z = z0 + wave;
        if (store && z >= 1 && z <= nz - 2) {
            const long long i = (long long)z * nx + x;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                cplx *p = P + (long long)k * N + i;
                *p = cadd(*p, part[wave][k][lane]);
            }
        }
    }
}
static dim3 lag_grid(const helm_op *op) {
    return dim3((unsigned)(((op->nx + OP_TILE_X - 1) / OP_TILE_X) * ((op->nz + LAG_ROWS - 1) / LAG_ROWS)));
}

// P[k][i] += sum_s UB[s][i] UF[s][i + off_k] for k < 9 and the interior cells i of the handle's grid: UF [nsrc][ldf], UB [nsrc][ldb], P [9][N] complex128.  P must
// not overlap the fields.  Returns when P is complete.
static int lag_imaging_launch(helm_op *op, HostField UF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    helm_tuning_refresh();
    if (!op || !UF.u || !dUB || !dP || nsrc < 1 || ldf < op->N || ldb < op->N) return HELM_ERR_ARG;
    if (int rc = planes_handle_args(op, "helm_lag_imaging_accumulate_device")) return rc;       // (both entry points refuse under this name)
    const size_t pbytes = (size_t)op->N * 9 * sizeof(cplx);
    if (ranges_overlap(UF.u, UF.bytes(nsrc, ldf), dP, pbytes) || ranges_overlap(dUB, (size_t)nsrc * ldb * sizeof(cplx), dP, pbytes)) return HELM_ERR_ARG;
    if (!UF.ok() || ((((uintptr_t)dUB) | ((uintptr_t)dP)) & 15)) return HELM_ERR_ARG;       // (the exponents and every alignment come after the handle)
    HIP_TRY(op, hipSetDevice(op->device));
    return UF.with([&](auto F) {
        HELM_LAUNCH(k_lag_imaging<decltype(F)>, lag_grid(op), dim3(64 * LAG_WAVES), 0, op->stream, F, ldf, (const cplx *)dUB, ldb, nsrc, (cplx *)dP, op->nz, op->nx);
        return launched(op);
    });
}
extern "C" int helm_lag_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    return lag_imaging_launch(op, HostField::c128(dUF), ldf, dUB, ldb, nsrc, dP);
}
extern "C" int helm_lag_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    return lag_imaging_launch(op, HostField::packed(dUF32, dExp), ldf, dUB, ldb, nsrc, dP);
}

// G[j] += w sum_(k, i) L_((k, i), j) P_k[i] (CONJ: conj(L)): the transpose of k_buoyancy_planes as a gather, one lane per cell j over the interior rows i = j - o of
// the 3 x 3 block around it.  Row i holds b_j three ways: kappa_j b_j times the mass weight in the plane of the lag o; (b_i + b_j) / 2 in the average of that
// lag; and, for i = j, b_i / 2 in all eight averages.  With T the row's own stiffness factors (mz_star: corners tc, verticals tv, horizontals th, the cross
// term tzx) the coefficient of the average of lag o is
//     Q_o = T_o (P_o - P_4)  [+ tzx (P_(sz, 0) - P_(0, sx)) for a corner o = (sz, sx)]
// (the centre plane takes every average with the opposite sign: the stiffness rows sum to zero).  One writer per cell, a fixed order.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_buoyancy_adjoint(MzParams P, const cplx *__restrict__ c, const cplx *__restrict__ Pl, cplx w, cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int jz = (int)(j / P.nx), jx = (int)(j % P.nx);
    cplx mass = cmake(0.0, 0.0), avg = cmake(0.0, 0.0);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int iz = jz - sz, ix = jx - sx;                 // row i sees cell j at the lag (sz, sx)
            if (iz < 1 || iz > P.nz - 2 || ix < 1 || ix > P.nx - 2) continue;
            const long long i = (long long)iz * P.nx + ix;
            const MzStiff t = mz_stiffness<CONJ>(P, mz_row_at(P, c, iz, ix));
            const double m = (sz == 0 && sx == 0) ? MZ_WC : ((sz == 0 || sx == 0) ? MZ_WD : MZ_WE);
            const cplx p = Pl[(long long)mz_slot(sz, sx) * N + i];
            mass.x += m * p.x; mass.y += m * p.y;
            if (sz == 0 && sx == 0) {
#pragma unroll
                for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
                    for (int ox = -1; ox <= 1; ++ox)
                        if (oz != 0 || ox != 0) avg = cadd(avg, lag_coefficient(t, Pl, N, i, oz, ox));
            } else avg = cadd(avg, lag_coefficient(t, Pl, N, i, sz, sx));
        }
    cplx kap = mz_kappa(P, c[j]);
    if (CONJ) kap = cconj(kap);
    cplx sum = cscale(avg, 0.5);
    cfma(sum, kap, mass);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// G[j] += w sum_(k, i) L_((k, i), j) P_k[i] for j < N (conj != 0: the conjugated coefficients), L the map of helm_buoyancy_planes_device for the operator the
// handle holds: P [9][N] complex128 (its boundary rows are not read), G N complex128.  G must not overlap P.  Returns when G is complete.
extern "C" int helm_buoyancy_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG) {
    helm_tuning_refresh();
    if (!op || !dP || !dG) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_buoyancy_adjoint_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dG)) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dP, (size_t)op->N * 9 * sizeof(cplx), dG, (size_t)op->N * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_buoyancy_adjoint_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
    if (conj) HELM_LAUNCH(k_buoyancy_adjoint<true>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dG);
    else HELM_LAUNCH(k_buoyancy_adjoint<false>, grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const cplx *)dP, cmake(w_re, w_im), (cplx *)dG);
    return launched(op);
}

// ------------------------------------------------------------------------------------------
// the total velocity derivative of MiniZephyr (linearisation='full'): mass term, PML stretch and the density that follows c
// ------------------------------------------------------------------------------------------
// A row is mz_star(row_i, bn, Kn): linear in (row, Kn) for fixed averaged buoyancies bn and linear in (bn, Kn) for a fixed row.  The row factors are functions of
// c_i, the mass terms Kn_k = kappa_j b_j of c_j (j = i + o_k), so along a real dc the nine planes of dA are
//     dC_i = mz_star(dc_i d row_i / dc, bn[b], Kn_k = (d kappa_j / dc) b_j dc_j)        (the mass term of k_virtual_sources_op and the stretch it leaves out)
//          + mz_star(row_i, bn[db], Kn_k = kappa_j db_j)                               (only where the density follows c: db = (d b / d c) dc, the caller's)
// with b = 1 / rho of the model the handle assembled with, boundary rows zero.  The forward and imaging loops are those of the density derivative
// (k_stencil_sources, k_lag_imaging); the transpose of the second star is k_buoyancy_adjoint.

// dC = V[dc] (+ L[db] when db is given): one lane per cell, the assembly's star once or twice.  An interior row reads only cells inside the grid.
__global__ __launch_bounds__(256) void k_velocity_planes(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const double *__restrict__ dc,
                                                         const double *__restrict__ db, cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);
    cplx out[9];
    if (iz == 0 || iz == P.nz - 1 || ix == 0 || ix == P.nx - 1) {
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = cmake(0.0, 0.0);
    } else {
        MzRow drow = mz_row_dc_at(P, c, iz, ix);
        const double v0 = dc[i];
        drow.X = cscale(drow.X, v0); drow.Z = cscale(drow.Z, v0); drow.px = cscale(drow.px, v0); drow.pz = cscale(drow.pz, v0);
        double bn[9];
        cplx Kn[9];
        const double b0 = 1.0 / rho[i];
#pragma unroll
        for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
            for (int sx = -1; sx <= 1; ++sx) {
                const long long j = i + (long long)sz * P.nx + sx;
                const double bj = 1.0 / rho[j];
                bn[mz_slot(sz, sx)] = (b0 + bj) / 2.0;
                Kn[mz_slot(sz, sx)] = cscale(mz_kappa_dc(P, c[j]), bj * dc[j]);
            }
        mz_star(P, drow, bn, Kn, out);
        if (db) {
            const MzRow row = mz_row_at(P, c, iz, ix);
            cplx more[9];
            const double d0 = db[i];
#pragma unroll
            for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
                for (int sx = -1; sx <= 1; ++sx) {
                    const long long j = i + (long long)sz * P.nx + sx;
                    const double dj = db[j];
                    bn[mz_slot(sz, sx)] = (d0 + dj) / 2.0;
                    Kn[mz_slot(sz, sx)] = cscale(mz_kappa(P, c[j]), dj);
                }
            mz_star(P, row, bn, Kn, more);
#pragma unroll
            for (int k = 0; k < 9; ++k) out[k] = cadd(out[k], more[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[(long long)k * N + i] = out[k];
}

// dC[9][N] = V[dc] + (dDb ? L[db] : 0) for the operator the handle holds (its c and rho, PML and the frequency of its last assembly): dc, db N float64 (db may be
// NULL), dC 9 N complex128, boundary rows zero.  Returns when dC is complete.
extern "C" int helm_velocity_planes_device(helm_op *op, const void *dDc, const void *dDb, void *dC) {
    helm_tuning_refresh();
    if (!op || !dDc || !dC) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, "helm_velocity_planes_device")) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dDc) | ((uintptr_t)dDb)) & 7) || (((uintptr_t)dC) & 15)) return HELM_ERR_ARG;
    const size_t cbytes = (size_t)op->N * 9 * sizeof(cplx);
    if (ranges_overlap(dDc, (size_t)op->N * 8, dC, cbytes) || (dDb && ranges_overlap(dDb, (size_t)op->N * 8, dC, cbytes))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "helm_velocity_planes_device: the handle holds no assembled operator");
    HIP_TRY(op, hipSetDevice(op->device));
    HELM_LAUNCH(k_velocity_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const double *)dDc,
                (const double *)dDb, (cplx *)dC);
    return launched(op);
}

// G[j] += w sum_(k, i) V_((k, i), j) P_k[i] (CONJ: conj(V)): the transpose of the first star of k_velocity_planes, one lane per cell j -- mz_transpose_at
// (survey_internal.hpp) with the first derivatives.  STRETCH false: the transpose of the mass term alone, the planes of k_mass_planes (survey_newton.hip).  One writer
// per cell, a fixed order; the boundary rows of P are not read.
template <bool CONJ, bool STRETCH>
__global__ __launch_bounds__(256) void k_velocity_adjoint(MzParams P, const cplx *__restrict__ c, const double *__restrict__ rho, const cplx *__restrict__ Pl, cplx w,
                                                          cplx *__restrict__ G) {
    const long long N = (long long)P.nz * P.nx;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const cplx sum = mz_transpose_at<1, CONJ, STRETCH>(P, c, rho, Pl, j);
    cplx g = G[j];
    cfma(g, w, sum);
    G[j] = g;
}

// G[j] += w sum_(k, i) V_((k, i), j) P_k[i] for j < N (conj != 0: the conjugated coefficients), V the map of helm_velocity_planes_device with dDb NULL for the
// operator the handle holds (helm_mass_adjoint_device: of helm_mass_planes_device, the mass term alone): P [9][N] complex128 (its boundary rows are not read), G N
// complex128.  G must not overlap P.  Returns when G is complete.
static int velocity_adjoint_launch(helm_op *op, const char *what, const void *dP, cplx w, int conj, bool stretch, void *dG) {
    helm_tuning_refresh();
    if (!op || !dP || !dG) return HELM_ERR_ARG;
    if (int rc = mz_handle_args(op, what)) return rc;
    if (op->nz < 3 || op->nx < 3 || ((((uintptr_t)dP) | ((uintptr_t)dG)) & 15)) return HELM_ERR_ARG;
    if (ranges_overlap(dP, (size_t)op->N * 9 * sizeof(cplx), dG, (size_t)op->N * sizeof(cplx))) return HELM_ERR_ARG;
    MzParams P;
    if (helm_mz_params(op, &P)) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle holds no assembled operator", what);
    HIP_TRY(op, hipSetDevice(op->device));
    const dim3 grid((unsigned)((op->N + 255) / 256));
#define VADJOINT(CJ, ST) HELM_LAUNCH((k_velocity_adjoint<CJ, ST>), grid, dim3(256), 0, op->stream, P, (const cplx *)op->d_c, (const double *)op->d_rho, (const cplx *)dP, w, (cplx *)dG)
    if (conj && stretch) VADJOINT(true, true);
    else if (conj) VADJOINT(true, false);
    else if (stretch) VADJOINT(false, true);
    else VADJOINT(false, false);
#undef VADJOINT
    return launched(op);
}
extern "C" int helm_velocity_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG) {
    return velocity_adjoint_launch(op, "helm_velocity_adjoint_device", dP, cmake(w_re, w_im), conj, true, dG);
}
extern "C" int helm_mass_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG) {
    return velocity_adjoint_launch(op, "helm_mass_adjoint_device", dP, cmake(w_re, w_im), conj, false, dG);
}
