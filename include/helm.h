/*
 * helm.h -- C ABI of libhelm: MI355X-native frequency-domain Helmholtz operator
 *           (assemble the 9-point 2-D / 27-point 3-D PML-damped complex stencil on the GPU, apply it,
 *           and solve A(w) u = q for many right-hand sides: in 2-D by a sparse direct factorisation
 *           kept per frequency -- nested dissection, multifrontal, batched dense kernels -- with the
 *           stencil kernel checking the true residual; in 3-D and as fallback by multigrid-
 *           preconditioned / Jacobi-preconditioned BiCGSTAB and CGNR built on the same stencil kernel).
 *
 * This is the drop-in boundary for the hot path of uwoseis/zephyr's backend.  Each entry
 * point names the reference interface it replaces (paths relative to the reference tree):
 *
 *   helm_create / helm_set_model   <- BaseModelDependent / BaseDiscretization config ingestion
 *                                     zephyr/backend/base.py:11-109, discretization.py:23-76
 *   helm_assemble                  <- MiniZephyr._initHelmholtzNinePoint  minizephyr.py:40-298
 *                                     Eurus._initHelmholtzNinePoint       eurus.py:28-485
 *   helm_get_diagonals             <- the `.A` property                   minizephyr.py:300-306, eurus.py:487-492
 *   helm_apply[_device]            <- `A * x` (scipy CSR product)         used by tests / parity
 *   helm_solve[_device]            <- BaseDiscretization.__mul__          discretization.py:78-106
 *                                     (problemo.BestSolver LU + premul + conjugate),
 *                                     Eurus.__mul__ pad/clip              eurus.py:512-533
 *   helm_prefactor                 <- the worker pool of BaseMPDist.__mul__ (distributors.py:80-96,161-168): the LU of the
 *                                     NEXT frequency is built while the current one is being solved
 *   helm_reserve                   <- (same pool: its workers' scratch, allocated before they start)
 *   helm_imaging_accumulate_device <- zero-lag imaging condition in HelmBaseProblem.Jtvec
 *                                     zephyr/middleware/problem.py:152,162
 *   helm_energy_accumulate_device,
 *   helm_energy_accumulate_c64_device <- (no counterpart) HelmBaseProblem.illumination: sum_s |u_s|^2 of wavefields in HBM
 *   helm_set_transposed            <- (no counterpart) the handle holds A^T: HelmBaseProblem.Jtvec(adjoint='transpose') back-propagates through A^-T
 *   helm_virtual_sources_device,
 *   helm_virtual_sources_c64_device <- (no counterpart) HelmBaseProblem.JvecBorn: conj(W (.) u_s), the right-hand sides of Born data
 *   helm_virtual_sources_op[_c64]_device,
 *   helm_imaging_op_accumulate[_c64]_device <- (no counterpart) the same two with linearisation='operator': the mass stencil of the assembled operator fused in
 *   helm_axpby_device,
 *   helm_sample_accumulate_device  <- MiniZephyr25D.__mul__: the sum over ky sub-problems
 *                                     (`reduce(np.add, ...)`, scaled)     minizephyr.py:435-460
 *   helm_sample_rows_device,
 *   helm_rhs_from_samples_device   <- a receiver array that moves with the source (geom mode 'relative'):
 *                                     HelmBaseSurvey rVec / getResidualSources   zephyr/middleware/survey.py:114-125,171-188
 *   helm_pack_c64_device,
 *   helm_imaging_accumulate_c64_device,
 *   helm_sample_rows_c64_device    <- forward fields handed to dpred / Jtvec as `u=` (problem.py:124-164, survey.py:190-198),
 *                                     kept in HBM at half size
 *   helm_misfit_moments_device,
 *   helm_misfit_terms_device,
 *   helm_misfit_adjoint_device     <- (no counterpart; the reference left the objective to SimPEG's l2_DataMisfit) zephyr_amd/misfit.py: the data misfit,
 *                                     its source estimate and its adjoint source on the sample panels of a work item
 *   helm_destroy                   <- `del obj.factors` / __del__         discretization.py:86-99
 *
 * Conventions
 *   - complex128 values are interleaved (re, im) doubles; a field is the row-major (nz, nx)
 *     ravel of the reference (linear index iz*nx + ix, base.py:93).
 *   - multi-RHS buffers hold each right-hand side contiguously: X[r*rows + i]   (the Python
 *     host passes np.ascontiguousarray(rhs.T)).
 *   - coefficient planes: C[block][k][iz*nx+ix], k = 3*(dz+1) + (dx+1), meaning
 *     (A x)[iz,ix] = sum_k C[k][iz,ix] * x[iz+dz, ix+dx].  MiniZephyr has 1 block, Eurus 4
 *     (M1, M2, M3, M4 of the 2N x 2N system, eurus.py:430-464).
 *   - every function returns an int status: 0 = ok, > 0 = number of right-hand sides that
 *     did not reach the tolerance (helm_solve only), < 0 = hard error (HELM_ERR_*); the text
 *     is available from helm_last_error().  No exceptions cross this boundary.
 *   - the caller owns host buffers; the library owns all device memory behind the handle.
 *     `_device` variants take device pointers valid on the handle's GPU.
 *   - a handle is bound to one GPU and must be used by one host thread at a time.
 */
#ifndef HELM_H
#define HELM_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct helm_op helm_op;

/* discretisation variants */
enum { HELM_MINIZEPHYR = 0, HELM_EURUS = 1, HELM_3D = 2 /* 27-point 3-D operator, created with helm_create3d */ };

/* Krylov methods */
enum {
    HELM_BICGSTAB = 0,   /* Jacobi-preconditioned BiCGSTAB */
    HELM_CGNR = 1,       /* Jacobi-scaled CGNR */
    HELM_AUTO = 2,       /* HELM_DIRECT for every 2-D system; if that fails, and in 3-D: HELM_MG where available, else
                            BiCGSTAB, with CGNR for right-hand sides that break down */
    HELM_MG = 3,         /* BiCGSTAB right-preconditioned by shifted-Laplacian multigrid (damped-Jacobi smoothing)
                            + PML strip line relaxation */
    HELM_DIRECT = 4      /* sparse direct: nested-dissection multifrontal factorisation kept on the handle until the next
                            helm_assemble and re-used for every right-hand side (what the reference's sparse LU does,
                            discretization.py:78-103), plus iterative refinement with the stencil kernel to rtol.
                            2-D: MiniZephyr, Eurus with eps == delta (block-triangular) and the coupled TTI system
                            (eps != delta, two unknowns per cell, row-equilibrated); not the 3-D operator */
};

/* hard errors */
enum {
    HELM_OK = 0,
    HELM_ERR_ARG = -1,         /* bad argument / dimension mismatch (reference: ValueError) */
    HELM_ERR_DEVICE = -2,      /* HIP runtime failure (no GPU, allocation, launch) */
    HELM_ERR_STATE = -3,       /* call order: model/assemble missing */
    HELM_ERR_UNSUPPORTED = -4, /* configuration outside the supported path */
    HELM_ERR_PML = -5          /* Eurus PML profile length hazard (reference raises ValueError, eurus.py:84-91) */
};

/* buffer layouts of the solve entry points (helm_solve_opts.flags).  Default (0): one right-hand side / wavefield per row,
 * X[r*rows + i] (what np.ascontiguousarray(rhs.T) gives).  NODE_MAJOR: the reference's own (rows, nrhs) C-order arrays,
 * X[i*nrhs + r] -- what `Disc * rhs` receives and what lu.solve returns (discretization.py:101-103).  With both set the direct
 * path uses the right-hand sides where they lie and writes the wavefield from the kernel that checks its residual: no transposes. */
enum { HELM_RHS_NODE_MAJOR = 1, HELM_OUT_NODE_MAJOR = 2, HELM_NODE_MAJOR = 3 };

typedef struct helm_solve_opts {
    int method;        /* HELM_BICGSTAB | HELM_CGNR | HELM_AUTO | HELM_MG | HELM_DIRECT */
    double rtol;       /* stop when ||q' - A u||_2 / ||q'||_2 <= rtol (q' = premul*rhs), per RHS */
    int maxit;         /* iteration cap per right-hand side */
    int check_every;   /* iterations between host-side convergence checks (0 = default) */
    int batch;         /* right-hand sides iterated together on the device (0 = default) */
    int flags;         /* buffer layouts: 0, or HELM_RHS_NODE_MAJOR | HELM_OUT_NODE_MAJOR */
} helm_solve_opts;

typedef struct helm_solve_info {
    int iterations;    /* iterations used by this right-hand side (HELM_DIRECT: triangular solves incl. refinement) */
    int status;        /* 0 converged, 1 iteration cap / stalled above rtol, 2 breakdown (not recovered), 3 direct path (in practice the coupled TTI system):
                        * the true residual has reached the floor fp64 allows for this right-hand side, relres <= 8 eps || |A||x| + |q| || / ||q||,
                        * which lies above rtol -- no fp64 vector does better (a backward-stable LU lands on the same floor); counted as solved */
    int restarts;      /* BiCGSTAB restarts taken */
    int method;        /* method that produced the returned wavefield */
    double relres;     /* final TRUE relative residual ||q' - A u|| / ||q'|| (unscaled system) */
} helm_solve_info;

/* --- lifecycle ------------------------------------------------------------------------ */
int helm_device_count(void);                   /* < 0 on HIP failure */
const char *helm_version(void);

/* freeSurf: 4 ints, reference order [iz=0 side, ix=nx-1 side, iz=nz-1 side, ix=0 side]
 * (minizephyr.py:103-115,269-298); ignored by Eurus as in the reference.
 * Returns NULL on failure; helm_last_error(NULL) holds the reason. */
helm_op *helm_create(int device, int variant, int nz, int nx, double dx, double dz,
                     int nPML, const int *freeSurf);
/* 3-D 27-point operator on an (nz, ny, nx) grid, linear index (iz*ny + iy)*nx + ix; 27 planes,
 * k = 9*(oz+1) + 3*(oy+1) + (ox+1).  No reference counterpart (the reference has no 3-D discretisation:
 * zephyr/backend/base.py:20,36-40, source.py:43-44); definition in oracle/helm3d_oracle.py.  All other entry
 * points (set_model with theta/eps/delta NULL, assemble with ky ignored and cPML the layer amplitude,
 * get_diagonals, apply, solve with rows = N) work on the returned handle; solves use the Jacobi-preconditioned
 * BiCGSTAB / CGNR, right-preconditioned by a 3-D shifted-Laplacian multigrid under HELM_MG / HELM_AUTO. */
helm_op *helm_create3d(int device, int nz, int ny, int nx, double dx, double dy, double dz, int nPML);
void helm_destroy(helm_op *op);
const char *helm_last_error(const helm_op *op);

/* Use an existing hipStream_t (e.g. torch's current stream) for all work; NULL = own stream. */
int helm_set_stream(helm_op *op, void *hip_stream);

/* --- model and assembly --------------------------------------------------------------- */
/* c: N complex; rho: N doubles or NULL (Gardner 310*Re(c)^0.25, discretization.py:70);
 * theta/eps/delta: N doubles each or NULL (zeros), Eurus only (base.py:112-149). */
int helm_set_model(helm_op *op, const double *c, const double *rho,
                   const double *theta, const double *eps, const double *delta);

/* freq complex (Hz); tau Laplace damping time constant (inf = none); ky cross-line wavenumber
 * (MiniZephyr only); cPML Eurus C-PML amplitude (eurus.py:500-504). */
int helm_assemble(helm_op *op, double freq_re, double freq_im, double tau, double ky, double cPML);

/* The transposed operator.  on != 0: the NEXT helm_assemble leaves the coefficient planes of A^T in the handle (on == 0: of A again), and everything that reads
 * them works on A^T from then on -- the direct factorisation and its true-residual check (relres is that of A^T x = premul q), the Jacobi-scaled planes and the
 * Krylov methods, the levels of the 2-D multigrid preconditioner, helm_apply, helm_get_diagonals: helm_solve* returns conj(A^-T (premul rhs)).  The 9-point
 * MiniZephyr operator is not symmetric (its rows are scaled by PML and density terms), so this, not the forward solve, back-propagates a residual exactly.
 * With slot k = 3 (dz + 1) + (dx + 1) and off_k = dz nx + dx:  CT[k][i] = C[8 - k][i + off_k]  where cell (iz + dz, ix + dx) is inside the grid, else 0.
 * The call itself drops what was derived from the planes (factors, also those in flight; scaled planes; preconditioner) when it changes the setting, and leaves
 * the planes as they are until the next helm_assemble.  2-D MiniZephyr handles; Eurus and 3-D handles: HELM_ERR_UNSUPPORTED. */
int helm_set_transposed(helm_op *op, int on);
int helm_get_transposed(const helm_op *op);    /* 1: the planes in the handle (helm_get_diagonals) are those of A^T, 0: of A */

/* The transposed 3-D operator, through an entry point of its own (helm_set_transposed keeps refusing 3-D handles).  on != 0: the NEXT helm_assemble of a
 * helm_create3d handle leaves the 27 planes of A^T in it (on == 0: of A again) and helm_get_transposed returns 1.  With slot k = 9 (oz + 1) + 3 (oy + 1) + (ox + 1):
 * CT[k][p] = C[26 - k][p + o]  where cell p + o is inside the grid, else 0 -- a permutation.  The 27-point operator is not symmetric: its rows are scaled by 1 / xi,
 * its mass entries carry K of the column's cell.  The preconditioner of such a handle is the transpose of the cycle of A: the standard shifted cycle with its levels
 * assembled transposed, the layer-preserving hierarchy built for A, its levels (Galerkin product included) transposed afterwards and its transfers exchanged
 * (P^T = D^-1 R, R^T = P D).  Methods 'auto', 'mg' and 'bicgstab' solve A^T x = premul q; the apply reads the 27 stored planes (the on-the-fly coefficients
 * rebuild A, not A^T).  What the call drops and when it takes effect: as helm_set_transposed.  Any other handle: HELM_ERR_UNSUPPORTED. */
int helm_set_transposed3d(helm_op *op, int on);

/* The transposed first block of an Eurus handle.  With eps == delta everywhere the Eurus system is block-triangular and an N-row right-hand side is solved
 * through M1 alone, u = M1^-1 q; on != 0 makes the NEXT helm_assemble leave the planes of M1^T in block 0 (on == 0: of M1 again), by the plane formula above, and
 * helm_get_transposed then returns 1.  helm_solve* with an N-row right-hand side returns conj(M1^-T (premul rhs)) through the direct path.  A handle that holds M1^T
 * serves nothing else: a stacked 2N right-hand side, blocks 1 .. 3 (helm_get_block_diagonals, helm_get_diagonals, helm_apply), the scaled planes, a Krylov `method`
 * and the Krylov fallback after a failed factorisation return HELM_ERR_UNSUPPORTED -- the untransposed blocks are never served in its place.  A model with
 * eps != delta anywhere (the coupled 2N x 2N system has no transposed solve), a MiniZephyr or a 3-D handle: HELM_ERR_UNSUPPORTED; before helm_set_model:
 * HELM_ERR_STATE.  helm_set_transposed keeps refusing Eurus handles. */
int helm_set_transposed_m1(helm_op *op, int on);
/* on != 0: helm_stencil_sources[_c64]_device and helm_lag_imaging_accumulate[_c64]_device serve this 2-D Eurus handle (they read nothing but nine planes and the
 * grid; the derivative routes of an Eurus problem run them on the planes of helm_eurus_planes_device).  0, the default: they return HELM_ERR_UNSUPPORTED for it as
 * they always did.  Any other handle: HELM_ERR_UNSUPPORTED. */
int helm_set_eurus_derivatives(helm_op *op, int on);

int helm_num_blocks(const helm_op *op);        /* 1 (MiniZephyr) or 4 (Eurus) */
long long helm_num_points(const helm_op *op);  /* N = nz*nx */

/* out: num_blocks * 9 * N complex, layout C[block][k][i] */
int helm_get_diagonals(helm_op *op, double *out);
/* out: 9 * N complex, the planes C[block][k][i] of one block.  Block 0 of an Eurus handle needs no other block to exist. */
int helm_get_block_diagonals(helm_op *op, int block, double *out);

/* --- operator application (parity / microbenchmark) ----------------------------------- */
/* Y[r] = M_block X[r], r < nrhs; adjoint != 0 applies the conjugate transpose. */
int helm_apply(helm_op *op, int block, int adjoint, const double *X, double *Y, int nrhs);
int helm_apply_device(helm_op *op, int block, int adjoint, const void *dX, void *dY, int nrhs);

/* --- solve ---------------------------------------------------------------------------- */
/* U[r] = conj( A^-1 (premul * RHS[r]) ).  rows = N, or 2N for Eurus stacked right-hand sides
 * (eurus.py:512-533: N-row input is zero-padded and the result clipped to N rows; 2N-row input
 * returns 2N rows).  info: nrhs entries or NULL.  opts NULL = defaults.  RHS and U may be the same buffer (in place) or disjoint; they
 * must not overlap partially. */
int helm_solve(helm_op *op, const double *RHS, double *U, int nrhs, long long rows,
               double premul_re, double premul_im,
               const helm_solve_opts *opts, helm_solve_info *info);
int helm_solve_device(helm_op *op, const void *dRHS, void *dU, int nrhs, long long rows,
                      double premul_re, double premul_im,
                      const helm_solve_opts *opts, helm_solve_info *info);

/* Sparse right-hand sides given as host COO triplets (row: int64, col: int32 = right-hand side, val: complex128; no duplicates) --
 * the reference's scipy-sparse source matrices (survey.py:162-169), which problemo densifies on the host before the LU solve.
 * Here only the triplets cross PCIe; U (host, nrhs*rows complex128, layout per opts->flags) receives the wavefields. */
int helm_solve_coo(helm_op *op, const long long *row, const int *col, const double *val, long long nnz, double *U, int nrhs,
                   long long rows, double premul_re, double premul_im, const helm_solve_opts *opts, helm_solve_info *info);
/* Pinned host memory for result arrays (device-to-host copies into it run at the PCIe rate); recycled by size.
 * Host arrays in general (r6): every entry point above that takes one (helm_set_model, helm_apply, helm_solve, helm_solve_coo, helm_get_diagonals) moves it through
 * pinned 4-MB chunks of the library unless the array is pinned memory itself (this call, hipHostMalloc, hipHostRegister) -- then it is copied straight, which is
 * what a caller with GBs of wavefields wants.  The caller's pageable pages are never registered with the runtime: memory registered that way and later unmapped
 * (free() of a large array) makes the kernel driver evict every queue of the process for 15-20 ms (profiles/r06_config4_dpred_spread.txt). */
void *helm_host_alloc(size_t bytes);
void helm_host_free(void *p, size_t bytes);

/* Start the factorisation the next helm_solve[_device] on this handle will need, without waiting for it: the launches go to
 * a high-priority stream of the handle and run beside whatever other handles are doing on the GPU (a dispatcher solving
 * frequency k calls this for frequency k+1: the latency-bound top of the elimination tree then hides under the
 * bandwidth-bound triangular solves of the previous frequency).  A hint: returns HELM_OK without doing anything where the
 * direct path does not apply (3-D, coupled TTI) or factors already exist.  Requires helm_assemble.  The reference builds its
 * LU lazily inside the first `Disc * rhs` (discretization.py:78-85) and overlaps frequencies with a process pool
 * (distributors.py:161-168). */
int helm_prefactor(helm_op *op);
/* The same with the number of right-hand sides the next solve will bring (the reference's pool hands a sub-problem its right-hand sides together
 * with the job: distributors.py:161-166).  2-D: helm_prefactor.  3-D: the multigrid hierarchy and the
 * factorisation of its directly solved level are built NOW, in the calling thread (hundreds of ms): a dispatcher's prepare thread calls this
 * for frequency k+1 while another handle iterates on frequency k.  A hint like helm_prefactor. */
int helm_prefactor_n(helm_op *op, int nrhs);
/* helm_prefactor for n operators of the same grid on one GPU at once (2-D; n <= 4): their factorisations are enqueued TOGETHER -- the elimination tree depends
 * on the grid alone, so the fronts of n frequencies ride in the same strided batches, batch index = front x frequency.  The top of the tree is a chain of small
 * dependent launches that leaves most of the chip idle (88 block steps of ~30 us at 1024^2, gather-bound levels of 8-16 unknowns, products over one to four
 * fronts); that chain is now walked once per set.  Each operator's factors come out bit for bit what helm_prefactor would have made of them and are solved with
 * as usual, one operator at a time; the launches go to the high-priority stream of ops[0].  A hint: operators that do not qualify (3-D, coupled TTI, factors
 * already there, different grids) are prefactored one by one.  The reference overlaps frequencies with a process pool (distributors.py:161-168). */
int helm_prefactor_many(helm_op **ops, int n);
/* The relative tolerance the solves on this operator will ask for, told before its factors are built (helm_prefactor takes no options):
 * fronts whose condition estimate exceeds rtol / (8 eps) are re-eliminated with a pivoted LU so that one pass meets rtol.  Default 1e-10;
 * a solve that builds the factors itself uses its own opts->rtol.  Counterpart of the `Solver` the reference receives through its
 * systemConfig (discretization.py:23-31,83-84: SuperLU's pivoting is not negotiable there). */
int helm_set_tolerance_hint(helm_op *op, double rtol);

/* Scratch for `concurrent` host-array solves (helm_solve / helm_solve_coo) of `nrhs` right-hand sides with `rows` rows running at the
 * same time on this handle's GPU, allocated now instead of inside the first solves: the shared scratch slots of the direct path and the
 * device images of right-hand sides and wavefields.  For dispatchers that start several workers per GPU -- the worker pool of
 * BaseMPDist.__mul__ (distributors.py:80-96): a hipMalloc issued beside running kernels and copies can take a second.  A hint:
 * HELM_OK unless the arguments are invalid. */
int helm_reserve(helm_op *op, int nrhs, long long rows, int concurrent);

/* Timing of the last solve/apply on this handle, measured with HIP events on the handle's
 * stream: total ms, and ms / launches / algorithmic bytes of the stencil-apply kernel. */
typedef struct helm_timing {
    double solve_ms;
    double apply_ms;
    long long apply_launches;
    double apply_bytes;      /* sum over launches of N*(32*B + 144) */
    double factor_ms;        /* HELM_DIRECT: factorisation time when this solve had to factor, else 0 */
    double gemm_ms;          /* HELM_DIRECT: ms / launches / flops (8 M N K per batch item) of the dense complex GEMM kernel */
    long long gemm_launches;
    double gemm_flops;
    double gemm_big_ms;      /* the same over the launches of at least 1 GFLOP (throughput-bound ones) */
    long long gemm_big_launches;
    double gemm_big_flops;
    double gemm_bytes;       /* operand bytes of the same launches, every operand once: 16 (M K + K N + M N (1 or 2)) per batch item */
    double gemm_sol_ms;      /* sum over the launches of max(flops / 78.6 TFLOP/s, bytes / 8 TB/s): what the two roofs allow */
} helm_timing;
int helm_last_timing(const helm_op *op, helm_timing *out);
/* enable per-launch HIP-event timing of the stencil kernel inside solves (costs a little) */
int helm_set_profiling(helm_op *op, int on);

/* --- FWI imaging condition ------------------------------------------------------------ */
/* G[i] += scaler[i] * sum_{s<nsrc} UF[s][i] * UB[s][i]   (complex, no conjugation;
 * problem.py:152).  scaler: N complex (= -w^2/c^3).  All device pointers. */
int helm_imaging_accumulate_device(helm_op *op, const void *dUF, const void *dUB, int nsrc,
                                   const void *dScaler, void *dG);

/* --- illumination / diagonal pseudo-Hessian (Shin, Jang & Min 2001) --------------------- */
/* E[i] += alpha * (W ? W[i] : 1) * sum_{s<nsrc} |U[s*ld + i]|^2,  i < N = helm_num_points(op).  U: nsrc columns of complex128, ld >= N apart, 16-byte
 * aligned; E and W (may be NULL): N doubles, 8-byte aligned; alpha >= 0, W >= 0.  Plain fp64 without atomics, the sum over s in the order s = 0, 1, ...:
 * the same bits on every run, and with E >= 0 on entry |result - exact| <= (nsrc + 7) 2^-53 exact per cell (2 roundings per |.|^2, nsrc - 1 additions,
 * alpha W, its product with the sum, the addition to E).  Null pointers other than dW, nsrc < 1, ld < N, a misaligned pointer, alpha < 0 or NaN:
 * HELM_ERR_ARG.  All device pointers; returns when E is complete. */
int helm_energy_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, double alpha, const void *dW, void *dE);
/* R[s ldr + i] = conj(W[i] U[s ldu + i]), s < nsrc, i < N: the right-hand sides of Born data from stored forward fields (W = model perturbation times the
 * gradient scaler).  U: nsrc columns of ldu >= N complex128 values (or, _c64, complex64 values with the int32 column exponents dExp of helm_pack_c64_device);
 * W: N complex128; R: nsrc columns of ldr >= N complex128, not overlapping U or W; 16-byte aligned (U32: 8, dExp: 4).  Per component |error| <= 3 2^-53 times
 * the sum of the absolute values of its two products; no atomics, the same bits on every run.  Null pointers, nsrc < 1, ldu or ldr < N, a misaligned or
 * overlapping pointer: HELM_ERR_ARG.  All device pointers; returns when R is complete. */
int helm_virtual_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, void *dR, long long ldr);
int helm_virtual_sources_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dW, void *dR, long long ldr);

/* --- the exact Frechet derivative of MiniZephyr (HelmBaseProblem.JvecBorn / Jtvec with linearisation='operator') -------------------------------
 * MiniZephyr carries the velocity as K = (omega_d^2 / c^2 - ky^2) / rho of the neighbouring cell, spread over the nine slots by the mass weights, and its boundary
 * rows are +-identity: (dA) u = mask_int (.) M0(dK (.) u), M0 the constant 9-point stencil with weights 0.6248 (centre), 0.09381 (edges), 1.297e-6 (corners) on the
 * handle's nz x nx grid (cells outside contribute nothing), mask_int zero on the four boundary lines.
 *
 * R[s ldr + i] = coef mask_int[i] M0(W (.) X[s])[i], X[s] = U[s] or (conj != 0) conj(U[s]), s < nsrc, i < N.  U: nsrc columns of ldu >= N complex128 values (or, _c64,
 * complex64 values with the int32 column exponents dExp of helm_pack_c64_device); W: N complex128; R: nsrc columns of ldr >= N complex128, not overlapping U or
 * W; 16-byte aligned (U32: 8, dExp: 4).
 *
 * G[i] += W[i] sum_{s<nsrc} UF[s ldf + i] M0(mask_int (.) UB[s])[i]: the imaging sum with the stencil (M0^T mask_int = M0 mask_int) applied to the back-propagated
 * columns UB (nsrc columns of ldb >= N complex128) on the fly; UF as U above; W, G: N complex128, G not overlapping the others.
 *
 * Plain fp64 in an order the code fixes (per cell: centre, the four edges, the four corners; s ascending), no atomics: the same bits on every run.  2-D MiniZephyr
 * handles; Eurus and 3-D handles: HELM_ERR_UNSUPPORTED.  Null pointers, nsrc < 1, a leading dimension < N, a misaligned or overlapping pointer: HELM_ERR_ARG.  All
 * device pointers; each call returns when its result is complete. */
int helm_virtual_sources_op_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im, int conj, void *dR,
                                   long long ldr);
int helm_virtual_sources_op_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im,
                                       int conj, void *dR, long long ldr);
int helm_imaging_op_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, const void *dW, void *dG);
int helm_imaging_op_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc, const void *dW,
                                          void *dG);

/* --- the velocity derivative of the 3-D 27-point operator on stored columns (survey3d.hip) -----------------------------------------------------
 * With an explicit density the derivative of a helm_create3d operator along the velocity is its mass term alone, dA[dc] = M~ diag(chi dc), chi = -2 K / c,
 * K = om~^2 / (rho c^2): M~ the constant 27-point stencil mu_o = a [o == 0] + (1 - a) m(ox) m(oy) m(oz) (a = 1/2, m(0) = 2/3, m(+-1) = 1/6) with the rows on the
 * box boundary zeroed.
 *
 * helm_mass3_sources_device:  R[s ldr + i] = coef M~(W (.) X[s])[i], X[s] = U[s] or (conj != 0) conj(U[s]), s < nsrc, i < N; the boundary rows of R are exact
 *     zeros.  U: nsrc columns of ldu >= N complex128; W: N complex128; R: nsrc columns of ldr >= N complex128, not overlapping U or W.
 * helm_mass3_imaging_accumulate_device:  P[j] += sum_{s<nsrc} UF[s ldf + j] (M~^T UB[s])[j] for every cell j; the boundary rows of UB are masked, not read.
 *     UF, UB: nsrc columns of ldf, ldb >= N complex128; P: N complex128, not overlapping them.  s ascending, one store per cell.
 * helm_mass3_chain_device:  chi at the model and the damped frequency of the handle's last assembly, one call for both directions.  dDc != NULL (Born): dOut is N
 *     complex128, dOut[j] = w chi_j dDc[j] (dDc N float64; dP is not read).  dDc == NULL (gradient): dOut is N float64, dOut[j] += Re(w chi_j dP[j]).
 *
 * Plain fp64 in an order the code fixes, no atomics: the same bits on every run.  3-D handles; any other handle: HELM_ERR_UNSUPPORTED.  Null pointers, nsrc < 1,
 * a leading dimension < N, a misaligned (16 bytes; float64 arrays 8) or overlapping pointer: HELM_ERR_ARG.  All device pointers; each call returns when its
 * result is complete. */
int helm_mass3_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im, int conj, void *dR,
                              long long ldr);
int helm_mass3_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP);
int helm_mass3_chain_device(helm_op *op, const void *dP, double w_re, double w_im, const void *dDc, void *dOut);

/* --- the buoyancy derivative of the 3-D 27-point operator on stored columns (survey3d_density.hip) ---------------------------------------------
 * An interior row is linear and homogeneous in b = 1 / rho: dA[db] = 1/2 diag(db) L + 1/2 L diag(db) + M~ diag(kappa db), kappa = om~^2 / c^2, L the matrix of
 *     lap_o(p) = Lx[ox](ix) m(oy) m(oz) / dx^2 + m(ox) Ly[oy](iy) m(oz) / dy^2 + m(ox) m(oy) Lz[oz](iz) / dz^2
 * on interior rows (boundary rows empty), the stretch tables of the handle's last assembly read at the ROW p: L is not symmetric.  The kappa part goes through
 * the helm_mass3_* entry points with the weights the chain below makes.
 *
 * helm_lap3_sources_device:  R[s ldr + i] = coef (1/2 B (.) (L X[s]) + 1/2 L(B (.) X[s]))[i], X[s] = U[s] or (conj != 0) conj(U[s]); B: N float64.  add == 0: the
 *     boundary rows of R are exact zeros; add != 0: the interior rows receive the value on top of what they hold, the boundary rows are left alone.
 * helm_lap3_imaging_accumulate_device:  P[j] += 1/2 sum_{s<nsrc} (UB0[s][j] (L UF[s])[j] + UF[s][j] (L^T UB0[s])[j]) for every cell j, UB0 = UB with its boundary
 *     rows masked (not read); conj != 0: both fields are conjugated as they are read.  s ascending, one store per cell.
 * helm_buoy3_chain_device:  chain = -1 / rho^2 (gardner == 0) or d b / d c = -b / (4 Re c) (gardner != 0), b = 1 / rho, at the model of the handle.  dIn != NULL
 *     (Born): dDb[j] = chain_j dIn[j] (N float64 each) and dOut[j] = w kappa_j dDb[j] (N complex128).  dIn == NULL (gradient): dOut is N float64,
 *     dOut[j] += chain_j Re(w (dPlap[j] + kappa_j dPmass[j])).
 *
 * Plain fp64 in an order the code fixes, no atomics.  Assembled 3-D handles; any other handle: HELM_ERR_UNSUPPORTED, not assembled: HELM_ERR_STATE.  Null
 * pointers, nsrc < 1, a leading dimension < N, a misaligned (16 bytes; float64 arrays 8) or overlapping pointer: HELM_ERR_ARG.  All device pointers; each call
 * returns when its result is complete. */
int helm_lap3_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dB, double coef_re, double coef_im, int conj, int add, void *dR,
                             long long ldr);
int helm_lap3_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, int conj, void *dP);
int helm_buoy3_chain_device(helm_op *op, int gardner, const void *dIn, const void *dPlap, const void *dPmass, double w_re, double w_im, void *dDb, void *dOut);

/* --- the pseudo-Hessian diagonal and the (c, rho) blocks of the 3-D 27-point operator from stored columns (survey3d_hessian.hip) ----------------------
 * H_p[i] = sum_s ||(dA / dp_i) X[s]||^2 and B_ab[i] = sum_s Re <(dA / da_i) X[s], (dA / db_i) X[s]>.  The column of a unit perturbation of cell i touches the 27 rows
 * p = i + d; per cell and column only X[s][i] and T = (L X[s])[i] enter, through r = A0_i X[s][i] + h_i T and the moments E = sum |X[i]|^2, D = sum |r|^2,
 * Y = sum conj(X[i]) r.  The rest is per-cell coefficients of the model of the handle's last assembly:
 *
 * helm_ph3_coefficients_device:  mode 0 (buoyancy): A0 = a_i(i), h = 1/2, S' = sum_{d != 0} |a_{i+d}(i)|^2, a_p(i) = [p interior] (1/2 lap_{-d}(i + d) + kappa_i mu_d),
 *     the tables read at the neighbour's row.  mode 1 (the total velocity derivative through the Gardner density, g = d b / d c = -b / (4 Re c)):
 *     A0 = chi mu_0 [i interior] + g a_i(i), h = g / 2, S' = sum_{d != 0} |chi mu_d [p interior] + g a_p(i)|^2, chi = -2 kappa b / c.  mode 2 (blocks): those of mode 0 and
 *     C' = sum_{d != 0} mu_d a_{i+d}(i), Smu = sum_{p interior} mu_d^2.  dA0, dC: N complex128; dH, dS, dSmu: N float64 (dC, dSmu may be NULL for modes 0, 1).
 * helm_ph3_moments_accumulate_device:  blocks == 0: dH[i] += alpha W_i (S'_i E + D) (dW NULL: no weight).  blocks != 0: three rows at stride ldh,
 *     dH[i] += alpha W_i |chi|^2 Smu E,  dH[ldh + i] += -alpha W_i Re conj(chi) (C' E + mu_0 [i interior] Y) / rho^2,  dH[2 ldh + i] += alpha W_i (S' E + D) / rho^4
 *     -- H_cc, H_crho, H_rhorho.  X[s] = U[s] or (conj != 0) conj(U[s]).  s ascending in one workgroup, one load and one store of dH per cell, no atomics.
 *
 * Handles, arguments and return codes as helm_lap3_sources_device (blocks != 0: ldh >= N). */
int helm_ph3_coefficients_device(helm_op *op, int mode, void *dA0, void *dH, void *dS, void *dC, void *dSmu);
int helm_ph3_moments_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ldu, int conj, int blocks, const void *dA0, const void *dHh, const void *dS,
                                       const void *dC, const void *dSmu, double alpha, const void *dW, void *dH, long long ldh);

/* --- the derivative maps of the Eurus block M1 (eps == delta) ---------------------------------------------------------------------------------
 * A row of M1 is linear and homogeneous in the buoyancies b = 1 / rho and the mass terms K = omega_d^2 b / c^2 of the 3 x 3 (edge-clamped) cells around it; its PML
 * averages do not depend on the model.  The entry built from the neighbour (sz, sx) lies in the matrix slot (-sz, sx).  An edge row keeps its centre entry alone,
 * and that entry depends on the model.
 *
 * helm_eurus_planes_device:  dC = V[dc] + L[db], the nine planes of d M1 along real (dc, db); either may be NULL.  L[db] is the row at b -> db,
 *     K -> omega_d^2 db / c^2; V[dc] the mass entries at K -> -2 omega_d^2 b dc / c^3.  dc, db: N float64; dC: 9 N complex128.
 * helm_eurus_adjoint_device:  Gc[j] += w (V^T P)[j], Gb[j] += w (L^T P)[j] (conj != 0: the conjugated coefficients) from one pass over P; either output may
 *     be NULL, not both.  P: 9 N complex128 (on edge rows the centre plane alone is read); Gc, Gb: N complex128.
 * helm_lag_centre_edges_accumulate[_c64]_device:  P[4][i] += sum_{s<nsrc} UB[s ldb + i] UF[s ldf + i] on the 2 (nz + nx) - 4 boundary cells i, which
 *     helm_lag_imaging_accumulate_device leaves alone.  Arguments as there.
 *
 * Plain fp64 in a fixed order, no atomics: the same bits on every run.  2-D Eurus handles whose model has eps == delta; anything else: HELM_ERR_UNSUPPORTED.
 * The maps are those of M1 whether or not the handle holds M1^T.  Argument checks as for the MiniZephyr derivatives below. */
int helm_eurus_planes_device(helm_op *op, const void *dDc, const void *dDb, void *dC);
int helm_eurus_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dGc, void *dGb);
int helm_lag_centre_edges_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP);
int helm_lag_centre_edges_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP);

/* --- the exact density derivative of MiniZephyr (HelmBaseProblem.JvecBorn / Jtvec with linearisation='operator', parameter='rho') ---------------
 * Every interior row of MiniZephyr is linear and homogeneous in the buoyancy field b = 1 / rho; its boundary rows are +-identity.  L maps a real field db (N) to
 * the nine planes dC[k][i], k = 3 (dz + 1) + (dx + 1), of d A / d b along db: the assembly's formulas on db, boundary rows zero, for the c, the PML and the frequency
 * of the operator the handle holds (HELM_ERR_STATE before the first helm_assemble).
 *
 * helm_buoyancy_planes_device:  dC = L[db].  db: N float64; dC: 9 N complex128.
 * helm_stencil_sources_device:  R[s ldr + i] = coef sum_k C[k][i] X[s][i + off_k], X[s] = U[s] or (conj != 0) conj(U[s]); cells outside the grid contribute
 *     nothing.  U: nsrc columns of ldu >= N complex128 (or, _c64, complex64 values with the int32 column exponents dExp of helm_pack_c64_device); C: 9 N
 *     complex128; R: nsrc columns of ldr >= N complex128.
 * helm_lag_imaging_accumulate_device:  P[k][i] += sum_{s<nsrc} UB[s ldb + i] UF[s ldf + i + off_k] for the interior cells i; the boundary lines of P are left
 *     as they are.  UF as U above; UB: nsrc columns of ldb >= N complex128; P: 9 N complex128.
 * helm_buoyancy_adjoint_device:  G[j] += w sum_{k, i} L_{(k, i), j} P[k][i] (conj != 0: conj(L)), the plain transpose of L; the boundary rows of P are not read.
 *     G: N complex128.
 *
 * Plain fp64 in an order the code fixes, no atomics: the same bits on every run.  An output must not overlap an input.  2-D MiniZephyr handles; Eurus and 3-D
 * handles: HELM_ERR_UNSUPPORTED.  Null pointers, nsrc < 1, a leading dimension < N, a grid below 3 x 3, a misaligned (16 bytes; U32: 8, dExp: 4, db: 8) or
 * overlapping pointer: HELM_ERR_ARG.  All device pointers; each call returns when its result is complete. */
int helm_buoyancy_planes_device(helm_op *op, const void *dDb, void *dC);
int helm_stencil_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im, int conj, void *dR,
                                long long ldr);
int helm_stencil_sources_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im,
                                    int conj, void *dR, long long ldr);
int helm_lag_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP);
int helm_lag_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP);
int helm_buoyancy_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG);

/* --- the total velocity derivative of MiniZephyr (HelmBaseProblem.JvecBorn / Jtvec with linearisation='full') -------------------------------------
 * A row is star(row_i, bn, Kn): the stretch factors row_i are functions of c_i, the mass terms Kn_k = kappa_j b_j of c_j, the averaged buoyancies bn of b = 1 / rho.
 * V maps a real field dc (N) to the nine planes of d A / d c along dc at the density the handle assembled with (the model's, or the Gardner default
 * 310 Re(c)^0.25 made by helm_set_model): star(dc_i d row_i / dc, bn[b], (d kappa_j / dc) b_j dc_j), boundary rows zero -- the mass term and the PML stretch.
 *
 * helm_velocity_planes_device:  dC = V[dc] + L[db] (dDb NULL: V[dc] alone).  db is the buoyancy perturbation that goes with dc where the density follows c
 *     (-0.25 b / Re(c) dc for the Gardner default; the caller's), L the map of helm_buoyancy_planes_device.  dc, db: N float64; dC: 9 N complex128.
 * helm_velocity_adjoint_device:  G[j] += w sum_{k, i} V_{(k, i), j} P[k][i] (conj != 0: conj(V)), the plain transpose of V; the boundary rows of P are not read.
 *     P: 9 N complex128; G: N complex128.  (The transpose of the L[db] part is helm_buoyancy_adjoint_device, times d b / d c.)
 *
 * The same rules as above: plain fp64 in a fixed order, one writer per entry; HELM_ERR_STATE before the first helm_assemble; Eurus, 3-D and ny > 0 handles
 * HELM_ERR_UNSUPPORTED; null (other than dDb), misaligned (16 bytes; dc, db: 8) or overlapping pointers and grids below 3 x 3 HELM_ERR_ARG. */
int helm_velocity_planes_device(helm_op *op, const void *dDc, const void *dDb, void *dC);
int helm_velocity_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG);

/* --- the residual part of the Newton Hessian of the exact derivatives (HelmBaseProblem.Hvec with resid=) ------------------------------------------
 * helm_velocity_curvature_device:  G[j] += w p[j] sum_{k, i} (d^2 A / dc_j^2)_{(k, i)} P[k][i] (conj != 0: the conjugated coefficients; stretch == 0: the mass term
 *     alone).  At the density the handle assembled with a row is star(row_i(c_i), bn, Kn_k = kappa(c_j) b_j) and the second derivative of the operator is zero between
 *     different cells: the sum is the transpose of helm_velocity_planes_device with d^2 row / dc^2 and d^2 kappa / dc^2 = 6 omega_d^2 / c^4 in the place of the first
 *     derivatives, times p.  P: 9 N complex128, its boundary rows not read; p: N float64; G: N complex128.
 * helm_stencil_sources_t_device:  R[s ldr + j] = coef sum_k C[8 - k][j + off_k] U[s][j + off_k] (conj != 0: conj(C)), cells outside the grid contributing nothing:
 *     (dC)^T U, or (dC)^H U, the transposed application of the nine planes of helm_velocity_planes_device / helm_buoyancy_planes_device.  The transposed plane set is
 *     not formed.  U, C, R as for helm_stencil_sources_device (note that conj conjugates the PLANES here, the columns there).  accumulate != 0: the CONJUGATE of
 *     that value is added to R instead (the columns a survey pipeline holds are the conjugates of the fields: the result joins a right-hand side where it lies).
 * helm_mass_planes_device:  dC[k][i] = m_k (d kappa_j / dc) b_j dc[j], j = i + off_k, on the interior rows, zero on the boundary rows: the mass term of
 *     helm_velocity_planes_device alone (linearisation='operator'), m the mass weights (centre, edges, corners).  dc: N float64; dC: 9 N complex128.
 * helm_mass_adjoint_device:  helm_velocity_adjoint_device for those planes, the transpose of the mass term alone.
 *
 * The same rules as above: plain fp64 in a fixed order, one writer per entry, no atomics; HELM_ERR_STATE before the first helm_assemble (the curvature); Eurus, 3-D
 * and ny > 0 handles HELM_ERR_UNSUPPORTED; null, misaligned (16 bytes; U32: 8, dExp: 4, p: 8) or overlapping pointers, nsrc < 1, a leading dimension < N and grids
 * below 3 x 3 HELM_ERR_ARG.  All device pointers; each call returns when its result is complete. */
int helm_velocity_curvature_device(helm_op *op, const void *dP, const void *dp, double w_re, double w_im, int conj, int stretch, void *dG);
int helm_stencil_sources_t_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im, int conj, int accumulate,
                                  void *dR, long long ldr);
int helm_stencil_sources_t_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ldu, const void *dC, double coef_re, double coef_im,
                                      int conj, int accumulate, void *dR, long long ldr);
int helm_mass_planes_device(helm_op *op, const void *dDc, void *dC);
int helm_mass_adjoint_device(helm_op *op, const void *dP, double w_re, double w_im, int conj, void *dG);

/* --- the mixed (c, b) second derivative of MiniZephyr (HelmBaseProblem.Hvec with parameter='joint' and resid=) --------------------------------------
 * A row is star(row_i(c_i), bn[b], Kn_k = kappa(c_j) b_j), bilinear in (row, bn) and linear in Kn: d^2 A / db^2 = 0 and along a velocity perturbation p and a buoyancy
 * perturbation beta the mixed derivative is star(p_i d row_i / dc, bn[beta], Kn_k = (d kappa_j / dc) beta_j p_j) -- the planes of helm_velocity_planes_device with
 * beta in the place of 1 / rho.
 *
 * helm_velocity_adjoint_b_device:  G[j] += w sum_{k, i} (those planes along p = e_j)_{(k, i)} P[k][i], the transpose in the velocity: helm_velocity_adjoint_device
 *     (stretch == 0: helm_mass_adjoint_device) with dB[j] read where it has 1 / rho[j].  dB: N float64 of any sign, zeros included; it is never inverted.
 * helm_mixed_adjoint_device:  G[j] += w sum_{k, i} (those planes along beta = e_j)_{(k, i)} P[k][i], the transpose in the buoyancy: the gather of
 *     helm_buoyancy_adjoint_device with the stiffness factors of row i replaced by p_i d row_i / dc and kappa_j by (d kappa_j / dc) p_j; cell j reads p at the rows
 *     around it.  dp: N float64 of any sign.  stretch == 0: the mass term alone, (d kappa_j / dc) p_j times the mass gather of P.
 *
 * conj != 0: the conjugated coefficients.  P: 9 N complex128, its boundary rows not read; G: N complex128.  The same rules as above: plain fp64 in a fixed order, one
 * writer per entry, no atomics; HELM_ERR_STATE before the first helm_assemble; Eurus, 3-D and ny > 0 handles HELM_ERR_UNSUPPORTED; null, misaligned (16 bytes; dB,
 * dp: 8) or overlapping pointers and grids below 3 x 3 HELM_ERR_ARG.  All device pointers; each call returns when its result is complete. */
int helm_velocity_adjoint_b_device(helm_op *op, const void *dP, const void *dB, double w_re, double w_im, int conj, int stretch, void *dG);
int helm_mixed_adjoint_device(helm_op *op, const void *dP, const void *dp, double w_re, double w_im, int conj, int stretch, void *dG);

/* --- the chain from (c, Q) to the complex velocity of a visco problem (HelmBaseProblem.JvecBorn / Jtvec / Hvec with parameter 'c', 'Q', 'cQ') -------------
 * A visco wrapper gives the handle of frequency f the complex velocity c~ = c (1 + lam q) (1 + i q / 2), q = 1 / Q, lam = ln(f / freqBase) / pi (0 without
 * dispersion).  With an explicit density every coefficient of MiniZephyr is holomorphic in c~, so the derivative along real (dc, dQ) is the derivative along the
 * complex perturbation dc~ = gamma dc + chi dQ, gamma = (1 + lam q)(1 + i q / 2), chi = -c~ q^2 [lam / (1 + lam q) + (i / 2) / (1 + i q / 2)].  The chain is computed
 * in the kernels from the handle's c~, the array dQ (N float64; inf allowed: gamma = 1, chi = 0) and the scalar lam.
 *
 * helm_visco_perturbation_device:   dDcz[i] = gamma_i vc[i] + chi_i vQ[i].  dVc, dVq: N float64, either may be NULL (not both); dDcz: N complex128.
 * helm_velocity_planes_z_device:    dC = V[dc~], helm_velocity_planes_device (dDb NULL) with the complex perturbation dDcz (N complex128); dC: 9 N complex128.
 *     (The mass term alone, linearisation='operator', is helm_virtual_sources_op_device with the complex weight W = -2 omega_d^2 dc~ / (c~^3 rho).)
 * helm_visco_chain_adjoint_device:  dGc[j] += gamma_j T[j], dGq[j] += chi_j T[j] (conj != 0: the conjugated chain), T the complex cell gradient of one item (what
 *     helm_velocity_adjoint_device / helm_mass_adjoint_device / helm_imaging_op_accumulate_device add into a zeroed buffer).  dGc or dGq may be NULL (not both).
 *
 * The same rules as above: plain fp64 in a fixed order, one lane and one writer per cell, no atomics; HELM_ERR_STATE before the first helm_assemble; Eurus, 3-D
 * and ny > 0 handles HELM_ERR_UNSUPPORTED; null (other than named), misaligned (16 bytes; dQ, dVc, dVq: 8) or overlapping pointers, a NaN lam and (planes) grids
 * below 3 x 3 HELM_ERR_ARG.  All device pointers; each call returns when its result is complete. */
int helm_visco_perturbation_device(helm_op *op, const void *dQ, double lam, const void *dVc, const void *dVq, void *dDcz);
int helm_velocity_planes_z_device(helm_op *op, const void *dDcz, void *dC);
int helm_visco_chain_adjoint_device(helm_op *op, const void *dQ, double lam, const void *dT, int conj, void *dGc, void *dGq);

/* --- the pseudo-Hessian diagonal of the exact derivatives (HelmBaseProblem.illumination with linearisation='full' / 'operator') ------------------
 * H[i] += alpha (dW ? W[i] : 1) sum_{s<nsrc} || (d A / d p_i) u^_s ||_2^2 for i < N, with U[s] = conj(u^_s) the stored columns (nsrc columns of ld >= N complex128,
 * or, _c64, complex64 values with the int32 column exponents dExp of helm_pack_c64_device) and d A / d p_i the derivative of the operator the handle holds:
 *     mode 0   p = c: star(d row_i / dc, bn[b], (d kappa_i / dc) b_i) -- the planes of helm_velocity_planes_device along e_i with dDb NULL
 *     mode 1   p = b: the planes of helm_buoyancy_planes_device along e_i (the caller's W carries 1 / rho^4 for the density)
 *     mode 2   p = c with the buoyancy following it: mode 0 plus dChain[i] times mode 1 (dChain: N float64, d b / d c; NULL for the other modes)
 * A unit perturbation of cell i touches the rows of the 3 x 3 block around it, and in those the lags that point back into the block: at most 33 complex
 * coefficients per cell, built in the kernel and kept in registers (the _packed entry points with dE != NULL read them from the array that
 * helm_pseudo_hessian_coefficients_device wrote for the same mode and chain: 10 N complex128 for mode 0, 33 N otherwise).  W, H: N float64; alpha >= 0.
 *
 * The fields are read once plus the rows above and below a tile; no scratch array.  Plain fp64 in a fixed order (columns in groups of four over the four waves of
 * a workgroup, the waves' sums added in wave order, one writer per cell), no atomics: the same bits on every run.  HELM_ERR_STATE before the first helm_assemble;
 * Eurus, 3-D and ny > 0 handles HELM_ERR_UNSUPPORTED; null (other than dChain, dW, dE), misaligned (U: 16, U32: 8, dExp: 4, dE: 16, the rest 8) or overlapping
 * pointers, nsrc < 1, ld < N, a negative or NaN alpha, a mode outside 0..2, a chain without mode 2 (or the reverse) and grids below 3 x 3 HELM_ERR_ARG.
 * All device pointers; each call returns when its result is complete. */
int helm_pseudo_hessian_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, int mode, const void *dChain, double alpha, const void *dW, void *dH);
int helm_pseudo_hessian_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int mode, const void *dChain, double alpha,
                                              const void *dW, void *dH);
int helm_pseudo_hessian_coefficients_device(helm_op *op, int mode, const void *dChain, void *dE);
int helm_pseudo_hessian_accumulate_packed_device(helm_op *op, const void *dU, int nsrc, long long ld, int mode, const void *dChain, const void *dE, double alpha,
                                                 const void *dW, void *dH);
int helm_pseudo_hessian_accumulate_packed_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int mode, const void *dChain,
                                                     const void *dE, double alpha, const void *dW, void *dH);

/* --- the exact diagonal of the Gauss-Newton Hessian (HelmBaseProblem.illumination with kind='gaussNewton') --------------------------------------------
 * H[i] = sum_s sum_r |g_r^T (d A / d p_i) u^_s|^2 factorises through the 3 x 3 block around i: with Gamma and Phi the Gram blocks of the receiver Green's
 * functions g_r and of the forward solves u^_s over the cells of the block it is Re tr(E_i^H Gamma_i E_i Phi_i), and two cells of a block are at most two steps
 * apart in either direction, so both are read off the autocorrelation planes at the lags of (-2..2)^2.
 *
 * helm_lag_gram_accumulate_device:  C[l][i] += sum_{s<nsrc} U[s ld + i] conj(U[s ld + i + off_l]) for the 13 lags of the half plane, l = 0..2: (0, 0..2),
 *     l = 3..7: (1, -2..2), l = 8..12: (2, -2..2) as (dz, dx), and every cell i whose partner i + off_l is inside the grid; the other entries are not touched (the
 *     other twelve lags are the conjugates, read at the shifted cell).  U: nsrc columns of ld >= N complex128 (or, _c64, complex64 values with the int32 column
 *     exponents dExp of helm_pack_c64_device); C: 13 N complex128.
 * helm_gauss_newton_diagonal_device:  H[i] += alpha (dW ? W[i] : 1) Re tr(E_i^H Gamma_i E_i Phi_i), Phi from the planes dCu and Gamma from the planes dCg (13 N
 *     complex128 each, of the stored conjugates: the coefficients are conjugated instead).  E_i by mode: 0, 1, 2 as helm_pseudo_hessian_accumulate_device (the
 *     velocity modes with the eight mass rows m_o (d kappa_i / dc) b_i in full); 3 the mass term alone; 4 the unit diagonal, H[i] += alpha W[i] Gamma[i, i] Phi[i, i].
 *     dChain: N float64 with mode 2, NULL otherwise.  W, H: N float64; alpha >= 0.
 *
 * Plain fp64 in a fixed order, one writer per entry, no atomics: the same bits on every run.  HELM_ERR_STATE before the first helm_assemble (the diagonal); Eurus,
 * 3-D and ny > 0 handles HELM_ERR_UNSUPPORTED; null (other than dChain, dW), misaligned (U, C: 16, U32: 8, dExp: 4, the rest 8) or overlapping pointers, nsrc < 1,
 * ld < N, a negative or NaN alpha, a mode outside 0..4, a chain without mode 2 (or the reverse) and grids below 3 x 3 (the diagonal) HELM_ERR_ARG.  All device
 * pointers; each call returns when its result is complete. */
int helm_lag_gram_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, void *dC);
int helm_lag_gram_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, void *dC);
int helm_gauss_newton_diagonal_device(helm_op *op, int mode, const void *dChain, const void *dW, const void *dCu, const void *dCg, double alpha, void *dH);

/* --- the per-cell 2 x 2 blocks of the joint (c, rho) Hessian (HelmBaseProblem.hessianBlocks) -----------------------------------------------------------
 * With E^c_i the derivative of the operator the handle holds with respect to the velocity of cell i at the handle's density (stretch != 0: mode 0 above; stretch 0:
 * the mass term alone, mode 3 of the diagonal) and E^b_i that with respect to its buoyancy (mode 1), the pair has a 2 x 2 Gram matrix (cc, cb, bb) under either
 * inner product of the two sections above.  Three rows of N float64, ldH >= N apart, in density units (d b / d rho = -1 / rho^2):
 *     H[0][i] += alpha cc_i,     H[ldH + i] += -alpha cb_i / rho_i^2,     H[2 ldH + i] += alpha bb_i / rho_i^4
 *
 * helm_gauss_newton_blocks_device:    xy_i = Re tr(E^x_i^H Gamma_i E^y_i Phi_i), Phi from dCu and Gamma from dCg as helm_gauss_newton_diagonal_device takes them.
 * helm_pseudo_hessian_blocks_device:  xy_i = sum_{s<nsrc} Re <E^x_i u^_s, E^y_i u^_s> over the rows of the 3 x 3 block, U as helm_pseudo_hessian_accumulate_device
 *     takes it (_c64: the complex64 store with its column exponents).
 * Rows 0 and 2 are what the diagonal entry points give for modes 0 / 3 and 1 (with W = 1 / rho^4); the middle row has either sign and xy^2 <= xx yy.
 *
 * Plain fp64 in a fixed order, one writer per entry, no atomics, no scratch: the same bits on every run.  HELM_ERR_STATE before the first helm_assemble; Eurus, 3-D
 * and ny > 0 handles HELM_ERR_UNSUPPORTED; null, misaligned (U, C: 16, U32: 8, dExp: 4, H: 8) or overlapping pointers (H counts 2 ldH + N entries), nsrc < 1,
 * ld < N, ldH < N, a negative or NaN alpha, a stretch outside 0..1 and grids below 3 x 3 HELM_ERR_ARG.  All device pointers; each call returns when its result
 * is complete. */
int helm_gauss_newton_blocks_device(helm_op *op, int stretch, const void *dCu, const void *dCg, double alpha, void *dH, long long ldH);
int helm_pseudo_hessian_blocks_device(helm_op *op, const void *dU, int nsrc, long long ld, int stretch, double alpha, void *dH, long long ldH);
int helm_pseudo_hessian_blocks_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, int stretch, double alpha, void *dH, long long ldH);

/* --- device-resident callers: sparse sources in, receiver samples out ---------------------------------- */
/* Dense right-hand sides from the COO triplets of the reference's sparse source matrix (survey.py:162-169,
 * source.py:213-317): R (nrhs x rows, zeroed by the call), R[col[k]][row[k]] = val[k]; no duplicate entries.
 * row: int64, col: int32, val: complex128, all device pointers. */
int helm_rhs_from_coo_device(helm_op *op, const void *d_row, const void *d_col, const void *d_val, long long nnz,
                             void *dR, int nrhs, long long rows);
/* the same with the layout of R chosen by `flags` (HELM_RHS_NODE_MAJOR: R[row[k]*nrhs + col[k]]) */
int helm_rhs_from_coo_device_layout(helm_op *op, const void *d_row, const void *d_col, const void *d_val, long long nnz,
                                    void *dR, int nrhs, long long rows, int flags);

/* Declared support of the next solve's right-hand sides (the reference's sources are scipy-sparse matrices, survey.py:86-89,162-188: where they
 * are nonzero is part of the input).  d_bits: one byte per row on the device, bit b = block b of 64 right-hand sides may be nonzero in that row; the
 * caller guarantees zeros elsewhere.  One shot: applies to the next helm_solve_device on this handle (same rows / nrhs, node-major layout), then
 * forgotten; NULL clears it.  HELM_ND_SUPPORT_CHECK=1 verifies the guarantee and fails the solve if it does not hold. */
int helm_set_rhs_support(helm_op *op, const void *d_bits, long long rows, int nrhs);
/* d_bits ((rows + 3) / 4 * 4 bytes on the device) from the triplets of a sparse right-hand-side matrix (device arrays, as for
 * helm_rhs_from_coo_device_layout) */
int helm_rhs_support_from_coo(helm_op *op, const void *d_row, const void *d_col, long long nnz, void *d_bits, long long rows, int nrhs);
/* Receiver sampling data = R u (survey.py:152-160): out[r][s] = sum_k val[k] * U[s][col[k]] over the entries k of CSR
 * row r (rowptr, col: int64; val: complex128; U: nsrc x ld; out: nrec x nsrc complex128; device pointers). */
int helm_sample_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                       const void *d_val, int nrec, void *d_out);
/* The same into an accumulator: out = beta * out + alpha * R u (complex alpha, beta; arguments as for helm_sample_device).  Sampling is linear, so the
 * data of a sum of wavefields (the cross-line wavenumbers of MiniZephyr25D, minizephyr.py:435-460) are summed here and the summed field is never formed.
 * beta == 0: out is not read (it may be uninitialised). */
int helm_sample_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                                  const void *d_val, int nrec, double alpha_re, double alpha_im, double beta_re, double beta_im, void *d_out);
/* The same with a row stride per source: source s samples CSR row r + s * row_stride.  row_stride == 0 is helm_sample_accumulate_device (one receiver
 * array for every source, bit for bit); row_stride >= nrec serves a receiver array that moves with the source (geom mode 'relative', survey.py:43-47,114-125):
 * the per-source matrices stacked into one CSR, row s * row_stride + r.  A batch of sources c0 .. c1-1 is d_rowptr + c0 * row_stride with nsrc = c1 - c0.
 * out: nrec x nsrc as above.  Other values of row_stride: HELM_ERR_ARG. */
int helm_sample_rows_device(helm_op *op, const void *dU, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                            const void *d_val, int nrec, long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im,
                            void *d_out);
/* Back-sources of a moving receiver array from the residual samples of one frequency (survey.py:171-188): R (nsrc x rows, zeroed by the call),
 * R[s - src0][cell] = sum_r R_s[r][cell] * resid[r][s - src0] for the sources src0 .. src0 + nsrc - 1.  The sum is a gather over a plan sorted by
 * (source, cell): touched pair t has source d_tsrc[t] (int32, absolute), cell d_tcell[t] (int64) and the entries d_tptr[t] .. d_tptr[t+1] (int64) of
 * d_trec (int32 receiver) and d_tval (complex128 weight), ordered by receiver; one thread sums a pair in that order, so repeated calls give the same bits.
 * d_resid: nrec x ld_resid complex128 (ld_resid >= nsrc).  A batch of sources is a contiguous range of pairs: offset d_tptr, d_tsrc and d_tcell by the
 * batch's first pair and leave d_trec / d_tval at their base.  ntouch == 0 gives all zeros.  The plan is trusted (cells < rows, receivers < nrec, sources
 * within the batch): validate it where it is built.  All device pointers; returns when R is complete. */
int helm_rhs_from_samples_device(helm_op *op, const void *d_resid, long long ld_resid, int nrec, int nsrc, int src0, const void *d_tptr,
                                 const void *d_tsrc, const void *d_tcell, const void *d_trec, const void *d_tval, long long ntouch, void *dR,
                                 long long rows);
/* Y[i] = beta * Y[i] + alpha * X[i], i < n: complex128 device arrays (16-byte aligned, X != Y, not overlapping), on the handle's stream; returns when Y is
 * complete.  The sum over sub-problems of a composite operator (MiniZephyr25D: the last term carries the composite's scaleTerm in alpha and beta, so there
 * is no scaling pass).  beta == 0: Y is not read (it may be uninitialised). */
int helm_axpby_device(helm_op *op, double alpha_re, double alpha_im, const void *dX, double beta_re, double beta_im, void *dY, long long n);

/* --- forward wavefields kept as complex64 with one power-of-two scale per column ---------------------- */
/* The optional half-size store of DeviceFields (zephyr_amd/fieldstore.py, fieldsDtype='complex64').  Column s of dU (nsrc columns of ld complex128 values,
 * each contiguous, 16-byte aligned) is written to dOut as complex64 values (float)(x * 2^-e_s), rounded to nearest, and e_s to dExp (nsrc int32):
 * e_s is the binary exponent of m_s = max_i max(|Re x_i|, |Im x_i|), 2^e_s <= m_s < 2^(e_s+1), clamped to +-1021; 0 for a zero column.  A consumer reads
 * (double)x^ * 2^e_s.  Per component |x^ - x| <= 2^-24 |x| where |x| >= 2^(e_s-126), and <= 2^(e_s-126) below.  The column maximum is reduced in a fixed
 * order without atomics: the same bits on every run.  All device pointers; returns when dOut and dExp are complete. */
int helm_pack_c64_device(helm_op *op, const void *dU, int nsrc, long long ld, void *dOut, void *dExp);
/* helm_imaging_accumulate_device with the forward field read from that store: G[i] += scaler[i] * sum_s (UF32[s][i] * 2^dExp[s]) * UB[s][i].  dUB, dScaler
 * and dG are complex128 as there; columns are N = helm_num_points(op) apart. */
int helm_imaging_accumulate_c64_device(helm_op *op, const void *dUF32, const void *dExp, const void *dUB, int nsrc, const void *dScaler, void *dG);
/* helm_energy_accumulate_device with U read from that store (dU32: nsrc columns of ld complex64 values, 8-byte aligned; dExp: their exponents): every
 * component is (double)x^ * 2^e_s, exact, before it is squared, so the result is that of the complex128 kernel on the unpacked values, under the same bound. */
int helm_energy_accumulate_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, double alpha, const void *dW, void *dE);
/* helm_sample_rows_device with the wavefields read from that store (dU32: nsrc columns of ld complex64 values, dExp: their exponents): the other arguments,
 * the row stride and the result are those of helm_sample_rows_device. */
int helm_sample_rows_c64_device(helm_op *op, const void *dU32, const void *dExp, int nsrc, long long ld, const void *d_rowptr, const void *d_col,
                                const void *d_val, int nrec, long long row_stride, double alpha_re, double alpha_im, double beta_re, double beta_im,
                                void *d_out);

/* The data misfit on the sample panels of a work item (zephyr_amd/misfit.py states the functional).  A panel is [nrec][ld] with the item's ncol <= ld columns
 * adjacent, sample [r][j] at r * ld + j, as the sampling entry points write it: dP the samples p, dD dobs, both complex128 and 16-byte aligned, dW2 the
 * weights w2 >= 0 as doubles (NULL: ones).  A sample with w2 == 0 is selected away: it may hold NaN in dD.  Every per-column sum is one lane walking
 * r = 0, 1, ... : a column has the same bits alone, anywhere in a batch and on every run.  No atomics.  Each call returns when its outputs are complete.
 * kind: 0 'l2', 1 'huber' (par0 = threshold > 0), 2 'hybrid' (par0 = epsilon > 0), 3 'logarithmic' (par0 = amplitude, par1 = phase weight, both >= 0; dobs
 * and the scaled samples must not be zero where w2 > 0).
 *
 * dMom[j] = (Re a_j, Im a_j, b_j), a_j = sum_r w2 conj(p) d, b_j = sum_r w2 |p|^2: 3 ncol doubles.  The source estimate of a group is sum a / sum b. */
int helm_misfit_moments_device(helm_op *op, const void *dP, const void *dD, const void *dW2, long long ld, int nrec, int ncol, void *dMom);
/* At the source factors dS[j] (ncol complex128), q = s p: dPsi = grad_q phi ([nrec][ld] complex128, 0 where w2 == 0; not one of the input panels) and
 * dOut[j] = (phi_j, Re c_j, Im c_j), c_j = sum_r conj(psi) p: 3 ncol doubles. */
int helm_misfit_terms_device(helm_op *op, int kind, double par0, double par1, const void *dP, const void *dD, const void *dW2, const void *dS, long long ld,
                             int nrec, int ncol, void *dPsi, void *dOut);
/* The adjoint source dV[r][j] = phase_r (conj(s_j) psi + w2 (e_j d - f_j p)), 0 where w2 == 0.  dCoef[j] = (Re e_j, Im e_j, f_j), e = c / b and
 * f = 2 Re(c s) / b of the column's group (3 ncol doubles), or NULL: a given source, the first term alone.  dPhase: nrec complex128 factors per receiver
 * (conj(t_r) / t_r of complex receiver terms, which makes the transposed sampling of the back-sources act as its conjugate transpose), or NULL.  dV may be dP:
 * the adjoint source then replaces the samples.  dGn: NULL, or a [nrec][ld] panel of doubles that receives the Gauss-Newton weights at fixed s (|s|^2 w2 for
 * 'l2'; 'logarithmic' needs par0 == par1, HELM_ERR_UNSUPPORTED otherwise). */
int helm_misfit_adjoint_device(helm_op *op, int kind, double par0, double par1, const void *dPsi, const void *dS, const void *dCoef, const void *dP,
                               const void *dD, const void *dW2, const void *dPhase, long long ld, int nrec, int ncol, void *dV, void *dGn);

/* Device buffers are recycled by size class; a class holds as many as the busiest moment so far needed.  How many operators a pipelined job has alive at its
 * busiest is a matter of thread timing, so a job that got by with three buffers of a class in its first items may ask for a fourth later -- a hipMalloc of GBs
 * beside running kernels, 0.5 ms on one box and 120 ms on another.  This call tops every class of 64 MB .. 16 GB whose busiest moment used ALL its buffers up to
 * `spare` more than that (idle ones; classes that kept one unused are left alone).  The library does it by itself when the last operator of a device is destroyed
 * (HELM_POOL_SPARE buffers, default 2; HELM_POOL_SPARE_AUTO=0: only on this call) -- a caller that times the region ending with that destroy calls it itself, before.
 * Counterpart of the reference's pool keeping its workers alive between products (distributors.py:80-96). */
int helm_pool_spares(int device, int spare);
/* Free the scratch memory the library keeps between calls (the direct path's shared workspace, tens of GB at
 * 1024^2 x 256 right-hand sides).  HELM_ERR_STATE while a solve is using it. */
int helm_trim(void);
/* Only the pinned host buffers the library holds idle (results of helm_solve / helm_solve_coo and helm_host_alloc memory that was
 * handed back): the idle pool is capped by bytes (HELM_HOSTPOOL_GB, default a quarter of the host's memory, at most 96 GB); helm_trim
 * calls this too.  Counterpart of dropping the reference's result arrays (discretization.py:101-103 returns fresh numpy arrays). */
int helm_host_trim(void);
/* (diagnostic) number of scratch slots of `device` that hold a buffer of at least `bytes` bytes -- the direct path's shared workspace is
 * kept PER DEVICE, HELM_WS_SLOTS (default 3) slots each, so that every GPU of an in-process multi-GPU job (distributors.py:80-96: one
 * address space per worker in the reference) finds its own; device < 0: the number of slots per device. */
int helm_debug_ws_slots(int device, long long bytes);
/* (diagnostic) number of elimination-tree plans the per-device cache holds for `device` (HELM_ND_PLANS, default 6 per device) */
int helm_debug_plan_cache(int device);
/* (diagnostic, no GPU needed) the scratch-slot table exercised with `ndev` logical devices and host memory: every device books `concurrent`
 * slots of `bytes`, then that many leases are taken on every device at once.  0: every lease was a booked slot of its own device and none
 * allocated; < 0: which check failed. */
int helm_debug_ws_selftest(int ndev, int concurrent, long long bytes);
/* (diagnostic) allocator calls of the library that reached the driver and took more than a millisecond since the last reset (what
 * HELM_ALLOC_TRACE=1 prints): a job that booked its memory with helm_reserve must issue none. */
int helm_debug_alloc_stats(int reset, long long *slow_calls, double *worst_ms);

/* Resolve every kernel of the library on `device` now: the HIP runtime looks a kernel up in its code object and builds its dispatch record the first
 * time it is launched on a device (1.8 ms of host time for the nine kernels of one tree level in a cold process), and a job meets some kernels only at
 * some frequencies -- pivoted leaves, the pivoted-LU treatment of ill-conditioned fronts, refinement widths.  Nothing is launched.  Called by the
 * library itself when the first operator of a device is created (HELM_WARM=0: not); returns the number of kernels the library holds (> 0) or
 * HELM_ERR_DEVICE.  Counterpart of starting the reference's worker pool before the first product (distributors.py:80-96). */
int helm_warm(int device);
/* (diagnostic) what the library made the HIP runtime create since the last reset: device / pinned allocations that reached the driver (count, bytes,
 * host milliseconds), events, streams, kernels launched for the first time in the process (count, host milliseconds of those launch calls); and, not
 * reset, the kernels registered / resolved by helm_warm and its milliseconds.  A job whose memory was booked shows zeros across its timed region. */
typedef struct helm_runtime_stats {
    long long dev_allocs;  double dev_alloc_bytes;  double dev_alloc_ms;
    long long host_allocs; double host_alloc_bytes; double host_alloc_ms;
    long long events_created, streams_created;
    long long first_launches; double first_launch_ms;
    long long kernels_registered, kernels_resolved; double warm_ms;
    long long dev_frees; double dev_free_ms;          /* hipFree calls (each waits for every stream of the device) */
    long long sync_calls; double sync_ms;             /* host-side waits of the library (stream / event / device synchronisations, blocking copies) */
    long long slow_syncs; double worst_sync_ms;       /* those of at least 10 ms (HELM_SYNC_TRACE=<ms> names their call sites on stderr) */
} helm_runtime_stats;
int helm_debug_runtime_stats(int reset, helm_runtime_stats *out);
/* (diagnostic) start != 0: a thread of the library starts reading the clock in a loop; start == 0: it stops, and the longest interval between two of its readings
 * (and how many exceeded 5 ms) come back.  A stall every thread of the process sits through shows here; a stall of the GPU or of the HIP runtime does not. */
int helm_debug_stall_watch(int start, double *worst_gap_ms, long long *gaps_over_5ms);

/* --- tuning ------------------------------------------------------------------------------
 * The options of the library that are real options (round 5: the seventy-odd HELM_* environment switches of rounds 1-4 were the tuning
 * interface; the measured-and-rejected ones are gone, HISTORY.md has what they measured).  Every field can still be given through the
 * environment variable named beside it -- looked at when an API call that starts work is entered (create, assemble, prefactor, solve, apply,
 * get_tuning), by the calling thread and nowhere below it, so a test may flip one BETWEEN two calls, never during one -- and helm_set_tuning
 * replaces the lot for the process (NULL: back to defaults + environment): while such a structure is in force EVERY field follows it and not the
 * environment, mg3_coarse, mg3_nd_leaf, mg3_bt_twist and mg3_beta (environment-only switches before they joined the structure) included.
 * Values are clamped to the ranges the code can run with whichever way they arrive (nd_leaf >= 2, nd_plans >= 1, nd_ws_gb > 0, nd_stable_safety >= 1, ws_slots 1..4, pf_prio -1/0/1, mg3_omega in (0, 2], mg3_coarse 0..2,
 * mg3_nd_leaf >= 2, mg3_beta >= 0 and finite).  Process-wide, like the reference's module-level defaults
 * (distributors.py:28-34); not per handle.  Diagnostics that change no result and no speed stay environment-only: HELM_ND_TRACE,
 * HELM_ND_DEBUG, HELM_GEMM_LOG, HELM_MG3_TRACE, HELM_ALLOC_TRACE, and the test hooks behind HELM_TESTING=1 (HELM_ND_POISON,
 * HELM_ND_SUPPORT_CHECK, HELM_LEAF_DBG, HELM_ND_INJECT_*, HELM_MG3_DEPTH_FORCE_DEEPER, HELM_MG3_DEPTH_SETUP_SCALE, HELM_MG3_KEEP_CAP). */
typedef struct helm_tuning {
    /* 2-D sparse direct path */
    int    nd_leaf;            /* HELM_ND_LEAF           8     regions with both sides <= this are eliminated whole (leaf fronts) */
    double nd_ws_gb;           /* HELM_ND_WS_GB          32    cap on the per-batch scratch of a direct solve; the batch is halved until it fits */
    int    nd_sparse_rhs;      /* HELM_ND_SPARSE_RHS     1     forward pass skips fronts that see nothing but zeros (point sources) */
    int    nd_stable;          /* HELM_ND_STABLE         1     ill-conditioned fronts are re-eliminated with a pivoted LU */
    double nd_stable_thr;      /* HELM_ND_STABLE_THR     0     fixed condition-estimate threshold; 0: rtol / (nd_stable_safety * eps) */
    double nd_stable_safety;   /* HELM_ND_STABLE_SAFETY  8 */
    int    nd_fused_leaf;      /* HELM_ND_FUSEDLEAF      1     leaf level of the factorisation in one kernel */
    int    nd_fused_leaf_min;  /* HELM_ND_FUSEDLEAF_MIN  2048  fewest leaves of a level for which it pays */
    int    nd_gjstep;          /* HELM_ND_GJSTEP         1     one launch per block step of the blocked Gauss-Jordan inversion */
    int    nd_gjstep_min;      /* HELM_ND_GJSTEP_MIN     128   smallest front inverted that way (r5: 512 -> 128, headline +1.3 %) */
    int    nd_overlap;         /* HELM_ND_OVERLAP_NM     1     first forward pass beside the factorisation (2: also while profiling) */
    int    nd_xcd_map;         /* HELM_ND_XCDMAP         2     workgroup ids regrouped so that a front's tiles share an XCD (0 off, 1 column tiles only) */
    int    nd_plans;           /* HELM_ND_PLANS          6     elimination-tree plans cached per device */
    int    nd_direct_out;      /* HELM_ND_DIRECT_OUT     1     back substitution writes the caller's wavefield array itself (node-major calls) */
    int    nd_many;            /* HELM_ND_MANY           1     helm_prefactor_many factors its operators in the same launches (0: one after the other) */
    int    nd_leaf_idle;       /* HELM_ND_LEAF_IDLE      1     sparse right-hand sides: idle leaf blocks and small separator fronts of the back substitution go to kernels that issue all their loads at once; the forward pass deals its separator levels from lists of active (front, block) pairs */
    /* dispatch / memory */
    int    auto_direct;        /* HELM_AUTO_DIRECT       1     HELM_AUTO takes the direct path in 2-D */
    int    auto_mg3;           /* HELM_AUTO_MG3          1     HELM_AUTO takes the multigrid-preconditioned path in 3-D */
    int    prof_ext;           /* HELM_PROF_EXT          1     profiled launches carry their own events (0: event records around them) */
    int    ws_slots;           /* HELM_WS_SLOTS          3     shared scratch slots per device */
    int    pf_prio;            /* HELM_PF_PRIO           1     stream priority of helm_prefactor (1 high, 0 normal, -1 low) */
    /* 3-D multigrid */
    int    mg3_keep;           /* HELM_MG3_KEEP          1     layer-preserving hierarchy (2: fail instead of retreating to the standard cycle) */
    int    mg3_keep_levels;    /* HELM_MG3_KEEP_LEVELS   -1    coarsenings above the directly solved level; -1: chosen by the depth model */
    int    mg3_galerkin;       /* HELM_MG3_GALERKIN      1     Galerkin operator on the directly solved level */
    int    mg3_depth_model;    /* HELM_MG3_DEPTH_MODEL   1     trade set-up seconds against booked iteration counts */
    int    mg3_bt_f32;         /* HELM_MG3_BT_F32        1     single-precision plane inverses of the block-tridiagonal coarse solve */
    int    mg3_otf;            /* HELM_MG3_OTF           1     27-point apply rebuilds its coefficients from c, rho and the PML profiles (1: from 4 right-hand sides per workgroup up, 2: always) */
    int    mg3_f32;            /* HELM_MG3_F32           1     the layer-preserving cycle keeps the work vectors of its finest level in complex64 (input, result and every coarser level stay complex128) */
    double mg3_omega;          /* HELM_MG3_OMEGA         0.9   Jacobi damping of the smoother */
    int    mg3_coarse;         /* HELM_MG3_COARSE        0     direct solver of the last layer-preserving level: 0 the cheaper one, 1 column dissection (environment: nd), 2 plane-by-plane elimination (bt) */
    int    mg3_nd_leaf;        /* HELM_MG3_ND_LEAF       2     leaf size of that column dissection */
    int    mg3_bt_twist;       /* HELM_MG3_BT_TWIST      1     the plane-by-plane elimination runs from both ends and meets in the middle (0: one chain) */
    double mg3_beta;           /* HELM_MG3_BETA          0     complex shift of the preconditioner; 0: min(8, 0.6 (ppw / 10)^2) for the standard cycle, 0.1 for the layer-preserving one */
    /* host-side waits */
    double sync_spin_ms;       /* HELM_SYNC_SPIN_MS      0     a wait of the library polls for this long before it blocks on the runtime's interrupt (saves the 20-50 us wake-up of each
                                                               wait; costs a CPU per waiting thread -- leave it off under a container CPU quota, where a spinning thread spends the budget the
                                                               launching threads need) */
    int    sync_sleep_us;      /* HELM_SYNC_SLEEP_US     0     > 0: a wait of the library polls with a sleep of this many microseconds between two looks instead of the runtime's wait, which keeps a
                                                               CPU busy while it lasts (2.5 CPUs per process in the pipelined bench job): for several processes under a container CPU quota */
    /* 2-D sparse direct path, continued (new fields join at the end: the layout of the earlier ones stays) */
    int    nd_fused_sep;       /* HELM_ND_FUSEDSEP       1     separator levels of at most 16 unknowns per front (s + m <= 128) are factored in one kernel per level */
    int    nd_fused_sep_min;   /* HELM_ND_FUSEDSEP_MIN   512   fewest fronts of a level for which it pays (measured) */
} helm_tuning;
int helm_get_tuning(helm_tuning *out);          /* the values in force now (environment applied) */
int helm_set_tuning(const helm_tuning *t);      /* NULL: defaults + environment again */

/* --- diagnostics of the direct solver ---------------------------------------------------- */
/* Elimination-tree plan of an (nz, nx) grid (host only, no GPU needed).  out == NULL: returns the number of fronts;
 * else writes 12 ints per front in processing order {z0, z1, x0, x1, cut, pos, s, m, kid0, kid1, smax, mmax}. */
int helm_direct_plan(int nz, int nx, int leaf, int *out, int cap);
/* cells (z*nx + x) of front `node` in local order [separator | ring]; returns s + m, or < 0 if the closed-form
 * index maps disagree with each other */
int helm_direct_plan_front(int nz, int nx, int leaf, int node, long long *cells, int cap);
/* dense kernels on host data (row-major complex128, batch contiguous): C = beta C + alpha A B; in-place inverse */
int helm_debug_zgemm(int device, int M, int N, int K, const double *alpha, const double *A, const double *B,
                     const double *beta, double *C, int batch);
int helm_debug_inverse(int device, int n, double *A, int batch);
/* average milliseconds per launch of one strided-batched GEMM shape (random operands, `reps` timed launches); variant < 16: the tile the
 * library would choose, 16 (t + 1): tile configuration t (0 64x64 ... 7 16x64) forced */
int helm_debug_zgemm_bench(int device, int M, int N, int K, int batch, int variant, int reps, double *ms_out);
/* (test hook, host only, no GPU) What a product of this shape would be launched as, computed by the code the launch itself runs.  nf_div: the number of
 * frequencies the batch is shared between (1: none; the choice is made for batch / nf_div).  force_tile: -1 none, 0-8 that tile (8 with at most 16 columns, as in production); force_slab: 0 none, 8 / 16 (16
 * exists for tiles 6 and 7 only).  have_handle: the call carries a handle (split over the inner dimension keeps its scratch there).  mode: 0 dense operands,
 * HELM_ZG_TABLE row-table operands, HELM_ZG_MASKS dense operands with masks, + HELM_ZG_TM64 one row tile per matrix.
 * report[0] tile 0-8, [1] K slab 8 / 16 (16: latency mode), [2] 1: the 16 MT + 1-row tile (XR: 49 x 64 with the slab of 8; [0] is then the tile the shape would have had without it), [3] split factor of the inner dimension (0: none), [4] its chunk. */
#define HELM_ZG_TABLE 1
#define HELM_ZG_MASKS 2
#define HELM_ZG_TM64  4
int helm_debug_zgemm_choice(int M, int N, int K, int batch, int nf_div, int force_tile, int force_slab, int have_handle, int mode, int report[5]);
/* (test hook) One product C = beta C + alpha A B on host data with everything the direct solver varies.  Complex operands are (re, im) pairs of doubles and every
 * length below counts complex elements.  Buffers the kernel must leave alone (padding, masked blocks, rows without an output row, C when beta == 0) come back as
 * they went in.  Malformed input is refused with HELM_ERR_ARG before a device is touched. */
typedef struct helm_zgemm_ex {
    int device, M, N, K, batch;
    int lda, ldb, ldc;                   /* leading dimensions of the dense operands (elements) */
    long long sa, sb, sc;                /* batch strides; 0 allowed for A and B */
    double alpha[2], beta[2];
    const double *A; long long a_len;
    double *B; long long b_len;          /* dense B (NULL with tabB); written only when c_is_b */
    double *C; long long c_len;          /* dense C, in / out (NULL with tabCo or c_is_b) */
    int force_tile, force_slab;          /* as in helm_debug_zgemm_choice */
    int xcd_map;                         /* -1: helm_tuning.nd_xcd_map; 0, 1, 2: that value for this call */
    int ntc;                             /* 1: nontemporal stores of C */
    int zr0, zr1, zc0, zc1, sk0, sk1;    /* beta masks (rows / columns of C taken as zero) and the diagonal block that is neither read nor written */
    int tm64, c_is_b;                    /* one row tile per matrix (M <= 64); c_is_b: C overwrites B (ldc = ldb, sc = sb; B comes back) */
    /* row-table mode: any of the three tables given (host ints, widened to the library's int4 entries; a negative entry: zero row of B / C not read / row not stored).
     * Item z uses entries [z tab_stride + off, ...): K of tabB, M of tabCi and tabCo.  The arenas are arena_rows x ldx, row-major. */
    const int *tabB, *tabCi, *tabCo; long long tab_len;
    int tab_stride, offB, offCi, offCo;
    int ldx; long long arena_rows;
    const double *Bx, *Bx2, *Cix;        /* Bx2 (rows k < k2 of B; NULL: Bx); Cix may be the same host pointer as Bx or Cox: then it is the same device arena */
    double *Cox, *Cox2;                  /* in / out; Cox may be the same host pointer as Bx */
    int k2, cj_out; double oscale[2];
    int *act;                            /* NULL, or batch x ceil(N / 64) ints: zeroed, handed to the launch as the sparse-right-hand-side flags, returned */
    int report[5];                       /* out: as helm_debug_zgemm_choice, for the launch that was made */
} helm_zgemm_ex;
int helm_debug_zgemm_ex(helm_zgemm_ex *p);
/* (test hook) One stage of the node-major plumbing around the direct solver's passes (zephyr_amd/csrc/nd_resid.hip) on host data, through the launchers the
 * solver itself calls: the lane / row-group choice, the loop over chunks of 256 columns, the offsets of the partial sums and their reduction are the code under
 * test.  Complex operands are (re, im) pairs of doubles and every length counts complex elements.  The handle is a temporary one for an (nz, nx) grid.
 * Everything a stage may write is copied back whole (padding included), so the caller can see what was left alone.  Malformed input is refused with
 * HELM_ERR_ARG before a device is touched.  The buffers by stage:
 *   RESID          r = q' - A x on nz * nx cells with the nine planes given (not assembled): Xin[cell * ldin + j], Q[cell * ldq + map(j)], j < ncol; qmap (ncol
 *                  entries below ldq, distinct when r is stored) or NULL; store: r to Rout (same indexing as Q; NULL: over Q); Uout[cell * ldu + j] =
 *                  conj(oscale x); qmask: one byte per cell, bit b = block b of 64 columns may hold a nonzero (not with qmap); xin_is_u: Xin holds
 *                  u = conj(oscale x) and q' = oscale q.  Out: rr[ncol] = ||r||^2, qq[ncol] = ||q'||^2 when qnorm, reduced as true_residual_norms
 *                  (solve_direct.hip) does; report = {lanes, row groups, workgroups, launches, tiles}.
 *   PREP           Rout[i * ncol + r] = oscale * Xin[r * rhs_ld + row_off + i] - Q[r * N + i] (Q: the `sub` operand, NULL for none) for ncol right-hand
 *                  sides of N rows; qq[ncol] = ||.||^2; report[2] = workgroups along the rows, [4] = tiles of 32 rows.
 *   PACK           Rout[cell * ncol + j] = Xin[cell * ldin + qmap[j]], N cells, ncol = k columns
 *   SCATTER_ADD    Q[cell * ldq + qmap[j]] += Xin[cell * ncol + j] (qmap distinct)
 *   RECOVER_X      Rout[i] = conj(Xin[i]) / oscale, N * ncol elements
 *   TRANSPOSE_OUT  Xin (N x ncol) -> Rout (ncol x N), conjugated when conj
 *   TRANSPOSE      the same through nd_transpose (the branch goes by N > ncol)
 * nblk_cap (RESID, PREP): partial sums per column the launch may use; 0: what the solver passes, max(2 helm_apply_num_blocks, helm_vec_num_blocks). */
#define HELM_NM_RESID         0
#define HELM_NM_PREP          1
#define HELM_NM_PACK          2
#define HELM_NM_SCATTER_ADD   3
#define HELM_NM_RECOVER_X     4
#define HELM_NM_TRANSPOSE_OUT 5
#define HELM_NM_TRANSPOSE     6
typedef struct helm_nm_stage {
    int device, stage, nz, nx;
    long long N;                         /* rows of every stage but RESID (which has nz * nx) */
    int ncol, nblk_cap;
    const double *planes; long long planes_len;
    const double *Xin; long long xin_len; int ldin;
    double *Q; long long q_len; int ldq;
    const int *qmap;
    int store, qnorm, xin_is_u, conj;
    double *Rout; long long rout_len;
    double *Uout; long long uout_len; int ldu;
    double oscale[2];                    /* RESID, RECOVER_X: oscale; PREP: premul */
    const unsigned char *qmask;
    long long rhs_ld, row_off;           /* PREP */
    double *rr, *qq;                     /* out, ncol doubles each */
    int report[5];                       /* out */
} helm_nm_stage;
int helm_debug_nm_stage(helm_nm_stage *p);
/* (test hook) One stage of the 2-D multigrid preconditioner (zephyr_amd/csrc/mg.hip) on host data, through the kernels and with the launch shapes vcycle /
 * apply_typed use: grid-stride launches of vblocks(N) x nrhs workgroups of 256 lanes, the dense coarse solve on ceil(nc / 256) x nrhs, the line solve on
 * 4 W x nrhs waves.  Complex operands are (re, im) pairs of doubles and every length counts complex elements.  Vectors are [nrhs][N], planes [9][N] in the
 * order of the assembled operator.  `active`: NULL or one byte per column; a column whose byte is 0 is handed to the kernels as a stopped right-hand side
 * (RhsScal.status), which they must leave alone.  Every output goes up as the caller filled it and comes back whole, so that what a stage leaves alone can
 * be seen.  Malformed input is refused with HELM_ERR_ARG before a device is touched.
 * Free-standing stages (no handle; device, nz, nx, nrhs from the structure):
 *   JAC0          y = omega_j m (.) x, m = dinv [N]                                             leaves alone: inactive columns
 *   AXPY1         y += x                                                                        inactive columns
 *   RESTRICT      y [nrhs][nzc nxc] = full weighting of x [nrhs][nz nx], nzc = (nz + 1) / 2     inactive columns
 *   PROLONG_ADD   y [nrhs][nz nx] += bilinear prolongation of x [nrhs][nzc nxc]                  inactive columns
 *   COARSE_DENSE  y = m^T x, m = invT [nc][nc] (the inverse stored transposed), nz = nc, nx = 1  inactive columns
 *   LINE_FACTOR   m = nine planes; zl[0..2] = m, cp, af of the 2 W z-lines [2 W][nz], xl[0..2] of the 2 W x-lines [2 W][nx - 2 W]; needs 2 W + 2 <= nz, nx
 *   LINE_SOLVE    k_line_factor, then y += wstrip T^-1 r on every strip line (zl / xl as LINE_FACTOR, or NULL).  Leaves alone: inactive columns and every
 *                 element of y outside the lines.  r is in / out and what it holds afterwards is unspecified (the forward sweep stages its result in it).
 * Hierarchy stages (op: a 2-D handle assembled at a frequency; mg_setup(op, nrhs) runs first and the hierarchy stays with the handle):
 *   LEVELS        out: nlevels, lev_* per level, W, sweeps, nu1, nu2, fdepth, omega_j, wstrip, beta, tau (shifted), cpml (weak), nc, ntiles and up to
 *                 tiles_cap entries of the tile list in tiles
 *   PLANES        level >= 0: y = the nine planes of that level [9 N_l], r = its dinv [N_l]; level == -1: y = the strip operator's planes, zl / xl its six
 *                 line-factor arrays (HELM_ERR_STATE when the strip is off); cinvT, when given: the transposed dense inverse [nc][nc]
 *   STRIP_RESID   y = x - A_strip r on the points of the listed tiles (x = in, r = out of one sweep; y stands for strip_r).  Leaves alone: other points,
 *                 inactive columns.  The handle's strip_r is zero again afterwards.
 *   CYCLE         y = vcycle(level, x) with fmode; x, y [nrhs][N_level].  Leaves alone: inactive columns
 *   APPLY         y = mg_apply(x), the whole M^-1.  Leaves alone: inactive columns
 *   nu1, nu2, fdepth, sweeps: -1 the solver's own, else that value for this call only (CYCLE, APPLY; sweeps > 0 with the strip off: HELM_ERR_STATE). */
#define HELM_MG_JAC0          0
#define HELM_MG_AXPY1         1
#define HELM_MG_RESTRICT      2
#define HELM_MG_PROLONG_ADD   3
#define HELM_MG_COARSE_DENSE  4
#define HELM_MG_LINE_FACTOR   5
#define HELM_MG_LINE_SOLVE    6
#define HELM_MG_LEVELS        7
#define HELM_MG_PLANES        8
#define HELM_MG_STRIP_RESID   9
#define HELM_MG_CYCLE         10
#define HELM_MG_APPLY         11
#define HELM_MG_MAX_LEVELS    16
typedef struct helm_mg_stage {
    int device, stage, nz, nx, nrhs, W;
    helm_op *op;                         /* hierarchy stages */
    double omega_j, wstrip;
    const unsigned char *active;
    const double *x; long long x_len;    /* the vector a stage reads */
    double *y; long long y_len;          /* in / out */
    const double *m; long long m_len;    /* dinv, invT or the nine planes */
    double *r; long long r_len;          /* LINE_SOLVE: residual, in / out; STRIP_RESID: the iterate (read); PLANES: dinv (out) */
    double *zl[3], *xl[3]; long long zl_len, xl_len;
    double *cinvT; long long cinvT_len;
    int level, fmode, nu1, nu2, fdepth, sweeps;
    /* out (LEVELS) */
    int nlevels, lev_nz[HELM_MG_MAX_LEVELS], lev_nx[HELM_MG_MAX_LEVELS], lev_npml[HELM_MG_MAX_LEVELS];
    double lev_dx[HELM_MG_MAX_LEVELS], lev_dz[HELM_MG_MAX_LEVELS];
    int o_W, o_sweeps, o_nu1, o_nu2, o_fdepth, o_nc, o_ntiles, o_tile_rows;
    double o_omega_j, o_wstrip, o_beta, o_tau, o_cpml;
    int *tiles; long long tiles_cap;
} helm_mg_stage;
int helm_debug_mg_stage(helm_mg_stage *p);
int helm_debug_inverse_bench(int device, int n, const double *A, int reps, int recurse_n, double *ms_out);

/* --- diagnostics of the 3-D multigrid hierarchy (host only, no GPU needed; zephyr_amd/csrc/mg3_keep.hip) ------------------ */
/* One axis of n nodes (spacing h, npml absorbing-layer nodes at each end, damping amplitude cpml) coarsened `level` times by the
 * layer-preserving rule (all layer nodes kept, the interior halved).  Returns the node count nc of that level (< 0: bad arguments)
 * and fills whichever outputs are not NULL: x[nc] coordinates, lay[nc] layer flags, lap[3 nc] complex factors L(-1), L(0), L(+1)
 * of (1/xi) d/dx (1/xi) d/dx on the non-uniform axis for omega = om_re + i om_im; the transfer to the next level: pc / pw [2 nc]
 * coarse nodes and weights every node interpolates from, *n_next its size, rf[n_next] / rw[3 n_next] centre node and weights of
 * the normalised transposed interpolation. */
int helm_mg3_axis(int n, int npml, double h, double cpml, double om_re, double om_im, int level, double *x, int *lay, double *lap,
                  int *pc, double *pw, int *n_next, int *rf, double *rw);

/* --- grid transfer of the multiscale family (zephyr_amd/csrc/regrid.hip) ------------------------------------------------------- */
/* Replaces SplineGridInterpolator.__mul__ (zephyr/backend/interpolation.py:180-205): RectBivariateSpline(kx=3, ky=3, s=0) of a field on
 * one regular grid evaluated on another with the same origin -- not-a-knot cubic interpolation along each axis, points beyond the input's
 * extent clamped to its edge -- for the down- / up-scalers of MultiGridHelper (zephyr/backend/distributors.py:515-572).
 * One axis (host only, no GPU needed): n_in nodes i h_in -> n_out points j h_out.  Returns the window width W (1 .. 64) and fills, when
 * not NULL, start[n_out] and taps[n_out * W] (cap: entries taps holds): output j = sum_t taps[j W + t] in[start[j] + t].  Taps below
 * 2^-60 of their row's largest are dropped. */
int helm_regrid_axis(int n_in, double h_in, int n_out, double h_out, int *start, double *taps, int cap);
/* Opaque transfer plan from grid A (nz_a, nx_a; spacings dz_a, dx_a) to grid B on `device`: both axes' taps uploaded once.  NULL on error
 * (helm_last_error(NULL)). */
typedef struct helm_regrid helm_regrid;
helm_regrid *helm_regrid_create(int device, int nz_a, int nx_a, double dz_a, double dx_a, int nz_b, int nx_b, double dz_b, double dx_b,
                                double zorig, double xorig);
void helm_regrid_destroy(helm_regrid *plan);
/* The exact transpose of the transfer.  helm_regrid_axis_t: windows of the transpose of what helm_regrid_axis returns for the same arguments --
 * returns WT and fills start[n_in], taps[n_in * WT]: row j (an input node of the forward axis) holds the forward taps of the contiguous
 * range of outputs that touch it, a node no output touches an all-zero window.  WT > 64 (possible only when the axis up-samples):
 * HELM_ERR_UNSUPPORTED.  helm_regrid_create_t: the plan from grid B to grid A with the transposed windows of both axes, for the grid
 * arguments of helm_regrid_create; applied and destroyed like any plan (mul on grid A).  This is not the plan created with the grids
 * exchanged: that one interpolates back, this one is the adjoint of the interpolation. */
int helm_regrid_axis_t(int n_in, double h_in, int n_out, double h_out, int *start, double *taps, int cap);
helm_regrid *helm_regrid_create_t(int device, int nz_a, int nx_a, double dz_a, double dx_a, int nz_b, int nx_b, double dz_b, double dx_b,
                                  double zorig, double xorig);
/* out[f] = beta out[f] + mul (.) (gain T in[f]) for k complex128 fields (device pointers); element i of field f at in[f in_fstride +
 * i in_estride] (a (k, N) block: fstride N, estride 1 -- the fast layout; an (N, k) block: fstride 1, estride k), likewise out.  mul: N_b
 * complex values on the device, NULL for 1; beta == 0: out is not read.  Runs on op's stream (NULL: the plan's own), so it is ordered after
 * what the caller queued there without a host wait, and returns when the transfer is done.  Its intermediate comes from the library's pool. */
int helm_regrid_apply_device(helm_regrid *plan, helm_op *op, int k, const void *dIn, long long in_fstride, long long in_estride, void *dOut,
                             long long out_fstride, long long out_estride, double gain_re, double gain_im, double beta, const void *dMul);
/* the same on host arrays (dense (k, N) or (N, k) blocks, mul: N_b complex or NULL), moved through the library's pinned chunks */
int helm_regrid_apply(helm_regrid *plan, int k, const double *in, long long in_fstride, long long in_estride, double *out, long long out_fstride,
                      long long out_estride, double gain_re, double gain_im, double beta, const double *mul);

#ifdef __cplusplus
}
#endif
#endif /* HELM_H */
