// What the units of the solve driver share (capi.hip: dispatch and the C ABI; solve_direct.hip: the direct path and helm_prefactor*; krylov.hip: the
// Krylov drivers).  Internal to those three, to the test hook of nd_resid.hip, which reduces its partial sums the way the direct path does, and to
// mg3_depth.hip, whose test hooks go through testing_hook like theirs.
#pragma once
#include "helm_internal.hpp"
#include "direct.hpp"
#include <cstdlib>

// fault-injection and branch-forcing hooks of the test-suite: honoured only when the process runs with HELM_TESTING=1 (read per call: the tests flip them)
inline int testing_hook(const char *name) {
    const char *t = getenv("HELM_TESTING"), *v = getenv(name);
    return t && atoi(t) != 0 && v ? atoi(v) : 0;
}
inline double testing_hook_d(const char *name, double d) {      // a hook with a floating-point value; d: what it is without HELM_TESTING=1
    const char *t = getenv("HELM_TESTING"), *v = getenv(name);
    return t && atoi(t) != 0 && v ? atof(v) : d;
}
// statuses of one right-hand side across the blocks / passes of a call, by severity: 0 converged < 3 at the fp64 floor (counted as solved)
// < 1 cap / stalled < 2 breakdown
inline int status_rank(int st) { return st == 0 ? 0 : (st == 3 ? 1 : (st == 1 ? 2 : 3)); }
inline int merge_status(int a, int b) { return status_rank(a) >= status_rank(b) ? a : b; }

struct NvGuard {     // Krylov vector length of the handle for the duration of a solve
    helm_op *op; long long old;
    NvGuard(helm_op *o, long long nv) : op(o), old(o->Nv) { o->Nv = nv; }
    ~NvGuard() { op->Nv = old; }
};

// the records of per-launch timing events start again from empty (a solve without a prefactorisation in flight; a prefactorisation)
inline void timing_reset_events(helm_op *op) {
    op->ev_used = 0; op->ev_pending.clear();
    op->ev_pending_gemm.clear(); op->ev_pending_gemm_n.clear(); op->ev_pending_gemm_bytes.clear(); op->ev_pending_gemm_sol.clear(); op->ev_pending_gemm_shape.clear();
}

// ---- per-handle workspace (krylov.hip) ----------------------------------------------------------
int ensure_ws(helm_op *op, size_t bytes);      // op->d_ws: Krylov vectors; the direct path's scratch when every shared slot is taken
int ensure_part(helm_op *op, int nrhs);        // op->d_part, d_scal, h_scal: partial sums and per-right-hand-side records for batches of nrhs

// scratch of one direct solve: a slot of the device's table (runtime.hip); when every slot is inside a solve (or the allocation failed) the handle's own workspace
struct WsLease {
    int slot = -1; void *ptr = nullptr;
    WsLease(helm_op *op, size_t bytes) {
        ptr = ws_checkout(op->device, bytes, &slot);
        if (!ptr) { slot = -1; ptr = ensure_ws(op, bytes) == HELM_OK ? op->d_ws : nullptr; }
    }
    ~WsLease() { ws_checkin(slot); }
};

// ---- direct path (solve_direct.hip) -------------------------------------------------------------
// Can this operator take the prefactorable direct path -- assembled, 2-D, no factorisation of it has failed, not the coupled TTI system (that one is
// row-equilibrated and factored inside its solve), the path not switched off (helm_tuning.auto_direct; `by_name`: the caller asked for HELM_DIRECT itself,
// which that switch does not govern) and no failure injected by the test-suite?
bool direct_path_ok(const helm_op *op, bool by_name = false);
// Batch width and scratch of the direct path: at most opts.batch (default 256) right-hand sides at a time, halved until a batch fits helm_tuning.nd_ws_gb.
// Per right-hand side the node-major pipeline keeps q', x, the stored residual and the correction (4 N) beside the two front-vector regions; the
// rhs-major path of the coupled system (sys2) q', r and the solve scratch.  The factorisation scratch, when the solve factors, lies behind it.
struct DirectBatch { long long per_rhs; int Bmax; size_t bytes() const { return (size_t)per_rhs * Bmax * sizeof(cplx); } };
DirectBatch direct_batch(const NdPlan &plan, long long N, int nrhs, int batch_opt, int sys2, const helm_tuning &tune);
// Solve M_block X = premul * RHS[:, row_off : row_off+N] - sub for nrhs right-hand sides; dXout: [nrhs][N] (NOT conjugated); info (optional) is
// filled per right-hand side.  Returns the number of right-hand sides left above rtol, or a negative error code.
// sys2 != 0: the coupled two-field Eurus system (block ignored, vectors [u; v] of length 2N, rows_in = N or 2N rows of right-hand side per
// source; sub unused); dXout then holds 2N values per right-hand side.
// dUconj (single-block systems, N rows per right-hand side): the result is left there already conjugated and dXout is not written.
int solve_block_direct(helm_op *op, int block, const cplx *dRHS, long long rhs_ld, long long row_off, cplx premul, const cplx *sub, cplx *dXout, int nrhs,
                       const helm_solve_opts &o, helm_solve_info *info, int sys2 = 0, long long rows_in = 0, cplx *dUconj = nullptr);

// ---- Krylov drivers (krylov.hip) ----------------------------------------------------------------
// k_fin: one workgroup per right-hand side sums the partials of the launch before it in a fixed order and advances that right-hand side's scalar
// record.  The direct path and the residual test hook use it for the plain sums: FIN_NORM (aux[b] = sum) and FIN_NORM2.
enum { FIN_BICG_INIT = 0, FIN_ALPHA = 1, FIN_OMEGA = 2, FIN_RHO = 3, FIN_RESTART = 4,
       FIN_CG_INIT = 5, FIN_CG_ALPHA = 6, FIN_CG_RR = 7, FIN_CG_BETA = 8, FIN_NORM = 9,
       FIN_NORM2 = 10 /* aux[b] = slot 0, aux[nrhs + b] = slot 1 */ };
int helm_launch_fin_ex(helm_op *op, int which, int nrhs, int nblk_part, const int *mask = nullptr, double *aux = nullptr);
// Apply of the coupled Eurus system [[M1, M2], [M3, M4]] (or its conjugate transpose) to vectors [u; v] of length 2N:
// four stencil launches, the second of each output half accumulating into the first and carrying the fused epilogue.
// raw = unscaled planes (true residual), otherwise the row-equilibrated system d_S.
int launch_sys2_apply(helm_op *op, bool raw, int adjoint, const cplx *X, cplx *Y, const cplx *W, int nrhs, int epi, const RhsScal *scal, const cplx *planes_override = nullptr);
// the same contract as solve_block_direct (always fills dXout): BiCGSTAB on the Jacobi-scaled or multigrid-preconditioned system, CGNR as the safety net
int solve_block_krylov(helm_op *op, int block, const cplx *dRHS, long long rhs_ld, long long row_off, cplx premul, const cplx *sub, cplx *dXout, int nrhs,
                       const helm_solve_opts &o, helm_solve_info *info, int sys2, long long rows_in);
