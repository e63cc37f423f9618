// The sparse direct path of a solve (set-up, batches, iterative refinement; the solver itself is nd_*.hip) and what prepares it ahead of
// the solve: helm_prefactor, helm_prefactor_many, helm_prefactor_n.
#include "solve_internal.hpp"
#include <algorithm>

// ---- the decisions of the direct path that more than one caller takes (solve_internal.hpp) -------------------------------------------------
bool direct_path_ok(const helm_op *op, bool by_name) {
    if (!op->assembled || op->ny > 0 || op->direct_failed) return false;
    if (op->variant == HELM_EURUS && !op->block_zero[2]) return false;          // coupled TTI: row-equilibrated inside the solve
    if (!by_name && helm_tuning_now().auto_direct == 0) return false;
    return !testing_hook("HELM_ND_INJECT_FAILURE");
}

DirectBatch direct_batch(const NdPlan &plan, long long N, int nrhs, int batch_opt, int sys2, const helm_tuning &tune) {
    DirectBatch d;
    d.per_rhs = sys2 ? nd_solve_ws_elems(plan, 1) + 2 * 2 * N : 4 * N + 2 * plan.vregion;
    d.Bmax = batch_opt > 0 ? batch_opt : 256;
    if (d.Bmax > nrhs) d.Bmax = nrhs;
    const double cap = tune.nd_ws_gb * 1e9;
    while (d.Bmax > 1 && (double)d.per_rhs * d.Bmax * sizeof(cplx) > cap) d.Bmax = (d.Bmax + 1) / 2;
    return d;
}

// ---- solve -----------------------------------------------------------------------------------------------------------------------------------
namespace {

int nd_debug() { static const int v = getenv("HELM_ND_DEBUG") ? atoi(getenv("HELM_ND_DEBUG")) : 0; return v; }

struct FactorOwner {       // a factor under construction is released on every early return
    NdFactor *p = nullptr;
    ~FactorOwner() { if (p) nd_free(p); }
};

// what the batches of one solve_block_direct call share: its arguments, the factors, the leased scratch and the small per-batch buffers
struct DirectCall {
    helm_op *op; int block, slot; NdFactor *f;
    const cplx *dRHS; long long rhs_ld, row_off; cplx premul; const cplx *sub; cplx *dXout, *dUconj; long long rows_in;
    const helm_solve_opts &o; helm_solve_info *info;
    cplx *ws; int Bmax; cplx *ws_factor;      // the lease: Bmax right-hand sides of solve scratch and, behind them, the factorisation scratch
    FactorOwner *fresh; bool factor_pending;  // the factors are still to be made (by the first node-major batch, beside its forward elimination)
    bool native_nm;
    int max_refine;                           // passes stop earlier when the residual stalls
    int nblk; char *ptail, *htail; double *d_aux, *h_aux;      // partials per right-hand side; tails of d_part / h_scal: 2 Bmax doubles, then Bmax ints
    int unconverged = 0;
};

// Verdict of a refinement round on the true relative residuals: stop when every right-hand side has met rtol, when the passes are used up, or when
// the worst residual no longer halves (refinement contracts by the accuracy of the factorisation per pass; give up when it has stopped doing so)
bool refine_done(const std::vector<double> &relres, double rtol, int round, int max_refine, double &prev_worst) {
    bool all_ok = true;
    double worst = 0.0;
    for (double rr : relres) {
        if (!(rr <= rtol)) all_ok = false;
        if (!(rr <= worst)) worst = rr;       // NaN-propagating max
    }
    if (nd_debug()) fprintf(stderr, "[helm direct] pass %d: worst true relres %.3e\n", round + 1, worst);
    const bool stalled = round > 0 && !(worst < 0.5 * prev_worst);
    prev_worst = worst;
    return all_ok || round >= max_refine || stalled;
}

// The right-hand sides above rtol when they are a minority (fewer than half; at least one is above when a pass is due): only their residual columns are
// packed to a narrower batch, solved, and the corrections added back.  Empty: the whole batch takes the pass.
std::vector<int> minority_above(const std::vector<double> &relres, double rtol) {
    std::vector<int> bad;
    const int n = (int)relres.size();
    for (int b = 0; b < n; ++b) if (!(relres[b] <= rtol)) bad.push_back(b);
    if ((int)bad.size() >= n / 2) bad.clear();
    return bad;
}

// what a batch reports per source: solved when within rtol or at the fp64 floor (status 3); returns how many were not
int report_batch(helm_solve_info *info, int first, double rtol, const std::vector<double> &relres, const std::vector<int> &at_floor, const std::vector<int> &extra_solves) {
    // fault injection for the tests of the partial fallback: report the first k right-hand sides as stalled
    const int inject_stall = testing_hook("HELM_ND_INJECT_STALL");
    int unconverged = 0;
    for (int b = 0; b < (int)relres.size(); ++b) {
        const bool ok = (relres[b] <= rtol * 1.0000001 || at_floor[b]) && !(first + b < inject_stall);
        if (!ok) unconverged += 1;
        if (info) {
            helm_solve_info &I = info[first + b];
            I.iterations += 1 + extra_solves[b]; I.method = HELM_DIRECT;
            I.relres = std::max(I.relres, relres[b]);
            I.status = merge_status(I.status, ok ? (at_floor[b] ? 3 : 0) : 1);
        }
    }
    return unconverged;
}

// Node-major pipeline (single-block systems): the right-hand sides are transposed once on the way in (fused with premul /
// the norm), stay [cell][rhs] through solve, true residual and refinement, and are transposed once on the way out.
// native_nm (HELM_NODE_MAJOR: both buffers in the reference's (N, nrhs) layout; one batch):
// the right-hand sides are used where they lie -- premul moves to the output, u = conj(premul A^-1 q), the relative residual does not see
// it -- ||q||^2 comes out of the first residual launch, and the wavefield is written by the launch that checks it
int direct_batch_nm(DirectCall &c, int first, int n) {
    helm_op *op = c.op; NdFactor *f = c.f;
    const helm_solve_opts &o = c.o;
    const long long N = op->N;
    const int Bmax = c.Bmax, nblk = c.nblk, cj = c.dUconj ? 1 : 0;
    const bool native_nm = c.native_nm;
    const cplx premul = c.premul;
    cplx *const dUconj = c.dUconj;
    double *d_aux = c.d_aux, *h_aux = c.h_aux;
    int rc;
    cplx *Qt = c.ws, *Xt = Qt + (long long)Bmax * N, *Rt = Xt + (long long)Bmax * N, *Dt = Rt + (long long)Bmax * N, *arenaV = Dt + (long long)Bmax * N;
    if (native_nm) Qt = const_cast<cplx *>(c.dRHS);             // read only from here on (the residual is stored to Rt, never over q)
    cplx *xout = cj ? dUconj + (long long)first * N : c.dXout + (long long)first * N;
    const cplx *rhs_b = c.dRHS + (long long)first * c.rhs_ld;
    const cplx *sub_b = c.sub ? c.sub + (long long)first * N : nullptr;
    const cplx *planes = op->d_C + (long long)c.block * op->nplanes * N;
    int *d_cols = (int *)(c.ptail + (size_t)Bmax * 2 * sizeof(double));
    int *h_cols = (int *)(c.htail + (size_t)op->scal_cap * 2 * sizeof(double));
    int nb_part = 0;
    if (!native_nm) {
        rc = nd_prep_transpose_norm(op, rhs_b, c.rhs_ld, c.row_off, premul, sub_b, Qt, N, n, (double *)op->d_part, nblk, &nb_part);
        if (rc) return rc;
        helm_launch_fin_ex(op, FIN_NORM, n, nb_part, nullptr, d_aux + n);           // ||q'||^2
    }
    bool have_qnorm = !native_nm;
    NdResidExtra rex;
    if (native_nm) { rex.Uout = dUconj; rex.ldu = n; rex.oscale = premul; }
    // direct output (helm_tuning.nd_direct_out; full-width batches, whose residual kernel can read the caller's array): the back substitution writes
    // u = conj(premul x) into dUconj itself and the residual launch below stores nothing -- x_in_u until a refinement pass needs x back in Xt
    NdDirectOut dout;
    // (not when the caller solves in place, dU == dRHS: the back substitution would overwrite q before the residual launch has read it -- that call takes the
    // path of the narrow batches, where the residual launch reads q[cell] and writes u[cell] in the same thread)
    bool x_in_u = native_nm && n > 128 && helm_tuning_now().nd_direct_out != 0 && (const void *)Qt != (const void *)dUconj;
    if (x_in_u) { dout.U = dUconj; dout.oscale = premul; }
    if (c.factor_pending) {
        float fms = 0.f;
        rc = nd_factor_solve_nm(op, c.block, f, c.ws_factor, nullptr, Qt, Xt, n, arenaV, op->side_stream, &fms, x_in_u ? &dout : nullptr);
        if (rc) return rc;
        op->direct[c.slot] = f; c.fresh->p = nullptr;
        op->timing.factor_ms += fms;
        c.factor_pending = false;
    } else {
        rc = nd_solve_nm(op, f, Qt, Xt, n, arenaV, x_in_u ? &dout : nullptr);
        if (rc) return rc;
    }
    auto recover_x = [&]() -> int {            // x of every cell back in Xt (the residual of what follows is evaluated from Xt again, ||q||^2 unscaled)
        if (!x_in_u) return HELM_OK;
        x_in_u = false; have_qnorm = false;
        return nd_recover_x(op, dUconj, Xt, (long long)n * N, premul);
    };
    // where the right-hand sides of this batch can be nonzero at all (the flags of the sparse forward pass just run on Qt): the residual
    // launches read q only there -- every later evaluation too, Qt does not change
    rex.qmask = nd_rhs_mask(op, f);
    std::vector<double> relres(n, 0.0), qq(n, 0.0);
    std::vector<int> extra_solves(n, 0);
    double prev_worst = 0.0;
    // every pass ends with the TRUE residual q' - A x of the vector that is returned (norms only); q' is kept for that
    auto true_residual_norms = [&]() -> int {
        rex.qnorm = have_qnorm ? 0 : 1;
        int r1;
        if (x_in_u) {
            NdResidExtra ru = rex; ru.Uout = nullptr; ru.xin_is_u = 1;
            r1 = nd_resid_nm(op, planes, dUconj, n, Qt, n, nullptr, n, 0, nullptr, (double *)op->d_part, nblk, &nb_part, &ru);
        } else
        r1 = nd_resid_nm(op, planes, Xt, n, Qt, n, nullptr, n, 0, nullptr, (double *)op->d_part, nblk, &nb_part, (native_nm || rex.qmask) ? &rex : nullptr);
        if (r1) return r1;
        helm_launch_fin_ex(op, have_qnorm ? FIN_NORM : FIN_NORM2, n, nb_part, nullptr, d_aux);
        have_qnorm = true;
        HIP_TRY(op, hipMemcpyAsync(h_aux, d_aux, 2 * n * sizeof(double), hipMemcpyDeviceToHost, op->stream));
        HIP_TRY(op, hipStreamSynchronize(op->stream));
        for (int b = 0; b < n; ++b) { qq[b] = h_aux[n + b]; relres[b] = qq[b] > 0 ? sqrt(h_aux[b] / qq[b]) : 0.0; }
        return HELM_OK;
    };
    rc = true_residual_norms();
    if (rc) return rc;
    for (int round = 0; !refine_done(relres, o.rtol, round, c.max_refine, prev_worst); ++round) {
        // r = q' - A x stored (Rt), dx = A^-1 r, x += dx
        rc = recover_x();
        if (rc) return rc;
        rc = nd_resid_nm(op, planes, Xt, n, Qt, n, nullptr, n, 1, Rt, (double *)op->d_part, nblk, &nb_part);
        if (rc) return rc;
        const std::vector<int> bad = minority_above(relres, o.rtol);
        const int k = (int)bad.size();
        if (k > 0) {
            for (int j = 0; j < k; ++j) h_cols[j] = bad[j];
            HIP_TRY(op, hipMemcpyAsync(d_cols, h_cols, k * sizeof(int), hipMemcpyHostToDevice, op->stream));
            cplx *Rp = Dt, *Dp = Dt + N * k;              // k < n / 2: both fit the correction buffer
            rc = nd_pack_cols(op, Rt, n, d_cols, k, Rp, N);
            if (rc) return rc;
            rc = nd_solve_nm(op, f, Rp, Dp, k, arenaV);
            if (rc) return rc;
            rc = nd_scatter_add_cols(op, Xt, n, d_cols, k, Dp, N);
            if (rc) return rc;
            for (int j = 0; j < k; ++j) extra_solves[bad[j]] += 1;
        } else {
            rc = nd_solve_nm(op, f, Rt, Dt, n, arenaV);
            if (rc) return rc;
            nd_axpy_one(op, Xt, Dt, (long long)n * N, 0);
            for (int b = 0; b < n; ++b) extra_solves[b] += 1;
        }
        rc = true_residual_norms();
        if (rc) return rc;
    }
    if (!native_nm) {           // (node-major callers: the last residual launch has written conj(premul x) already)
        rc = nd_transpose_out(op, Xt, N, n, xout, cj);
        if (rc) return rc;
    }
    // Right-hand sides refinement left above rtol: is the residual at the floor fp64 allows (relres ~ eps || |A||x| + |q| || / ||q||,
    // see direct_batch_sys2)?  Evaluated node-major with |planes| and |x|; ||.|| of the sum bounded by the sum of norms.
    std::vector<int> at_floor(n, 0);
    bool any = false;
    for (int b = 0; b < n; ++b) if (!(relres[b] <= o.rtol)) any = true;
    const size_t pbytes = (size_t)op->nplanes * N * sizeof(cplx);
    cplx *absP = any ? (cplx *)helm_pool_alloc(op->device, pbytes) : nullptr;
    if (any && absP) {
        rc = recover_x();
        if (!rc) rc = helm_launch_abs(op, planes, absP, (long long)op->nplanes * N, 1.0);
        if (!rc) rc = helm_launch_abs(op, Xt, Dt, (long long)n * N, 1.0);
        if (!rc && hipMemsetAsync(Rt, 0, (size_t)n * N * sizeof(cplx), op->stream) != hipSuccess) rc = HELM_ERR_DEVICE;
        if (!rc) rc = nd_resid_nm(op, absP, Dt, n, Rt, n, nullptr, n, 0, nullptr, (double *)op->d_part, nblk, &nb_part);      // -|A||x|
        if (!rc) {
            helm_launch_fin_ex(op, FIN_NORM, n, nb_part, nullptr, d_aux);
            if (hipMemcpyAsync(h_aux, d_aux, n * sizeof(double), hipMemcpyDeviceToHost, op->stream) != hipSuccess || hipStreamSynchronize(op->stream) != hipSuccess) rc = HELM_ERR_DEVICE;
        }
        helm_pool_free(op->device, absP, pbytes);
        if (rc) return rc;
        for (int b = 0; b < n; ++b) {
            const double fl = qq[b] > 0 ? 1.1102230246251565e-16 * (sqrt(h_aux[b]) + sqrt(qq[b])) / sqrt(qq[b]) : 0.0;
            if (!(relres[b] <= o.rtol) && relres[b] <= 8.0 * fl) at_floor[b] = 1;
            if (nd_debug() && !(relres[b] <= o.rtol)) fprintf(stderr, "[helm direct] rhs %d: relres %.3e, fp64 floor %.3e\n", first + b, relres[b], fl);
        }
    }
    c.unconverged += report_batch(c.info, first, o.rtol, relres, at_floor, extra_solves);
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}

// The coupled two-field system keeps its vectors rhs-major, [u; v] of 2N per right-hand side: q' zero-padded to 2N rows, the solve on the
// row-equilibrated system A_s = D A (the factors exist: the coupled system is factored before its first batch), the true residual on the raw planes.
int direct_batch_sys2(DirectCall &c, int first, int n) {
    helm_op *op = c.op; NdFactor *f = c.f;
    const helm_solve_opts &o = c.o;
    const long long N = op->N, NV = 2 * N;
    const int Bmax = c.Bmax;
    double *d_aux = c.d_aux, *h_aux = c.h_aux;
    int rc;
    cplx *q = c.ws, *r = q + (long long)Bmax * NV, *nws = q + 2LL * Bmax * NV;
    cplx *x = c.dXout + (long long)first * NV;
    const cplx *rhs_b = c.dRHS + (long long)first * c.rhs_ld;
    HIP_TRY(op, hipMemsetAsync(q, 0, (size_t)n * NV * sizeof(cplx), op->stream));
    for (int half = 0; half < (c.rows_in == 2 * N ? 2 : 1); ++half) {
        rc = helm_launch_prep_rhs(op, rhs_b, c.rhs_ld, half * N, c.premul, nullptr, nullptr, nullptr, q, NV, half * N, n);
        if (rc) return rc;
    }
    helm_launch_norm2(op, q, n);
    helm_launch_fin_ex(op, FIN_NORM, n, helm_vec_num_blocks(op), nullptr, d_aux + n);
    for (int half = 0; half < 2; ++half) {
        rc = helm_launch_prep_rhs(op, q, NV, half * N, cmake(1.0, 0.0), nullptr, nullptr, op->d_rs + half * N, x, NV, half * N, n);
        if (rc) return rc;
    }
    rc = nd_solve(op, f, x, x, n, nws);
    if (rc) return rc;
    std::vector<double> relres(n, 0.0);
    std::vector<int> extra_solves(n, 0);
    double prev_worst = 0.0;
    for (int round = 0; ; ++round) {
        rc = launch_sys2_apply(op, true, 0, x, r, q, n, EPI_RESID, nullptr);
        if (rc) return rc;
        helm_launch_fin_ex(op, FIN_NORM, n, 2 * helm_apply_num_blocks(op), nullptr, d_aux);
        HIP_TRY(op, hipMemcpyAsync(h_aux, d_aux, 2 * n * sizeof(double), hipMemcpyDeviceToHost, op->stream));
        HIP_TRY(op, hipStreamSynchronize(op->stream));
        for (int b = 0; b < n; ++b) { const double qq = h_aux[n + b]; relres[b] = qq > 0 ? sqrt(h_aux[b] / qq) : 0.0; }
        if (refine_done(relres, o.rtol, round, c.max_refine, prev_worst)) break;
        const std::vector<int> bad = minority_above(relres, o.rtol);
        const int k = (int)bad.size();
        if (k > 0) {            // their residual columns are packed to the front of r (whole 16 MB rows)
            for (int j = 0; j < k; ++j)
                if (bad[j] != j) HIP_TRY(op, hipMemcpyAsync(r + (long long)j * NV, r + (long long)bad[j] * NV, (size_t)NV * sizeof(cplx), hipMemcpyDeviceToDevice, op->stream));
            rc = helm_launch_rowscale_inplace(op, r, op->d_rs, NV, k);
            if (rc) return rc;
            rc = nd_solve(op, f, r, r, k, nws);
            if (rc) return rc;
            for (int j = 0; j < k; ++j) nd_axpy_one(op, x + (long long)bad[j] * NV, r + (long long)j * NV, NV);
            for (int j = 0; j < k; ++j) extra_solves[bad[j]] += 1;
        } else {
            rc = helm_launch_rowscale_inplace(op, r, op->d_rs, NV, n);
            if (rc) return rc;
            rc = nd_solve(op, f, r, r, n, nws);       // dx = A^-1 r
            if (rc) return rc;
            nd_axpy_one(op, x, r, (long long)n * NV);
            for (int b = 0; b < n; ++b) extra_solves[b] += 1;
        }
    }
    // Where refinement has stalled above rtol, is that the floor of fp64 itself?  The residual of ANY fp64 vector x
    // near the solution carries rounding of size eps (|A||x| + |q|) componentwise, so ||r|| / ||q|| cannot be pushed below
    // ~ eps || |A||x| + |q| || / ||q||, whatever the solver (a backward-stable sparse LU lands there too).  Evaluated with the
    // stencil kernel on |planes| and |x|; right-hand sides within 8x of it are reported as status 3, not as failures.
    std::vector<int> at_floor(n, 0);
    bool any = false;
    for (int b = 0; b < n; ++b) if (!(relres[b] <= o.rtol)) any = true;
    const size_t pbytes = (size_t)36 * N * sizeof(cplx);
    cplx *absP = any ? (cplx *)helm_pool_alloc(op->device, pbytes) : nullptr;
    if (any && absP) {
        cplx *absx = r, *negq = nws, *yy = nws + (long long)n * NV;
        rc = helm_launch_abs(op, op->d_C, absP, 36LL * N, 1.0);
        if (!rc) rc = helm_launch_abs(op, x, absx, (long long)n * NV, 1.0);
        if (!rc) rc = helm_launch_abs(op, q, negq, (long long)n * NV, -1.0);
        if (!rc) rc = launch_sys2_apply(op, true, 0, absx, yy, negq, n, EPI_RESID, nullptr, absP);      // -(|q| + |A||x|)
        if (!rc) {
            helm_launch_fin_ex(op, FIN_NORM, n, 2 * helm_apply_num_blocks(op), nullptr, d_aux);
            if (hipMemcpyAsync(h_aux, d_aux, n * sizeof(double), hipMemcpyDeviceToHost, op->stream) != hipSuccess || hipStreamSynchronize(op->stream) != hipSuccess) rc = HELM_ERR_DEVICE;
        }
        helm_pool_free(op->device, absP, pbytes);
        if (rc) return rc;
        for (int b = 0; b < n; ++b) {
            // ||q||^2 was left in h_aux[n + b] by the residual rounds
            const double qq = h_aux[n + b];
            const double fl = qq > 0 ? 1.1102230246251565e-16 * sqrt(h_aux[b] / qq) : 0.0;
            if (!(relres[b] <= o.rtol) && relres[b] <= 8.0 * fl) at_floor[b] = 1;
            if (nd_debug()) fprintf(stderr, "[helm direct] rhs %d: relres %.3e, fp64 floor %.3e\n", first + b, relres[b], fl);
        }
    }
    c.unconverged += report_batch(c.info, first, o.rtol, relres, at_floor, extra_solves);
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}

}  // namespace

// Sparse direct path (nd_*.hip): factor once per assembled operator (the coupled system row-equilibrated, factors kept in slot 1), then per batch
// q' -> x by the multifrontal triangular solves and iterative refinement on the true residual q' - A x (stencil kernel) until rtol is met.
int solve_block_direct(helm_op *op, int block, const cplx *dRHS, long long rhs_ld, long long row_off, cplx premul,
                       const cplx *sub, cplx *dXout, int nrhs, const helm_solve_opts &o, helm_solve_info *info,
                       int sys2, long long rows_in, cplx *dUconj) {
    const long long N = op->N;
    NvGuard nvguard(op, sys2 ? 2 * N : N);
    const int slot = sys2 ? 1 : block;
    int rc;
    NdFactor *f = op->direct[slot];
    const bool need_factor = (f == nullptr);
    // factors enqueued by helm_prefactor on the handle's factor stream: everything this call launches comes after them
    if (op->pf_pending && f && op->pf_done) HIP_TRY(op, hipStreamWaitEvent(op->stream, op->pf_done, 0));
    // fault injection for the tests of the AUTO fallback
    if (testing_hook("HELM_ND_INJECT_FAILURE")) HELM_FAIL(op, HELM_ERR_DEVICE, "direct solver: injected failure (HELM_ND_INJECT_FAILURE)");
    FactorOwner fresh;
    if (need_factor) {
        f = new NdFactor();
        fresh.p = f;
        rc = nd_get_plan(op, helm_tuning_now().nd_leaf, sys2 ? 2 : 1, &f->pd);
        if (rc) return rc;
    }
    const DirectBatch db = direct_batch(f->pd->plan, N, nrhs, o.batch, sys2, helm_tuning_now());
    const int Bmax = db.Bmax;
    // factorisation scratch sits behind the solve scratch (they are live together when the forward elimination of the first batch runs
    // beside the factorisation on a second stream, below)
    const long long fws = need_factor ? nd_factor_ws_elems(f->pd->plan) : 0LL;
    const long long ws_elems = db.per_rhs * Bmax + fws;
    WsLease lease(op, (size_t)ws_elems * sizeof(cplx));
    if (!lease.ptr) HELM_FAIL(op, HELM_ERR_DEVICE, "direct solver: cannot allocate %.1f GB of scratch", ws_elems * 16e-9);
    cplx *ws_factor = (cplx *)lease.ptr + db.per_rhs * Bmax;
    if (sys2) {     // the coupled system is factored row-equilibrated (its v rows are orders of magnitude smaller than its u rows,
        rc = helm_launch_rowscaled_system(op);      // which would mislead the magnitude-based pivoting): A_s = D A, A_s x = D q'
        if (rc) return rc;
    }
    // node-major pipeline: the forward elimination of the first batch may run beside the factorisation (HELM_ND_OVERLAP_NM)
    // -- measured on the 16-frequency job: 44.9 -> 43.8 ms per work item; the factorisation itself stretches from 17.6 to 22.2 ms under
    // the competing launches but 5 ms of forward pass disappear behind it.  Not while per-launch profiling is on: HIP events around
    // kernels that share the chip with another stream measure the sharing, not the kernel (HELM_ND_OVERLAP_NM=2 forces it anyway).
    const int overlap_nm = helm_tuning_now().nd_overlap;
    const bool nm_overlap = need_factor && (overlap_nm == 2 || (overlap_nm == 1 && !op->profiling)) && !sys2;
    bool factor_pending = need_factor;
    if (need_factor && !nm_overlap) {
        hipEvent_t f0, f1;
        HIP_TRY(op, hipEventCreate(&f0)); HIP_TRY(op, hipEventCreate(&f1));
        hipEventRecord(f0, op->stream);
        rc = nd_factor(op, block, f, ws_factor, sys2 ? op->d_S : nullptr);
        hipEventRecord(f1, op->stream);
        hipEventSynchronize(f1);
        float ms = 0.f; hipEventElapsedTime(&ms, f0, f1);
        hipEventDestroy(f0); hipEventDestroy(f1);
        if (rc) return rc;
        op->direct[slot] = f; fresh.p = nullptr;
        op->timing.factor_ms += ms;
        factor_pending = false;
    }
    if (factor_pending && !op->side_stream) {
        // lowest priority: the forward pass that runs beside the factorisation must not delay the factorisation's chain of small launches
        op->side_stream = helm_stream_acquire(op->device, -1);
        if (!op->side_stream) HELM_FAIL(op, HELM_ERR_DEVICE, "hipStreamCreate failed");
    }
    rc = ensure_part(op, Bmax);
    if (rc) return rc;
    const int nblk = std::max(2 * helm_apply_num_blocks(op), helm_vec_num_blocks(op));
    char *ptail = (char *)op->d_part + (size_t)Bmax * 4 * nblk * sizeof(double);
    char *htail = (char *)op->h_scal + (size_t)op->scal_cap * sizeof(RhsScal);
    // HELM_NODE_MAJOR: helm_solve_device only passes it for one batch of a single-block system
    const bool native_nm = !sys2 && (o.flags & HELM_NODE_MAJOR) == HELM_NODE_MAJOR && nrhs <= Bmax && !sub && row_off == 0 && dUconj;
    if ((o.flags & HELM_NODE_MAJOR) && !native_nm) HELM_FAIL(op, HELM_ERR_STATE, "direct solver: node-major buffers reached a path that cannot take them");
    DirectCall c{op, block, slot, f, dRHS, rhs_ld, row_off, premul, sub, dXout, dUconj, rows_in, o, info, (cplx *)lease.ptr, Bmax, ws_factor,
                 &fresh, factor_pending, native_nm, sys2 ? 40 : 10, nblk, ptail, htail, (double *)ptail, (double *)htail};
    for (int first = 0; first < nrhs; first += Bmax) {
        const int n = std::min(Bmax, nrhs - first);
        rc = sys2 ? direct_batch_sys2(c, first, n) : direct_batch_nm(c, first, n);
        if (rc) return rc;
    }
    return c.unconverged;
}

// ---- prefactorisation -----------------------------------------------------------------------------------------------------------------------
// A factorisation started by helm_prefactor is complete (or abandoned): wait for it, book its time, give its scratch back.
void helm_pf_retire(helm_op *op) {
    if (!op || !op->pf_pending) return;
    hipSetDevice(op->device);
    if (op->pf_done) hipEventSynchronize(op->pf_done);
    float ms = 0.f;
    if (op->pf_t0 && op->pf_t1 && hipEventElapsedTime(&ms, op->pf_t0, op->pf_t1) == hipSuccess) op->timing.factor_ms += ms / std::max(1, op->pf_share);
    if (op->pf_ws) helm_pool_free(op->device, op->pf_ws, op->pf_ws_bytes);
    op->pf_ws = nullptr; op->pf_ws_bytes = 0; op->pf_share = 1;
    op->pf_pending = false;
    scratch_sweep(op->device, false);          // (this operator's factorisation has finished: its set's scratch, and any older one's, goes back now)
}

// 3-D: what the next solve would build first -- the multigrid hierarchy with its directly solved level (hundreds of ms of GPU work and host logic,
// with waits in between) -- built NOW, in the calling thread.  Meant for a dispatcher's prepare thread: the set-up of frequency k+1 then runs
// beside the Krylov iterations of frequency k on another handle.  nrhs: right-hand sides the solve will bring (batch width, depth decision).
static int prefactor3d(helm_op *op, int nrhs) {
    if (op->mg3 || op->mg3_no_keep) return HELM_OK;
    const int auto_mg3 = helm_tuning_now().auto_mg3;
    if (!auto_mg3 || std::min(op->nz, std::min(op->ny, op->nx)) < 24) return HELM_OK;
    HIP_TRY(op, hipSetDevice(op->device));
    const int Bmax = std::max(1, std::min(nrhs > 0 ? nrhs : 16, 16));
    NvGuard guard(op, op->N);
    if (helm_ensure_scaled(op) != HELM_OK) return HELM_OK;
    if (ensure_ws(op, (size_t)11 * Bmax * op->N * sizeof(cplx)) != HELM_OK || ensure_part(op, Bmax) != HELM_OK) return HELM_OK;
    op->mg3_rhs_hint = nrhs > 0 ? nrhs : 16;
    // on a low-priority stream: the set-up is compute-bound products that would otherwise take the CUs from the (bandwidth-bound, critical-path)
    // iterations of the frequency being solved on another handle
    static const int prio = getenv("HELM_PF3_PRIO") ? atoi(getenv("HELM_PF3_PRIO")) : -1;
    hipStream_t main = op->stream, low = prio < 0 ? helm_stream_acquire(op->device, -1) : nullptr;
    if (low) op->stream = low;
    (void)mg_setup(op, Bmax);            // a hint: a failure here is the solve's to report
    if (low) {
        hipStreamSynchronize(low);
        op->stream = main;
        mg3_retarget_stream(op, main);
        helm_stream_release(op->device, -1, low);
    }
    return HELM_OK;
}

// The tolerance the solves on this operator will ask for, told BEFORE its factors are built (helm_prefactor has no options argument): which
// ill-conditioned fronts get the pivoted-LU treatment follows from it (direct.hip, stabilise_group).  Every solve records its own rtol as well,
// so a factorisation that happens inside a solve needs no hint.
extern "C" int helm_set_tolerance_hint(helm_op *op, double rtol) {
    helm_tuning_refresh();
    if (!op || !(rtol > 0)) return HELM_ERR_ARG;
    op->rtol_hint = rtol; op->rtol_hint_set = true;
    return HELM_OK;
}

// Enqueue the factorisations of ops[0 .. n) -- operators of one grid on one device that pass direct_path_ok and have no factors yet -- on the factor stream of
// ops[0]: a single operator by its own launches, a set by the same launches for all (nd_factor_enqueue_many).  The launches' timing records are booked with
// the solve that uses the factors; the scratch goes back to the pool when the factorisation has finished on the GPU.
static int pf_enqueue(helm_op *const *ops, int n) {
    helm_op *op0 = ops[0];
    HIP_TRY(op0, hipSetDevice(op0->device));
    if (!op0->fstream) {
        op0->fstream_prio = helm_tuning_now().pf_prio;       // priority class of the factor stream (HELM_PF_PRIO: 1 highest, 0 normal, -1 lowest)
        op0->fstream = helm_stream_acquire(op0->device, op0->fstream_prio);
        if (!op0->fstream) HELM_FAIL(op0, HELM_ERR_DEVICE, "hipStreamCreate failed");
    }
    for (int k = 0; k < n; ++k) {
        helm_op *op = ops[k];
        if (!op->pf_done) HIP_TRY(op, hipEventCreateWithFlags(&op->pf_done, hipEventDisableTiming));
        if (!op->pf_t0) HIP_TRY(op, hipEventCreate(&op->pf_t0));
        if (!op->pf_t1) HIP_TRY(op, hipEventCreate(&op->pf_t1));
    }
    NdFactor *fs[ND_NF_MAX] = {nullptr, nullptr, nullptr, nullptr};
    auto drop = [&]() { for (int k = 0; k < n; ++k) { nd_free(fs[k]); fs[k] = nullptr; } };
    for (int k = 0; k < n; ++k) {
        fs[k] = new NdFactor();
        const int rc = nd_get_plan(ops[k], helm_tuning_now().nd_leaf, 1, &fs[k]->pd);
        if (rc) { drop(); return rc; }
    }
    const size_t wsb = (size_t)n * (size_t)nd_factor_ws_elems(fs[0]->pd->plan) * sizeof(cplx);
    void *ws = helm_pool_alloc(op0->device, wsb);
    if (!ws) { drop(); HELM_FAIL(op0, HELM_ERR_DEVICE, "direct solver: cannot allocate %.1f GB of factorisation scratch", wsb / 1e9); }
    if (n > 1) scratch_sweep(op0->device, false);           // (scratch of earlier sets whose factorisations have finished)
    timing_reset_events(op0);
    hipStream_t main = op0->stream;
    op0->stream = op0->fstream;                  // (the assembled planes of every operator are complete: helm_assemble synchronises)
    for (int k = 0; k < n; ++k) hipEventRecord(ops[k]->pf_t0, op0->fstream);
    const int rc = n == 1 ? nd_factor_enqueue(op0, 0, fs[0], (cplx *)ws, nullptr) : nd_factor_enqueue_many(op0, n, ops, fs, (cplx *)ws);
    for (int k = 0; k < n; ++k) { hipEventRecord(ops[k]->pf_t1, op0->fstream); hipEventRecord(ops[k]->pf_done, op0->fstream); }
    op0->stream = main;
    if (rc) { hipStreamSynchronize(op0->fstream); helm_pool_free(op0->device, ws, wsb); drop(); return rc; }
    scratch_defer(op0->device, op0->fstream, ws, wsb);
    for (int k = 0; k < n; ++k) {
        helm_op *op = ops[k];
        op->direct[0] = fs[k];
        op->pf_ws = nullptr; op->pf_ws_bytes = 0; op->pf_share = n; op->pf_pending = true;
    }
    return HELM_OK;
}

// The factorisations of n operators in the same launches (include/helm.h).  The elimination tree is geometry only, so the fronts of n frequencies ride in one
// strided batch each: the latency-bound chain at the top of the tree (88 block steps of ~30 us, the gather-bound small separator levels, products of one to
// four fronts that fill a quarter of the chip) is paid once per set instead of once per frequency.  Operators that do not qualify for the direct path's
// prefactorisation, or that differ in grid / device, are prefactored one by one (the call is a hint, like helm_prefactor).
extern "C" int helm_prefactor_many(helm_op **ops, int n) {
    helm_tuning_refresh();
    if (!ops || n < 1) return HELM_ERR_ARG;
    for (int k = 0; k < n; ++k) if (!ops[k]) return HELM_ERR_ARG;
    bool together = n >= 2 && n <= ND_NF_MAX && helm_tuning_now().nd_many != 0;
    for (int k = 0; k < n && together; ++k) {
        helm_op *op = ops[k];
        if (!direct_path_ok(op) || op->direct[0] || op->pf_pending || op->device != ops[0]->device || op->nz != ops[0]->nz || op->nx != ops[0]->nx || op->variant != ops[0]->variant || op->transposed != ops[0]->transposed) together = false;
        for (int j = 0; j < k; ++j) if (ops[j] == op) together = false;
    }
    if (together) return pf_enqueue(ops, n);
    for (int k = 0; k < n; ++k) { const int rc = helm_prefactor(ops[k]); if (rc) return rc; }
    return HELM_OK;
}

extern "C" int helm_prefactor_n(helm_op *op, int nrhs) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "operator not assembled");
    if (op->ny > 0) return prefactor3d(op, nrhs);
    return helm_prefactor(op);
}

extern "C" int helm_prefactor(helm_op *op) {
    helm_tuning_refresh();
    if (!op) return HELM_ERR_ARG;
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "operator not assembled");
    // a hint: only the single-block 2-D systems the direct path of HELM_AUTO / HELM_DIRECT factors once per frequency
    if (!direct_path_ok(op) || op->direct[0] || op->pf_pending) return HELM_OK;
    return pf_enqueue(&op, 1);
}
