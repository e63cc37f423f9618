// Host-side Krylov drivers of libhelm: BiCGSTAB on the Jacobi-scaled or multigrid-preconditioned system, CGNR as the safety net and for the
// coupled TTI system, with the kernels that only they launch: the fused vector updates (k_bicg_*, k_cg_*) and k_fin, the single-workgroup
// deterministic reduction of the partial sums that also advances the scalar recurrences.
//
// The drivers only enqueue kernels: all vectors and all scalar recurrences stay on the device;
// the host looks at the per-RHS status records every `check_every` iterations.
#include "solve_internal.hpp"
#include <algorithm>
#include <limits>

// ---- workspace ------------------------------------------------------------------------------
int ensure_ws(helm_op *op, size_t bytes) {
    if (op->ws_bytes >= bytes) return HELM_OK;
    // from the size-keyed pool: a job makes one operator per frequency and the Krylov workspace of a 3-D batch is tens of GB
    if (op->d_ws) { hipStreamSynchronize(op->stream); helm_pool_free(op->device, op->d_ws, op->ws_bytes); op->d_ws = nullptr; op->ws_bytes = 0; }
    op->d_ws = helm_pool_alloc(op->device, bytes);
    if (!op->d_ws) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the solver workspace (%.1f GB) failed", bytes / 1e9);
    op->ws_bytes = bytes;
    return HELM_OK;
}
int ensure_part(helm_op *op, int nrhs) {
    const int nblk = std::max(2 * helm_apply_num_blocks(op), helm_vec_num_blocks(op));
    const size_t bytes = (size_t)nrhs * 4 * nblk * sizeof(double) + (size_t)nrhs * (2 * sizeof(double) + sizeof(int)) + 256;
    if (op->part_bytes < bytes) {
        if (op->d_part) { hipStreamSynchronize(op->stream); helm_pool_free(op->device, op->d_part, op->part_bytes); op->d_part = nullptr; op->part_bytes = 0; }
        op->d_part = helm_pool_alloc(op->device, bytes);
        if (!op->d_part) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the partial-sum buffer failed");
        op->part_bytes = bytes;
    }
    if (op->scal_cap < nrhs) {
        if (op->d_scal || op->h_scal) hipStreamSynchronize(op->stream);
        helm_pool_free(op->device, op->d_scal, (size_t)op->scal_cap * sizeof(RhsScal));
        helm_hostpool_free(op->h_scal, op->h_scal_bytes);
        op->d_scal = nullptr; op->h_scal = nullptr; op->scal_cap = 0; op->h_scal_bytes = 0;
        op->d_scal = (RhsScal *)helm_pool_alloc(op->device, (size_t)nrhs * sizeof(RhsScal));
        const size_t hb = (size_t)nrhs * sizeof(RhsScal) + (size_t)nrhs * (2 * sizeof(double) + sizeof(int)) + 64;
        op->h_scal = (RhsScal *)helm_hostpool_alloc(hb);
        if (!op->d_scal || !op->h_scal) HELM_FAIL(op, HELM_ERR_DEVICE, "allocation of the per-right-hand-side records failed");
        op->h_scal_bytes = hb;
        op->scal_cap = nrhs;
    }
    return HELM_OK;
}

// ---- vector updates (grid.x over points with a grid-stride loop, grid.y = rhs) -----------------
namespace {

struct VecPtrs {   // all [nrhs][Nv] complex, stride Nv
    cplx *x, *r, *r0, *p, *v, *s, *t;
};

// BiCGSTAB / CGNR start: x = 0, r = r0 = bbar, p = v = 0, partial (r, r)
__global__ __launch_bounds__(256) void k_krylov_init(const cplx *__restrict__ bbar, VecPtrs w, long long N,
                                                     double *__restrict__ part, int nblk) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    double s[1] = {0.0};
    const cplx zero = cmake(0.0, 0.0);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        const cplx v = bbar[g];
        w.x[g] = zero; w.r[g] = v; w.r0[g] = v; w.p[g] = zero; w.v[g] = zero;
        s[0] += cabs2(v);
    }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) part[((long long)b * 4) * nblk + blockIdx.x] = s[0];
}

// p = r + beta (p - omega v)
__global__ __launch_bounds__(256) void k_bicg_p(VecPtrs w, long long N, const RhsScal *__restrict__ scal) {
    const int b = blockIdx.y;
    if (scal[b].status != ST_ACTIVE) return;
    const cplx beta = cmake(scal[b].beta_re, scal[b].beta_im), omega = cmake(scal[b].omega_re, scal[b].omega_im);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        const cplx r = w.r[g], p = w.p[g], v = w.v[g];
        cplx tmp = csub(p, cmul(omega, v));
        w.p[g] = cadd(r, cmul(beta, tmp));
    }
}

// s = r - alpha v
__global__ __launch_bounds__(256) void k_bicg_s(VecPtrs w, long long N, const RhsScal *__restrict__ scal) {
    const int b = blockIdx.y;
    if (scal[b].status != ST_ACTIVE) return;
    const cplx alpha = cmake(scal[b].alpha_re, scal[b].alpha_im);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        w.s[g] = csub(w.r[g], cmul(alpha, w.v[g]));
    }
}

// x += alpha p + omega s ; r = s - omega t ; partials (r0, r), (r, r)
__global__ __launch_bounds__(256) void k_bicg_xr(VecPtrs w, const cplx *__restrict__ xp, const cplx *__restrict__ xs, long long N,
                                                 const RhsScal *__restrict__ scal, double *__restrict__ part, int nblk) {
    __shared__ double red[12];
    const int b = blockIdx.y;
    if (scal[b].status != ST_ACTIVE) return;
    const cplx alpha = cmake(scal[b].alpha_re, scal[b].alpha_im), omega = cmake(scal[b].omega_re, scal[b].omega_im);
    double s[3] = {0.0, 0.0, 0.0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        const cplx sv = w.s[g], tv = w.t[g], pv = xp[g];
        const cplx sx = (xs == w.s) ? sv : xs[g];
        cplx xv = w.x[g];
        cfma(xv, alpha, pv);
        cfma(xv, omega, sx);
        w.x[g] = xv;
        const cplx rv = csub(sv, cmul(omega, tv));
        w.r[g] = rv;
        const cplx r0 = w.r0[g];
        s[0] += r0.x * rv.x + r0.y * rv.y;
        s[1] += r0.x * rv.y - r0.y * rv.x;
        s[2] += cabs2(rv);
    }
    block_sum<3>(s, red);
    if (threadIdx.x == 0) {
        double *pp = part + ((long long)b * 4) * nblk + blockIdx.x;
        pp[0] = s[0]; pp[(long long)nblk] = s[1]; pp[2LL * nblk] = s[2];
    }
}

// r0 = r, p = v = 0 for right-hand sides being (re)started (status == ST_ACTIVE after FIN_RESTART
// is decided by `mask[b]`)
__global__ __launch_bounds__(256) void k_restart_copy(VecPtrs w, long long N, const int *__restrict__ mask) {
    const int b = blockIdx.y;
    if (!mask[b]) return;
    const cplx zero = cmake(0.0, 0.0);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        w.r0[g] = w.r[g]; w.p[g] = zero; w.v[g] = zero;
    }
}

// CGNR: x += alpha p ; r -= alpha w(v) ; partial (r, r)
__global__ __launch_bounds__(256) void k_cg_xr(VecPtrs w, long long N, const RhsScal *__restrict__ scal,
                                               double *__restrict__ part, int nblk) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    if (scal[b].status != ST_ACTIVE) return;
    const double alpha = scal[b].alpha_re;
    double s[1] = {0.0};
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        const cplx pv = w.p[g], wv = w.v[g];
        cplx xv = w.x[g], rv = w.r[g];
        xv.x += alpha * pv.x; xv.y += alpha * pv.y;
        rv.x -= alpha * wv.x; rv.y -= alpha * wv.y;
        w.x[g] = xv; w.r[g] = rv;
        s[0] += cabs2(rv);
    }
    block_sum<1>(s, red);
    if (threadIdx.x == 0) part[((long long)b * 4) * nblk + blockIdx.x] = s[0];
}

// CGNR: p = z(s) + beta p
__global__ __launch_bounds__(256) void k_cg_p(VecPtrs w, long long N, const RhsScal *__restrict__ scal, int first) {
    const int b = blockIdx.y;
    if (scal[b].status != ST_ACTIVE) return;
    const double beta = first ? 0.0 : scal[b].beta_re;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const long long g = (long long)b * N + i;
        const cplx z = w.s[g];
        cplx p = first ? cmake(0.0, 0.0) : w.p[g];
        w.p[g] = cmake(z.x + beta * p.x, z.y + beta * p.y);
    }
}

// ------------------------------------------------------------------------------------------
// finalize: one workgroup per right-hand side sums the per-workgroup partials in a fixed order
// (bitwise reproducible) and advances the scalar recurrences.
// ------------------------------------------------------------------------------------------
__device__ inline void fin_sum(const double *part, int b, int nblk, double (&out)[4], double *smem) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nblk; i += blockDim.x) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] += part[((long long)b * 4 + q) * nblk + i];
    }
    block_sum<4>(v, smem);
    __shared__ double bc[4];
    if (threadIdx.x == 0) { bc[0] = v[0]; bc[1] = v[1]; bc[2] = v[2]; bc[3] = v[3]; }
    __syncthreads();
    out[0] = bc[0]; out[1] = bc[1]; out[2] = bc[2]; out[3] = bc[3];
}

struct FinParams {
    RhsScal *scal;
    const double *part;
    int nblk;
    int which;
    double rtol;
    const int *mask;    // FIN_RESTART: which RHS to touch
    double *aux;        // FIN_NORM: aux[b] = sum
};

__device__ inline bool finite2(cplx a) { return isfinite(a.x) && isfinite(a.y); }

__global__ __launch_bounds__(256) void k_fin(FinParams f) {
    __shared__ double smem[16];
    const int b = blockIdx.x;
    RhsScal *S = f.scal ? f.scal + b : nullptr;
    if (f.which == FIN_NORM || f.which == FIN_NORM2) {
        double v[4];
        fin_sum(f.part, b, f.nblk, v, smem);
        if (threadIdx.x == 0) { f.aux[b] = v[0]; if (f.which == FIN_NORM2) f.aux[gridDim.x + b] = v[1]; }
        return;
    }
    if (f.which == FIN_RESTART) {
        if (!f.mask[b]) {   // right-hand sides parked while others restart resume where they were
            if (threadIdx.x == 0 && S->status == ST_PARKED) S->status = ST_ACTIVE;
            return;
        }
    }
    else if (f.which != FIN_BICG_INIT && S->status != ST_ACTIVE) return;
    double v[4];
    fin_sum(f.part, b, f.nblk, v, smem);
    if (threadIdx.x != 0) return;

    switch (f.which) {
    case FIN_BICG_INIT: {           // v[0] = (b, b) of the scaled system
        S->bb = v[0]; S->rr = v[0];
        S->rho_re = v[0]; S->rho_im = 0.0;
        S->alpha_re = 1.0; S->alpha_im = 0.0; S->omega_re = 1.0; S->omega_im = 0.0;
        S->beta_re = 0.0; S->beta_im = 0.0;
        S->tol2 = f.rtol * f.rtol;
        S->iters = 0;
        S->pad0 = 0;                // restarts
        S->pad1 = 0;
        S->status = (v[0] == 0.0 || !isfinite(v[0])) ? ST_CONVERGED : ST_ACTIVE;
        break;
    }
    case FIN_RESTART: {             // v[0] = (r, r) of the recomputed true residual; r0 := r
        S->rr = v[0];
        S->rho_re = v[0]; S->rho_im = 0.0;
        S->alpha_re = 1.0; S->alpha_im = 0.0; S->omega_re = 1.0; S->omega_im = 0.0;
        S->beta_re = 0.0; S->beta_im = 0.0;
        S->pad0 += 1;
        S->status = (v[0] <= S->tol2 * S->bb) ? ST_CONVERGED : ST_ACTIVE;
        break;
    }
    case FIN_ALPHA: {               // sigma = (r0, v); alpha = rho / sigma
        const cplx sigma = cmake(v[0], v[1]);
        const cplx rho = cmake(S->rho_re, S->rho_im);
        const cplx alpha = cdiv(rho, sigma);
        if (cabs2(sigma) == 0.0 || !finite2(alpha)) { S->status = ST_BREAKDOWN; break; }
        S->alpha_re = alpha.x; S->alpha_im = alpha.y;
        break;
    }
    case FIN_OMEGA: {               // omega = (t, s) / (t, t)
        const double tt = v[2];
        cplx omega = cmake(0.0, 0.0);
        if (tt > 0.0) omega = cmake(v[0] / tt, v[1] / tt);
        if (!finite2(omega)) { S->status = ST_BREAKDOWN; break; }
        S->omega_re = omega.x; S->omega_im = omega.y;
        break;
    }
    case FIN_RHO: {                 // rho' = (r0, r); rr = (r, r); beta = (rho'/rho)(alpha/omega)
        const cplx rhon = cmake(v[0], v[1]);
        const double rr = v[2];
        S->iters += 1;
        S->rr = rr;
        if (!isfinite(rr) || !finite2(rhon)) { S->status = ST_BREAKDOWN; break; }
        if (rr <= S->tol2 * S->bb) { S->status = ST_CONVERGED; break; }
        const cplx rho = cmake(S->rho_re, S->rho_im);
        const cplx alpha = cmake(S->alpha_re, S->alpha_im), omega = cmake(S->omega_re, S->omega_im);
        if (cabs2(omega) == 0.0 || cabs2(rho) == 0.0 || cabs2(rhon) == 0.0) { S->status = ST_BREAKDOWN; break; }
        const cplx beta = cmul(cdiv(rhon, rho), cdiv(alpha, omega));
        if (!finite2(beta)) { S->status = ST_BREAKDOWN; break; }
        S->beta_re = beta.x; S->beta_im = beta.y;
        S->rho_re = rhon.x; S->rho_im = rhon.y;
        break;
    }
    case FIN_CG_INIT: {             // v[0] = (z, z)
        S->rho_re = v[0]; S->rho_im = 0.0;
        if (v[0] == 0.0) S->status = ST_CONVERGED;
        break;
    }
    case FIN_CG_ALPHA: {            // v[0] = (w, w); alpha = gamma / (w, w)
        if (v[0] == 0.0 || !isfinite(v[0])) { S->status = ST_BREAKDOWN; break; }
        S->alpha_re = S->rho_re / v[0]; S->alpha_im = 0.0;
        break;
    }
    case FIN_CG_RR: {               // v[0] = (r, r)
        S->iters += 1;
        S->rr = v[0];
        if (!isfinite(v[0])) { S->status = ST_BREAKDOWN; break; }
        if (v[0] <= S->tol2 * S->bb) S->status = ST_CONVERGED;
        break;
    }
    case FIN_CG_BETA: {             // v[0] = (z, z) new
        if (S->rho_re == 0.0) { S->status = ST_BREAKDOWN; break; }
        S->beta_re = v[0] / S->rho_re; S->beta_im = 0.0;
        S->rho_re = v[0];
        break;
    }
    default: break;
    }
}

void launch_fin(helm_op *op, int which, int nrhs, int nblk_part, const int *mask, double *aux, double rtol) {
    FinParams f; f.scal = op->d_scal; f.part = (const double *)op->d_part; f.nblk = nblk_part; f.which = which; f.rtol = rtol; f.mask = mask; f.aux = aux;
    HELM_LAUNCH(k_fin, dim3(nrhs), dim3(256), 0, op->stream, f);
}

// workgroups x right-hand sides of a vector update
dim3 vec_grid(const helm_op *op, int nrhs) { return dim3(vec_blocks(op->Nv), nrhs); }

// x = 0, r = r0 = bvec, p = v = 0 and the scalar records, for a system whose right-hand side is already formed
int launch_krylov_init(helm_op *op, const cplx *bvec, VecPtrs w, int nrhs, double rtol) {
    const dim3 grid = vec_grid(op, nrhs);
    HELM_LAUNCH(k_krylov_init, grid, dim3(256), 0, op->stream, bvec, w, op->Nv, (double *)op->d_part, (int)grid.x);
    launch_fin(op, FIN_BICG_INIT, nrhs, grid.x, nullptr, nullptr, rtol);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

void launch_cg_p(helm_op *op, VecPtrs w, int nrhs, int first) {      // p = z(s) + beta p
    HELM_LAUNCH(k_cg_p, vec_grid(op, nrhs), dim3(256), 0, op->stream, w, op->Nv, (const RhsScal *)op->d_scal, first);
}

// ---- Krylov drivers ---------------------------------------------------------------------------
struct Batch {
    int nrhs;
    VecPtrs w;
    cplx *bbar;          // right-hand side of the system being iterated (scaled q' or, with the MG preconditioner, q')
    cplx *bscaled = nullptr;                 // D^-1 q' (right-hand side of the Jacobi-scaled system; CGNR fallback)
    cplx *phat = nullptr, *shat = nullptr;   // preconditioned directions (MG mode)
    bool pre = false;    // true: BiCGSTAB on A right-preconditioned by multigrid; false: Jacobi-scaled system
    bool sys2 = false;   // coupled two-field Eurus system (vectors of length 2N, four stencil launches per apply)
    int nba = 0;         // partial sums written by one (system) apply
    const cplx *planes = nullptr;            // planes of the iterated operator (raw for pre, scaled otherwise)
    int *d_mask; double *d_aux;      // device, nrhs ints / 2*nrhs doubles (inside d_part tail)
    int *h_mask; double *h_aux;      // pinned (inside h_scal tail)
};

int download_scal(helm_op *op, int nrhs) {
    HIP_TRY(op, hipMemcpyAsync(op->h_scal, op->d_scal, (size_t)nrhs * sizeof(RhsScal), hipMemcpyDeviceToHost, op->stream));
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}
int upload_scal(helm_op *op, int nrhs) {
    HIP_TRY(op, hipMemcpyAsync(op->d_scal, op->h_scal, (size_t)nrhs * sizeof(RhsScal), hipMemcpyHostToDevice, op->stream));
    return HELM_OK;
}

ApplyArgs scaled_apply(helm_op *op, int block, const cplx *X, cplx *Y, const cplx *W, int nrhs, int adjoint, int epi, bool masked) {
    ApplyArgs a = ApplyArgs();
    a.planes = op->d_Cs + (long long)block * op->nplanes * op->N; a.X = X; a.Y = Y; a.W = W; a.ld = op->N; a.nrhs = nrhs;
    a.scaled = 1; a.adjoint = adjoint; a.epi = epi; a.scal = masked ? op->d_scal : nullptr; a.part = (double *)op->d_part;
    return a;
}

// apply of the operator the BiCGSTAB batch iterates on (Jacobi-scaled planes, or raw planes in MG mode)
ApplyArgs batch_apply(helm_op *op, const Batch &B, const cplx *X, cplx *Y, const cplx *W, int epi) {
    ApplyArgs a = ApplyArgs();
    a.planes = B.planes; a.X = X; a.Y = Y; a.W = W; a.ld = op->N; a.nrhs = B.nrhs;
    a.scaled = B.pre ? 0 : 1; a.adjoint = 0; a.epi = epi; a.scal = op->d_scal; a.part = (double *)op->d_part;
    return a;
}

}  // namespace

// (solve_internal.hpp)
int helm_launch_fin_ex(helm_op *op, int which, int nrhs, int nblk_part, const int *mask, double *aux) {
    launch_fin(op, which, nrhs, nblk_part, mask, aux, 0.0);
    return HELM_OK;
}

// (solve_internal.hpp)
int launch_sys2_apply(helm_op *op, bool raw, int adjoint, const cplx *X, cplx *Y, const cplx *W, int nrhs, int epi, const RhsScal *scal, const cplx *planes_override) {
    const long long N = op->N;
    const int nblk = helm_apply_num_blocks(op);
    const cplx *P = planes_override ? planes_override : (raw ? op->d_C : op->d_S);
    if (epi == EPI_DOT_XY) { epi = EPI_DOT_WY; W = X; }
    for (int half = 0; half < 2; ++half) {
        // forward: out_half = M[half][0] in0 + M[half][1] in1 ; adjoint: out_half = M[0][half]^H in0 + M[1][half]^H in1
        const int blkA = adjoint ? (0 * 2 + half) : (half * 2 + 0), blkB = adjoint ? (1 * 2 + half) : (half * 2 + 1);
        ApplyArgs a = ApplyArgs();
        a.ld = 2 * N; a.nrhs = nrhs; a.scal = scal; a.part = (double *)op->d_part; a.part_stride = 2 * nblk; a.adjoint = adjoint; a.scaled = 0;
        a.planes = P + (long long)blkA * 9 * N; a.X = X; a.Y = Y + half * N; a.epi = EPI_NONE; a.profile = 0;
        int rc = helm_launch_apply(op, a);
        if (rc) return rc;
        a.planes = P + (long long)blkB * 9 * N; a.X = X + N; a.acc = 1; a.epi = epi; a.W = W ? W + half * N : nullptr; a.part_off = half * nblk; a.profile = 1;
        rc = helm_launch_apply(op, a);
        if (rc) return rc;
    }
    return HELM_OK;
}

namespace {

int launch_batch_apply(helm_op *op, const Batch &B, const cplx *X, cplx *Y, const cplx *W, int epi) {
    if (B.sys2) return launch_sys2_apply(op, false, 0, X, Y, W, B.nrhs, epi, op->d_scal);
    return helm_launch_apply(op, batch_apply(op, B, X, Y, W, epi));
}

// Restart the right-hand sides flagged in h_mask from their current iterate x:
// r = bbar - Abar x, r0 = r, p = v = 0, scalars reset.  Host copy of scal must be fresh.
int restart_masked(helm_op *op, int block, Batch &B) {
    const int n = B.nrhs;
    for (int b = 0; b < n; ++b) {
        if (B.h_mask[b]) op->h_scal[b].status = ST_ACTIVE;
        else if (op->h_scal[b].status == ST_ACTIVE) op->h_scal[b].status = ST_PARKED;
    }
    int rc = upload_scal(op, n);
    if (rc) return rc;
    HIP_TRY(op, hipMemcpyAsync(B.d_mask, B.h_mask, n * sizeof(int), hipMemcpyHostToDevice, op->stream));
    rc = launch_batch_apply(op, B, B.w.x, B.w.r, B.bbar, EPI_RESID);
    if (rc) return rc;
    HELM_LAUNCH(k_restart_copy, vec_grid(op, n), dim3(256), 0, op->stream, B.w, op->Nv, (const int *)B.d_mask);
    helm_launch_fin_ex(op, FIN_RESTART, n, B.nba, B.d_mask, nullptr);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int run_bicgstab(helm_op *op, int block, Batch &B, int maxit, int check_every, int max_restarts, std::vector<int> &restarts) {
    const int n = B.nrhs;
    const int nba = B.nba, nbv = helm_vec_num_blocks(op);
    const dim3 vgrid = vec_grid(op, n);
    const RhsScal *scal = op->d_scal;
    int it_done = 0;
    while (true) {
        int rc = download_scal(op, n);
        if (rc) return rc;
        bool any_active = false, any_break = false;
        int min_iters = std::numeric_limits<int>::max();
        int nactive = 0;
        for (int b = 0; b < n; ++b) {
            B.h_mask[b] = 0;
            RhsScal &S = op->h_scal[b];
            if (S.status == ST_ACTIVE) {
                if (S.iters >= maxit) S.status = ST_FROZEN;   // iteration cap: stop working on it
                else { any_active = true; nactive += 1; min_iters = std::min(min_iters, S.iters); }
            } else if (S.status == ST_BREAKDOWN && restarts[b] < max_restarts && S.iters < maxit) {
                B.h_mask[b] = 1; any_break = true; restarts[b] += 1;
            }
        }
        if (any_break) {
            rc = restart_masked(op, block, B);
            if (rc) return rc;
            continue;     // re-read the status (a restarted RHS may already satisfy the tolerance)
        }
        if (!any_active) {
            // un-freeze bookkeeping for the caller: frozen-by-cap stays FROZEN
            upload_scal(op, n);
            break;
        }
        upload_scal(op, n);
        op->active_hint = nactive;
        const int chunk = std::max(1, std::min(check_every, maxit - min_iters));
        for (int k = 0; k < chunk; ++k) {
            HELM_LAUNCH(k_bicg_p, vgrid, dim3(256), 0, op->stream, B.w, op->Nv, scal);
            const cplx *pin = B.w.p, *sin = B.w.s;
            if (B.pre) { rc = mg_apply(op, B.w.p, B.phat, n, op->d_scal); if (rc) return rc; pin = B.phat; }
            rc = launch_batch_apply(op, B, pin, B.w.v, B.w.r0, EPI_DOT_W);
            if (rc) return rc;
            helm_launch_fin_ex(op, FIN_ALPHA, n, nba);
            HELM_LAUNCH(k_bicg_s, vgrid, dim3(256), 0, op->stream, B.w, op->Nv, scal);
            if (B.pre) {
                rc = mg_apply(op, B.w.s, B.shat, n, op->d_scal); if (rc) return rc; sin = B.shat;
                rc = launch_batch_apply(op, B, sin, B.w.t, B.w.s, EPI_DOT_WY);
            } else {
                rc = launch_batch_apply(op, B, sin, B.w.t, nullptr, EPI_DOT_XY);
            }
            if (rc) return rc;
            helm_launch_fin_ex(op, FIN_OMEGA, n, nba);
            HELM_LAUNCH(k_bicg_xr, vgrid, dim3(256), 0, op->stream, B.w, pin, sin, op->Nv, scal, (double *)op->d_part, nbv);      // x += alpha pin + omega sin ; r = s - omega t
            helm_launch_fin_ex(op, FIN_RHO, n, nbv);
        }
        HIP_TRY(op, hipGetLastError());
        it_done += chunk;
    }
    op->active_hint = -1;
    return HELM_OK;
}

// CGNR on the Jacobi-scaled system for the right-hand sides flagged in h_mask (warm start from x).
int run_cgnr(helm_op *op, int block, Batch &B, int maxit, int check_every) {
    const int n = B.nrhs;
    const int nba = B.nba, nbv = helm_vec_num_blocks(op);
    // r = bbar - Abar x for flagged RHS; others frozen
    for (int b = 0; b < n; ++b) {
        RhsScal &S = op->h_scal[b];
        if (B.h_mask[b]) { S.status = ST_ACTIVE; S.iters = 0; }
        else if (S.status == ST_ACTIVE) S.status = ST_FROZEN;
    }
    int rc = upload_scal(op, n);
    if (rc) return rc;
    auto cg_apply = [&](const cplx *X, cplx *Y, const cplx *W, int adjoint, int epi) -> int {
        if (B.sys2) return launch_sys2_apply(op, false, adjoint, X, Y, W, n, epi, op->d_scal);
        return helm_launch_apply(op, scaled_apply(op, block, X, Y, W, n, adjoint, epi, true));
    };
    rc = cg_apply(B.w.x, B.w.r, B.bscaled, 0, EPI_RESID);
    if (rc) return rc;
    helm_launch_fin_ex(op, FIN_CG_RR, n, nba);            // rr (and convergence check); iters becomes 1
    rc = cg_apply(B.w.r, B.w.s, nullptr, 1, EPI_DOT_YY);   // z = A^H r
    if (rc) return rc;
    helm_launch_fin_ex(op, FIN_CG_INIT, n, nba);
    launch_cg_p(op, B.w, n, 1);
    while (true) {
        rc = download_scal(op, n);
        if (rc) return rc;
        bool any_active = false;
        int min_iters = std::numeric_limits<int>::max();
        for (int b = 0; b < n; ++b) {
            RhsScal &S = op->h_scal[b];
            if (S.status == ST_ACTIVE) {
                if (S.iters >= maxit) S.status = ST_FROZEN;
                else { any_active = true; min_iters = std::min(min_iters, S.iters); }
            }
        }
        upload_scal(op, n);
        if (!any_active) break;
        const int chunk = std::max(1, std::min(check_every, maxit - min_iters));
        for (int k = 0; k < chunk; ++k) {
            rc = cg_apply(B.w.p, B.w.v, nullptr, 0, EPI_DOT_YY);   // w = A p
            if (rc) return rc;
            helm_launch_fin_ex(op, FIN_CG_ALPHA, n, nba);
            HELM_LAUNCH(k_cg_xr, vec_grid(op, n), dim3(256), 0, op->stream, B.w, op->Nv, (const RhsScal *)op->d_scal, (double *)op->d_part, nbv);
            helm_launch_fin_ex(op, FIN_CG_RR, n, nbv);
            rc = cg_apply(B.w.r, B.w.s, nullptr, 1, EPI_DOT_YY); // z = A^H r
            if (rc) return rc;
            helm_launch_fin_ex(op, FIN_CG_BETA, n, nba);
            launch_cg_p(op, B.w, n, 0);
        }
        HIP_TRY(op, hipGetLastError());
    }
    return HELM_OK;
}

// the right-hand sides whose BiCGSTAB run ended in a breakdown (with_frozen: or at its iteration cap) flagged in h_mask; is there one?
// Host copy of scal must be fresh.
bool mask_failed(helm_op *op, Batch &B, bool with_frozen) {
    bool any = false;
    for (int b = 0; b < B.nrhs; ++b) {
        const int st = op->h_scal[b].status;
        B.h_mask[b] = (st == ST_BREAKDOWN || (with_frozen && st == ST_FROZEN));
        any = any || B.h_mask[b];
    }
    return any;
}

}  // namespace

int solve_block_krylov(helm_op *op, int block, const cplx *dRHS, long long rhs_ld, long long row_off, cplx premul, const cplx *sub, cplx *dXout, int nrhs,
                       const helm_solve_opts &o, helm_solve_info *info, int sys2, long long rows_in) {
    const long long N = op->N;
    const long long NV = sys2 ? 2 * N : N;
    NvGuard guard(op, NV);
    { const int rcs = helm_ensure_scaled(op); if (rcs) return rcs; }
    int Bmax = o.batch > 0 ? o.batch : 16;
    if (Bmax > nrhs) Bmax = nrhs;
    int rc = ensure_ws(op, (size_t)11 * Bmax * NV * sizeof(cplx));
    if (rc) return rc;
    if (sys2) {
        // the coupled TTI system is only tractable by the normal-equations method on the row-equilibrated system
        if (o.method == HELM_MG || o.method == HELM_BICGSTAB) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the coupled TTI system (eps != delta) is solved with row-equilibrated CGNR only (method 'auto' or 'cgnr')");
        rc = helm_launch_rowscaled_system(op);
        if (rc) return rc;
    }
    rc = ensure_part(op, Bmax);
    if (rc) return rc;
    // preconditioner choice: multigrid for the main block when asked for (or AUTO on Eurus, where it is validated)
    bool use_mg = false;
    const int auto_mg3 = helm_tuning_now().auto_mg3;
    const bool mg3_ok = op->ny > 0 && (o.method == HELM_MG || (o.method == HELM_AUTO && auto_mg3 && std::min(op->nz, std::min(op->ny, op->nx)) >= 24));
    if (!sys2 && block == 0 && (mg3_ok || (op->ny == 0 && (o.method == HELM_MG || (o.method == HELM_AUTO && std::min(op->nz, op->nx) >= 32))))) {
        op->mg3_rhs_hint = nrhs;
        rc = mg_setup(op, Bmax);
        if (rc == HELM_OK) use_mg = true;
        else if (o.method == HELM_MG) return rc;
    }
    // (an iteration of the layer-preserving 3-D cycle costs tens of milliseconds and ten of them are a whole solve: poll after every one)
    auto pick_check_every = [&]() { return o.check_every > 0 ? o.check_every : (use_mg && op->ny > 0 && mg3_is_layer_preserving(op) ? 1 : (use_mg ? 10 : 50)); };
    int check_every = pick_check_every();
    int unconverged = 0;
    for (int first = 0; first < nrhs; first += Bmax) {
        const int n = std::min(Bmax, nrhs - first);
        Batch B;
        B.nrhs = n;
        cplx *base = (cplx *)op->d_ws;
        const long long vs = (long long)Bmax * NV;
        B.sys2 = sys2 != 0;
        B.nba = (sys2 ? 2 : 1) * helm_apply_num_blocks(op);
        B.w.x = base; B.w.r = base + vs; B.w.r0 = base + 2 * vs; B.w.p = base + 3 * vs; B.w.v = base + 4 * vs;
        B.w.s = base + 5 * vs; B.w.t = base + 6 * vs; B.bscaled = base + 7 * vs;
        cplx *qprime = base + 8 * vs;
        B.phat = base + 9 * vs; B.shat = base + 10 * vs;
        B.pre = use_mg;
        B.bbar = use_mg ? qprime : B.bscaled;
        B.planes = use_mg ? op->d_C + (long long)block * op->nplanes * N : op->d_Cs + (long long)block * op->nplanes * N;
        const int nblk = std::max(2 * helm_apply_num_blocks(op), helm_vec_num_blocks(op));
        char *ptail = (char *)op->d_part + (size_t)Bmax * 4 * nblk * sizeof(double);
        B.d_aux = (double *)ptail; B.d_mask = (int *)(ptail + (size_t)Bmax * 2 * sizeof(double));
        char *htail = (char *)op->h_scal + (size_t)op->scal_cap * sizeof(RhsScal);
        B.h_aux = (double *)htail; B.h_mask = (int *)(htail + (size_t)op->scal_cap * 2 * sizeof(double));

        const cplx *rhs_b = dRHS + (long long)first * rhs_ld;
        const cplx *sub_b = sub ? sub + (long long)first * N : nullptr;
        // q' = premul*rhs - sub (unscaled), ||q'||^2 -> aux[n..2n)
        if (sys2) {
            HIP_TRY(op, hipMemsetAsync(qprime, 0, (size_t)n * NV * sizeof(cplx), op->stream));
            HIP_TRY(op, hipMemsetAsync(B.bscaled, 0, (size_t)n * NV * sizeof(cplx), op->stream));
            for (int half = 0; half < (rows_in == 2 * N ? 2 : 1); ++half) {
                rc = helm_launch_prep_rhs(op, rhs_b, rhs_ld, half * N, premul, nullptr, nullptr, nullptr, qprime, NV, half * N, n);
                if (rc) return rc;
                rc = helm_launch_prep_rhs(op, rhs_b, rhs_ld, half * N, premul, nullptr, nullptr, op->d_rs + half * N, B.bscaled, NV, half * N, n);
                if (rc) return rc;
            }
        } else {
            rc = helm_launch_prep_rhs(op, rhs_b, rhs_ld, row_off, premul, sub_b, nullptr, nullptr, qprime, N, 0, n);
            if (rc) return rc;
        }
        helm_launch_norm2(op, qprime, n);
        helm_launch_fin_ex(op, FIN_NORM, n, helm_vec_num_blocks(op), nullptr, B.d_aux + n);
        // scaled system start
        if (sys2) {
            rc = launch_krylov_init(op, B.bscaled, B.w, n, o.rtol * 0.5);
            if (rc) return rc;
        } else {
            VecPtrs w = B.w;
            w.t = B.bscaled;   // prep writes the scaled right-hand side D^-1 q' through w.t; the init reads it there and leaves t alone
            // NB: row offset is applied by giving prep a shifted base pointer
            rc = helm_launch_prep_rhs(op, rhs_b + row_off, rhs_ld, 0, premul, sub_b, op->d_dinv + (long long)block * N, nullptr, w.t, N, 0, n);
            if (rc) return rc;
            rc = launch_krylov_init(op, w.t, w, n, o.rtol * 0.5);
            if (rc) return rc;
            if (use_mg) {      // iterate on the unscaled system A (M^-1 y) = q'
                rc = launch_krylov_init(op, qprime, B.w, n, o.rtol * 0.9);
                if (rc) return rc;
            }
        }
        std::vector<int> restarts(n, 0), refinements(n, 0);     // after a breakdown (at most 25) / for a refinement round (at most max_refine)
        std::vector<int> method_used(n, (o.method == HELM_CGNR || sys2) ? HELM_CGNR : (use_mg ? HELM_MG : HELM_BICGSTAB));
        std::vector<int> total_iters(n, 0);
        std::vector<double> relres(n, 0.0);
        const int max_refine = 3;
        for (int round = 0; round <= max_refine; ++round) {
            if (o.method == HELM_CGNR || sys2) {
                rc = download_scal(op, n);
                if (rc) return rc;
                bool any = false;
                for (int b = 0; b < n; ++b) { B.h_mask[b] = (op->h_scal[b].status == ST_ACTIVE); any = any || B.h_mask[b]; }
                if (any) { rc = run_cgnr(op, block, B, o.maxit, check_every); if (rc) return rc; }
            } else {
                // in AUTO mode a preconditioned run that has not converged after 5000 iterations is handed to CGNR
                int cap = (use_mg && o.method == HELM_AUTO) ? std::min(o.maxit, 5000) : o.maxit;
                // the layer-preserving 3-D hierarchy needs tens of iterations; if it has not converged after 300 (test hook: HELM_MG3_KEEP_CAP) the
                // frequency retreats to the standard cycle and goes on from the iterates reached
                const bool keep3 = use_mg && op->ny > 0 && mg3_is_layer_preserving(op);
                // (first round only: the retreat below is what the cap is for, and it is taken there)
                if (keep3 && round == 0) { const int hook = testing_hook("HELM_MG3_KEEP_CAP"); cap = std::min(cap, hook > 0 ? hook : 300); }
                rc = run_bicgstab(op, block, B, cap, check_every, 25, restarts);
                if (rc) return rc;
                if (keep3 && round == 0) {
                    rc = download_scal(op, n);
                    if (rc) return rc;
                    if (mask_failed(op, B, true)) {
                        rc = mg3_retreat(op, Bmax);
                        if (rc) return rc;
                        check_every = pick_check_every();          // the standard cycle needs hundreds of iterations: poll every 10, not every one
                        rc = restart_masked(op, block, B);
                        if (rc) return rc;
                        rc = run_bicgstab(op, block, B, o.method == HELM_AUTO ? std::min(o.maxit, 5000) : o.maxit, check_every, 25, restarts);
                        if (rc) return rc;
                    }
                }
                if (o.method == HELM_AUTO && use_mg && round == 0 && op->ny == 0) {      // (no adjoint apply, hence no CGNR, in 3-D)
                    rc = download_scal(op, n);
                    if (rc) return rc;
                    if (mask_failed(op, B, true)) {     // safety net: Jacobi-scaled CGNR from the current iterate
                        helm_launch_norm2(op, B.bscaled, n);
                        helm_launch_fin_ex(op, FIN_NORM, n, helm_vec_num_blocks(op), nullptr, B.d_aux);
                        HIP_TRY(op, hipMemcpyAsync(B.h_aux, B.d_aux, n * sizeof(double), hipMemcpyDeviceToHost, op->stream));
                        HIP_TRY(op, hipStreamSynchronize(op->stream));
                        for (int b = 0; b < n; ++b) if (B.h_mask[b]) {
                            RhsScal &S = op->h_scal[b];
                            total_iters[b] += S.iters; method_used[b] = HELM_CGNR;
                            S.bb = B.h_aux[b]; S.tol2 = 0.25 * o.rtol * o.rtol;
                        }
                        rc = run_cgnr(op, block, B, o.maxit, 50);
                        if (rc) return rc;
                    }
                }
                if (o.method == HELM_AUTO && !use_mg && !sys2) {
                    rc = download_scal(op, n);
                    if (rc) return rc;
                    const bool any = mask_failed(op, B, false);
                    for (int b = 0; b < n; ++b) if (B.h_mask[b]) { method_used[b] = HELM_CGNR; total_iters[b] += op->h_scal[b].iters; }
                    if (any) { rc = run_cgnr(op, block, B, o.maxit, check_every); if (rc) return rc; }
                }
            }
            // true residual of the UNSCALED system: s = q' - A x
            if (sys2) {
                rc = launch_sys2_apply(op, true, 0, B.w.x, B.w.s, qprime, n, EPI_RESID, nullptr);
            } else {
                ApplyArgs a = ApplyArgs();
                a.planes = op->d_C + (long long)block * op->nplanes * N; a.X = B.w.x; a.Y = B.w.s; a.W = qprime; a.ld = N; a.nrhs = n;
                a.scaled = 0; a.adjoint = 0; a.epi = EPI_RESID; a.scal = nullptr; a.part = (double *)op->d_part;
                rc = helm_launch_apply(op, a);
            }
            if (rc) return rc;
            helm_launch_fin_ex(op, FIN_NORM, n, B.nba, nullptr, B.d_aux);
            HIP_TRY(op, hipMemcpyAsync(B.h_aux, B.d_aux, 2 * n * sizeof(double), hipMemcpyDeviceToHost, op->stream));
            rc = download_scal(op, n);
            if (rc) return rc;
            bool refine = false;
            for (int b = 0; b < n; ++b) {
                const double qq = B.h_aux[n + b];
                relres[b] = qq > 0 ? sqrt(B.h_aux[b] / qq) : 0.0;
                B.h_mask[b] = 0;
                RhsScal &S = op->h_scal[b];
                if (S.status == ST_CONVERGED && relres[b] > o.rtol && round < max_refine && S.iters < o.maxit) {
                    // the scaled criterion was met but the unscaled residual is not there yet: tighten and go on
                    const double f = std::max(1e-3, 0.3 * o.rtol / relres[b]);
                    S.tol2 *= f * f;
                    B.h_mask[b] = 1; refine = true;
                }
            }
            if (!refine) break;
            if (o.method == HELM_CGNR || sys2) {
                // (run_cgnr counts every round from zero: what the finished round used goes to the total here)
                for (int b = 0; b < n; ++b) if (B.h_mask[b]) { total_iters[b] += op->h_scal[b].iters; op->h_scal[b].status = ST_ACTIVE; }
                upload_scal(op, n);
            } else {
                for (int b = 0; b < n; ++b) if (B.h_mask[b]) refinements[b] += 1;      // a restart like those after a breakdown: helm_solve_info.restarts counts it
                rc = restart_masked(op, block, B);
                if (rc) return rc;
            }
        }
        // results
        for (int b = 0; b < n; ++b) {
            const RhsScal &S = op->h_scal[b];
            if (!(relres[b] <= o.rtol * 1.0000001)) unconverged += 1;
            if (info) {
                helm_solve_info &I = info[first + b];
                I.iterations += total_iters[b] + S.iters;
                I.restarts += restarts[b] + refinements[b];
                I.method = method_used[b];
                I.relres = std::max(I.relres, relres[b]);
                const int st = (relres[b] <= o.rtol * 1.0000001) ? 0 : (S.status == ST_BREAKDOWN ? 2 : 1);
                I.status = merge_status(I.status, st);
            }
        }
        HIP_TRY(op, hipMemcpyAsync(dXout + (long long)first * NV, B.w.x, (size_t)n * NV * sizeof(cplx), hipMemcpyDeviceToDevice, op->stream));
        HIP_TRY(op, hipStreamSynchronize(op->stream));
        if (use_mg && op->ny > 0 && mg3_is_layer_preserving(op)) {      // what this class of hierarchy needed: the depth model's book
            double sum = 0.0;
            for (int b = 0; b < n; ++b) sum += total_iters[b] + op->h_scal[b].iters;
            mg3_record_iterations(op, sum / n, o.rtol);
        }
    }
    return unconverged;
}
