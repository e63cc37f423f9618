// Multigrid preconditioners for the 3-D 27-point operator (right-preconditioned BiCGSTAB of krylov.hip): the entry points of helm_internal.hpp,
// the standard hierarchy's set-up and both cycles with every kernel they launch.
// 1. Standard cycle (grids below 20 points per wavelength, fallback): one V(1,1) cycle on the
//    complex-shifted operator (1/tau_M = 1/tau + omega beta / 2) with a weak absorbing layer (cPML_M), rediscretised on coarser
//    grids (model by injection, spacing doubled, layer thickness halved), damped Jacobi smoothing through the 3-D stencil
//    kernel, full-weighting restriction / trilinear prolongation, dense inverse on the coarsest grid (dense kernels of direct.hpp).
// 2. Layer-preserving hierarchy (oversampled grids such as BASELINE config 5): coarse grids keep every node of the
//    absorbing layers, l1-Jacobi, true layer with a small shift, direct solve of the level that still has ~10 points per wavelength.
//    mg3_keep.hip builds it, mg3_coarse.hip solves its last level, mg3_depth.hip says how deep it goes; DESIGN.md section 6: the measurements.
#include "mg3_internal.hpp"
#include <cstdlib>

bool mg3_trace() { const char *v = getenv("HELM_MG3_TRACE"); return v && atoi(v) != 0; }
size_t mg3_available_bytes(int device, size_t *total) {
    size_t freeb = 0, totb = 0;
    hipMemGetInfo(&freeb, &totb);
    if (total) *total = totb;
    return freeb + helm_pool_idle_bytes(device);
}

// the four work vectors of a level ([batch][N] each) come from the size-keyed buffer pool: the next frequency's hierarchy has the same shapes
bool mg3_level_vectors(helm_op *op, Mg3Level &L, int batch) {
    L.vbytes = (size_t)batch * L.N * sizeof(cplx);
    cplx **v[4] = {&L.u, &L.f, &L.r, &L.t};
    for (int i = 0; i < 4; ++i) { *v[i] = (cplx *)helm_pool_alloc(op->device, L.vbytes); if (!*v[i]) return false; }
    return true;
}

namespace {

// the hierarchy goes back, whichever kind it is: a level's vectors to the pool, its operator (which borrowed the handle's stream) destroyed
void hierarchy_free(helm_op *op, Mg3Precond *P) {
    mg3_keep_free(P);
    for (Mg3Level &L : P->lv) {
        cplx **v[4] = {&L.u, &L.f, &L.r, &L.t};
        for (int i = 0; i < 4; ++i) { if (*v[i]) helm_pool_free(op->device, *v[i], L.vbytes); *v[i] = nullptr; }
        if (L.op) { L.op->own_stream = false; L.op->stream = nullptr; helm_destroy(L.op); }
    }
    P->lv.clear();
}

template <class TU>
__global__ void k3_jac0(const cplx *__restrict__ f, const cplx *__restrict__ dinv, TU *__restrict__ u, long long N, double w) {
    const cplx *fb = f + (long long)blockIdx.y * N; TU *ub = u + (long long)blockIdx.y * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x)
        ub[i] = vfrom<TU>(cmul(cscale(dinv[i], w), fb[i]));
}
__device__ __forceinline__ cplx mg_cvt64(cplx a) { return a; }
__device__ __forceinline__ cplx mg_cvt64(cplxf a) { return to_f64(a); }

// coarse = R fine, R = P^T / 8 (full weighting; weights 1, 1/2, 1/4, 1/8 by distance class, fine points outside the grid skipped)
__global__ void k3_restrict(const cplx *__restrict__ fine, cplx *__restrict__ coarse, int nz, int ny, int nx, int nzc, int nyc, int nxc) {
    const long long Nf = (long long)nz * ny * nx, Nc = (long long)nzc * nyc * nxc;
    const cplx *fb = fine + (long long)blockIdx.y * Nf; cplx *cb = coarse + (long long)blockIdx.y * Nc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Nc; i += (long long)gridDim.x * blockDim.x) {
        const int X = (int)(i % nxc), Y = (int)((i / nxc) % nyc), Z = (int)(i / ((long long)nxc * nyc));
        cplx acc = cmake(0.0, 0.0);
        for (int dz = -1; dz <= 1; ++dz) { const int z = 2 * Z + dz; if (z < 0 || z >= nz) continue;
            for (int dy = -1; dy <= 1; ++dy) { const int y = 2 * Y + dy; if (y < 0 || y >= ny) continue;
                for (int dx = -1; dx <= 1; ++dx) { const int x = 2 * X + dx; if (x < 0 || x >= nx) continue;
                    const double w = (dz ? 0.5 : 1.0) * (dy ? 0.5 : 1.0) * (dx ? 0.5 : 1.0) * 0.125;
                    const cplx v = fb[((long long)z * ny + y) * nx + x];
                    acc.x += w * v.x; acc.y += w * v.y;
                } } }
        cb[i] = acc;
    }
}

// fine += P coarse (trilinear)
__global__ void k3_prolong_add(const cplx *__restrict__ coarse, cplx *__restrict__ fine, int nz, int ny, int nx, int nzc, int nyc, int nxc) {
    const long long Nf = (long long)nz * ny * nx, Nc = (long long)nzc * nyc * nxc;
    cplx *fb = fine + (long long)blockIdx.y * Nf; const cplx *cb = coarse + (long long)blockIdx.y * Nc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Nf; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((long long)nx * ny));
        const int X = x >> 1, Y = y >> 1, Z = z >> 1;
        const int ox = x & 1, oy = y & 1, oz = z & 1;
        cplx acc = cmake(0.0, 0.0);
        for (int a = 0; a <= oz; ++a) { const int ZZ = Z + a; if (ZZ >= nzc) continue;
            for (int b = 0; b <= oy; ++b) { const int YY = Y + b; if (YY >= nyc) continue;
                for (int c = 0; c <= ox; ++c) { const int XX = X + c; if (XX >= nxc) continue;
                    const double w = (oz ? 0.5 : 1.0) * (oy ? 0.5 : 1.0) * (ox ? 0.5 : 1.0);
                    const cplx v = cb[((long long)ZZ * nyc + YY) * nxc + XX];
                    acc.x += w * v.x; acc.y += w * v.y;
                } } }
        fb[i] = cadd(fb[i], acc);
    }
}

// dense row-major matrix of the 27-plane operator (coarsest level)
__global__ void k3_dense(const cplx *__restrict__ planes, cplx *__restrict__ A, int nz, int ny, int nx) {
    const long long N = (long long)nz * ny * nx;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((long long)nx * ny));
        for (int k = 0; k < 27; ++k) {
            const int z2 = z + k / 9 - 1, y2 = y + (k / 3) % 3 - 1, x2 = x + k % 3 - 1;
            if (z2 < 0 || z2 >= nz || y2 < 0 || y2 >= ny || x2 < 0 || x2 >= nx) continue;
            A[i * N + ((long long)z2 * ny + y2) * nx + x2] = planes[(long long)k * N + i];
        }
    }
}

__global__ void k3_transpose_sq(const cplx *__restrict__ A, cplx *__restrict__ T, int n) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < (long long)n * n; e += (long long)gridDim.x * blockDim.x)
        T[(e % n) * n + e / n] = A[e];
}

inline dim3 vgrid(long long N, int nrhs) { return dim3((unsigned)std::min<long long>((N + 255) / 256, 16384), nrhs); }

template <typename T> std::vector<T> inject3(const std::vector<T> &a, int nz, int ny, int nx) {
    const int nzc = (nz + 1) / 2, nyc = (ny + 1) / 2, nxc = (nx + 1) / 2;
    std::vector<T> out((size_t)nzc * nyc * nxc);
    for (int Z = 0; Z < nzc; ++Z) for (int Y = 0; Y < nyc; ++Y) for (int X = 0; X < nxc; ++X)
        out[((size_t)Z * nyc + Y) * nxc + X] = a[((size_t)(2 * Z) * ny + 2 * Y) * nx + 2 * X];
    return out;
}

// (TF: element type of the fine vector -- complex64 for the finest level of a cycle that keeps its work vectors in single precision)
template <class TF>
__global__ void k3_restrict_t(const TF *__restrict__ fine, cplx *__restrict__ coarse, int ny, int nx, int nzc, int nyc, int nxc, long long Nf,
                              const RTab *__restrict__ tz, const RTab *__restrict__ ty, const RTab *__restrict__ tx) {
    const long long Nc = (long long)nzc * nyc * nxc;
    const TF *fb = fine + (long long)blockIdx.y * Nf; cplx *cb = coarse + (long long)blockIdx.y * Nc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Nc; i += (long long)gridDim.x * blockDim.x) {
        const int X = (int)(i % nxc), Y = (int)((i / nxc) % nyc), Z = (int)(i / ((long long)nxc * nyc));
        const RTab rz = tz[Z], ry = ty[Y], rx = tx[X];
        const double wz[3] = {rz.wl, rz.wc, rz.wr}, wy[3] = {ry.wl, ry.wc, ry.wr}, wx[3] = {rx.wl, rx.wc, rx.wr};
        cplx acc = cmake(0.0, 0.0);
        for (int a = 0; a < 3; ++a) { if (wz[a] == 0.0) continue;
            for (int b = 0; b < 3; ++b) { if (wy[b] == 0.0) continue;
                const double wab = wz[a] * wy[b];
                const TF *row = fb + ((long long)(rz.f + a - 1) * ny + (ry.f + b - 1)) * nx + rx.f;
                for (int c = 0; c < 3; ++c) { if (wx[c] == 0.0) continue;
                    const cplx v = mg_cvt64(row[c - 1]);
                    const double w = wab * wx[c];
                    acc.x += w * v.x; acc.y += w * v.y;
                } } }
        cb[i] = acc;
    }
}

template <class TF>
__global__ void k3_prolong_add_t(const cplx *__restrict__ coarse, TF *__restrict__ fine, int nz, int ny, int nx, int nyc, int nxc, long long Nc,
                                 const PTab *__restrict__ tz, const PTab *__restrict__ ty, const PTab *__restrict__ tx) {
    const long long Nf = (long long)nz * ny * nx;
    TF *fb = fine + (long long)blockIdx.y * Nf; const cplx *cb = coarse + (long long)blockIdx.y * Nc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Nf; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % nx), y = (int)((i / nx) % ny), z = (int)(i / ((long long)nx * ny));
        const PTab pz = tz[z], py = ty[y], px = tx[x];
        const int cz[2] = {pz.c0, pz.c1}, cy[2] = {py.c0, py.c1}, cx[2] = {px.c0, px.c1};
        const double wz[2] = {pz.w0, pz.w1}, wy[2] = {py.w0, py.w1}, wx[2] = {px.w0, px.w1};
        cplx acc = cmake(0.0, 0.0);
        for (int a = 0; a < 2; ++a) { if (wz[a] == 0.0) continue;
            for (int b = 0; b < 2; ++b) { if (wy[b] == 0.0) continue;
                for (int c = 0; c < 2; ++c) { if (wx[c] == 0.0) continue;
                    const cplx v = cb[((long long)cz[a] * nyc + cy[b]) * nxc + cx[c]];
                    const double w = wz[a] * wy[b] * wx[c];
                    acc.x += w * v.x; acc.y += w * v.y;
                } } }
        fb[i] = vfrom<TF>(cadd(mg_cvt64(fb[i]), acc));
    }
}

// coarse vector (.)= the product of the three axes' wc (INV: its reciprocal), per right-hand side.  The restriction of the tables is R = D P^T with
// D = diag(wc_z wc_y wc_x) (mg3_keep.hip coarsen_axis normalises every row of P^T), so D^-1 (R r) = P^T r and P (D u) = R^T u: the transfers of the transposed
// cycle, which a transposed handle runs (cycle_keep).
__global__ void k3_scale_rt(cplx *__restrict__ v, int nzc, int nyc, int nxc, const RTab *__restrict__ tz, const RTab *__restrict__ ty, const RTab *__restrict__ tx,
                            int inv) {
    const long long Nc = (long long)nzc * nyc * nxc;
    cplx *vb = v + (long long)blockIdx.y * Nc;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < Nc; i += (long long)gridDim.x * blockDim.x) {
        const int X = (int)(i % nxc), Y = (int)((i / nxc) % nyc), Z = (int)(i / ((long long)nxc * nyc));
        const double d = tz[Z].wc * ty[Y].wc * tx[X].wc, f = inv ? 1.0 / d : d;
        const cplx a = vb[i];
        vb[i] = cmake(a.x * f, a.y * f);
    }
}

// smallest Re(c) of the model, on the device (positive doubles order like their bit patterns)
__global__ void k3_min_re(const cplx *__restrict__ c, long long n, unsigned long long *out) {
    double m = 1e300;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) m = fmin(m, c[e].x);
    for (int off = 32; off > 0; off >>= 1) m = fmin(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0) atomicMin(out, (unsigned long long)__double_as_longlong(m));
}

// one apply of a level's operator; dinv: the smoother's inverse diagonal (null: the level's own), x32 / y32: x / y hold complex64
int level_apply(helm_op *top, Mg3Level &L, const cplx *x, cplx *y, const cplx *w, int nrhs, int epi, double omega_j, const cplx *dinv = nullptr, int x32 = 0, int y32 = 0) {
    ApplyArgs a;
    a.planes = L.op->d_C; a.X = x; a.Y = y; a.W = w; a.ld = L.N; a.nrhs = nrhs; a.epi = epi; a.scaled = 0; a.adjoint = 0;
    a.scal = nullptr; a.part = (double *)top->d_part; a.dinv = dinv ? dinv : L.op->d_dinv; a.omega_j = omega_j; a.profile = 0; a.x32 = x32; a.y32 = y32;
    return helm_launch_apply(L.op, a);
}

// final_out (level 0 only): where the last post-smoothing sweep writes the result -- the caller's output vector, no copy
int cycle(helm_op *op, Mg3Precond *P, size_t l, int nrhs, cplx *final_out = nullptr) {
    Mg3Level &L = P->lv[l];
    hipStream_t st = op->stream;
    if (l + 1 == P->lv.size()) {        // coarsest: u = Cinv f, stored as U = F Cinv^T
        return nd_dense_gemm(op, nrhs, P->nc, P->nc, cmake(1, 0), L.f, P->nc, P->cinvT, P->nc, cmake(0, 0), L.u, P->nc);
    }
    Mg3Level &C = P->lv[l + 1];
    HELM_LAUNCH(k3_jac0<cplx>, vgrid(L.N, nrhs), dim3(256), 0, st, (const cplx *)L.f, (const cplx *)L.op->d_dinv, L.u, L.N, P->omega_j);
    int rc;
    for (int s = 1; s < P->nu1; ++s) {
        rc = level_apply(op, L, L.u, L.t, L.f, nrhs, EPI_JACOBI, P->omega_j); if (rc) return rc;
        std::swap(L.u, L.t);
    }
    rc = level_apply(op, L, L.u, L.r, L.f, nrhs, EPI_RESID, 0.0); if (rc) return rc;
    HELM_LAUNCH(k3_restrict, vgrid(C.N, nrhs), dim3(256), 0, st, L.r, C.f, L.nz, L.ny, L.nx, C.nz, C.ny, C.nx);
    rc = cycle(op, P, l + 1, nrhs); if (rc) return rc;
    HELM_LAUNCH(k3_prolong_add, vgrid(L.N, nrhs), dim3(256), 0, st, C.u, L.u, L.nz, L.ny, L.nx, C.nz, C.ny, C.nx);
    for (int s = 0; s < P->nu2; ++s) {
        if (final_out && s == P->nu2 - 1) return level_apply(op, L, L.u, final_out, L.f, nrhs, EPI_JACOBI, P->omega_j);
        rc = level_apply(op, L, L.u, L.t, L.f, nrhs, EPI_JACOBI, P->omega_j); if (rc) return rc;
        std::swap(L.u, L.t);
    }
    if (final_out) HIP_TRY(op, hipMemcpyAsync(final_out, L.u, (size_t)nrhs * L.N * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    return HELM_OK;
}

int cycle_keep(helm_op *op, Mg3Precond *P, size_t l, int nrhs, cplx *final_out = nullptr) {
    Mg3Keep *K = P->keep;
    Mg3Level &L = P->lv[l];
    hipStream_t st = op->stream;
    if (l + 1 == P->lv.size()) return mg3_coarse_solve(op, K, L, L.f, L.u, nrhs);
    Mg3Level &C = P->lv[l + 1];
    const cplx *dl1 = K->dl1[l];
    const double w = K->omega_l1;
    // f32 (round 6, helm_tuning.mg3_f32): the work vectors u, t, r of the FINEST level hold complex64 -- the cycle is a preconditioner, its input and its result
    // stay complex128 (the outer BiCGSTAB recurrences, the operator applies that form its residuals and the convergence check are untouched), and single precision
    // in between costs the Krylov method nothing it can see (iteration counts in the tests).  What it buys: half the bytes of every vector the sweeps, the residual
    // and the transfers of that level move, and half the staging of the 27-point kernel's tiles, which is what bounds it.
    const bool f32 = l == 0 && P->fine32 && final_out != nullptr && P->nu2 >= 1;
    auto smooth = [&](const cplx *x, cplx *y) { return level_apply(op, L, x, y, L.f, nrhs, EPI_JACOBI, w, dl1, f32, f32 && y != final_out); };
    if (f32) HELM_LAUNCH(k3_jac0<cplxf>, vgrid(L.N, nrhs), dim3(256), 0, st, (const cplx *)L.f, dl1, (cplxf *)L.u, L.N, w);
    else HELM_LAUNCH(k3_jac0<cplx>, vgrid(L.N, nrhs), dim3(256), 0, st, (const cplx *)L.f, dl1, L.u, L.N, w);
    int rc;
    for (int s = 1; s < P->nu1; ++s) { rc = smooth(L.u, L.t); if (rc) return rc; std::swap(L.u, L.t); }
    rc = level_apply(op, L, L.u, L.r, L.f, nrhs, EPI_RESID, 0.0, nullptr, f32, f32);
    if (rc) return rc;
    if (f32) HELM_LAUNCH(k3_restrict_t<cplxf>, vgrid(C.N, nrhs), dim3(256), 0, st, (const cplxf *)L.r, C.f, L.ny, L.nx, C.nz, C.ny, C.nx, L.N,
                         (const RTab *)K->rt[0][l], (const RTab *)K->rt[1][l], (const RTab *)K->rt[2][l]);
    else HELM_LAUNCH(k3_restrict_t<cplx>, vgrid(C.N, nrhs), dim3(256), 0, st, (const cplx *)L.r, C.f, L.ny, L.nx, C.nz, C.ny, C.nx, L.N,
                       (const RTab *)K->rt[0][l], (const RTab *)K->rt[1][l], (const RTab *)K->rt[2][l]);
    // a transposed handle runs the transpose of the cycle of A: restriction P^T = D^-1 R, prolongation R^T = P D (k3_scale_rt; the levels hold A_l^T)
    const bool tr = op->transposed;
    if (tr) HELM_LAUNCH(k3_scale_rt, vgrid(C.N, nrhs), dim3(256), 0, st, C.f, C.nz, C.ny, C.nx, (const RTab *)K->rt[0][l], (const RTab *)K->rt[1][l], (const RTab *)K->rt[2][l], 1);
    rc = cycle_keep(op, P, l + 1, nrhs); if (rc) return rc;
    if (tr) HELM_LAUNCH(k3_scale_rt, vgrid(C.N, nrhs), dim3(256), 0, st, C.u, C.nz, C.ny, C.nx, (const RTab *)K->rt[0][l], (const RTab *)K->rt[1][l], (const RTab *)K->rt[2][l], 0);
    if (f32) HELM_LAUNCH(k3_prolong_add_t<cplxf>, vgrid(L.N, nrhs), dim3(256), 0, st, (const cplx *)C.u, (cplxf *)L.u, L.nz, L.ny, L.nx, C.ny, C.nx, C.N,
                         (const PTab *)K->pt[0][l], (const PTab *)K->pt[1][l], (const PTab *)K->pt[2][l]);
    else HELM_LAUNCH(k3_prolong_add_t<cplx>, vgrid(L.N, nrhs), dim3(256), 0, st, (const cplx *)C.u, L.u, L.nz, L.ny, L.nx, C.ny, C.nx, C.N,
                       (const PTab *)K->pt[0][l], (const PTab *)K->pt[1][l], (const PTab *)K->pt[2][l]);
    for (int s = 0; s < P->nu2; ++s) {
        if (final_out && s == P->nu2 - 1) return smooth(L.u, final_out);
        rc = smooth(L.u, L.t); if (rc) return rc;
        std::swap(L.u, L.t);
    }
    if (final_out) HIP_TRY(op, hipMemcpyAsync(final_out, L.u, (size_t)nrhs * L.N * sizeof(cplx), hipMemcpyDeviceToDevice, st));
    return HELM_OK;
}

}  // namespace

// the hierarchy's level operators launch on the stream they were built on: point them at another one (helm_prefactor_n builds on a
// low-priority stream, the solves run on the handle's own)
void mg3_retarget_stream(helm_op *op, hipStream_t st) {
    if (!op->mg3) return;
    for (Mg3Level &L : op->mg3->lv) if (L.op) L.op->stream = st;
}

void mg3_destroy(helm_op *op) {
    Mg3Precond *P = op->mg3;
    if (!P) return;
    hierarchy_free(op, P);
    hipFree(P->cinvT);
    delete P;
    op->mg3 = nullptr;
}

// measure the grid's points per wavelength, choose the depth, try the layer-preserving set-up, else build the standard hierarchy
int mg3_setup(helm_op *op, int batch) {
    if (op->mg3 && op->mg3->batch >= batch) return HELM_OK;
    if (op->mg3) mg3_destroy(op);
    int rc = HELM_OK;
    Mg3Precond *P = new Mg3Precond();
    op->mg3 = P;
    P->batch = batch;
    const helm_tuning tune = helm_tuning_now();
    // Jacobi damping: measured at 256 x 256 x 128, 4 sources (tools/sweep3d.sh): 0.8 / 0.9 / 1.0 / 1.1 -> 10.9 / 9.6 / 10.0 / 16.4 s at 3 Hz and
    // 7.4 / 7.0 / 6.6 / 8.9 s at 5 Hz
    P->omega_j = tune.mg3_omega;
    P->nu1 = 1; P->nu2 = 1; P->min_n = 8;
    const double omega = 2.0 * M_PI * std::abs(std::complex<double>(op->a_freq_re, op->a_freq_im));
    double cmin = 1e300;
    {
        unsigned long long *dmin = (unsigned long long *)helm_pool_alloc(op->device, 64);     // (64 bytes: the pool's smallest size class)
        unsigned long long hmin = ~0ULL;
        if (!dmin) HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: scratch allocation failed");
        hipMemcpyAsync(dmin, &hmin, sizeof(hmin), hipMemcpyHostToDevice, op->stream);
        HELM_LAUNCH(k3_min_re, dim3(2048), dim3(256), 0, op->stream, (const cplx *)op->d_c, op->N, dmin);
        hipMemcpyAsync(&hmin, dmin, sizeof(hmin), hipMemcpyDeviceToHost, op->stream);
        HIP_TRY(op, hipStreamSynchronize(op->stream));
        helm_pool_free(op->device, dmin, 64);
        if (hmin != ~0ULL) { long long b = (long long)hmin; cmin = __builtin_bit_cast(double, b); }
    }
    const double hmax = std::max(op->dx, std::max(op->dy, op->dz));
    const double ppw = omega > 0 ? cmin / (omega / (2.0 * M_PI) * hmax) : 10.0;
    const double over = std::max(1.0, ppw / 10.0);
    // shift: 0.6 at 10 grid points per wavelength, growing with the square of the oversampling up to 8 -- measured at
    // 256 x 256 x 128, 40-100 points per wavelength: beta 0.6 / 3 / 6 / 12 -> 26 / 16 / 14 / 14 s per 4 sources at 3 Hz
    P->beta = tune.mg3_beta > 0 ? tune.mg3_beta : std::min(8.0, 0.6 * over * over);
    // Oversampled grids: the layer-preserving hierarchy (mg3_keep.hip).  Falls back to the standard cycle when no level can be dropped or the direct
    // solver of its last level does not fit.
    const int ncoarsen = mg3_choose_depth(op, batch, ppw, tune);
    if (tune.mg3_keep && !op->mg3_no_keep && ncoarsen > 0 && op->a_cpml > 0 && omega > 0) {
        const double betak = tune.mg3_beta > 0 ? tune.mg3_beta : 0.1;
        double inv_tau_k = omega * betak / 2.0;
        if (std::isfinite(op->a_tau) && op->a_tau != 0.0) inv_tau_k += 1.0 / op->a_tau;
        const int rck = mg3_keep_setup(op, P, batch, ncoarsen, 1.0 / inv_tau_k, tune);
        if (rck == HELM_OK) { P->beta = betak; P->kept_levels = ncoarsen; P->ppw_direct = ppw / (double)(1 << ncoarsen); hipStreamSynchronize(op->stream); return HELM_OK; }
        if (tune.mg3_keep == 2) { const std::string msg = op->err; mg3_destroy(op); helm_set_error(op, msg.c_str()); return rck; }
        // not this time: release what was built and go on with the standard hierarchy
        hierarchy_free(op, P);
    }
    double inv_tau = omega * P->beta / 2.0;
    if (std::isfinite(op->a_tau) && op->a_tau != 0.0) inv_tau += 1.0 / op->a_tau;
    const double tauM = 1.0 / inv_tau;
    // layer of the preconditioner: gamma / omega = 2 (measured at 256 x 256 x 128 with the shift above: 0.2 omega -> 26 / 14 / 8.8 s
    // per 4 sources at 2 / 3 / 5 Hz, 2 omega -> 22 / 10.5 / 7.4 s, 5 omega worse again, the true layer (300) does not converge;
    // with the small shift beta = 0.6 only gamma / omega <= 0.4 was stable)
    P->cpml_m = 2.0 * omega;
    const double cpml = std::min(P->cpml_m, op->a_cpml > 0 ? op->a_cpml : P->cpml_m);
    rc = helm_ensure_host_model(op);               // (the standard hierarchy injects its models on the host)
    if (rc) return rc;
    std::vector<cplx> c = op->h_c;
    std::vector<double> rho = op->h_rho;
    int nz = op->nz, ny = op->ny, nx = op->nx, npml = op->nPML;
    double dx = op->dx, dy = op->dy, dz = op->dz;
    auto fail = [&](int code, const char *msg) { helm_set_error(op, msg); mg3_destroy(op); return code; };
    while (true) {
        Mg3Level L;
        L.nz = nz; L.ny = ny; L.nx = nx; L.N = (long long)nz * ny * nx;
        L.op = helm_create3d(op->device, nz, ny, nx, dx, dy, dz, npml);
        if (!L.op) return fail(HELM_ERR_DEVICE, helm_last_error(nullptr));
        P->lv.push_back(L);
        Mg3Level &Lr = P->lv.back();
        if (helm_set_stream(Lr.op, op->stream)) return fail(HELM_ERR_DEVICE, "3-D multigrid: cannot share the stream");
        // the levels of a transposed operator's preconditioner are transposed too.  Here R = P^T / 8 (a constant) and the smoother is point Jacobi, so
        // the cycle of the transposed levels with the same transfers IS the transpose of the cycle of A; the layer-preserving hierarchy has more to do (mg3_keep.hip)
        Lr.op->transposed_next = op->transposed;
        rc = helm_set_model(Lr.op, (const double *)c.data(), rho.data(), nullptr, nullptr, nullptr);
        if (!rc) rc = helm_assemble(Lr.op, op->a_freq_re, op->a_freq_im, tauM, 0.0, cpml);
        if (!rc) rc = helm_ensure_scaled(Lr.op);
        if (rc) return fail(rc, helm_last_error(Lr.op));
        if (!mg3_level_vectors(op, Lr, batch)) return fail(HELM_ERR_DEVICE, "3-D multigrid: level vectors do not fit");
        const int nzc = (nz + 1) / 2, nyc = (ny + 1) / 2, nxc = (nx + 1) / 2;
        const int npmlc = std::max((npml - 1) / 2 + 1, 2);
        const long long Nc = (long long)nzc * nyc * nxc;
        if (std::min(nz, std::min(ny, nx)) <= P->min_n || std::min(nzc, std::min(nyc, nxc)) < 2 * npmlc + 2 || Lr.N <= 4096 || Nc < 27) break;
        c = inject3(c, nz, ny, nx); rho = inject3(rho, nz, ny, nx);
        nz = nzc; ny = nyc; nx = nxc; dx *= 2; dy *= 2; dz *= 2; npml = npmlc;
    }
    // coarsest level: dense inverse
    Mg3Level &Lc = P->lv.back();
    if (Lc.N > 8192) return fail(HELM_ERR_UNSUPPORTED, "3-D multigrid: coarsest grid too large for a dense inverse");
    P->nc = (int)Lc.N;
    cplx *A = nullptr, *W = nullptr;
    const size_t mb = (size_t)P->nc * P->nc * sizeof(cplx);
    if (helm_malloc_retry(op->device, (void **)&A, mb) != hipSuccess || helm_malloc_retry(op->device, (void **)&W, mb) != hipSuccess || helm_malloc_retry(op->device, (void **)&P->cinvT, mb) != hipSuccess) {
        hipFree(A); hipFree(W); return fail(HELM_ERR_DEVICE, "3-D multigrid: coarsest inverse does not fit");
    }
    hipMemsetAsync(A, 0, mb, op->stream);
    HELM_LAUNCH(k3_dense, dim3((unsigned)((Lc.N + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)Lc.op->d_C, A, Lc.nz, Lc.ny, Lc.nx);
    rc = nd_dense_inverse(op, A, P->nc, W);
    if (!rc) HELM_LAUNCH(k3_transpose_sq, dim3(4096), dim3(256), 0, op->stream, (const cplx *)A, P->cinvT, P->nc);
    hipStreamSynchronize(op->stream);
    hipFree(A); hipFree(W);
    if (rc) return fail(rc, "3-D multigrid: coarsest inverse failed");
    return HELM_OK;
}

bool mg3_is_layer_preserving(const helm_op *op) { return op->mg3 && op->mg3->keep; }

int mg3_retreat(helm_op *op, int batch) {
    op->mg3_no_keep = true;
    mg3_destroy(op);
    return mg3_setup(op, batch);
}

// out[b] = M^-1 in[b]
int mg3_apply(helm_op *op, const cplx *in, cplx *out, int nrhs) {
    Mg3Precond *P = op->mg3;
    if (!P || nrhs > P->batch) HELM_FAIL(op, HELM_ERR_STATE, "3-D multigrid preconditioner not set up");
    Mg3Level &L0 = P->lv[0];
    // the finest level reads its right-hand side in place and its last sweep writes straight into `out` (these two device copies
    // of batch x 128 MB were 9 % of the GPU time of a config-5 solve)
    cplx *own_f = L0.f;
    if (P->lv.size() > 1) L0.f = const_cast<cplx *>(in);
    else HIP_TRY(op, hipMemcpyAsync(L0.f, in, (size_t)nrhs * L0.N * sizeof(cplx), hipMemcpyDeviceToDevice, op->stream));
    const int rc = P->keep ? cycle_keep(op, P, 0, nrhs, P->lv.size() > 1 ? out : nullptr) : cycle(op, P, 0, nrhs, P->lv.size() > 1 ? out : nullptr);
    L0.f = own_f;
    if (rc) return rc;
    if (P->lv.size() == 1) HIP_TRY(op, hipMemcpyAsync(out, L0.u, (size_t)nrhs * L0.N * sizeof(cplx), hipMemcpyDeviceToDevice, op->stream));
    return HELM_OK;
}
