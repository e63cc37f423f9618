// The derivative of the 3-D 27-point operator along the buoyancy b = 1 / rho on stored columns, each kernel beside the C entry point that launches it.
//
// An interior row of the operator is C_o(p) = (b_p + b_{p+o}) / 2 lap_o(p) + b_{p+o} kappa_{p+o} mu_o (helm3d.hip), kappa = om~^2 / c^2,
//     lap_o(p) = Lx[ox](ix) m(oy) m(oz) / dx^2 + m(ox) Ly[oy](iy) m(oz) / dy^2 + m(ox) m(oy) Lz[oz](iz) / dz^2,
// the stretch tables (op->d_L3) read at the ROW p.  The row is linear and homogeneous in b, so with L the matrix of lap_o(p) on interior rows
//     dA[db] = 1/2 diag(db) L + 1/2 L diag(db) + M~ diag(kappa db).
// The kappa part is the mass stencil of survey3d.hip with another weight (k_mass3_sources / k_mass3_imaging as they are); what is here is the Laplacian pair
// and the chain kernel that makes the weights.  L is NOT symmetric -- the stretch factors sit at the row -- so the imaging sum needs L^T:
//     (L^T z)_j = sum_o lap_o(j - o) z_{j-o} = sum_o' lap_{-o'}(j + o') z_{j+o'},   the tables read at the neighbour j + o'.
//
// Both kernels walk the grid as k_stencil3 and the mass kernels do: a workgroup of 256 takes a 64 x 4 tile of one z-plane, z fastest, stages the three
// z-planes of a column with halo in LDS, double-buffered, and loops over the columns with the next column's loads in flight.  No thread keeps 27 coefficients:
// lap_o is a sum of three separable terms, so the 27-point sum is formed from nine table values per thread in an order the code fixes (lap3_sum),
//     ax(p, r) = sum_ox Lx[ox] t,  am(p, r) = m0 t(0) + m1 (t(-1) + t(+1))                                   along x
//     px(p) = m0 ax(0) + m1 (ax(-1) + ax(+1)),  py(p) = sum_oy Ly[oy] am(oy),  pm(p) = m0 am(0) + m1 (am(-1) + am(+1))   along y
//     sum = (m0 px(0) + m1 (px(-1) + px(+1))) / dx^2 + (m0 py(0) + m1 (py(-1) + py(+1))) / dy^2 + (sum_oz Lz[oz] pm(oz)) / dz^2
// so the same bits come out of every run.  No atomics.  LDS: k_lap3_sources 2 x 19008 B of products and 9504 B of B with halo = 47520 B;
// k_lap3_imaging two fields, double-buffered, 4 x 19008 = 76032 B (two workgroups per compute unit of 160 KB).
// The tile, the tables, lap3_sum and kappa3s are in survey3d_lap.hpp: survey3d_hessian.hip walks the same way.
#include "survey3d_lap.hpp"

namespace {

// R[s ldr + i] (+)= coef (1/2 B (.) (L X_s) + 1/2 L(B (.) X_s))[i] = coef / 2 sum_o lap_o(i) (B_i + B_{i+o}) X_s[i + o], X_s = U_s or (CONJ) conj(U_s), for the
// columns s = blockIdx.y, blockIdx.y + gridDim.y, ... < nsrc.  X_s is staged, B with halo is staged once; the sum (B_i + B_{i+o}) X is formed on the way out of
// LDS.  ADD: the interior rows of R receive the sum on top of what they hold and its boundary rows are left alone; otherwise the boundary rows are written as
// exact zeros.  Per cell and column 16 bytes read (times the halo factor 1.55 across planes, from L2) and 16 written (ADD: 16 more read).
template <bool CONJ, bool ADD>
__global__ __launch_bounds__(256) void k_lap3_sources(const cplx *__restrict__ U, int nsrc, long long ldu, const double *__restrict__ B, cplx coef,
                                                      cplx *__restrict__ R, long long ldr, Lap3Params q) {
    __shared__ cplx tile[2][D3NEL];
    __shared__ double bt[D3NEL];
    const int tid = threadIdx.x, lane = tid & 63, wy = tid >> 6;
    const int nz = q.nz, ny = q.ny, nx = q.nx;
    const Tile3d T(nz, q.ntx);
    const int col = T.x0 + lane, row = T.y0 + wy;
    const bool ok = col < nx && row < ny;
    const bool inside = ok && col >= 1 && col <= nx - 2 && row >= 1 && row <= ny - 2 && T.iz >= 1 && T.iz <= nz - 2;
    const long long idx = ((long long)T.iz * ny + row) * nx + col;
    long long cell[D3NLOAD];
    cplx pre[D3NLOAD];
#pragma unroll
    for (int l = 0; l < D3NLOAD; ++l) {
        const int e = tid + 256 * l;
        bool bnd;
        cell[l] = e < D3NEL ? tile3d_cell(T, e, nz, ny, nx, bnd) : -1;
        if (e < D3NEL) bt[e] = cell[l] >= 0 ? B[cell[l]] : 0.0;
    }
    const Lap3Tab tab = lap3_row_tables(q, ok, col, row, T.iz);
    const cplx half = cmake(0.5 * coef.x, 0.5 * coef.y);
    auto prefetch = [&](int s) {
        const cplx *Us = U + (long long)s * ldu;
#pragma unroll
        for (int l = 0; l < D3NLOAD; ++l) pre[l] = cell[l] >= 0 ? Us[cell[l]] : cmake(0.0, 0.0);
    };
    int s = blockIdx.y, buf = 0;
    if (s < nsrc) prefetch(s);
    __syncthreads();                   // bt is complete
    const int ce = wy * D3LW + lane;   // the tile element of the cell's (-1, -1, -1) neighbour
    const double b0 = bt[D3PLANE + ce + D3LW + 1];
    for (; s < nsrc; s += gridDim.y, buf ^= 1) {
#pragma unroll
        for (int l = 0; l < D3NLOAD; ++l) {
            const int e = tid + 256 * l;
            if (e < D3NEL) tile[buf][e] = CONJ ? cconj(pre[l]) : pre[l];
        }
        if (s + (int)gridDim.y < nsrc) prefetch(s + gridDim.y);
        __syncthreads();               // (one barrier per column: the buffer written two columns from now was last read before the NEXT barrier)
        cplx *out = R + (long long)s * ldr + idx;
        if (inside) {                  // (a boundary row forms no sum: it is left alone, or written as zero)
            const cplx *tb = &tile[buf][ce];
            const double *bb = &bt[ce];
            const cplx sum = lap3_sum(tab, q.idx2, q.idy2, q.idz2, [&](int p, int r, int cc) {
                const int e = p * D3PLANE + r * D3LW + cc;
                const double w = b0 + bb[e];
                return cmake(w * tb[e].x, w * tb[e].y);
            });
            if (ADD) { cplx r0 = *out; cfma(r0, half, sum); *out = r0; }
            else *out = cmul(half, sum);
        } else if (!ADD && ok) *out = cmake(0.0, 0.0);
    }
}

// P[j] += 1/2 sum_{s<nsrc} ( B0_s[j] (L F_s)[j] + F_s[j] (L^T B0_s)[j] ), F_s = UF[s ldf + .], B0_s = UB[s ldb + .] with its boundary rows masked to zero WHILE
// STAGING (whatever they hold is never loaded); CONJ: both fields conjugated while staging (the stored columns are conj(u^) and conj(z~); L is complex, so the
// conjugation cannot wait for the sum).  Every cell j of the grid receives its sum -- a boundary node is a column of interior rows.  s ascending in one
// register per thread, one load and one store of P per cell, no atomics.  Per cell and column 16 bytes of UF and 16 of UB (each times the halo factor), 32 of P.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_lap3_imaging(const cplx *__restrict__ UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc,
                                                      cplx *__restrict__ P, Lap3Params q) {
    __shared__ cplx tf[2][D3NEL];
    __shared__ cplx tz[2][D3NEL];
    const int tid = threadIdx.x, lane = tid & 63, wy = tid >> 6;
    const int nz = q.nz, ny = q.ny, nx = q.nx;
    const Tile3d T(nz, q.ntx);
    const int col = T.x0 + lane, row = T.y0 + wy;
    const bool ok = col < nx && row < ny;
    const long long idx = ((long long)T.iz * ny + row) * nx + col;
    long long cell[D3NLOAD];
    bool rowz[D3NLOAD];                // the cell is an interior row: its UB is read
    cplx pf[D3NLOAD], pz[D3NLOAD];
#pragma unroll
    for (int l = 0; l < D3NLOAD; ++l) {
        const int e = tid + 256 * l;
        bool bnd = true;
        cell[l] = e < D3NEL ? tile3d_cell(T, e, nz, ny, nx, bnd) : -1;
        rowz[l] = cell[l] >= 0 && !bnd;
    }
    const Lap3Tab tab = lap3_row_tables(q, ok, col, row, T.iz), tabT = lap3_transposed_tables(q, ok, col, row, T.iz);
    auto prefetch = [&](int s) {
        const cplx *Fs = UF + (long long)s * ldf, *Zs = UB + (long long)s * ldb;
#pragma unroll
        for (int l = 0; l < D3NLOAD; ++l) {
            pf[l] = cell[l] >= 0 ? Fs[cell[l]] : cmake(0.0, 0.0);
            pz[l] = rowz[l] ? Zs[cell[l]] : cmake(0.0, 0.0);
        }
    };
    cplx acc = cmake(0.0, 0.0);
    const int ce = wy * D3LW + lane, cc0 = D3PLANE + D3LW + 1;
    int buf = 0;
    prefetch(0);
    for (int s = 0; s < nsrc; ++s, buf ^= 1) {
#pragma unroll
        for (int l = 0; l < D3NLOAD; ++l) {
            const int e = tid + 256 * l;
            if (e < D3NEL) { tf[buf][e] = CONJ ? cconj(pf[l]) : pf[l]; tz[buf][e] = CONJ ? cconj(pz[l]) : pz[l]; }
        }
        if (s + 1 < nsrc) prefetch(s + 1);
        __syncthreads();
        const cplx *fb = &tf[buf][ce], *zb = &tz[buf][ce];
        const cplx lf = lap3_sum(tab, q.idx2, q.idy2, q.idz2, [&](int p, int r, int cc) { return fb[p * D3PLANE + r * D3LW + cc]; });
        const cplx lz = lap3_sum(tabT, q.idx2, q.idy2, q.idz2, [&](int p, int r, int cc) { return zb[p * D3PLANE + r * D3LW + cc]; });
        cfma(acc, zb[cc0], lf);
        cfma(acc, fb[cc0], lz);
    }
    if (ok) { const cplx p = P[idx]; P[idx] = cmake(p.x + 0.5 * acc.x, p.y + 0.5 * acc.y); }
}

// One lane per cell; b = 1.0 / rho as the assembly forms it.  chain_j = -1 / rho_j^2 = -b_j^2 (GARDNER false: the density chain) or d b / d c = -b_j / (4 Re c_j)
// (GARDNER true: the density follows the velocity, rho = 310 Re(c)^0.25).
// din given (Born): db[j] = chain_j din[j] (N float64) and W[j] = w kappa_j db[j] (N complex128).
// din NULL (gradient): G[j] += chain_j Re(w (Plap[j] + kappa_j Pmass[j])) (N float64).
template <bool GARDNER>
__global__ __launch_bounds__(256) void k_buoy3_chain(const cplx *__restrict__ c, const double *__restrict__ rho, cplx om, const double *__restrict__ din,
                                                     const cplx *__restrict__ Plap, const cplx *__restrict__ Pmass, cplx w, double *__restrict__ db,
                                                     void *__restrict__ out, long long N) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const cplx cj = c[j];
    const double b = 1.0 / rho[j];
    const double chain = GARDNER ? -b / (4.0 * cj.x) : -(b * b);
    const cplx wk = cmul(w, kappa3s(cmul(om, om), cj));
    if (din) {
        const double d = chain * din[j];
        db[j] = d;
        static_cast<cplx *>(out)[j] = cmake(wk.x * d, wk.y * d);
    } else {
        const cplx pl = Plap[j], pm = Pmass[j];
        const double re = (w.x * pl.x - w.y * pl.y) + (wk.x * pm.x - wk.y * pm.y);
        static_cast<double *>(out)[j] += chain * re;
    }
}


}  // namespace

extern "C" int helm_lap3_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dB, double coef_re, double coef_im, int conj, int add,
                                        void *dR, long long ldr) {
    helm_tuning_refresh();
    if (!op || !dU || !dB || !dR || nsrc < 1 || ldu < op->N || ldr < op->N) return HELM_ERR_ARG;
    { const int rc = buoy3_handle_args(op, "helm_lap3_sources_device"); if (rc) return rc; }
    if (((((uintptr_t)dU) | ((uintptr_t)dR)) & 15) || (((uintptr_t)dB) & 7)) return HELM_ERR_ARG;
    const size_t nr = sizeof(cplx) * ((size_t)(nsrc - 1) * ldr + op->N);
    if (ranges_overlap(dR, nr, dU, sizeof(cplx) * ((size_t)(nsrc - 1) * ldu + op->N)) || ranges_overlap(dR, nr, dB, sizeof(double) * (size_t)op->N)) return HELM_ERR_ARG;
    Lap3Params q;
    int nblk;
    { const int rc = lap3_params(op, "helm_lap3_sources_device", &q, &nblk); if (rc) return rc; }
    HIP_TRY(op, hipSetDevice(op->device));
    int split = 1;                      // few tiles: the columns are spread over grid.y, as helm_mass3_sources_device spreads them
    if (nblk < 2048) { split = (2048 + nblk - 1) / nblk; if (split > nsrc) split = nsrc; if (split > 65535) split = 65535; }
    const dim3 grid((unsigned)nblk, (unsigned)split);
    const cplx coef = cmake(coef_re, coef_im);
#define LAP3_SRC(C, A) HELM_LAUNCH((k_lap3_sources<C, A>), grid, dim3(256), 0, op->stream, (const cplx *)dU, nsrc, ldu, (const double *)dB, coef, (cplx *)dR, ldr, q)
    if (conj) { if (add) LAP3_SRC(true, true); else LAP3_SRC(true, false); }
    else { if (add) LAP3_SRC(false, true); else LAP3_SRC(false, false); }
#undef LAP3_SRC
    return launched(op);
}

extern "C" int helm_lap3_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, int conj, void *dP) {
    helm_tuning_refresh();
    if (!op || !dUF || !dUB || !dP || nsrc < 1 || ldf < op->N || ldb < op->N) return HELM_ERR_ARG;
    { const int rc = buoy3_handle_args(op, "helm_lap3_imaging_accumulate_device"); if (rc) return rc; }
    if ((((uintptr_t)dUF) | ((uintptr_t)dUB) | ((uintptr_t)dP)) & 15) return HELM_ERR_ARG;
    const size_t nb = sizeof(cplx) * (size_t)op->N;
    if (ranges_overlap(dP, nb, dUF, sizeof(cplx) * ((size_t)(nsrc - 1) * ldf + op->N)) || ranges_overlap(dP, nb, dUB, sizeof(cplx) * ((size_t)(nsrc - 1) * ldb + op->N))) return HELM_ERR_ARG;
    Lap3Params q;
    int nblk;
    { const int rc = lap3_params(op, "helm_lap3_imaging_accumulate_device", &q, &nblk); if (rc) return rc; }
    HIP_TRY(op, hipSetDevice(op->device));
    if (conj) HELM_LAUNCH((k_lap3_imaging<true>), dim3((unsigned)nblk), dim3(256), 0, op->stream, (const cplx *)dUF, ldf, (const cplx *)dUB, ldb, nsrc, (cplx *)dP, q);
    else HELM_LAUNCH((k_lap3_imaging<false>), dim3((unsigned)nblk), dim3(256), 0, op->stream, (const cplx *)dUF, ldf, (const cplx *)dUB, ldb, nsrc, (cplx *)dP, q);
    return launched(op);
}

extern "C" int helm_buoy3_chain_device(helm_op *op, int gardner, const void *dIn, const void *dPlap, const void *dPmass, double w_re, double w_im, void *dDb, void *dOut) {
    helm_tuning_refresh();
    if (!op || !dOut || (dIn ? !dDb : (!dPlap || !dPmass))) return HELM_ERR_ARG;
    { const int rc = buoy3_handle_args(op, "helm_buoy3_chain_device"); if (rc) return rc; }
    if (((uintptr_t)dOut & (dIn ? 15 : 7)) || ((uintptr_t)dIn & 7) || ((uintptr_t)dDb & 7) || ((uintptr_t)dPlap & 15) || ((uintptr_t)dPmass & 15)) return HELM_ERR_ARG;
    const size_t nd = sizeof(double) * (size_t)op->N, nc = sizeof(cplx) * (size_t)op->N;
    if (dIn && (ranges_overlap(dOut, nc, dIn, nd) || ranges_overlap(dOut, nc, dDb, nd) || ranges_overlap(dDb, nd, dIn, nd))) return HELM_ERR_ARG;
    if (!dIn && (ranges_overlap(dOut, nd, dPlap, nc) || ranges_overlap(dOut, nd, dPmass, nc))) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    const cplx om = damped_omega3(op);
    const dim3 grid((unsigned)((op->N + 255) / 256));
    if (gardner) HELM_LAUNCH((k_buoy3_chain<true>), grid, dim3(256), 0, op->stream, (const cplx *)op->d_c, (const double *)op->d_rho, om, (const double *)dIn,
                             (const cplx *)dPlap, (const cplx *)dPmass, cmake(w_re, w_im), (double *)dDb, dOut, op->N);
    else HELM_LAUNCH((k_buoy3_chain<false>), grid, dim3(256), 0, op->stream, (const cplx *)op->d_c, (const double *)op->d_rho, om, (const double *)dIn,
                     (const cplx *)dPlap, (const cplx *)dPmass, cmake(w_re, w_im), (double *)dDb, dOut, op->N);
    return launched(op);
}
