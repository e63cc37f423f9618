// The pseudo-Hessian diagonal and the per-cell (c, rho) blocks of the 3-D 27-point operator from stored columns, each kernel beside the C entry point that
// launches it.
//
//     H_p[i] = sum_s ||(dA / dp_i) u^_s||^2,     B_ab[i] = sum_s Re <(dA / da_i) u^_s, (dA / db_i) u^_s>
//
// The column of a unit perturbation of cell i touches the 27 rows p = i + d around it (survey3d_density.hip has dA[db]; mu is even, mu_{i-p} = mu_d):
//     velocity (explicit rho):  v^c_p = chi_i mu_d [p interior] u^_i,                                        chi = -2 kappa b / c
//     buoyancy:                 v^b_p = a_p(i) u^_i + [p == i] 1/2 (L u^)_i,   a_p(i) = [p interior] (1/2 lap_{-d}(i + d) + kappa_i mu_d)
// lap_{-d}(i + d) reads the stretch tables at the NEIGHBOUR's row -- the column entry L[i + d, i], what lap3_transposed_tables forms.  So per cell and column
// only u^_i and T_i = (L u^)_i are needed, everything else is a per-cell coefficient that does not depend on the source.  With r_s = A0_i u^_{s,i} + h_i T_{s,i}
// and the moments E = sum_s |u^_i|^2, D = sum_s |r_s|^2, Y = sum_s conj(u^_i) r_s:
//     H_bb = S' E + D                                         A0 = a_i(i), h = 1/2, S' = sum_{d != 0} |a_{i+d}(i)|^2
//     H_cc = |chi|^2 Smu E                                    Smu = sum_{p interior} mu_d^2
//     H_cb = Re conj(chi) (C' E + mu_0 [i interior] Y)        C' = sum_{d != 0} mu_d a_{i+d}(i)
//     Gardner total (v^c + g v^b, g = d b / d c):  H = S' E + D with A0 = chi mu_0 [i interior] + g a_i(i), h = g / 2, S' = sum_{d != 0} |chi mu_d [p interior] + g a_p(i)|^2
// and H_rhorho = H_bb / rho^4, H_crho = -H_cb / rho^2.  D is a sum of squares and is never expanded: |a|^2 E + Re(conj(a) X) + 1/4 sum |T|^2 is algebraically the
// same and cancels wherever L u^ ~ -kappa u^, which is everywhere away from a source.
//
// k_ph3_coefficients makes the coefficient planes once per operator and model, one lane per cell.  k_ph3_moments is the loop over the columns: the tile and the
// walk of k_lap3_sources (64 x 4 of one z-plane, three planes with halo in LDS, double-buffered, the next column's loads in flight, lap3_sum with the row
// tables), but it stores no column: the moments stay in registers, s ascending in one workgroup (gridDim.y == 1), and after the last column every cell is
// loaded and stored once.  One writer per cell, no atomics: the same bits on every run.  LDS 2 x 19008 B.
// The velocity diagonal with an explicit density launches neither kernel: it is k_energy with the weight |chi|^2 Smu.
#include "survey3d_lap.hpp"

namespace {

enum { PH3_BUOYANCY = 0, PH3_GARDNER = 1, PH3_BLOCKS = 2 };

// chi = -2 kappa b / c of one cell
__device__ __forceinline__ cplx chi3(cplx kap, double b, cplx cj) {
    const double s = -2.0 * b, tx = kap.x * s, ty = kap.y * s, d = cj.x * cj.x + cj.y * cj.y;
    return cmake((tx * cj.x + ty * cj.y) / d, (ty * cj.x - tx * cj.y) / d);
}

// The coefficient planes of a model, one lane per cell i = (iz, row, col): A0 (complex), h, S' (real), and for PH3_BLOCKS C' (complex) and Smu (real).
// kappa by the expression k_buoy3_chain uses, the Gardner chain as k_buoy3_chain<true> forms it, the 27 rows in the fixed order dz, dy, dx ascending.
template <int MODE>
__global__ __launch_bounds__(256) void k_ph3_coefficients(const cplx *__restrict__ c, const double *__restrict__ rho, cplx om, cplx *__restrict__ A0, double *__restrict__ Hh,
                                                          double *__restrict__ S, cplx *__restrict__ C, double *__restrict__ Smu, Lap3Params q) {
    const long long N = (long long)q.nz * q.ny * q.nx, j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const int col = (int)(j % q.nx), row = (int)((j / q.nx) % q.ny), iz = (int)(j / ((long long)q.nx * q.ny));
    const Lap3Tab tabT = lap3_transposed_tables(q, true, col, row, iz);
    const cplx cj = c[j];
    const double b = 1.0 / rho[j];
    const cplx kap = kappa3s(cmul(om, om), cj);
    const cplx chi = MODE == PH3_GARDNER ? chi3(kap, b, cj) : cmake(0.0, 0.0);
    const double g = MODE == PH3_GARDNER ? -b / (4.0 * cj.x) : 1.0;
    cplx a0 = cmake(0.0, 0.0), cs = cmake(0.0, 0.0);
    double s = 0.0, smu = 0.0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const double mz = dz ? D3M1 : D3M0, my = dy ? D3M1 : D3M0, mx = dx ? D3M1 : D3M0;
                const bool centre = dz == 0 && dy == 0 && dx == 0;
                const double mu = 0.5 * (mx * my * mz) + (centre ? 0.5 : 0.0);
                const int pz = iz + dz, py = row + dy, px = col + dx;
                const bool pin = pz >= 1 && pz <= q.nz - 2 && py >= 1 && py <= q.ny - 2 && px >= 1 && px <= q.nx - 2;      // the row p is not an identity row
                const double wx = (my * mz) * q.idx2, wy = (mx * mz) * q.idy2, wz = (mx * my) * q.idz2;
                const cplx tx = tabT.x[dx + 1], ty = tabT.y[dy + 1], tz = tabT.z[dz + 1];
                const cplx lap = cmake((tx.x * wx + ty.x * wy) + tz.x * wz, (tx.y * wx + ty.y * wy) + tz.y * wz);
                const cplx a = pin ? cmake(0.5 * lap.x + kap.x * mu, 0.5 * lap.y + kap.y * mu) : cmake(0.0, 0.0);
                cplx t = a;
                if (MODE == PH3_GARDNER) t = pin ? cmake(chi.x * mu + g * a.x, chi.y * mu + g * a.y) : cmake(0.0, 0.0);
                if (centre) a0 = t;
                else {
                    s += t.x * t.x + t.y * t.y;
                    if (MODE == PH3_BLOCKS) { cs.x += mu * a.x; cs.y += mu * a.y; }
                }
                if (MODE == PH3_BLOCKS && pin) smu += mu * mu;
            }
    A0[j] = a0;
    Hh[j] = MODE == PH3_GARDNER ? 0.5 * g : 0.5;
    S[j] = s;
    if (MODE == PH3_BLOCKS) { C[j] = cs; Smu[j] = smu; }
}

struct Ph3Planes {
    const cplx *A0; const double *h, *S; const cplx *C; const double *Smu;      // the planes of k_ph3_coefficients (C, Smu: blocks alone)
    const cplx *c; const double *rho; cplx om;                                    // the model of the handle (blocks alone: chi and the density factors)
};

// H[i] += alpha W_i (S'_i E + D) (W NULL: no weight); BLOCKS: the rows H_cc, H_crho, H_rhorho at stride ldh,
//     H[i] += alpha W_i |chi|^2 Smu E,   H[ldh + i] += -alpha W_i b^2 Re conj(chi) (C' E + mu_0 [i interior] Y),   H[2 ldh + i] += alpha W_i b^4 (S' E + D)
// over the columns s = 0 .. nsrc - 1 of U, X_s = U_s or (CONJ) conj(U_s) as it is staged.  A boundary cell forms no sum (T = 0, A0 = 0: only E accumulates).
// Per cell and column 16 bytes read (times the halo factor across planes, from L2); per cell 8 (24) bytes of H read and written, once.
template <bool CONJ, bool BLOCKS>
__global__ __launch_bounds__(256) void k_ph3_moments(const cplx *__restrict__ U, int nsrc, long long ldu, Ph3Planes k, double alpha, const double *__restrict__ W,
                                                     double *__restrict__ H, long long ldh, Lap3Params q) {
    __shared__ cplx tile[2][D3NEL];
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
    }
    const Lap3Tab tab = lap3_row_tables(q, ok, col, row, T.iz);
    const cplx a0 = inside ? k.A0[idx] : cmake(0.0, 0.0);
    const double hh = inside ? k.h[idx] : 0.0;
    auto prefetch = [&](int s) {
        const cplx *Us = U + (long long)s * ldu;
#pragma unroll
        for (int l = 0; l < D3NLOAD; ++l) pre[l] = cell[l] >= 0 ? Us[cell[l]] : cmake(0.0, 0.0);
    };
    prefetch(0);
    const int ce = wy * D3LW + lane;   // the tile element of the cell's (-1, -1, -1) neighbour
    double E = 0.0, D = 0.0, Yr = 0.0, Yi = 0.0;
    int buf = 0;
    for (int s = 0; s < nsrc; ++s, buf ^= 1) {
#pragma unroll
        for (int l = 0; l < D3NLOAD; ++l) {
            const int e = tid + 256 * l;
            if (e < D3NEL) tile[buf][e] = CONJ ? cconj(pre[l]) : pre[l];
        }
        if (s + 1 < nsrc) prefetch(s + 1);
        __syncthreads();               // (one barrier per column: the buffer written two columns from now was last read before the NEXT barrier)
        const cplx *tb = &tile[buf][ce];
        const cplx u = tb[D3PLANE + D3LW + 1];
        E += u.x * u.x + u.y * u.y;
        if (inside) {                  // (a boundary cell forms no sum)
            const cplx t = lap3_sum(tab, q.idx2, q.idy2, q.idz2, [&](int p, int r, int cc) { return tb[p * D3PLANE + r * D3LW + cc]; });
            cplx r = cmul(a0, u);
            r.x += hh * t.x; r.y += hh * t.y;
            D += r.x * r.x + r.y * r.y;
            if (BLOCKS) { Yr += u.x * r.x + u.y * r.y; Yi += u.x * r.y - u.y * r.x; }          // conj(u) r
        }
    }
    if (!ok) return;
    const double w = W ? alpha * W[idx] : alpha;
    const double hbb = k.S[idx] * E + D;
    if (!BLOCKS) { H[idx] += w * hbb; return; }
    const cplx cj = k.c[idx];
    const double b = 1.0 / k.rho[idx], b2 = b * b;
    const cplx chi = chi3(kappa3s(cmul(k.om, k.om), cj), b, cj), cp = k.C[idx];
    const double mu0 = 0.5 + 0.5 * (D3M0 * D3M0 * D3M0);
    cplx x = cmake(cp.x * E, cp.y * E);
    if (inside) { x.x += mu0 * Yr; x.y += mu0 * Yi; }
    H[idx] += w * ((chi.x * chi.x + chi.y * chi.y) * k.Smu[idx] * E);
    H[ldh + idx] += -(w * b2) * (chi.x * x.x + chi.y * x.y);                                    // Re conj(chi) x
    H[2 * ldh + idx] += (w * (b2 * b2)) * hbb;
}

}  // namespace

extern "C" int helm_ph3_coefficients_device(helm_op *op, int mode, void *dA0, void *dH, void *dS, void *dC, void *dSmu) {
    helm_tuning_refresh();
    if (!op || !dA0 || !dH || !dS || mode < PH3_BUOYANCY || mode > PH3_BLOCKS || (mode == PH3_BLOCKS && (!dC || !dSmu))) return HELM_ERR_ARG;
    { const int rc = buoy3_handle_args(op, "helm_ph3_coefficients_device"); if (rc) return rc; }
    if (((((uintptr_t)dA0) | ((uintptr_t)dC)) & 15) || ((((uintptr_t)dH) | ((uintptr_t)dS) | ((uintptr_t)dSmu)) & 7)) return HELM_ERR_ARG;
    const size_t nd = sizeof(double) * (size_t)op->N, nc = sizeof(cplx) * (size_t)op->N;
    const void *pl[5] = {dA0, dH, dS, mode == PH3_BLOCKS ? dC : nullptr, mode == PH3_BLOCKS ? dSmu : nullptr};
    const size_t nb[5] = {nc, nd, nd, nc, nd};
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b)
            if (pl[a] && pl[b] && ranges_overlap(pl[a], nb[a], pl[b], nb[b])) return HELM_ERR_ARG;
    Lap3Params q;
    int nblk;
    { const int rc = lap3_params(op, "helm_ph3_coefficients_device", &q, &nblk); if (rc) return rc; }
    HIP_TRY(op, hipSetDevice(op->device));
    const cplx om = damped_omega3(op);
    const dim3 grid((unsigned)((op->N + 255) / 256));
#define PH3_COEF(M) HELM_LAUNCH((k_ph3_coefficients<M>), grid, dim3(256), 0, op->stream, (const cplx *)op->d_c, (const double *)op->d_rho, om, (cplx *)dA0, (double *)dH, \
                                (double *)dS, (cplx *)dC, (double *)dSmu, q)
    if (mode == PH3_BUOYANCY) PH3_COEF(PH3_BUOYANCY);
    else if (mode == PH3_GARDNER) PH3_COEF(PH3_GARDNER);
    else PH3_COEF(PH3_BLOCKS);
#undef PH3_COEF
    return launched(op);
}

extern "C" int helm_ph3_moments_accumulate_device(helm_op *op, const void *dU, int nsrc, long long ldu, int conj, int blocks, const void *dA0, const void *dHh,
                                                  const void *dS, const void *dC, const void *dSmu, double alpha, const void *dW, void *dH, long long ldh) {
    helm_tuning_refresh();
    if (!op || !dU || !dA0 || !dHh || !dS || !dH || nsrc < 1 || ldu < op->N || (blocks && (!dC || !dSmu || ldh < op->N))) return HELM_ERR_ARG;
    { const int rc = buoy3_handle_args(op, "helm_ph3_moments_accumulate_device"); if (rc) return rc; }
    if (((((uintptr_t)dU) | ((uintptr_t)dA0) | ((uintptr_t)dC)) & 15) || ((((uintptr_t)dHh) | ((uintptr_t)dS) | ((uintptr_t)dSmu) | ((uintptr_t)dW) | ((uintptr_t)dH)) & 7))
        return HELM_ERR_ARG;
    const size_t nd = sizeof(double) * (size_t)op->N, nc = sizeof(cplx) * (size_t)op->N;
    const size_t nh = blocks ? sizeof(double) * (2 * (size_t)ldh + op->N) : nd;
    if (ranges_overlap(dH, nh, dU, sizeof(cplx) * ((size_t)(nsrc - 1) * ldu + op->N)) || ranges_overlap(dH, nh, dA0, nc) || ranges_overlap(dH, nh, dHh, nd) ||
        ranges_overlap(dH, nh, dS, nd) || (dW && ranges_overlap(dH, nh, dW, nd)) || (blocks && (ranges_overlap(dH, nh, dC, nc) || ranges_overlap(dH, nh, dSmu, nd))))
        return HELM_ERR_ARG;
    Lap3Params q;
    int nblk;
    { const int rc = lap3_params(op, "helm_ph3_moments_accumulate_device", &q, &nblk); if (rc) return rc; }
    HIP_TRY(op, hipSetDevice(op->device));
    const Ph3Planes k = {(const cplx *)dA0, (const double *)dHh, (const double *)dS, (const cplx *)dC, (const double *)dSmu, (const cplx *)op->d_c,
                         (const double *)op->d_rho, damped_omega3(op)};
    const dim3 grid((unsigned)nblk);       // (one workgroup walks every column of its tile: the sum over s has one order)
#define PH3_MOM(C, B) HELM_LAUNCH((k_ph3_moments<C, B>), grid, dim3(256), 0, op->stream, (const cplx *)dU, nsrc, ldu, k, alpha, (const double *)dW, (double *)dH, ldh, q)
    if (conj) { if (blocks) PH3_MOM(true, true); else PH3_MOM(true, false); }
    else { if (blocks) PH3_MOM(false, true); else PH3_MOM(false, false); }
#undef PH3_MOM
    return launched(op);
}
