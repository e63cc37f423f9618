// The derivative kernels of the 3-D 27-point operator on stored columns, each beside the C entry point that launches it.
//
// With an explicit density the whole derivative of the 3-D operator along the velocity is its mass term (helm3d.hip: bbar and the stretch factors do not
// depend on c):  dA[dc] = M~ diag(dK),  dK_j = chi_j dc_j,  chi = -2 K / c,  K = om~^2 / (rho c^2).  M~ is the constant 27-point stencil
//     mu_o = a [o == 0] + (1 - a) m(ox) m(oy) m(oz),   a = 1/2, m(0) = 2/3, m(+-1) = 1/6,
// with the rows on the box boundary zeroed (identity rows of A do not move); an interior row never reads outside the grid.  Helm3DProblem.JvecBorn needs
// M~ applied to W (.) U_s on the way to the solver (k_mass3_sources) and Helm3DProblem.Jtvec(adjoint='transpose') its transpose applied to the back-propagated
// columns inside the imaging sum (k_mass3_imaging): the weights are symmetric, so M~^T L is the same mu sum over L with the boundary ROWS OF L masked to zero.
// Neither reads 27 planes: the weights are compile-time constants, the mask comes from the indices.
//
// Both walk the grid as k_stencil3 does (helm3d.hip): a workgroup of 256 takes a 64 x 4 tile of one z-plane, stages the three z-planes of a column with halo in
// LDS (3 x 6 x 66 elements, double-buffered: 38 KB), tiles ordered z fastest so that the workgroups in flight share their halo planes in L2, and loops over the
// columns inside the workgroup with the next column's loads in flight.  The 27-point sum is formed separably in an order the code fixes,
//     row(p, r)  = m0 t(0) + m1 (t(-1) + t(+1))            along x
//     plane(p)   = m0 row(p, 0) + m1 (row(p, -1) + row(p, +1))   along y
//     sep        = m0 plane(0) + m1 (plane(-1) + plane(+1))      along z
//     sum        = a t_centre + (1 - a) sep
// so the same bits come out of every run.  No atomics.
#include "survey_internal.hpp"

namespace {

constexpr int S3X = 64, S3Y = 4;                       // the tile of k_stencil3
constexpr int S3LW = S3X + 2, S3LH = S3Y + 2;
constexpr int S3PLANE = S3LW * S3LH;                   // 396 elements of one staged plane
constexpr int S3NEL = 3 * S3PLANE;
constexpr int S3NLOAD = (S3NEL + 255) / 256;           // elements staged per thread
constexpr double S3M0 = 2.0 / 3.0, S3M1 = 1.0 / 6.0, S3BLEND = 0.5;

// where a workgroup works: tile (tx, ty) of plane iz, z fastest
struct Tile3 {
    int iz, x0, y0;
    __device__ __forceinline__ Tile3(int nz, int ntx) {
        const int t = blockIdx.x;
        iz = t % nz; x0 = ((t / nz) % ntx) * S3X; y0 = (t / (nz * ntx)) * S3Y;
    }
};
// element e of the staged tile -> its global cell, -1 where that lies outside the grid; bnd: the cell is on the box boundary
__device__ __forceinline__ long long tile3_cell(const Tile3 &T, int e, int nz, int ny, int nx, bool &bnd) {
    const int p = e / S3PLANE, rem = e - p * S3PLANE, r = rem / S3LW, cc = rem - r * S3LW;
    const int gz = T.iz - 1 + p, gy = T.y0 - 1 + r, gx = T.x0 - 1 + cc;
    bnd = gz == 0 || gz == nz - 1 || gy == 0 || gy == ny - 1 || gx == 0 || gx == nx - 1;
    if (gz < 0 || gz >= nz || gy < 0 || gy >= ny || gx < 0 || gx >= nx) return -1;
    return ((long long)gz * ny + gy) * nx + gx;
}
// the mu sum at the thread's cell from a staged tile (tb: the tile element of the cell's (-1, -1, -1) neighbour)
__device__ __forceinline__ cplx mass3_sum(const cplx *tb) {
    cplx pl[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        cplx rw[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const cplx *q = tb + p * S3PLANE + r * S3LW;
            rw[r] = cmake(S3M0 * q[1].x + S3M1 * (q[0].x + q[2].x), S3M0 * q[1].y + S3M1 * (q[0].y + q[2].y));
        }
        pl[p] = cmake(S3M0 * rw[1].x + S3M1 * (rw[0].x + rw[2].x), S3M0 * rw[1].y + S3M1 * (rw[0].y + rw[2].y));
    }
    const cplx sep = cmake(S3M0 * pl[1].x + S3M1 * (pl[0].x + pl[2].x), S3M0 * pl[1].y + S3M1 * (pl[0].y + pl[2].y));
    const cplx ctr = tb[S3PLANE + S3LW + 1];
    return cmake(S3BLEND * ctr.x + (1.0 - S3BLEND) * sep.x, S3BLEND * ctr.y + (1.0 - S3BLEND) * sep.y);
}

// R[s ldr + i] = coef M~(W (.) X_s)[i], X_s = U_s or (CONJ) conj(U_s), for the columns s = blockIdx.y, blockIdx.y + gridDim.y, ... < nsrc.  The PRODUCTS are
// staged, so that the 27-point sum runs over W (.) X_s; a thread keeps the W of the elements it stages in registers over the column loop.  The boundary rows of R
// are written as exact zeros.  Per cell and column 16 bytes read (times the halo factor (6 x 66 x 3) / (4 x 64 x 3) across planes: 1.55 from L2) and 16 written.
template <bool CONJ>
__global__ __launch_bounds__(256) void k_mass3_sources(const cplx *__restrict__ U, int nsrc, long long ldu, const cplx *__restrict__ W, cplx coef,
                                                       cplx *__restrict__ R, long long ldr, int nz, int ny, int nx, int ntx) {
    __shared__ cplx tile[2][S3NEL];
    const int tid = threadIdx.x, lane = tid & 63, wy = tid >> 6;
    const Tile3 T(nz, ntx);
    const int col = T.x0 + lane, row = T.y0 + wy;
    const bool ok = col < nx && row < ny;
    const bool inside = ok && col >= 1 && col <= nx - 2 && row >= 1 && row <= ny - 2 && T.iz >= 1 && T.iz <= nz - 2;
    const long long idx = ((long long)T.iz * ny + row) * nx + col;
    long long cell[S3NLOAD];
    cplx w[S3NLOAD], pre[S3NLOAD];
#pragma unroll
    for (int l = 0; l < S3NLOAD; ++l) {
        const int e = tid + 256 * l;
        bool bnd;
        cell[l] = e < S3NEL ? tile3_cell(T, e, nz, ny, nx, bnd) : -1;
        w[l] = cell[l] >= 0 ? W[cell[l]] : cmake(0.0, 0.0);
    }
    auto prefetch = [&](int s) {
        const cplx *Us = U + (long long)s * ldu;
#pragma unroll
        for (int l = 0; l < S3NLOAD; ++l) pre[l] = cell[l] >= 0 ? Us[cell[l]] : cmake(0.0, 0.0);
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int l = 0; l < S3NLOAD; ++l) {
            const int e = tid + 256 * l;
            if (e < S3NEL) tile[buf][e] = cmul(w[l], CONJ ? cconj(pre[l]) : pre[l]);
        }
    };
    int s = blockIdx.y, buf = 0;
    if (s < nsrc) prefetch(s);
    for (; s < nsrc; s += gridDim.y, buf ^= 1) {
        stage(buf);
        if (s + (int)gridDim.y < nsrc) prefetch(s + gridDim.y);
        __syncthreads();               // (one barrier per column: the buffer written two columns from now was last read before the NEXT barrier)
        if (ok) R[(long long)s * ldr + idx] = inside ? cmul(coef, mass3_sum(&tile[buf][wy * S3LW + lane])) : cmake(0.0, 0.0);
    }
}

// P[j] += sum_{s<nsrc} UF[s ldf + j] (M~^T L_s)[j], L_s = UB[s ldb + .]: the boundary rows of L are masked to zero WHILE STAGING (whatever they hold is never
// multiplied), every cell j of the grid -- boundary nodes included, they are columns of interior rows -- receives its sum.  s ascending in one register per
// thread, one load and one store of P per cell, no atomics.  Per cell 16 bytes of UF and 16 of UB per column (the latter times the halo factor), 32 of P.
__global__ __launch_bounds__(256) void k_mass3_imaging(const cplx *__restrict__ UF, long long ldf, const cplx *__restrict__ UB, long long ldb, int nsrc,
                                                       cplx *__restrict__ P, int nz, int ny, int nx, int ntx) {
    __shared__ cplx tile[2][S3NEL];
    const int tid = threadIdx.x, lane = tid & 63, wy = tid >> 6;
    const Tile3 T(nz, ntx);
    const int col = T.x0 + lane, row = T.y0 + wy;
    const bool ok = col < nx && row < ny;
    const long long idx = ((long long)T.iz * ny + row) * nx + col;
    long long cell[S3NLOAD];
    cplx pre[S3NLOAD], uf;
#pragma unroll
    for (int l = 0; l < S3NLOAD; ++l) {
        const int e = tid + 256 * l;
        bool bnd = true;
        cell[l] = e < S3NEL ? tile3_cell(T, e, nz, ny, nx, bnd) : -1;
        if (bnd) cell[l] = -1;         // (mask_int: a boundary row of L is not even loaded)
    }
    auto prefetch = [&](int s) {
        const cplx *Ls = UB + (long long)s * ldb;
#pragma unroll
        for (int l = 0; l < S3NLOAD; ++l) pre[l] = cell[l] >= 0 ? Ls[cell[l]] : cmake(0.0, 0.0);
        uf = ok ? UF[(long long)s * ldf + idx] : cmake(0.0, 0.0);
    };
    cplx acc = cmake(0.0, 0.0);
    int buf = 0;
    prefetch(0);
    for (int s = 0; s < nsrc; ++s, buf ^= 1) {
#pragma unroll
        for (int l = 0; l < S3NLOAD; ++l) {
            const int e = tid + 256 * l;
            if (e < S3NEL) tile[buf][e] = pre[l];
        }
        const cplx ufs = uf;
        if (s + 1 < nsrc) prefetch(s + 1);
        __syncthreads();
        cfma(acc, ufs, mass3_sum(&tile[buf][wy * S3LW + lane]));
    }
    if (ok) { const cplx p = P[idx]; P[idx] = cmake(p.x + acc.x, p.y + acc.y); }
}

// K = om~^2 / (rho c^2) of one cell: the expression of kfield3 (helm3d.hip), contraction pinned as there, so that chi is formed from the K the assembly used
__device__ __forceinline__ cplx kfield3s(cplx om2, cplx cj, double rj) {
#pragma clang fp contract(off)
    const double br = (cj.x * cj.x - cj.y * cj.y) * rj, bi = (cj.x * cj.y + cj.y * cj.x) * rj;
    if (fabs(br) >= fabs(bi)) {
        const double r = bi / br, d = br + bi * r;
        return cmake((om2.x + om2.y * r) / d, (om2.y - om2.x * r) / d);
    }
    const double r = br / bi, d = br * r + bi;
    return cmake((om2.x * r + om2.y) / d, (om2.y * r - om2.x) / d);
}
__device__ __forceinline__ cplx cdiv3(cplx a, cplx b) {
    if (fabs(b.x) >= fabs(b.y)) { const double r = b.y / b.x, d = b.x + b.y * r; return cmake((a.x + a.y * r) / d, (a.y - a.x * r) / d); }
    const double r = b.x / b.y, d = b.x * r + b.y;
    return cmake((a.x * r + a.y) / d, (a.y * r - a.x) / d);
}
// One lane per cell, chi_j = -2 K_j / c_j.  dc given (Born): out is N complex128, out[j] = w chi_j dc[j].  dc NULL (gradient): out is N float64,
// out[j] += Re(w chi_j P[j]).
__global__ __launch_bounds__(256) void k_mass3_chain(const cplx *__restrict__ c, const double *__restrict__ rho, cplx om, const cplx *__restrict__ P, cplx w,
                                                     const double *__restrict__ dc, void *__restrict__ out, long long N) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    const cplx cj = c[j];
    const cplx K = kfield3s(cmul(om, om), cj, rho[j]);      // (om~^2 formed on the device, as k_assemble_3d forms it)
    const cplx chi = cdiv3(cmake(-2.0 * K.x, -2.0 * K.y), cj);
    const cplx wc = cmul(w, chi);
    if (dc) { const double d = dc[j]; static_cast<cplx *>(out)[j] = cmake(wc.x * d, wc.y * d); }
    else { const cplx p = P[j]; static_cast<double *>(out)[j] += wc.x * p.x - wc.y * p.y; }
}

int helm3_handle_args(helm_op *op, const char *what) {
    if (op->variant != HELM_3D || op->ny <= 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "%s: the mass stencil of this derivative is that of the 3-D 27-point operator (a helm_create3d handle)", what);
    return HELM_OK;
}
inline int tiles3(const helm_op *op, int *ntx) {
    *ntx = (op->nx + S3X - 1) / S3X;
    return *ntx * ((op->ny + S3Y - 1) / S3Y) * op->nz;
}

}  // namespace

extern "C" int helm_mass3_sources_device(helm_op *op, const void *dU, int nsrc, long long ldu, const void *dW, double coef_re, double coef_im, int conj, void *dR,
                                         long long ldr) {
    helm_tuning_refresh();
    if (!op || !dU || !dW || !dR || nsrc < 1 || ldu < op->N || ldr < op->N) return HELM_ERR_ARG;
    { const int rc = helm3_handle_args(op, "helm_mass3_sources_device"); if (rc) return rc; }
    if ((((uintptr_t)dU) | ((uintptr_t)dW) | ((uintptr_t)dR)) & 15) return HELM_ERR_ARG;
    const size_t nb = sizeof(cplx) * (size_t)op->N;
    if (ranges_overlap(dR, sizeof(cplx) * ((size_t)(nsrc - 1) * ldr + op->N), dU, sizeof(cplx) * ((size_t)(nsrc - 1) * ldu + op->N)) ||
        ranges_overlap(dR, sizeof(cplx) * ((size_t)(nsrc - 1) * ldr + op->N), dW, nb)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    int ntx;
    const int nblk = tiles3(op, &ntx);
    int split = 1;                      // few tiles: the columns are spread over grid.y, as helm3d_launch_apply spreads its right-hand sides
    if (nblk < 2048) { split = (2048 + nblk - 1) / nblk; if (split > nsrc) split = nsrc; if (split > 65535) split = 65535; }
    const dim3 grid((unsigned)nblk, (unsigned)split);
    const cplx coef = cmake(coef_re, coef_im);
    if (conj) HELM_LAUNCH((k_mass3_sources<true>), grid, dim3(256), 0, op->stream, (const cplx *)dU, nsrc, ldu, (const cplx *)dW, coef, (cplx *)dR, ldr, op->nz, op->ny, op->nx, ntx);
    else HELM_LAUNCH((k_mass3_sources<false>), grid, dim3(256), 0, op->stream, (const cplx *)dU, nsrc, ldu, (const cplx *)dW, coef, (cplx *)dR, ldr, op->nz, op->ny, op->nx, ntx);
    return launched(op);
}

extern "C" int helm_mass3_imaging_accumulate_device(helm_op *op, const void *dUF, long long ldf, const void *dUB, long long ldb, int nsrc, void *dP) {
    helm_tuning_refresh();
    if (!op || !dUF || !dUB || !dP || nsrc < 1 || ldf < op->N || ldb < op->N) return HELM_ERR_ARG;
    { const int rc = helm3_handle_args(op, "helm_mass3_imaging_accumulate_device"); if (rc) return rc; }
    if ((((uintptr_t)dUF) | ((uintptr_t)dUB) | ((uintptr_t)dP)) & 15) return HELM_ERR_ARG;
    const size_t nb = sizeof(cplx) * (size_t)op->N;
    if (ranges_overlap(dP, nb, dUF, sizeof(cplx) * ((size_t)(nsrc - 1) * ldf + op->N)) || ranges_overlap(dP, nb, dUB, sizeof(cplx) * ((size_t)(nsrc - 1) * ldb + op->N))) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    int ntx;
    const int nblk = tiles3(op, &ntx);
    HELM_LAUNCH(k_mass3_imaging, dim3((unsigned)nblk), dim3(256), 0, op->stream, (const cplx *)dUF, ldf, (const cplx *)dUB, ldb, nsrc, (cplx *)dP, op->nz, op->ny, op->nx, ntx);
    return launched(op);
}

extern "C" int helm_mass3_chain_device(helm_op *op, const void *dP, double w_re, double w_im, const void *dDc, void *dOut) {
    helm_tuning_refresh();
    if (!op || !dOut || (!dP && !dDc)) return HELM_ERR_ARG;
    { const int rc = helm3_handle_args(op, "helm_mass3_chain_device"); if (rc) return rc; }
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "helm_mass3_chain_device: the handle is not assembled (chi is formed at the frequency of its last assembly)");
    if (((uintptr_t)dOut & (dDc ? 15 : 7)) || ((uintptr_t)dDc & 7) || ((uintptr_t)dP & 15)) return HELM_ERR_ARG;
    HIP_TRY(op, hipSetDevice(op->device));
    cplx om = cmake(2.0 * M_PI * op->a_freq_re, 2.0 * M_PI * op->a_freq_im);
    if (std::isfinite(op->a_tau) && op->a_tau != 0.0) om.y -= 1.0 / op->a_tau;
    HELM_LAUNCH(k_mass3_chain, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)op->d_c, (const double *)op->d_rho, om,
                       (const cplx *)dP, cmake(w_re, w_im), (const double *)dDc, dOut, op->N);
    return launched(op);
}
