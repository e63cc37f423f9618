// Coefficient assembly on the GPU: model (c, rho[, theta, eps, delta]) -> 9 (MiniZephyr) or
// 4 x 9 (Eurus) complex planes resident in HBM, bug-compatible with the reference.
//
//   MiniZephyr: zephyr/backend/minizephyr.py:40-298   (OMEGA-style 9-point star, Roecker PML)
//   Eurus:      zephyr/backend/eurus.py:28-485        (Operto 2009 mixed-grid TTI, C-PML)
//
// One thread per grid point; everything is elementwise on (c, rho) with clamped ("edge"
// padded) neighbour reads, so the kernel is a coalesced streaming pass: it runs once per
// frequency and is not on the per-iteration path.
//
// Also here: what is derived from the planes or the model once per operator -- the Jacobi-scaled planes (k_scale_planes), the
// row-equilibrated coupled Eurus system (k_rowscale_system) and Gardner's density (k_gardner_rho).
#include "helm_internal.hpp"
#include "mz_row.hpp"
#include "eu_row.hpp"

namespace {

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__host__ __device__ inline int slot(int dz, int dx) { return mz_slot(dz, dx); }

// MiniZephyr: minizephyr.py:98-133 (PML), :169-202 (buoyancy / K), :219-243 (star), :269-298 (edges)
__global__ __launch_bounds__(256) void k_assemble_mz(MzParams P, const cplx *__restrict__ c,
                                                     const double *__restrict__ rho,
                                                     const double *__restrict__ distx, const double *__restrict__ sgnx,
                                                     const double *__restrict__ distz, const double *__restrict__ sgnz,
                                                     cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);

    // PML stretch factors from the local (unpadded) velocity (mz_row.hpp: the buoyancy derivative of survey_frechet.hip takes the same)
    const MzRow row = mz_row_factors(P, c[i], distx[ix], sgnx[ix], distz[iz], sgnz[iz]);

    // neighbour properties with edge padding
    double bn[9];
    cplx Kn[9];
    const double b0 = 1.0 / rho[i];
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int jz = clampi(iz + sz, 0, P.nz - 1), jx = clampi(ix + sx, 0, P.nx - 1);
            const long long j = (long long)jz * P.nx + jx;
            const double r = rho[j];
            const cplx cj = c[j];
            bn[slot(sz, sx)] = (b0 + 1.0 / r) / 2.0;
            const cplx k = mz_kappa(P, cj);
            Kn[slot(sz, sx)] = cmake(k.x / r, k.y / r);
        }

    cplx out[9];
    mz_star(P, row, bn, Kn, out);

    // boundary rows: +/- identity, write order left, right, iz=0, iz=nz-1 (later wins)
    int edge = -1;
    if (ix == 0) edge = 3;
    if (ix == P.nx - 1) edge = 1;
    if (iz == 0) edge = 0;
    if (iz == P.nz - 1) edge = 2;
    if (edge >= 0) {
        const int f = edge == 0 ? P.fs0 : edge == 1 ? P.fs1 : edge == 2 ? P.fs2 : P.fs3;
#pragma unroll
        for (int k = 0; k < 9; ++k) out[k] = cmake(0.0, 0.0);
        out[4] = cmake(f ? -1.0 : 1.0, 0.0);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) C[(long long)k * N + i] = out[k];
}

// Eurus: eurus.py:140-168 (PML averages), :170-226 (buoyancy squares/lines), :229-269 (mass),
// :279-295 (TTI fields), :300-427 (the nine entries), :479-485 (edges), :117-127 (z-flipped slots); the formulas themselves are eu_row.hpp's
__global__ __launch_bounds__(256) void k_assemble_eurus(EuParams P, const cplx *__restrict__ c,
                                                        const double *__restrict__ rho,
                                                        const double *__restrict__ theta, const double *__restrict__ eps,
                                                        const double *__restrict__ delta,
                                                        const cplx *__restrict__ xix, const cplx *__restrict__ xiz,
                                                        cplx *__restrict__ C) {
    const long long N = (long long)P.nz * P.nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / P.nx), ix = (int)(i % P.nx);

    // padded 1-D PML profiles: index p = i+1
    const cplx xl = xix[ix], xc = xix[ix + 1], xr = xix[ix + 2];
    const cplx zl = xiz[iz], zc = xiz[iz + 1], zr = xiz[iz + 2];
    const EuPml pml = eu_pml_of(P.dx, P.dz, xl, xc, xr, zl, zc, zr);

    double b[9];
    cplx K[9];
    const cplx om2 = cmul(P.om, P.om);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int jz = clampi(iz + sz, 0, P.nz - 1), jx = clampi(ix + sx, 0, P.nx - 1);
            const long long j = (long long)jz * P.nx + jx;
            const double r = rho[j];
            const cplx cj = c[j];
            b[slot(sz, sx)] = 1.0 / r;
            K[slot(sz, sx)] = cdiv(om2, cscale(cmul(cj, cj), r));
        }
    const EuStiff stiff = eu_stiffness(pml, b);
    cplx Kw[9];
    eu_mass_weighted(K, Kw);

    double th = 0, ep = 0, de = 0;
    if (P.aniso) { th = theta ? theta[i] : 0.0; ep = eps ? eps[i] : 0.0; de = delta ? delta[i] : 0.0; }
    const EuTti t = eu_tti(th, ep, de);
    const double massv[4] = {1.0, 0.0, 0.0, 1.0};
    const double c1xv[4] = {t.Ax, t.Cx, t.Ex, t.Ex}, c1zv[4] = {t.Bx, t.Dx, t.Fx, t.Fx};
    const double c2xv[4] = {t.Bx, t.Dx, t.Fx, t.Fx}, c2zv[4] = {t.Bz, t.Dz, t.Fz, t.Fz};

    const bool edge = (ix == 0) || (ix == P.nx - 1) || (iz == 0) || (iz == P.nz - 1);

#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m >= P.nblk_out) break;
        const EuEntries e = eu_row_entries(pml, stiff, Kw, massv[m], c1xv[m], c1zv[m], c2xv[m], c2zv[m]);
        // nine locals, not e.GG .. e.CC in the stores: `edge ? zero : X` selects between addresses, and against the struct the kernel takes 16 bytes more stack
        const cplx GG = e.GG, HH = e.HH, II = e.II, DD = e.DD, EE = e.EE, FF = e.FF, AA = e.AA, BB = e.BB, CC = e.CC;

        const cplx zero = cmake(0.0, 0.0);
        cplx *Cm = C + (long long)m * 9 * N;
        // matrix slots with the reference's mord = (-nx, +1): property row index-1 couples to u(iz+1)
        Cm[(long long)slot(1, -1) * N + i] = edge ? zero : GG;
        Cm[(long long)slot(1, 0) * N + i] = edge ? zero : HH;
        Cm[(long long)slot(1, 1) * N + i] = edge ? zero : II;
        Cm[(long long)slot(0, -1) * N + i] = edge ? zero : DD;
        Cm[(long long)slot(0, 0) * N + i] = EE;
        Cm[(long long)slot(0, 1) * N + i] = edge ? zero : FF;
        Cm[(long long)slot(-1, -1) * N + i] = edge ? zero : AA;
        Cm[(long long)slot(-1, 0) * N + i] = edge ? zero : BB;
        Cm[(long long)slot(-1, 1) * N + i] = edge ? zero : CC;
    }
}

// The planes of A^T from the planes of A.  Row i of A holds A[i][i + off_k] = C[k][i] with k = 3 (dz + 1) + (dx + 1), off_k = dz nx + dx; hence
// A^T[i][i + off_k] = A[i + off_k][i] = C[8 - k][i + off_k] (slot 8 - k is the offset -off_k), and zero where cell (iz + dz, ix + dx) lies outside the grid.
// The test is per axis: i + off_k of a cell at a row end is a valid linear index of the NEXT grid row.  Pure data movement, out of place: one lane per
// cell, nine loads and nine stores that are each contiguous across the wave (neighbouring lanes read neighbouring cells of one plane), no atomics.
__global__ __launch_bounds__(256) void k_transpose_planes(const cplx *__restrict__ C, cplx *__restrict__ CT, int nz, int nx) {
    const long long N = (long long)nz * nx;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int iz = (int)(i / nx), ix = (int)(i % nx);
    cplx v[9];
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int k = slot(dz, dx);
            const bool in = iz + dz >= 0 && iz + dz < nz && ix + dx >= 0 && ix + dx < nx;
            v[k] = in ? C[(long long)(8 - k) * N + i + (long long)dz * nx + dx] : cmake(0.0, 0.0);
        }
#pragma unroll
    for (int k = 0; k < 9; ++k) CT[(long long)k * N + i] = v[k];
}

// 1-D profile builders (host).  MiniZephyr: minizephyr.py:98-118,126-127 (assignment order kept).
void mz_profiles(int n, int npml, double h, bool fs_low, bool fs_high, std::vector<double> &dist, std::vector<double> &sgn) {
    dist.assign(n, 0.0);
    sgn.assign(n, 0.0);
    // numpy slice semantics a[:npml] / a[-npml:] clip to the array
    const int lo_len = npml < n ? npml : n;
    for (int k = 0; k < lo_len; ++k) dist[k] = (double)(npml - k) * h;
    const int hi_start = n - npml > 0 ? n - npml : 0;
    // a[-npml:] = arange(1..npml): when npml > n numpy would raise; we keep the tail-aligned values
    for (int k = hi_start; k < n; ++k) dist[k] = (double)(k - (n - npml) + 1) * h;
    if (!fs_high) for (int k = hi_start; k < n; ++k) sgn[k] = -1.0;
    if (!fs_low) for (int k = 0; k < lo_len; ++k) sgn[k] = 1.0;
}

// ---- what the solvers derive from the assembled planes and the model -------------------------------------
// Jacobi scaling: Cs = planes divided by the centre plane, dinv = 1 / centre plane
__global__ __launch_bounds__(256) void k_scale_planes(const cplx *__restrict__ C, cplx *__restrict__ Cs,
                                                      cplx *__restrict__ dinv, long long N, int nblocks, double floor_frac,
                                                      int nplanes, int centre) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    for (int m = 0; m < nblocks; ++m) {
        const cplx *Cm = C + (long long)m * nplanes * N;
        cplx *Sm = Cs + (long long)m * nplanes * N;
        cplx d = Cm[(long long)centre * N + i];
        const bool zero = (d.x == 0.0 && d.y == 0.0);
        if (floor_frac > 0.0 && !zero) {
            // smoother safeguard on multigrid levels: where the diagonal nearly cancels (k h ~ 2: mass term
            // against the Laplacian) keep its phase but not less than floor_frac of the row's absolute sum
            double rows = 0.0;
            for (int k = 0; k < nplanes; ++k) rows += sqrt(cabs2(Cm[(long long)k * N + i]));
            const double ad = sqrt(cabs2(d));
            if (ad < floor_frac * rows) d = cscale(d, floor_frac * rows / ad);
        }
        const cplx di = zero ? cmake(0.0, 0.0) : crecip(d);
        dinv[(long long)m * N + i] = di;
        for (int k = 0; k < nplanes; ++k) Sm[(long long)k * N + i] = (k == centre) ? cmake(1.0, 0.0) : cmul(Cm[(long long)k * N + i], di);
    }
}

// Row equilibration of the coupled two-field Eurus system [[M1, M2], [M3, M4]]: every system row is divided by its
// 2-norm (the diagonal of M4 nearly vanishes where eps ~ delta, so Jacobi scaling is useless there).
__global__ __launch_bounds__(256) void k_rowscale_system(const cplx *__restrict__ C, cplx *__restrict__ S, double *__restrict__ rs, long long N) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        double n2 = 0.0;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int k = 0; k < 9; ++k) n2 += cabs2(C[((long long)(2 * row + blk) * 9 + k) * N + i]);
        const double inv = n2 > 0.0 ? 1.0 / sqrt(n2) : 0.0;
        rs[(long long)row * N + i] = inv;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const long long idx = ((long long)(2 * row + blk) * 9 + k) * N + i;
                S[idx] = cscale(C[idx], inv);
            }
    }
}

// Gardner's relation, the reference's density default: rho = 310 Re(c)^0.25 (discretization.py:70)
__global__ __launch_bounds__(256) void k_gardner_rho(const cplx *__restrict__ c, double *__restrict__ rho, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        rho[i] = 310.0 * pow(c[i].x, 0.25);
}

}  // namespace

// The padded C-PML profiles xi = 1 - i gamma / omega of an Eurus handle along x (nx + 2) and z (nz + 2), eurus.py:77-97.  np.arange(0, L+h, h) has
// ceil((L+h)/h) entries; the reference breaks (broadcast ValueError) when float rounding makes that != nPML: non-zero then.
static int eu_profiles(const helm_op *op, cplx om, double cPML, std::vector<cplx> &xix, std::vector<cplx> &xiz) {
    auto build = [&](int n, double h, std::vector<cplx> &xi) -> int {
        const double L = h * (op->nPML - 1);
        const int len = (int)ceil((L + h) / h);
        if (len != op->nPML && !op->block0_only) return HELM_ERR_PML;   // preconditioner levels are free of the hazard
        std::vector<double> g(n, 0.0);
        for (int k = 0; k < op->nPML; ++k) g[k] = cPML * cos((M_PI / 2) * ((0.0 + k * h) / L));
        for (int k = 0; k < op->nPML; ++k) g[n - op->nPML + k] = cPML * cos((M_PI / 2) * ((0.0 + (op->nPML - 1 - k) * h) / L));
        xi.resize(n + 2);
        for (int p = 0; p < n + 2; ++p) {
            const int k = p == 0 ? 0 : (p == n + 1 ? n - 1 : p - 1);
            // xi = 1 - (1j*gamma)/om
            cplx q = cdiv(cmake(0.0, g[k]), om);
            xi[p] = cmake(1.0 - q.x, -q.y);
        }
        return 0;
    };
    return (build(op->nx, op->dx, xix) || build(op->nz, op->dz, xiz)) ? HELM_ERR_PML : 0;
}

// MzParams of a handle's grid and PML at a frequency: what k_assemble_mz is launched with
static MzParams mz_params_at(const helm_op *op, cplx om, double ky) {
    MzParams P;
    P.nz = op->nz; P.nx = op->nx; P.dx = op->dx; P.dz = op->dz; P.aky = 2.0 * M_PI * ky; P.om = om;
    const double lx = op->dx * (op->nPML - 1), lz = op->dz * (op->nPML - 1);
    P.fx = op->pml_scale * 3.0 * log(1.0 / 1e-3) / (2.0 * lx * lx * lx);
    P.fz = op->pml_scale * 3.0 * log(1.0 / 1e-3) / (2.0 * lz * lz * lz);
    P.fs0 = op->fs[0]; P.fs1 = op->fs[1]; P.fs2 = op->fs[2]; P.fs3 = op->fs[3]; P.npml = op->nPML;
    return P;
}
// omega~ = 2 pi f - i / tau      (discretization.py:38-41)
static cplx mz_damped_omega(double freq_re, double freq_im, double tau) {
    const double twopi = 2.0 * M_PI;
    cplx om = cmake(twopi * freq_re, twopi * freq_im);
    if (std::isfinite(tau) && tau != 0.0) om.y -= 1.0 / tau;
    return om;
}

// MzParams of the operator the handle holds, from the arguments its last assembly recorded
int helm_mz_params(const helm_op *op, MzParams *P) {
    if (!op || !P || op->variant != HELM_MINIZEPHYR || op->ny > 0 || !op->assembled || op->nPML < 2) return HELM_ERR_ARG;
    *P = mz_params_at(op, mz_damped_omega(op->a_freq_re, op->a_freq_im, op->a_tau), op->a_ky);
    return HELM_OK;
}

// EuParams and the device PML profiles of the Eurus operator the handle holds, from the arguments its last assembly recorded: what the derivative kernels of
// survey_eurus.hip are launched with.  The profiles (nx + nz + 4 values) are uploaded at the first call after an assembly and kept until the next one.
int helm_eu_params(helm_op *op, EuParams *P, const cplx **xix, const cplx **xiz) {
    if (!op || !P || op->variant != HELM_EURUS || op->ny > 0 || !op->assembled || op->nPML < 2) return HELM_ERR_ARG;
    const cplx om = mz_damped_omega(op->a_freq_re, op->a_freq_im, op->a_tau);
    P->nz = op->nz; P->nx = op->nx; P->dx = op->dx; P->dz = op->dz; P->om = om; P->aniso = op->aniso ? 1 : 0; P->nblk_out = 1;
    if (!op->d_eu_xi) {
        std::vector<cplx> hx, hz;
        if (eu_profiles(op, om, op->a_cpml, hx, hz)) return HELM_ERR_PML;
        hx.insert(hx.end(), hz.begin(), hz.end());
        const size_t bytes = sizeof(cplx) * ((size_t)op->nx + op->nz + 4);
        cplx *d = (cplx *)helm_pool_alloc(op->device, bytes);
        if (!d) return HELM_ERR_DEVICE;
        if (helm_upload_staged(op, d, hx.data(), bytes)) { helm_pool_free(op->device, d, bytes); return HELM_ERR_DEVICE; }
        op->d_eu_xi = d;
    }
    *xix = op->d_eu_xi; *xiz = op->d_eu_xi + op->nx + 2;
    return HELM_OK;
}
void helm_eu_params_drop(helm_op *op) {
    if (op->d_eu_xi) { helm_pool_free(op->device, op->d_eu_xi, sizeof(cplx) * ((size_t)op->nx + op->nz + 4)); op->d_eu_xi = nullptr; }
}

int helm_launch_assemble(helm_op *op, double freq_re, double freq_im, double tau, double ky, double cPML) {
    const int nz = op->nz, nx = op->nx;
    const long long N = op->N;
    const cplx om = mz_damped_omega(freq_re, freq_im, tau);
    const int threads = 256;
    const int blocks = (int)((N + threads - 1) / threads);

    if (op->variant == HELM_MINIZEPHYR) {
        if (op->nPML < 2) HELM_FAIL(op, HELM_ERR_ARG, "nPML must be >= 2 (PML length dx*(nPML-1) is a divisor)");
        if (op->nPML > nx || op->nPML > nz) HELM_FAIL(op, HELM_ERR_ARG, "nPML larger than the grid (reference raises a broadcast ValueError)");
        std::vector<double> distx, sgnx, distz, sgnz;
        mz_profiles(nx, op->nPML, op->dx, op->fs[3], op->fs[1], distx, sgnx);
        mz_profiles(nz, op->nPML, op->dz, op->fs[0], op->fs[2], distz, sgnz);
        double *d_prof = nullptr;
        const size_t bytes = sizeof(double) * (2 * (size_t)nx + 2 * (size_t)nz);
        d_prof = (double *)helm_pool_alloc(op->device, bytes);          // (pool: hipMalloc / hipFree per assembly would wait for every stream of the device)
        if (!d_prof) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the PML profiles failed");
        std::vector<double> h(2 * (size_t)nx + 2 * (size_t)nz);
        std::copy(distx.begin(), distx.end(), h.begin());
        std::copy(sgnx.begin(), sgnx.end(), h.begin() + nx);
        std::copy(distz.begin(), distz.end(), h.begin() + 2 * nx);
        std::copy(sgnz.begin(), sgnz.end(), h.begin() + 2 * nx + nz);
        HIP_TRY(op, hipMemcpyAsync(d_prof, h.data(), bytes, hipMemcpyHostToDevice, op->stream));
        const MzParams P = mz_params_at(op, om, ky);
        HELM_LAUNCH(k_assemble_mz, dim3(blocks), dim3(threads), 0, op->stream, P, op->d_c, op->d_rho,
                           d_prof, d_prof + nx, d_prof + 2 * nx, d_prof + 2 * nx + nz, op->d_C);
        HIP_TRY(op, hipGetLastError());
        HIP_TRY(op, hipStreamSynchronize(op->stream));
        helm_pool_free(op->device, d_prof, bytes);
        op->block_zero[0] = false;
        if (op->transposed) { const int rct = helm_launch_transpose_planes(op); if (rct) return rct; }
    } else {
        if (op->nPML < 2) HELM_FAIL(op, HELM_ERR_ARG, "nPML must be >= 2");
        if (op->nPML > nx || op->nPML > nz) HELM_FAIL(op, HELM_ERR_ARG, "nPML larger than the grid");
        std::vector<cplx> xix, xiz;
        if (eu_profiles(op, om, cPML, xix, xiz))
            HELM_FAIL(op, HELM_ERR_PML, "np.arange(0, L+h, h) length != nPML for this dx/dz/nPML (reference raises ValueError, eurus.py:84-91)");
        cplx *d_xi = nullptr;
        const size_t bytes = sizeof(cplx) * ((size_t)nx + nz + 4);
        d_xi = (cplx *)helm_pool_alloc(op->device, bytes);
        if (!d_xi) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the PML profiles failed");
        std::vector<cplx> h(xix);
        h.insert(h.end(), xiz.begin(), xiz.end());
        HIP_TRY(op, hipMemcpyAsync(d_xi, h.data(), bytes, hipMemcpyHostToDevice, op->stream));
        EuParams P;
        P.nz = nz; P.nx = nx; P.dx = op->dx; P.dz = op->dz; P.om = om; P.aniso = op->aniso ? 1 : 0;
        P.nblk_out = op->block0_only ? 1 : (op->asm_nblk == 1 ? 1 : 4);
        HELM_LAUNCH(k_assemble_eurus, dim3(blocks), dim3(threads), 0, op->stream, P, op->d_c, op->d_rho,
                           op->d_theta, op->d_eps, op->d_delta, d_xi, d_xi + nx + 2, op->d_C);
        HIP_TRY(op, hipGetLastError());
        HIP_TRY(op, hipStreamSynchronize(op->stream));
        helm_pool_free(op->device, d_xi, bytes);
        op->blocks_ready = P.nblk_out;
        if (op->transposed) { const int rct = helm_launch_transpose_block0(op); if (rct) return rct; }
    }
    return HELM_OK;
}

// d_C <- the planes of its transpose (2-D, one block): into a pool buffer of the planes' own size class, which then takes d_C's place.  On op->stream, i.e.
// behind the assembly it follows (the low-priority set-up stream of helm_assemble included); returns when the planes are complete.
int helm_launch_transpose_planes(helm_op *op) {
    if (op->ny > 0 || op->nblocks != 1 || op->nplanes != 9) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the transposed operator exists for the 2-D single-block system only");
    const size_t bytes = (size_t)9 * (size_t)op->N * sizeof(cplx);
    cplx *d_T = (cplx *)helm_pool_alloc(op->device, bytes);
    if (!d_T) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the transposed coefficient planes failed");
    HELM_LAUNCH(k_transpose_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)op->d_C, d_T, op->nz, op->nx);
    const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(op->stream);
    if (e1 != hipSuccess || e2 != hipSuccess) { helm_pool_free(op->device, d_T, bytes); HIP_TRY(op, e1); HIP_TRY(op, e2); }
    helm_pool_free(op->device, op->d_C, bytes);       // (nothing reads the old planes any more: the stream is drained)
    op->d_C = d_T;
    return HELM_OK;
}

// Block 0 of an Eurus handle's d_C <- the planes of M1^T (helm_set_transposed_m1): the buffer of the four blocks keeps its size, so the transpose goes to a
// pool buffer of one block and is copied back.  On op->stream, behind the assembly it follows; returns when the planes are complete.
int helm_launch_transpose_block0(helm_op *op) {
    if (op->ny > 0 || op->variant != HELM_EURUS || op->nplanes != 9) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "the transposed M1 exists for 2-D Eurus handles only");
    const size_t bytes = (size_t)9 * (size_t)op->N * sizeof(cplx);
    cplx *d_T = (cplx *)helm_pool_alloc(op->device, bytes);
    if (!d_T) HELM_FAIL(op, HELM_ERR_DEVICE, "hipMalloc of the transposed coefficient planes failed");
    HELM_LAUNCH(k_transpose_planes, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)op->d_C, d_T, op->nz, op->nx);
    const hipError_t e1 = hipGetLastError();
    const hipError_t e2 = hipMemcpyAsync(op->d_C, d_T, bytes, hipMemcpyDeviceToDevice, op->stream);
    const hipError_t e3 = hipStreamSynchronize(op->stream);
    helm_pool_free(op->device, d_T, bytes);
    HIP_TRY(op, e1); HIP_TRY(op, e2); HIP_TRY(op, e3);
    return HELM_OK;
}

int helm_launch_scale_planes(helm_op *op) {
    const int blocks = (int)((op->N + 255) / 256);
    HELM_LAUNCH(k_scale_planes, dim3(blocks), dim3(256), 0, op->stream, op->d_C, op->d_Cs, op->d_dinv, op->N, op->nblocks, op->diag_floor, op->nplanes, op->centre);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int helm_launch_rowscaled_system(helm_op *op) {
    if (!op->d_S) HIP_TRY(op, hipMalloc(&op->d_S, (size_t)36 * op->N * sizeof(cplx)));
    if (!op->d_rs) HIP_TRY(op, hipMalloc(&op->d_rs, (size_t)2 * op->N * sizeof(double)));
    HELM_LAUNCH(k_rowscale_system, dim3((unsigned)((op->N + 255) / 256)), dim3(256), 0, op->stream, (const cplx *)op->d_C, op->d_S, op->d_rs, op->N);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int helm_launch_gardner_rho(helm_op *op) {
    HELM_LAUNCH(k_gardner_rho, dim3(vec_blocks(op->N)), dim3(256), 0, op->stream, (const cplx *)op->d_c, op->d_rho, op->N);
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}
