// What the translation units of the 3-D buoyancy derivative share (survey3d_density.hip: the derivative maps; survey3d_hessian.hip: the pseudo-Hessian built on
// them): the tile and the walk of k_stencil3, the stretch tables of a launch at a row and at the neighbours' rows, the 27-point sum in its fixed order
// (survey3d_density.hip says how it is formed), kappa of a cell, and what every entry point asks of its handle.  Each translation unit gets its own copy
// (an anonymous namespace), inlined where it is used.
#pragma once
#include "survey_internal.hpp"

namespace {

constexpr int D3X = 64, D3Y = 4;                       // the tile of k_stencil3
constexpr int D3LW = D3X + 2, D3LH = D3Y + 2;
constexpr int D3PLANE = D3LW * D3LH;                   // 396 elements of one staged plane
constexpr int D3NEL = 3 * D3PLANE;
constexpr int D3NLOAD = (D3NEL + 255) / 256;           // elements staged per thread
constexpr double D3M0 = 2.0 / 3.0, D3M1 = 1.0 / 6.0;

struct Tile3d {
    int iz, x0, y0;
    __device__ __forceinline__ Tile3d(int nz, int ntx) {
        const int t = blockIdx.x;
        iz = t % nz; x0 = ((t / nz) % ntx) * D3X; y0 = (t / (nz * ntx)) * D3Y;
    }
};
// element e of the staged tile -> its global cell, -1 where that lies outside the grid; bnd: the cell is on the box boundary (or outside)
__device__ __forceinline__ long long tile3d_cell(const Tile3d &T, int e, int nz, int ny, int nx, bool &bnd) {
    const int p = e / D3PLANE, rem = e - p * D3PLANE, r = rem / D3LW, cc = rem - r * D3LW;
    const int gz = T.iz - 1 + p, gy = T.y0 - 1 + r, gx = T.x0 - 1 + cc;
    bnd = gz <= 0 || gz >= nz - 1 || gy <= 0 || gy >= ny - 1 || gx <= 0 || gx >= nx - 1;
    if (gz < 0 || gz >= nz || gy < 0 || gy >= ny || gx < 0 || gx >= nx) return -1;
    return ((long long)gz * ny + gy) * nx + gx;
}

// the geometry and the stretch tables of a launch: Lx(-1)[nx], Lx(0)[nx], Lx(+1)[nx] (and Ly, Lz alike), as k_assemble_3d reads them
struct Lap3Params {
    const cplx *Lx, *Ly, *Lz;
    double idx2, idy2, idz2;
    int nz, ny, nx, ntx;
};
struct Lap3Tab { cplx x[3], y[3], z[3]; };

__device__ __forceinline__ cplx d3_wsum(cplx a, cplx b, cplx c) {            // m0 b + m1 (a + c)
    return cmake(D3M0 * b.x + D3M1 * (a.x + c.x), D3M0 * b.y + D3M1 * (a.y + c.y));
}
__device__ __forceinline__ cplx d3_dot(const cplx *l, cplx a, cplx b, cplx c) {   // l[0] a + l[1] b + l[2] c
    cplx s = cmul(l[0], a);
    cfma(s, l[1], b);
    cfma(s, l[2], c);
    return s;
}
// sum_o lap_o t(o) with the tables of `tab` (tab.x[cc] multiplies the neighbour at x offset cc - 1, ...); get(p, r, cc) is the value at offset (p - 1, r - 1, cc - 1)
template <class GET>
__device__ __forceinline__ cplx lap3_sum(const Lap3Tab &tab, double idx2, double idy2, double idz2, GET get) {
    cplx px[3], py[3], pm[3];
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        cplx ax[3], am[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const cplx t0 = get(p, r, 0), t1 = get(p, r, 1), t2 = get(p, r, 2);
            ax[r] = d3_dot(tab.x, t0, t1, t2);
            am[r] = d3_wsum(t0, t1, t2);
        }
        px[p] = d3_wsum(ax[0], ax[1], ax[2]);
        py[p] = d3_dot(tab.y, am[0], am[1], am[2]);
        pm[p] = d3_wsum(am[0], am[1], am[2]);
    }
    const cplx sx = d3_wsum(px[0], px[1], px[2]), sy = d3_wsum(py[0], py[1], py[2]), sz = d3_dot(tab.z, pm[0], pm[1], pm[2]);
    return cmake((idx2 * sx.x + idy2 * sy.x) + idz2 * sz.x, (idx2 * sx.y + idy2 * sy.y) + idz2 * sz.y);
}
// the tables of L at the thread's own row (col, row, iz); zeros for a thread outside the grid
__device__ __forceinline__ Lap3Tab lap3_row_tables(const Lap3Params &q, bool ok, int col, int row, int iz) {
    Lap3Tab t;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        t.x[o] = ok ? q.Lx[(long long)o * q.nx + col] : cmake(0.0, 0.0);
        t.y[o] = ok ? q.Ly[(long long)o * q.ny + row] : cmake(0.0, 0.0);
        t.z[o] = ok ? q.Lz[(long long)o * q.nz + iz] : cmake(0.0, 0.0);
    }
    return t;
}
// the tables of L^T at the thread's cell j: what multiplies the neighbour j + o' is lap_{-o'}(j + o'), the factor L[-o'] of the NEIGHBOUR's row; zero where the
// neighbour lies outside the grid (nothing is read past a table's end)
__device__ __forceinline__ Lap3Tab lap3_transposed_tables(const Lap3Params &q, bool ok, int col, int row, int iz) {
    Lap3Tab t;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
        const int gx = col + o - 1, gy = row + o - 1, gz = iz + o - 1;
        t.x[o] = ok && gx >= 0 && gx < q.nx ? q.Lx[(long long)(2 - o) * q.nx + gx] : cmake(0.0, 0.0);
        t.y[o] = ok && gy >= 0 && gy < q.ny ? q.Ly[(long long)(2 - o) * q.ny + gy] : cmake(0.0, 0.0);
        t.z[o] = ok && gz >= 0 && gz < q.nz ? q.Lz[(long long)(2 - o) * q.nz + gz] : cmake(0.0, 0.0);
    }
    return t;
}

// kappa = om~^2 / c^2 of one cell: the expression of kfield3 (helm3d.hip) at rho = 1 (the products with 1.0 are exact), contraction pinned as there
__device__ __forceinline__ cplx kappa3s(cplx om2, cplx cj) {
#pragma clang fp contract(off)
    const double br = (cj.x * cj.x - cj.y * cj.y) * 1.0, bi = (cj.x * cj.y + cj.y * cj.x) * 1.0;
    if (fabs(br) >= fabs(bi)) {
        const double r = bi / br, d = br + bi * r;
        return cmake((om2.x + om2.y * r) / d, (om2.y - om2.x * r) / d);
    }
    const double r = br / bi, d = br * r + bi;
    return cmake((om2.x * r + om2.y) / d, (om2.y * r - om2.x) / d);
}

// om~ = 2 pi f - i / tau of the handle's last assembly
inline cplx damped_omega3(const helm_op *op) {
    cplx om = cmake(2.0 * M_PI * op->a_freq_re, 2.0 * M_PI * op->a_freq_im);
    if (std::isfinite(op->a_tau) && op->a_tau != 0.0) om.y -= 1.0 / op->a_tau;
    return om;
}

inline int buoy3_handle_args(helm_op *op, const char *what) {
    if (op->variant != HELM_3D || op->ny <= 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "%s: the buoyancy derivative here is that of the 3-D 27-point operator (a helm_create3d handle)", what);
    if (!op->assembled) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle is not assembled (the stretch tables and kappa are those of its last assembly)", what);
    return HELM_OK;
}
inline int lap3_params(helm_op *op, const char *what, Lap3Params *q, int *nblk) {
    const size_t want = 3 * ((size_t)op->nx + (size_t)op->ny + (size_t)op->nz);
    if (!op->d_L3 || op->l3_elems != want) HELM_FAIL(op, HELM_ERR_STATE, "%s: the handle holds no stretch tables (they are uploaded by helm_assemble)", what);
    q->Lx = op->d_L3; q->Ly = op->d_L3 + 3 * (size_t)op->nx; q->Lz = op->d_L3 + 3 * (size_t)op->nx + 3 * (size_t)op->ny;
    const bool over = op->lap_override.size() == want;        // (a multigrid level on a stretched grid: 1 / h^2 is inside its tables)
    q->idx2 = over ? 1.0 : 1.0 / (op->dx * op->dx); q->idy2 = over ? 1.0 : 1.0 / (op->dy * op->dy); q->idz2 = over ? 1.0 : 1.0 / (op->dz * op->dz);
    q->nz = op->nz; q->ny = op->ny; q->nx = op->nx;
    q->ntx = (op->nx + D3X - 1) / D3X;
    *nblk = q->ntx * ((op->ny + D3Y - 1) / D3Y) * op->nz;
    return HELM_OK;
}

}  // namespace
