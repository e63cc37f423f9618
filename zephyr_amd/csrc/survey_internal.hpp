// What the translation units of a survey share: survey.hip (the plumbing: right-hand sides, axpby, the complex64 pack, imaging, energy, sampling),
// survey_frechet.hip (the derivative kernels of the 2-D MiniZephyr operator), survey_hessian.hip (the two Hessian diagonals built on them) and survey_newton.hip
// (the second derivative and the transposed planes of the Newton Hessian-vector product), survey_joint.hip (the transposes of the mixed (c, b) derivative) and
// survey_visco.hip (the chain from (c, Q) to the complex velocity of a visco problem).  The readers
// of a stored field on the device (FieldC128 / FieldC64) and its description on the host (HostField), how an entry point ends and refuses, the walk of the
// stencil kernels over the grid, and the row factors of MiniZephyr at a cell.
//
// The complex64 store (zephyr_amd/fieldstore.py, config key fieldsDtype='complex64'): a wavefield column s is kept as
// complex64 values x * 2^-e_s with ONE power-of-two scale per column, e_s the binary exponent of the column's largest component
// (2^e_s <= max_i max(|Re|, |Im|) < 2^(e_s+1), clamped to +-1021; 0 for a zero column).  The scaling is exact, so the only rounding is the conversion to
// fp32 (2^-24 relative where the scaled value is a normal fp32 number), and fields of any magnitude survive where a plain conversion would overflow or
// flush.  A consumer reads (double)x^ * 2^e_s, exact again.  The loops over a stored field exist once, as templates over the reader of the
// forward field (FieldC128 / FieldC64 below): the complex64 entry points give the complex128 sum of the unpacked field term for term because it is the
// same loop.
#pragma once
#include "helm_internal.hpp"
#include "mz_row.hpp"
#include <algorithm>
#include <utility>

// what every entry point here ends on: the launch error, then the stream drained (the result is complete when the call returns)
static inline int launched(helm_op *op) {
    HIP_TRY(op, hipGetLastError());
    HIP_TRY(op, hipStreamSynchronize(op->stream));
    return HELM_OK;
}
static inline bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + nb && pb < pa + na;
}
static inline int mz_handle_args(helm_op *op, const char *what) {
    if (op->variant != HELM_MINIZEPHYR || op->ny > 0) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "%s: the density and velocity derivatives are those of the 2-D MiniZephyr operator", what);
    return HELM_OK;
}
// the two loops over stored columns that read nothing but nine planes and the grid (k_stencil_sources, k_lag_imaging) serve a 2-D Eurus handle too once it has
// opted in (helm_set_eurus_derivatives); without that every handle is refused as it always was
static inline int planes_handle_args(helm_op *op, const char *what) {
    if (op->variant == HELM_EURUS && op->ny == 0 && op->eu_derivatives) return HELM_OK;
    return mz_handle_args(op, what);
}

// ------------------------------------------------------------------------------------------
// the loops over a forward field, one body for both formats of the store
// ------------------------------------------------------------------------------------------
typedef float2 cplxf32;      // what the store holds: 8 bytes per value
__device__ __forceinline__ double pow2(int e) { return __longlong_as_double((long long)(e + 1023) << 52); }      // |e| <= 1021: a normal number

// How a kernel reads the field, passed by value: load(i) is the raw 16- or 8-byte load of element i, value(x, s) what a loaded element of column s stands
// for.  The two are separate so that a kernel can issue several loads before the first use.
struct FieldC128 {
    typedef cplx raw;
    const cplx *__restrict__ u;
    __device__ __forceinline__ raw load(long long i) const { return u[i]; }
    __device__ __forceinline__ cplx value(raw x, int) const { return x; }
    // value() in two steps, for a loop that reads one column many times: scale(s) once, scaled(x, scale) per element
    __device__ __forceinline__ double scale(int) const { return 1.0; }
    __device__ __forceinline__ cplx scaled(raw x, double) const { return x; }
};
struct FieldC64 {
    typedef cplxf32 raw;
    const cplxf32 *__restrict__ u;
    const int *__restrict__ exps;
    __device__ __forceinline__ raw load(long long i) const { return u[i]; }
    // each component is scaled in fp64 (exact: 2^(2 e_s) alone would overflow where the field does not)
    __device__ __forceinline__ cplx value(raw x, int s) const { const double sc = pow2(exps[s]); return cmake((double)x.x * sc, (double)x.y * sc); }
    __device__ __forceinline__ double scale(int s) const { return pow2(exps[s]); }
    __device__ __forceinline__ cplx scaled(raw x, double sc) const { return cmake((double)x.x * sc, (double)x.y * sc); }
};

// The same field as an entry point receives it: the values, the exponents of the columns (complex64 alone) and which format that is.  Each pair of entry
// points, helm_X_device and helm_X_c64_device, is one launcher that takes this: the checks, the grid and the launch are written once.
struct HostField {
    const void *u, *exps;
    bool c64;
    static HostField c128(const void *u) { return {u, nullptr, false}; }
    static HostField packed(const void *u32, const void *exps) { return {u32, exps, true}; }
    bool present() const { return u && (exps || !c64); }
    // complex128 values are loaded as 16-byte vectors, complex64 values as 8-byte ones, exponents as ints
    bool ok() const { return present() && !(c64 ? (((uintptr_t)u) & 7) || (((uintptr_t)exps) & 3) : ((uintptr_t)u) & 15); }
    size_t bytes(int nsrc, long long ld) const { return (size_t)nsrc * ld * (c64 ? sizeof(cplxf32) : sizeof(cplx)); }
    // fn(FieldC128{...}) or fn(FieldC64{...}): fn is a generic lambda that launches the kernel of the reader it is given
    template <class FN>
    int with(FN &&fn) const { return c64 ? fn(FieldC64{(const cplxf32 *)u, (const int *)exps}) : fn(FieldC128{(const cplx *)u}); }
};

// ------------------------------------------------------------------------------------------
// the walk of the stencil kernels (survey_frechet.hip states it in full)
// ------------------------------------------------------------------------------------------
constexpr int OP_TILE_X = 62;       // output cells per wave along x
constexpr int OP_ROWS = 32;         // output rows per wave
constexpr int OP_UNROLL = 4;        // columns walked together

struct MassRow { cplx t, h; };

// t(x - 1) + t(x + 1) from the neighbouring lanes.  Lane 0 and lane 63 get their own value for the missing neighbour: they are halo lanes, whose h is never used.
__device__ __forceinline__ cplx lane_neighbours(cplx t) {
    const double lx = __shfl_up(t.x, 1, 64), ly = __shfl_up(t.y, 1, 64), rx = __shfl_down(t.x, 1, 64), ry = __shfl_down(t.y, 1, 64);
    return cmake(lx + rx, ly + ry);
}

// where a wave works: its tile and rows from the flat job index (x tiles fastest), its lane's cell
struct OpJob {
    int x, z0, z1; bool live, xin, store;
    __device__ __forceinline__ OpJob(int nz, int nx) {
        const int lane = threadIdx.x & 63;
        const int ntx = (nx + OP_TILE_X - 1) / OP_TILE_X, nzc = (nz + OP_ROWS - 1) / OP_ROWS;
        const long long job = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
        live = job < (long long)ntx * nzc;
        const int tile = live ? (int)(job % ntx) : 0, chunk = live ? (int)(job / ntx) : 0;
        x = tile * OP_TILE_X + lane - 1;
        z0 = chunk * OP_ROWS;
        z1 = min(z0 + OP_ROWS, nz);
        xin = x >= 0 && x < nx;
        store = lane >= 1 && lane <= OP_TILE_X && x < nx;
    }
};
static inline dim3 op_grid(const helm_op *op, int groups) {
    const long long jobs = (long long)((op->nx + OP_TILE_X - 1) / OP_TILE_X) * ((op->nz + OP_ROWS - 1) / OP_ROWS);
    return dim3((unsigned)((jobs + 3) / 4), (unsigned)groups);
}

// the left and right neighbours kept apart, for the stencils whose coefficients differ between them
struct LagRow { cplx t, l, r; };
__device__ __forceinline__ void lane_left_right(cplx t, cplx &l, cplx &r) {
    l = cmake(__shfl_up(t.x, 1, 64), __shfl_up(t.y, 1, 64));          // (lane 0 and lane 63 are halo lanes: their l / r are never used)
    r = cmake(__shfl_down(t.x, 1, 64), __shfl_down(t.y, 1, 64));
}

// ------------------------------------------------------------------------------------------
// the row factors of MiniZephyr at a cell, their derivative along c, and the stiffness factors of a row
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ MzRow mz_row_at(const MzParams &P, const cplx *__restrict__ c, int iz, int ix) {
    double dX, sX, dZ, sZ;
    mz_profile_at(P.nx, P.npml, P.dx, P.fs3, P.fs1, ix, dX, sX);
    mz_profile_at(P.nz, P.npml, P.dz, P.fs0, P.fs2, iz, dZ, sZ);
    return mz_row_factors(P, c[(long long)iz * P.nx + ix], dX, sX, dZ, sZ);
}
__device__ __forceinline__ MzRow mz_row_dc_at(const MzParams &P, const cplx *__restrict__ c, int iz, int ix) {
    double dX, sX, dZ, sZ;
    mz_profile_at(P.nx, P.npml, P.dx, P.fs3, P.fs1, ix, dX, sX);
    mz_profile_at(P.nz, P.npml, P.dz, P.fs0, P.fs2, iz, dZ, sZ);
    return mz_row_factors_dc(P, c[(long long)iz * P.nx + ix], dX, sX, dZ, sZ);
}

// the same for the derivative of order ORDER (1 or 2) of the factors along c
template <int ORDER>
__device__ __forceinline__ MzRow mz_row_dnc_at(const MzParams &P, const cplx *__restrict__ c, int iz, int ix) {
    double dX, sX, dZ, sZ;
    mz_profile_at(P.nx, P.npml, P.dx, P.fs3, P.fs1, ix, dX, sX);
    mz_profile_at(P.nz, P.npml, P.dz, P.fs0, P.fs2, iz, dZ, sZ);
    const cplx c0 = c[(long long)iz * P.nx + ix];
    return ORDER == 1 ? mz_row_factors_dc(P, c0, dX, sX, dZ, sZ) : mz_row_factors_d2c(P, c0, dX, sX, dZ, sZ);
}

// T of a row (mz_star: corners tc, verticals tv, horizontals th, the cross term tzx): what multiplies the averaged buoyancies.  survey_frechet.hip
// (k_buoyancy_adjoint) says how the transposes use it.
struct MzStiff { cplx tv[2], th[2], tc[2][2], tzx; };
template <bool CONJ>
__device__ __forceinline__ MzStiff mz_stiffness(const MzParams &P, MzRow row) {
    if (CONJ) { row.X = cconj(row.X); row.Z = cconj(row.Z); row.px = cconj(row.px); row.pz = cconj(row.pz); }
    const double dxx = P.dx * P.dx, dzz = P.dz * P.dz, dxz = (dxx + dzz) / 2.0, dd = sqrt(dxz);
    MzStiff t;
    const cplx ZpX = cscale(cadd(row.Z, row.X), 1.0 / (4 * dxz));
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const double sg = a ? 1.0 : -1.0;
        t.tv[a] = cscale(cadd(cscale(row.Z, 1.0 / P.dz), cscale(row.pz, sg / 2.0)), MZ_WA / P.dz);
        t.th[a] = cscale(cadd(cscale(row.X, 1.0 / P.dx), cscale(row.px, sg / 2.0)), MZ_WA / P.dx);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const double sx = b ? 1.0 : -1.0;
            t.tc[a][b] = cscale(cadd(ZpX, cscale(cadd(cscale(row.pz, sg), cscale(row.px, sx)), 1.0 / (4 * dd))), MZ_WB);
        }
    }
    t.tzx = cscale(csub(row.Z, row.X), MZ_WB / (4 * dxz));
    return t;
}
// Q_o of row i for the lag o = (sz, sx) != (0, 0)
__device__ __forceinline__ cplx lag_coefficient(const MzStiff &t, const cplx *__restrict__ Pl, long long N, long long i, int sz, int sx) {
    const cplx d = csub(Pl[(long long)mz_slot(sz, sx) * N + i], Pl[4 * N + i]);
    if (sz == 0) return cmul(t.th[(sx + 1) / 2], d);
    if (sx == 0) return cmul(t.tv[(sz + 1) / 2], d);
    cplx q = cmul(t.tc[(sz + 1) / 2][(sx + 1) / 2], d);
    cfma(q, t.tzx, csub(Pl[(long long)mz_slot(sz, 0) * N + i], Pl[(long long)mz_slot(0, sx) * N + i]));
    return q;
}

// sum_(k, i) (d^ORDER A / dc_j^ORDER)_((k, i)) P_k[i] at cell j (CONJ: the conjugated coefficients; STRETCH false: the mass term alone): the body that the
// transposes of the first and of the second derivative share (survey_frechet.hip k_velocity_adjoint; survey_newton.hip k_velocity_curvature).  The mass part is the
// gather of k_buoyancy_adjoint over the interior rows i = j - o, times (d^ORDER kappa_j / dc^ORDER) b_j.  The stretch part is local to row j: its differentiated
// stiffness factors (mz_stiffness is linear in the row) times the averaged buoyancies a_o = (b_j + b_(j+o)) / 2 and the Q-differences of P at j (lag_coefficient); a
// boundary row has none.  A fixed order; the boundary rows of P are not read.  BARRAY: `rho` is not a density but the field that stands in the place of the
// buoyancy, read as it is -- any sign, zeros included (survey_joint.hip k_velocity_adjoint_b, the transpose of the mixed derivative d^2 A / dc db in c).
template <int ORDER, bool CONJ, bool STRETCH, bool BARRAY = false>
__device__ __forceinline__ cplx mz_transpose_at(const MzParams &P, const cplx *__restrict__ c, const double *__restrict__ rho, const cplx *__restrict__ Pl, long long j) {
    const long long N = (long long)P.nz * P.nx;
    const int jz = (int)(j / P.nx), jx = (int)(j % P.nx);
    const double bj = BARRAY ? rho[j] : 1.0 / rho[j];
    cplx mass = cmake(0.0, 0.0), stretch = cmake(0.0, 0.0);
#pragma unroll
    for (int sz = -1; sz <= 1; ++sz)
#pragma unroll
        for (int sx = -1; sx <= 1; ++sx) {
            const int iz = jz - sz, ix = jx - sx;                 // row i sees cell j at the lag (sz, sx)
            if (iz < 1 || iz > P.nz - 2 || ix < 1 || ix > P.nx - 2) continue;
            const double m = (sz == 0 && sx == 0) ? MZ_WC : ((sz == 0 || sx == 0) ? MZ_WD : MZ_WE);
            const cplx p = Pl[(long long)mz_slot(sz, sx) * N + (long long)iz * P.nx + ix];
            mass.x += m * p.x; mass.y += m * p.y;
        }
    if (STRETCH && jz >= 1 && jz <= P.nz - 2 && jx >= 1 && jx <= P.nx - 2) {
        const MzStiff dt = mz_stiffness<CONJ>(P, mz_row_dnc_at<ORDER>(P, c, jz, jx));
#pragma unroll
        for (int oz = -1; oz <= 1; ++oz)
#pragma unroll
            for (int ox = -1; ox <= 1; ++ox)
                if (oz != 0 || ox != 0) {
                    const double bo = rho[j + (long long)oz * P.nx + ox];
                    const double a = (bj + (BARRAY ? bo : 1.0 / bo)) / 2.0;
                    stretch = cadd(stretch, cscale(lag_coefficient(dt, Pl, N, j, oz, ox), a));
                }
    }
    cplx dk = cscale(ORDER == 1 ? mz_kappa_dc(P, c[j]) : mz_kappa_d2c(P, c[j]), bj);
    if (CONJ) dk = cconj(dk);
    cplx sum = stretch;
    cfma(sum, dk, mass);
    return sum;
}
