// The batched 9-point stencil apply of the matrix-free Krylov path and of the 2-D multigrid cycle:
//   * k_stencil_t -- complex128 (complex64 on multigrid levels), LDS-staged tiles, coefficients
//                    register-blocked over the right-hand-side loop, fused dot-product epilogues
//                    (wave64 shuffle reduction -> LDS -> one partial per workgroup; the reductions are in helm_internal.hpp)
//   * helm_launch_apply -- its launcher, which also routes 3-D operators to helm3d.hip
//
// The arithmetic replaces the sparse-LU solve behind BaseDiscretization.__mul__
// (zephyr/backend/discretization.py:78-106).  This is HBM-bound work (<= 2.25 flop/B, no MFMA):
// the design rules are 16-B-per-lane coalesced accesses, one pass per vector per kernel, and
// an XCD-aware tile order so that halo rows are served by the XCD's own L2.
#include "helm_internal.hpp"
#include <type_traits>

namespace {

// Round-robin dispatch puts workgroup b on XCD b % 8; give every XCD one contiguous run of
// tiles (a band of grid rows) so z-/x-neighbouring tiles share an L2.  Bijective for any count.
__device__ inline int xcd_swizzle(int bid, int nblk) {
    const int q = nblk / HELM_NXCD, rem = nblk % HELM_NXCD;
    const int x = bid % HELM_NXCD, k = bid / HELM_NXCD;
    const int start = x * q + (x < rem ? x : rem);
    return start + k;
}

// ------------------------------------------------------------------------------------------
// stencil apply
// ------------------------------------------------------------------------------------------
template <class V>
struct StencilParamsT {
    const V *planes;
    const V *X;
    V *Y;
    const V *W;
    long long ld, N;
    int nz, nx, nrhs, ntx, ntz, nblk;
    const RhsScal *scal;
    double *part;
    const V *dinv;
    double omega_j;
    const int *tiles;
    int planes_tiled;     // 1: planes are stored tile-blocked, [tile][k][row in tile][64] (one contiguous 9*TZ KB chunk per tile)
    // fused multigrid stages (XMODE template parameter)
    int acc, part_stride, part_off;
    V *U;                 // XMODE 1: the smoothed iterate u = omega_j dinv (.) W is also written here
    const V *E;           // XMODE 2: coarse-grid correction, [nrhs][nzc*nxc]; the input is X + P E (bilinear)
    int nzc, nxc;
};
typedef StencilParamsT<cplx> StencilParams;

constexpr int TX = 64;

// XMODE selects how the input tile is produced:
//   0  X is read                                                       (everything else)
//   1  X = omega_j * dinv (.) W, also stored to U        [multigrid: first Jacobi sweep fused into the residual]
//   2  X = X + P E (bilinear prolongation of E)          [multigrid: coarse correction fused into the post-smoothing sweep]
template <class V, int P, bool SCALED, bool ADJ, int EPI, int XMODE = 0>
__global__ __launch_bounds__(256) void k_stencil_t(StencilParamsT<V> q) {
    constexpr int TZ = 4 * P;
    constexpr int LW = TX + 2;             // tile row length in elements
    constexpr int LR = TZ + 2;             // tile rows
    constexpr int NLOAD = (LR + 3) / 4;    // main-column row loads per wave
    __shared__ __attribute__((aligned(16))) V tile[2][LR * LW];
    __shared__ double red[16];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int t = xcd_swizzle(blockIdx.x, q.nblk);
    if (q.tiles) t = q.tiles[t];
    const int tz = t / q.ntx, tx = t - tz * q.ntx;
    const int z0 = tz * TZ, x0 = tx * TX;
    const int nz = q.nz, nx = q.nx;
    const long long N = q.N;
    const int col = x0 + lane;
    const bool colok = col < nx;

    // ---- coefficients for this thread's P points, kept in registers over the RHS loop ----
    V cf[P][9];
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int row = z0 + wave * P + j;
        const bool ok = colok && row < nz;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (SCALED && k == 4) { cf[j][k] = vone<V>(); continue; }
            V v = vzero<V>();
            if (!ADJ) {
                if (q.planes_tiled) v = q.planes[((long long)t * 9 + k) * (TZ * TX) + (wave * P + j) * TX + lane];
                else if (ok) v = q.planes[(long long)k * N + (long long)row * nx + col];
            } else {
                // (A^H x)[i] = sum over neighbours n of conj(A[n,i]) x[n]; the entry A[n,i] sits in
                // plane slot(-dz,-dx) at point n = i + (dz,dx)
                const int dz = k / 3 - 1, dx = k % 3 - 1;
                const int rn = row + dz, cn = col + dx;
                if (ok && rn >= 0 && rn < nz && cn >= 0 && cn < nx)
                    v = cconj(q.planes[(long long)(8 - k) * N + (long long)rn * nx + cn]);
            }
            cf[j][k] = v;
        }
    }

    // ---- RHS loop with register prefetch + double-buffered LDS tile ----
    V pre[NLOAD];
    V prehalo = vzero<V>();
    // value of the (virtual) input vector at grid point (grow, gcol) of right-hand side b
    auto input_at = [&](int b, int grow, int gcol) -> V {
        const long long idx = (long long)grow * nx + gcol;
        if (XMODE == 1) {
            return cmul(cscale(q.dinv[idx], q.omega_j), q.W[(long long)b * q.ld + idx]);
        } else if (XMODE == 2) {
            V v = q.X[(long long)b * q.ld + idx];
            const V *e = q.E + (long long)b * q.nzc * q.nxc;
            const int I = grow >> 1, J = gcol >> 1;
            const bool oi = grow & 1, oj = gcol & 1;
            const double wi0 = oi ? 0.5 : 1.0, wj0 = oj ? 0.5 : 1.0;
            V a = cscale(e[(long long)I * q.nxc + J], wi0 * wj0);
            if (oj && J + 1 < q.nxc) { const V c1 = e[(long long)I * q.nxc + J + 1]; a.x += wi0 * 0.5 * c1.x; a.y += wi0 * 0.5 * c1.y; }
            if (oi && I + 1 < q.nzc) {
                const V c2 = e[(long long)(I + 1) * q.nxc + J]; a.x += 0.5 * wj0 * c2.x; a.y += 0.5 * wj0 * c2.y;
                if (oj && J + 1 < q.nxc) { const V c3 = e[(long long)(I + 1) * q.nxc + J + 1]; a.x += 0.25 * c3.x; a.y += 0.25 * c3.y; }
            }
            return cadd(v, a);
        } else {
            return q.X[(long long)b * q.ld + idx];
        }
    };
    auto prefetch = [&](int b) {
#pragma unroll
        for (int l = 0; l < NLOAD; ++l) {
            const int r = wave + 4 * l;                 // tile row
            const int grow = z0 - 1 + r;
            V v = vzero<V>();
            if (r < LR && colok && grow >= 0 && grow < nz) v = input_at(b, grow, col);
            pre[l] = v;
        }
        prehalo = vzero<V>();
        if (tid < 2 * LR) {
            const int r = tid >> 1, side = tid & 1;
            const int grow = z0 - 1 + r, gcol = side ? x0 + TX : x0 - 1;
            if (grow >= 0 && grow < nz && gcol >= 0 && gcol < nx) prehalo = input_at(b, grow, gcol);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int l = 0; l < NLOAD; ++l) {
            const int r = wave + 4 * l;
            if (r < LR) tile[buf][r * LW + 1 + lane] = pre[l];
        }
        if (tid < 2 * LR) {
            const int r = tid >> 1, side = tid & 1;
            tile[buf][r * LW + (side ? TX + 1 : 0)] = prehalo;
        }
    };

    const int bstep = gridDim.y;
    int b = blockIdx.y;
    while (b < q.nrhs && !rhs_active(q.scal, b)) b += bstep;
    if (b < q.nrhs) prefetch(b);
    int buf = 0;
    while (b < q.nrhs) {
        stage(buf);
        int bn = b + bstep;
        while (bn < q.nrhs && !rhs_active(q.scal, bn)) bn += bstep;
        if (bn < q.nrhs) prefetch(bn);
        __syncthreads();

        V acc[P];
#pragma unroll
        for (int j = 0; j < P; ++j) acc[j] = vzero<V>();
        V xc_keep[P];
        const V *trow = &tile[buf][(wave * P) * LW + lane];
#pragma unroll
        for (int rr = 0; rr < P + 2; ++rr) {
            const V xl = trow[rr * LW + 0], xm = trow[rr * LW + 1], xr = trow[rr * LW + 2];
#pragma unroll
            for (int j = 0; j < P; ++j) {
                const int dzi = rr - j;            // 0,1,2 <-> dz = -1,0,+1
                if (dzi < 0 || dzi > 2) continue;
                cfma(acc[j], cf[j][dzi * 3 + 0], xl);
                if (SCALED && dzi == 1) { acc[j].x += xm.x; acc[j].y += xm.y; }
                else cfma(acc[j], cf[j][dzi * 3 + 1], xm);
                cfma(acc[j], cf[j][dzi * 3 + 2], xr);
                if (dzi == 1) xc_keep[j] = xm;
            }
        }

        double dsum[4] = {0.0, 0.0, 0.0, 0.0};
        V *Yb = q.Y + (long long)b * q.ld;
        const V *Wb = (EPI == EPI_DOT_W || EPI == EPI_RESID || EPI == EPI_JACOBI || EPI == EPI_DOT_WY) ? q.W + (long long)b * q.ld : nullptr;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const int row = z0 + wave * P + j;
            if (colok && row < nz) {
                const long long idx = (long long)row * nx + col;
                V y = acc[j];
                if (q.acc) y = cadd(y, Yb[idx]);
                if (EPI == EPI_RESID) {
                    const V w = Wb[idx];
                    y = csub(w, y);
                    dsum[0] += cabs2(y);
                    if (XMODE == 1) q.U[(long long)b * q.ld + idx] = xc_keep[j];
                } else if (EPI == EPI_DOT_W) {
                    const V w = Wb[idx];          // (w, y) = sum conj(w) y
                    dsum[0] += w.x * y.x + w.y * y.y;
                    dsum[1] += w.x * y.y - w.y * y.x;
                } else if (EPI == EPI_DOT_XY) {
                    const V x = xc_keep[j];       // (y, x) = sum conj(y) x ; (y, y)
                    dsum[0] += y.x * x.x + y.y * x.y;
                    dsum[1] += y.x * x.y - y.y * x.x;
                    dsum[2] += cabs2(y);
                } else if (EPI == EPI_DOT_YY) {
                    dsum[0] += cabs2(y);
                } else if (EPI == EPI_DOT_WY) {
                    const V w = Wb[idx];          // (y, w) = sum conj(y) w ; (y, y)
                    dsum[0] += y.x * w.x + y.y * w.y;
                    dsum[1] += y.x * w.y - y.y * w.x;
                    dsum[2] += cabs2(y);
                } else if (EPI == EPI_JACOBI) {
                    const V res = csub(Wb[idx], y);
                    const V d = q.dinv[idx];
                    y = xc_keep[j];
                    cfma(y, cscale(d, q.omega_j), res);
                }
                Yb[idx] = y;
            }
        }
        if (EPI != EPI_NONE && EPI != EPI_JACOBI && sizeof(V) == sizeof(cplx)) {   // single-precision (multigrid) launches need no partials
            block_sum<4>(dsum, red);
            if (tid == 0) {
                double *pp = q.part + ((long long)b * 4) * q.part_stride + q.part_off + blockIdx.x;
                pp[0] = dsum[0];
                pp[(long long)q.part_stride] = dsum[1];
                pp[2LL * q.part_stride] = dsum[2];
                pp[3LL * q.part_stride] = dsum[3];
            }
        }
        buf ^= 1;
        b = bn;
    }
}

}  // namespace

// ==========================================================================================
// host launchers
// ==========================================================================================
#ifndef STENCIL_P
#define STENCIL_P 1
#endif

int helm_stencil_tile_rows() { return 4 * STENCIL_P; }

int helm_apply_num_blocks(const helm_op *op) {
    if (op->ny > 0) return helm3d_apply_num_blocks(op);
    const int ntx = (op->nx + TX - 1) / TX, ntz = (op->nz + 4 * STENCIL_P - 1) / (4 * STENCIL_P);
    return ntx * ntz;
}

template <int P, bool SCALED, bool ADJ>
static void launch_stencil_epi(hipStream_t st, dim3 grid, const StencilParams &q, int epi) {
    switch (epi) {
    case EPI_NONE: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_NONE>), grid, dim3(256), 0, st, q); break;
    case EPI_DOT_W: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_DOT_W>), grid, dim3(256), 0, st, q); break;
    case EPI_DOT_XY: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_DOT_XY>), grid, dim3(256), 0, st, q); break;
    case EPI_DOT_YY: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_DOT_YY>), grid, dim3(256), 0, st, q); break;
    case EPI_RESID: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_RESID>), grid, dim3(256), 0, st, q); break;
    case EPI_JACOBI: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_JACOBI>), grid, dim3(256), 0, st, q); break;
    case EPI_DOT_WY: HELM_LAUNCH((k_stencil_t<cplx, P, SCALED, ADJ, EPI_DOT_WY>), grid, dim3(256), 0, st, q); break;
    }
}

// Kernel parameters of a 2-D launch.  The single-precision launches (multigrid levels) know neither tile-blocked planes nor an accumulating second
// half nor a partial-sum layout of the caller's.
template <class V>
static StencilParamsT<V> stencil_params(const helm_op *op, const ApplyArgs &a) {
    constexpr bool F64 = std::is_same<V, cplx>::value;
    StencilParamsT<V> q;
    q.planes = (const V *)a.planes; q.X = (const V *)a.X; q.Y = (V *)a.Y; q.W = (const V *)a.W; q.ld = a.ld; q.N = op->N;
    q.nz = op->nz; q.nx = op->nx; q.nrhs = a.nrhs;
    q.ntx = (op->nx + TX - 1) / TX; q.ntz = (op->nz + 4 * STENCIL_P - 1) / (4 * STENCIL_P);
    q.nblk = a.tiles ? a.ntiles : q.ntx * q.ntz;
    q.scal = a.scal; q.part = a.part; q.dinv = (const V *)a.dinv; q.omega_j = a.omega_j; q.tiles = a.tiles; q.planes_tiled = F64 ? a.planes_tiled : 0;
    q.U = (V *)a.U; q.E = (const V *)a.E; q.nzc = a.nzc; q.nxc = a.nxc;
    q.acc = F64 ? a.acc : 0; q.part_stride = F64 && a.part_stride > 0 ? a.part_stride : q.nblk; q.part_off = F64 ? a.part_off : 0;
    return q;
}
// tiles x right-hand-side groups: few tiles are topped up to about 1024 workgroups by splitting the right-hand-side loop
static dim3 stencil_grid(int nblk, int nrhs) {
    int split = 1;
    if (nblk < 1024) { split = (1024 + nblk - 1) / nblk; if (split > nrhs) split = nrhs; if (split < 1) split = 1; }
    return dim3(nblk, split);
}

// single-precision launches (multigrid levels): unscaled, forward, EPI_NONE / EPI_RESID / EPI_JACOBI; no event is ever recorded
static int launch_apply_f32(helm_op *op, const ApplyArgs &a) {
    const StencilParamsT<cplxf> q = stencil_params<cplxf>(op, a);
    if (q.nblk < 1) return HELM_OK;
    const dim3 grid = stencil_grid(q.nblk, a.nrhs);
    if (a.xmode == 1 && a.epi == EPI_RESID) HELM_LAUNCH((k_stencil_t<cplxf, STENCIL_P, false, false, EPI_RESID, 1>), grid, dim3(256), 0, op->stream, q);
    else if (a.xmode == 2 && a.epi == EPI_JACOBI) HELM_LAUNCH((k_stencil_t<cplxf, STENCIL_P, false, false, EPI_JACOBI, 2>), grid, dim3(256), 0, op->stream, q);
    else if (a.xmode != 0) HELM_FAIL(op, HELM_ERR_ARG, "unsupported fused stencil mode");
    else switch (a.epi) {
    case EPI_NONE: HELM_LAUNCH((k_stencil_t<cplxf, STENCIL_P, false, false, EPI_NONE>), grid, dim3(256), 0, op->stream, q); break;
    case EPI_RESID: HELM_LAUNCH((k_stencil_t<cplxf, STENCIL_P, false, false, EPI_RESID>), grid, dim3(256), 0, op->stream, q); break;
    case EPI_JACOBI: HELM_LAUNCH((k_stencil_t<cplxf, STENCIL_P, false, false, EPI_JACOBI>), grid, dim3(256), 0, op->stream, q); break;
    default: HELM_FAIL(op, HELM_ERR_ARG, "unsupported single-precision stencil epilogue");
    }
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}

int helm_launch_apply(helm_op *op, const ApplyArgs &a) {
    if (op->ny > 0) {           // 3-D operator: own kernel, same profiling bookkeeping
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (op->profiling && a.profile && op->ev_pool.size() < 8192) {
            if (op->ev_used + 2 > op->ev_pool.size())
                if (helm_events_grow(op, 64)) HELM_FAIL(op, HELM_ERR_DEVICE, "hipEventCreate failed");
            e0 = op->ev_pool[op->ev_used]; e1 = op->ev_pool[op->ev_used + 1];
        }
        int rc = helm3d_launch_apply(op, a, e0, e1);
        if (rc) return rc;
        if (e0) {
            const int nact = (a.scal && op->active_hint >= 0 && op->active_hint < a.nrhs) ? op->active_hint : a.nrhs;
            const bool operand = (a.epi == EPI_DOT_W || a.epi == EPI_RESID);
            op->ev_pending.push_back(std::make_pair((int)op->ev_used, (double)op->N * (32.0 * nact + 432.0 + (operand ? 16.0 * nact : 0.0))));
            op->ev_used += 2;
        }
        return HELM_OK;
    }
    if (a.f32) return launch_apply_f32(op, a);
    const StencilParams q = stencil_params<cplx>(op, a);
    if (q.nblk < 1) return HELM_OK;
    const dim3 grid = stencil_grid(q.nblk, a.nrhs);

    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool prof = op->profiling && a.profile;
    if (prof) {
        if (op->ev_used + 2 > op->ev_pool.size() && op->ev_pool.size() >= 8192) { e0 = nullptr; }
        else if (op->ev_used + 2 > op->ev_pool.size()) {
            if (helm_events_grow(op, 64)) HELM_FAIL(op, HELM_ERR_DEVICE, "hipEventCreate failed");
        }
        if (op->ev_used + 2 <= op->ev_pool.size()) {
            e0 = op->ev_pool[op->ev_used]; e1 = op->ev_pool[op->ev_used + 1];
            hipEventRecord(e0, op->stream);
        } else e0 = nullptr;
    }
    if (a.xmode == 1 && a.epi == EPI_RESID && !a.scaled && !a.adjoint) {
        HELM_LAUNCH((k_stencil_t<cplx, STENCIL_P, false, false, EPI_RESID, 1>), grid, dim3(256), 0, op->stream, q);
    } else if (a.xmode == 2 && a.epi == EPI_JACOBI && !a.scaled && !a.adjoint) {
        HELM_LAUNCH((k_stencil_t<cplx, STENCIL_P, false, false, EPI_JACOBI, 2>), grid, dim3(256), 0, op->stream, q);
    } else if (a.xmode != 0) {
        HELM_FAIL(op, HELM_ERR_ARG, "unsupported fused stencil mode");
    } else if (a.scaled) {
        if (a.adjoint) launch_stencil_epi<STENCIL_P, true, true>(op->stream, grid, q, a.epi);
        else launch_stencil_epi<STENCIL_P, true, false>(op->stream, grid, q, a.epi);
    } else {
        if (a.adjoint) launch_stencil_epi<STENCIL_P, false, true>(op->stream, grid, q, a.epi);
        else launch_stencil_epi<STENCIL_P, false, false>(op->stream, grid, q, a.epi);
    }
    if (prof && e0) {
        hipEventRecord(e1, op->stream);
        int nact = (a.scal && op->active_hint >= 0 && op->active_hint < a.nrhs) ? op->active_hint : a.nrhs;   // inactive RHS are skipped on the device
        // algorithmic bytes of the launch: the stencil apply N*(32*B + 144) plus, for the fused
        // epilogues that take an operand vector (dot with r0 / s, residual w - Ax), that operand's one read
        const bool operand = (a.epi == EPI_DOT_W || a.epi == EPI_DOT_WY || a.epi == EPI_RESID || a.epi == EPI_JACOBI);
        op->ev_pending.push_back(std::make_pair((int)op->ev_used, (double)op->N * (32.0 * nact + 144.0 + (operand ? 16.0 * nact : 0.0))));
        op->ev_used += 2;
    }
    HIP_TRY(op, hipGetLastError());
    return HELM_OK;
}
