// Direct solver, the bottom of the factorisation in one kernel per level: the leaves, and the small separator fronts just above them.
#include "nd_internal.hpp"
#include "nd_gj32w.hpp"

namespace {

// ---- the leaf level of the factorisation in one kernel (round 4) ---------------------------------------------------------------------------
// A leaf front is [F11 F12; F21 0] with F11 the 9-point operator of an h x w block of cells (h, w <= 8: a BANDED matrix of half-width w + 1) and
// F12 / F21 the stencil across the block's boundary (at most three entries per ring cell).  What the passes need from it is dense --
// [F11^-1 | G = -F11^-1 F12] (s x (s + m)), G21 = F21 F11^-1 (m x s) and the Schur complement S = F21 G (m x m) -- but getting there does not
// have to be: the batched path wrote every leaf as a dense 81 x 81 front (1.7 GB at 1024^2), inverted F11 by a 25 + 24 block recursion of
// Gauss-Jordan sweeps and small products and formed G21, S and G with three more batched products: 3.0 ms of a 16-ms factorisation, and round 3's
// first fused attempt (a scalar dense Gauss-Jordan in LDS) was slower still (4.2 ms).  Here one workgroup of two waves takes a leaf:
//   1. the band of F11 (SP x 19) and the sparse F12 / F21 tables go straight from the coefficient planes into LDS -- no front in HBM;
//   2. wave 0 factors the band, LU without pivoting (a 9 x 9 window per step); a pivot below 1 % of its row's largest original entry flags
//      the leaf, which k_leaf_factor_pivoted then re-does with a row-pivoted dense Gauss-Jordan (indefinite leaves at few points per
//      wavelength; none at the bench's 17);
//   3. every thread takes ONE column of [I | -F12] and runs the banded forward / backward substitution on it in registers, the factor's
//      entries arriving as LDS broadcasts: 2 x 9 x SP complex multiply-adds per column instead of SP^2 for a dense inverse, 81 columns at once;
//      the result is a column of [F11^-1 | G], stored row by row (consecutive threads = consecutive addresses) and, for the block's boundary
//      cells, kept in LDS;
//   4. G21 and S are the three-term sums  sum_t F21[r][a_t] X[a_t][c]  over those LDS rows.
// SP: padded size of F11 (49 for blocks of up to 7 x 7 cells, 64 up to 8 x 8; identity on the padding).
#define LEAF_NB 19           // band row: columns i - 9 .. i + 9
#define LEAF_NBR 28          // most boundary cells of a leaf (8 x 8: 64 - 36)
struct LeafTabs {
    int idx[LEAF_MP][3];     // leaf cells (local index) adjacent to ring cell r, -1: none
    cplx f12[LEAF_MP][3];    // F12[idx][r]: row = the leaf cell
    cplx f21[LEAF_MP][3];    // F21[r][idx]: row = the ring cell
};
// band of F11, the boundary-row map and the sparse tables of leaf n into LDS (all threads of the workgroup call; no barrier inside)
template <int SP>
__device__ __forceinline__ void leaf_load(const NdDev &n, const cplx *planes, int nz, int nx, cplx *band, float *rowmax, int *brow, LeafTabs &T, int tid, int nthreads) {
    const long long N = (long long)nz * nx;
    const int w = n.x1 - n.x0, h = n.z1 - n.z0;
    for (int e = tid; e < SP * LEAF_NB; e += nthreads) band[e] = (e % LEAF_NB == LEAF_BW && e / LEAF_NB >= n.s) ? cmake(1.0, 0.0) : cmake(0.0, 0.0);
    for (int a = tid; a < SP; a += nthreads) {
        int br = -1;
        if (a < n.s) {
            const int lz = a / w, lx = a % w;
            if (lz == 0 || lz == h - 1 || lx == 0 || lx == w - 1) {          // rank among the boundary cells, in local order
                int cnt = 0;
                for (int q = 0; q < a; ++q) { const int qz = q / w, qx = q % w; if (qz == 0 || qz == h - 1 || qx == 0 || qx == w - 1) cnt += 1; }
                br = cnt;
            }
        }
        brow[a] = br;
        rowmax[a] = 1.0f;
    }
    for (int e = tid; e < LEAF_MP * 3; e += nthreads) { T.idx[e / 3][e % 3] = -1; T.f12[e / 3][e % 3] = cmake(0.0, 0.0); T.f21[e / 3][e % 3] = cmake(0.0, 0.0); }
}
template <int SP>
__device__ __forceinline__ void leaf_fill(const NdDev &n, const cplx *planes, int nz, int nx, cplx *band, float *rowmax, LeafTabs &T, int tid, int nthreads) {
    const long long N = (long long)nz * nx;
    const int w = n.x1 - n.x0;
    for (int a = tid; a < n.s; a += nthreads) {                              // one leaf cell per thread: its nine stencil entries
        const int z = n.z0 + a / w, x = n.x0 + a % w;
        float mx = 0.f;
        #pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int z2 = z + k / 3 - 1, x2 = x + k % 3 - 1;
            if (z2 < n.z0 || z2 >= n.z1 || x2 < n.x0 || x2 >= n.x1) continue;
            const cplx v = planes[(long long)k * N + (long long)z * nx + x];
            const int b = (z2 - n.z0) * w + (x2 - n.x0);
            band[a * LEAF_NB + (b - a) + LEAF_BW] = v;
            mx = fmaxf(mx, (float)fmax(fabs(v.x), fabs(v.y)));
        }
        rowmax[a] = mx;
    }
    for (int r = tid; r < n.m; r += nthreads) {                              // one ring cell per thread: its (at most three) neighbours inside the block
        int zr, xr;
        nd_cell(n, n.s + r, zr, xr);
        int t = 0;
        for (int k = 0; k < 9; ++k) {
            const int z2 = zr + k / 3 - 1, x2 = xr + k % 3 - 1;
            if (z2 < n.z0 || z2 >= n.z1 || x2 < n.x0 || x2 >= n.x1 || t >= 3) continue;
            const int a = (z2 - n.z0) * w + (x2 - n.x0);
            T.idx[r][t] = a;
            T.f21[r][t] = planes[(long long)k * N + (long long)zr * nx + xr];                        // row = ring cell, neighbour offset k
            T.f12[r][t] = planes[(long long)(8 - k) * N + (long long)z2 * nx + x2];                  // row = leaf cell, the opposite offset
            t += 1;
        }
    }
}

template <int SP>
__global__ __launch_bounds__(128, 4) void k_leaf_factor(const NdDev *nodes, int first, cplx *arenaF, cplx *fac, cplx *g21base, const cplx *planes, int nz, int nx, int *flags, int dbg,
                                                        int nf, int kf) {
    __shared__ cplx band[SP * LEAF_NB];
    __shared__ LeafTabs T;
    __shared__ float rowmax[SP];
    __shared__ int brow[SP];
    __shared__ int bad;
    const NdDev n = nodes[first + blockIdx.x];
    const int tid = threadIdx.x;
    const int smax = n.smax, mmax = n.mmax, nmax = smax + mmax;
    if (tid == 0) bad = 0;
    leaf_load<SP>(n, planes, nz, nx, band, rowmax, brow, T, tid, 128);
    __syncthreads();
    leaf_fill<SP>(n, planes, nz, nx, band, rowmax, T, tid, 128);
    __syncthreads();
    if (tid < 64 && !(dbg & 1)) {                                            // wave 0: banded LU, no pivoting, window of 9 x 9 per step
        int mybad = 0;
        for (int k = 0; k < SP; ++k) {
            const cplx p = band[k * LEAF_NB + LEAF_BW];
            const double pm = fmax(fabs(p.x), fabs(p.y));
            if (!(pm >= 0.01 * (double)rowmax[k])) mybad = 1;
            const cplx pi = crecip(p);
            for (int e = tid; e < LEAF_BW * LEAF_BW; e += 64) {
                const int di = e / LEAF_BW + 1, dj = e % LEAF_BW + 1;
                const int i = k + di, j = k + dj;
                if (i < SP && j < SP) {
                    const cplx l = cmul(band[i * LEAF_NB + LEAF_BW - di], pi);
                    const cplx u = band[k * LEAF_NB + LEAF_BW + dj];
                    cplx &aij = band[i * LEAF_NB + (j - i) + LEAF_BW];
                    aij = csub(aij, cmul(l, u));
                }
            }
            // the multipliers of column k replace it (after every lane has read the old column: LDS serves a wave's instructions in order)
            if (tid < LEAF_BW && k + tid + 1 < SP) { cplx &l = band[(k + tid + 1) * LEAF_NB + LEAF_BW - (tid + 1)]; l = cmul(l, pi); }
            if (tid == LEAF_BW) band[k * LEAF_NB + LEAF_BW] = pi;            // (1 / pivot where the pivot was: no later step reads row k's diagonal)
        }
        if (mybad && tid == 0) bad = 1;
    }
    __syncthreads();
    if (tid == 0) flags[blockIdx.x] = (dbg & 8) ? 1 : bad;                  // (8: every leaf through the pivoted kernel -- a test)
    // ---- one column of [I | -F12] per thread through the banded substitutions.  Only a window of nine values lives in registers: the forward
    // pass parks its result in the column's own place in the factor storage, the backward pass picks it up from there (the thread's own stores,
    // L2-resident) and overwrites it with the solution -- ~70 registers, so that several leaves share a SIMD and cover each other's latencies
    // (a first version kept the whole column in registers: 400 of them, one wave per SIMD, and was no faster than the batched path).
    const int c = tid;
    const bool active = c < SP + mmax;
    const int gc = c < SP ? c : smax + (c - SP);                             // column in the [F11^-1 | G] rows of smax + mmax
    const bool stored = active && (c < SP ? c < smax : true);
    // (nf, kf: frequency kf of nf factored together -- this front's slots lie at nf * offset + kf * slot, direct.hpp; 1, 0: on its own)
    cplx *Fcol = fac + (long long)nf * n.finv_off + (long long)kf * smax * nmax + gc;
    // right-hand side of this column: e_c, or -F12[:, c - SP] (three entries at most)
    int ra0 = -1, ra1 = -1, ra2 = -1;
    cplx rv0 = cmake(0.0, 0.0), rv1 = rv0, rv2 = rv0;
    if (c < SP) { ra0 = c; rv0 = cmake(1.0, 0.0); }
    else if (c - SP < n.m) {
        ra0 = T.idx[c - SP][0]; rv0 = cneg(T.f12[c - SP][0]);
        ra1 = T.idx[c - SP][1]; rv1 = cneg(T.f12[c - SP][1]);
        ra2 = T.idx[c - SP][2]; rv2 = cneg(T.f12[c - SP][2]);
    }
#define LEAF_RHS(i_) (ra0 == (i_) ? rv0 : (ra1 == (i_) ? rv1 : (ra2 == (i_) ? rv2 : cmake(0.0, 0.0))))
    // The factor's entries are the same for every column, i.e. wave-uniform: ONE ds_read per row brings the row's 19 band entries into lanes
    // 0..18 (multipliers in 0..8, 1 / pivot in 9, the upper row in 10..18), fetched a row ahead, and v_readlane hands each to the whole wave.
    const int lb = (tid & 63) < LEAF_NB ? (tid & 63) : LEAF_NB - 1;
    auto bcast = [](cplx v, int l) {
        cplx r;
        r.x = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v.x), l), __builtin_amdgcn_readlane(__double2loint(v.x), l));
        r.y = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v.y), l), __builtin_amdgcn_readlane(__double2loint(v.y), l));
        return r;
    };
    if (!(dbg & 2)) {
        {
            cplx yw[SP];                                                     // (fully unrolled: each entry is live for nine rows only)
            cplx cur = band[0 * LEAF_NB + lb];
            #pragma unroll
            for (int i = 0; i < SP; ++i) {
                cplx nxt = cur;
                if (i + 1 < SP) nxt = band[(i + 1) * LEAF_NB + lb];
                cplx acc = LEAF_RHS(i);
                #pragma unroll
                for (int d = 1; d <= LEAF_BW; ++d)
                    if (i - d >= 0) { const cplx l = bcast(cur, LEAF_BW - d); acc.x = fma(l.y, yw[i - d].y, fma(-l.x, yw[i - d].x, acc.x)); acc.y = fma(-l.y, yw[i - d].x, fma(-l.x, yw[i - d].y, acc.y)); }
                yw[i] = acc;
                if (stored && i < smax) Fcol[(long long)i * nmax] = acc;
                cur = nxt;
            }
        }
        {
            constexpr int AHEAD = 6;                                         // rows fetched back ahead of the one being worked on
            cplx xw[SP], yq[SP];                                             // (fully unrolled: every entry is a value of its own, live for a few rows)
            #pragma unroll
            for (int i = SP - 1; i >= SP - AHEAD && i >= 0; --i) yq[i] = (stored && i < smax) ? Fcol[(long long)i * nmax] : LEAF_RHS(i);
            cplx cur = band[(SP - 1) * LEAF_NB + lb];
            #pragma unroll
            for (int i = SP - 1; i >= 0; --i) {
                if (i - AHEAD >= 0) yq[i - AHEAD] = (stored && i - AHEAD < smax) ? Fcol[(long long)(i - AHEAD) * nmax] : LEAF_RHS(i - AHEAD);
                cplx nxt = cur;
                if (i > 0) nxt = band[(i - 1) * LEAF_NB + lb];
                cplx acc = yq[i];
                #pragma unroll
                for (int d = 1; d <= LEAF_BW; ++d)
                    if (i + d < SP) { const cplx u = bcast(cur, LEAF_BW + d); acc.x = fma(u.y, xw[i + d].y, fma(-u.x, xw[i + d].x, acc.x)); acc.y = fma(-u.y, xw[i + d].x, fma(-u.x, xw[i + d].y, acc.y)); }
                acc = cmul(acc, bcast(cur, LEAF_BW));
                xw[i] = acc;
                if (stored && i < smax) Fcol[(long long)i * nmax] = acc;
                cur = nxt;
            }
        }
    }
    __syncthreads();                                                         // (every column of this leaf is in place: the other wave's too)
    // G21 = F21 F11^-1 (columns c < smax) and S = F21 G (columns SP .. SP + mmax): three-term sums over rows of [F11^-1 | G] read back
    if (active && !(dbg & 4)) {
        cplx *G21 = g21base + ((long long)blockIdx.x * nf + kf) * mmax * smax;
        cplx *S = arenaF + (long long)nf * n.foff + (long long)kf * mmax * nmax + smax;
        for (int r = 0; r < mmax; ++r) {
            cplx acc = cmake(0.0, 0.0);
            if (r < n.m && stored) {
                #pragma unroll
                for (int t = 0; t < 3; ++t) {
                    const int a = T.idx[r][t];
                    if (a >= 0) cfma(acc, T.f21[r][t], Fcol[(long long)a * nmax]);
                }
            }
            if (c < SP) { if (c < smax) G21[(long long)r * smax + c] = acc; }
            else S[(long long)r * nmax + (c - SP)] = acc;
        }
    }
}


// a flagged leaf once more, with row pivoting: dense Gauss-Jordan of F11 in LDS, then the same three sparse products
__global__ __launch_bounds__(256) void k_leaf_factor_pivoted(const NdDev *nodes, int first, cplx *arenaF, cplx *fac, cplx *g21base, const cplx *planes, int nz, int nx, const int *flags,
                                                             int nf, int kf) {
    if (!flags[blockIdx.x]) return;
    __shared__ cplx a[GJ_MAX][GJ_MAX + 1];
    __shared__ cplx fcol[GJ_MAX];
    __shared__ int piv[GJ_MAX];
    __shared__ LeafTabs T;
    const NdDev n = nodes[first + blockIdx.x];
    const int tid = threadIdx.x;
    const int smax = n.smax, mmax = n.mmax, nmax = smax + mmax, w = n.x1 - n.x0;
    const long long N = (long long)nz * nx;
    for (int e = tid; e < GJ_MAX * GJ_MAX; e += 256) { const int i = e / GJ_MAX, j = e % GJ_MAX; a[i][j] = (i == j && i >= n.s) ? cmake(1.0, 0.0) : cmake(0.0, 0.0); }
    for (int e = tid; e < LEAF_MP * 3; e += 256) { T.idx[e / 3][e % 3] = -1; T.f12[e / 3][e % 3] = cmake(0.0, 0.0); T.f21[e / 3][e % 3] = cmake(0.0, 0.0); }
    __syncthreads();
    for (int q = tid; q < n.s; q += 256) {
        const int z = n.z0 + q / w, x = n.x0 + q % w;
        for (int k = 0; k < 9; ++k) {
            const int z2 = z + k / 3 - 1, x2 = x + k % 3 - 1;
            if (z2 < n.z0 || z2 >= n.z1 || x2 < n.x0 || x2 >= n.x1) continue;
            a[q][(z2 - n.z0) * w + (x2 - n.x0)] = planes[(long long)k * N + (long long)z * nx + x];
        }
    }
    for (int r = tid; r < n.m; r += 256) {
        int zr, xr;
        nd_cell(n, n.s + r, zr, xr);
        int t = 0;
        for (int k = 0; k < 9; ++k) {
            const int z2 = zr + k / 3 - 1, x2 = xr + k % 3 - 1;
            if (z2 < n.z0 || z2 >= n.z1 || x2 < n.x0 || x2 >= n.x1 || t >= 3) continue;
            T.idx[r][t] = (z2 - n.z0) * w + (x2 - n.x0);
            T.f21[r][t] = planes[(long long)k * N + (long long)zr * nx + xr];
            T.f12[r][t] = planes[(long long)(8 - k) * N + (long long)z2 * nx + x2];
            t += 1;
        }
    }
    __syncthreads();
    gj_lds<GJ_MAX>(a, fcol, piv, smax, tid, 256);                         // a = F11^-1 (identity on the padding)
    cplx *Frow = fac + (long long)nf * n.finv_off + (long long)kf * smax * nmax;
    for (int e = tid; e < smax * nmax; e += 256) {
        const int i = e / nmax, cc = e % nmax;
        cplx v;
        if (cc < smax) v = a[i][cc];
        else {                                                               // G[i][b] = -sum_t F11^-1[i][a_t] F12[a_t][b]
            v = cmake(0.0, 0.0);
            const int b = cc - smax;
            if (b < n.m) for (int t = 0; t < 3; ++t) { const int q = T.idx[b][t]; if (q >= 0) cfma(v, a[i][q], cneg(T.f12[b][t])); }
        }
        Frow[(long long)i * nmax + cc] = v;
    }
    cplx *G21 = g21base + ((long long)blockIdx.x * nf + kf) * mmax * smax;
    cplx *S = arenaF + (long long)nf * n.foff + (long long)kf * mmax * nmax + smax;
    for (int e = tid; e < mmax * nmax; e += 256) {
        const int r = e / nmax, cc = e % nmax;
        cplx v = cmake(0.0, 0.0);
        if (r < n.m) {
            if (cc < smax) { for (int t = 0; t < 3; ++t) { const int q = T.idx[r][t]; if (q >= 0) cfma(v, T.f21[r][t], a[q][cc]); } }
            else {
                const int b = cc - smax;
                if (b < n.m)
                    for (int t = 0; t < 3; ++t) {
                        const int q = T.idx[r][t];
                        if (q < 0) continue;
                        cplx gqb = cmake(0.0, 0.0);
                        for (int u = 0; u < 3; ++u) { const int q2 = T.idx[b][u]; if (q2 >= 0) cfma(gqb, a[q][q2], cneg(T.f12[b][u])); }
                        cfma(v, T.f21[r][t], gqb);
                    }
            }
        }
        if (cc < smax) G21[(long long)r * smax + cc] = v; else S[(long long)r * nmax + (cc - smax)] = v;
    }
}

// ---- the small separator levels of the factorisation in one kernel each ------------------------------------------------------------------------
// The three levels above the leaves (8 or 16 separator cells, rings of 48-96 at 1024^2) went through seven launches apiece -- build, two condition
// estimates, the one-wave inverse, two products with an inner dimension of 8 or 16 -- each of which filled the chip and moved the front through HBM
// again.  Here a workgroup of four waves takes one (front, frequency) from the coefficient planes and the children's Schur complements to its
// factors and its own Schur complement:
//   1. [F11 | F12] (smax rows of smax + mmax) is gathered into LDS with k_nd_build_front's maps, sum order and padding, every load of a pass issued
//      before the first is used (a term that is not there loads its base's first element and is zeroed when it is used: no load is branched around);
//   2. the condition estimates of a watched group are formed of the block in LDS exactly as k_front_cond<0> / <1> form them of the one in HBM;
//   3. wave 0 inverts F11 in registers (gj32w_core) while the other waves gather their first 16 ring rows of F21 -- as matrix-core operands, straight
//      into registers: F21 never exists as a block;
//   4. both products run TRANSPOSED on the matrix cores, G21^T = F11^-T F21^T and S^T = C^T - F12^T G21^T, 16 ring rows per wave at a time: the
//      accumulator layout of the first (lane: ring row l & 15, k = (l >> 4) + 4 q) is the B-operand layout of the second, register q = k group q,
//      so G21 goes from one product to the next without leaving the registers.  Term by term these are the products of zgemm3_body -- the same
//      four real instructions per k group in the same order on accumulators kept apart, the two factors of every multiplication exchanged;
//   5. [F11^-1 | F12], G21 and S are stored where the batched path leaves them; [F21 | .] of the arena is not written (nobody reads it: the parent
//      takes S, and the re-elimination of a flagged front builds the whole front again from the children).
// SP: smax padded to the matrix cores' k groups (8 or 16).  LDS: 16 (SP = 8) or 32 KB of front, the inverse once more in fragment order (2 / 4 KB), 4 KB of tables:
// 22 / 40 KB, four workgroups per compute unit; 115 registers, four waves per SIMD.  Variants measured and not kept: HISTORY.md.
static __device__ cplx g_sep_zero[4];        // stands in for the Schur complement of a child that is not there

// k_front_cond<AFTER> (nd_factor.hip) of an n x n block held in LDS: the same sums in the same order, so that the lists of flagged fronts come out the same
template <int AFTER>
__device__ __forceinline__ void sep_cond(const cplx *M, int ld, int n, int tr, double *dsh, unsigned char *lone, double *wsh, double *red, double *out, double *wglob, int tid) {
    const int lane = tid & 63, wv = tid >> 6;
    double best = 0.0;
    if (tr) {
        const int j = tid;
        if (j < n) {
            double v = 0.0, off = 0.0;
            for (int i = 0; i < n; ++i) {
                const cplx a = M[i * ld + j];
                const double m = fabs(a.x) + fabs(a.y);
                v += AFTER ? m * wsh[i] : m;
                if (!AFTER && i != j) off += m;
            }
            if (!AFTER) { dsh[j] = v; lone[j] = off == 0.0; }
            best = v;
        }
        if (AFTER) for (int o = 32; o > 0; o >>= 1) best = fmax(best, __shfl_down(best, o));
    } else
    for (int i = wv; i < n; i += 4) {
        double v = 0.0, off = 0.0;
        for (int j = lane; j < n; j += 64) {
            const cplx a = M[i * ld + j];
            const double m = fabs(a.x) + fabs(a.y);
            v += AFTER ? m * wsh[j] : m;
            if (!AFTER && j != i) off += m;
        }
        for (int o = 32; o > 0; o >>= 1) { v += __shfl_down(v, o); if (!AFTER) off += __shfl_down(off, o); }
        v = __shfl(v, 0);
        if (!AFTER && lane == 0) { dsh[i] = v; lone[i] = off == 0.0; }
        best = fmax(best, v);
    }
    if (!AFTER) {
        __syncthreads();
        double a = 0.0, any = 0.0;
        for (int i = 0; i < n; ++i) { any = fmax(any, dsh[i]); if (!lone[i]) a = fmax(a, dsh[i]); }
        if (!(a > 0.0)) a = any > 0.0 ? any : 1.0;
        if (tid < n) { const double w = lone[tid] ? dsh[tid] / a : 1.0; wsh[tid] = w; wglob[tid] = w; }
        if (tid == 0) *out = a;
        __syncthreads();
        return;
    }
    if (lane == 0) red[wv] = best;
    __syncthreads();
    if (tid == 0) *out = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

template <int SP>
__global__ __launch_bounds__(256, 4) void k_sep_factor_small(const NdDev *nodes, int first, cplx *arenaF, cplx *fac, cplx *g21base, NdPlanesSet pset, int nz, int nx, int nf,
                                                             double *est, double *est_rows, long long nbatch, int tr) {
    constexpr int KG = SP / 4;
    __shared__ cplx FS[SP * 128];            // [F11 | F12], rows of smax + mmax <= 128: the image of the front's slot in the factor storage
    __shared__ int4 finfo[128];              // per padded front row: cell (z, x; z = -1: padding), position on child 0's / child 1's ring (-1: not there)
    __shared__ Gj32w GS;
    __shared__ cplx FI[KG * 64];             // F11^-1 once more, in the order the first product reads it: lane l of k group g at g * 64 + l (zero on the padding)
    __shared__ double dsh[16], wsh[16], red[4];
    __shared__ unsigned char lone[16];
    const long long b = blockIdx.x;          // batch index = front * nf + frequency
    const int front = (int)(b / nf), kf = (int)(b - (long long)front * nf);
    const cplx *planes = pset.p[kf];
    const NdDev n = nodes[first + front];
    const int smax = n.smax, mmax = n.mmax, nmax = smax + mmax;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63, lr = lane & 15, lq = lane >> 4;      // (wave: uniform, in a scalar register)
    const long long N = (long long)nz * nx;
    const int ns = n.s;
    // per padded front row: its cell, then its position on each child's ring (the children's records one after the other: three records at once do not fit
    // the scalar registers; a thread looks after the same rows in every pass, so no barrier between them)
    for (int r = tid; r < nmax; r += 256) {
        int a = -1;
        if (r < n.s) a = r;
        else if (r >= smax && r - smax < n.m) a = n.s + r - smax;
        int4 e = make_int4(-1, 0, -1, -1);
        if (a >= 0) nd_cell(n, a, e.x, e.y);
        finfo[r] = e;
    }
    const cplx *S0 = g_sep_zero, *S1 = g_sep_zero;           // the children's Schur complements (this frequency's), row lengths ld0 / ld1
    int ld0 = 0, ld1 = 0;
    #pragma unroll
    for (int slot = 0; slot < 2; ++slot) {
        if (n.kid[slot] < 0) continue;
        const NdDev c = nodes[n.kid[slot]];
        const int ldc = c.smax + c.mmax;
        const cplx *Sc = arenaF + (long long)nf * c.foff + (long long)kf * c.mmax * ldc + c.smax;
        if (slot == 0) { S0 = Sc; ld0 = ldc; } else { S1 = Sc; ld1 = ldc; }
        for (int r = tid; r < nmax; r += 256) {
            const int4 e = finfo[r];
            if (e.x < 0) continue;
            const int la = nd_local(c, nz, nx, e.x, e.y);
            if (la >= c.s) { if (slot == 0) finfo[r].z = la - c.s; else finfo[r].w = la - c.s; }
        }
    }
    const long long finv_off = n.finv_off, foff = n.foff;
    __syncthreads();
    // The three terms of front entry (r, c) -- stencil coefficient, child 0's and child 1's Schur-complement entry, summed in that order (k_nd_build_front) -- as
    // byte offsets from three bases that sit in scalar registers (the planes, the children's blocks; 32 bits: the caller checks that the planes stay below 4 GB).
    // A term that is not there loads its base's first element and is set to zero when it is used (mask bit t: term t is there; bit 3: an identity entry of the
    // padding): no load is branched around, so that all loads of a pass are in flight together.
    auto addr = [&](int r, int c, bool ok, unsigned (&o)[3]) -> unsigned {
        o[0] = 0u; o[1] = 0u; o[2] = 0u;
        if (!ok) return 0u;
        const int4 ia = finfo[r], ib = finfo[c];
        if (ia.x < 0 || ib.x < 0) return (r == c && r < smax) ? 8u : 0u;
        unsigned m = 0u;
        if (r < smax || c < smax) {              // ring x ring entries belong to an ancestor
            const int dz = ib.x - ia.x, dx = ib.y - ia.y;
            if (dz >= -1 && dz <= 1 && dx >= -1 && dx <= 1) { o[0] = (unsigned)(((dz + 1) * 3 + dx + 1) * (int)N + ia.x * nx + ia.y) * 16u; m |= 1u; }
        }
        if (ia.z >= 0 && ib.z >= 0) { o[1] = (unsigned)(ia.z * ld0 + ib.z) * 16u; m |= 2u; }
        if (ia.w >= 0 && ib.w >= 0) { o[2] = (unsigned)(ia.w * ld1 + ib.w) * 16u; m |= 4u; }
        return m;
    };
    auto at = [](const cplx *base, unsigned off) -> cplx { return *reinterpret_cast<const cplx *>(reinterpret_cast<const char *>(base) + off); };
    auto entry = [](unsigned m, cplx v0, cplx v1, cplx v2) -> cplx {
        const cplx z = cmake(0.0, 0.0);
        return (m & 8u) ? cmake(1.0, 0.0) : cadd(cadd((m & 1u) ? v0 : z, (m & 2u) ? v1 : z), (m & 4u) ? v2 : z);
    };
    // ---- 1. [F11 | F12] into LDS, four entries (twelve loads) per thread in flight
    const int tot = smax * nmax;
    for (int e0 = 0; e0 < tot; e0 += 1024) {
        unsigned o[4][3], m[4];
        #pragma unroll
        for (int u = 0; u < 4; ++u) { const int e = e0 + u * 256 + tid; const int r = e / nmax; m[u] = addr(r, e - r * nmax, e < tot, o[u]); }
        cplx v[4][3];
        #pragma unroll
        for (int u = 0; u < 4; ++u) { v[u][0] = at(planes, o[u][0]); v[u][1] = at(S0, o[u][1]); v[u][2] = at(S1, o[u][2]); }
        #pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * 256 + tid;
            if (e < tot) FS[e] = entry(m[u], v[u][0], v[u][1], v[u][2]);
        }
    }
    __syncthreads();
    // ---- 2. condition estimate, before the inversion
    if (est) sep_cond<0>(FS, nmax, ns, tr, dsh, lone, wsh, red, est + b, est_rows + b * smax, tid);
    // 16 ring rows of F21 as the B operand of the transposed first product: lane (lq, lr) holds F21[16 rb + lr][4 g + lq], g = 0 .. KG - 1
    auto gather_f21 = [&](int rb, int lr, int lq, cplx (&f)[KG]) {
        unsigned o[KG][3], m[KG];
        const int rr = 16 * rb + lr;
        #pragma unroll
        for (int g = 0; g < KG; ++g) { const int j = 4 * g + lq; m[g] = addr(smax + rr, j, rr < mmax && j < smax, o[g]); }
        cplx v[KG][3];
        #pragma unroll
        for (int g = 0; g < KG; ++g) { v[g][0] = at(planes, o[g][0]); v[g][1] = at(S0, o[g][1]); v[g][2] = at(S1, o[g][2]); }
        #pragma unroll
        for (int g = 0; g < KG; ++g) f[g] = entry(m[g], v[g][0], v[g][1], v[g][2]);
    };
    // ---- 3. F11 -> F11^-1 in place (wave 0, as k_gj32w_inverse does it); the other waves fetch their first block of F21 meanwhile
    if (wave == 0) {
        const int r = lane & 31, h = lane >> 5;
        cplx a[16];
        #pragma unroll
        for (int c = 0; c < 16; ++c) {
            const int j = 16 * h + c;
            const bool in = r < smax && j < smax;
            const cplx v = FS[in ? r * nmax + j : 0];
            a[c] = in ? v : cmake(r == j ? 1.0 : 0.0, 0.0);
        }
        gj32w_core(a, GS, smax, r, h);
        // inv[i][sigma(kcol)] = R[sigma(i)][kcol]: this lane holds storage row r = sigma(i), i.e. output row i = sinv[r]
        if (r < smax) {
            const int i = GS.sinv[r] & 31;
            #pragma unroll
            for (int c = 0; c < 16; ++c) {
                const int kcol = 16 * h + c;
                const int col = GS.sigma[kcol & 31] & 31;
                if (kcol < smax && i < smax && col < smax) FS[i * nmax + col] = a[c];
            }
        }
    }
    __syncthreads();
    if (est) sep_cond<1>(FS, nmax, ns, tr, dsh, lone, wsh, red, est + nbatch + b, est_rows + b * smax, tid);
    // ---- 5a. [F11^-1 | F12] where the passes look for it
    {
        cplx *Fout = fac + (long long)nf * finv_off + (long long)kf * smax * nmax;
        for (int e = tid; e < tot; e += 256) Fout[e] = FS[e];
        for (int e = tid; e < KG * 64; e += 256) {
            const int j = 4 * (e >> 6) + ((e & 63) >> 4), k = e & 15;
            const bool in = j < smax && k < smax;
            const cplx v = FS[in ? j * nmax + k : 0];                                 // F11^-1[j][k]
            FI[e] = in ? v : cmake(0.0, 0.0);
        }
    }
    __syncthreads();
    // ---- 4. the two products, 16 ring rows per wave at a time
    cplx *G21 = g21base + b * mmax * smax;
    cplx *S = arenaF + (long long)nf * foff + (long long)kf * mmax * nmax + smax;
    const int nblk = (mmax + 15) >> 4;
    const cplx mone = cmake(-1.0, 0.0);
    for (int rb = wave; rb < nblk; rb += 4) {
        cplx f21[KG];
        gather_f21(rb, lr, lq, f21);
        const int rr = 16 * rb + lr;                                                   // this lane's ring row in both accumulators
        const bool rok = rr < mmax;
        // G21^T = F11^-T F21^T: lane holds G21[rr][lq + 4 q] in (gr[q], gi[q])
        v4f64 gr = (v4f64){0, 0, 0, 0}, gi = (v4f64){0, 0, 0, 0};
        #pragma unroll
        for (int g = 0; g < KG; ++g) {
            const cplx fv = FI[g * 64 + lane];                                      // F11^-1[4 g + lq][k = lr]
            const cplx a = f21[g];
            gr = __builtin_amdgcn_mfma_f64_16x16x4f64(fv.x, a.x, gr, 0, 0, 0);
            gi = __builtin_amdgcn_mfma_f64_16x16x4f64(fv.y, a.x, gi, 0, 0, 0);
            gr = __builtin_amdgcn_mfma_f64_16x16x4f64(fv.y, -a.y, gr, 0, 0, 0);
            gi = __builtin_amdgcn_mfma_f64_16x16x4f64(fv.x, a.y, gi, 0, 0, 0);
        }
        #pragma unroll
        for (int q = 0; q < KG; ++q) {
            const int k = lq + 4 * q;
            if (rok && k < smax) G21[(long long)rr * smax + k] = cmake(gr[q], gi[q]);
        }
        const int4 er = finfo[smax + (rok ? rr : 0)];
        // the children's entries of S[rr][16 cb + lq + 4 q], q = 0 .. 3: eight loads, none waited for here.  A masked entry loads the block's first element and is
        // set to zero when it is used (bit q / 4 + q of the mask: child 0 / 1 has the entry) -- no branch around a load, and every address is the child's base in
        // scalar registers plus a 32-bit offset
        auto load_cv = [&](int cb, cplx (&c0)[4], cplx (&c1)[4]) -> unsigned {
            unsigned mask = 0;
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = 16 * cb + lq + 4 * q;
                const bool ok = rok && c < mmax;
                const int4 ec = finfo[smax + (ok ? c : 0)];
                const bool ok0 = ok && er.z >= 0 && ec.z >= 0, ok1 = ok && er.w >= 0 && ec.w >= 0;
                const unsigned o0 = ok0 ? (unsigned)(er.z * ld0 + ec.z) * 16u : 0u, o1 = ok1 ? (unsigned)(er.w * ld1 + ec.w) * 16u : 0u;
                c0[q] = at(S0, o0);
                c1[q] = at(S1, o1);
                mask |= (ok0 ? 1u : 0u) << q | (ok1 ? 16u : 0u) << q;
            }
            return mask;
        };
        for (int cb = 0; cb < nblk; ++cb) {
            cplx nx0[4], nx1[4];
            const unsigned nmask = load_cv(cb, nx0, nx1);
            v4f64 sr = (v4f64){0, 0, 0, 0}, si = (v4f64){0, 0, 0, 0};
            #pragma unroll
            for (int g = 0; g < KG; ++g) {
                const int k = 4 * g + lq, cc = 16 * cb + lr;
                const bool in = k < smax && cc < mmax;
                cplx fb = FS[in ? k * nmax + smax + cc : 0];                         // F12[k][cc]
                if (!in) fb = cmake(0.0, 0.0);
                const double ar = gr[g], ai = gi[g];                                // G21[rr][4 g + lq]
                sr = __builtin_amdgcn_mfma_f64_16x16x4f64(fb.x, ar, sr, 0, 0, 0);
                si = __builtin_amdgcn_mfma_f64_16x16x4f64(fb.y, ar, si, 0, 0, 0);
                sr = __builtin_amdgcn_mfma_f64_16x16x4f64(fb.y, -ai, sr, 0, 0, 0);
                si = __builtin_amdgcn_mfma_f64_16x16x4f64(fb.x, ai, si, 0, 0, 0);
            }
            #pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = 16 * cb + lq + 4 * q;
                const cplx cv = cadd((nmask >> q) & 1u ? nx0[q] : cmake(0.0, 0.0), (nmask >> (4 + q)) & 1u ? nx1[q] : cmake(0.0, 0.0));
                if (rok && c < mmax) S[(long long)rr * nmax + c] = cadd(cv, cmul(mone, cmake(sr[q], si[q])));
            }
        }
    }
}

}  // namespace

// the whole elimination of nbatch = fronts x frequencies small separator fronts of one level (smax <= 16, smax + mmax <= 128, one unknown per cell);
// est / est_rows: where k_front_cond would leave the condition estimates of a watched group (null: not watched), nbatch_all: the group's batch (the
// second estimate lies that far behind the first), tr: a transposed handle
void launch_sep_factor_small(hipStream_t st, int smax, int nb, const NdDev *d_nodes, int first, cplx *arenaF, cplx *fac, cplx *g21b, const NdPlanesSet &ps, int nz, int nx, int nf,
                             double *est, double *est_rows, long long nbatch_all, int tr) {
    if (smax <= 8) ZG_LAUNCH(k_sep_factor_small<8>, dim3(nb), d_nodes, first, arenaF, fac, g21b, ps, nz, nx, nf, est, est_rows, nbatch_all, tr);
    else ZG_LAUNCH(k_sep_factor_small<16>, dim3(nb), d_nodes, first, arenaF, fac, g21b, ps, nz, nx, nf, est, est_rows, nbatch_all, tr);
}

// (nf, kf: frequency kf of a set of nf -- fac / arenaF / g21b are the SET's bases, the kernels place this frequency's slots among the interleaved ones)
void launch_leaf_factor(hipStream_t st, int smax, int nb, const NdDev *d_nodes, int first, cplx *arenaF, cplx *fac, cplx *g21b, const cplx *planes, int nz, int nx, int *flags, int dbg,
                        int nf, int kf) {
    if (smax <= 49) HELM_LAUNCH(k_leaf_factor<49>, dim3(nb), dim3(128), 0, st, d_nodes, first, arenaF, fac, g21b, planes, nz, nx, flags, dbg, nf, kf);
    else HELM_LAUNCH(k_leaf_factor<64>, dim3(nb), dim3(128), 0, st, d_nodes, first, arenaF, fac, g21b, planes, nz, nx, flags, dbg, nf, kf);
    HELM_LAUNCH(k_leaf_factor_pivoted, dim3(nb), dim3(256), 0, st, d_nodes, first, arenaF, fac, g21b, planes, nz, nx, (const int *)flags, nf, kf);
}
