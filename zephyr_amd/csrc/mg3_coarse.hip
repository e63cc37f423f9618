// Direct solvers of the last level of the layer-preserving 3-D hierarchy (mg3_keep.hip builds the level, cycle_keep of mg3d.hip solves on it).
//   Bt3: block-tridiagonal elimination over the planes normal to the longest axis -- dense plane inverses in HBM (8.7 GB in single precision for the
//        79 x 79 x 47 level of config 5), twisted set-up on two streams, applied as split-K products in two chains.
//   Nd3: the column dissection -- the multifrontal solver of the 2-D path over the grid of z-columns.
// mg3_coarse_is_nd chooses between them; mg3_bt_shape is the one place that knows what Bt3 allocates.
#include "mg3_internal.hpp"
#include <map>
#include <tuple>
#include <mutex>

// what the plane-by-plane elimination of a level of d = (nz, ny, nx) nodes allocates for `batch` right-hand sides
BtShape mg3_bt_shape(const int d[3], int batch, const helm_tuning &tune) {
    BtShape S;
    for (int a = 1; a < 3; ++a) if (d[a] > d[S.axis]) S.axis = a;       // planes normal to the longest axis are the smallest
    S.np = d[S.axis]; S.m = d[(S.axis + 1) % 3] * d[(S.axis + 2) % 3];
    // split-K: ~512 workgroups of 128 columns each (k_bt_apply); more than 16 right-hand sides go through the generic batched GEMM instead
    S.own = batch <= 16;
    S.ksplit = S.own ? std::max(1, std::min(16, 512 / ((S.m + 127) / 128))) : std::max(1, std::min(16, 255 / ((S.m + 63) / 64)));
    S.kc = (S.m + S.ksplit - 1) / S.ksplit;
    S.mpad = S.own ? S.m : S.kc * S.ksplit;          // (the generic GEMM wants equal K chunks: zero rows / columns up to mpad)
    // single-precision plane inverses (default): only two double-precision planes per chain exist at a time during the set-up
    S.f32 = S.own && tune.mg3_bt_f32 != 0;
    S.ld32 = (S.m + 1) & ~1;
    S.wbytes = (size_t)S.m * S.m * sizeof(cplx);
    S.tbytes = S.f32 ? 4 * S.wbytes : (size_t)S.np * S.mpad * S.m * sizeof(cplx);
    S.tbytes32 = S.f32 ? (size_t)S.np * S.m * S.ld32 * sizeof(float2) : 0;
    return S;
}

namespace {
// ---- block-tridiagonal direct solver of the coarsest level ------------------------------------------------------------
__device__ __forceinline__ int bt_slot(int axis, int os, int da, int db) {
    const int oz = axis == 0 ? os : da, oy = axis == 0 ? da : (axis == 1 ? os : db), ox = axis == 2 ? os : db;
    return 9 * (oz + 1) + 3 * (oy + 1) + (ox + 1);
}

// T_k = S_k^T with S_k = A_kk - sum over the eliminated neighbour planes k + d (d = -1 and / or +1) of A_{k,k+d} S_{k+d}^{-1} A_{k+d,k};
// Tm / Tp = T_{k-1}^{-1} / T_{k+1}^{-1} or null (element [b][a] of T^{-1} is S^{-1}[a][b]).
// One thread per entry, i (the row of S) fastest: coalesced writes of T[j][i] and reads of T^{-1}[b][a ~ i].
__global__ __launch_bounds__(256) void k_bt_schur_t(const cplx *__restrict__ planes, BtGeom g, int k, const cplx *__restrict__ Tm, const cplx *__restrict__ Tp,
                                                    cplx *__restrict__ T) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)g.m * g.m) return;
    const int i = (int)(e % g.m), j = (int)(e / g.m);
    const int ia = i / g.nb, ib = i % g.nb, ja = j / g.nb, jb = j % g.nb;
    const long long node_i = (long long)k * g.ss + ia * g.sa + ib * g.sb;
    cplx v = cmake(0.0, 0.0);
    if (abs(ja - ia) <= 1 && abs(jb - ib) <= 1) v = planes[(long long)bt_slot(g.axis, 0, ja - ia, jb - ib) * g.N + node_i];
    for (int side = 0; side < 2; ++side) {
        const cplx *Tn = side ? Tp : Tm;
        if (!Tn) continue;
        const int d = side ? 1 : -1;
        // the nine entries of row i of A_{k,k+d} (kept in registers) and of column j of A_{k+d,k}
        cplx am9[9]; int off9[9];
        #pragma unroll
        for (int d1 = 0; d1 < 9; ++d1) {
            const int aa = ia + (d1 / 3 - 1), ab = ib + (d1 % 3 - 1);
            const bool in = aa >= 0 && aa < g.na && ab >= 0 && ab < g.nb;
            off9[d1] = in ? aa * g.nb + ab : -1;
            am9[d1] = in ? planes[(long long)bt_slot(g.axis, d, d1 / 3 - 1, d1 % 3 - 1) * g.N + node_i] : cmake(0.0, 0.0);
        }
        for (int d2 = 0; d2 < 9; ++d2) {
            const int ba = ja - (d2 / 3 - 1), bb = jb - (d2 % 3 - 1);
            if (ba < 0 || ba >= g.na || bb < 0 || bb >= g.nb) continue;
            const long long node_b = (long long)(k + d) * g.ss + ba * g.sa + bb * g.sb;
            const cplx ap = planes[(long long)bt_slot(g.axis, -d, d2 / 3 - 1, d2 % 3 - 1) * g.N + node_b];
            if (ap.x == 0.0 && ap.y == 0.0) continue;
            const cplx *trow = Tn + (long long)(ba * g.nb + bb) * g.m;
            cplx acc = cmake(0.0, 0.0);
            #pragma unroll
            for (int d1 = 0; d1 < 9; ++d1) if (off9[d1] >= 0) cfma(acc, am9[d1], trow[off9[d1]]);
            v = csub(v, cmul(acc, ap));
        }
    }
    T[(long long)j * g.m + i] = v;
}

// packed right-hand side of plane k:  Y = [f_k] - A_{k,k-1} Zm - A_{k,k+1} Zp  (each neighbour optional; without f the sign is +:
// Y = A_{k,k-1} Zm + A_{k,k+1} Zp, the back-substitution term)
__global__ __launch_bounds__(256) void k_bt_rhs(const cplx *__restrict__ planes, BtGeom g, int k, const cplx *__restrict__ f, const cplx *__restrict__ Zm,
                                                const cplx *__restrict__ Zp, cplx *__restrict__ Y, int mpad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, r = blockIdx.y;
    if (i >= g.m) return;
    const int ia = i / g.nb, ib = i % g.nb;
    const long long node = (long long)k * g.ss + ia * g.sa + ib * g.sb;
    cplx v = cmake(0.0, 0.0);
    for (int side = 0; side < 2; ++side) {
        const cplx *Zn = side ? Zp : Zm;
        if (!Zn) continue;
        const cplx *zr = Zn + (long long)r * g.m;
        for (int d = 0; d < 9; ++d) {
            const int aa = ia + (d / 3 - 1), ab = ib + (d % 3 - 1);
            if (aa < 0 || aa >= g.na || ab < 0 || ab >= g.nb) continue;
            cfma(v, planes[(long long)bt_slot(g.axis, side ? 1 : -1, d / 3 - 1, d % 3 - 1) * g.N + node], zr[aa * g.nb + ab]);
        }
    }
    if (f) v = csub(f[(long long)r * g.N + node], v);
    Y[(long long)r * mpad + i] = v;
}

// parts[ks][r][c] = sum over the k rows of chunk ks of Y[r][k] T[k][c]   (r < 16 right-hand sides).
// The plane inverses are read once per solve and nothing else is: a memory-bound product (8 flop per byte at 16 right-hand sides).
// A workgroup takes 128 columns and one K chunk; every lane owns two columns (c, c + 64) so that one LDS broadcast of a right-hand-side
// value feeds two multiply-adds (with one column per lane the 16 broadcasts per row bound the kernel at 2.8 TB/s); wave w streams rows
// w, w + 4, ... of T (two coalesced 1-KB segments per row) and the four waves add their partial sums through LDS at the end.
#define BTA_KS 128
template <int NR>
__global__ __launch_bounds__(256, 2) void k_bt_apply(const cplx *__restrict__ Y, int ldy, const cplx *__restrict__ T, int m, int kc, int nrhs,
                                                     cplx *__restrict__ parts) {
    __shared__ cplx ys[BTA_KS][NR];                      // 32 KB; doubles as the reduction buffer (3 waves x 8 values x 64 lanes = 24 KB)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 128 + lane, c1 = c0 + 64;
    const int kbeg = blockIdx.y * kc, kend = min(m, kbeg + kc);
    cplx acc0[NR], acc1[NR];
    #pragma unroll
    for (int r = 0; r < NR; ++r) { acc0[r] = cmake(0.0, 0.0); acc1[r] = cmake(0.0, 0.0); }
    const bool live0 = c0 < m, live1 = c1 < m;
    for (int k0 = kbeg; k0 < kend; k0 += BTA_KS) {
        __syncthreads();
        for (int e = threadIdx.x; e < BTA_KS * NR; e += 256) {
            const int kk = e % BTA_KS, r = e / BTA_KS;
            ys[kk][r] = (r < nrhs && k0 + kk < kend) ? Y[(long long)r * ldy + k0 + kk] : cmake(0.0, 0.0);
        }
        __syncthreads();
        const int kn = min(BTA_KS, kend - k0);
        for (int kk = w; kk < kn; kk += 16) {            // four rows of this wave per step: eight 16-byte loads in flight per lane
            cplx t0[4], t1[4];
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = kk + 4 * u;
                const cplx *row = T + (long long)(k0 + k) * m;
                t0[u] = (live0 && k < kn) ? row[c0] : cmake(0.0, 0.0);
                t1[u] = (live1 && k < kn) ? row[c1] : cmake(0.0, 0.0);
            }
            #pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = min(kk + 4 * u, BTA_KS - 1);
                #pragma unroll
                for (int r = 0; r < NR; ++r) { const cplx y = ys[k][r]; cfma(acc0[r], y, t0[u]); cfma(acc1[r], y, t1[u]); }
            }
        }
    }
    // waves 1-3 hand their sums to wave 0, eight values per lane and round
    cplx *red = &ys[0][0];
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
        #pragma unroll
        for (int g = 0; g < NR; g += 8) {
            __syncthreads();
            if (w > 0) {
                #pragma unroll
                for (int r = 0; r < 8; ++r) red[((w - 1) * 8 + r) * 64 + lane] = half ? acc1[g + r] : acc0[g + r];
            }
            __syncthreads();
            if (w == 0) {
                #pragma unroll
                for (int r = 0; r < 8; ++r) {
                    cplx v = half ? acc1[g + r] : acc0[g + r];
                    #pragma unroll
                    for (int q = 0; q < 3; ++q) v = cadd(v, red[(q * 8 + r) * 64 + lane]);
                    if (half) acc1[g + r] = v; else acc0[g + r] = v;
                }
            }
        }
    }
    if (w != 0) return;
    cplx *out = parts + ((long long)blockIdx.y * nrhs) * m;
    #pragma unroll
    for (int r = 0; r < NR; ++r) if (r < nrhs) {
        if (live0) out[(long long)r * m + c0] = acc0[r];
        if (live1) out[(long long)r * m + c1] = acc1[r];
    }
}

// Single-precision variant: the plane inverses are stored as float2 (half the bytes, half the 17 GB) and the products run in fp32 --
// the cycle is a preconditioner, its coarse solve does not need more than ~1e-5.  A lane owns two ADJACENT columns (one 16-byte load).
template <int NR>
__global__ __launch_bounds__(256, 2) void k_bt_apply32(const cplx *__restrict__ Y, int ldy, const float2 *__restrict__ T, int m, int ld, int kc, int nrhs,
                                                       cplx *__restrict__ parts) {
    __shared__ float2 ys[BTA_KS][NR];                    // 16 KB; doubles as the reduction buffer (3 waves x 8 values x 64 lanes = 12 KB)
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c0 = blockIdx.x * 128 + 2 * lane, c1 = c0 + 1;
    const int kbeg = blockIdx.y * kc, kend = min(m, kbeg + kc);
    float2 acc0[NR], acc1[NR];
    #pragma unroll
    for (int r = 0; r < NR; ++r) { acc0[r] = make_float2(0.f, 0.f); acc1[r] = make_float2(0.f, 0.f); }
    const bool live0 = c0 < m, live1 = c1 < m;
    for (int k0 = kbeg; k0 < kend; k0 += BTA_KS) {
        __syncthreads();
        for (int e = threadIdx.x; e < BTA_KS * NR; e += 256) {
            const int kk = e % BTA_KS, r = e / BTA_KS;
            const cplx v = (r < nrhs && k0 + kk < kend) ? Y[(long long)r * ldy + k0 + kk] : cmake(0.0, 0.0);
            ys[kk][r] = make_float2((float)v.x, (float)v.y);
        }
        __syncthreads();
        const int kn = min(BTA_KS, kend - k0);
        for (int kk = w; kk < kn; kk += 32) {            // eight rows of this wave per step
            float4 t[8];
            #pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = kk + 4 * u;
                t[u] = (live0 && k < kn) ? *reinterpret_cast<const float4 *>(T + (long long)(k0 + k) * ld + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            #pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int k = min(kk + 4 * u, BTA_KS - 1);
                #pragma unroll
                for (int r = 0; r < NR; ++r) {
                    const float2 y = ys[k][r];
                    acc0[r].x = fmaf(y.x, t[u].x, acc0[r].x); acc0[r].x = fmaf(-y.y, t[u].y, acc0[r].x);
                    acc0[r].y = fmaf(y.x, t[u].y, acc0[r].y); acc0[r].y = fmaf(y.y, t[u].x, acc0[r].y);
                    acc1[r].x = fmaf(y.x, t[u].z, acc1[r].x); acc1[r].x = fmaf(-y.y, t[u].w, acc1[r].x);
                    acc1[r].y = fmaf(y.x, t[u].w, acc1[r].y); acc1[r].y = fmaf(y.y, t[u].z, acc1[r].y);
                }
            }
        }
    }
    float2 *red = &ys[0][0];
    #pragma unroll
    for (int half = 0; half < 2; ++half) {
        #pragma unroll
        for (int g = 0; g < NR; g += 8) {
            __syncthreads();
            if (w > 0) {
                #pragma unroll
                for (int r = 0; r < 8; ++r) red[((w - 1) * 8 + r) * 64 + lane] = half ? acc1[g + r] : acc0[g + r];
            }
            __syncthreads();
            if (w == 0) {
                #pragma unroll
                for (int r = 0; r < 8; ++r) {
                    float2 v = half ? acc1[g + r] : acc0[g + r];
                    #pragma unroll
                    for (int q = 0; q < 3; ++q) { const float2 o = red[(q * 8 + r) * 64 + lane]; v.x += o.x; v.y += o.y; }
                    if (half) acc1[g + r] = v; else acc0[g + r] = v;
                }
            }
        }
    }
    if (w != 0) return;
    cplx *out = parts + ((long long)blockIdx.y * nrhs) * m;
    #pragma unroll
    for (int r = 0; r < NR; ++r) if (r < nrhs) {
        if (live0) out[(long long)r * m + c0] = cmake((double)acc0[r].x, (double)acc0[r].y);
        if (live1) out[(long long)r * m + c1] = cmake((double)acc1[r].x, (double)acc1[r].y);
    }
}

__global__ void k_bt_to_f32(const cplx *__restrict__ T, float2 *__restrict__ T32, int m, int ld) {
    const long long n = (long long)m * ld;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(e / ld), c = (int)(e % ld);
        const cplx v = c < m ? T[(long long)r * m + c] : cmake(0.0, 0.0);
        T32[e] = make_float2((float)v.x, (float)v.y);
    }
}

// Z (+)= sum of the split-K partial products: sub = 0: Z = sum, 1: Z -= sum
__global__ void k_bt_reduce(const cplx *__restrict__ parts, int nparts, long long n, cplx *__restrict__ Z, int sub) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        cplx s = parts[e];
        for (int p = 1; p < nparts; ++p) s = cadd(s, parts[(long long)p * n + e]);
        Z[e] = sub ? csub(Z[e], s) : s;
    }
}

__global__ void k_bt_scatter(const cplx *__restrict__ Z, BtGeom g, int nrhs, cplx *__restrict__ u) {
    const long long tot = (long long)g.np * g.m;
    const int r = blockIdx.y;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const int k = (int)(e / g.m), i = (int)(e % g.m);
        const long long node = (long long)k * g.ss + (i / g.nb) * g.sa + (i % g.nb) * g.sb;
        u[(long long)r * g.N + node] = Z[((long long)k * nrhs + r) * g.m + i];
    }
}

BtGeom bt_geom(const Bt3 &B) { BtGeom g; g.axis = B.axis; g.np = B.np; g.na = B.na; g.nb = B.nb; g.m = B.m; g.ss = B.ss; g.sa = B.sa; g.sb = B.sb; g.N = B.N; return g; }

void bt_free(Bt3 &B) {
    if (B.Tinv) helm_pool_free(B.device, B.Tinv, B.tbytes);
    if (B.Tinv32) helm_pool_free(B.device, B.Tinv32, B.tbytes32);
    for (int c = 0; c < 2; ++c) { hipFree(B.Y[c]); hipFree(B.parts[c]); }
    hipFree(B.Z);
    for (int e = 0; e < 3; ++e) if (B.ev[e]) hipEventDestroy(B.ev[e]);
    if (B.aux) helm_destroy(B.aux);
    B = Bt3();
}

// Twisted block elimination: the planes left of `mid` are eliminated left to right, those right of it right to left, plane mid last.
// The two chains are independent, so they run on two streams (set-up: two dense inversions in flight, whose latency-bound pivot and
// panel steps fill each other's gaps; solve: two half-length chains of small launches).
int bt_setup(helm_op *op, Bt3 &B, const Mg3Level &L, int batch, const helm_tuning &tune) {
    const int dims[3] = {L.nz, L.ny, L.nx};
    const long long strides[3] = {(long long)L.ny * L.nx, L.nx, 1};
    static_cast<BtShape &>(B) = mg3_bt_shape(dims, batch, tune);
    const int axis = B.axis, ia = axis == 0 ? 1 : 0, ib = axis == 2 ? 1 : 2;
    B.na = dims[ia]; B.nb = dims[ib];
    B.ss = strides[axis]; B.sa = strides[ia]; B.sb = strides[ib]; B.N = L.N; B.batch = batch;
    B.mid = tune.mg3_bt_twist ? B.np / 2 : B.np - 1;
    B.nparts = B.ksplit; B.device = op->device;
    const long long mm = (long long)B.m * B.m;
    const size_t wbytes = B.wbytes, tb = B.tbytes;
    {   // leave room for the Krylov workspace: the plane inverses may take a third of the device memory
        size_t totb = 0;
        const size_t freeb = mg3_available_bytes(op->device, &totb);
        const double cap = std::min(totb / 3.0, 0.95 * (double)freeb);     // (free memory: several 3-D handles may be alive)
        if ((double)(tb + B.tbytes32) > cap)
            HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "3-D multigrid: the plane inverses of the directly solved level (%.1f GB) exceed the budget of %.1f GB", (tb + B.tbytes32) / 1e9, cap / 1e9);
    }
    hipStreamSynchronize(op->stream);          // (buffers of the previous frequency go back to the pool only when their work is done)
    B.aux = helm_create3d(op->device, 3, 3, 3, 1.0, 1.0, 1.0, 2);
    if (!B.aux) HELM_FAIL(op, HELM_ERR_DEVICE, "%s", helm_last_error(nullptr));
    // set-up: two inversions in flight pay while they are latency-bound (m = 1617 at 2 Hz: 0.37 -> 0.30 s); two saturating ones only get in each
    // other's way (m = 3713: 1.49 -> 1.93 s), so from the size at which the look-ahead Gauss-Jordan takes over both chains share one stream
    const bool conc = B.m < 2048;
    hipStream_t sts[2] = {op->stream, conc ? B.aux->stream : op->stream};
    helm_op *ctx[2] = {op, conc ? B.aux : op};
    B.Tinv = (cplx *)helm_pool_alloc(op->device, tb);
    if (B.f32) B.Tinv32 = (float2 *)helm_pool_alloc(op->device, B.tbytes32);
    cplx *W[2] = {(cplx *)helm_pool_alloc(op->device, wbytes), (cplx *)helm_pool_alloc(op->device, wbytes)};
    bool ok = B.Tinv && W[0] && W[1] && (!B.f32 || B.Tinv32) && helm_malloc_retry(op->device, (void **)&B.Z, (size_t)B.np * batch * B.m * sizeof(cplx)) == hipSuccess;
    for (int c = 0; c < 2 && ok; ++c)
        ok = helm_malloc_retry(op->device, (void **)&B.Y[c], (size_t)batch * B.mpad * sizeof(cplx)) == hipSuccess &&
             helm_malloc_retry(op->device, (void **)&B.parts[c], (size_t)B.nparts * batch * B.m * sizeof(cplx)) == hipSuccess;
    for (int e = 0; e < 3 && ok; ++e) ok = hipEventCreateWithFlags(&B.ev[e], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        for (int c = 0; c < 2; ++c) if (W[c]) helm_pool_free(op->device, W[c], wbytes);
        bt_free(B);
        HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: the plane inverses of the coarsest level (%.1f GB) do not fit", (tb + B.tbytes32) / 1e9);
    }
    if (!B.f32 && B.mpad != B.m) hipMemsetAsync(B.Tinv, 0, tb, op->stream);
    for (int c = 0; c < 2; ++c) hipMemsetAsync(B.Y[c], 0, (size_t)batch * B.mpad * sizeof(cplx), op->stream);
    hipEventRecord(B.ev[0], op->stream);
    hipStreamWaitEvent(sts[1], B.ev[0], 0);
    const BtGeom g = bt_geom(B);
    const cplx *planes = L.op->d_C;
    const unsigned sg = (unsigned)((mm + 255) / 256);
    // where the (transposed, double-precision) Schur complement of plane k lives: its own slot, or a ping-pong pair per chain (f32)
    auto slot = [&](int chain, int step, int k) { return B.f32 ? B.Tinv + ((long long)chain * 2 + (step & 1)) * mm : B.Tinv + (long long)k * B.mpad * B.m; };
    auto finish = [&](int chain, cplx *Tk, int k) -> int {
        const int rc = nd_dense_inverse(ctx[chain], Tk, B.m, W[chain]);
        if (rc) { helm_set_error(op, helm_last_error(ctx[chain])); return rc; }
        if (B.f32) HELM_LAUNCH(k_bt_to_f32, dim3(4096), dim3(256), 0, sts[chain], (const cplx *)Tk, B.Tinv32 + (long long)k * B.m * B.ld32, B.m, B.ld32);
        return HELM_OK;
    };
    int rc = HELM_OK;
    const int nl = B.mid, nr = B.np - 1 - B.mid;
    const cplx *lastL = nullptr, *lastR = nullptr;
    for (int step = 0; step < std::max(nl, nr) && !rc; ++step) {        // launches of the two chains interleaved
        if (step < nl) {
            const int k = step;
            cplx *Tk = slot(0, step, k);
            HELM_LAUNCH(k_bt_schur_t, dim3(sg), dim3(256), 0, sts[0], planes, g, k, lastL, (const cplx *)nullptr, Tk);
            rc = finish(0, Tk, k); lastL = Tk;
        }
        if (step < nr && !rc) {
            const int k = B.np - 1 - step;
            cplx *Tk = slot(1, step, k);
            HELM_LAUNCH(k_bt_schur_t, dim3(sg), dim3(256), 0, sts[1], planes, g, k, (const cplx *)nullptr, lastR, Tk);
            rc = finish(1, Tk, k); lastR = Tk;
        }
    }
    if (!rc) {                                                           // the plane where the chains meet
        hipEventRecord(B.ev[1], sts[1]);
        hipStreamWaitEvent(sts[0], B.ev[1], 0);
        cplx *Tk = slot(0, nl, B.mid);
        HELM_LAUNCH(k_bt_schur_t, dim3(sg), dim3(256), 0, sts[0], planes, g, B.mid, lastL, lastR, Tk);
        rc = finish(0, Tk, B.mid);
    }
    hipStreamSynchronize(sts[1]);
    hipStreamSynchronize(sts[0]);
    for (int c = 0; c < 2; ++c) helm_pool_free(op->device, W[c], wbytes);
    if (B.f32 && B.Tinv) { helm_pool_free(op->device, B.Tinv, B.tbytes); B.Tinv = nullptr; }
    if (rc) { bt_free(B); return rc; }
    return HELM_OK;
}

void nd3_free(Nd3 &D) { if (D.ws) helm_pool_free(D.device, D.ws, D.ws_bytes); if (D.f) nd_free(D.f); D = Nd3(); }

bool nd3_applicable(int nz, int ny, int nx) { return nz >= 3 && nz < 128 && ny >= 3 && nx >= 3 && ny < 4096 && nx < 4096; }

}  // namespace

// (host side: the plan only; cached, the plan of a 79 x 79 grid has 2000 fronts)
Nd3Cost mg3_nd_cost(int nz, int ny, int nx, int leaf) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int, int>, Nd3Cost> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_tuple(nz, ny, nx, leaf);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    NdPlan P;
    nd_build_plan(P, ny, nx, leaf, nz);
    Nd3Cost c;
    for (const NdGroup &g : P.groups) {
        c.flops += (double)g.cnt * 8.0 * (2.0 * g.smax * g.smax * g.smax + (double)g.smax * g.smax * g.mmax + (double)g.smax * g.mmax * g.mmax);
        c.top = std::max(c.top, g.smax);
    }
    c.fac_bytes = (double)P.fac_elems * sizeof(cplx);
    c.ws_bytes = (double)nd_factor_ws_elems(P) * sizeof(cplx);
    cache[key] = c;
    return c;
}

// Which direct solver the level gets.  helm_tuning.mg3_coarse forces one; otherwise the column dissection wherever it applies and needs fewer
// flops than the plane-by-plane elimination (np inversions of m^3): on config 5's 47 x 79 x 79 level 10.5 against 32.6 TFLOP.
bool mg3_coarse_is_nd(int nz, int ny, int nx, const helm_tuning &tune) {
    if (tune.mg3_coarse == 2 || !nd3_applicable(nz, ny, nx)) return false;
    if (tune.mg3_coarse == 1) return true;
    const int d[3] = {nz, ny, nx};
    const BtShape S = mg3_bt_shape(d, 1, tune);          // (np and m do not depend on the batch)
    const double m = S.m;
    return mg3_nd_cost(nz, ny, nx, tune.mg3_nd_leaf).flops < (double)S.np * 8.0 * m * m * m;
}

namespace {

int nd3_setup(helm_op *op, Nd3 &D, const Mg3Level &L, int batch, int leaf) {
    if (!nd3_applicable(L.nz, L.ny, L.nx)) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "3-D multigrid: the column dissection takes levels with fewer than 128 layers");
    D.device = op->device; D.batch = batch;
    int rc = nd_get_plan_dims(op, L.ny, L.nx, leaf, L.nz, &D.pd);
    if (rc) return rc;
    const NdPlan &P = D.pd->plan;
    const size_t fwb = (size_t)nd_factor_ws_elems(P) * sizeof(cplx);
    D.ws_bytes = (size_t)nd_solve_ws_elems(P, batch) * sizeof(cplx);
    {
        const size_t freeb = mg3_available_bytes(op->device, nullptr);
        const double need = (double)P.fac_elems * sizeof(cplx) + (double)fwb + (double)D.ws_bytes;
        if (need > 0.9 * (double)freeb) HELM_FAIL(op, HELM_ERR_UNSUPPORTED, "3-D multigrid: the factors of the directly solved level (%.1f GB) do not fit", need / 1e9);
    }
    hipStreamSynchronize(op->stream);
    D.f = new NdFactor();
    D.f->pd = D.pd;
    cplx *fw = (cplx *)helm_pool_alloc(op->device, fwb);
    D.ws = (cplx *)helm_pool_alloc(op->device, D.ws_bytes);
    if (!fw || !D.ws) { if (fw) helm_pool_free(op->device, fw, fwb); nd3_free(D); HELM_FAIL(op, HELM_ERR_DEVICE, "3-D multigrid: scratch of the column dissection does not fit"); }
    rc = nd_factor(op, 0, D.f, fw, L.op->d_C);
    helm_pool_free(op->device, fw, fwb);
    if (rc) { nd3_free(D); return rc; }
    if (mg3_trace())
        fprintf(stderr, "[helm mg3] column dissection of the %d x %d x %d level: %zu fronts, factors %.2f GB, %.2f TFLOP\n", L.nz, L.ny, L.nx, P.nodes.size(),
                P.fac_elems * 16e-9, D.f->flops * 1e-12);
    return HELM_OK;
}

// u = A^-1 f on the coarsest level (f, u: [nrhs][N])
int bt_solve(helm_op *op, Bt3 &B, const Mg3Level &L, const cplx *f, cplx *u, int nrhs) {
    hipStream_t sts[2] = {op->stream, B.aux->stream};
    const BtGeom g = bt_geom(B);
    const cplx *planes = L.op->d_C;
    const dim3 rg((B.m + 255) / 256, nrhs);
    const long long pz = (long long)nrhs * B.m;              // one packed plane of Z
    const unsigned redg = (unsigned)std::min<long long>((pz + 255) / 256, 4096);
    // Z_k (-)= Y S_k^-T on the stream of `chain`
    auto apply_inverse = [&](int chain, int k, int sub) -> int {
        hipStream_t st = sts[chain];
        cplx *Zk = B.Z + k * pz;
        if (B.f32) {
            HELM_LAUNCH(k_bt_apply32<16>, dim3((B.m + 127) / 128, B.ksplit), dim3(256), 0, st, (const cplx *)B.Y[chain], B.mpad,
                               (const float2 *)(B.Tinv32 + (long long)k * B.m * B.ld32), B.m, B.ld32, B.kc, nrhs, B.parts[chain]);
            HELM_LAUNCH(k_bt_reduce, dim3(redg), dim3(256), 0, st, (const cplx *)B.parts[chain], B.nparts, pz, Zk, sub);
            return HELM_OK;
        }
        const cplx *Tk = B.Tinv + (long long)k * B.mpad * B.m;
        if (B.own) {
            HELM_LAUNCH(k_bt_apply<16>, dim3((B.m + 127) / 128, B.ksplit), dim3(256), 0, st, (const cplx *)B.Y[chain], B.mpad, Tk, B.m, B.kc, nrhs, B.parts[chain]);
            HELM_LAUNCH(k_bt_reduce, dim3(redg), dim3(256), 0, st, (const cplx *)B.parts[chain], B.nparts, pz, Zk, sub);
            return HELM_OK;
        }
        // generic batched GEMM (more than 16 right-hand sides): it launches on the handle's own stream, so this path keeps to one chain order
        const int rc = nd_dense_gemm_batched(chain ? B.aux : op, nrhs, B.m, B.kc, cmake(1, 0), B.Y[chain], B.mpad, B.kc, Tk, B.m, (long long)B.kc * B.m, cmake(0, 0),
                                             B.parts[chain], B.m, pz, B.ksplit);
        if (rc) return rc;
        HELM_LAUNCH(k_bt_reduce, dim3(redg), dim3(256), 0, st, (const cplx *)B.parts[chain], B.ksplit, pz, Zk, sub);
        return HELM_OK;
    };
    auto rhs = [&](int chain, int k, const cplx *fk, const cplx *Zm, const cplx *Zp) {
        HELM_LAUNCH(k_bt_rhs, rg, dim3(256), 0, sts[chain], planes, g, k, fk, Zm, Zp, B.Y[chain], B.mpad);
    };
    const int nl = B.mid, nr = B.np - 1 - B.mid;
    int rc = HELM_OK;
    hipEventRecord(B.ev[0], sts[0]);                       // f is ready
    hipStreamWaitEvent(sts[1], B.ev[0], 0);
    for (int step = 0; step < std::max(nl, nr); ++step) {  // forward: z_k = S_k^-1 (f_k - A_{k,k-+1} z_{k-+1}), both chains
        if (step < nl) { const int k = step; rhs(0, k, f, k ? B.Z + (k - 1) * pz : nullptr, nullptr); rc = apply_inverse(0, k, 0); if (rc) return rc; }
        if (step < nr) { const int k = B.np - 1 - step; rhs(1, k, f, nullptr, step ? B.Z + (k + 1) * pz : nullptr); rc = apply_inverse(1, k, 0); if (rc) return rc; }
    }
    hipEventRecord(B.ev[1], sts[1]);
    hipStreamWaitEvent(sts[0], B.ev[1], 0);
    rhs(0, B.mid, f, nl ? B.Z + (B.mid - 1) * pz : nullptr, nr ? B.Z + (B.mid + 1) * pz : nullptr);     // the plane where the chains meet: x_mid
    rc = apply_inverse(0, B.mid, 0); if (rc) return rc;
    hipEventRecord(B.ev[2], sts[0]);
    hipStreamWaitEvent(sts[1], B.ev[2], 0);
    for (int step = 0; step < std::max(nl, nr); ++step) {  // back substitution outwards: x_k = z_k - S_k^-1 A_{k,k+-1} x_{k+-1}
        if (step < nl) { const int k = B.mid - 1 - step; rhs(0, k, nullptr, nullptr, B.Z + (k + 1) * pz); rc = apply_inverse(0, k, 1); if (rc) return rc; }
        if (step < nr) { const int k = B.mid + 1 + step; rhs(1, k, nullptr, B.Z + (k - 1) * pz, nullptr); rc = apply_inverse(1, k, 1); if (rc) return rc; }
    }
    hipEventRecord(B.ev[1], sts[1]);
    hipStreamWaitEvent(sts[0], B.ev[1], 0);
    HELM_LAUNCH(k_bt_scatter, dim3((unsigned)std::min<long long>(((long long)B.np * B.m + 255) / 256, 4096), nrhs), dim3(256), 0, sts[0],
                       (const cplx *)B.Z, g, nrhs, u);
    return HELM_OK;
}

}  // namespace

int mg3_coarse_setup(helm_op *op, Mg3Keep *K, const Mg3Level &L, int batch, const helm_tuning &tune) {
    const int rc = mg3_coarse_is_nd(L.nz, L.ny, L.nx, tune) ? nd3_setup(op, K->nd, L, batch, tune.mg3_nd_leaf) : HELM_ERR_UNSUPPORTED;
    return rc == HELM_ERR_UNSUPPORTED ? bt_setup(op, K->bt, L, batch, tune) : rc;      // (also when the dissection's factors do not fit: the plane inverses are single precision)
}
int mg3_coarse_solve(helm_op *op, Mg3Keep *K, const Mg3Level &L, const cplx *f, cplx *u, int nrhs) {
    return K->nd.on() ? nd_solve(op, K->nd.f, f, u, nrhs, K->nd.ws) : bt_solve(op, K->bt, L, f, u, nrhs);
}
void mg3_coarse_free(Mg3Keep *K) { bt_free(K->bt); nd3_free(K->nd); }
