// Direct solver: the one-wave Gauss-Jordan sweep of a block of at most 32 x 32 held in registers, shared by the batched inverse (nd_gj.hip:
// k_gj32w_inverse) and the fused factorisation of the small separator levels (nd_leaf.hip: k_sep_factor_small).
#pragma once
#include "nd_internal.hpp"

__device__ __forceinline__ double gj_rcp(double x) {
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    return fma(fma(-x, y, 1.0), y, y);
}
__device__ __forceinline__ unsigned gj_key(cplx v, int i) {
    const float m = (float)fmax(fabs(v.x), fabs(v.y));
    return (__float_as_uint(m) & ~31u) | (unsigned)i;
}
__device__ __forceinline__ cplx gj_recip(cplx d) {
    const double rr = gj_rcp(d.x * d.x + d.y * d.y);
    return cmake(d.x * rr, -d.y * rr);
}

// ---- throughput variant for thousands of small blocks: one WAVE per matrix, the matrix in registers -------------------------------
// Lane l holds half a row: row r = l & 31, columns 16 h .. 16 h + 15 with h = l >> 5 (16 complex = 64 VGPRs).  The 32 elimination steps
// are unrolled so that every register index is static.  Per step the wave exchanges three things through its own 1.5 KB of LDS (LDS
// operations of one wave execute in order, no barrier): the pivot keys of column k, the pivot row (written by its two owner lanes, read
// as broadcasts), and the multipliers a[r][k] for the half that does not hold column k.  Pivoting is implicit -- rows stay where they
// are, sigma(k) records the pivot row of step k -- and is undone when the result is stored: inv[i][sigma(k)] = R[sigma(i)][k].
// ~220 wave-instructions per step against ~840 for the four-wave kernel above: the leaf level's two launches of 16 384 blocks are
// issue-bound, so this is what they cost.
struct Gj32w {
    cplx prow[32];
    cplx fcol[32];
    unsigned cand[32];
    int sigma[32];       // pivot row of step k
    int sinv[32];        // step at which row r was the pivot
};
// the elimination itself: lane (r, h) holds a[c] = entry (r, 16 h + c) of the block padded with the identity; on return the storage rows of the inverse
// (see k_gj32w_inverse for the permutation that undoes the implicit pivoting)
__device__ __forceinline__ void gj32w_core(cplx (&a)[16], Gj32w &S, int n, int r, int h) {
    bool used = r >= n;                            // padding rows never pivot
    if (h == 0) { S.sigma[r] = r; S.sinv[r] = r; }  // (a singular block may leave entries unset: keep every index in range)
    // The pivot row is NOT scaled when it is chosen: the other rows are eliminated with the multiplier f / d against the unscaled row,
    // and the factor 1 / d of the pivot row rides along in `srow` until the end (every later operation on that row is linear in it).
    // That leaves 16 complex multiply-adds per lane and step -- scaling the row at once would double the fp64 work of a step.
    cplx srow = cmake(1.0, 0.0);
    #pragma unroll
    for (int k = 0; k < 32; ++k) {
        if (k < n) {
            const int kc = k & 15, kh = k >> 4;
            // pivot keys and multipliers of column k, from the half that holds it (candidates are unused rows: their scale is still 1)
            if (h == kh) {
                S.cand[r] = used ? (unsigned)r : gj_key(a[kc], r);
                S.fcol[r] = a[kc];
            }
            __builtin_amdgcn_wave_barrier();
            const uint4 *c4 = reinterpret_cast<const uint4 *>(S.cand);
            unsigned m = 0;
            #pragma unroll
            for (int q = 0; q < 8; ++q) { const uint4 v = c4[q]; m = max(m, max(max(v.x, v.y), max(v.z, v.w))); }
            const int p = (int)(m & 31u);
            const cplx f = S.fcol[r];
            __builtin_amdgcn_wave_barrier();
            // the pivot row, written by its two owner lanes
            if (r == p) {
                #pragma unroll
                for (int c = 0; c < 16; ++c) S.prow[16 * h + c] = a[c];
                if (h == 0) { S.sigma[k] = p; S.sinv[p] = k; }
                used = true;
            }
            __builtin_amdgcn_wave_barrier();
            const cplx d = S.prow[k];
            const double rr = gj_rcp(d.x * d.x + d.y * d.y);
            const cplx dinv = cmake(d.x * rr, -d.y * rr);
            const cplx fp = (r == p) ? cmake(0.0, 0.0) : cmul(f, dinv);
            #pragma unroll
            for (int c = 0; c < 16; ++c) {
                const cplx pr = S.prow[16 * h + c];
                a[c].x = fma(-fp.x, pr.x, a[c].x); a[c].x = fma(fp.y, pr.y, a[c].x);
                a[c].y = fma(-fp.x, pr.y, a[c].y); a[c].y = fma(-fp.y, pr.x, a[c].y);
            }
            if (h == kh) a[kc] = (r == p) ? cmake(1.0, 0.0) : cneg(fp);        // column k of the running inverse
            if (r == p) srow = dinv;
            __builtin_amdgcn_wave_barrier();
        }
    }
    #pragma unroll
    for (int c = 0; c < 16; ++c) a[c] = cmul(a[c], srow);
}
