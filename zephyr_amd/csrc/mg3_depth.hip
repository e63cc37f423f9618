// How many layer-preserving coarsenings a 3-D hierarchy gets (mg3_choose_depth, asked by mg3_setup): the 10-points rule, the memory budget of the
// direct solver of the last level, and a cost model that trades set-up seconds (timed on this device) against the extra iterations of a deeper
// hierarchy (booked by the solves of this process).  DESIGN.md section 6 has the measurements.
#include "mg3_internal.hpp"
#include "solve_internal.hpp"
#include <map>
#include <tuple>
#include <mutex>

// ---- what the layer-preserving cycle has actually needed: iterations per right-hand side, by class -----------------------------------------
// The depth decision (mg3_choose_depth) trades set-up seconds against extra iterations of the deeper hierarchy.  Round 3 priced those with three
// constants measured on config 5 (+11 / +22 / +38 at >= 8 / 6 / 5 points per wavelength on the direct level).  Now every solve through a
// layer-preserving hierarchy books its mean iteration count under (grid, coarsenings, points per wavelength of the direct level to the nearest
// 0.5, log10 rtol), and the decision uses the booked counts of both candidates where it has them; the constants remain only as the prior for a
// class that has never run in this process (the first frequency of the first job).
namespace {
struct ItKey { int nz, ny, nx, depth, ppw2, ltol; bool operator<(const ItKey &o) const { return std::tie(nz, ny, nx, depth, ppw2, ltol) < std::tie(o.nz, o.ny, o.nx, o.depth, o.ppw2, o.ltol); } };
std::mutex g_its_mu;
std::map<ItKey, std::pair<double, int>> &g_its = *new std::map<ItKey, std::pair<double, int>>();     // key -> (sum of mean iterations, solves)
ItKey it_key(const helm_op *op, int depth, double ppwd, double rtol) {
    return ItKey{op->nz, op->ny, op->nx, depth, (int)std::lround(2.0 * ppwd), (int)std::lround(-std::log10(std::max(rtol, 1e-16)))};
}
// mean iterations booked for the class, < 0 when it has never run
double its_lookup(const helm_op *op, int depth, double ppwd, double rtol) {
    std::lock_guard<std::mutex> lk(g_its_mu);
    auto it = g_its.find(it_key(op, depth, ppwd, rtol));
    return it == g_its.end() || it->second.second == 0 ? -1.0 : it->second.first / it->second.second;
}
// The tolerance class a set-up looks its iteration counts up under: the handle's stated tolerance (helm_set_tolerance_hint, or a solve on it), else --
// a C caller that prefactors a fresh handle without stating one -- the tolerance of the last solve booked on this grid in the process, so that
// what was recorded under the solves' real rtol is found again instead of the prior constants being used silently.
std::map<std::tuple<int, int, int>, double> &g_last_rtol = *new std::map<std::tuple<int, int, int>, double>();       // (g_its_mu held)
double lookup_rtol(const helm_op *op) {
    if (op->rtol_hint_set) return op->rtol_hint;
    std::lock_guard<std::mutex> lk(g_its_mu);
    auto it = g_last_rtol.find(std::make_tuple(op->nz, op->ny, op->nx));
    return it == g_last_rtol.end() ? op->rtol_hint : it->second;
}
}
void mg3_record_iterations(helm_op *op, double mean_iterations, double rtol) {
    if (!op || !op->mg3 || !op->mg3->keep || !(mean_iterations > 0)) return;
    std::lock_guard<std::mutex> lk(g_its_mu);
    g_last_rtol[std::make_tuple(op->nz, op->ny, op->nx)] = rtol;
    std::pair<double, int> &e = g_its[it_key(op, op->mg3->kept_levels, op->mg3->ppw_direct, rtol)];
    e.first += mean_iterations; e.second += 1;
}

namespace {
// ---- what the depth decision is made from: timed on this device at set-up, once per process and size class ---------------------------------
__global__ void k3_cal_fill(cplx *A, int n) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < (long long)n * n; e += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(e / n), j = (int)(e % n);
        const unsigned h = (unsigned)(i * 2654435761u) ^ (unsigned)(j * 40503u);
        A[e] = i == j ? cmake(4.0, 1.0) : cmake(((h & 1023) / 1024.0 - 0.5) / n, (((h >> 10) & 1023) / 1024.0 - 0.5) / n);
    }
}
std::mutex g_cal_mu;
std::map<std::pair<int, int>, double> g_cal_inverse;       // (device, size) -> seconds of one dense inversion
// seconds the second of two runs of `run` takes on the handle's stream (`prep`, ahead of each, is not timed); < 0: could not be timed
template <class Prep, class Run> double second_run_seconds(helm_op *op, Prep prep, Run run) {
    double t = -1.0;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess) {
        prep(); int rc = run();
        prep(); hipEventRecord(e0, op->stream);
        if (!rc) rc = run();
        hipEventRecord(e1, op->stream);
        float ms = 0.f;
        if (!rc && hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess && ms > 0) t = ms * 1e-3;
    }
    if (e0) hipEventDestroy(e0); if (e1) hipEventDestroy(e1);
    hipStreamSynchronize(op->stream);
    return t;
}
// seconds the dense blocked Gauss-Jordan takes for one m x m plane: timed on a synthetic matrix of min(m, 4096) rows, scaled with the cube of
// the size above that (the rate still rises a little there, so large planes are over- rather than under-estimated)
double inverse_seconds_class(helm_op *op, int m) {
    const int mc = std::max(32, std::min(m, 4096));
    double t = -1.0;
    {
        std::lock_guard<std::mutex> lk(g_cal_mu);
        auto it = g_cal_inverse.find(std::make_pair(op->device, mc));
        if (it != g_cal_inverse.end()) t = it->second;
    }
    if (t < 0) {
        const size_t mb = (size_t)mc * mc * sizeof(cplx);
        cplx *A = (cplx *)helm_pool_alloc(op->device, mb), *W = (cplx *)helm_pool_alloc(op->device, mb);
        if (A && W) t = second_run_seconds(op, [&] { HELM_LAUNCH(k3_cal_fill, dim3(1024), dim3(256), 0, op->stream, A, mc); }, [&] { return nd_dense_inverse(op, A, mc, W); });
        helm_pool_free(op->device, A, mb); helm_pool_free(op->device, W, mb);
        if (t < 0) t = 8.0 * mc * (double)mc * mc / 20e12;             // (could not time it: a nominal rate)
        std::lock_guard<std::mutex> lk(g_cal_mu);
        g_cal_inverse[std::make_pair(op->device, mc)] = t;
    }
    const double r = (double)m / mc;
    return t * r * r * r;
}
// All size classes are timed the first time any of them is asked for -- the first set-up of the process, before anything else runs on the GPU:
// a dispatcher later builds the next frequency's preconditioner BESIDE the current frequency's iterations, and a timing taken there would
// measure the sharing (set-ups that look slow send the depth decision one level deeper than it should go).
double inverse_seconds(helm_op *op, int m) {
    static const int classes[5] = {256, 512, 1024, 2048, 4096};
    {
        bool have = false;
        { std::lock_guard<std::mutex> lk(g_cal_mu); have = g_cal_inverse.count(std::make_pair(op->device, 4096)) != 0; }
        if (!have) for (int c : classes) (void)inverse_seconds_class(op, c);
    }
    int mc = 4096;
    for (int c : classes) if (m <= c) { mc = c; break; }
    const double t = inverse_seconds_class(op, mc);
    const double r = (double)m / mc;
    return t * r * r * r;
}
// seconds one fine-grid 27-point apply takes per right-hand side at the batch width of this call (the unit an iteration is priced in)
double apply_seconds_per_rhs(helm_op *op, int batch) {
    const int nb = std::max(1, std::min(batch, 16));
    const size_t vb = (size_t)nb * op->N * sizeof(cplx);
    cplx *X = (cplx *)helm_pool_alloc(op->device, vb), *Y = (cplx *)helm_pool_alloc(op->device, vb);
    double t = -1.0;
    if (X && Y) {
        hipMemsetAsync(X, 0, vb, op->stream);
        ApplyArgs a = ApplyArgs();
        a.planes = op->d_C; a.X = X; a.Y = Y; a.ld = op->N; a.nrhs = nb; a.epi = EPI_NONE; a.profile = 0;
        t = second_run_seconds(op, [] {}, [&] { return helm_launch_apply(op, a); }) / nb;
    }
    helm_pool_free(op->device, X, vb); helm_pool_free(op->device, Y, vb);
    if (t < 0) t = (double)op->N * (32.0 + 432.0 / nb) / 3.5e12;       // (could not time it: a nominal streaming rate)
    return t;
}

// memory and set-up time of the direct solver of level l, whichever kind it gets (coarse_is_nd): the plane-by-plane elimination is np timed
// inversions; the column dissection is priced at its flop count over the rate of a timed inversion of its top separator's size (its big
// fronts run the same blocked Gauss-Jordan and the same tile kernel: 10.5 TFLOP in 0.42 s on config 5 = the 25 TFLOP/s of the 3713^2 inversion)
struct CoarseEst { bool nd = false; double bytes = 0, seconds = 0; int np = 0, m = 0; };
CoarseEst coarse_estimate(helm_op *op, int l, int batch, bool timed, const helm_tuning &tune) {
    CoarseEst e;
    int d[3]; mg3_keep_level_dims(op, l, d);
    e.nd = mg3_coarse_is_nd(d[0], d[1], d[2], tune);
    if (e.nd) {
        const Nd3Cost c = mg3_nd_cost(d[0], d[1], d[2], tune.mg3_nd_leaf);
        e.bytes = c.fac_bytes + c.ws_bytes;
        if (timed) { const int mt = std::max(64, c.top); e.seconds = c.flops / (8.0 * mt * (double)mt * mt / inverse_seconds(op, mt)); }
        e.np = 1; e.m = c.top;
    } else {
        const BtShape S = mg3_bt_shape(d, batch, tune);
        e.bytes = (double)S.tbytes + (double)S.tbytes32; e.np = S.np; e.m = S.m;
        if (timed) e.seconds = e.np * inverse_seconds(op, e.m);
    }
    return e;
}

}  // namespace

// Oversampled grids get the layer-preserving hierarchy with a direct solve where the interior still has >= 10 points per wavelength; 0: the
// standard cycle (no level can be dropped).  ppw: points per wavelength of the fine grid.
int mg3_choose_depth(helm_op *op, int batch, double ppw, const helm_tuning &tune) {
    const double ppwc = 9.9;
    int ncoarsen = 0;
    while (ncoarsen < 5 && ppw / (double)(2 << ncoarsen) >= ppwc) ++ncoarsen;
    const int interior = std::min(op->nz, std::min(op->ny, op->nx)) - 2 * op->nPML;
    while (ncoarsen > 0 && (interior >> ncoarsen) < 3) --ncoarsen;
    // if the plane inverses of that level do not fit the budget, go one level deeper as long as it keeps HELM_MG3_PPWF (6) points per
    // wavelength: 20-35 iterations instead of 6-15, still an order of magnitude fewer than the standard cycle
    if (ncoarsen > 0) {
        size_t totb = 0;
        const size_t freeb = mg3_available_bytes(op->device, &totb);
        // budget of the plane inverses: a third of the device, and never more than what is free now less the Krylov vectors of this call
        const double krylov = 11.0 * batch * (double)op->N * sizeof(cplx);
        const double cap = std::min(totb / 3.0, std::max(0.0, (double)freeb - (op->d_ws ? 0.0 : krylov)));
        const double ppwf = 6.0;
        while (ncoarsen < 5 && coarse_estimate(op, ncoarsen, batch, false, tune).bytes > cap && ppw / (double)(2 << ncoarsen) >= ppwf && (interior >> (ncoarsen + 1)) >= 3) ++ncoarsen;
        // ... and one level deeper (down to 5 points) when that SAVES time for the right-hand sides of the call that builds the preconditioner:
        // the set-up of the deeper level is cheaper (np plane inversions of m^3 work each) but every right-hand side pays more iterations.
        //   set-up saved   = np_d t_inv(m_d) - np_{d+1} t_inv(m_{d+1}),  t_inv timed on this device (inverse_seconds)
        //   iterations paid = nrhs * extra * t_iter,  t_iter = 18 fine-grid applies per right-hand side, the apply timed on this grid at this
        //                    batch width (apply_seconds_per_rhs).  18: an iteration of the right-preconditioned BiCGSTAB is 2 applies, 2 cycles of
        //                    ~3.7 fine-grid-apply equivalents each (two smoothing sweeps + the residual on the finest level, ~20 % more for the
        //                    levels below it), 224 B per point of vector updates (~4 applies at 16 right-hand sides) and two coarse solves;
        //                    on config 5 this reproduces the 2.6 ms per right-hand side and iteration measured there.
        //   extra          = +11 / +22 / +38 iterations with the Galerkin direct level at >= 8 / 6 / 5 points per wavelength -- a property of the
        //                    cycle, not of the machine: measured on config 5 (homogeneous) and on the heterogeneous probes of DESIGN.md 5.3.
        if (op->mg3_rhs_hint > 0 && tune.mg3_depth_model && ncoarsen < 5 && (interior >> (ncoarsen + 1)) >= 3) {
            const double ppwd = ppw / (double)(2 << ncoarsen);
            if (ppwd >= 5.0) {
                const CoarseEst e0 = coarse_estimate(op, ncoarsen, batch, true, tune), e1 = coarse_estimate(op, ncoarsen + 1, batch, true, tune);
                const double saved = testing_hook_d("HELM_MG3_DEPTH_SETUP_SCALE", 1.0) * (e0.seconds - e1.seconds);
                // iterations the deeper hierarchy costs per right-hand side: booked counts of both classes where this process has run them,
                // the prior (+11 / +22 / +38) on top of the booked count of the other, or alone, where it has not
                const double prior = ppwd >= 8.0 ? 11.0 : (ppwd >= 6.0 ? 22.0 : 38.0);
                const double rt_cls = lookup_rtol(op);
                const double its0 = its_lookup(op, ncoarsen, 2.0 * ppwd, rt_cls), its1 = its_lookup(op, ncoarsen + 1, ppwd, rt_cls);      // (ppwd: the DEEPER candidate's direct level)
                const double extra_its = (its0 > 0 && its1 > 0) ? std::max(0.0, its1 - its0) : prior;
                const double t_iter = 18.0 * apply_seconds_per_rhs(op, batch);
                const double paid = op->mg3_rhs_hint * extra_its * t_iter;
                const bool deeper = saved > paid || testing_hook("HELM_MG3_DEPTH_FORCE_DEEPER") != 0;
                if (mg3_trace()) {
                    fprintf(stderr, "[mg3 depth] %d coarsenings (%.1f points per wavelength on the direct level): set-up %d x %d^2 (%s); one deeper: %d x %d^2 (%s); saves %.3f s, "
                                    "costs %d rhs x %.0f iterations x %.2f ms = %.3f s -> %s\n", ncoarsen, ppwd, e0.np, e0.m, e0.nd ? "column dissection, top separator" : "planes",
                            e1.np, e1.m, e1.nd ? "column dissection, top separator" : "planes", saved, op->mg3_rhs_hint, extra_its,
                            t_iter * 1e3, paid, deeper ? "deeper" : "stay");
                    fprintf(stderr, "[mg3 depth]   iterations booked in this process: this depth %.1f, one deeper %.1f (< 0: never run; prior +%.0f)\n", its0, its1, prior);
                }
                if (deeper) ++ncoarsen;
            }
        }
    }
    return tune.mg3_keep_levels >= 0 ? tune.mg3_keep_levels : ncoarsen;
}
