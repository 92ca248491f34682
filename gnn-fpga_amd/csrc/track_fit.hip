// track_fit.hip - the fit of every track candidate for gfx950: per track the thirteen moments of its hits, Karimaki's
// non-iterative circle fit (NIM A305 (1991) 187, unweighted) in (x, y) and a straight line z = z0 + cot r in (r, z).
// The reference has no counterpart (it ends at segment scores); gnn-fpga_amd/tracks.py fit_tracks_numpy is the
// specification and k_track_fit restates it operation for operation, so that every output equals it bit for bit.
//
//   k_track_fit   one lane per track, 256 lanes per workgroup.  The lane walks its track's hits in list order
//                 (ascending hit id) and adds each hit's thirteen terms to thirteen registers, starting from 0.0:
//                 the order of the additions IS the specification's.  The parameters follow from those registers
//                 after the loop.  A track of more than max_hits hits is flagged and not walked, so a lane's loop is
//                 at most max_hits long whatever the batch holds (mode "components" makes 10 k-hit components).
//
// Arithmetic.  float64; + - * /, sqrt and comparisons only - the direction (cos, sin) of half the angle atan2(a, b)
// comes from two square roots, no transcendental function.  Every operation is rounded on its own: contraction is off
// for this file, by the pragma below and by the Makefile's flag for this unit (see toy_graphs.hip for why both).
// Memory.  A hit costs 4 bytes of track_hits, read in order, and three gathered doubles: about 28 bytes per hit in a
// track.  All offsets are 64-bit.  A hit id outside [0, n_hits) is flagged and not read; a track_ptr pair that leaves
// track_hits (the specification refuses such input on the host) is flagged the same way and nothing is read.
#include "common.h"

#pragma clang fp contract(off)

namespace gnn {
namespace {

constexpr int kFitMoments = 13, kFitParams = 8;
constexpr int kFitFew = 1, kFitMany = 2, kFitNonFinite = 4, kFitCircle = 8, kFitLine = 16, kFitRange = 32;

__global__ __launch_bounds__(kBlock) void k_track_fit(const int32_t *__restrict__ track_ptr,
                                                      const int32_t *__restrict__ track_hits, int64_t n_tracks,
                                                      int64_t n_track_hits, const double *__restrict__ x,
                                                      const double *__restrict__ y, const double *__restrict__ z,
                                                      int64_t n_hits, int max_hits, double *__restrict__ moments,
                                                      double *__restrict__ params, int32_t *__restrict__ n_fit,
                                                      int32_t *__restrict__ status)
{
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_tracks) return;
    const double nan = __builtin_nan("");
    const int64_t lo = track_ptr[t], hi = track_ptr[t + 1];
    const bool listed = lo >= 0 && hi >= lo && hi <= n_track_hits;
    const int64_t n = listed ? hi - lo : 0;
    int st = (listed ? 0 : kFitRange) | (n < 3 ? kFitFew : 0) | (n > max_hits ? kFitMany : 0);

    double sx = 0.0, sy = 0.0, sz = 0.0, sr2 = 0.0, sxx = 0.0, sxy = 0.0, syy = 0.0, sxr = 0.0, syr = 0.0, srr = 0.0;
    double sr = 0.0, srz = 0.0, szz = 0.0;
    double xi = 0.0, yi = 0.0, ri = 0.0, xo = 0.0, yo = 0.0, ro = 0.0;      // the hits of smallest and largest r2
    const int64_t walk = n > max_hits ? 0 : n;
    for (int64_t k = 0; k < walk; ++k) {
        const int64_t h = track_hits[lo + k];
        if (h < 0 || h >= n_hits) {
            st |= kFitRange;
            continue;
        }
        const double hx = x[h], hy = y[h], hz = z[h];
        if (!(__builtin_isfinite(hx) && __builtin_isfinite(hy) && __builtin_isfinite(hz))) st |= kFitNonFinite;
        const double xx = hx * hx, yy = hy * hy;
        const double r2 = xx + yy;
        const double r = sqrt(r2);
        sx = sx + hx;
        sy = sy + hy;
        sz = sz + hz;
        sr2 = sr2 + r2;
        sxx = sxx + xx;
        sxy = sxy + hx * hy;
        syy = syy + yy;
        sxr = sxr + hx * r2;
        syr = syr + hy * r2;
        srr = srr + r2 * r2;
        sr = sr + r;
        srz = srz + r * hz;
        szz = szz + hz * hz;
        if (k == 0 || r2 < ri) xi = hx, yi = hy, ri = r2;       // strict: a tie stays with the earlier hit
        if (k == 0 || r2 > ro) xo = hx, yo = hy, ro = r2;
    }

    const double nf = (double)n;
    const double mx = sx / nf, my = sy / nf, mz = sz / nf, mr2 = sr2 / nf, mxx = sxx / nf, mxy = sxy / nf;
    const double myy = syy / nf, mxr = sxr / nf, myr = syr / nf, mrr = srr / nf, mr = sr / nf, mrz = srz / nf;
    const double mzz = szz / nf;
    const double Cxx = mxx - mx * mx, Cxy = mxy - mx * my, Cyy = myy - my * my;
    const double Cxr = mxr - mx * mr2, Cyr = myr - my * mr2, Crr = mrr - mr2 * mr2;
    const double a = 2.0 * (Crr * Cxy - Cxr * Cyr);
    const double b = Crr * (Cxx - Cyy) - Cxr * Cxr + Cyr * Cyr;
    const double hh = sqrt(a * a + b * b);
    const double cp = sqrt((1.0 + b / hh) / 2.0);               // b >= 0: the cosine first
    const double sp = (a / hh) / (2.0 * cp);
    const double sq = sqrt((1.0 - b / hh) / 2.0);               // b < 0: the sine first, with the sign of a
    const double sn = a >= 0.0 ? sq : -sq;
    const double cn = (a / hh) / (2.0 * sn);
    double c = b >= 0.0 ? cp : cn, s = b >= 0.0 ? sp : sn;
    if (c * (xo - xi) + s * (yo - yi) < 0.0) c = -c, s = -s;    // from the innermost hit to the outermost
    const double kappa = (s * Cxr - c * Cyr) / Crr;
    const double delta = -kappa * mr2 + s * mx - c * my;
    const double w = 1.0 - 4.0 * delta * kappa;
    const double u = sqrt(w);
    const double rho = 2.0 * kappa / u;
    const double d = 2.0 * delta / (1.0 + u);
    const double f = 1.0 + rho * d;
    const double chi2c = nf * f * f * (s * s * Cxx - 2.0 * s * c * Cxy + c * c * Cyy - kappa * kappa * Crr);
    const double Crz = mrz - mr * mz, Cr = mr2 - mr * mr, Czz = mzz - mz * mz;
    const double cot = Crz / Cr;
    const double z0 = mz - cot * mr;
    const double chi2l = nf * (Czz - cot * Crz);

    const bool unfit = (st & (kFitFew | kFitMany | kFitNonFinite | kFitRange)) != 0;
    if (!unfit && !(Crr > 0.0 && hh > 0.0 && w > 0.0)) st |= kFitCircle;
    if (!unfit && !(Cr > 0.0)) st |= kFitLine;
    const bool blank = (st & (kFitMany | kFitNonFinite | kFitRange)) != 0;
    const bool no_circle = unfit || (st & kFitCircle), no_line = unfit || (st & kFitLine);

    double *m = moments + t * kFitMoments;
    m[0] = blank ? nan : sx;
    m[1] = blank ? nan : sy;
    m[2] = blank ? nan : sz;
    m[3] = blank ? nan : sr2;
    m[4] = blank ? nan : sxx;
    m[5] = blank ? nan : sxy;
    m[6] = blank ? nan : syy;
    m[7] = blank ? nan : sxr;
    m[8] = blank ? nan : syr;
    m[9] = blank ? nan : srr;
    m[10] = blank ? nan : sr;
    m[11] = blank ? nan : srz;
    m[12] = blank ? nan : szz;
    double *p = params + t * kFitParams;
    p[0] = no_circle ? nan : rho;
    p[1] = no_circle ? nan : c;
    p[2] = no_circle ? nan : s;
    p[3] = no_circle ? nan : d;
    p[4] = no_circle ? nan : chi2c;
    p[5] = no_line ? nan : cot;
    p[6] = no_line ? nan : z0;
    p[7] = no_line ? nan : chi2l;
    n_fit[t] = (int32_t)n;
    status[t] = st;
}

}  // namespace
}  // namespace gnn

using namespace gnn;

extern "C" {

int gnn_track_fit(const int32_t *track_ptr, const int32_t *track_hits, int64_t n_tracks, int64_t n_track_hits,
                  const double *x, const double *y, const double *z, int64_t n_hits, int32_t max_hits, double *moments,
                  double *params, int32_t *n_fit, int32_t *status, void *stream)
{
    static const char *who = "gnn_track_fit";
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_tracks < 0 || n_tracks >= 0x7fffffffLL) return fail(GNN_ERR_BADARG, "%s: n_tracks negative or 2^31 and more", who);
    if (n_track_hits < 0 || n_track_hits >= 0x7fffffffLL)
        return fail(GNN_ERR_BADARG, "%s: n_track_hits negative or 2^31 and more", who);
    if (n_hits < 0 || n_hits >= 0x7fffffffLL) return fail(GNN_ERR_BADARG, "%s: n_hits negative or 2^31 and more", who);
    if (max_hits < 3) return fail(GNN_ERR_BADARG, "%s: max_hits %d, a fit needs at least 3 hits", who, max_hits);
    if (n_tracks == 0) return 0;
    if (!track_ptr) return fail(GNN_ERR_BADARG, "%s: pointer track_ptr missing", who);
    if (n_track_hits > 0 && !track_hits) return fail(GNN_ERR_BADARG, "%s: pointer track_hits missing", who);
    if (n_hits > 0 && (!x || !y || !z)) return fail(GNN_ERR_BADARG, "%s: pointer x, y or z missing", who);
    if (!moments || !params) return fail(GNN_ERR_BADARG, "%s: pointer moments or params missing", who);
    if (!n_fit || !status) return fail(GNN_ERR_BADARG, "%s: pointer n_fit or status missing", who);
    GNN_LAUNCH("k_track_fit", k_track_fit, (unsigned)((n_tracks + kBlock - 1) / kBlock), kBlock, s, track_ptr, track_hits,
               n_tracks, n_track_hits, x, y, z, n_hits, (int)max_hits, moments, params, n_fit, status);
    return 0;
}

}  // extern "C"
