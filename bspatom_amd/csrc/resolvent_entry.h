// resolvent_entry.h -- what the two coupled-channel kernels (resolvent_coupled.hip, resolvent_wide.hip) share: the entry of the coupled
// matrix and the wave-level pieces of the pivot search.  One definition, so that both calls factor the same numbers.
#pragma once
#include "common.h"
#include "wave_ops.h"

namespace bsp {

// The maximum over the 64 lanes of values that are >= 0 in lane 0 (wave_sum's scan with fmax: zeros shift in and change nothing)
__device__ __forceinline__ double rc_wave_max(double x)
{
    x = fmax(x, dpp_mov<0x111>(x)); x = fmax(x, dpp_mov<0x112>(x)); x = fmax(x, dpp_mov<0x114>(x)); x = fmax(x, dpp_mov<0x118>(x));
    return fmax(fmax(read_lane(x, 15), read_lane(x, 31)), fmax(read_lane(x, 47), read_lane(x, 63)));
}
// *p where ok, else zero: a guarded load, never a load through a selected address (that one is a FLAT load, whose wait drains the
// global loads and stores in flight as well)
__device__ __forceinline__ double2 rc_load(const double2 *p, bool ok)
{
    double2 v = make_double2(0.0, 0.0);
    if (ok) v = *p;
    return v;
}
// M(R, C) of item `it`, R = i nch + c, C = j nch + c2.  fl: the sum of the magnitudes of the terms (the pivot threshold's floor).
__device__ __forceinline__ void rc_entry(const ResolventCoupledArgs &a, int it, int R, int C, double &re, double &im, double &fl)
{
    re = 0.0; im = 0.0; fl = 0.0;
    const int n = a.n, b = a.k - 1, nch = a.nch;
    if (C < 0 || C >= n * nch) return;
    const int i = R / nch, c = R - i * nch, j = C / nch, c2 = C - j * nch;
    const int d = (i > j) ? (i - j) : (j - i);
    if (d > b) return;
    if (c == c2) {
        const int lo = (i > j) ? j : i, mc = it * nch + c;
        const double zr = a.z[2 * mc], zi = a.z[2 * mc + 1];
        const double s = a.SB[(size_t)d * n + lo], h = a.HB[((size_t)a.chan[mc] * a.k + d) * n + lo];
        re = h - zr * s;
        im = -(zi * s);
        fl = (fabs(h) + fabs(zr * s)) + fabs(zi * s);
        const int ws = a.w[mc];
        if (a.WB && ws >= 0) {
            const double wv = a.WB[((size_t)ws * (2 * b + 1) + (j - i + b)) * n + i];
            im -= wv;
            fl += fabs(wv);
        }
    }
    const size_t cs = (size_t)(2 * b + 1) * n;
    for (int p = 0; p < a.ncoup; ++p) {
        if (a.cr[p] != c || a.cc[p] != c2) continue;
        const size_t at = a.ctr[p] ? (size_t)(i - j + b) * n + j : (size_t)(j - i + b) * n + i;   // G(i, j), or G(j, i) for the transpose
        const double *co = a.acoef + ((size_t)it * a.ncoup + p) * a.nop * 2;
        for (int o = 0; o < a.nop; ++o) {
            const double g = a.GB[(size_t)o * cs + at];
            re += co[2 * o] * g;
            im += co[2 * o + 1] * g;
            fl += (fabs(co[2 * o]) + fabs(co[2 * o + 1])) * fabs(g);
        }
    }
}

}  // namespace bsp
