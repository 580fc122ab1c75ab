// spline_overlap.h -- b = S v on one wave with the S-norm of v beside it: rule 1 of include/bspatom_tdse_spline.h and the N_ch of the
// spline rows, one definition for tdse_split.hip (the right-hand side of every substep, the rows) and spline_window.hip (the
// right-hand side of every stage, the result).  The body is compiled with contraction OFF wherever it is included (the pragma is
// scoped to the body, as in band_lu_wave.h): every sum here has its order fixed by a header.
#pragma once
#include "common.h"

namespace bsp {

// y = S v by rule 1 of include/bspatom_tdse_spline.h: y_re(i), y_im(i) start at +0.0 and add S(i, i + d) v(i + d) for d = -(k-1) .. k-1
// ascending, columns outside 0 .. n-1 skipped.  Lane-strided over the rows; a row's loads are issued together by blocks of CH
// diagonals, every address clamped into its array and what was loaded outside dropped by a select (rs_band_apply's way).  v is
// visible to the wave.  Returns, where nrm is set, this lane's part of Re sum_i conj(v(i)) y(i), rows ascending (else zero).
template <int BT>
__device__ __forceinline__ double sp_overlap(const int n, const int b, const double *__restrict__ SB, const double2 *v, double2 *y, const bool nrm,
                                             const int lane)
{
#pragma clang fp contract(off)
    constexpr int CH = (2 * BT + 1 + 2) / 3;
    const int nd = 2 * b + 1;
    double s = 0.0;
    for (int i = lane; i < n; i += 64) {
        double yr = 0.0, yi = 0.0;
#pragma unroll 1
        for (int d0 = 0; d0 < nd; d0 += CH) {
            double t[CH];
            double2 xv[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int d = d0 + u - b, ad = d < 0 ? -d : d, lo = d < 0 ? i + d : i;
                const bool in = d0 + u < nd && lo >= 0 && i + d < n;
                t[u] = SB[in ? (size_t)ad * n + lo : 0];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int j = i + d0 + u - b;
                xv[u] = v[j < 0 ? 0 : (j >= n ? n - 1 : j)];
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int j = i + d0 + u - b;
                const bool in = d0 + u < nd && j >= 0 && j < n;
                const double ur = yr + t[u] * xv[u].x, ui = yi + t[u] * xv[u].y;
                yr = in ? ur : yr;
                yi = in ? ui : yi;
            }
        }
        y[i] = make_double2(yr, yi);
        if (nrm) {
            const double2 cv = v[i];
            s = s + (cv.x * yr + cv.y * yi);
        }
    }
    return s;
}

}  // namespace bsp
