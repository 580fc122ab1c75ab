// resolvent_pencil.h -- the matrix of a one-wave resolvent item, H_l - i W - z S, and the scratch of the slot that factors it: what
// resolvent.hip (resolvent_kernel, resolvent_chain_kernel) and spline_window.hip (spline_window_kernel) both hand to
// band_lu_wave.h's wave_lu_factor.  One definition, so that "bspatom_resolvent's matrix" in the guarantees of
// include/bspatom_spline_window.h (W3) names code, not a copy.  The bodies are compiled with contraction OFF wherever they are
// included (the pragma is scoped to the body, as in band_lu_wave.h); the two fused products are written out.
#pragma once
#include "common.h"

namespace bsp {

// doubles of one slot's scratch -- U [n][2b+1], L [n][b], y [n] complex, then piv [n] ints --, even (a slot starts on a 16-byte
// boundary)
__host__ __device__ inline size_t rs_slot_doubles(int n, int k)
{
    const size_t b = (size_t)k - 1, piv = ((size_t)n + 1) / 2;
    return 2 * ((size_t)n * (2 * b + 1) + (size_t)n * b + (size_t)n) + piv + (piv & 1);
}

// The matrix of an item, wave_lu_factor's argument.  SB, HB upper bands [k][n] used symmetrically (eigvec.hip::pencil_entry), WB the
// absorber's FULL band [2k-1][n] with WB[d + b][i] = W(i, i + d), both triangles as given, or null.  entry: M(r, c); diag: |M(j,j)| by
// cabs1 and the sum of the magnitudes of its terms (rs_pertol).  h - zr s and -(zi s) - w round once.
struct RsPencil {
    const double *SB, *HB, *WB;
    int n, b;
    double zr, zi;
    __device__ __forceinline__ void entry(int r, int c, double &re, double &im) const
    {
#pragma clang fp contract(off)
        const int d = (r > c) ? (r - c) : (c - r);
        re = 0.0; im = 0.0;
        if (d > b || r < 0 || c < 0 || r >= n || c >= n) return;
        const int lo = (r > c) ? c : r;
        const double s = SB[(size_t)d * n + lo];
        re = __builtin_fma(-zr, s, HB[(size_t)d * n + lo]);
        im = -(zi * s);
        if (WB) im = im - WB[(size_t)(c - r + b) * n + r];
    }
    __device__ __forceinline__ void diag(int j, double &mag, double &flo) const
    {
#pragma clang fp contract(off)
        const double s = SB[j], h = HB[j], wv = WB ? WB[(size_t)b * n + j] : 0.0;
        mag = fabs(__builtin_fma(-zr, s, h)) + fabs(__builtin_fma(-zi, s, -wv));
        flo = (fabs(h) + fabs(zr * s)) + (fabs(zi * s) + fabs(wv));
    }
};

}  // namespace bsp
