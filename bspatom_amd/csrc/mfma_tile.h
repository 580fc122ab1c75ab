// mfma_tile.h -- the LDS image of a staged operand tile and one k-step of a wave tile on v_mfma_f64_16x16x4_f64, shared by
// the kernels of gemm_f64.hip and dipole.hip.
#pragma once
#include "common.h"

namespace bsp {

// One k-step (depth 4) of a (16 TM) x (16 TN) wave tile: acc[i][j] += A(16 rows of block i, 4) * B(4, 16 cols of block j).
// Arow / Brow: LDS row k0 + (lane >> 4) of this wave's A / B tile.  (A core on v_mfma_f64_4x4x4, whose layouts nest in
// these -- tools/microbench/mfma4_probe.hip -- and which a register-only loop runs at 72 TFLOP/s against 36-48 for
// 16x16x4 -- tools/microbench/mfma_f64_peak.hip -- was tried: 20 instead of 8 LDS reads per step, and the kernels
// came out 2-5 % SLOWER; they are not bound by the matrix pipe.)
// LDS image of a staged tile: row k holds its columns permuted inside every aligned group of 16, column x at x ^ lds_swz(k).
// The row stride (BX + 16 doubles) puts rows k and k + 2 on the same banks; an operand that is contiguous along k in memory is
// stored with eight lanes of a 16-lane group on rows k, k + 2, .., k + 14 of ONE column -- an eight-way bank conflict per
// ds_write_b64 without the permutation (counters, profiles/r03_lds_util.json: 63 % of symm's LDS-array cycles and 70 % of
// gemm_kernel<64,64>'s were conflict cycles), none with it: the eight rows land on eight different even offsets.  A fragment
// read takes the 16 columns of a group in permuted order (the same banks); pairs of columns stay pairs (the offset is even).
__device__ __forceinline__ int lds_swz(int k) { return ((k >> 1) & 7) << 1; }

// SW = false: no operand of the kernel is staged with the transposed store (the rank-128 update): plain rows
template <int TM, int TN, bool SW = true>
__device__ __forceinline__ void mfma_step(const double *Arow, const double *Brow, int lane, int kr, double4_t (&acc)[TM][TN])
{
    double a[TM], b[TN];
    const int c = SW ? (lane & 15) ^ lds_swz(kr) : (lane & 15);
#pragma unroll
    for (int i = 0; i < TM; ++i) a[i] = Arow[i * 16 + c];
#pragma unroll
    for (int j = 0; j < TN; ++j) b[j] = Brow[j * 16 + c];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], acc[i][j], 0, 0, 0);
}

}  // namespace bsp
