// wave_ops.h -- one definition of each wave-level primitive of the kernels (device code, gfx950, waves of 64 lanes).
// A double is two dwords to the cross-lane instructions: every primitive moves the halves separately.
#pragma once
#include <hip/hip_runtime.h>

namespace bsp {

// x of the lane a DPP control selects (CTRL: row_shr, row_ror, quad_perm, row_mirror ...); 0 where the control has no source lane
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double x)
{
    union { double d; int i[2]; } u, r;
    u.d = x;
    r.i[0] = __builtin_amdgcn_update_dpp(0, u.i[0], CTRL, 0xf, 0xf, true);
    r.i[1] = __builtin_amdgcn_update_dpp(0, u.i[1], CTRL, 0xf, 0xf, true);
    return r.d;
}
// x of lane l (uniform l), the same in every lane
__device__ __forceinline__ double read_lane(double x, int l)
{
    union { double d; int i[2]; } u, r;
    u.d = x;
    r.i[0] = __builtin_amdgcn_readlane(u.i[0], l);
    r.i[1] = __builtin_amdgcn_readlane(u.i[1], l);
    return r.d;
}
// x of the first active lane
__device__ __forceinline__ double read_first_lane(double x)
{
    union { double d; int i[2]; } u, r;
    u.d = x;
    r.i[0] = __builtin_amdgcn_readfirstlane(u.i[0]);
    r.i[1] = __builtin_amdgcn_readfirstlane(u.i[1]);
    return r.d;
}
// x of lane srclane, a lane's own choice (through the LDS crossbar)
__device__ __forceinline__ double bpermute(double x, int srclane)
{
    union { double d; int i[2]; } u, r;
    u.d = x;
    r.i[0] = __builtin_amdgcn_ds_bpermute(srclane << 2, u.i[0]);
    r.i[1] = __builtin_amdgcn_ds_bpermute(srclane << 2, u.i[1]);
    return r.d;
}
// A barrier that waits for LDS traffic only: global loads and stores stay in flight across it (__syncthreads() would drain
// vmcnt(0) as well).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// Sum over the 64 lanes, the same bits in every lane: a row scan (row_shr 1, 2, 4, 8, zeros shift in -- lane 15 of each 16-lane
// row then holds the row total) and the four row totals as (l15 + l31) + (l47 + l63).  ~10x shorter dependent chain than a
// ds_bpermute butterfly.
__device__ __forceinline__ double wave_sum(double x)
{
    x += dpp_mov<0x111>(x); x += dpp_mov<0x112>(x); x += dpp_mov<0x114>(x); x += dpp_mov<0x118>(x);
    return (read_lane(x, 15) + read_lane(x, 31)) + (read_lane(x, 47) + read_lane(x, 63));
}
// the same over lanes 0 .. 31 alone: l15 + l31
__device__ __forceinline__ double wave_sum32(double x)
{
    x += dpp_mov<0x111>(x); x += dpp_mov<0x112>(x); x += dpp_mov<0x114>(x); x += dpp_mov<0x118>(x);
    return read_lane(x, 15) + read_lane(x, 31);
}

// Sums over the 16 lanes of a DPP row, the total in every lane of the row (bitwise the same in all of them: each step adds the two
// halves of a pair, and addition commutes).  Two butterflies with DIFFERENT orders of summation -- not interchangeable:
// rsum16: quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror
__device__ __forceinline__ double rsum16(double x)
{
    x += dpp_mov<0xB1>(x);
    x += dpp_mov<0x4E>(x);
    x += dpp_mov<0x141>(x);
    x += dpp_mov<0x140>(x);
    return x;
}
// four of them at once: the same four operations per value (the same bits), the four dependent chains interleaved so that the DPP
// hazard slots and the add latencies of one are filled by the others (back to back the compiler pads them with s_nop)
__device__ __forceinline__ void rsum16x4(double (&x)[4])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] += dpp_mov<0xB1>(x[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] += dpp_mov<0x4E>(x[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] += dpp_mov<0x141>(x[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] += dpp_mov<0x140>(x[q]);
}
// cw_rowsum: row_ror 8, 4, 2, 1
__device__ __forceinline__ double cw_rowsum(double x)
{
    x += dpp_mov<0x128>(x);
    x += dpp_mov<0x124>(x);
    x += dpp_mov<0x122>(x);
    x += dpp_mov<0x121>(x);
    return x;
}

}  // namespace bsp
