// tdse_launch.h -- what the launchers of tdse.hip, tdse_static.hip, tdse_fields.hip and tdse_adapt.hip share, host code only: the grids
// with their bounds, the coefficient structs of the tableau, the phase pointer of a stage, the dispatch of a stage number to a
// template argument, and the launchers the four files call among themselves.  Which column tile a stage takes is each file's choice.
#pragma once
#include <type_traits>
#include "common.h"
#include "tdse_stage.h"

namespace bsp {

extern const double TDSE_A[6][5], TDSE_D[6], TDSE_B[6];          // the tableau (tdse.hip)

// a stage on column tiles of 16 TN columns, TN = 1 or 2: tm row tiles of TBM states, tn column tiles, one workgroup per (channel, tile)
struct StageGrid { int tm, tn; unsigned grid; bool ok; };
inline StageGrid stage_grid(const TdseDims &d, int TN)
{
    const int tm = (d.count + TBM - 1) / TBM, tn = TN == 1 ? d.NC / 16 : (d.NC + 31) / 32;
    const long long grid = (long long)d.nch * tm * tn;
    return {tm, tn, (unsigned)grid, grid <= 0x7fffffffLL};
}

// workgroups of 256 threads over n items
struct Blocks { unsigned n; bool ok; };
inline Blocks blocks256(long long n)
{
    const long long b = (n + 255) / 256;
    return {(unsigned)b, b <= 0x7fffffffLL};
}
// the reduction of the row-tile partials: one thread per (scan, channel)
inline Blocks reduce_blocks(const TdseDims &d) { return blocks256((long long)d.nscan * d.nch); }

// the step kernel: 32 rows by 8 scans per workgroup
struct StepGrid { long long rows; dim3 grid; bool ok; };
inline StepGrid step_grid(const TdseDims &d)
{
    const long long rows = (long long)d.nch * d.count, gx = (rows + 31) / 32;
    const int gy = (d.NC / 2 + 7) / 8;
    return {rows, dim3((unsigned)gx, (unsigned)gy), gx <= 0x7fffffffLL && gy <= 65535};
}

// doubles of the working amplitudes, and of each k_s
inline size_t k_stride(const TdseDims &d) { return (size_t)d.nch * d.count * d.NC; }

template <int S> StageCoef stage_coef()
{
    StageCoef cf;
    for (int j = 0; j < 5; ++j) cf.w[j] = TDSE_A[S][j];
    return cf;
}

inline StepCoef step_coef()
{
    StepCoef sc;
    for (int j = 0; j < 6; ++j) { sc.d[j] = TDSE_D[j]; sc.e[j] = TDSE_D[j] - TDSE_B[j]; }
    return sc;
}

// Lawson: the phases of stage S in the table of launch_tdse_phases (stage 0 has none); null in the plain scheme
inline const double *stage_phases(int S, const TdseDims &d, const TdseBufs &w)
{
    return w.ph && S > 0 ? w.ph + (size_t)(S - 1) * d.nch * d.count * 2 : nullptr;
}
// the phases of the full step, c_4 = 1
inline const double *step_phases(const TdseDims &d, const TdseBufs &w) { return w.ph ? w.ph + (size_t)3 * d.nch * d.count * 2 : nullptr; }

// f(std::integral_constant<int, S>) for the stage number S = 0 .. 5
template <class F> int dispatch_stage(int S, F &&f)
{
    switch (S) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    default: return f(std::integral_constant<int, 5>{});
    }
}

// tdse_static.hip: what tdse.hip's launchers launch when w.W is set (stage S, the observing stage 0) or w.ow is 6 (the reduction)
int launch_tdse_static_stage(int S, const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st);
int launch_tdse_static_observe(const TdseDims &d, const TdseBufs &w, const double *fld, bool lawson, hipStream_t st);
int launch_tdse_static_reduce(const TdseDims &d, const TdseBufs &w, double *d_row, hipStream_t st);
// tdse_fields.hip: what they launch instead when w.nf > 1
int launch_tdse_fields_stage(int S, const TdseDims &d, const TdseBufs &w, const double *fld, double dt, hipStream_t st);
int launch_tdse_fields_observe(const TdseDims &d, const TdseBufs &w, const double *fld, bool lawson, hipStream_t st);
int launch_tdse_fields_reduce(const TdseDims &d, const TdseBufs &w, double *d_row, hipStream_t st);

}  // namespace bsp
