// common.h -- shared declarations of libbspatom (MI355X / gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// status codes of the C ABI (include/bspatom.h)
#define BSP_OK 0
#define BSP_ERR_HIP (-1)       // HIP runtime error (message on stderr)
#define BSP_ERR_ARG (-2)       // invalid argument
#define BSP_ERR_BSPLVB (-3)    // 'FATAL ERROR - BSPLVB' (reference bsplvb.f90:30-34)
#define BSP_ERR_NOGPU (-4)     // no gfx950 device visible
#define BSP_ERR_UNSUPPORTED (-5)

#define BSP_HIP(x)                                                                          \
    do {                                                                                    \
        hipError_t e_ = (x);                                                                \
        if (e_ != hipSuccess) {                                                             \
            fprintf(stderr, "bspatom: HIP error '%s' at %s:%d\n", hipGetErrorString(e_),    \
                    __FILE__, __LINE__);                                                    \
            return BSP_ERR_HIP;                                                             \
        }                                                                                   \
    } while (0)

typedef double double4_t __attribute__((ext_vector_type(4)));

// Batch stride (doubles) of the band storage AB[npad][128] of one l-channel.  The 1088-double
// (8.5 KiB) skew keeps the channels, which march through their bands in lock-step during sb2st, from
// hitting the same HBM channel/bank at the same instant (a power-of-two stride would).
__host__ __device__ inline size_t ab_stride(int npad) { return (size_t)npad * 128 + 1088; }

namespace bsp {

constexpr int SBR_XDPP_DEFAULT = 2;   // Options::sbr_xdpp: the best measured setting (profiles/r24_chase8_dpp.txt)

// ---- run-time switches (A/B comparisons, diagnostics, test hooks) ---------------------------------
// Read ONCE per process from the environment (BSP_* variables) at the first use; the tests flip
// them in-process through bspatom_set_option (include/bspatom.h) to drive the fallback paths.
struct Options {
    int sb2st_version = 0;       // 0: by size (9 = two steps, sbr2.hip, for n >= 512; else 8); 9 / 8 / 7 / 3 force a generation
    int sb2st_ring = 0;          // BSP_SB2ST_RING: ring size (0 = by channel count)
    int sb2st_margin = 3, sb2st_hyst = 2;
    int sb2st_lead = 0;          // BSP_SB2ST_LEAD: 0 = by ring size (pairs: 8, larger rings: 16; re-scan of round 2)
    int sb2st_check = 0;         // BSP_SB2ST_CHECK: synchronise and report ring formation / holds on stderr
    int sb2st_diag = 0;          // BSP_SB2ST_DIAG: instrumented kernel
    int sb2st_force_abort = 0;   // test hook: 1 = every ring ABORTs its handshake (member 0 runs alone); 2 = pretend the
                                 // members sit on different XCDs (same fallback through the other branch)
    int sy2sb_groups = 2, sy2sb_lookahead = 1, sy2sb_segs = 0;
    int panel_qr = 3;            // BSP_PANEL_QR: 3 = TSQR + Householder reconstruction on many workgroups (tsqr.hip); 2 = one workgroup per
                                 // channel with LDS-DMA (n <= 8256; above 4096 rows it falls back to 1), 1 = the first panel kernel
    int tsqr_max_m = 2048;       // BSP_TSQR_MAX_M: panels with more rows than this (and at most 8192) take the one-workgroup kernel (0 = no limit); a rule in m alone,
                                 // so the arithmetic does not depend on the batch size
    int tsqr_regcap = 1;         // BSP_TSQR_REGCAP: 1 = the 256-register variants of the tsqr.hip kernels (they fit beside one GEMM workgroup), 0 = uncapped
    int gemm_diag = 0;
    int bisect = 3, bisect_ept = 0;
    int bisect_secant = 1;       // BSP_BISECT_SECANT: 1 = lock-step rounds take a safeguarded secant step where a bracket holds one eigenvalue
                                 // (tridiag.hip; ~22 rounds instead of ~50); 0 = bisection only; >= 2: as 1, and the value is the
                                 // fraction of a workgroup's 1024 eigenvalues (1 / value) left to the multisection tail (1 = 8)
    int bisect_tail = 1;         // BSP_BISECT_TAIL: 0 = lock-step bisection to the end (no multisection tail), for A/B timing
    int bisect_pair = 1;         // BSP_BISECT_PAIR: a workgroup of bisect3_kernel runs two logical workgroups of its channel, x and x + ceil(nw / 2),
                                 // one after the other -- 1 = when there are more workgroups than CUs, 0 = never, 2 = always; bit-identical results
                                 // (only where the queue below does not take the launch)
    int bisect_queue = 1;        // BSP_BISECT_QUEUE: the workgroups of bisect3_kernel claim their logical workgroups from a list, the first on a CU from
                                 // its costly end, the second from its cheap end (tridiag.hip) -- 1 = when there are more logical workgroups than CUs
                                 // (it then takes the place of the pairs), 0 = never, 2 = always; bit-identical results
    int bisect_queue_grid = 0;   // BSP_BISECT_QUEUE_GRID: test hook: the queue launch has at most this many hardware workgroups (0 = no cap)
    int bisect_diag = 0;         // BSP_BISECT_DIAG: instrumented bisect3_kernel: placement, wall-clock stamps and rounds of every workgroup (stderr)
    int no_eigvec_prefetch = 0;
    int vec_early = 1;           // BSP_VEC_EARLY: band route, the consumed eigenvector's eigenvalue from the pencil's inertia right after the assembly (bandsect.hip); 0: from the tridiagonal matrix at the end; 2: as 1 with the check made to fail
    int vec_own_cu = 1;          // BSP_VEC_OWN_CU: the early vector's workgroup asks for a CU's whole LDS (eigvec.hip::early_vector_kernel) -- 1: for batches of more than 32 channels (capi.hip), 2: always, 0: never
    int sb2sb_mfma = 1;          // 1: block-chasing item on the matrix cores (sbr2.hip); 0: the first, all-VALU kernel (cross-check)
    int sb16_rows = 1;           // BSP_SB16_ROWS: 1 = band 16 -> 1 with a whole chase item per DPP row, four sweeps per wave (sbr2.hip); 0 = the
                                 // first layout (one tile spread over a wave), kept as the cross-check
    int poison_c = 0;            // test hook: fill the dense C buffer with NaN bit patterns before every solve (nothing outside the
                                 // blocks the standard form writes may ever be read)
    int route = 0;               // BSP_ROUTE: 0 = by size (the band route wherever crawford_supported), 1 = dense route (standard form, sy2sb,
                                 // two-step bulge chasing: north_star's letter, and every pencil wider than 8), 2 = band route (crawford.hip:
                                 // the pencil stays banded; one-column chase on tiles of 8; UNSUPPORTED where it cannot run)
    int fused_probe = 0;         // BSP_FUSED_PROBE: TIMING EXPERIMENT ONLY (wrong results): the rank-128 update runs 16 K-steps instead of 8 and
                                 // symm is not launched -- the upper bound of what a fused update + symm sweep over A22 can gain (round-3 verdict, item 1)
    int cw_items4 = 1;           // BSP_CW_ITEMS4: 1 = crawford_item4_kernel (four chase items per wave, an item per DPP row in the RQ loop),
                                 // 0 = crawford_item_kernel (one item per wave; the cross-check)
    int cw_nw = 1;               // BSP_CW_NW: waves per workgroup of crawford_item4_kernel (1 or 4; a wave never talks to another)
    int cw_streams = 2;          // BSP_CW_STREAMS: the band reduction's channels in this many groups (1 .. 4), each on a stream of its own
    int cw_chunk_min = 1024;     // BSP_CW_CHUNK_MIN: from this many functions on, the S-only part hands its factor over in CW_CHUNKS pieces (crawford_prepare)
    int s_overlap = 1;           // BSP_S_OVERLAP: band route: the S-only part of the reduction (band Cholesky ..) on a stream of its own beside the
                                 // assembly of the H_l
    int cw_diag = 0;             // BSP_CW_DIAG: s_memtime stamps of the phases of crawford_item4_kernel's waves, averaged over a solve (stderr)
    int cw_split = 0;            // BSP_CW_SPLIT: > 0 = the band reduction runs from both ends of the pencil (n a multiple of 8); the value is the share
                                 // of the blocks, in percent, of the leading part (at most 50 = half the chase items).  NOT the default: the
                                 // leading part's fill is chased towards r = 0 and the eigenvalues next to zero pay for it (at 50 %: 21.8 instead
                                 // of 38.2 ms for the reduction, up to 13 x the error next to zero, 7345 instead of 50 of C4's 524288
                                 // eigenvalues beyond 1e-10 relative; profiles/r04_experiments.txt, 11).  0 = one process over all blocks
    int cw_band8 = 1;            // BSP_CW_BAND8: 1 = the band reduction hands over the band of half-width 8 it really leaves (one 8 x 8 block
                                 // made triangular at the end) and the chase runs on tiles of 8; 0 = half-width 15, tiles of 16 (as first built)
    int sb8_wgs = 0;             // BSP_SB8_WGS: workgroups of the tiles-of-8 chase per CU the rings are sized for (0 = what fits: 2)
    int sbr_phased = 1;          // BSP_SBR_PHASED: tiles-of-8 chase: 1 = the step loop of a chasing wave in three parts (ramp-up, a branch-free
                                 // steady part, ramp-down; sbr2.hip), 0 = one general loop (the cross-check); bit-identical results
    int sbr_lag = 0;             // BSP_SBR_LAG: tiles-of-8 chase, the data-moving wave's lag (steps between the request of a column and the
                                 // wait for it): 0 = short in the passes where the ring is bound by its stagger, long elsewhere; 1 = always
                                 // long; 2 = always short; bit-identical results
    int sbr_xdpp = SBR_XDPP_DEFAULT;   // BSP_SBR_XDPP: tiles-of-8 chase, the phased loop: what reaches the FMAs as a DPP operand (row_newbcast inside the 8
                                 // lanes that own an item) instead of through LDS: 0 = nothing (the cross-check), 1 = z of the diagonal-tile
                                 // wave, 2 = that wave's reflector as well (the default), 3 = the reflector in all three roles (as fast as 2
                                 // at 128 channels, slower than 0 at 16: profiles/r24_chase8_dpp.txt); bit-identical results
    int cw_ipw = 0;              // BSP_CW_IPW: items per wave of crawford_item4_kernel (0 = 4; 1, 2: experiment 9; bit-identical results)
    int cw_ldspad = 0;           // BSP_CW_LDSPAD: KB of unused dynamic LDS per workgroup of crawford_item4_kernel (timing experiment: occupancy)
    int cw_onediv = 0;           // BSP_CW_ONEDIV: reflectors of the band route's RQ loop in the one-division form (A/B switch)
    int cw_bcast = 1;            // BSP_CW_BCAST: crawford_item4_kernel's reflector row 1 = as a DPP operand of the FMAs (row_newbcast; half the
                                 // registers and LDS, four waves per SIMD), 0 = through LDS (the cross-check); bit-identical results
    int cw_spread = 1;           // BSP_CW_SPREAD: a quad's congruences (phase B of crawford_item4_kernel's DPP form) on the waves of a workgroup, one
                                 // SIMD each: 0 = never, 1 (the default) = on 4 / 2 waves where the launch has at most cw_spread_cap4 / cw_spread_cap2 quads over all
                                 // channels, 2 / 4 = on that many waves at every launch (the tests' hook); bit-identical results
    int cw_spread_cap4 = -1;     // BSP_CW_SPREAD_CAP4, BSP_CW_SPREAD_CAP2: the two caps of cw_spread=1 in quads per launch (-1 = the measured ones,
    int cw_spread_cap2 = -1;     // crawford.hip::CW_SPREAD_CAP4 / 2, scaled by the chip's CUs)
    int dipole_stage_mb = 0;    // BSP_DIPOLE_STAGE_MB: > 0 = device scratch of one group of pairs of bspatom_dipole_matrix in MB (0 = 2 GiB); small
                                 // values force several groups (the results do not depend on the grouping: the test's hook)
    int wf_stage_mb = 0;         // BSP_WF_STAGE_MB: > 0 = device staging of bspatom_tabulate / bspatom_wavefunctions (U and dU of one group of vectors,
                                 // one group's eigenvector block) in MB (0 = 256 MiB); small values force several groups (the test's hook)
    int tdse_stage_mb = 0;       // BSP_TDSE_STAGE_MB: > 0 = device staging of bspatom_tdse_propagate's host variant (the field table and the snapshots of one
                                 // group of steps) in MB (0 = 256 MiB); small values force several groups (the test's hook)
    int tdse_adapt_group = 0;    // BSP_TDSE_ADAPT_GROUP: > 0 = attempts that bspatom_tdse_adaptive enqueues between two looks at its control block (0 = 16); the
                                 // result does not depend on it (the test's hook)
    int tdse_spline_group = 0;   // BSP_TDSE_SPLINE_GROUP: > 0 = steps per launch of bspatom_tdse_spline (0 = 64): no launch runs for long; the result does
                                 // not depend on it (the test's hook)
    int tdse_split_group = 0;    // BSP_TDSE_SPLIT_GROUP: > 0 = steps whose launches bspatom_tdse_split enqueues before it waits for them (0 = 64); the result
                                 // does not depend on it (the test's hook)
    int resolvent_stage_mb = 0;  // BSP_RESOLVENT_STAGE_MB: > 0 = bound in MB on the slot scratch of bspatom_resolvent and on the X of one group of matrices
                                 // of its host variant (0 = 2048); one slot and one matrix at least; results do not depend on it (the test's hook)
    int resolvent_slots = 0;     // BSP_RESOLVENT_SLOTS: > 0 = work slots (resident waves) of resolvent_kernel, 0 = the occupancy query x CUs;
                                 // results do not depend on it (the test's hook)
    int window_rhs = 0;          // BSP_WINDOW_RHS: > 0 = right-hand sides that one factorisation of bspatom_spline_window serves in one work item (0 = 8);
                                 // results do not depend on it (the test's hook; 1 = a factorisation per packet, the measurement's baseline)
    int ktime = 0;               // 1: HIP events around every launch of the kernels in KSlot (bspatom_kernel_times; bench.py's
                                 // per-kernel roofline entries are measured with it in one extra, untimed step)
};
Options &opts();

// one process per GPU: the device of the first successfully created problem (capi.hip); -1 while none exists
int process_device();
int process_device_check(int device);          // BSP_OK, or BSP_ERR_UNSUPPORTED (message on stderr) if another device is latched
void process_device_latch(int device);
int device_cus();                              // compute units of the current device, asked once per process (the device is latched); 256 if the query fails

// A kernel's opt-in for `bytes` of dynamic LDS.  A property of the latched device: every caller keeps a once-flag of its own.
template <class K>
inline hipError_t allow_lds(K kernel, size_t bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
// The work slots of a persistent grid: the workgroups of `kernel` (threads, bytes of dynamic LDS) the current device keeps resident
// (the occupancy query x CUs, one each if a query fails), at most `items`.  A wrong estimate costs speed, never progress.
template <class K>
inline int persistent_slots(K kernel, int threads, size_t lds_bytes, int items, int *slots)
{
    int per_cu = 0;
    const int cus = device_cus();
    BSP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, lds_bytes));
    const long r = (long)(per_cu > 0 ? per_cu : 1) * (cus > 0 ? cus : 1);
    *slots = (int)(r < items ? r : items);
    return BSP_OK;
}

// ---- launch-side state: the streams, events and small device blocks the launchers need besides the caller's buffers --------
// One per problem handle (capi_internal.h), one local to every stage-level entry point and to bsp_dsygv_.  Every member is created at
// first need by the launcher that uses it; release() (and the destructor) waits for the streams it owns before it frees anything.
// One host thread per problem: nothing here is locked.
struct Sy2sbLane {                       // one pipeline of sy2sb_run: main + high-priority side stream and their events
    hipStream_t main = nullptr, side = nullptr;
    hipEvent_t evA = nullptr, evB = nullptr, done = nullptr;
};
constexpr int SY2SB_MAXG = 4;
struct LaunchCtx {
    // crawford_run: streams of the further channel groups, fork / join events (re-recorded by every solve)
    hipStream_t cw_aux[3] = {nullptr, nullptr, nullptr};
    hipEvent_t cw_fork = nullptr, cw_join[3] = {nullptr, nullptr, nullptr};
    // sy2sb_run: the lanes and the fork event
    Sy2sbLane lanes[SY2SB_MAXG];
    hipEvent_t sy_fork = nullptr;
    // launch_bisect: rows beyond the LDS (grown on demand), the queue's counters
    double2 *bis_tail = nullptr;
    size_t bis_tail_cap = 0;
    unsigned *bis_qcnt = nullptr;
    // launch_sb2st: the check word of BSP_SB2ST_CHECK
    int *sb2st_chk = nullptr;

    LaunchCtx() = default;
    LaunchCtx(const LaunchCtx &) = delete;
    LaunchCtx &operator=(const LaunchCtx &) = delete;
    ~LaunchCtx() { release(); }
    hipError_t sync();                   // waits for every stream the ctx owns; the first error
    void release();                      // sync(), then destroys / frees everything; the ctx is as new afterwards
};

// ---- per-kernel launch timing (off unless opts().ktime) --------------------------------------------
// Two events per launch, recorded on the launch's own stream; bspatom_kernel_times() sums the elapsed times per slot after
// the device has drained.  Launches of different streams overlap, so the sums of a slot are sums of launch DURATIONS (what
// rocprofv3 --kernel-trace --stats reports), not wall time.
enum KSlot { KS_SYR2K = 0, KS_SYMM, KS_PANEL_QR, KS_CHAIN, KS_SB2SB, KS_SB16ST, KS_BISECT, KS_STDFORM, KS_CRAWFORD, KS_OPBAND, KS_TDSE, KS_COUNT };
void ktime_begin(int slot, hipStream_t st);
void ktime_end(int slot, hipStream_t st);
struct KScope {
    int slot; hipStream_t st; bool on;
    KScope(int slot_, hipStream_t st_) : slot(slot_), st(st_), on(opts().ktime != 0) { if (on) ktime_begin(slot, st); }
    ~KScope() { if (on) ktime_end(slot, st); }
};

// ---- batched fp64 MFMA GEMM: C[b] = alpha * A[b] * B[b] + beta * C[b] ----------------------
// Element (i,k) of A[b] is at A + b*bA + i*sAm + k*sAk (one of sAm, sAk must be 1), likewise
// B(k,j) at B + b*bB + k*sBk + j*sBn and C(i,j) at C + b*bC + i*sCm + j*sCn.
struct GemmDesc {
    int M, N, K, batch;
    const double *A; long sAm, sAk, bA;
    const double *B; long sBk, sBn, bB;
    double *C; long sCm, sCn, bC;
    double alpha, beta;
    int lower_only;   // 1: C is square/symmetric, compute only tiles touching i >= j (col-major C)
    int yoff;         // gemm2 MODE 1: first kernel-view row block (= caller column block) of this launch
    int ksplit;       // gemm_kernel: > 1 = split-K, grid.z = batch * ksplit, slice s covers k in [s*kchunk, (s+1)*kchunk)
    int kchunk;       //              and writes alpha * partial to C + s*bCs (beta ignored); set by gemm_splitk_f64
    long bCs;
    // gemm2 MODE 1: the valid tiles are enumerated in 8 x 8 super-blocks; entry s = super-block (sbx, sby) in tile
    // units / 8, sbpre = number of valid tiles up to and including it (set by syr2k_lower_f64)
    int nsb, toff;           // toff: first tile (of the enumeration) of this launch; lower_only = number of tiles in it
    int sbpre[80];           // dwords: a uniform index then reads them with scalar loads (16-bit entries made the tile search a
    int sbxy[80];            // chain of dependent VECTOR loads, ~3 us at the head of every workgroup); sbxy = sbx | sby << 8
};
int gemm_f64(const GemmDesc &g, hipStream_t st);
// C = alpha * A B + beta * C with the K range cut into `splits` slices that run as separate workgroups (for products
// with a small C and a long K: one tile per channel cannot fill the chip); `part` holds splits * batch * M * N
// doubles; the slices are summed in a fixed order (deterministic).
int gemm_splitk_f64(const GemmDesc &g, int splits, double *part, hipStream_t st);
// C[b] (m x 64) = alpha * A[b] (m x 64) * B[b] (64 x 64, ld 64) + beta * C[b], column-major (gemm_f64.hip)
int tsmm64_f64(int m, int batch, const double *A, long lda, long bsA, const double *B, long bsB, double *C, long ldc, long bsC,
               double alpha, double beta, hipStream_t st);
// pipelined, symmetry-aware products of sy2sb (see gemm_f64.hip)
// part: 0 = all tiles, 1 = only column block 0 (look-ahead part), 2 = column blocks >= 1
// seg / nseg: the launch covers the seg-th of nseg equal slices of the tile enumeration (nseg = 1: all)
int syr2k_lower_f64(int m, int batch, double *A22, long ld, long bsA, const double *buf, long ldb, long bsBuf, int seg, int nseg,
                    int part, hipStream_t st);
int symm_lower_f64(int m, int batch, const double *A22, long ld, long bsA, const double *W, long ldw, long bsW,
                   double *Y, long ldy, long bsY, hipStream_t st);

// ---- stage kernels (launchers) -------------------------------------------------------------
// assemble.hip
int launch_point_table(int nkp, int k, int ka, int nfun, const double *d_rt, const double *d_aind,
                       const double *d_xg, const double *d_wg, const double *d_vpot, double *d_ptab,
                       int *d_left, int *d_status, hipStream_t st);
int launch_assemble_bands(int nfun, int k, int ka, int nkp, int kind_pot, const double *d_bl, int l0,
                          int nl, const double *d_ptab, const int *d_left, double *d_SB, double *d_HB,
                          hipStream_t st);
int launch_dipole_bands(int nfun, int k, int ka, int nkp, const double *d_ptab, const int *d_left, double *d_RB,
                        hipStream_t st);
// bandchol.hip
int launch_band_cholesky(int n, int k, const double *d_SB, double *d_UB, double *d_rdiag, int *d_info,
                         hipStream_t st);
int launch_band_cholesky_range(int n, int k, int jstart, int jstop, const double *d_SB, double *d_UB, double *d_rdiag, int *d_info,
                               hipStream_t st);
int launch_band_cholesky_pair(int n, int k, int jstop, const double *d_SB, double *d_UB, double *d_rdiag, int *d_info, hipStream_t st);
// full = 0: C's lower triangle and first block super-diagonal only (all the reduction reads); 1: the whole matrix
int launch_standard_form(int n, int npad, int k, int nl, const double *d_HB, const double *d_UB,
                         const double *d_rdiag, double *d_Y, double *d_C, hipStream_t st, int full = 0);
// crawford.hip: band route -- the banded pencil to a banded standard-form matrix (half-width 8) without the dense C_l
struct CrawfordWork {
    double *SBf, *UBf, *rdiagf;  // [2][k][n] overlap in reversed order and as it is, their Cholesky factors, [2][n] reciprocal pivots
    double *Qel, *LiB;           // [2][N][256] elimination transforms, [2][N][64] inverse diagonal blocks of L (N = ceil(n / 8))
    double *D, *E, *G;           // [nl][2 (N + 2)][64] diagonal / sub-diagonal blocks of the working matrix, the fill in flight (run from
                                 // both ends: [2 nl][blocks of the longer part + 2][64]); D holds packed lower triangles, 36 doubles a block
    double *U;                   // [2 nl][28] the strict upper triangle of diagonal block 0 (inside D's region, behind the records)
    int *info;                   // device word: order of the minor at which the Cholesky factorisation of the reversed overlap broke down
};
bool crawford_supported(int n, int k);
size_t crawford_work_bytes(int n, int k, int nl);
void crawford_carve(void *base, int n, int k, int nl, CrawfordWork *w);
// the S-only part (run: unless s_prepared).  evc (CW_CHUNKS events, or null): the factor is computed in CW_CHUNKS launches, each followed
// by the elimination transforms of its blocks and by evc[c], so that a run given the same events starts on the first blocks while the
// rest of the factor is still being computed (without them the caller orders the run behind the whole of it)
constexpr int CW_CHUNKS = 4;
int crawford_prepare(int n, int k, const double *d_SB, const CrawfordWork &w, hipStream_t st, hipEvent_t *evc = nullptr);
int crawford_run(LaunchCtx &cx, int n, int npad, int k, int nl, const double *d_SB, const double *d_HB, const CrawfordWork &w, double *d_AB,
                 hipStream_t st, bool s_prepared = false, hipEvent_t *evc = nullptr);
// sy2sb.hip
// tsqr.hip: panel factorisation on many workgroups (TSQR + Householder reconstruction), BSP_PANEL_QR=3
long tsqr_scr_doubles(int npad);
long tsqr_cntr_ints(int npad);
int tsqr_panel(int npad, int r0, int c0, int batch, double *d_A, double *buf, double *W, double *scr, int *cntr, hipStream_t st);
struct Sy2sbWork {
    double *tsqr_scr;   // [batch][tsqr_scr_doubles(npad)]
    int *tsqr_cntr;     // [batch][tsqr_cntr_ints(npad)], zeroed at the start of every sy2sb_run
    double *buf2;   // second [V | Z | V] set (panels alternate: look-ahead QR writes one while the update reads the other)
    double *tau2;
    double *buf;    // [batch][npad][3*nb]  : [V | Z | V]
    double *W;      // [batch][npad][nb]
    double *G;      // [batch][nb][nb]
    double *T;      // [batch][nb][nb]
    double *Kmat;   // [batch][nb][nb]
    double *tau;    // [batch][nb]
    double *part;   // [SY2SB_SPLITK][batch][nb][nb] split-K partial sums of G and K
};
constexpr int SY2SB_SPLITK = 16;
size_t sy2sb_work_bytes(int npad, int nb, int batch);
void sy2sb_carve(void *base, int npad, int nb, int batch, Sy2sbWork *w);
int sy2sb_run(LaunchCtx &cx, int npad, int nb, int batch, double *d_A, const Sy2sbWork &w, hipStream_t st);
int sy2sb_panel_only(int npad, int c0, int batch, double *d_A, const Sy2sbWork &w, hipStream_t st);
int launch_extract_band(int npad, int nb, int batch, const double *d_A, double *d_AB, hipStream_t st);
// sb2st.hip
// ctl: device scratch of sb2st_ctl_bytes(batch) bytes owned by the caller (per problem)
size_t sb2st_ctl_bytes(int batch);
// two-step route (sbr2.hip): band 64 -> 16 by block bulge chasing, then 16 -> tridiagonal in an LDS window
int launch_sb2sb(int n, int npad, int batch, double *d_AB, hipStream_t st);
int launch_sb16st(int n, int npad, int batch, double *d_AB, double *d_d, double *d_e, hipStream_t st, int *d_status, void *ctl, int hb = 16);
int launch_sb2st(LaunchCtx &cx, int n, int npad, int b, int batch, double *d_AB, double *d_d, double *d_e, hipStream_t st, int *d_status,
                 void *ctl);
// tridiag.hip
int launch_bisect(LaunchCtx &cx, int n, int ldn, int batch, const double *d_d, const double *d_e, double *d_w, long ldw, hipStream_t st);
int launch_bisect_one(int n, const double *d_d, const double *d_e, int m, double *d_out, hipStream_t st);
// bandsect.hip: eigenvalue m (0-based, ascending) of the banded pencil itself (upper bands, k - 1 <= 8), one workgroup
int launch_band_multisect(int n, int k, const double *d_SB, const double *d_HB, int m, double *d_out, hipStream_t st);
// eigvec.hip: that eigenvalue and its eigenvector in one launch of one workgroup (d_HB: the channel's own band; d_work: invit_work_doubles
// for one vector).  own_cu: the workgroup asks for OWN_CU_LDS bytes of LDS, so that nothing of the band route's kernels fits beside it
constexpr size_t OWN_CU_LDS = 144 * 1024;           // of 160 KB: 16 KB left
int launch_early_vector(int n, int k, const double *d_SB, const double *d_HB, int m, double *d_E, double *d_work, double *d_vec,
                        int *d_info, hipStream_t st, bool own_cu);
// eigvec.hip
// vector iv: channel chan[iv] of HB (HB + chan*k*n), eigenvalue E[iv]; work: nvec*invit_work_doubles; d_start (or null): start[iv]
// = 0 for the constant start vector, r > 0 for member r of a run of coinciding eigenvalues, whose r predecessors are the vectors in
// front of it in d_vec; one launch computes the vectors with start[iv] == rank, rank r after rank r - 1 (eigvec.hip::invit_kernel)
int launch_inverse_iteration(int n, int k, int nvec, const double *d_SB, const double *d_HB,
                             const int *d_chan, const double *d_E, double *d_work, double *d_vec,
                             int *d_info, hipStream_t st, const int *d_start = nullptr, int rank = 0);
size_t invit_work_doubles(int n, int k);
// the same vectors for a channel range, persistent grid (invit_batch_kernel): item it = c * count + j is eigenvalue E[c*n + j] of
// channel c (HB + c*k*n), vector at d_vec + it*n; d_work: slots * invit_batch_slot_doubles, slots from invit_batch_slots
size_t invit_batch_slot_doubles(int n, int k);
int invit_batch_slots(int k, int items, int *slots);
int launch_inverse_iteration_batch(int n, int k, int count, int items, int slots, const double *d_SB, const double *d_HB,
                                   const double *d_E, double *d_work, double *d_vec, int *d_info, hipStream_t st);
int launch_band_apply(int n, int k, const double *d_RB, const double a[3], const double *d_x, double *d_v, hipStream_t st);
int launch_dots(int n, int m, const double *d_Z, const double *d_v, double *d_D, hipStream_t st);
// dipole.hip: dipole matrix blocks of many channel pairs (bspatom_dipole_matrix)
// W[q][j][:] = (a[3q] R_r + a[3q+1] R_1/r + a[3q+2] R_d/dr) x_j for the `count` vectors at d_base + d_xoff[q] of each of nitems
// items, every column bit-identical to launch_band_apply's
int launch_band_apply_block(int n, int k, int count, int nitems, const double *d_RB, const double *d_acoef, const long long *d_xoff,
                            const double *d_base, double *d_W, hipStream_t st);
// K slices of one pair's product, a rule in (n, count_ini, count_fin) alone
void dipole_kslices(int n, int count_ini, int count_fin, int *chunk, int *nslices);
// d_out[p][i][f] = W_p[i][:] . Z_p[f][:] for npairs pairs on one grid; W_p at d_base + d_pw[2p] ([count_ini][n]), Z_p at
// d_base + d_pw[2p+1] ([count_fin][n]); d_part: npairs * nslices * count_ini * count_fin doubles when nslices > 1 (summed in slice order)
int launch_dipole_block(int n, int count_ini, int count_fin, int npairs, const long long *d_pw, const double *d_base, double *d_part,
                        double *d_out, hipStream_t st);
// opmat.hip: bands and pair blocks of caller-given radial operators (bspatom_operator_bands / bspatom_operator_matrix)
// d_GB[(o*(2k-1) + (d+k-1))*nfun + i] = sum_q B_i(r_q) g_o(q) X_j(r_q) w_q, j = i + d, X = B (d_deriv[o] == 0) or B' (1); d_g[nop][nr] on the
// quadrature grid of wf_quadrature, d_qfirst[nkp-1]: quadrature index of every knot interval's first point, -1 for zero width
int launch_operator_bands(int nfun, int k, int ka, int nkp, int nop, int nr, const double *d_ptab, const int *d_left,
                          const int *d_qfirst, const double *d_g, const int *d_deriv, double *d_GB, hipStream_t st);
// launch_band_apply_block with nop coefficients per item: W[q][j][:] = (sum_o a[q*nop + o] G_o) x_j, entries of the sum formed for o
// ascending, rows over diagonals ascending, no FMA
int launch_band_combine_apply(int n, int k, int nop, int count, int nitems, const double *d_GB, const double *d_acoef,
                              const long long *d_xoff, const double *d_base, double *d_W, hipStream_t st);
// resolvent.hip: (H_l - i W_w - z S) x = b for nmat matrices (bspatom_resolvent).  Matrix m: channel chan[m] of HB (HB + chan*k*n),
// z = (z[2m], z[2m+1]), absorber band WB + w[m]*(2k-1)*n (w null or w[m] < 0: none).  B: nrhs, P: nproj vectors of n complex;
// X[m][r][n], R[m][r][nproj] complex (either may be null); info[m]: pivots replaced.  Every pointer is device memory.
// work: slots * resolvent_slot_doubles (16-byte aligned), slots at most resolvent_slots.
struct ResolventArgs {
    int n, k, nmat, nrhs, nproj;
    const double *SB, *HB;
    const int *chan;
    const double *z, *WB;
    const int *w;
    const double *B, *P;
    double *X, *R;
    int *info;
    double *work;
};
size_t resolvent_slot_doubles(int n, int k);
int resolvent_slots(int k, int nmat, int *slots);
int launch_resolvent(const ResolventArgs &a, int slots, hipStream_t st);
// Chains of resolvents (bspatom_resolvent_chain): matrix (c, s) is entry c*nstage + s of chan, z, w, info; x_{c,0,r} = M^-1 B_r,
// x_{c,s,r} = M_{c,s}^-1 (A_{c,s} x_{c,s-1,r}), A_{c,s} = sum_o acoef[(c*(nstage-1) + s-1)*nop + o] G_o, GB nop full bands
// [2k-1][n] (nstage == 1: GB, acoef unused).  R[c][s][r][nproj] of every stage, X[c][r][n] of the last (either may be null).
// work: slots * resolvent_chain_slot_doubles(n, k, nrhs): resolvent_slot_doubles, then the nrhs vectors of the previous stage.
struct ResolventChainArgs {
    int n, k, nchain, nstage, nop, nrhs, nproj;
    const double *SB, *HB;
    const int *chan;
    const double *z, *WB;
    const int *w;
    const double *GB, *acoef;
    const double *B, *P;
    double *X, *R;
    int *info;
    double *work;
};
size_t resolvent_chain_slot_doubles(int n, int k, int nrhs);
int resolvent_chain_slots(int k, int nchain, int *slots);
int launch_resolvent_chain(const ResolventChainArgs &a, int slots, hipStream_t st);
// resolvent_coupled.hip: nch channels coupled in one banded LU (bspatom_resolvent_coupled).  Matrix m: channel c is entry m*nch + c
// of chan, z (complex) and w (-1: no absorber; never null here); coupling entry p adds sum_o acoef[(m*ncoup + p)*nop + o] (complex)
// G_o, or its transpose where ctr[p], to block (cr[p], cc[p]).  B: nrhs, P: nproj vectors of nch*n complex, channel-major;
// X[m][r][nch][n], R[m][r][nproj] complex (either may be null).  Every pointer is device memory.
// work: slots * resolvent_coupled_slot_doubles (16-byte aligned), slots at most resolvent_coupled_slots.
struct ResolventCoupledArgs {
    int n, k, nch, nmat, nrhs, nproj, ncoup, nop;
    const double *SB, *HB;
    const int *chan;
    const double *z, *WB;
    const int *w;
    const int *cr, *cc, *ctr;
    const double *GB, *acoef;
    const double *B, *P;
    double *X, *R;
    int *info;
    double *work;
};
int resolvent_coupled_max_band();              // half-width limit of the coupled matrix, nch*k - 1 (BSPATOM_COUPLED_MAX_BAND)
size_t resolvent_coupled_slot_doubles(int n, int k, int nch);
int resolvent_coupled_slots(int k, int nch, int nmat, int *slots);
int launch_resolvent_coupled(const ResolventCoupledArgs &a, int slots, hipStream_t st);
// resolvent_wide.hip: the same system and arguments in a blocked LU for half-widths up to BSPATOM_COUPLED_WIDE_MAX_BAND
// (bspatom_resolvent_coupled_wide); work: slots * resolvent_wide_slot_doubles, which counts the nrhs vectors of a slot too
int resolvent_wide_max_band();
size_t resolvent_wide_slot_doubles(int n, int k, int nch, int nrhs);
int resolvent_wide_slots(int k, int nch, int nmat, int *slots);
int launch_resolvent_wide(const ResolventCoupledArgs &a, int slots, hipStream_t st);
// tdse_spline.hip: Crank-Nicolson steps in the spline basis on resolvent_coupled.hip's LU (bspatom_tdse_spline).  m describes the
// matrix as for launch_resolvent_coupled with ONE record of channels: chan, w [nch], z [nch] = (0, 2/dt); acoef: the coefficients of
// this launch's first step, [step][scan][ncoup][nop] complex; P, nproj: the projections of the rows; info [nscan]: the launch ADDS
// its replaced pivots; work: slots * resolvent_coupled_slot_doubles.  m.nmat, m.nrhs, m.B, m.X, m.R are not read.
// The launch runs steps n0 .. n0 + nst - 1 of every scan on c [nscan][nch][n] complex.  snap (or null): the snapshot after step n,
// (n + 1) % snap_every == 0, goes to snapshot (n + 1) / snap_every - 1 - s0 of snap [.][nscan][nch][n].  obs (or null): the row of
// step n, n % obs_every == 0, goes to row n / obs_every - j0 of obs [.][nscan][nch + 2 nproj]; with fin != 0 the packets after the
// launch's last step are measured into row jfin - j0 (nst = 0: a launch that only measures).
struct TdseSplineArgs {
    ResolventCoupledArgs m;
    int nscan, n0, nst, snap_every, s0, obs_every, j0, fin, jfin;
    double g;                                  // 4 / dt
    double *c, *snap, *obs;
};
int tdse_spline_slots(int k, int nch, int nscan, int *slots);
int launch_tdse_spline(const TdseSplineArgs &a, int slots, hipStream_t st);
// tdse_spline_wide.hip: the same steps and arguments on resolvent_wide.hip's blocked LU, half-widths up to BSPATOM_COUPLED_WIDE_MAX_BAND
// (bspatom_tdse_spline_wide); work: slots * resolvent_wide_slot_doubles(n, k, nch, 1)
int tdse_spline_wide_slots(int k, int nch, int nscan, int *slots);
int launch_tdse_spline_wide(const TdseSplineArgs &a, int slots, hipStream_t st);
// tdse_split.hip: split Crank-Nicolson steps in the spline basis (bspatom_tdse_split), one wave per (scan, channel) system of
// half-width k - 1.  fac [nch]: the channel's atomic factorisation among the nfac distinct ones, which are described by fchan, fw
// [nfac] -- the band in HB and the absorber (-1: none) -- and kept in fstore (nfac * tdse_split_factor_doubles; finfo [nfac]: their
// replaced pivots).  GB: ONE full band; Q [nch][nch], lam [nch]; f: the field of this launch's step, [nscan] complex.
// g = 8 / dt, zi = 4 / dt, h = dt / 2.  in, out: the packets [nscan][nch][n] complex, 16-byte aligned, never the same buffer.
// row (or null): this step's row [nscan][nch + 2 nproj]; part: [nscan][nproj][nch] complex between the atomic and the field launch;
// snap (or null): a copy of out [nscan][nch][n]; pinfo [nscan][nch]: the field launch ADDS its replaced pivots.
// work: slots * tdse_split_slot_doubles.  launch_tdse_split's what: 0 the atomic factorisations, 1 an atomic half step (mix: its
// input mixed with Q), 2 a field step; measure: the row alone.
struct TdseSplitArgs {
    int n, k, nch, nscan, nproj, nfac, mix, measure;
    const double *SB, *HB, *WB, *GB;
    const int *fac, *fchan, *fw;
    const double *Q, *lam, *f, *P;
    double g, zi, h;
    const double *in;
    double *out, *snap, *row, *part, *fstore;
    int *finfo, *pinfo;
    double *work;
};
int tdse_split_max_k();                        // the one-wave window's limit on k
size_t tdse_split_factor_doubles(int n, int k);
size_t tdse_split_slot_doubles(int n, int k);
int tdse_split_slots(int k, int items, int *slots);
int launch_tdse_split(const TdseSplitArgs &a, int what, int slots, hipStream_t st);
// spline_expect.hip: e(q, o) = sum_c conj(c_c)^T G_o (sum_c' B_o(c, c') c_c') on packets in the spline basis (bspatom_spline_expect).
// GE: nexp full bands [2k-1][n]; the rows of the angular matrices compacted by the host: row r = o*nch + c holds its non-zero entries
// rptr[r] .. rptr[r+1]-1, cidx ascending, cval; c: the packets [nscan][nch][n] complex, 16-byte aligned; part: [nscan][nexp][nch]
// complex, one partial per item, between the two launches; e: [nscan][nexp] complex; work: slots * spline_expect_slot_doubles.
struct SplineExpectArgs {
    int n, k, nch, nscan, nexp;
    const double *GE;
    const int *rptr, *cidx;
    const double *cval;
    const double *c;
    double *part, *e;
    double *work;
};
size_t spline_expect_slot_doubles(int n);
int spline_expect_slots(int items, int *slots);
int launch_spline_expect(const SplineExpectArgs &a, int slots, hipStream_t st);
// out [nrows][rw0 + 2 nexp] = row0 [nrows][rw0] beside e [nrows][2 nexp]: the rows of bspatom_tdse_split_observe
int launch_spline_expect_rows(double *out, const double *row0, const double *e, int rw0, int nexp, int nrows, hipStream_t st);
// spline_window.hip: N(q, c, e) = x^H S x, x = prod_j (H_l - z_{e,j} S)^-1 S applied to packet (q, c) (bspatom_spline_window).  The
// channels' ng distinct bands: gchan [ng], the place in HB.  rhs: the packets q * nch + c grouped by band; block blk of the nblk
// blocks is bn[blk] <= wrhs of them from rhs[b0[blk]] on, all of band bg[blk]; bhead[blk]: the first block of its band.  An item is
// (e, blk).  z: [ne][nfac] complex; c: [nscan][nch][n] complex, 16-byte aligned; N: [nscan][nch][ne]; info: [ne][ng][nfac], the
// replaced pivots of every factorisation, written by the head blocks.  work: slots * spline_window_slot_doubles(n, k, wrhs).
struct SplineWindowArgs {
    int n, k, ne, nfac, ng, nblk, wrhs;
    const double *SB, *HB;
    const int *gchan, *rhs, *bg, *b0, *bn, *bhead;
    const double *z, *c;
    double *N;
    int *info;
    double *work;
};
size_t spline_window_slot_doubles(int n, int k, int wrhs);
int spline_window_slots(int k, int items, int *slots);
int launch_spline_window(const SplineWindowArgs &a, int slots, hipStream_t st);
int launch_wf_tabulate(int nkp, int k, int n, const double *d_rt, const double *d_c, double ra,
                       double rb, int npts, double *d_r, double *d_u, int *d_status, hipStream_t st);
// wavefn.hip: u(r), u'(r) of blocks of coefficient vectors (bspatom_tabulate, bspatom_wavefunctions)
// host: points / weights of the assembly's quadrature on the intervals of positive width and their rows of the point table
int wf_quadrature(int nkp, int ka, const double *rt, const double *xg, const double *wg, int *rows, double *r, double *w);
bool wf_points_valid(int nkp, const double *rt, int npts, const double *r);
// basis table of a call, point index fastest: d_tab[j * npts + ip] (j < k: B, k <= j < 2k: B'), d_tleft[ip] = left
int launch_basis_table(int nkp, int k, int nfun, int npts, const double *d_rt, const double *d_aind, const double *d_r, double *d_tab,
                       int *d_tleft, int *d_status, hipStream_t st);
int launch_basis_gather(int k, int npts, const int *d_rows, const double *d_ptab, const int *d_pleft, double *d_tab, int *d_tleft,
                        hipStream_t st);
// d_U[v * npts + ip] = sum_j d_Z[v * nfun + j] B_j(r_ip), d_dU likewise with B' (null: values only)
int launch_tabulate(int k, int nfun, int npts, int nvec, const double *d_tab, const int *d_tleft, const double *d_Z, double *d_U,
                    double *d_dU, hipStream_t st);
// tdse.hip: the TDSE in the eigenstate basis (bspatom_tdse_propagate).  Working layout of the amplitudes: [nch][count][NC] real,
// column 2q / 2q + 1 = Re / Im of scan q, NC = tdse_columns(nscan) (2 nscan rounded up to 16, the rest zero)
struct TdseDims { int nch, count, nscan, NC; };
struct TdseBufs {
    const int *cptr, *ent;       // entries cptr[c] .. cptr[c+1]-1 of channel c, ascending p: ent[3e] = p, [3e+1] = the other channel, [3e+2] = 1 if c = ci[p]
    const double *E, *D;         // [nch][count]; [npairs][count][count]
    double *a, *K;               // working amplitudes; the six k_s, each nch * count * NC doubles
    unsigned long long *err2;    // [nscan] bit patterns of max |sum_s (d_s - b_s) k_s|^2, zeroed by the caller
    double *part;                // observables: [nch][ceil(count / 64)][NC / 2][4] partials of the row tiles (null: nothing is observed)
    const double *ph;            // Lawson steps: [5][nch][count][2] cos, sin of E c_s dt, s = 1 .. 5 (launch_tdse_phases); null: the plain scheme
    // bspatom_tdse_static: W = [nstat][count][count] static blocks, whose entries follow a channel's driven ones in ent, [3e] = j,
    // [3e+1] = si[j], [3e+2] = 2 + skind[j], and part is 6 doubles wide (null: no static entry, the kernels of the other calls);
    // ow = doubles per (scan, channel) of a row of observables, 4 or 6
    const double *W = nullptr;
    int ow = 4;
    // bspatom_tdse_fields with nf > 1 drive fields: a driven entry's [3e+2] is 4 g + {0, 1}, g its field; the field table of a stage
    // is [nf][nscan][2]; part and the rows are ow = 4 + 2 nf doubles wide, and the kernels of tdse_fields.hip run, with or without W
    int nf = 1;
};
int tdse_columns(int nscan);
// one step: six stage launches and the step kernel; d_field: the 6 * w.nf * nscan complex values of this step; d_snap: null, or where the
// new amplitudes go in the caller's layout [nscan][nch][count] complex; d_obs: null, or where the observables of the amplitudes
// BEFORE the step go, [nscan][nch][4] (then stage 0 is the observing kernel, followed by the reduction: eight launches)
int launch_tdse_step(const TdseDims &d, const TdseBufs &w, const double *d_field, double dt, double *d_snap, double *d_obs, hipStream_t st);
// the observables of w.a into d_row [nscan][nch][4]: tdse_observe_kernel and the reduction of its row-tile partials.  d_field: the
// stage-0 field of a step that follows, whose k_0 the kernel then leaves exactly as the plain stage does; null: the measurement alone
int launch_tdse_observe(const TdseDims &d, const TdseBufs &w, const double *d_field, double *d_row, hipStream_t st);
// the phase table of bspatom_tdse_lawson from d_E, once per call
int launch_tdse_phases(const TdseDims &d, const double *d_E, double dt, double *d_ph, hipStream_t st);
// (with w.W set, w.ow = 6 or w.nf > 1 these launch the kernels of tdse_static.hip and tdse_fields.hip: tdse_launch.h)
int launch_tdse_pack(const TdseDims &d, const double *d_user, double *d_work, hipStream_t st);
int launch_tdse_unpack(const TdseDims &d, const double *d_work, double *d_user, hipStream_t st);

// tdse_adapt.hip: bspatom_tdse_adaptive.  The control block in device memory: this header, then at TDSE_CTL_HDR bytes the six field
// values per scan of the coming attempt, fld[(s nscan + q) 2 + {0, 1}], then errmax[nscan], the largest estimate of an accepted step.
// Only tdse_adapt_control_kernel writes it on the device; the host writes it between groups of launches, after the stream has drained.
struct TdseAdaptCtl {
    int n, m, j;                  // the coming attempt: coarse step, level, position
    int flag;                     // the decision of the last attempt: 0 rejected, 1 accepted, 2 forced; -1 before the first
    int done;                     // n == nend: every launch behind it returns at its first instruction
    int nend;                     // the end of the group of coarse steps that is staged
    int row, snap;                // where the row of the coming attempt goes / the snapshot of the accepted one, within the group; -1: none
    int row0, snap0, node0;       // the group's first row, snapshot and field node
    int pad_;
    long long acc_t;              // the number of the last accepted attempt (tdse_adapt_commit_kernel compares its own with it), -1
    long long stats[6];           // accepted, rejected, forced, deepest level, (level at the end: m), attempts
};
constexpr size_t TDSE_CTL_HDR = 128;
static_assert(sizeof(TdseAdaptCtl) <= TDSE_CTL_HDR, "the arrays of the control block start behind its header");
inline size_t tdse_ctl_bytes(int nscan) { return TDSE_CTL_HDR + (size_t)13 * nscan * sizeof(double); }
__host__ __device__ inline const double *tdse_ctl_fld(const TdseAdaptCtl *c) { return (const double *)((const char *)c + TDSE_CTL_HDR); }
// what the controller is given besides the block; the log arrays may be null (log_cap = 0)
struct TdseAdaptArgs {
    int nsub, max_level, snap_every, obs_every, log_cap;
    double dt, tol;
    const double *fn;             // the nodes of the staged group, from node0 on
    int *log_i;
    double *log_e, *log_f;
};
// the field of the attempt (n, m, j) of a fresh block or a new group: the controller's last part alone
int launch_tdse_adapt_init(const TdseDims &d, const TdseBufs &w, TdseAdaptCtl *ctl, const TdseAdaptArgs &g, hipStream_t st);
// one attempt, number t: six stages (stage 0 observing, with the reduction to the row ctl->row of d_obs, when d_obs is given), the step into
// the candidate buffer cand, the controller, the commit (a, and the snapshot ctl->snap of d_snap).  w.ph: one table per level, phlev doubles each
int launch_tdse_adapt_attempt(const TdseDims &d, const TdseBufs &w, TdseAdaptCtl *ctl, const TdseAdaptArgs &g, long long t, double *cand,
                              size_t phlev, double *d_snap, double *d_obs, hipStream_t st);

// capi.hip: enqueue Cholesky -> standard form -> sy2sb -> sb2st -> bisection on `st` for nl channels
// whose upper bands are already in d_SB / d_HB.  ev (optional): 5 events recorded at the stage
// boundaries [after chol+std, after sy2sb, after sb2st, after bisect] starting from ev[0] = begin.
struct PipeBufs {
    double *UB, *rdiag, *Y, *C, *AB, *d, *e;
    void *work;
    int *info;
    int *status = nullptr;   // device word set to a BSP_ERR_* code by kernels that detect a failure
    void *sbctl = nullptr;   // sb2st pairing/progress control block (sb2st_ctl_bytes(nl))
    void *cwork = nullptr;   // band route: crawford_work_bytes(n, k, nl); Y, C, work may be null when only that route runs
    hipEvent_t *s_events = nullptr;   // band route, S-only part already enqueued elsewhere (s_prepared): CW_CHUNKS events, see crawford_prepare
    hipEvent_t chase_after = nullptr; // band route: the chase waits for this event (the early vector's kernels hold LDS two workgroups of the chase need)
};
// 1 = dense route, 2 = band route, for a pencil of this size under the current switches (BSP_ROUTE)
int pipeline_route(int n, int k);
size_t pipe_bytes_per_channel(int npad);
int pipeline_enqueue(LaunchCtx &cx, int n, int npad, int k, int nl, const double *d_SB, const double *d_HB,
                     const PipeBufs &b, double *d_Eout, hipStream_t st, hipEvent_t *ev, bool with_bisect = true, bool s_prepared = false);

}  // namespace bsp
