// capi_stage.hip -- the stage-level entry points of the C ABI (include/bspatom.h: bspatom_stage_*): one kernel stage on host
// arrays, for the tests.  Each call uploads, runs on the null stream, waits and downloads; nothing here belongs to a problem: a call
// that needs launch-side state holds a LaunchCtx of its own, declared behind its arrays (so it is released, its streams drained, first).
#include "capi_internal.h"

using namespace bsp;

static int need_gpu()
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        fprintf(stderr, "bspatom: no HIP device (libbspatom has no CPU path)\n");
        return BSP_ERR_NOGPU;
    }
    return BSP_OK;
}

// the bands of `batch` matrices between the host layout, dense [batch][npad][128], and the device layout, ab_stride(npad) apart
static int copy_band_in(int npad, int batch, const double *AB, double *d_AB)
{
    for (int b = 0; b < batch; ++b)
        BSP_HIP(hipMemcpy(d_AB + b * ab_stride(npad), AB + (size_t)b * npad * 128, (size_t)npad * 128 * sizeof(double), hipMemcpyHostToDevice));
    return BSP_OK;
}
static int copy_band_out(int npad, int batch, const double *d_AB, double *AB)
{
    for (int b = 0; b < batch; ++b)
        BSP_HIP(hipMemcpy(AB + (size_t)b * npad * 128, d_AB + b * ab_stride(npad), (size_t)npad * 128 * sizeof(double), hipMemcpyDeviceToHost));
    return BSP_OK;
}

extern "C" int bspatom_stage_gemm(int M, int N, int K, int batch, const double *A, long sAm, long sAk, long bA,
                                  long lenA, const double *B, long sBk, long sBn, long bB, long lenB, double *C,
                                  long sCm, long sCn, long bC, long lenC, double alpha, double beta)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    DevArray<double> dA, dB, dC;
    if ((rc = dA.put(A, lenA)) || (rc = dB.put(B, lenB)) || (rc = dC.put(C, lenC))) return rc;
    GemmDesc g{};
    g.M = M; g.N = N; g.K = K; g.batch = batch;
    g.A = dA.p; g.sAm = sAm; g.sAk = sAk; g.bA = bA;
    g.B = dB.p; g.sBk = sBk; g.sBn = sBn; g.bB = bB;
    g.C = dC.p; g.sCm = sCm; g.sCn = sCn; g.bC = bC;
    g.alpha = alpha; g.beta = beta; g.lower_only = 0;
    if ((rc = gemm_f64(g, 0))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    return dC.get(C, lenC);
}

extern "C" int bspatom_stage_standard_form(int n, int k, int nl, const double *SB, const double *HB, double *UB,
                                           double *C, int32_t *info)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    const int np = round_up(n, 64);
    DevArray<double> dSB, dHB, dUB, dr, dY, dC;
    DevArray<int> dinfo;
    if ((rc = dSB.put(SB, (size_t)k * n)) || (rc = dHB.put(HB, (size_t)nl * k * n)) || (rc = dUB.alloc((size_t)k * n)) ||
        (rc = dr.alloc(n)) || (rc = dY.alloc((size_t)nl * np * np)) || (rc = dC.alloc((size_t)nl * np * np)) ||
        (rc = dinfo.alloc(1))) return rc;
    BSP_HIP(hipMemset(dinfo.p, 0, sizeof(int)));
    BSP_HIP(hipMemset(dY.p, 0, (size_t)nl * np * np * sizeof(double)));
    if ((rc = launch_band_cholesky(n, k, dSB.p, dUB.p, dr.p, dinfo.p, 0))) return rc;
    if ((rc = launch_standard_form(n, np, k, nl, dHB.p, dUB.p, dr.p, dY.p, dC.p, 0, 1))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    int hi = 0;
    if ((rc = dinfo.get(&hi, 1))) return rc;
    if (info) *info = hi;
    if (UB && (rc = dUB.get(UB, (size_t)k * n))) return rc;
    return dC.get(C, (size_t)nl * np * np);
}

extern "C" int bspatom_stage_sy2sb(int npad, int batch, const double *A, double *AB)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    if (npad % 64) return BSP_ERR_ARG;
    DevArray<double> dA, dAB;
    DevArray<char> work;
    if ((rc = dA.put(A, (size_t)batch * npad * npad)) || (rc = dAB.alloc((size_t)batch * ab_stride(npad))) ||
        (rc = work.alloc(sy2sb_work_bytes(npad, 64, batch)))) return rc;
    LaunchCtx cx;
    Sy2sbWork w;
    sy2sb_carve(work.p, npad, 64, batch, &w);
    rc = sy2sb_run(cx, npad, 64, batch, dA.p, w, 0);
    if (!rc) rc = launch_extract_band(npad, 64, batch, dA.p, dAB.p, 0);
    const hipError_t e = hipDeviceSynchronize();          // on every path, before the work area is freed
    if (rc) return rc;
    BSP_HIP(e);
    return copy_band_out(npad, batch, dAB.p, AB);
}

extern "C" int bspatom_stage_panel(int npad, int c0, int batch, double *A, double *V, double *W)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    if (npad % 64 || c0 % 64 || c0 + 128 > npad || batch < 1) return BSP_ERR_ARG;
    const int m = npad - c0 - 64;
    DevArray<double> dA;
    DevArray<char> work;
    if ((rc = dA.put(A, (size_t)batch * npad * npad)) || (rc = work.alloc(sy2sb_work_bytes(npad, 64, batch)))) return rc;
    BSP_HIP(hipMemset(work.p, 0, sy2sb_work_bytes(npad, 64, batch)));
    Sy2sbWork w;
    sy2sb_carve(work.p, npad, 64, batch, &w);
    rc = sy2sb_panel_only(npad, c0, batch, dA.p, w, 0);
    const hipError_t e = hipDeviceSynchronize();          // on every path, before the work area is freed
    if (rc) return rc;
    BSP_HIP(e);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < 64; ++c) {          // column c of V (first slot of [V | Z | V]) and of W, rows 0 .. m-1
            BSP_HIP(hipMemcpy(V + ((size_t)b * 64 + c) * m, w.buf + (size_t)b * npad * 192 + (size_t)c * npad, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
            BSP_HIP(hipMemcpy(W + ((size_t)b * 64 + c) * m, w.W + (size_t)b * npad * 64 + (size_t)c * npad, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
        }
    return dA.get(A, (size_t)batch * npad * npad);
}

extern "C" int bspatom_stage_sb2st(int n, int npad, int batch, const double *AB, double *d, double *e)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    DevArray<double> dAB, dd, de;
    DevArray<char> ctl;
    if ((rc = dAB.alloc((size_t)batch * ab_stride(npad))) || (rc = copy_band_in(npad, batch, AB, dAB.p)) ||
        (rc = dd.alloc((size_t)batch * npad)) || (rc = de.alloc((size_t)batch * npad)) || (rc = ctl.alloc(sb2st_ctl_bytes(batch)))) return rc;
    LaunchCtx cx;
    if ((rc = launch_sb2st(cx, n, npad, 64, batch, dAB.p, dd.p, de.p, 0, nullptr, ctl.p))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    if ((rc = dd.get(d, (size_t)batch * npad))) return rc;
    return de.get(e, (size_t)batch * npad);
}

extern "C" int bspatom_stage_sb2sb(int n, int npad, int batch, double *AB)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    DevArray<double> dAB;
    if ((rc = dAB.alloc((size_t)batch * ab_stride(npad))) || (rc = copy_band_in(npad, batch, AB, dAB.p))) return rc;
    if ((rc = launch_sb2sb(n, npad, batch, dAB.p, 0))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    return copy_band_out(npad, batch, dAB.p, AB);
}

extern "C" int bspatom_stage_crawford(int n, int k, int nl, const double *SB, const double *HB, double *AB, int32_t *info)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    if (n < 1 || k < 2 || nl < 1 || !SB || !HB || !AB) return BSP_ERR_ARG;
    if (!crawford_supported(n, k)) return BSP_ERR_UNSUPPORTED;
    const int npad = round_up(n, 64);
    DevArray<double> dSB, dHB, dAB, dW;
    if ((rc = dSB.put(SB, (size_t)k * n)) || (rc = dHB.put(HB, (size_t)nl * k * n)) || (rc = dAB.alloc((size_t)nl * ab_stride(npad))) ||
        (rc = dW.alloc(crawford_work_bytes(n, k, nl) / sizeof(double) + 1))) return rc;
    BSP_HIP(hipMemset(dAB.p, 0, (size_t)nl * ab_stride(npad) * sizeof(double)));
    LaunchCtx cx;
    CrawfordWork cw;
    crawford_carve(dW.p, n, k, nl, &cw);
    if ((rc = crawford_run(cx, n, npad, k, nl, dSB.p, dHB.p, cw, dAB.p, 0))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    int ci = 0;
    BSP_HIP(hipMemcpy(&ci, cw.info, sizeof(int), hipMemcpyDeviceToHost));
    if (info) *info = ci;
    return copy_band_out(npad, nl, dAB.p, AB);
}

extern "C" int bspatom_stage_band_eigenvalue(int n, int k, const double *SB, const double *HB, int m, double *lambda)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    if (!SB || !HB || !lambda || n < 1) return BSP_ERR_ARG;
    DevArray<double> dS, dH, dl;
    if ((rc = dS.put(SB, (size_t)k * n)) || (rc = dH.put(HB, (size_t)k * n)) || (rc = dl.alloc(1))) return rc;
    if ((rc = launch_band_multisect(n, k, dS.p, dH.p, m, dl.p, 0))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    return dl.get(lambda, 1);
}

extern "C" int bspatom_stage_bisect(int n, int batch, const double *d, const double *e, double *w)
{
    int rc;
    if ((rc = need_gpu())) return rc;
    DevArray<double> dd, de, dw;
    if ((rc = dd.put(d, (size_t)batch * n)) || (rc = de.put(e, (size_t)batch * n)) || (rc = dw.alloc((size_t)batch * n))) return rc;
    LaunchCtx cx;
    if ((rc = launch_bisect(cx, n, n, batch, dd.p, de.p, dw.p, n, 0))) return rc;
    BSP_HIP(hipDeviceSynchronize());
    return dw.get(w, (size_t)batch * n);
}
