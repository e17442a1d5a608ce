// C ABI of the device-math probe (include/bfgx.h, "device math probe"); included by bfgx_api.hip.

extern "C" int bfgx_math_probe(int device, int32_t fn, int64_t n, const double *a, const double *b, double *out0, double *out1)
{
    if (fn < 0 || fn >= kProbeCount) return fail(BFGX_ERR_INVALID, "math probe: unknown function id %d", (int)fn);
    if (!a || !out0 || (probe_two_args(fn) && !b) || (probe_two_results(fn) && !out1)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < 0 || n > kProbeMaxN) return fail(BFGX_ERR_INVALID, "math probe: n must be in [0, %lld]", (long long)kProbeMaxN);
    if (n == 0) return BFGX_OK;
    if (int rc = tables_begin(device)) return rc;
    const size_t bytes = sizeof(double) * (size_t)n;
    DevBuf da, db, d0, d1;
    if (da.up(a, bytes) || db.up(probe_two_args(fn) ? b : nullptr, bytes) || d0.up(fn == kProbeMulAddNc ? out0 : nullptr, bytes) ||
        d1.up(nullptr, bytes))
        return fail(BFGX_ERR_HIP, "device allocation/copy failed");
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + kProbeThreads - 1) / kProbeThreads)), dim3(kProbeThreads), 0, 0, fn, n,
                       da.as<double>(), db.as<double>(), d0.as<double>(), d1.as<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out0, d0.p, bytes, hipMemcpyDeviceToHost));
    if (probe_two_results(fn)) HIP_TRY(hipMemcpy(out1, d1.p, bytes, hipMemcpyDeviceToHost));
    return BFGX_OK;
}
