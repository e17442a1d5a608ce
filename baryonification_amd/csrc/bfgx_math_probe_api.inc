// C ABI of the device-math probe (include/bfgx.h, "device math probe"); included by bfgx_api.hip.

extern "C" int bfgx_math_probe(int device, int32_t fn, int64_t n, const double *a, const double *b, double *out0, double *out1)
{
    if (fn < 0 || fn >= kProbeCount) return fail(BFGX_ERR_INVALID, "math probe: unknown function id %d", (int)fn);
    if (!a || !out0 || (probe_two_args(fn) && !b) || (probe_two_results(fn) && !out1)) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (n < 0 || n > kProbeMaxN) return fail(BFGX_ERR_INVALID, "math probe: n must be in [0, %lld]", (long long)kProbeMaxN);
    if (n == 0) return BFGX_OK;
    HostCall c(device);
    const double *da = c.in(a, n), *db = c.in(probe_two_args(fn) ? b : nullptr, n);
    double *d0 = fn == kProbeMulAddNc ? c.inout(out0, n) : c.out(out0, n);            // mul_add_nc reads its third argument from out0
    double *d1 = c.out(probe_two_results(fn) ? out1 : nullptr, n);
    if (int rc = c.ready()) return rc;
    hipLaunchKernelGGL(math_probe_kernel, dim3((unsigned)((n + kProbeThreads - 1) / kProbeThreads)), dim3(kProbeThreads), 0, 0, fn, n,
                       da, db, d0, d1);
    return c.finish();
}
