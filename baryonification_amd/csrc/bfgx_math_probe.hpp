// Test probe of bfgx_math.hpp: one kernel that evaluates ONE of the device math functions elementwise, so that the suite can hold each
// of them to its stated bound against a high-precision reference (tests/test_gpu_math.py).  No product path launches it.
// What it shows is the sequence as compiled into this kernel; instruction scheduling and fp contraction inside the product kernels may
// differ, and the end-to-end parity tests stay responsible for that.
#pragma once
#include "bfgx_math.hpp"
#include "bfgx_kernels.hpp"

namespace bfgx {

// ids of bfgx_math_probe's `fn` (include/bfgx.h BFGX_MATH_*)
enum MathProbeFn : int32_t {
    kProbeRcp = 0, kProbeRsq, kProbeSqrt, kProbeLog, kProbeLogKReg, kProbeExp, kProbeSinCosSmall, kProbeSinCosSmallKReg, kProbeSinCosBounded,
    kProbeSinCosDphi, kProbeAtanSmall, kProbeAsinSmall, kProbeAtan2, kProbeMulAddNc, kProbeRingTheta, kProbeCount
};

constexpr int64_t kProbeMaxN = (int64_t)1 << 22;
constexpr int kProbeThreads = 256;

__host__ __device__ inline bool probe_two_args(int32_t fn) { return fn == kProbeAtan2 || fn == kProbeMulAddNc || fn == kProbeRingTheta; }
__host__ __device__ inline bool probe_two_results(int32_t fn) { return fn >= kProbeSinCosSmall && fn <= kProbeSinCosDphi; }

// one thread per element; every argument comes from global memory (nothing to fold).  kProbeMulAddNc reads its addend from out0.
__global__ void __launch_bounds__(kProbeThreads)
math_probe_kernel(int32_t fn, int64_t n, const double *__restrict__ a, const double *__restrict__ b, double *out0, double *__restrict__ out1)
{
    const LogK<KReg> logk;                         // (constructed once, at the top: see KReg)
    const SinCosK<KReg> sck;
    const int64_t i = (int64_t)blockIdx.x * kProbeThreads + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    const double y = probe_two_args(fn) ? b[i] : 0.0;
    double r0 = 0.0, r1 = 0.0;
    switch (fn) {
    case kProbeRcp: r0 = fast_rcp(x); break;
    case kProbeRsq: r0 = fast_rsq(x); break;
    case kProbeSqrt: r0 = fast_sqrt(x); break;
    case kProbeLog: r0 = fast_log(x); break;
    case kProbeLogKReg: r0 = fast_log(x, logk); break;
    case kProbeExp: r0 = fast_exp(x); break;
    case kProbeSinCosSmall: sincos_small(x, r0, r1); break;
    case kProbeSinCosSmallKReg: sincos_small(x, r0, r1, sck); break;
    case kProbeSinCosBounded: sincos_bounded(x, r0, r1); break;
    case kProbeSinCosDphi: sincos_dphi(x, r0, r1); break;
    case kProbeAtanSmall: r0 = atan_small(x); break;
    case kProbeAsinSmall: r0 = asin_small(x); break;
    case kProbeAtan2: r0 = atan2_generic(x, y); break;                     // (a, b) = (y, x) of atan2
    case kProbeMulAddNc: r0 = add_nc(mul_nc(x, y), out0[i]); break;
    case kProbeRingTheta: r0 = ring_theta_nolibm(make_hpx((int64_t)x), (int)y); break;
    default: break;
    }
    out0[i] = r0;
    if (probe_two_results(fn)) out1[i] = r1;
}

}  // namespace bfgx
