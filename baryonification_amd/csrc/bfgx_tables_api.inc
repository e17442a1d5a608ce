// bfgx_tables_api.inc -- C ABI of the table builders (a6-a8): projection, enclosed mass, displacement rows, pressure profile.
// Kernels: bfgx_tables.hpp.  Needs bfgx_hostcall.hpp.

extern "C" {

int bfgx_project_profile(int device, int64_t nrows, int32_t nl, const double *l, const double *rho,
                         int64_t nr, const double *r, double scale, double *sigma_out)
{
    if (!l || !rho || !r || !sigma_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535 || nl < 2 || nl > 2048 || nr < 1) return fail(BFGX_ERR_INVALID, "bad sizes (1 <= nrows <= 65535, 2 <= nl <= 2048)");
    HostCall c(device);
    const double *dl = c.in(l, nl), *drho = c.in(rho, nrows * nl), *dr = c.in(r, nr);
    double *dout = c.out(sigma_out, nrows * nr);
    if (int rc = c.ready()) return rc;
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((nr + 255) / 256), (unsigned)nrows), dim3(256), 3 * sizeof(double) * nl, 0,
                       nl, dl, drho, nr, dr, scale, dout);
    return c.finish();
}

static int enclosed_mass_rows(int dim, int device, int64_t nrows, int64_t n_int, const double *r_int, const double *Sigma,
                              int32_t nr, const double *r, double *M_f)
{
    if (!r_int || !Sigma || !r || !M_f) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || n_int < 3 || nr < 1) return fail(BFGX_ERR_INVALID, "bad sizes");
    HostCall c(device);
    const double *dri = c.in(r_int, n_int), *dS = c.in(Sigma, nrows * n_int), *dr = c.in(r, nr);
    double *dcx = c.scratch<double>(nrows * n_int), *dcy = c.scratch<double>(nrows * n_int), *dM = c.out(M_f, nrows * nr);
    if (int rc = c.ready()) return rc;
    hipLaunchKernelGGL(enclosed_mass_kernel, dim3((unsigned)nrows), dim3(kTabThreads), 0, 0, n_int, dri, dS, nr, dr, dcx, dcy, dM, dim);
    return c.finish();
}

int bfgx_enclosed_mass_from_sigma(int device, int64_t nrows, int64_t n_int, const double *r_int, const double *Sigma,
                                  int32_t nr, const double *r, double *M_f)
{
    return enclosed_mass_rows(2, device, nrows, n_int, r_int, Sigma, nr, r, M_f);
}

int bfgx_enclosed_mass_3d(int device, int64_t nrows, int64_t n_int, const double *r_int, const double *rho,
                          int32_t nr, const double *r, double *M_f)
{
    return enclosed_mass_rows(3, device, nrows, n_int, r_int, rho, nr, r, M_f);
}

int bfgx_enclosed_mass_2d(int device, int64_t nrows, int32_t nl, const double *l, const double *rho, double a,
                          int64_t n_int, const double *r_int, int32_t nr, const double *r, double *M_f)
{
    if (!l || !rho || !r_int || !r || !M_f) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nrows > 65535 || nl < 2 || nl > 2048 || n_int < 3 || nr < 1) return fail(BFGX_ERR_INVALID, "bad sizes");
    HostCall c(device);
    const double *dl = c.in(l, nl), *drho = c.in(rho, nrows * nl), *dri = c.in(r_int, n_int);
    double *dS = c.scratch<double>(nrows * n_int);
    const double *dr = c.in(r, nr);
    double *dcx = c.scratch<double>(nrows * n_int), *dcy = c.scratch<double>(nrows * n_int), *dM = c.out(M_f, nrows * nr);
    if (int rc = c.ready()) return rc;
    // Sigma = model.projected(r_int) * a   (BaryonCorrection.py:646), then the prefix sum + log-log PCHIP
    hipLaunchKernelGGL(project_kernel, dim3((unsigned)((n_int + 255) / 256), (unsigned)nrows), dim3(256), 3 * sizeof(double) * nl, 0,
                       nl, dl, drho, n_int, dri, a, dS);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(enclosed_mass_kernel, dim3((unsigned)nrows), dim3(kTabThreads), 0, 0, n_int, dri, dS, nr, dr, dcx, dcy, dM, 2);
    return c.finish();
}

int bfgx_displacement_rows(int device, int64_t nrows, int32_t nr, const double *r, const double *M_dmo, const double *M_dmb,
                           double *d_out, int32_t *status)
{
    if (!r || !M_dmo || !M_dmb || !d_out || !status) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nr < 3 || nr > kMaxNR) return fail(BFGX_ERR_INVALID, "N_samples_R must be in [3, %d]", kMaxNR);
    HostCall c(device);
    const double *dr = c.in(r, nr), *da = c.in(M_dmo, nrows * nr), *db = c.in(M_dmb, nrows * nr);
    double *dd = c.out(d_out, nrows * nr);
    int32_t *ds = c.out(status, nrows);
    if (int rc = c.ready()) return rc;
    const size_t lds = kDisplacementLdsPerNode * nr;
    HIP_TRY(hipFuncSetAttribute((const void *)displacement_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(displacement_kernel, dim3((unsigned)nrows), dim3(256), lds, 0, nr, dr, da, db, dd, ds);
    return c.finish();
}

int bfgx_pressure_profile(int device, int64_t nrows, const double *r500, const double *rho_tot, const double *rho_gas,
                          int32_t nr_out, const double *r_out, double cutoff, double *P_out)
{
    if (!r500 || !rho_tot || !rho_gas || !r_out || !P_out) return fail(BFGX_ERR_INVALID, "NULL argument");
    if (nrows < 1 || nr_out < 1) return fail(BFGX_ERR_INVALID, "bad sizes");
    HostCall c(device);
    const double *dg = c.in(r500, kPressureN), *dt = c.in(rho_tot, nrows * kPressureN), *dgas = c.in(rho_gas, nrows * kPressureN);
    const double *dr = c.in(r_out, nr_out);
    double *dP = c.out(P_out, nrows * nr_out);
    if (int rc = c.ready()) return rc;
    const double G = kGnewt / (kMpcToMeter * kMpcToMeter * kMpcToMeter) * kSolarMass;       // Thermodynamic.py:11
    const double unit = (kSolarMass * 1e3) / (kMpcToMeter * 1e2);                           // :265
    hipLaunchKernelGGL(pressure_kernel, dim3((unsigned)nrows), dim3(256), 0, 0, dg, dt, dgas, nr_out, dr, G, unit, cutoff, dP);
    return c.finish();
}

}  // extern "C"
