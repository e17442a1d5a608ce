// bfgx_profiles_common.inc -- the host half that the three profile measurements share (included in bfgx_api.hip before bfgx_stack_api.inc,
// bfgx_snapshot_stack_api.inc and bfgx_grid_stack_api.inc): the refusals with one text for all and the copy-back of the results.  StackOut
// (bfgx_stack_core.hpp) names the outputs on the host and on the device alike.

namespace {

int profiles_validate_bins(int32_t nb, const double *r_edges)
{
    if (nb < 1 || nb > kStackMaxBins) return fail(BFGX_ERR_INVALID, "%d radial bins: must be 1 .. %d (the bins of a halo live on chip)", (int)nb, kStackMaxBins);
    for (int i = 0; i <= nb; ++i)
        if (!std::isfinite(r_edges[i]) || r_edges[i] < 0.0) return fail(BFGX_ERR_INVALID, "r_edges must be finite and >= 0");
    for (int i = 0; i < nb; ++i)
        if (!(r_edges[i + 1] > r_edges[i])) return fail(BFGX_ERR_INVALID, "r_edges must be strictly ascending");
    return BFGX_OK;
}

int profiles_validate_shear(const double *g1, const double *g2, const StackOut &o)
{
    if ((g1 == nullptr) != (g2 == nullptr)) return fail(BFGX_ERR_INVALID, "NULL argument: the shear pair needs both g1 and g2");
    if (g1 && (!o.npix_shear || !o.sum_t || !o.sum_x)) return fail(BFGX_ERR_INVALID, "NULL argument: a shear pair needs npix_shear, sum_t and sum_x");
    return BFGX_OK;
}

// the bfgx_model of a measurement only carries the runner's cosmology, mass definition and epsilon_max: its table must be valid and is
// ignored.  table_first: which of the two refusals a model with both faults gets (the shell entries check the model first)
int profiles_validate_placeholder(const bfgx_model *model, bool table_first)
{
    if (!table_first)
        if (int rc = validate_model(model)) return rc;
    if (model->table.ndim != 3) return fail(BFGX_ERR_INVALID, "the profile measurement takes a model with a (dummy) 3-axis table: there is nothing to tabulate");
    return table_first ? validate_model(model) : BFGX_OK;
}

// the results of `cells` (halo, bin) cells from the device to the caller's arrays, on stream s (sum: where the call has one)
int profiles_copy_back(hipStream_t s, const StackOut &host, const StackOut &dev, size_t cells, bool shear)
{
    if (cells == 0) return BFGX_OK;
    HIP_TRY(hipMemcpyAsync(host.npix, dev.npix, cells * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    if (host.sum) HIP_TRY(hipMemcpyAsync(host.sum, dev.sum, cells * sizeof(double), hipMemcpyDeviceToHost, s));
    if (shear) {
        HIP_TRY(hipMemcpyAsync(host.npix_shear, dev.npix_shear, cells * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(host.sum_t, dev.sum_t, cells * sizeof(double), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(host.sum_x, dev.sum_x, cells * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    return BFGX_OK;
}

}  // namespace
