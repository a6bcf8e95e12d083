// rcp_summary.cpp -- rcp_summary_cols / rcp_summary_rows / rcp_order_rows: argument checks, scratch
// from the library's pool and the launch sequences of rcp_summary.hip.  Everything is enqueued on
// the caller's stream; nothing here synchronises with the host.
#include "rcp_internal.h"
#include "rcp_summary.h"

using namespace rcpi;

namespace {

// Checks that need no device (they run first, so a bad call fails the same way on any machine)
int check_desc(const rcp_matrix_desc* m) {
    if (!m) return fail(RCP_EINVAL, "matrix descriptor is NULL");
    if (m->n_rows < 0 || m->n_cols < 0) return fail(RCP_EINVAL, "negative matrix shape");
    if (m->ld < m->n_rows) return fail(RCP_EINVAL, "ld (%lld) < n_rows (%lld)", (long long)m->ld, (long long)m->n_rows);
    if (m->n_samples < 1) return fail(RCP_EINVAL, "n_samples (%d) < 1", m->n_samples);
    if (m->n_rows >= (int64_t(1) << 31)) return fail(RCP_EUNSUPPORTED, "n_rows >= 2^31");
    if (m->n_rows > 0 && m->n_cols > 0) {
        if (!m->d_mat) return fail(RCP_EINVAL, "d_mat is NULL");
        for (int32_t s = 0; s < m->n_samples; ++s)
            if (!m->d_mat[s]) return fail(RCP_EINVAL, "d_mat[%d] is NULL", s);
    }
    return RCP_OK;
}

int check_groups(const int32_t* d_group, int32_t n_groups) {
    if (!d_group) return RCP_OK;
    if (n_groups < 1) return fail(RCP_EINVAL, "n_groups (%d) < 1 with group ids", n_groups);
    if (n_groups > kSumMaxGroups)
        return fail(RCP_EUNSUPPORTED, "n_groups (%d) above the %d this build reduces", n_groups, kSumMaxGroups);
    return RCP_OK;
}

// The device that holds the matrices (the caller's current device when there is nothing to read)
int matrix_device(const rcp_matrix_desc* m, int* dev) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(RCP_ENODEVICE, "no HIP device visible");
    HIP_TRY(hipGetDevice(dev));
    if (m->n_rows > 0 && m->n_cols > 0) {
        hipPointerAttribute_t a;
        if (hipPointerGetAttributes(&a, m->d_mat[0]) == hipSuccess && a.type == hipMemoryTypeDevice)
            *dev = a.device;
        else
            (void)hipGetLastError();
    }
    return RCP_OK;
}

int64_t at_least_one(int64_t n) { return n > 0 ? n : 1; }

}  // namespace

// the same checks for rcp_quantile.cpp
int rcpi::summary_check_desc(const rcp_matrix_desc* m) { return check_desc(m); }
int rcpi::summary_matrix_device(const rcp_matrix_desc* m, int* dev) { return matrix_device(m, dev); }

extern "C" int rcp_summary_cols(const rcp_matrix_desc* m, const int32_t* d_group, int32_t n_groups, double* d_mean,
                                double* d_sd, int64_t* d_count, void* hip_stream) {
    RCP_TRY
    if (int rc = check_desc(m)) return rc;
    if (int rc = check_groups(d_group, n_groups)) return rc;
    const int32_t G = d_group ? n_groups : 1;
    const int64_t n_slabs = (m->n_rows + kSumColSlabRows - 1) / kSumColSlabRows;
    if (n_slabs * m->n_cols > 0x7fffffffLL)
        return fail(RCP_EUNSUPPORTED, "matrix above 2^31 (column, %d-row slab) pairs", kSumColSlabRows);
    int dev = 0;
    if (int rc = matrix_device(m, &dev)) return rc;
    if (m->n_cols == 0) return RCP_OK;
    DeviceGuard guard(dev);
    HIP_TRY(guard.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // one sample's partials, reused sample after sample in stream order
    const int64_t np = at_least_one(n_slabs * G * m->n_cols);
    PoolBuf part(s), mask(s);
    HIP_TRY(part.alloc(3 * np * sizeof(double)));
    HIP_TRY(mask.alloc(at_least_one(n_slabs) * sizeof(unsigned long long)));
    double* pn = part.as<double>();
    double* pmean = pn + np;
    double* pm2 = pmean + np;
    for (int32_t k = 0; k < m->n_samples; ++k) {
        const int64_t o = (int64_t)k * G * m->n_cols;
        HIP_TRY(rcp_launch_colstats(m->n_rows > 0 ? m->d_mat[k] : nullptr, m->n_rows, m->n_cols, m->ld, m->log2p1,
                                    d_group, G, pn, pmean, pm2, mask.as<unsigned long long>(), s));
        HIP_TRY(rcp_launch_colstats_final(n_slabs, m->n_cols, G, pn, pmean, pm2,
                                          d_group ? mask.as<unsigned long long>() : nullptr,
                                          d_mean ? d_mean + o : nullptr, d_sd ? d_sd + o : nullptr,
                                          d_count ? d_count + o : nullptr, s));
    }
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_summary_rows(const rcp_matrix_desc* m, double* d_sum, double* d_max, double* d_mean, double* d_sd,
                                void* hip_stream) {
    RCP_TRY
    if (int rc = check_desc(m)) return rc;
    int dev = 0;
    if (int rc = matrix_device(m, &dev)) return rc;
    if (m->n_rows == 0) return RCP_OK;
    DeviceGuard guard(dev);
    HIP_TRY(guard.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    for (int32_t k = 0; k < m->n_samples; ++k) {
        const int64_t o = (int64_t)k * m->n_rows;
        HIP_TRY(rcp_launch_rowstats(m->n_cols > 0 ? m->d_mat[k] : nullptr, m->n_rows, m->n_cols, m->ld, m->log2p1,
                                    d_sum ? d_sum + o : nullptr, d_max ? d_max + o : nullptr,
                                    d_mean ? d_mean + o : nullptr, d_sd ? d_sd + o : nullptr, s));
    }
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_order_rows(const rcp_matrix_desc* m, int32_t what, int32_t ref_sample, int32_t decreasing,
                              const int32_t* d_group, int32_t n_groups, int32_t* d_order, double* d_key,
                              void* hip_stream) {
    RCP_TRY
    if (int rc = check_desc(m)) return rc;
    if (what != RCP_KEY_SUM && what != RCP_KEY_MAX && what != RCP_KEY_AVG)
        return fail(RCP_EINVAL, "what (%d) is not an RCP_KEY_*", what);
    if (ref_sample < -1 || ref_sample >= m->n_samples)
        return fail(RCP_EINVAL, "ref_sample (%d) outside -1 .. %d", ref_sample, m->n_samples - 1);
    if (int rc = check_groups(d_group, n_groups)) return rc;
    if (!d_order) return fail(RCP_EINVAL, "d_order is NULL");
    int dev = 0;
    if (int rc = matrix_device(m, &dev)) return rc;
    const int64_t n = m->n_rows;
    if (n == 0) return RCP_OK;
    DeviceGuard guard(dev);
    HIP_TRY(guard.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int32_t first = ref_sample < 0 ? 0 : ref_sample;
    const int32_t S = ref_sample < 0 ? m->n_samples : 1;
    PoolBuf stat(s), k0(s), k1(s), i0(s), i1(s), temp(s);
    HIP_TRY(stat.alloc((size_t)S * n * sizeof(double)));
    HIP_TRY(k0.alloc(n * sizeof(uint64_t)));
    HIP_TRY(k1.alloc(n * sizeof(uint64_t)));
    HIP_TRY(i0.alloc(n * sizeof(int32_t)));
    if (d_group) HIP_TRY(i1.alloc(n * sizeof(int32_t)));
    for (int32_t k = 0; k < S; ++k) {
        double* o = stat.as<double>() + (int64_t)k * n;
        HIP_TRY(rcp_launch_rowstats(m->n_cols > 0 ? m->d_mat[first + k] : nullptr, n, m->n_cols, m->ld, m->log2p1,
                                    what == RCP_KEY_SUM ? o : nullptr, what == RCP_KEY_MAX ? o : nullptr,
                                    what == RCP_KEY_AVG ? o : nullptr, nullptr, s));
    }
    HIP_TRY(rcp_launch_order_keys(stat.as<double>(), S, n, what, decreasing != 0, d_group, n_groups, d_key,
                                  k0.as<uint64_t>(), i0.as<int32_t>(), s));
    // stable radix sort of the keys; with groups a second stable sort on the group id, which keeps
    // each group's rows in key order and the rows no group holds (id n_groups) last, in row order
    int32_t* sorted = d_group ? i1.as<int32_t>() : d_order;
    size_t tb = 0;
    HIP_TRY(rcp_sort_pairs(nullptr, &tb, k0.as<uint64_t>(), k1.as<uint64_t>(), i0.as<int32_t>(), sorted, n, 0, 64, s));
    HIP_TRY(temp.alloc(std::max<size_t>(tb, 16)));  // (a NULL temp would be a size query)
    HIP_TRY(rcp_sort_pairs(temp.p, &tb, k0.as<uint64_t>(), k1.as<uint64_t>(), i0.as<int32_t>(), sorted, n, 0, 64, s));
    if (d_group) {
        HIP_TRY(rcp_launch_order_groups(n, sorted, d_group, n_groups, k0.as<uint64_t>(), s));
        size_t tb2 = 0;
        HIP_TRY(rcp_sort_pairs(nullptr, &tb2, k0.as<uint64_t>(), k1.as<uint64_t>(), sorted, d_order, n, 0, 8, s));
        if (tb2 > temp.bytes) HIP_TRY(temp.alloc(tb2));
        HIP_TRY(rcp_sort_pairs(temp.p, &tb2, k0.as<uint64_t>(), k1.as<uint64_t>(), sorted, d_order, n, 0, 8, s));
    }
    return RCP_OK;
    RCP_CATCH
}
