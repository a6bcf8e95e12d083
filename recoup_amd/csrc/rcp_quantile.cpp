// rcp_quantile.cpp -- rcp_summary_quantiles / rcp_summary_median_mad / rcp_quantile_ranks: argument
// checks, scratch from the library's pool and the launch sequence of rcp_quantile.hip.  Everything
// is enqueued on the caller's stream; nothing here synchronises with the host.
#include <math.h>

#include "rcp_internal.h"
#include "rcp_summary.h"

using namespace rcpi;

namespace {

// index = 1 + (n - 1) * p with the product and the sum rounded separately, whatever the host
// compiler would like to contract
void ranks_of(int64_t n, double p, int64_t* lo, int64_t* hi, double* h) {
#pragma clang fp contract(off)
    if (n == 0) {
        *lo = *hi = 0;
        *h = 0.0;
        return;
    }
    const double prod = (double)(n - 1) * p;
    const double index = 1.0 + prod;
    const double fl = floor(index);
    *lo = (int64_t)fl;
    *hi = (int64_t)ceil(index);
    *h = index - fl;
}

bool bad_prob(double p) { return !(p >= 0.0 && p <= 1.0); }  // NaN included

// Scratch of one selection, reused sample after sample in stream order
struct Scratch {
    PoolBuf state, hist, flag, succ;
    explicit Scratch(hipStream_t s) : state(s), hist(s), flag(s), succ(s) {}
    hipError_t alloc(int64_t n_seg, int32_t np) {
        const size_t slots = (size_t)n_seg * np;
        if (hipError_t e = state.alloc(slots * sizeof(RcpQState))) return e;
        if (hipError_t e = hist.alloc(slots * kQBins * sizeof(uint32_t))) return e;
        if (hipError_t e = flag.alloc((size_t)n_seg * sizeof(uint32_t))) return e;
        return succ.alloc(slots * sizeof(unsigned long long));
    }
};

struct Selection {
    const double* mat;
    int64_t n_rows, n_cols, ld;
    int log2p1;
    const double* center;  // NULL, or [n_segments]: select over |t(x) - center[segment]|
    int32_t scope;
    int32_t np;
    int mad_scale;
};

// x_(lo) by kQPasses digit passes, x_(hi) by a successor pass where some probability interpolates,
// then q [n_segments][np].  The segments hold n >= 1 elements each.
hipError_t select(const Selection& a, const RcpQRanks& ranks, Scratch& w, double* q, hipStream_t s) {
    const int64_t n_seg = a.scope == RCP_QUANTILE_COLS ? a.n_cols : 1;
    if (hipError_t e = hipMemsetAsync(w.hist.p, 0, w.hist.bytes, s)) return e;
    if (hipError_t e = hipMemsetAsync(w.flag.p, 0, w.flag.bytes, s)) return e;
    for (int32_t pass = 0; pass < kQPasses; ++pass) {
        if (hipError_t e = rcp_launch_qhist(a.mat, a.n_rows, a.n_cols, a.ld, a.log2p1, a.center, a.scope, a.np, pass,
                                            w.state.as<RcpQState>(), w.hist.as<uint32_t>(), w.flag.as<uint32_t>(), s))
            return e;
        if (hipError_t e = rcp_launch_qpick(n_seg, a.np, pass, &ranks, w.state.as<RcpQState>(), w.hist.as<uint32_t>(), s))
            return e;
    }
    bool interp = false;
    for (int32_t j = 0; j < a.np; ++j) interp |= ranks.interp[j] != 0;
    if (interp) {
        if (hipError_t e = hipMemsetAsync(w.succ.p, 0xff, w.succ.bytes, s)) return e;
        if (hipError_t e = rcp_launch_qsucc(a.mat, a.n_rows, a.n_cols, a.ld, a.log2p1, a.center, a.scope, a.np,
                                            w.state.as<RcpQState>(), w.succ.as<unsigned long long>(), s))
            return e;
    }
    return rcp_launch_qfinal(n_seg, a.np, &ranks, w.state.as<RcpQState>(), w.succ.as<unsigned long long>(),
                             w.flag.as<uint32_t>(), a.mad_scale, q, s);
}

int fill_ranks(int64_t n, const double* probs, int32_t np, RcpQRanks* r) {
    *r = RcpQRanks{};
    for (int32_t j = 0; j < np; ++j) {
        int64_t lo = 0, hi = 0;
        double h = 0.0;
        ranks_of(n, probs[j], &lo, &hi, &h);
        r->k[j] = (uint32_t)(lo - 1);
        r->interp[j] = hi != lo;
        r->h[j] = h;
    }
    return RCP_OK;
}

// Checks shared by both calls, after the descriptor's: counters and grids
int check_sizes(const rcp_matrix_desc* m, int32_t scope) {
    if (scope == RCP_QUANTILE_MATRIX && m->n_rows > 0 && m->n_cols > (int64_t)0xffffffffLL / m->n_rows)
        return fail(RCP_EUNSUPPORTED, "a segment of 2^32 or more elements (%lld x %lld): counters are 32-bit",
                    (long long)m->n_rows, (long long)m->n_cols);
    const int64_t n_slabs = (m->n_rows + kSumColSlabRows - 1) / kSumColSlabRows;
    if (n_slabs > 0 && m->n_cols > (int64_t)0x7fffffffLL / n_slabs)
        return fail(RCP_EUNSUPPORTED, "matrix above 2^31 (column, %d-row slab) pairs", kSumColSlabRows);
    return RCP_OK;
}

}  // namespace

extern "C" int rcp_quantile_ranks(int64_t n, double p, int64_t* lo, int64_t* hi, double* h) {
    RCP_TRY
    if (n < 0) return fail(RCP_EINVAL, "n (%lld) < 0", (long long)n);
    if (!lo || !hi || !h) return fail(RCP_EINVAL, "an output of rcp_quantile_ranks is NULL");
    if (bad_prob(p)) return fail(RCP_EINVAL, "probability %g outside [0, 1]", p);
    ranks_of(n, p, lo, hi, h);
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_summary_quantiles(const rcp_matrix_desc* m, int32_t scope, const double* probs, int32_t n_probs,
                                     double* d_q, void* hip_stream) {
    RCP_TRY
    if (int rc = summary_check_desc(m)) return rc;
    if (scope != RCP_QUANTILE_MATRIX && scope != RCP_QUANTILE_COLS)
        return fail(RCP_EINVAL, "scope (%d) is not an RCP_QUANTILE_*", scope);
    if (!probs) return fail(RCP_EINVAL, "probs is NULL");
    if (n_probs < 1) return fail(RCP_EINVAL, "n_probs (%d) < 1", n_probs);
    if (n_probs > RCP_QUANTILE_MAX_PROBS)
        return fail(RCP_EUNSUPPORTED, "n_probs (%d) above the %d one call selects", n_probs, RCP_QUANTILE_MAX_PROBS);
    for (int32_t j = 0; j < n_probs; ++j)
        if (bad_prob(probs[j])) return fail(RCP_EINVAL, "'probs' outside [0,1]: probs[%d] = %g", j, probs[j]);
    if (!d_q) return fail(RCP_EINVAL, "d_q is NULL");
    if (int rc = check_sizes(m, scope)) return rc;
    int dev = 0;
    if (int rc = summary_matrix_device(m, &dev)) return rc;
    const int64_t n_seg = scope == RCP_QUANTILE_COLS ? m->n_cols : 1;
    if (n_seg == 0) return RCP_OK;
    DeviceGuard guard(dev);
    HIP_TRY(guard.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int64_t n = scope == RCP_QUANTILE_COLS ? m->n_rows : m->n_rows * m->n_cols;
    if (n == 0) {  // quantile(numeric(0), p) is NA
        HIP_TRY(rcp_launch_qfill_nan(d_q, (int64_t)m->n_samples * n_seg * n_probs, s));
        return RCP_OK;
    }
    RcpQRanks ranks;
    fill_ranks(n, probs, n_probs, &ranks);
    Scratch w(s);
    HIP_TRY(w.alloc(n_seg, n_probs));
    for (int32_t k = 0; k < m->n_samples; ++k) {
        const Selection a{m->d_mat[k], m->n_rows, m->n_cols, m->ld, m->log2p1 != 0, nullptr, scope, n_probs, 0};
        HIP_TRY(select(a, ranks, w, d_q + (int64_t)k * n_seg * n_probs, s));
    }
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_summary_median_mad(const rcp_matrix_desc* m, double* d_median, double* d_mad, void* hip_stream) {
    RCP_TRY
    if (int rc = summary_check_desc(m)) return rc;
    if (!d_median && !d_mad) return fail(RCP_EINVAL, "d_median and d_mad are both NULL");
    if (int rc = check_sizes(m, RCP_QUANTILE_COLS)) return rc;
    int dev = 0;
    if (int rc = summary_matrix_device(m, &dev)) return rc;
    if (m->n_cols == 0) return RCP_OK;
    DeviceGuard guard(dev);
    HIP_TRY(guard.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (m->n_rows == 0) {  // median(numeric(0)) is NA
        const int64_t n_out = (int64_t)m->n_samples * m->n_cols;
        if (d_median) HIP_TRY(rcp_launch_qfill_nan(d_median, n_out, s));
        if (d_mad) HIP_TRY(rcp_launch_qfill_nan(d_mad, n_out, s));
        return RCP_OK;
    }
    const double half = 0.5;
    RcpQRanks ranks;
    fill_ranks(m->n_rows, &half, 1, &ranks);
    Scratch w(s);
    HIP_TRY(w.alloc(m->n_cols, 1));
    PoolBuf center(s);  // the medians when the caller does not want them
    if (!d_median) HIP_TRY(center.alloc((size_t)m->n_cols * sizeof(double)));
    for (int32_t k = 0; k < m->n_samples; ++k) {
        double* med = d_median ? d_median + (int64_t)k * m->n_cols : center.as<double>();
        Selection a{m->d_mat[k], m->n_rows, m->n_cols, m->ld, m->log2p1 != 0, nullptr, RCP_QUANTILE_COLS, 1, 0};
        HIP_TRY(select(a, ranks, w, med, s));
        if (!d_mad) continue;
        // the second selection reads the medians the first one wrote, in stream order
        a.center = med;
        a.mad_scale = 1;
        HIP_TRY(select(a, ranks, w, d_mad + (int64_t)k * m->n_cols, s));
    }
    return RCP_OK;
    RCP_CATCH
}
