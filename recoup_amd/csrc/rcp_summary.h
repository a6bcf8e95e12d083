// rcp_summary.h -- launchers of rcp_summary.hip (summaries of kept profile matrices), shared with
// rcp_summary.cpp.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/recoup_amd.h"

// rows of one column that one workgroup of the column-statistics kernel reduces (256 lanes x 16)
constexpr int kSumColSlabRows = 4096;
// rows of one workgroup of the row-statistics kernel (one per lane of a wave; its 4 waves split the columns)
constexpr int kSumRowTile = 64;
// group ids the column statistics and the grouped order accept: [0, kSumMaxGroups)
constexpr int kSumMaxGroups = RCP_SUMMARY_MAX_GROUPS;  // (a 64-bit mask of the groups present in a slab)
static_assert(kSumMaxGroups <= 64, "group mask is one 64-bit word");

#if defined(__HIP__)
// Order-preserving 64-bit form of a double (shared by the row order and the quantile selection)
__device__ __forceinline__ uint64_t rcp_sort_key(double v) {
    const uint64_t u = (uint64_t)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
#endif

// ---- quantile selection (rcp_quantile.hip) ----
// A most-significant-digit radix selection over the sort keys: kQPasses passes of kQBits bits.
constexpr int kQBits = 8;
constexpr int kQBins = 1 << kQBits;
constexpr int kQPasses = 64 / kQBits;
constexpr int kQMaxProbs = RCP_QUANTILE_MAX_PROBS;
// (column, slab) units one workgroup of a streaming pass counts before it flushes its histogram;
// in whole-matrix scope at least this many, and as many as leave about kQMatrixGroups workgroups
constexpr int kQUnitsPerGroup = 4;
constexpr int kQMatrixGroups = 2048;

// Per (segment, requested probability): the selection's state between passes
struct RcpQState {
    unsigned long long prefix;  // the key digits chosen so far (the others 0)
    unsigned long long less;    // elements of the segment below every key with this prefix
    uint32_t k;                 // 0-based rank of x_(lo) among the keys with this prefix
    uint32_t ceq;               // keys in the digit chosen last (after the last pass: keys equal to x_(lo))
    int32_t rep;                // the slot whose histogram this one shares (smallest slot with the same
                                // prefix); after the last pass: the slot whose successor it shares, -1: none needed
    int32_t pad;
};
// Per requested probability, the same for every segment: from rcp_quantile_ranks
struct RcpQRanks {
    uint32_t k[kQMaxProbs];       // lo - 1
    int32_t interp[kQMaxProbs];   // hi == lo + 1
    double h[kQMaxProbs];
};
// Work split of a streaming pass
struct RcpQGeom {
    int64_t n_slabs, n_units, units_per_group, groups_per_col, grid;
};
RcpQGeom rcp_quantile_geometry(int64_t n_rows, int64_t n_cols, int32_t scope);

namespace rcpi {
// rcp_summary.cpp's descriptor checks (no device needed) and the device that holds the matrices
int summary_check_desc(const rcp_matrix_desc* m);
int summary_matrix_device(const rcp_matrix_desc* m, int* dev);
}  // namespace rcpi

extern "C" {
// One digit pass: counts digit `pass` of the keys that match their slot's prefix into
// hist[(segment * n_probs + slot) * kQBins + digit] (integer atomics; hist is zero on entry), and on
// pass 0 sets nanflag[segment] when the segment holds a NaN.  center != NULL: keys of
// |t(x) - center[segment]|.
hipError_t rcp_launch_qhist(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                            const double* center, int32_t scope, int32_t n_probs, int32_t pass,
                            const RcpQState* state, uint32_t* hist, uint32_t* nanflag, hipStream_t stream);
// Per (segment, slot): the digit that holds the rank, the new state; zeroes the histograms it read
hipError_t rcp_launch_qpick(int64_t n_segments, int32_t n_probs, int32_t pass, const RcpQRanks* ranks,
                            RcpQState* state, uint32_t* hist, hipStream_t stream);
// succ[segment * n_probs + slot] = min(succ, smallest key above the slot's x_(lo)) for slots that need it
hipError_t rcp_launch_qsucc(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                            const double* center, int32_t scope, int32_t n_probs, const RcpQState* state,
                            unsigned long long* succ, hipStream_t stream);
// q[segment * n_probs + slot] from the state, the successor and the NaN flag; times 1.4826 for mad
hipError_t rcp_launch_qfinal(int64_t n_segments, int32_t n_probs, const RcpQRanks* ranks, const RcpQState* state,
                             const unsigned long long* succ, const uint32_t* nanflag, int mad_scale, double* q,
                             hipStream_t stream);
hipError_t rcp_launch_qfill_nan(double* q, int64_t n, hipStream_t stream);

// Partials of one sample: for slab b, group g, column c the triple (n, mean, M2) of the rows of the
// slab that belong to g, at [(b * n_groups + g) * n_cols + c] of pn / pmean / pm2 -- written only
// for the groups present in the slab, which mask[b] lists (bit g).  d_group == NULL: one group.
hipError_t rcp_launch_colstats(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                               const int32_t* d_group, int32_t n_groups, double* pn, double* pmean, double* pm2,
                               unsigned long long* mask, hipStream_t stream);
// Merge the slabs of every (group, column) in slab order and write mean / sd / count (any may be NULL)
hipError_t rcp_launch_colstats_final(int64_t n_slabs, int64_t n_cols, int32_t n_groups, const double* pn,
                                     const double* pmean, const double* pm2, const unsigned long long* mask,
                                     double* mean, double* sd, int64_t* count, hipStream_t stream);
// Row statistics of one sample over its n_cols columns (outputs [n_rows], any may be NULL)
hipError_t rcp_launch_rowstats(const double* mat, int64_t n_rows, int64_t n_cols, int64_t ld, int log2p1,
                               double* o_sum, double* o_max, double* o_mean, double* o_sd, hipStream_t stream);
// The ordering key of every row from stat [n_samples][n_rows] (what: RCP_KEY_*), the sortable 64-bit
// form of it (reversed for `decreasing`; 0 for a row no group holds) and the identity permutation
hipError_t rcp_launch_order_keys(const double* stat, int32_t n_samples, int64_t n_rows, int what, int decreasing,
                                 const int32_t* d_group, int32_t n_groups, double* d_key, uint64_t* skey,
                                 int32_t* idx, hipStream_t stream);
// gkey[i] = group of row idx[i] (n_groups for a row no group holds)
hipError_t rcp_launch_order_groups(int64_t n_rows, const int32_t* idx, const int32_t* d_group, int32_t n_groups,
                                   uint64_t* gkey, hipStream_t stream);
}
