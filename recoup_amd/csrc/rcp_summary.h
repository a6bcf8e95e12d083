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

extern "C" {
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
