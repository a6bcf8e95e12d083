// rcp_plan.h -- the stages of plan creation (rcp_plan.cpp), for rcp_plan_create_ex and for the
// stand-alone driver of tests/plan.  The first three stages decide a plan's shape on the host
// alone: they make no HIP call and read no environment variable.
//
//   build_rows      the caller's row table -> oriented segments (Builder)
//   plan_parts      the bins' parts: slices, R-RNG layouts, interpolated rows
//   plan_shape      chunk geometry, the pileup kernel, fold, rounds, heavy slots, grid
//   plan_tables     the remaining host tables and their places in the arena     (rcp_plan.cpp)
//   plan_bind       device arenas, uploads, pointers                            (rcp_plan.cpp)
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "rcp_internal.h"

namespace rcpi {

// host copies of the device tables
struct Builder {
    std::vector<int32_t> row_chrom, row_seg, row_len;
    std::vector<uint8_t> row_static;
    std::vector<RcpSeg> segs;
    std::vector<int32_t> lay_index, lay_cnt;
    std::vector<std::pair<int32_t, int32_t>> lay_regions;  // (offset in lay_cnt, n bins)
    std::vector<int32_t> interp_row, interp_part, interp_mode, interp_pos, nb_pos;
};

// What the shape of a plan depends on besides its rows, bins and options.
struct PlanFacts {
    int32_t n_cus = 256;        // compute units of the plan's device (256 when the query fails)
    int32_t ignore_strand = 1;  // rcp_rows_desc.ignore_strand: the plan reads the merged layout
    bool has_st = false;        // that layout has the starts-only stream (reads of one width)
    int32_t n_chrom = 0;
    // diagnostics knobs of the environment (A/B runs), read once per plan
    bool lean_rounds2 = false;  // RCP_LEAN_ROUNDS=2: two-round items for binned lean plans too
    bool no_lean_fold = false;  // RCP_NO_LEAN_FOLD: per-base lean plans keep the locate launch
    int32_t coop_min = -1;      // RCP_COOP_MIN: the cooperative rows' threshold (-1: the default)
    int32_t gen_rounds = 0;     // RCP_GEN_ROUNDS: the general kernel's rounds, 1 / 2 / 4 (else: not set)
};

// What the shape reads from the row table, computed once (summarize_rows).
struct RowSummary {
    bool multi_rows = false;       // some row has more than one segment
    int32_t max_row_len = 0;
    int32_t max_heavy_len = 0;     // the longest row short enough for the heavy path
    // "every row is one plain range" (one segment, no range list, no zero-width query), twice:
    // statically-NULL rows and rows without segments skipped -- fold of the general kernel, the
    // bin-difference kernel and the lean fold (their kernels write such rows' zeros themselves)
    bool single_plain_nonnull = true;
    // ... and the lean kernel's own test, which looks at statically-NULL rows too (only rows
    // without segments pass unseen)
    bool single_plain_lean = true;
};

// What plan_parts found out about the parts (beside RcpPlanDev::part and Builder's tables).
struct PlanParts {
    int64_t n_cols = 0;
    bool pow2_bins = true;  // every binned row: uniform power-of-two bins (no R-RNG layout)
    int32_t max_interp_len = 0, max_interp_bins = 0;
    int32_t max_bin[RCP_MAX_PARTS];  // widest bin of each part (median: of those inside a wave chunk)
};

int build_rows(int32_t n_chrom, const rcp_rows_desc* rows, Builder* B);
RowSummary summarize_rows(const Builder& B);
// P->n_parts, stat, scale and part[] (all but the chunking); B: layouts and interpolated rows
int plan_parts(const rcp_bins_desc* bins, Builder* B, RcpPlanDev* P, PlanParts* out);
// the non-pointer fields of plan->dev and the scalar fields of *plan; B: a median plan's
// block-window rows join the interpolated ones
int plan_shape(const PlanFacts& F, const RowSummary& S, const PlanParts& Q, const rcp_bins_desc* bins, bool cov_only,
               const rcp_plan_opts* opts, Builder* B, rcp_plan* plan);

}  // namespace rcpi
