// rcp_plan.cpp -- plans: what a (row table, bins, options) profile needs on the device and how
// its kernels are launched.
//
// Creating a plan is a sequence of stages (rcp_plan.h).  build_rows, plan_parts and plan_shape
// decide everything -- which pileup kernel runs, the column chunks, fold, rounds, heavy slots,
// the grid -- from the row table, the bins, the options and a PlanFacts, on the host alone: no
// HIP call, no environment variable, so tests/plan drives them without a device.  plan_tables
// lays the host tables out and plan_bind allocates, uploads and sets the pointers; neither
// decides a shape field.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/recoup_amd.h"
#include "rcp_device.h"
#include "rcp_internal.h"
#include "rcp_plan.h"
#include "rcp_rng.h"
#include "rcp_stage.h"

using namespace rcpi;

// ---- planning constants

// auto split off: on one GPU's 1/8, 1/4, 1/2 shard of C4, 4 and 8 column chunks instead of 2
// were slower (1/8: pileup 0.109 -> 0.143 / 0.203 ms; profiles/r02c/lean_chunk_split_ab.log) --
// an item's time is set by its 64 rows' read round trips, not by its width
constexpr int kLeanItemsPerWg = 0;  // work items per persistent workgroup, at least
// Per-base plans (C5's TSS windows: reads piled in the window's middle, so the middle column
// chunks are several times the outer ones' work) on few row tiles -- one GPU's shard -- take at
// least this many work items per workgroup: narrower chunks let the per-XCD claims balance the
// heavy middle items against the light outer ones (with ~1.5 items per workgroup the pass lasts
// as long as the slowest workgroup's heavy items)
constexpr int kLeanItemsPerWgBase = 4;
constexpr int kLeanMinChunkBins = 64;                   // no column chunks narrower than this
constexpr int32_t kFoldConcurrentMaxRows = 8192;        // per-base lean fold of plans in flight, rows at most
// AUTO keeps binned plans of fewer rows on the general kernel: a lean item is 64 rows, the
// general kernel's workgroup 32, and with about one item per workgroup the item's read round
// trips set the pass.  C4 shards (1000 bins of 2 bp), ms per pass lean / general: 25 k rows
// 0.141 / 0.133, 33 k 0.160 / 0.154, 40 k 0.187 / 0.197, 50 k 0.217 / 0.232; per-base C5
// shards stay lean (12.5 k rows: 0.317 / 0.435).  profiles/r03/pipeline/small_shard_kernels.log
constexpr int kLeanMinRowsBinned = 36000;

namespace {

constexpr int kWaveMax = 2047;         // positions per wave sub-chunk (64 x 32 slots incl. the end sentinel)
constexpr int kStageMaxBins = 512;  // bins per chunk (LDS stage = bins x 17 words)
constexpr size_t kLdsBudget = 80 * 1024;  // pileup LDS per workgroup (80 KB: two per CU)
constexpr int kHeavyThreshold = 4096;  // candidate reads per column chunk above which a row is split across workgroups
                                        // (8192 before the lean kernel dealt rows dynamically; C4 0.647 -> 0.633 ms)
constexpr int kHeavySlice = 4096;  // candidate reads per heavy work item
constexpr int kHeavyMaxLen = 16383;    // longer rows never take the heavy path
// general-kernel plans of at most this many rows search their rows' read ranges in the pileup
// kernel (P.fold): one GPU's share of a region table, where the locate launch and its record round
// trip are a third of the pass
constexpr int kFoldMaxRows = 65536;
// ... and pile a fused-bins chunk of a row with more candidate reads than this with the whole
// workgroup (8 waves, 16 reads per lane in flight) instead of one wave
constexpr int kCoopMin = 8192;
constexpr int kGeneralMaxChunks = 8;  // column chunks a wide binned part is cut into (general kernel)

// A wave's difference array: 64 lanes x per positions (per a power of two >= 4), each lane's
// chunk padded by 4 words (rcp_kernels.hip scan_wave).  Returns the LDS words and the
// position capacity for a chunk of `positions`.
void wave_geometry(int32_t positions, int32_t* words, int32_t* capacity) {
    int32_t need = (positions + 1 + 63) / 64;
    int32_t per = 4;
    while (per < need) per <<= 1;
    *words = 64 * (per + 4);
    *capacity = 64 * per - 1;
}

}  // namespace

// =====================================================================================
// the row table
// =====================================================================================

namespace {

uint8_t stream_mask(int ignore_strand, int8_t q) {
    // findOverlaps strand compatibility: '*' matches everything (Appendix A, Q2)
    if (ignore_strand) return 0x1;  // the merged layout: every strand in stream 0
    if (q == RCP_STRAND_ANY) return 0x7;
    return (uint8_t)((1u << q) | (1u << RCP_STRAND_ANY));
}

}  // namespace

namespace rcpi {

int build_rows(int32_t n_chrom, const rcp_rows_desc* rows, Builder* B) {
    const int R = rows->n_rows;
    B->row_chrom.assign(R, -1);
    B->row_seg.assign(R + 1, 0);
    B->row_len.assign(R, 0);
    B->row_static.assign(R, 0);
    for (int r = 0; r < R; ++r) {
        const int64_t j0 = rows->seg_off[r], j1 = rows->seg_off[r + 1];
        if (j1 < j0) return fail(RCP_EINVAL, "seg_off not monotone at row %d", r);
        B->row_seg[r] = (int32_t)B->segs.size();
        if (j1 == j0) {
            B->row_static[r] = 1;
            continue;
        }
        const int32_t chrom = rows->seg_chrom[j0];
        B->row_chrom[r] = chrom;
        if (chrom < 0 || chrom >= n_chrom) B->row_static[r] = 1;
        int32_t off = 0;
        // groups appear as contiguous runs of seg_group
        int64_t g0 = j0;
        int prev_group = -1;
        while (g0 < j1) {
            const int grp = rows->seg_group ? rows->seg_group[g0] : 0;
            if (grp < 0 || grp > 3) return fail(RCP_EINVAL, "seg_group %d outside 0..3 (row %d)", grp, r);
            if (grp <= prev_group) return fail(RCP_EINVAL, "groups of row %d not contiguous/increasing", r);
            prev_group = grp;
            int64_t g1 = g0;
            while (g1 < j1 && (rows->seg_group ? rows->seg_group[g1] : 0) == grp) ++g1;
            const bool multi = rows->group_is_list && rows->group_is_list[grp];
            const bool rev_group = rows->seg_strand[g0] == RCP_STRAND_MINUS;  // strand(x)[1] == "-"
            const int32_t gfirst = (int32_t)B->segs.size();
            const int32_t gcount = (int32_t)(g1 - g0);
            if (gcount > 32767) return fail(RCP_EUNSUPPORTED, "more than 32767 ranges in one mask element");
            for (int64_t q = 0; q < gcount; ++q) {
                const int64_t j = rev_group ? (g1 - 1 - q) : (g0 + q);
                if (rows->seg_chrom[j] != chrom) {
                    if (multi) return fail(RCP_EUNSUPPORTED, "row %d: mask element spans several chromosomes", r);
                    return fail(RCP_EUNSUPPORTED, "row %d: groups on different chromosomes", r);
                }
                const int32_t s = rows->seg_start[j], e = rows->seg_end[j];
                RcpSeg sg{};
                sg.gfirst = gfirst;
                sg.gcount = (int16_t)gcount;
                sg.multi = multi ? 1 : 0;
                sg.group = (uint8_t)grp;
                sg.streams = stream_mask(rows->ignore_strand, rows->seg_strand[j]);
                if (e >= s) {
                    // i2k piece s:e; R drops index 0 and fails on negative indices
                    if (s < 0) B->row_static[r] = 1;
                    sg.lo = std::max<int32_t>(s, 1);
                    sg.hi = e;
                    sg.query_ok = 1;
                    sg.rev = rev_group ? 1 : 0;
                    if (sg.hi < sg.lo) continue;  // only index 0: nothing left
                } else {
                    // zero-width range: findOverlaps finds nothing (documented); s:(s-1) still
                    // yields two positions, which only matters for rows that are NULL anyway
                    if (multi) return fail(RCP_EUNSUPPORTED, "row %d: zero-width range inside a range list", r);
                    if (e < 0) B->row_static[r] = 1;
                    sg.lo = std::max<int32_t>(e, 1);
                    sg.hi = s;
                    sg.query_ok = 0;
                    sg.rev = rev_group ? 0 : 1;
                    if (sg.hi < sg.lo) continue;
                }
                sg.off = off;
                off += sg.hi - sg.lo + 1;
                B->segs.push_back(sg);
            }
            // fix gcount for skipped empty pieces
            const int32_t kept = (int32_t)B->segs.size() - gfirst;
            for (int32_t q = gfirst; q < gfirst + kept; ++q) B->segs[q].gcount = (int16_t)kept;
            // nearest other ranges of the group (the pileup's one-range weight shortcut)
            for (int32_t q = gfirst; q < gfirst + kept; ++q) {
                RcpSeg& a = B->segs[q];
                a.nb_lo = INT32_MIN;
                a.nb_hi = INT32_MAX;
                if (!multi) continue;
                for (int32_t t = gfirst; t < gfirst + kept; ++t) {
                    if (t == q || !B->segs[t].query_ok) continue;
                    const RcpSeg& b = B->segs[t];
                    if (b.hi < a.lo) a.nb_lo = std::max(a.nb_lo, b.hi);
                    else if (b.lo > a.hi) a.nb_hi = std::min(a.nb_hi, b.lo);
                    else a.nb_lo = INT32_MAX;  // intersecting ranges: always count
                }
            }
            g0 = g1;
        }
        B->row_len[r] = off;
    }
    B->row_seg[R] = (int32_t)B->segs.size();
    return RCP_OK;
}

}  // namespace rcpi

// =====================================================================================
// the shape of a plan
// =====================================================================================

namespace rcpi {

RowSummary summarize_rows(const Builder& B) {
    RowSummary S;
    const int R = (int)B.row_len.size();
    for (int r = 0; r < R; ++r) {
        const int32_t j0 = B.row_seg[r], j1 = B.row_seg[r + 1];
        S.multi_rows = S.multi_rows || j1 - j0 > 1;
        S.max_row_len = std::max(S.max_row_len, B.row_len[r]);
        if (B.row_len[r] <= kHeavyMaxLen) S.max_heavy_len = std::max(S.max_heavy_len, B.row_len[r]);
        if (j1 == j0) continue;
        const bool plain = j1 - j0 == 1 && !B.segs[j0].multi && B.segs[j0].query_ok;
        if (!plain) S.single_plain_lean = false;
        if (!plain && !B.row_static[r]) S.single_plain_nonnull = false;
    }
    return S;
}

int plan_parts(const rcp_bins_desc* bins, Builder* Bp, RcpPlanDev* Pp, PlanParts* out) {
    Builder& B = *Bp;
    RcpPlanDev& P = *Pp;
    const int R = (int)B.row_len.size();
    const bool rounding = bins->rng_kind == RCP_RNG_ROUNDING;
    P.n_parts = bins->n_parts;
    P.stat = bins->stat;
    P.scale = bins->scale;
    int64_t col = 0;
    bool lean_ok = true;  // so far: uniform power-of-two bins (no R-RNG layouts)
    int32_t max_interp_len = 0, max_interp_bins = 0;
    std::fill(out->max_bin, out->max_bin + RCP_MAX_PARTS, 1);
    std::map<std::pair<int, int>, int32_t> layout_cache;  // (n, dif) -> offset in lay_cnt
    std::map<std::pair<int, int>, int32_t> nb_cache;      // (n, L) -> offset in nb_pos
    for (int p = 0; p < bins->n_parts; ++p) {
        RcpPart& pt = P.part[p];
        const int32_t f1 = bins->flank[0], f2 = bins->flank[1];
        if (f1 < 0 || f2 < 0) return fail(RCP_EINVAL, "negative flank");
        switch (bins->where ? bins->where[p] : RCP_WHERE_WHOLE) {
            case RCP_WHERE_WHOLE: pt.lo_off = 0; pt.lo_end = 0; pt.hi_off = 0; pt.hi_end = 1; break;
            case RCP_WHERE_CENTER: pt.lo_off = f1; pt.lo_end = 0; pt.hi_off = -f2; pt.hi_end = 1; break;
            case RCP_WHERE_UPSTREAM: pt.lo_off = 0; pt.lo_end = 0; pt.hi_off = f1; pt.hi_end = 0; break;
            case RCP_WHERE_DOWNSTREAM: pt.lo_off = -f2; pt.lo_end = 1; pt.hi_off = 0; pt.hi_end = 1; break;
            default: return fail(RCP_EINVAL, "where[%d] = %d", p, bins->where[p]);
        }
        const int nb = bins->n_bins[p];
        if (nb < 0) return fail(RCP_EINVAL, "n_bins[%d] < 0", p);
        pt.per_base = nb == 0;
        pt.n_bins = pt.per_base ? (bins->per_base_width ? bins->per_base_width[p] : 0) : nb;
        if (pt.n_bins <= 0) return fail(RCP_EINVAL, "part %d has no columns", p);
        pt.col_off = (int32_t)col;
        col += pt.n_bins;
        pt.lay_base = (int32_t)B.lay_index.size();
        int32_t max_bin = 1;
        if (!pt.per_base) {
            B.lay_index.resize(B.lay_index.size() + pt.n_bins, -1);
            for (int r = 0; r < R; ++r) {
                int32_t head, L;
                rcp_part_slice(pt, B.row_len[r], &head, &L);
                if (B.row_static[r] || B.row_seg[r] == B.row_seg[r + 1]) continue;  // always NULL
                if (L < 0 || head < 0 || head + L > B.row_len[r])
                    return fail(RCP_EUNSUPPORTED, "row %d: part %d slice out of its %d-long coverage", r, p,
                                B.row_len[r]);
                if (L < pt.n_bins) {
                    int mode = bins->interp;
                    if (mode == RCP_INTERP_AUTO)
                        mode = ((double)(pt.n_bins - L) / pt.n_bins < 0.2) ? RCP_INTERP_NEIGHBORHOOD : RCP_INTERP_SPLINE;
                    int32_t pos_off = -1;
                    if (mode == RCP_INTERP_NEIGHBORHOOD) {
                        auto key = std::make_pair(pt.n_bins, L);
                        auto it = nb_cache.find(key);
                        if (it == nb_cache.end()) {
                            std::vector<int32_t> pos;
                            if (!rcp::neighborhood_positions(pt.n_bins, L, rounding, &pos))
                                return fail(RCP_ESEMANTIC,
                                            "splitVector neighborhood interpolation of %d values into %d bins: R raises an error",
                                            L, pt.n_bins);
                            pos_off = (int32_t)B.nb_pos.size();
                            B.nb_pos.insert(B.nb_pos.end(), pos.begin(), pos.end());
                            nb_cache[key] = pos_off;
                        } else {
                            pos_off = it->second;
                        }
                    } else if (mode == RCP_INTERP_SPLINE && L < 1) {
                        return fail(RCP_ESEMANTIC, "spline() of zero points: R raises an error");
                    } else if (mode == RCP_INTERP_LINEAR && L < 1) {
                        return fail(RCP_EUNSUPPORTED, "empty slice with the 'linear' interpolation");
                    }
                    B.interp_row.push_back(r);
                    B.interp_part.push_back(p);
                    B.interp_mode.push_back(mode);
                    B.interp_pos.push_back(pos_off);
                    max_interp_len = std::max(max_interp_len, L);
                    max_interp_bins = std::max(max_interp_bins, pt.n_bins);
                    continue;
                }
                const int32_t bs = L / pt.n_bins;
                const int32_t dif = L - bs * pt.n_bins;
                if (dif || (bs & (bs - 1))) lean_ok = false;
                // median bins wider than a wave chunk go to the slow-row kernel (mode 4) and do
                // not size the chunks of the others
                if (bins->stat != RCP_STAT_MEDIAN || bs + (dif ? 1 : 0) < kWaveMax)
                    max_bin = std::max(max_bin, bs + (dif ? 1 : 0));
                if (dif) {
                    int32_t& slot = B.lay_index[pt.lay_base + dif];
                    if (slot < 0) {
                        auto key = std::make_pair(pt.n_bins, dif);
                        auto it = layout_cache.find(key);
                        if (it == layout_cache.end()) {
                            const std::vector<int32_t> cnt = rcp::bin_layout_counts(pt.n_bins, dif, rounding);
                            const int32_t o = (int32_t)B.lay_cnt.size();
                            B.lay_cnt.insert(B.lay_cnt.end(), cnt.begin(), cnt.end());
                            B.lay_regions.emplace_back(o, pt.n_bins);
                            layout_cache[key] = o;
                            slot = o;
                        } else {
                            slot = it->second;
                        }
                    }
                }
            }
        }
        out->max_bin[p] = max_bin;
    }
    if (max_interp_len > kChunkMax)
        return fail(RCP_EUNSUPPORTED, "interpolated slice of %d positions exceeds %d", max_interp_len, kChunkMax);
    out->n_cols = col;
    out->pow2_bins = lean_ok;
    out->max_interp_len = max_interp_len;
    out->max_interp_bins = max_interp_bins;
    return RCP_OK;
}

}  // namespace rcpi

namespace {

// ---- the stages of plan_shape.  Each reads the fields the earlier ones wrote.

// Geometry.  A workgroup handles <= kStageMaxBins bins of a part for 32 rows; a wave
// piles a row's positions for those bins in sub-chunks of at most `chunk_cap` positions
// (bins straddling sub-chunks accumulate).  Pick the largest wave chunk (<= kWaveMax) whose
// LDS (4 wave arrays + [bin][row] stage + row metadata) keeps two workgroups per CU.
// Writes the parts' chunking, P.wave_words, P.chunk_cap and P.stage_cap.
void shape_chunks(const RowSummary& S, const PlanParts& Q, bool median, bool cov_only, int32_t min_col_chunks,
                  RcpPlanDev& P) {
    int32_t stage_cap = 1;
    int32_t need = 64;
    for (int p = 0; p < P.n_parts; ++p) {
        RcpPart& pt = P.part[p];
        // equal chunks of at most kStageMaxBins bins
        int32_t nch = (pt.n_bins + kStageMaxBins - 1) / kStageMaxBins;
        int32_t cb = (pt.n_bins + nch - 1) / nch;
        // wide binned chunks would be piled in several wave sub-chunks, each streaming the
        // chunk's reads again: split them into more (up to 8) column chunks instead -- more
        // workgroups for small row counts, and per-chunk read ranges from locate.  The general
        // kernel's cap stays at the 8 chunks its A/B measured (lean plans split further, to
        // RCP_MAX_CRANGE_CHUNKS: split_lean_columns)
        const int32_t pos_max = 1023;
        if (!median && !pt.per_base && Q.max_bin[p] > 0 && (int64_t)cb * Q.max_bin[p] > pos_max) {
            const int32_t cb2 = std::max<int32_t>(1, pos_max / Q.max_bin[p]);
            const int32_t nch2 = (pt.n_bins + cb2 - 1) / cb2;
            if (nch2 <= kGeneralMaxChunks) {
                nch = nch2;
                cb = (pt.n_bins + nch - 1) / nch;
            }
        }
        // opts->min_col_chunks (one-part plans): at least that many column chunks
        if (!median && P.n_parts == 1 && min_col_chunks > nch) {
            nch = std::min<int32_t>(std::min(min_col_chunks, RCP_MAX_CRANGE_CHUNKS), pt.n_bins);
            cb = (pt.n_bins + nch - 1) / nch;
        }
        if (median) cb = std::min<int32_t>(cb, std::max<int32_t>(1, kWaveMax / Q.max_bin[p]));
        pt.chunk_bins = cb;
        pt.n_chunks = (pt.n_bins + cb - 1) / cb;
        stage_cap = std::max(stage_cap, cb);
        need = std::max<int64_t>(need, std::min<int64_t>((int64_t)cb * Q.max_bin[p], kWaveMax));
    }
    if (cov_only) need = std::max(need, std::min(S.max_row_len, kWaveMax));
    int32_t min_cap = 64;
    if (median)
        for (int p = 0; p < P.n_parts; ++p) min_cap = std::max(min_cap, P.part[p].chunk_bins * Q.max_bin[p]);
    const int32_t cands[] = {need, 2047, 1023, 511};  // 64 * 2^k - 1: the +1 sentinel fits
    int32_t chunk_cap = -1;
    for (int32_t ch : cands) {
        if (ch > need || ch < min_cap) continue;
        RcpPlanDev t{};
        int32_t cap_unused = 0;
        wave_geometry(ch, &t.wave_words, &cap_unused);
        t.stage_cap = cov_only ? 0 : stage_cap;
        chunk_cap = ch;
        if (rcp_pileup_lds_bytes(&t, cov_only ? 1 : 0) <= kLdsBudget) break;
    }
    if (chunk_cap < 0) chunk_cap = need;
    wave_geometry(chunk_cap, &P.wave_words, &P.chunk_cap);
    P.stage_cap = stage_cap;
}

// Median plans: rows whose bins exceed the wave chunk take block-level windows (mode 4)
int add_median_window_rows(Builder& B, RcpPlanDev& P) {
    const int R = (int)B.row_len.size();
    for (int p = 0; p < P.n_parts; ++p) {
        const RcpPart& pt = P.part[p];
        if (pt.per_base) continue;
        for (int r = 0; r < R; ++r) {
            if (B.row_static[r] || B.row_seg[r] == B.row_seg[r + 1]) continue;
            int32_t head, L;
            rcp_part_slice(pt, B.row_len[r], &head, &L);
            if (L < pt.n_bins) continue;
            const int32_t bs = L / pt.n_bins, dif = L - bs * pt.n_bins;
            const int32_t w = bs + (dif ? 1 : 0);
            if (w <= P.chunk_cap) continue;
            if (w > kChunkMax)
                return fail(RCP_EUNSUPPORTED, "row %d: a median bin of %d positions exceeds %d", r, w, kChunkMax);
            B.interp_row.push_back(r);
            B.interp_part.push_back(p);
            B.interp_mode.push_back(4);
            B.interp_pos.push_back(dif ? B.lay_index[pt.lay_base + dif] : -1);
            P.interp_cap = std::max(P.interp_cap, w);
        }
    }
    return RCP_OK;
}

// every chunk is one wave pass: its widest row slice fits the wave's difference array (no
// sub-chunks, which read locate's segment ranges)
bool chunks_one_wave_pass(const RcpPlanDev& P, const PlanParts& Q) {
    for (int p = 0; p < P.n_parts; ++p) {
        const RcpPart& pt = P.part[p];
        const int64_t w = pt.per_base ? 1 : Q.max_bin[p];
        if ((int64_t)pt.chunk_bins * w > P.chunk_cap) return false;
    }
    return true;
}

bool all_parts_per_base(const RcpPlanDev& P) {
    for (int p = 0; p < P.n_parts; ++p)
        if (!P.part[p].per_base) return false;
    return true;
}

bool all_parts_binned(const RcpPlanDev& P) {
    for (int p = 0; p < P.n_parts; ++p)
        if (P.part[p].per_base) return false;
    return true;
}

// ---- the pileup kernels' shape rules (plan_shape weighs them against what the caller asked
// for, opts->pileup_kernel)

// the lean kernel and its general-bins mode: a mean plan, each chunk inside one wave's fused
// pass (<= 1023 positions)
bool lean_family_shape(const RcpPlanDev& P, const PlanParts& Q, bool cov_only) {
    return !cov_only && P.stat == RCP_STAT_MEAN && P.chunk_cap <= 1023 && chunks_one_wave_pass(P, Q);
}

// lean pileup kernel: every row one plain range (no exon list, no zero-width query), uniform
// power-of-two bins and the stage inside the store waves' registers
bool lean_shape(const RcpPlanDev& P, const PlanParts& Q, const RowSummary& S, bool cov_only) {
    return lean_family_shape(P, Q, cov_only) && Q.pow2_bins && P.stage_cap <= rcp_lean_max_bins() &&
           S.single_plain_lean;
}

// its general-bins mode: any uniform width, R-RNG layouts and multi-range rows, as long as every
// chunk holds <= rcp_lean_gen_max_bins() bins.  Measured slower than the general kernel on C2
// (0.082 vs 0.063 ms) and C3 (0.96 vs 0.88 ms), so AUTO does not choose it
bool lean_gen_shape(const RcpPlanDev& P, const PlanParts& Q, bool cov_only) {
    return lean_family_shape(P, Q, cov_only) && P.stage_cap <= rcp_lean_gen_max_bins();
}

// row-wave kernel: mean bins of any layout, every bin inside one window
bool rows_shape(const RcpPlanDev& P, const PlanParts& Q, bool cov_only) {
    if (cov_only || P.stat != RCP_STAT_MEAN) return false;
    for (int p = 0; p < P.n_parts; ++p)
        if (!P.part[p].per_base && Q.max_bin[p] > rcp_rows_window_cap()) return false;
    return true;
}

// bin-difference kernel: mean plans of one binned part whose rows are single ranges, every
// row's slice a whole number of bins of >= rcp_bins_min_width() positions (no splitVector
// layout, no interpolation), <= rcp_bins_max_bins() bins.  A row is one wave's pass over its
// bins (no column chunks)
bool bins_shape(const RcpPlanDev& P, const Builder& B, const RowSummary& S, bool cov_only) {
    const RcpPart& pt0 = P.part[0];
    if (cov_only || P.stat != RCP_STAT_MEAN || P.n_parts != 1 || pt0.per_base || pt0.n_bins <= 0 ||
        pt0.n_bins > rcp_bins_max_bins() || !S.single_plain_nonnull || !B.interp_row.empty())
        return false;
    const int R = (int)B.row_len.size();
    for (int r = 0; r < R; ++r) {
        if (B.row_static[r] || B.row_seg[r] == B.row_seg[r + 1]) continue;  // NULL rows: zeros
        int32_t head, L;
        rcp_part_slice(pt0, B.row_len[r], &head, &L);
        if (L < pt0.n_bins || L % pt0.n_bins != 0 || L / pt0.n_bins < rcp_bins_min_width()) return false;
    }
    return true;
}

// Whether the pileup kernel searches its rows' read ranges itself (no locate and heavy
// launches) -- never when the caller asked for the heavy path.
int choose_fold(const PlanFacts& F, const RcpPlanDev& P, const Builder& B, const PlanParts& Q, const RowSummary& S,
                bool cov_only, const rcp_plan_opts* opts) {
    const int R = (int)B.row_len.size();
    if (opts->heavy_threshold > 0) return 0;
    // small tables of single ranges in the merged layout, no row interpolated (rcp_interp_kernel
    // reads locate's segment ranges)
    const bool small_merged = F.ignore_strand && B.interp_row.empty() && R > 0 && R <= kFoldMaxRows;
    switch (P.lean) {
        // each wave searches its rows' (segment, stream) ranges itself (no 64-B record round trip;
        // a skewed row stays with the wave that claimed it)
        case RCP_PILEUP_ROWS: return 1;
        // the locate and heavy launches were as long as the pileup on C2
        case RCP_PILEUP_BINS: return 1;
        // one GPU's shard of a peak table (C4 1/8 spent locate 25 + heavy 8 us ahead of a 93-us
        // pileup): the kernel searches each row's and chunk's read ranges (fold_row) and piles a
        // skewed row with the whole workgroup instead of heavy slices.  Every chunk must be one
        // wave pass
        case RCP_PILEUP_GENERAL:
            return !cov_only && small_merged && chunks_one_wave_pass(P, Q) && S.single_plain_nonnull;
        // one GPU's shard of a per-base table (C5 1/8 spent locate 45 us ahead of a 143-us pileup):
        // the store wave that claims an item searches its rows' read ranges while the pile waves
        // work on the previous item.  (Binned lean plans keep the locate: their skewed rows need
        // the heavy slices.)  Plans built for several samples in flight (rcp_plan_opts.concurrent)
        // of a larger table keep the locate launch: it runs beside another sample's pileup there,
        // while the claim's searches lengthen this kernel (full C5 at D = 2: 0.459-0.463 vs
        // 0.472-0.480 ms a step)
        case RCP_PILEUP_LEAN:
            return all_parts_per_base(P) && small_merged && (opts->concurrent <= 1 || R <= kFoldConcurrentMaxRows) &&
                   !F.no_lean_fold && S.single_plain_nonnull;
        default: return 0;
    }
}

// Lean plans with few row tiles (one GPU's shard of a region table): the persistent grid (two
// workgroups per CU) takes (row tile, column chunk) items; with few items per workgroup the
// last ones leave most workgroups idle, so cut the parts into more column chunks (each streams
// only its reads: crange) until there are >= kLeanItemsPerWg[Base] per workgroup, or
// min_col_chunks asks for more
void split_lean_columns(const PlanFacts& F, int R, bool lean_base, int32_t min_col_chunks, RcpPlanDev& P) {
    const int64_t grid = (2 * (int64_t)F.n_cus + 7) / 8 * 8;
    const int64_t trows = P.lean_rounds == 2 ? 32 : rcp_tile_rows();
    const int64_t tiles = ((int64_t)R + trows - 1) / trows;
    auto can_split = [&]() {
        if (P.n_chunks_total * 2 > RCP_MAX_CRANGE_CHUNKS) return false;
        for (int p = 0; p < P.n_parts; ++p)
            if (P.part[p].chunk_bins < 2 * kLeanMinChunkBins) return false;
        return true;
    };
    auto split = [&]() {
        P.n_chunks_total = 0;
        for (int p = 0; p < P.n_parts; ++p) {
            RcpPart& pt = P.part[p];
            const int32_t nch = 2 * pt.n_chunks;
            pt.chunk_bins = (pt.n_bins + nch - 1) / nch;
            pt.n_chunks = (pt.n_bins + pt.chunk_bins - 1) / pt.chunk_bins;
            P.n_chunks_total += pt.n_chunks;
        }
    };
    const int64_t want = (lean_base ? kLeanItemsPerWgBase : kLeanItemsPerWg) * grid;
    while (can_split() && (tiles * P.n_chunks_total < want || P.n_chunks_total < min_col_chunks)) split();
    P.stage_cap = 1;
    for (int p = 0; p < P.n_parts; ++p) P.stage_cap = std::max(P.stage_cap, P.part[p].chunk_bins);
}

// locate keeps the per-chunk read ranges of single-range rows (RcpPlanDev::crange)
bool keeps_crange(const RcpPlanDev& P) { return P.n_chunks_total > 1 && P.n_chunks_total <= RCP_MAX_CRANGE_CHUNKS; }

}  // namespace

namespace rcpi {

int plan_shape(const PlanFacts& F, const RowSummary& S, const PlanParts& Q, const rcp_bins_desc* bins, bool cov_only,
               const rcp_plan_opts* opts, Builder* Bp, rcp_plan* plan) {
    Builder& B = *Bp;
    RcpPlanDev& P = plan->dev;
    const int R = (int)B.row_len.size();
    plan->n_rows = R;
    plan->n_seg = (int64_t)B.segs.size();
    plan->max_row_len = S.max_row_len;
    P.n_rows = R;
    P.n_chrom = F.n_chrom;
    P.n_cus = F.n_cus;
    P.merged = F.ignore_strand ? 1 : 0;
    P.multi_rows = S.multi_rows;
    // persistent pileup grids: all workgroup slots alone, 7/8 beside other samples in flight
    // (rcp_plan_opts.concurrent; profiles/r04/r4p)
    P.grid_fill = opts->concurrent > 1 ? 7 : 8;

    shape_chunks(S, Q, bins->stat == RCP_STAT_MEDIAN, cov_only, opts->min_col_chunks, P);
    P.n_cols = Q.n_cols;
    plan->n_cols = Q.n_cols;
    if (opts->out_ld == RCP_OUT_LD_PADDED) P.out_ld = ((int64_t)R + 15) & ~int64_t(15);
    else if (opts->out_ld == 0) P.out_ld = R;
    else if (opts->out_ld >= R) P.out_ld = opts->out_ld;
    else return fail(RCP_EINVAL, "out_ld = %lld < n_rows = %d", (long long)opts->out_ld, R);
    plan->out_ld = P.out_ld;
    P.interp_cap = std::max(Q.max_interp_len, 1);
    if (bins->stat == RCP_STAT_MEDIAN) {
        const int rc = add_median_window_rows(B, P);
        if (rc) return rc;
    }
    P.n_chunks_total = 0;
    for (int p = 0; p < P.n_parts; ++p) P.n_chunks_total += P.part[p].n_chunks;

    // ---- the pileup kernel.  RCP_KERNEL_GENERAL keeps every plan on the general kernel; _LEAN,
    // _LEAN_ANY, _ROWS and _BINS take their kernel where the shape allows it; AUTO takes
    //   the bin-difference kernel wherever the shape allows it (C2: 200 bins of 20 bp),
    //   the lean kernel for per-base plans and for binned ones of >= kLeanMinRowsBinned rows,
    //   the row-wave kernel for other plans with multi-range rows (coverageRnaRef, genebody + flanks)
    const int kind = opts->pileup_kernel;
    const bool lean = kind != RCP_KERNEL_GENERAL && lean_shape(P, Q, S, cov_only) &&
                      !(kind == RCP_KERNEL_AUTO && R < kLeanMinRowsBinned && all_parts_binned(P));
    const bool lean_gen = !lean && kind == RCP_KERNEL_LEAN_ANY && lean_gen_shape(P, Q, cov_only);
    const bool row_wave = !lean && (kind == RCP_KERNEL_ROWS || (kind == RCP_KERNEL_AUTO && S.multi_rows)) &&
                          rows_shape(P, Q, cov_only);
    const bool bin_diff = (kind == RCP_KERNEL_AUTO || kind == RCP_KERNEL_BINS) && bins_shape(P, B, S, cov_only);
    P.lean = bin_diff ? RCP_PILEUP_BINS
             : row_wave ? RCP_PILEUP_ROWS
             : lean     ? RCP_PILEUP_LEAN
             : lean_gen ? RCP_PILEUP_LEAN_GEN
                        : RCP_PILEUP_GENERAL;
    // Per-base lean plans (baseCoverageMatrix: every part one column per position) take work
    // items of two 16-row rounds instead of four: ms per pass four / two rounds, C5 0.752 / 0.673,
    // its 1/8 shard 0.272 / 0.253, 1/4 0.319 / 0.290; binned C4 is slower with them (0.553 / 0.563
    // pileup; 1/8 shard 0.107 / 0.115).  profiles/r03/pipeline/lean_rounds_ab.log
    // (RCP_LEAN_ROUNDS=2: diagnostics A/B of two-round items for binned lean plans.)  Set from
    // the lean shape alone: a plan the bin-difference kernel takes from the lean one keeps the
    // knob's value, which that kernel does not read
    const bool per_base = all_parts_per_base(P);
    P.lean_rounds = (lean || lean_gen) && (per_base || F.lean_rounds2) ? 2 : 0;
    const bool lean_base = P.lean == RCP_PILEUP_LEAN && per_base;  // a lean plan whose every part is per base
    if (P.lean == RCP_PILEUP_BINS) {  // a row is one wave's pass over its bins: no column chunks
        P.part[0].chunk_bins = P.part[0].n_bins;
        P.part[0].n_chunks = 1;
        P.n_chunks_total = 1;
        P.stage_cap = P.part[0].n_bins;
    }
    P.fold = choose_fold(F, P, B, Q, S, cov_only, opts);
    P.coop_min = F.coop_min >= 0 ? F.coop_min : kCoopMin;
    if (P.lean == RCP_PILEUP_LEAN && R > 0) split_lean_columns(F, R, lean_base, opts->min_col_chunks, P);

    // ---- skewed rows: heavy slots sized for the eligible (short enough) rows
    const int32_t heavy_thr = opts->heavy_threshold < 0 ? kHeavyThreshold : opts->heavy_threshold;
    P.heavy_threshold = heavy_thr;
    P.heavy_max_len = S.max_heavy_len;
    P.heavy_stride = ((S.max_heavy_len + 1) + 63) & ~63;
    P.heavy_slice = kHeavySlice;
    P.heavy_cap = (int32_t)std::min<int64_t>(std::max(R, 1), std::min<int64_t>(4096, (256ll << 20) / (4ll * P.heavy_stride)));
    if (heavy_thr <= 0 || R == 0 || P.fold) P.heavy_threshold = 0;

    // heaviest-first lean items (rcp_device.h lpt): per-base lean plans of few 32-row items,
    // i.e. one GPU's shard of a per-base table (C5 1/8: TSS windows' middle column chunks hold
    // several times the outer chunks' reads; in per-XCD order a workgroup that drew two heavy
    // items sets the pass)
    // (a full per-base table, e.g. C5's 6256 items, keeps the per-XCD order and its L2 locality)
    const int64_t lpt_items = ((int64_t)R + 31) / 32 * P.n_chunks_total;
    P.lpt = lean_base && keeps_crange(P) && R > 0 && !P.fold && lpt_items <= (int64_t)kLeanItemsPerWgBase * 2 * F.n_cus;
    P.lpt_cap = P.lpt ? (int32_t)lpt_items : 0;

    // uniform-width reads: the general kernel and per-base lean plans stream the starts alone;
    // binned lean plans keep the (start, end) pairs -- C4's latency-bound pile measured 4 % slower
    // with starts (pileup 0.578 vs 0.555 ms, same box), C5's dense per-base rows 6 % faster
    // (0.58 vs 0.62), the 1/8 C4 shard's general kernel 4 % (profiles/r03/pipeline/general_starts_ab.log,
    // lean_starts_c4_ab.log)
    plan->use_st = F.has_st && (P.lean != RCP_PILEUP_LEAN || lean_base);

    P.n_interp = (int32_t)B.interp_row.size();
    // x (L+1) | b, c, d (3 (L+1)) for the spline, or the neighborhood fill's n pre-fill values
    P.interp_stride = (Q.max_interp_len + 1) + std::max(Q.max_interp_bins, 3 * (Q.max_interp_len + 1)) + 8;

    switch (P.lean) {
        case RCP_PILEUP_BINS: plan->lds = rcp_pileup_bins_lds_bytes(&P); break;
        case RCP_PILEUP_ROWS: plan->lds = rcp_pileup_rows_lds_bytes(&P); break;
        case RCP_PILEUP_GENERAL: plan->lds = rcp_pileup_lds_bytes(&P, cov_only ? 1 : 0); break;
        default: plan->lds = rcp_pileup_lean_lds_bytes(&P); break;
    }
    // the row-wave kernel's persistent grid holds one workgroup per CU for the whole pass: the
    // interpolation rows (a side stream, forked after locate) fit beside it only in the LDS it
    // leaves -- their spline arrays then go to global scratch (C3: 148 KB + 4 KB, vs 20 KB that
    // waited for the pileup to end)
    P.interp_lds_budget =
        P.lean == RCP_PILEUP_ROWS ? (int32_t)std::max<int64_t>(0, 160 * 1024 - (int64_t)plan->lds) : 0;
    // general kernel: 2 rounds (32 rows) per workgroup (C3: 0.88 ms vs 0.91 with 4 rounds, 0.89
    // with 1), 1 when the row table is small, so that the grid still holds two workgroups per
    // CU (C2: 10k rows -> 625 workgroups instead of 157; pileup 0.076 -> 0.063 ms)
    int tile = 16, rmax = 4;
    rcp_tile_geometry(&tile, &rmax);
    P.rounds = std::min(rmax, 2);
    while (P.rounds > 1 &&
           (int64_t)((R + tile * P.rounds - 1) / (tile * P.rounds)) * P.n_chunks_total < 2 * (int64_t)F.n_cus)
        P.rounds /= 2;
    // (RCP_GEN_ROUNDS: diagnostics A/B of the rounds per workgroup, 1 / 2 / 4)
    if (F.gen_rounds == 1 || F.gen_rounds == 2 || F.gen_rounds == 4) P.rounds = std::min(F.gen_rounds, rmax);
    switch (P.lean) {
        case RCP_PILEUP_BINS: plan->tile_rows = tile; break;
        case RCP_PILEUP_GENERAL: plan->tile_rows = tile * P.rounds; break;
        default: plan->tile_rows = P.lean_rounds == 2 ? 2 * tile : rcp_tile_rows(); break;
    }
    plan->grid = (int64_t)((R + plan->tile_rows - 1) / plan->tile_rows) * P.n_chunks_total;
    if (P.lean == RCP_PILEUP_BINS) plan->grid = (plan->grid + 7) / 8 * 8;
    if (plan->lds > 160 * 1024) return fail(RCP_EUNSUPPORTED, "plan needs %zu B of LDS", plan->lds);
    return RCP_OK;
}

}  // namespace rcpi

// =====================================================================================
// tables, device memory, the C ABI
// =====================================================================================

namespace {

// The plan's device tables as one arena: pieces are laid out (256-B aligned) and then copied
// straight from the host vectors through the pinned staging buffers (rcp_stage.h) -- no host
// blob to assemble (C4: 26 MB, ~15 ms of host copies and page faults into a fresh vector).
struct Arena {
    struct Piece {
        const void* p;
        size_t bytes, off;
    };
    std::vector<Piece> pieces;
    size_t total = 0;
    template <class T>
    size_t add(const std::vector<T>& v) {
        const size_t off = (total + 255) & ~size_t(255);
        if (!v.empty()) pieces.push_back({v.data(), sizeof(T) * v.size(), off});
        total = off + sizeof(T) * std::max<size_t>(v.size(), 1);
        return off;
    }
    hipError_t upload(void* dev, int device, hipStream_t s) const {
        for (const Piece& q : pieces) {
            const hipError_t e = rcp::stage_h2d(static_cast<char*>(dev) + q.off, q.p, q.bytes, device, s);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
};

}  // namespace

namespace {

// The host tables a plan uploads beside Builder's, and where each lies in the arena.
struct PlanTables {
    std::vector<uint32_t> lay_bit;
    std::vector<int32_t> interp_of, tile_perm;
    std::vector<RcpRowInfo> row_info;
    std::vector<double> spl_tb;
    Arena blob;
    size_t o_row_chrom, o_row_seg, o_row_len, o_row_static, o_segs, o_lay_index, o_lay_cnt, o_lay_bit, o_irow, o_ipart,
        o_imode, o_ipos, o_iof, o_tperm, o_nb, o_rinfo, o_spl;
};

// The locate kernel's chunk windows for the rows of the first row's length (all rows of
// C2 / C4 / C5), when no part of that length has an R-RNG layout: the same arithmetic as
// the kernel's chunk_window, once per plan instead of once per (row, chunk)
void chunk_window_table(const Builder& B, RcpPlanDev& P) {
    P.cw_len = -1;
    if (!keeps_crange(P) || P.n_rows == 0) return;
    const int32_t nr = B.row_len[0];
    int c = 0;
    for (int p = 0; p < P.n_parts; ++p) {
        const RcpPart& pt = P.part[p];
        for (int cp = 0; cp < pt.n_chunks; ++cp, ++c) {
            int32_t head, L;
            rcp_part_slice(pt, nr, &head, &L);
            const int32_t n = pt.n_bins, k0 = cp * pt.chunk_bins;
            P.cw[2 * c] = 0;
            P.cw[2 * c + 1] = -1;
            if (k0 >= n || (pt.per_base ? L != n : L < n)) continue;
            const int32_t bs = pt.per_base ? 1 : L / n;
            if (!pt.per_base && L - bs * n != 0) return;  // an R-RNG layout: the kernel computes these rows itself
            if (P.stat == 1 && bs > P.chunk_cap) continue;
            const int32_t kend = std::min(k0 + pt.chunk_bins, n);
            P.cw[2 * c] = head + bs * k0;
            P.cw[2 * c + 1] = bs * (kend - k0);
        }
    }
    P.cw_len = nr;
}

// The tables of the shaped plan that Builder does not hold yet, all laid out in T->blob (B and
// *T must outlive the upload: the arena copies straight from their vectors), and P.cw.
void plan_tables(const rcp_readset* rs, const ReadLayout& RL, const Builder& B, const PlanParts& Q, RcpPlanDev& P,
                 PlanTables* T) {
    const int R = P.n_rows;
    Arena& blob = T->blob;
    T->o_row_chrom = blob.add(B.row_chrom);
    T->o_row_seg = blob.add(B.row_seg);
    T->o_row_len = blob.add(B.row_len);
    T->o_row_static = blob.add(B.row_static);
    T->o_segs = blob.add(B.segs);
    T->o_lay_index = blob.add(B.lay_index);
    T->o_lay_cnt = blob.add(B.lay_cnt);
    // the same layouts as bit masks (word lay + j: bins 32 j .. 32 j + 31 enlarged), indexed
    // like lay_cnt: one load per 32 bins where the row-wave flush needs the bin widths
    T->lay_bit.assign(B.lay_cnt.size(), 0u);
    for (const auto& rg : B.lay_regions)
        for (int32_t k = 0; k < rg.second; ++k)
            if (B.lay_cnt[rg.first + k + 1] != B.lay_cnt[rg.first + k]) T->lay_bit[rg.first + (k >> 5)] |= 1u << (k & 31);
    T->o_lay_bit = blob.add(T->lay_bit);
    T->o_irow = blob.add(B.interp_row);
    T->o_ipart = blob.add(B.interp_part);
    T->o_imode = blob.add(B.interp_mode);
    T->o_ipos = blob.add(B.interp_pos);
    // row-wave plans interpolate the rows they pile (rcp_pileup_rows_kernel): entry of (row, part)
    if (P.lean == RCP_PILEUP_ROWS && !B.interp_row.empty()) {
        T->interp_of.assign((size_t)R * P.n_parts, -1);
        for (size_t e = 0; e < B.interp_row.size(); ++e)
            T->interp_of[(size_t)B.interp_row[e] * P.n_parts + B.interp_part[e]] = (int32_t)e;
    }
    T->o_iof = blob.add(T->interp_of);
    // ... and claim the 16-row tiles holding such rows first, most first: the spline's serial
    // chains then run beside the other waves' pileup, not in the grid's tail
    if (!T->interp_of.empty()) {
        const int32_t n_tiles = (R + 15) / 16;
        std::vector<int32_t> cnt(n_tiles, 0);
        for (int32_t r : B.interp_row) ++cnt[r / 16];
        T->tile_perm.resize(n_tiles);
        for (int32_t t = 0; t < n_tiles; ++t) T->tile_perm[t] = t;
        std::stable_sort(T->tile_perm.begin(), T->tile_perm.end(), [&](int32_t a, int32_t b) { return cnt[a] > cnt[b]; });
    }
    T->o_tperm = blob.add(T->tile_perm);
    T->o_nb = blob.add(B.nb_pos);
    // locate's per-row input (RcpRowInfo)
    T->row_info.resize((size_t)std::max(R, 1));
    for (int r = 0; r < R; ++r) {
        RcpRowInfo& ri = T->row_info[r];
        std::memset(&ri, 0, sizeof(ri));
        ri.j0 = B.row_seg[r];
        ri.j1 = B.row_seg[r + 1];
        ri.chrom = B.row_chrom[r];
        ri.row_len = B.row_len[r];
        ri.stat = B.row_static[r];
        const bool cok = ri.chrom >= 0 && ri.chrom < rs->n_chrom;
        ri.seqlen = cok ? rs->seqlen[ri.chrom] : -1;
        if (cok) {
            ri.d0 = RL.h_dir_off[(size_t)ri.chrom * 3];
            ri.nb = (int32_t)(RL.h_dir_off[(size_t)ri.chrom * 3 + 1] - ri.d0) - 1;
        }
        if (ri.j1 > ri.j0) ri.seg0 = B.segs[ri.j0];
    }
    T->o_rinfo = blob.add(T->row_info);
    // fmm pivots (see RcpPlanDev::spl_tb): the elimination of R's fmm_spline with d[i] = 1
    T->spl_tb.assign(2 * ((size_t)std::max(Q.max_interp_len, 1) + 1), 0.0);
    {
        double bp = -1.0;
        T->spl_tb[1] = bp;
        for (size_t i = 1; 2 * i + 1 < T->spl_tb.size(); ++i) {
            const double t = 1.0 / bp;
            bp = 4.0 - t;
            T->spl_tb[2 * i] = t;
            T->spl_tb[2 * i + 1] = bp;
        }
    }
    T->o_spl = blob.add(T->spl_tb);
    chunk_window_table(B, P);
}

// The plan's device memory: the table arena (uploaded), the work arena (locate outputs,
// heavy-row state, status words; cleared), the interpolation scratch and the row-wave stage; and
// every pointer of plan->dev, into them and into the readset's layout.
int plan_bind(const rcp_readset* rs, const ReadLayout& RL, const PlanTables& T, rcp_plan* plan, PlanTimer& ptimer) {
    RcpPlanDev& P = plan->dev;
    const int R = P.n_rows;
    HIP_TRY(plan->tables.alloc(T.blob.total, nullptr));
    HIP_TRY(T.blob.upload(plan->tables.p, rs->device, nullptr));
    PLAN_MARK("tables upload");
    char* base = plan->tables.as<char>();
    // ---- work arena: locate outputs, heavy-row state, status words
    const int64_t S = std::max<int64_t>(plan->n_seg, 1);
    const int64_t Rw = std::max(R, 1);
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t w_lo = 0;
    const size_t w_hi = al(w_lo + 12 * S);
    const size_t w_valid = al(w_hi + 12 * S);
    const size_t w_ncand = al(w_valid + Rw);
    const size_t w_hrows = al(w_ncand + 4 * Rw);
    const size_t w_hoff = al(w_hrows + 4 * (size_t)P.heavy_cap);
    const size_t w_gdiff = al(w_hoff + 4 * ((size_t)P.heavy_cap + 1));
    const size_t w_rec = al(w_gdiff + (P.heavy_threshold > 0 ? 4 * (size_t)P.heavy_cap * P.heavy_stride : 0));
    const bool keep_crange = keeps_crange(P);
    const size_t w_crange = al(w_rec + sizeof(RcpRowRec) * Rw);
    const size_t w_order = al(w_crange + (keep_crange ? sizeof(uint2) * 3 * (size_t)P.n_chunks_total * Rw : 0));
    const size_t w_status = al(w_order + 4 * (size_t)RCP_LPT_CLASSES * (size_t)P.lpt_cap);
    static_assert(2 * RCP_STATUS_WORDS * 4 <= 256, "two status sets");
    HIP_TRY(plan->work.alloc(w_status + 256, nullptr));
    PLAN_MARK("work alloc");
    char* wb = plan->work.as<char>();
    P.ncand = reinterpret_cast<uint32_t*>(wb + w_ncand);
    P.heavy_rows = reinterpret_cast<int32_t*>(wb + w_hrows);
    P.heavy_nslice = reinterpret_cast<uint32_t*>(wb + w_hoff);
    P.heavy_gdiff = reinterpret_cast<int32_t*>(wb + w_gdiff);
    P.rec = reinterpret_cast<RcpRowRec*>(wb + w_rec);
    P.crange = keep_crange ? reinterpret_cast<uint2*>(wb + w_crange) : nullptr;
    P.item_order = P.lpt ? reinterpret_cast<int32_t*>(wb + w_order) : nullptr;
    if (P.n_interp) HIP_TRY(plan->scratch.alloc(8 * (size_t)P.n_interp * P.interp_stride, nullptr));

    P.se = RL.se.as<int2>();
    P.st = plan->use_st ? RL.st.as<int32_t>() : nullptr;
    P.st_w = RL.st_w;
    P.pmax = RL.pmax.as<int32_t>();
    P.stream_off = RL.stream_off.as<int64_t>();
    P.seqlen = rs->d_seqlen.as<int64_t>();
    P.dir_l = RL.dir_l.as<int32_t>();
    P.dir_u = RL.dir_l.as<int32_t>() + 1;  // interleaved with dir_l (stride 2)
    P.dir_off = RL.dir_off.as<int64_t>();
    P.dir_k = RL.dir_k.as<int32_t>();
    P.dir_shift = RL.dir_shift;
    P.row_chrom = reinterpret_cast<const int32_t*>(base + T.o_row_chrom);
    P.row_seg = reinterpret_cast<const int32_t*>(base + T.o_row_seg);
    P.row_len = reinterpret_cast<const int32_t*>(base + T.o_row_len);
    P.row_static = reinterpret_cast<const uint8_t*>(base + T.o_row_static);
    P.segs = reinterpret_cast<const RcpSeg*>(base + T.o_segs);
    P.row_info = reinterpret_cast<const RcpRowInfo*>(base + T.o_rinfo);
    P.seg_lo = reinterpret_cast<uint32_t*>(wb + w_lo);
    P.seg_hi = reinterpret_cast<uint32_t*>(wb + w_hi);
    P.valid = reinterpret_cast<uint8_t*>(wb + w_valid);
    plan->status_sets = reinterpret_cast<uint32_t*>(wb + w_status);
    P.status = plan->status_sets;  // set by begin_exec per execution
    P.status_prev = plan->status_sets + RCP_STATUS_WORDS;
    P.lay_index = reinterpret_cast<const int32_t*>(base + T.o_lay_index);
    P.lay_cnt = reinterpret_cast<const int32_t*>(base + T.o_lay_cnt);
    P.lay_bit = reinterpret_cast<const uint32_t*>(base + T.o_lay_bit);
    P.interp_row = reinterpret_cast<const int32_t*>(base + T.o_irow);
    P.interp_part = reinterpret_cast<const int32_t*>(base + T.o_ipart);
    P.interp_mode = reinterpret_cast<const int32_t*>(base + T.o_imode);
    P.interp_pos = reinterpret_cast<const int32_t*>(base + T.o_ipos);
    P.interp_of = T.interp_of.empty() ? nullptr : reinterpret_cast<const int32_t*>(base + T.o_iof);
    P.tile_perm = T.tile_perm.empty() ? nullptr : reinterpret_cast<const int32_t*>(base + T.o_tperm);
    P.nb_pos = reinterpret_cast<const int32_t*>(base + T.o_nb);
    P.spl_tb = reinterpret_cast<const double*>(base + T.o_spl);
    P.interp_scratch = plan->scratch.as<double>();
    P.csr_off = nullptr;
    P.csr_out = nullptr;
    P.csr_rs = nullptr;
    P.csr_sub = nullptr;
    P.csr_sub_off = nullptr;
    // row-wave plans whose tile stage does not fit LDS stage their bin numerators row-major
    // (uint32 numerators, divided at the flush)
    P.rm32 = nullptr;
    P.rinfo = nullptr;
    if (P.lean == RCP_PILEUP_ROWS && R > 0 && P.n_cols > 0) {
        HIP_TRY(plan->rm.alloc(4 * (size_t)R * (size_t)P.n_cols + 8 * (size_t)R * RCP_MAX_PARTS, nullptr));
        P.rinfo = plan->rm.as<int2>();
        P.rm32 = reinterpret_cast<uint32_t*>(P.rinfo + (size_t)R * RCP_MAX_PARTS);
    }
    PLAN_MARK("rest");
    // cleared before the plan is returned: its executions run on the caller's (non-blocking)
    // streams, which do not wait for the null stream
    HIP_TRY(hipMemsetAsync(plan->work.p, 0, plan->work.bytes, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    PLAN_MARK("memset");
    return RCP_OK;
}

// compute units of the device: the persistent grids' and the general kernel's rounds are sized by them
int device_cus(int device) {
    int cus = 256;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}

// the diagnostics knobs of the environment: the only place the planner reads it
void read_env_knobs(PlanFacts* F) {
    const char* e = std::getenv("RCP_LEAN_ROUNDS");
    F->lean_rounds2 = e && std::atoi(e) == 2;
    F->no_lean_fold = std::getenv("RCP_NO_LEAN_FOLD") != nullptr;
    e = std::getenv("RCP_COOP_MIN");
    F->coop_min = e ? std::max(0, std::atoi(e)) : -1;
    e = std::getenv("RCP_GEN_ROUNDS");
    F->gen_rounds = e ? std::atoi(e) : 0;
}

}  // namespace

extern "C" int rcp_plan_create(const rcp_readset* rs, const rcp_rows_desc* rows, const rcp_bins_desc* bins,
                               rcp_plan** out) {
    RCP_TRY
    return rcp_plan_create_ex(rs, rows, bins, nullptr, out);
    RCP_CATCH
}

extern "C" int rcp_plan_create_ex(const rcp_readset* rs, const rcp_rows_desc* rows, const rcp_bins_desc* bins,
                                  const rcp_plan_opts* opts, rcp_plan** out) {
    RCP_TRY
    if (!rs || !rows || !out) return fail(RCP_EINVAL, "NULL argument");
    const rcp_plan_opts default_opts{RCP_KERNEL_AUTO, -1, 0, 0, 0, {0, 0}};
    if (!opts) opts = &default_opts;
    if (opts->pileup_kernel < RCP_KERNEL_AUTO || opts->pileup_kernel > RCP_KERNEL_BINS)
        return fail(RCP_EINVAL, "pileup_kernel = %d", opts->pileup_kernel);
    if (opts->concurrent < 0) return fail(RCP_EINVAL, "concurrent = %d", opts->concurrent);
    *out = nullptr;
    const rcp_bins_desc coverage_only{};  // bins == NULL: a calcCoverage-only plan
    const bool cov_only = bins == nullptr;
    if (cov_only) bins = &coverage_only;
    if (rows->n_rows < 0) return fail(RCP_EINVAL, "n_rows < 0");
    if (rows->n_rows > 0 && (!rows->seg_off || !rows->seg_chrom || !rows->seg_start || !rows->seg_end || !rows->seg_strand))
        return fail(RCP_EINVAL, "NULL row array");
    if (!cov_only && (bins->n_parts < 1 || bins->n_parts > RCP_MAX_PARTS))
        return fail(RCP_EINVAL, "n_parts = %d", bins->n_parts);
    if (bins->stat != RCP_STAT_MEAN && bins->stat != RCP_STAT_MEDIAN) return fail(RCP_EINVAL, "stat = %d", bins->stat);
    if (bins->interp < 0 || bins->interp > 3) return fail(RCP_EINVAL, "interp = %d", bins->interp);
    DeviceGuard g(rs->device);
    HIP_TRY(g.err);

    PlanTimer ptimer;
    if (!rows->ignore_strand) {  // findOverlaps with strand compatibility: the stranded layout
        const int rc0 = ensure_stranded(rs);
        if (rc0) return rc0;
    } else if (!rs->has_merged) {
        return fail(RCP_EINVAL, "this readset holds no strand-merged layout (a shard built for ignore.strand = FALSE)");
    }
    const ReadLayout& RL = rows->ignore_strand ? rs->merged : rs->stranded;
    PlanFacts F;
    F.n_cus = device_cus(rs->device);
    F.ignore_strand = rows->ignore_strand;
    F.has_st = RL.st.p != nullptr;
    F.n_chrom = rs->n_chrom;
    read_env_knobs(&F);

    auto plan = std::make_unique<rcp_plan>();
    plan->rs = rs;
    Builder B;
    int rc = build_rows(F.n_chrom, rows, &B);
    if (rc) return rc;
    PLAN_MARK("build_rows");
    plan->row_len.assign(B.row_len.begin(), B.row_len.end());
    const RowSummary S = summarize_rows(B);
    PlanParts Q;
    if ((rc = plan_parts(bins, &B, &plan->dev, &Q)) != 0) return rc;
    if ((rc = plan_shape(F, S, Q, bins, cov_only, opts, &B, plan.get())) != 0) return rc;
    PLAN_MARK("parts+geometry");
    PlanTables T;
    plan_tables(rs, RL, B, Q, plan->dev, &T);
    PLAN_MARK("tables (host)");
    if ((rc = plan_bind(rs, RL, T, plan.get(), ptimer)) != 0) return rc;
    *out = plan.release();
    return RCP_OK;
    RCP_CATCH
}

// =====================================================================================
// executions
// =====================================================================================

namespace rcpi {

// A new execution: alternate the status sets (RcpPlanDev::status / status_prev); the locate
// kernel clears the previous execution's heavy slots and zeroes its set.
// after an execution's launches on s: the plan's arrays stay allocated until this point (rcp_plan)
int end_exec(rcp_plan* plan, hipStream_t s) {
    if (plan->n_streams == 0) {
        plan->last = s;
        plan->n_streams = 1;
    } else if (plan->last != s) {
        plan->n_streams = 2;
    }
    if (!plan->ev_done) HIP_TRY(hipEventCreateWithFlags(&plan->ev_done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(plan->ev_done, s));
    return RCP_OK;
}

void begin_exec(rcp_plan* plan) {
    plan->epoch ^= 1;
    plan->dev.status = plan->status_sets + RCP_STATUS_WORDS * plan->epoch;
    plan->dev.status_prev = plan->status_sets + RCP_STATUS_WORDS * (plan->epoch ^ 1);
}

}  // namespace rcpi

extern "C" int rcp_plan_destroy(rcp_plan* plan) {
    RCP_TRY
    if (!plan) return RCP_OK;
    DeviceGuard g(plan->rs->device);
    delete plan;
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_plan_info_get(const rcp_plan* plan, rcp_plan_info* info) {
    RCP_TRY
    if (!plan || !info) return fail(RCP_EINVAL, "NULL argument");
    info->n_cols = plan->n_cols;
    info->n_segments = plan->n_seg;
    info->n_interp_rows = plan->dev.n_interp;
    info->lds_bytes = (int64_t)plan->lds;
    info->grid = plan->grid;
    info->tile_rows = plan->tile_rows;
    info->chunk_positions = plan->dev.chunk_cap;
    info->pileup_kernel = plan->dev.lean;
    info->read_bytes = plan->use_st ? 4 : 8;
    info->out_ld = plan->out_ld;
    info->fold = plan->dev.fold;
    info->reserved = 0;
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_plan_row_lengths(const rcp_plan* plan, int64_t* out_len) {
    RCP_TRY
    if (!plan || !out_len) return fail(RCP_EINVAL, "NULL argument");
    std::memcpy(out_len, plan->row_len.data(), 8 * plan->row_len.size());
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_plan_validity(rcp_plan* plan, uint8_t* d_valid, void* hip_stream) {
    RCP_TRY
    if (!plan) return fail(RCP_EINVAL, "NULL plan");
    DeviceGuard g(plan->rs->device);
    HIP_TRY(g.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    begin_exec(plan);
    RcpPlanDev Q = plan->dev;
    Q.valid_out = d_valid;
    HIP_TRY(rcp_launch_locate(&Q, s));
    Q.heavy_threshold = 0;  // no slices: the heavy launch only zeroes the previous status set
    HIP_TRY(rcp_launch_heavy(&Q, kHeavyGrid, s));
    return end_exec(plan, s);
    RCP_CATCH
}

extern "C" int rcp_plan_execute_stages(rcp_plan* plan, double* d_out, uint8_t* d_valid, int64_t* d_binsum,
                                       void* hip_stream, int stages) {
    RCP_TRY
    if (!plan) return fail(RCP_EINVAL, "NULL plan");
    if (plan->dev.n_parts == 0) return fail(RCP_EINVAL, "coverage-only plan (created with bins == NULL)");
    if (!d_out && plan->n_rows && plan->n_cols) return fail(RCP_EINVAL, "NULL output");
    DeviceGuard g(plan->rs->device);
    HIP_TRY(g.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (stages & RCP_STAGE_LOCATE) {
        // locate (also clears the previous execution's heavy slots and status words, and writes
        // the caller's validity vector), heavy slices; a folded plan's pileup kernel does both
        begin_exec(plan);
        if (!plan->dev.fold) {
            RcpPlanDev Q = plan->dev;
            Q.valid_out = d_valid;
            HIP_TRY(rcp_launch_locate(&Q, s));
            HIP_TRY(rcp_launch_heavy(&Q, kHeavyGrid, s));
        }
    }
    // rows with fewer positions than bins (splines of short genes: serial chains) write only their
    // own cells.  Row-wave plans with the HBM stage pile them in the pileup kernel (interp_stage:
    // the interpolation kernel, after it, reads their depth from the stage -- no second pileup of
    // the row); other plans' interpolation reads only locate's outputs and runs on a side stream
    // beside the pileup, joining the caller's stream after it
    plan->dev.interp_stage = (plan->dev.lean == RCP_PILEUP_ROWS && plan->dev.rm32 && !d_binsum) ? 1 : 0;
    const bool fork = (stages & RCP_STAGE_PILEUP) && (stages & RCP_STAGE_INTERP) && plan->dev.n_interp > 0 &&
                      !plan->dev.interp_stage && !plan->dev.fold;  // (folded: the pileup kernel locates)
    if (fork) {
        if (!plan->side) {
            HIP_TRY(hipStreamCreateWithFlags(&plan->side, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&plan->ev_fork, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&plan->ev_join, hipEventDisableTiming));
        }
        HIP_TRY(hipEventRecord(plan->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(plan->side, plan->ev_fork, 0));
        HIP_TRY(rcp_launch_interp(&plan->dev, d_out, plan->side));
        HIP_TRY(hipEventRecord(plan->ev_join, plan->side));
    }
    if (stages & RCP_STAGE_PILEUP) {
        RcpPlanDev Q = plan->dev;
        if (Q.fold) Q.valid_out = d_valid;
        HIP_TRY(rcp_launch_pileup(&Q, d_out, d_binsum, 0, s));
    }
    // (row-wave plans with the HBM stage interpolate in the pileup kernel: the wave that piled
    // the row runs its spline)
    const bool fused = plan->dev.interp_stage && plan->dev.interp_of;
    if (fork) HIP_TRY(hipStreamWaitEvent(s, plan->ev_join, 0));
    else if ((stages & RCP_STAGE_INTERP) && !fused) HIP_TRY(rcp_launch_interp(&plan->dev, d_out, s));
    return end_exec(plan, s);
    RCP_CATCH
}

extern "C" int rcp_plan_execute(rcp_plan* plan, double* d_out, uint8_t* d_valid, int64_t* d_binsum,
                                void* hip_stream) {
    RCP_TRY
    return rcp_plan_execute_stages(plan, d_out, d_valid, d_binsum, hip_stream, RCP_STAGE_ALL);
    RCP_CATCH
}

extern "C" int rcp_plan_status(rcp_plan* plan, void* hip_stream) {
    RCP_TRY
    if (!plan) return fail(RCP_EINVAL, "NULL plan");
    DeviceGuard g(plan->rs->device);
    HIP_TRY(g.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    uint32_t st = 0;
    HIP_TRY(hipMemcpyAsync(&st, plan->dev.status, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st & RCP_STATUS_WIDTH)
        return fail(RCP_EUNSUPPORTED, "a per-base part met a row whose slice width differs from the column count");
    if (st & RCP_STATUS_INTERP) return fail(RCP_EUNSUPPORTED, "internal plan/layout mismatch (status %u)", st);
    if (st & RCP_STATUS_OVERFLOW) return fail(RCP_EUNSUPPORTED, "bin numerator exceeded 2^32");
    return RCP_OK;
    RCP_CATCH
}

extern "C" int rcp_plan_heavy_rows(rcp_plan* plan, void* hip_stream, int32_t* n_rows) {
    RCP_TRY
    if (!plan || !n_rows) return fail(RCP_EINVAL, "NULL argument");
    DeviceGuard g(plan->rs->device);
    HIP_TRY(g.err);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, plan->dev.status + 1, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *n_rows = (int32_t)std::min<uint32_t>(n, (uint32_t)std::max(plan->dev.heavy_cap, 0));
    return RCP_OK;
    RCP_CATCH
}
