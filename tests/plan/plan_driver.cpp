// plan_driver -- the planner's shape decisions without a device (tests/test_plan_shape.py).
//
//   plan_driver CASE.txt [CASE.txt ...]
//
// Runs build_rows -> plan_parts -> plan_shape (rcp_plan.h) on each case file and prints what
// rcp_plan_info reports of the plan, then the shape fields behind it, as "key value" lines
// after a "case FILE" line.  No readset, no HIP call: the facts a plan takes from its device
// and its reads (compute units, starts-only stream) come from the file.
//
// A case file is whitespace-separated integers, after each keyword:
//   facts  n_cus ignore_strand has_st n_chrom lean_rounds2 no_lean_fold coop_min gen_rounds
//   opts   pileup_kernel heavy_threshold out_ld min_col_chunks concurrent
//   bins   n_parts stat interp rng_kind flank1 flank2
//   part   where n_bins per_base_width                      (n_parts times)
//   groups has_seg_group is_list[0..3]                      (is_list all 0: group_is_list NULL)
//   rows   n_rows n_seg
//   off    seg_off[0..n_rows]
//   seg    chrom start end strand group                     (n_seg times)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../recoup_amd/csrc/rcp_plan.h"

using namespace rcpi;

namespace {

struct Case {
    PlanFacts F;
    rcp_plan_opts opts{};
    rcp_bins_desc bins{};
    std::vector<int32_t> where, n_bins, width;
    int has_group = 0;
    uint8_t is_list[4] = {0, 0, 0, 0};
    std::vector<int64_t> seg_off;
    std::vector<int32_t> chrom, start, end;
    std::vector<int8_t> strand, group;
    rcp_rows_desc rows{};
};

bool expect(std::istream& in, const char* word) {
    std::string w;
    return (in >> w) && w == word;
}

bool read_case(const char* path, Case* c) {
    std::ifstream in(path);
    long long v[8];
    auto ints = [&](int n) {
        for (int i = 0; i < n; ++i)
            if (!(in >> v[i])) return false;
        return true;
    };
    if (!in || !expect(in, "facts") || !ints(8)) return false;
    c->F.n_cus = (int32_t)v[0];
    c->F.ignore_strand = (int32_t)v[1];
    c->F.has_st = v[2] != 0;
    c->F.n_chrom = (int32_t)v[3];
    c->F.lean_rounds2 = v[4] != 0;
    c->F.no_lean_fold = v[5] != 0;
    c->F.coop_min = (int32_t)v[6];
    c->F.gen_rounds = (int32_t)v[7];
    if (!expect(in, "opts") || !ints(5)) return false;
    c->opts.pileup_kernel = (int32_t)v[0];
    c->opts.heavy_threshold = (int32_t)v[1];
    c->opts.out_ld = v[2];
    c->opts.min_col_chunks = (int32_t)v[3];
    c->opts.concurrent = (int32_t)v[4];
    if (!expect(in, "bins") || !ints(6)) return false;
    const int n_parts = (int)v[0];
    if (n_parts < 1 || n_parts > RCP_MAX_PARTS) return false;
    c->bins.n_parts = n_parts;
    c->bins.stat = (int32_t)v[1];
    c->bins.interp = (int32_t)v[2];
    c->bins.rng_kind = (int32_t)v[3];
    c->bins.flank[0] = (int32_t)v[4];
    c->bins.flank[1] = (int32_t)v[5];
    c->bins.scale = 1.0;
    for (int p = 0; p < n_parts; ++p) {
        if (!expect(in, "part") || !ints(3)) return false;
        c->where.push_back((int32_t)v[0]);
        c->n_bins.push_back((int32_t)v[1]);
        c->width.push_back((int32_t)v[2]);
    }
    c->bins.where = c->where.data();
    c->bins.n_bins = c->n_bins.data();
    c->bins.per_base_width = c->width.data();
    if (!expect(in, "groups") || !ints(5)) return false;
    c->has_group = (int)v[0];
    bool any_list = false;
    for (int i = 0; i < 4; ++i) {
        c->is_list[i] = (uint8_t)v[1 + i];
        any_list = any_list || v[1 + i];
    }
    if (!expect(in, "rows") || !ints(2)) return false;
    const long long n_rows = v[0], n_seg = v[1];
    if (n_rows < 0 || n_seg < 0 || !expect(in, "off")) return false;
    c->seg_off.resize((size_t)n_rows + 1);
    for (auto& o : c->seg_off)
        if (!(in >> o) || o < 0 || o > n_seg) return false;
    for (long long j = 0; j < n_seg; ++j) {
        if (!expect(in, "seg") || !ints(5)) return false;
        c->chrom.push_back((int32_t)v[0]);
        c->start.push_back((int32_t)v[1]);
        c->end.push_back((int32_t)v[2]);
        c->strand.push_back((int8_t)v[3]);
        c->group.push_back((int8_t)v[4]);
    }
    c->rows.n_rows = (int32_t)n_rows;
    c->rows.seg_off = c->seg_off.data();
    c->rows.seg_chrom = c->chrom.data();
    c->rows.seg_start = c->start.data();
    c->rows.seg_end = c->end.data();
    c->rows.seg_strand = c->strand.data();
    c->rows.seg_group = c->has_group ? c->group.data() : nullptr;
    c->rows.group_is_list = any_list ? c->is_list : nullptr;
    c->rows.ignore_strand = c->F.ignore_strand;
    return true;
}

int shape(const Case& c, rcp_plan* plan) {
    Builder B;
    int rc = build_rows(c.F.n_chrom, &c.rows, &B);
    if (rc) return rc;
    const RowSummary S = summarize_rows(B);
    PlanParts Q;
    if ((rc = plan_parts(&c.bins, &B, &plan->dev, &Q)) != 0) return rc;
    return plan_shape(c.F, S, Q, &c.bins, false, &c.opts, &B, plan);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: plan_driver CASE.txt [CASE.txt ...]\n");
        return 2;
    }
    printf("bins_min_width %d\n", rcp_bins_min_width());
    for (int a = 1; a < argc; ++a) {
        Case c;
        if (!read_case(argv[a], &c)) {
            fprintf(stderr, "%s: malformed case file\n", argv[a]);
            return 2;
        }
        rcp_plan plan;
        printf("case %s\n", argv[a]);
        const int rc = shape(c, &plan);
        printf("rc %d\n", rc);
        if (rc) {
            printf("error %s\n", g_err.c_str());
            continue;
        }
        const RcpPlanDev& P = plan.dev;
        // rcp_plan_info (rcp_plan_info_get)
        printf("n_cols %lld\nn_segments %lld\nn_interp_rows %d\nlds_bytes %zu\ngrid %lld\ntile_rows %d\n",
               (long long)plan.n_cols, (long long)plan.n_seg, P.n_interp, plan.lds, (long long)plan.grid, plan.tile_rows);
        printf("chunk_positions %d\npileup_kernel %d\nread_bytes %d\nout_ld %lld\nfold %d\n", P.chunk_cap, P.lean,
               plan.use_st ? 4 : 8, (long long)plan.out_ld, P.fold);
        // the shape behind it
        for (int p = 0; p < P.n_parts; ++p)
            printf("part%d_chunk_bins %d\npart%d_n_chunks %d\n", p, P.part[p].chunk_bins, p, P.part[p].n_chunks);
        printf("n_chunks_total %d\nstage_cap %d\nrounds %d\nlean_rounds %d\nlpt %d\nlpt_cap %d\n", P.n_chunks_total,
               P.stage_cap, P.rounds, P.lean_rounds, P.lpt, P.lpt_cap);
        printf("heavy_threshold %d\nheavy_cap %d\nheavy_stride %d\ngrid_fill %d\ncoop_min %d\nmulti_rows %d\n",
               P.heavy_threshold, P.heavy_cap, P.heavy_stride, P.grid_fill, P.coop_min, P.multi_rows);
    }
    return 0;
}
