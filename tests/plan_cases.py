"""The planner's shape cases: row tables, bins and plan options whose plans are pinned in
tests/golden/plan_shapes.json (recorded by tools/record_plan_shapes.py through
``engine.Plan(...).info``).  tests/test_plan_shape.py gives the same cases to the stand-alone
planner (tests/plan/plan_driver.cpp, no device), tests/test_gpu_plan_shape.py to the library.

Every case is one chromosome of 4,000,000 bp, '+' rows, ignore_strand = 1 and default options
unless it says otherwise, planned over a few hundred reads of one width (``uniform``: the
layout then has the starts-only stream) and of mixed widths.
"""
import numpy as np

CHROM_LEN = 4_000_000
N_READS = 400
BINS_MIN_WIDTH = 4  # rcp_bins_min_width(): the bin-difference kernel's narrowest bin


def _rows(n, width, short=None, null_row=False, long_row=None):
    """n single-range rows of ``width`` bp.  short: row n/2 has that many bp instead (fewer than
    its bins: interpolated); long_row: row 0 has that many; null_row: row 5 is the zero-width
    range start = 5, end = -3, statically NULL through its negative coordinate, whose one
    segment (positions 1..5, query_ok = 0) stays in the table."""
    start = 1001 + (np.arange(n, dtype=np.int64) * 101) % 3_900_000
    w = np.full(n, width, dtype=np.int64)
    if short:
        w[n // 2] = short
    if long_row:
        w[0] = long_row
    end = start + w - 1
    if null_row:
        start[5], end[5] = 5, -3
    return {"seg_off": np.arange(n + 1), "chrom": np.zeros(n, np.int32), "start": start, "end": end,
            "strand": np.zeros(n, np.int8), "seg_group": None, "group_is_list": None}


def _list_rows(n, k=3, width=500, gap=200):
    """n rows, each one range list (GRangesList element) of k ranges of ``width`` bp."""
    first = 1001 + (np.arange(n, dtype=np.int64) * 10007) % 3_900_000
    start = (first[:, None] + np.arange(k) * (width + gap)).ravel()
    return {"seg_off": np.arange(n + 1) * k, "chrom": np.zeros(n * k, np.int32), "start": start,
            "end": start + width - 1, "strand": np.zeros(n * k, np.int8), "seg_group": np.zeros(n * k, np.int8),
            "group_is_list": np.array([1, 0, 0, 0], np.uint8)}


def _case(name, rows, parts, **kw):
    c = {"name": name, "rows": rows, "parts": parts, "flank": (0, 0), "stat": "mean", "ignore_strand": True,
         "kernel": "auto", "heavy_threshold": -1, "min_col_chunks": 0, "concurrent": 0}
    c.update(kw)
    return c


def cases():
    """[case]: name, rows (lambda -> table), parts, flank, stat, ignore_strand and the plan options."""
    W = [("whole", 1000)]
    r2000 = lambda: _rows(64, 2000)
    r4000 = lambda: _rows(64, 4000)
    base = [("whole", 0, 4000)]
    out = [
        _case("bins1000_lean", r2000, W, kernel="lean"),
        _case("bins1000_auto", r2000, W),  # a small table: the general kernel with fold
        _case("bins1000_general", r2000, W, kernel="general"),
        # kLeanMinRowsBinned
        _case("bins1000_auto_35999", lambda: _rows(35999, 2000), W),
        _case("bins1000_auto_36000", lambda: _rows(36000, 2000), W),
        _case("base4000", r4000, base),
        # kFoldConcurrentMaxRows
        _case("base4000_conc2_8192", lambda: _rows(8192, 4000), base, concurrent=2),
        _case("base4000_conc2_8193", lambda: _rows(8193, 4000), base, concurrent=2),
        _case("base4000_heavy1000", r4000, base, heavy_threshold=1000),
        _case("bins200", r4000, [("whole", 200)]),  # the bin-difference kernel
        _case("bins200_narrow", lambda: _rows(64, 200 * (BINS_MIN_WIDTH - 1)), [("whole", 200)]),
        _case("bins200_short_row", lambda: _rows(64, 4000, short=150), [("whole", 200)]),
        _case("list_rows", _list_rows_64, [("whole", 100)]),  # the row-wave kernel, fold 1
        _case("list_rows_heavy1000", _list_rows_64, [("whole", 100)], heavy_threshold=1000),
        _case("list_rows_general", _list_rows_64, [("whole", 100)], kernel="general"),
        _case("rrng_auto", lambda: _rows(64, 2050), W),  # R-RNG layout, dif = 50
        _case("rrng_lean_any", lambda: _rows(64, 2050), W, kernel="lean_any"),
        # ... in chunks of 250 bins, within rcp_lean_gen_max_bins(): the lean kernel's general-bins mode
        _case("rrng_lean_any_min4", lambda: _rows(64, 2050), W, kernel="lean_any", min_col_chunks=4),
        # 200 bins of 50 bp: the bin-difference kernel (no column chunks); on the general kernel
        # one chunk in wave sub-chunks (its 10 column chunks would exceed kGeneralMaxChunks), and
        # with bins of 25 bp 5 column chunks
        _case("bins200_wide", lambda: _rows(64, 10000), [("whole", 200)]),
        _case("bins200_wide_general", lambda: _rows(64, 10000), [("whole", 200)], kernel="general"),
        _case("bins200_w25_general", lambda: _rows(64, 5000), [("whole", 200)], kernel="general"),
        _case("bins2000", r4000, [("whole", 2000)]),  # more than one stage chunk
        _case("median_bins200", r4000, [("whole", 200)], stat="median"),
        # a median bin of 3000 positions: wider than a wave chunk (interpolation mode 4)
        _case("median_long_row", lambda: _rows(64, 4000, long_row=600000), [("whole", 200)], stat="median"),
        _case("three_parts", lambda: _rows(64, 5000), [("upstream", 50), ("center", 200), ("downstream", 50)],
              flank=(500, 500)),
        _case("bins1000_lean_min4", r2000, W, kernel="lean", min_col_chunks=4),
        _case("bins1000_lean_stranded", r2000, W, kernel="lean", ignore_strand=False),
        _case("base4000_stranded", r4000, base, ignore_strand=False),
        # the lean kernel's single-range test looks at NULL rows, the others' skip them
        _case("null_row_lean", lambda: _rows(64, 2000, null_row=True), W, kernel="lean"),
        _case("null_row_auto", lambda: _rows(64, 2000, null_row=True), W),
        _case("null_row_bins200", lambda: _rows(64, 4000, null_row=True), [("whole", 200)]),
        _case("no_rows", lambda: _rows(0, 2000), W),
    ]
    return out


def _list_rows_64():
    return _list_rows(64)


def variants():
    """[(id, case, uniform)]: every case with reads of one width and of mixed widths."""
    out = []
    for c in cases():
        for uniform in (True, False):
            out.append(("%s-%s" % (c["name"], "uniform" if uniform else "mixed"), c, uniform))
    return out


def reads(uniform):
    """(chrom, start, end, strand) of N_READS reads on the one chromosome."""
    rng = np.random.default_rng(7)
    start = np.sort(rng.integers(1, CHROM_LEN - 200, N_READS)).astype(np.int32)
    width = np.full(N_READS, 50) if uniform else rng.integers(30, 81, N_READS)
    return (np.zeros(N_READS, np.int32), start, (start + width - 1).astype(np.int32),
            (np.arange(N_READS) % 2).astype(np.int8))


def build_plan(case, uniform, device=0):
    """The case's plan on the device: (ReadSet, Plan)."""
    from recoup_amd.engine import Bins, Plan, ReadSet, RowTable
    t = case["rows"]()
    rs = ReadSet(*reads(uniform), np.array([CHROM_LEN], np.int64), device=device)
    rows = RowTable(t["seg_off"], t["chrom"], t["start"], t["end"], t["strand"], seg_group=t["seg_group"],
                    group_is_list=t["group_is_list"], ignore_strand=case["ignore_strand"])
    bins = Bins(case["parts"], flank=case["flank"], stat=case["stat"])
    return rs, Plan(rs, rows, bins, kernel=case["kernel"], heavy_threshold=case["heavy_threshold"],
                    min_col_chunks=case["min_col_chunks"], concurrent=case["concurrent"])
