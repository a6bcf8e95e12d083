"""The planner's decisions on CPU: tests/plan/plan_driver runs build_rows -> plan_parts ->
plan_shape (recoup_amd/csrc/rcp_plan.h) on the cases of tests/plan_cases.py, with no device, and
must report what tests/golden/plan_shapes.json holds -- ``engine.Plan(...).info`` of the same
cases, recorded on the GPU (tools/record_plan_shapes.py).  tests/test_gpu_plan_shape.py holds
the library to the same fixture."""
import json
import os
import subprocess

import pytest

from tests import plan_cases

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN = os.path.join(HERE, "plan")
DRIVER = os.path.join(PLAN, "build", "plan_driver")
WHERE = {"whole": 0, "center": 1, "upstream": 2, "downstream": 3}
KERNEL = {"auto": 0, "general": 1, "lean_any": 2, "rows": 3, "lean": 4, "bins": 5}
STAT = {"mean": 0, "median": 1}
GENERAL, LEAN, LEAN_GEN, ROWS, BINS = range(5)  # rcp_plan_info.pileup_kernel

with open(os.path.join(HERE, "golden", "plan_shapes.json")) as _f:
    GOLDEN = json.load(_f)
EXPECTED = {c["id"]: c for c in GOLDEN["cases"]}
VARIANTS = plan_cases.variants()
IDS = [v[0] for v in VARIANTS]


def _case_text(case, uniform):
    """The driver's case file (tests/plan/plan_driver.cpp)."""
    t = case["rows"]()
    n_seg = len(t["start"])
    grp = t["seg_group"] if t["seg_group"] is not None else [0] * n_seg
    lst = t["group_is_list"] if t["group_is_list"] is not None else [0, 0, 0, 0]
    lines = ["facts %d %d %d 1 0 0 -1 0" % (GOLDEN["n_cus"], case["ignore_strand"], uniform),
             "opts %d %d 0 %d %d" % (KERNEL[case["kernel"]], case["heavy_threshold"], case["min_col_chunks"],
                                     case["concurrent"]),
             "bins %d %d 0 0 %d %d" % (len(case["parts"]), STAT[case["stat"]], case["flank"][0], case["flank"][1])]
    for p in case["parts"]:
        lines.append("part %d %d %d" % (WHERE[p[0]], p[1], p[2] if len(p) > 2 else 0))
    lines.append("groups %d %s" % (t["seg_group"] is not None, " ".join(str(int(x)) for x in lst)))
    lines.append("rows %d %d" % (len(t["seg_off"]) - 1, n_seg))
    lines.append("off " + " ".join(str(int(x)) for x in t["seg_off"]))
    for j in range(n_seg):
        lines.append("seg %d %d %d %d %d" % (t["chrom"][j], t["start"][j], t["end"][j], t["strand"][j], grp[j]))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def shapes(tmp_path_factory):
    """{variant id: {field: int}} and the driver's bins_min_width, from one run of the driver."""
    from recoup_amd import build
    build.build(verbose=False)
    subprocess.check_call(["make", "-s", "-C", PLAN], stdout=subprocess.DEVNULL)
    tmp = tmp_path_factory.mktemp("plan_cases")
    paths = []
    for vid, case, uniform in VARIANTS:
        p = tmp / (vid + ".txt")
        p.write_text(_case_text(case, uniform))
        paths.append(str(p))
    r = subprocess.run([DRIVER, *paths], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out, cur, head = {}, None, {}
    for line in r.stdout.splitlines():
        k, v = line.split(" ", 1)
        if k == "case":
            cur = out.setdefault(os.path.basename(v)[:-len(".txt")], {})
        elif k == "error":
            cur[k] = v
        else:
            (head if cur is None else cur)[k] = int(v)
    return out, head


def test_fixture_holds_every_case():
    assert sorted(EXPECTED) == sorted(IDS)
    assert all(EXPECTED[vid]["uniform"] == uniform for vid, _, uniform in VARIANTS)


def test_narrow_case_is_one_below_the_bin_difference_width(shapes):
    assert shapes[1]["bins_min_width"] == plan_cases.BINS_MIN_WIDTH


@pytest.mark.parametrize("vid", IDS)
def test_driver_reports_the_recorded_plan(shapes, vid):
    got = shapes[0][vid]
    assert got.get("rc") == 0, got
    want = EXPECTED[vid]["info"]
    assert {k: got[k] for k in want} == want


@pytest.mark.parametrize("vid,case,uniform", VARIANTS, ids=IDS)
def test_shape_fields_agree_with_the_reported_ones(shapes, vid, case, uniform):
    """What rcp_plan_info does not expose, held to what it does: the recorded grid, tile_rows,
    fold and pileup_kernel follow from these fields by the launchers' own arithmetic."""
    s = shapes[0][vid]
    n_rows = len(case["rows"]()["seg_off"]) - 1
    n_parts = len(case["parts"])
    kernel = s["pileup_kernel"]
    chunks = [s["part%d_n_chunks" % p] for p in range(n_parts)]
    cbins = [s["part%d_chunk_bins" % p] for p in range(n_parts)]
    for (part, nch, cb) in zip(case["parts"], chunks, cbins):
        n = part[2] if part[1] == 0 else part[1]
        assert nch == -(-n // cb)
    assert s["n_chunks_total"] == sum(chunks)
    assert s["stage_cap"] == max(cbins)
    grid = -(-n_rows // s["tile_rows"]) * s["n_chunks_total"]
    assert s["grid"] == (-(-grid // 8) * 8 if kernel == BINS else grid)
    if kernel == GENERAL:
        assert s["rounds"] in (1, 2) and s["tile_rows"] == 16 * s["rounds"]
    elif kernel == BINS:
        assert s["tile_rows"] == 16 and chunks == [1]
    else:
        assert s["tile_rows"] == (32 if s["lean_rounds"] == 2 else 64)
    per_base = all(p[1] == 0 for p in case["parts"])
    assert s["lean_rounds"] == (2 if kernel in (LEAN, LEAN_GEN) and per_base else 0)
    assert s["grid_fill"] == (7 if case["concurrent"] > 1 else 8)
    want_heavy = 4096 if case["heavy_threshold"] < 0 else case["heavy_threshold"]
    assert s["heavy_threshold"] == (0 if s["fold"] or n_rows == 0 else want_heavy)
    assert s["lpt_cap"] == (-(-n_rows // 32) * s["n_chunks_total"] if s["lpt"] else 0)
    assert not s["lpt"] or (kernel == LEAN and per_base and not s["fold"])
    assert s["read_bytes"] == (4 if uniform and not (kernel == LEAN and not per_base) else 8)
    assert s["multi_rows"] == (case["name"].startswith("list_rows"))


def test_column_chunks(shapes):
    s = shapes[0]
    assert s["bins2000-uniform"]["part0_n_chunks"] == 4          # 512 bins a stage chunk at most
    assert s["bins200_wide_general-uniform"]["part0_n_chunks"] == 1  # 10 chunks would exceed the general cap
    assert s["bins200_w25_general-uniform"]["part0_n_chunks"] == 5   # <= 1023 positions a chunk
    assert s["bins1000_lean_min4-uniform"]["part0_n_chunks"] == 4
    assert s["rrng_lean_any_min4-uniform"]["part0_chunk_bins"] == 250
    # the center part's 200 bins of 20 bp: 51 bins (<= 1023 positions) a chunk
    assert [s["three_parts-uniform"]["part%d_n_chunks" % p] for p in range(3)] == [1, 4, 1]
    # a per-base lean plan of few rows is cut into 16 column chunks and claimed heaviest first
    # unless it folds
    assert s["base4000-uniform"]["n_chunks_total"] == 16
    assert s["base4000-uniform"]["lpt"] == 0 and s["base4000_heavy1000-uniform"]["lpt"] == 1
