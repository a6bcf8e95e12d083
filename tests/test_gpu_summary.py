"""Device summaries of kept profile matrices on the GPU: rcp_summary_cols / rcp_summary_rows /
rcp_order_rows and the calcPlotProfiles / orderProfiles family over them.

Every expected value is NumPy on the host with np.longdouble accumulation of the same input (what
R's long-double mean / var do), never the library.  Matrices are built directly as device tensors
with every padding element (rows n_rows .. ld-1 of a column) NaN, so a kernel that reads padding
poisons its result.

Tolerance of a mean or sd over n values: 8 * B with B = (log2(n) + 8) * 2^-53 * max|x| -- the
roundoff bound of a tree sum of n terms plus a few ulp for log2 and the division, times 8 of
margin.  Orders use dyadic values (integers below 4096 over 8), whose sums are exact in fp64 in
any order: the expected order is exactly the stable argsort and keys are compared bit for bit."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import recoup_amd as ra
from recoup_amd import _lib
from tests.golden import c1_cases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLAB = 4096      # kSumColSlabRows (recoup_amd/csrc/rcp_summary.h): rows of a column one workgroup reduces
ROW_TILE = 64    # kSumRowTile: rows of one workgroup of the row kernel (63 / 65 straddle it)
CAP = 64         # RCP_SUMMARY_MAX_GROUPS
N_ROWS = [1, 63, 65, SLAB + 1]
N_COLS = [1, 3, 257]
EPS = 2.0 ** -53
LD = np.longdouble


def test_restated_constants_match_the_source(gpu):
    txt = open(os.path.join(ROOT, "recoup_amd", "csrc", "rcp_summary.h")).read()
    assert int(re.search(r"kSumColSlabRows = (\d+)", txt).group(1)) == SLAB
    assert int(re.search(r"kSumRowTile = (\d+)", txt).group(1)) == ROW_TILE
    hdr = open(os.path.join(ROOT, "include", "recoup_amd.h")).read()
    assert int(re.search(r"RCP_SUMMARY_MAX_GROUPS (\d+)", hdr).group(1)) == CAP


# ------------------------------------------------------------------------------ plumbing
def padded(n):
    return (n + 15) // 16 * 16 + 16


def device_matrix(x, ld):
    """x [n_rows, n_cols] -> device tensor (n_cols, ld), column-major with NaN padding."""
    t = torch.full((x.shape[1], ld), float("nan"), dtype=torch.float64, device="cuda")
    t[:, :x.shape[0]] = torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
    return t


def _desc(ts, n_rows, n_cols, ld, log, col0=0):
    arr = (ctypes.c_void_p * len(ts))(*[t.data_ptr() + 8 * col0 * ld for t in ts])
    d = _lib.MatrixDesc(n_rows, n_cols, ld, len(ts), int(log), arr)
    d._keep = arr
    return d


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gid(gid):
    return None if gid is None else torch.from_numpy(np.asarray(gid, np.int32)).cuda()


def cols(ts, n_rows, n_cols, ld, log=False, gid=None, G=1, col0=0):
    S = len(ts)
    n = max(S * G * n_cols, 1)
    mean = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    sd = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    d = _desc(ts, n_rows, n_cols, ld, log, col0)
    g = _gid(gid)
    _lib.check(_lib.lib().rcp_summary_cols(ctypes.byref(d), _lib.ptr(g), G, _lib.ptr(mean), _lib.ptr(sd),
                                           _lib.ptr(cnt), _stream()))
    return [a.cpu().numpy()[:S * G * n_cols].reshape(S, G, n_cols) for a in (mean, sd, cnt)]


def rows(ts, n_rows, n_cols, ld, log=False, col0=0):
    S = len(ts)
    out = [torch.full((max(S * n_rows, 1),), 7.0, dtype=torch.float64, device="cuda") for _ in range(4)]
    d = _desc(ts, n_rows, n_cols, ld, log, col0)
    _lib.check(_lib.lib().rcp_summary_rows(ctypes.byref(d), *[_lib.ptr(a) for a in out], _stream()))
    return [a.cpu().numpy()[:S * n_rows].reshape(S, n_rows) for a in out]


WHAT = {"sum": 0, "max": 1, "avg": 2}


def order(ts, n_rows, n_cols, ld, what, ref, dec, gid=None, G=0, col0=0):
    o = torch.full((max(n_rows, 1),), -7, dtype=torch.int32, device="cuda")
    k = torch.full((max(n_rows, 1),), 7.0, dtype=torch.float64, device="cuda")
    d = _desc(ts, n_rows, n_cols, ld, False, col0)
    g = _gid(gid)
    _lib.check(_lib.lib().rcp_order_rows(ctypes.byref(d), WHAT[what], ref, int(dec), _lib.ptr(g), G, _lib.ptr(o),
                                         _lib.ptr(k), _stream()))
    return o.cpu().numpy()[:n_rows], k.cpu().numpy()[:n_rows]


# ------------------------------------------------------------------------------ references
def transform(x, log):
    xl = x.astype(LD)
    return np.log2(xl + 1) if log else xl


def bound(n, xmax):
    return 8 * (np.log2(max(n, 1)) + 8) * EPS * np.asarray(xmax, LD)


def mean_sd(v, axis):
    """long-double mean and sd (n - 1) of v along axis; sd NaN for n < 2."""
    n = v.shape[axis]
    m = v.sum(axis=axis) / n
    if n < 2:
        return m, np.full(m.shape, np.nan, LD)
    dev = v - np.expand_dims(m, axis)
    return m, np.sqrt((dev * dev).sum(axis=axis) / (n - 1))


def check_cols(tag, x, got, log, gid=None, G=1):
    """got = (mean, sd, count) [G, n_cols] of one sample against the reference of x [n_rows, n_cols]."""
    mean, sd, cnt = got
    xl = transform(x, log)
    worst = 0.0
    for g in range(G):
        sel = np.ones(x.shape[0], bool) if gid is None else np.asarray(gid) == g
        n = int(sel.sum())
        assert (cnt[g] == n).all(), (tag, g, cnt[g], n)
        if n == 0:
            assert np.isnan(mean[g]).all() and np.isnan(sd[g]).all(), (tag, g)
            continue
        v = xl[sel]
        m, s = mean_sd(v, 0)
        B = bound(n, np.abs(v).max(axis=0))
        em = np.abs(mean[g].astype(LD) - m)
        worst = max(worst, float((em / B).max()))
        assert (em <= B).all(), (tag, "mean", g, float((em / B).max()))
        if n == 1:
            assert np.isnan(sd[g]).all(), (tag, g)
        else:
            es = np.abs(sd[g].astype(LD) - s)
            worst = max(worst, float((es / B).max()))
            assert (es <= B).all(), (tag, "sd", g, float((es / B).max()))
    print(f"{tag}: worst error / allowance {worst:.3g}")


def check_rows(tag, x, got, log):
    """got = (sum, max, mean, sd) [n_rows] of one sample; x [n_rows, n_cols]."""
    gs, gm, gmean, gsd = got
    xl = transform(x, log)
    n = x.shape[1]
    m, s = mean_sd(xl, 1)
    B = bound(n, np.abs(xl).max(axis=1))
    assert (np.abs(gs.astype(LD) - xl.sum(axis=1)) <= n * B).all(), (tag, "sum")
    if log:
        assert (np.abs(gm.astype(LD) - xl.max(axis=1)) <= B).all(), (tag, "max")
    else:
        assert np.array_equal(gm, x.max(axis=1)), (tag, "max")
    em = np.abs(gmean.astype(LD) - m)
    assert (em <= B).all(), (tag, "mean", float((em / B).max()))
    if n == 1:
        assert np.isnan(gsd).all(), (tag, "sd")
    else:
        es = np.abs(gsd.astype(LD) - s)
        assert (es <= B).all(), (tag, "sd", float((es / B).max()))


def lds(n_rows, pad):
    return padded(n_rows) if pad else n_rows


# ------------------------------------------------------------------------------ column statistics
@pytest.mark.parametrize("pad", [False, True], ids=["ld=n_rows", "ld=padded"])
@pytest.mark.parametrize("n_rows", N_ROWS)
def test_column_mean_sd(gpu, n_rows, pad):
    rng = np.random.default_rng(100 + n_rows + pad)
    ld = lds(n_rows, pad)
    for n_cols in N_COLS:
        x = rng.gamma(2.0, 50.0, (3, n_rows, n_cols))
        ts = [device_matrix(x[s], ld) for s in range(3)]
        for S in (1, 3):
            for log in (False, True):
                mean, sd, cnt = cols(ts[:S], n_rows, n_cols, ld, log)
                for s in range(S):
                    check_cols(f"cols {n_rows}x{n_cols} ld {ld} S{S} log{int(log)} s{s}", x[s],
                               (mean[s], sd[s], cnt[s]), log)


def _groups(rng, n_rows, G):
    """ids in [0, G): group 1 with exactly one row, group G - 1 empty (G >= 3), a fifth of the rows
    left out (-1), one id beyond the groups (left out as well)."""
    gid = rng.integers(0, G, n_rows).astype(np.int32)
    if G >= 3:
        gid[gid == G - 1] = 0
        gid[gid == 1] = 0
    if n_rows >= 16:
        gid[rng.choice(n_rows, n_rows // 5, replace=False)] = -1
        gid[3] = G + 5
    if G >= 3 and n_rows > 7:
        gid[7] = 1
    return gid


@pytest.mark.parametrize("G", [1, 3, CAP])
def test_column_stats_by_group(gpu, G):
    rng = np.random.default_rng(7 + G)
    for n_rows, n_cols in ((65, 3), (SLAB + 1, 3), (2 * SLAB + 5, 1)):
        ld = padded(n_rows)
        gid = _groups(rng, n_rows, G)
        x = rng.gamma(2.0, 50.0, (3, n_rows, n_cols))
        ts = [device_matrix(x[s], ld) for s in range(3)]
        for S, log in ((1, False), (3, True)):
            mean, sd, cnt = cols(ts[:S], n_rows, n_cols, ld, log, gid, G)
            ref_gid = np.where((gid >= 0) & (gid < G), gid, -1)
            for s in range(S):
                check_cols(f"groups G{G} {n_rows}x{n_cols} S{S} s{s}", x[s], (mean[s], sd[s], cnt[s]), log,
                           ref_gid, G)


@pytest.mark.parametrize("pad", [False, True], ids=["ld=n_rows", "ld=padded"])
def test_cancellation(gpu, pad):
    """A column of 1e6 + k/8, k = 0..7: sd about 0.29 beside values of 1e6.  sum(x^2) - n * mean^2
    misses the allowance (about 1.8e-8) by three orders of magnitude; deviations about the mean do
    not.  The same values along a row for the row kernel."""
    n = SLAB + 1
    ld = lds(n, pad)
    col = 1e6 + (np.arange(n) % 8) / 8.0
    x = np.stack([col, col[::-1]], axis=1)
    mean, sd, cnt = cols([device_matrix(x, ld)], n, 2, ld)
    check_cols(f"cancellation ld {ld}", x, (mean[0], sd[0], cnt[0]), False)
    gid = (np.arange(n) % 3).astype(np.int32)
    mean, sd, cnt = cols([device_matrix(x, ld)], n, 2, ld, False, gid, 3)
    check_cols(f"cancellation groups ld {ld}", x, (mean[0], sd[0], cnt[0]), False, gid, 3)
    xr = np.ascontiguousarray(x[:257].T)  # 2 rows x 257 columns
    got = rows([device_matrix(xr, lds(2, pad))], 2, 257, lds(2, pad))
    check_rows("cancellation rows", xr, [a[0] for a in got], False)


def test_middle_column_range(gpu):
    """Columns 2..4 of a 7-column matrix, selected by offsetting the pointer; with ld = n_rows odd
    every other column starts off a 16-byte boundary."""
    rng = np.random.default_rng(5)
    for n_rows, ld in ((65, 65), (65, padded(65)), (SLAB + 1, SLAB + 1)):
        x = rng.gamma(2.0, 50.0, (n_rows, 7))
        t = device_matrix(x, ld)
        mean, sd, cnt = cols([t], n_rows, 3, ld, col0=2)
        check_cols(f"range ld {ld}", x[:, 2:5], (mean[0], sd[0], cnt[0]), False)
        check_rows(f"range rows ld {ld}", x[:, 2:5], [a[0] for a in rows([t], n_rows, 3, ld, col0=2)], False)
        xd = np.floor(x) / 8.0
        o, k = order([device_matrix(xd, ld)], n_rows, 3, ld, "sum", 0, False, col0=2)
        key = xd[:, 2:5].sum(axis=1)
        assert np.array_equal(k.view(np.uint64), key.view(np.uint64))
        assert np.array_equal(o, np.argsort(key, kind="stable"))


def test_empty_shapes(gpu):
    t = torch.full((4, 32), float("nan"), dtype=torch.float64, device="cuda")
    mean, sd, cnt = cols([t], 0, 4, 32)        # no rows: every column is numeric(0)
    assert np.isnan(mean).all() and np.isnan(sd).all() and (cnt == 0).all()
    mean, sd, cnt = cols([t], 20, 0, 32)
    assert mean.size == 0
    s, m, a, d = rows([t], 20, 0, 32)          # no columns: sum(numeric(0)) = 0, max = -Inf
    assert (s == 0).all() and np.isneginf(m).all() and np.isnan(a).all() and np.isnan(d).all()
    assert rows([t], 0, 4, 32)[0].size == 0
    o, k = order([t], 0, 4, 32, "sum", -1, True)
    assert o.size == 0


# ------------------------------------------------------------------------------ row statistics
@pytest.mark.parametrize("pad", [False, True], ids=["ld=n_rows", "ld=padded"])
@pytest.mark.parametrize("n_rows", N_ROWS)
def test_row_stats(gpu, n_rows, pad):
    rng = np.random.default_rng(200 + n_rows + pad)
    ld = lds(n_rows, pad)
    for n_cols in N_COLS:
        x = rng.gamma(2.0, 50.0, (3, n_rows, n_cols))
        ts = [device_matrix(x[s], ld) for s in range(3)]
        for S, log in ((1, False), (3, True), (3, False)):
            got = rows(ts[:S], n_rows, n_cols, ld, log)
            for s in range(S):
                check_rows(f"rows {n_rows}x{n_cols} ld {ld} S{S} log{int(log)} s{s}", x[s], [a[s] for a in got], log)


# ------------------------------------------------------------------------------ order
def expected_key(x, what, ref):
    """x [S, n_rows, n_cols] dyadic: every sum below is exact; the means round once."""
    n_cols = x.shape[2]
    st = {"sum": x.sum(axis=2), "max": x.max(axis=2), "avg": x.sum(axis=2) / n_cols}[what]
    if ref >= 0:
        return st[ref]
    acc = st[0]
    for s in range(1, len(st)):  # samples in list order
        acc = np.maximum(acc, st[s]) if what == "max" else acc + st[s]
    return acc / len(st) if what == "avg" and len(st) > 1 else acc


def expected_order(key, dec, gid=None, G=0):
    ix = np.argsort(-key if dec else key, kind="stable")
    if gid is None:
        return ix
    gp = np.where((gid >= 0) & (gid < G), gid, G)
    held = ix[gp[ix] < G]
    held = held[np.argsort(gp[held], kind="stable")]
    return np.concatenate([held, np.flatnonzero(gp == G)])


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_row_order(gpu, n_rows):
    rng = np.random.default_rng(300 + n_rows)
    for n_cols, pad in zip(N_COLS, (True, False, True)):
        ld = lds(n_rows, pad)
        # rows drawn from a pool half as long, the same draw in every sample: duplicated rows tie
        pick = rng.integers(0, max(n_rows // 2, 1), n_rows)
        x = np.stack([(rng.integers(0, 4096, (max(n_rows // 2, 1), n_cols)) / 8.0)[pick] for _ in range(3)])
        ts = [device_matrix(x[s], ld) for s in range(3)]
        gid = _groups(rng, n_rows, 3)
        for what in ("sum", "max", "avg"):
            for ref in (-1, 0, 2):
                key = expected_key(x, what, ref)
                for dec in (False, True):
                    for g, G in ((None, 0), (gid, 3)):
                        o, k = order(ts, n_rows, n_cols, ld, what, ref, dec, g, G)
                        tag = (n_rows, n_cols, what, ref, dec, g is not None)
                        assert np.array_equal(k.view(np.uint64), key.view(np.uint64)), tag
                        assert np.array_equal(o, expected_order(key, dec, g, G)), tag


def test_order_signed_zero_ties(gpu):
    """-0.0 and 0.0 are one key to R: they tie, and ties keep row order in both directions."""
    x = np.array([0.0, -0.0, 1.0, -0.0, 0.0, -1.0, -0.0])[:, None]
    t = device_matrix(x, padded(7))
    o, k = order([t], 7, 1, padded(7), "max", 0, False)
    assert np.array_equal(k.view(np.uint64), x[:, 0].view(np.uint64))  # the key itself keeps its sign
    assert o.tolist() == [5, 0, 1, 3, 4, 6, 2]
    o, _ = order([t], 7, 1, padded(7), "max", 0, True)
    assert o.tolist() == [2, 0, 1, 3, 4, 6, 5]


# ------------------------------------------------------------------------------ reproducibility
def test_bit_identical_across_calls_and_streams(gpu):
    rng = np.random.default_rng(11)
    n_rows, n_cols = 2 * SLAB + 77, 257
    ld = padded(n_rows)
    x = rng.gamma(2.0, 50.0, (n_rows, n_cols))
    t = device_matrix(x, ld)
    gid = _groups(rng, n_rows, 3)

    def run():
        out = list(cols([t], n_rows, n_cols, ld, True, gid, 3)) + list(cols([t], n_rows, n_cols, ld))
        out += rows([t], n_rows, n_cols, ld, True)
        out += order([t], n_rows, n_cols, ld, "avg", 0, True, gid, 3)
        return [np.ascontiguousarray(a).view(np.uint8) for a in out]

    first = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        second = run()
    torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------ end to end
FLANK = (2000, 2000)


@pytest.fixture(scope="module")
def kept(gpu):
    """test.input (two samples) -> coverageRef -> profileMatrix(keep_on_device=True): TSS windows
    of 4000 bp in 125 bins of 32 bp, so every bin mean is an integer over 32."""
    d = c1_cases.load_inputs()
    G = c1_cases.genome(d)
    genome = ra.GRanges(G["chrom"], G["start"], G["end"], G["strand"], names=G["names"])
    inp = []
    for s in c1_cases.samples(d):
        sl = {lv: int(v) for lv, v in zip(s["seqlevels"], s["seqlengths"]) if v >= 0}
        reads = ra.GRanges(np.full(len(s["start"]), "chr12"), s["start"], s["end"], s["strand"],
                           seqlevels=s["seqlevels"], seqlengths=sl)
        inp.append({"id": s["id"], "name": s["name"], "ranges": reads})
    inp = ra.coverageRef(inp, genome, "tss", FLANK)
    inp = ra.profileMatrix(inp, FLANK, {"flankBinSize": 0, "regionBinSize": 125, "sumStat": "mean"},
                           keep_on_device=True)
    for s in inp:
        p = np.asarray(s["profile"])
        assert p.shape == (100, 125) and np.array_equal(p * 32, np.round(p * 32))
    return inp, genome


@pytest.mark.parametrize("scale", ["natural", "log2"])
def test_calc_plot_profiles_end_to_end(kept, scale):
    inp, _ = kept
    opts = {"plotParams": {"sumStat": "mean", "signalScale": scale, "smooth": False}}
    for sdim in (2, 1):
        got = ra.calcPlotProfiles(inp, opts, sdim=sdim)
        for s, g in zip(inp, got):
            xl = transform(np.asarray(s["profile"]), scale == "log2")
            axis = 0 if sdim == 2 else 1
            m, sd = mean_sd(xl, axis)
            B = bound(xl.shape[axis], np.abs(xl).max(axis=axis))
            assert g["profile"].shape == m.shape
            assert (np.abs(g["profile"].astype(LD) - m) <= B).all()
            assert (np.abs((g["upper"] - g["profile"]).astype(LD) - sd) <= 2 * B).all()
            assert (np.abs((g["profile"] - g["lower"]).astype(LD) - sd) <= 2 * B).all()


def test_design_plot_profiles_end_to_end(kept):
    inp, _ = kept
    design = np.array(["b", "a", "c", "a"] * 25)
    opts = {"plotParams": {"sumStat": "mean", "signalScale": "natural"}}
    got = ra.calcDesignPlotProfiles(inp, design, opts)
    for s, g in zip(inp, got):
        assert list(g) == ["a", "b", "c"]
        for lv in g:
            v = np.asarray(s["profile"])[design == lv].astype(LD)
            m, sd = mean_sd(v, 0)
            B = bound(v.shape[0], np.abs(v).max(axis=0))
            assert (np.abs(g[lv]["profile"].astype(LD) - m) <= B).all()
            assert (np.abs((g[lv]["upper"] - g[lv]["profile"]).astype(LD) - sd) <= 2 * B).all()


@pytest.mark.parametrize("what", ["suma", "sum2", "max1", "maxa", "avga", "avg2"])
@pytest.mark.parametrize("direction", ["descending", "ascending"])
def test_order_profiles_end_to_end(kept, what, direction):
    inp, _ = kept
    x = np.stack([np.asarray(s["profile"]) for s in inp])
    key = expected_key(x, what[:3], -1 if what[-1] == "a" else int(what[-1]) - 1)
    opts = {"orderBy": {"what": what, "order": direction, "custom": None}}
    got = ra.orderProfiles(inp, opts)
    want = expected_order(key, direction == "descending")
    assert np.array_equal(got["ix"], want)
    assert np.array_equal(got["x"].view(np.uint64), key[want].view(np.uint64))
    design = np.array([1, 0, 0, None] * 25, object)
    gid = np.array([1, 0, 0, -1] * 25, np.int32)
    got = ra.orderProfilesByDesign(inp, design, opts)
    assert np.array_equal(got["ix"], expected_order(key, direction == "descending", gid, 2)[:75])
    assert ra.orderProfiles(inp, {"orderBy": {"what": "none", "order": direction}})["ix"].tolist() == list(range(100))


def test_profile_columns_only(kept):
    """A recoupProfiles matrix keeps the heatmap's 200 columns after the profile's 4000: the curve
    covers the profile's own columns only."""
    _, genome = kept
    inp = []
    d = c1_cases.load_inputs()
    for s in list(c1_cases.samples(d))[:1]:
        sl = {lv: int(v) for lv, v in zip(s["seqlevels"], s["seqlengths"]) if v >= 0}
        reads = ra.GRanges(np.full(len(s["start"]), "chr12"), s["start"], s["end"], s["strand"],
                           seqlevels=s["seqlevels"], seqlengths=sl)
        inp.append({"id": s["id"], "name": s["name"], "ranges": reads})
    inp = ra.coverageRef(inp, genome, "tss", FLANK)
    inp = ra.recoupProfiles(inp, genome, "tss", FLANK, {"flankBinSize": 0, "regionBinSize": 0}, keep_on_device=True)
    s = inp[0]
    assert s["profile_device"].shape[0] == 4200 and s["profile"].shape == (100, 4000)
    g = ra.calcPlotProfiles(inp, {"plotParams": {"sumStat": "mean", "signalScale": "natural"}})[0]
    xl = np.asarray(s["profile"]).astype(LD)
    m, sd = mean_sd(xl, 0)
    B = bound(100, np.abs(xl).max(axis=0))
    assert g["profile"].shape == (4000,)
    assert (np.abs(g["profile"].astype(LD) - m) <= B).all()
    key = np.asarray(s["profile"]).sum(axis=1)  # integer depths: exact
    got = ra.orderProfiles(inp, {"orderBy": {"what": "sum1", "order": "descending"}})
    assert np.array_equal(got["ix"], expected_order(key, True))
