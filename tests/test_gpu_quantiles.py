"""Exact quantiles of kept profile matrices on the GPU: rcp_summary_quantiles /
rcp_summary_median_mad and profileQuantiles / heatmapColorLimits / calcMedianPlotProfiles over them.

Every expected value is a NumPy restatement of the semantics in include/recoup_amd.h (R's type-7
quantile, median and mad) over np.sort of the same data, the formula written out in float64
scalars -- never np.quantile / np.median (their lerp rounds differently) and never the library.
Selection is exact, so results are compared as uint64 bit patterns (NaN equals NaN).  Matrices are
built directly as device tensors with every padding element (rows n_rows .. ld-1 of a column) NaN,
so a kernel that reads padding poisons its result.

Only the log2 cases have an allowance: 4 * 2^-53 * max|log2(x + 1)| absolute on quantiles and
medians and three times that on mad (centre, deviation, scale) -- the device's and NumPy's log2 are
each documented to about 1 ulp and are not the same function; the factor leaves 2x on their sum."""
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
SLAB = 4096          # kSumColSlabRows: rows of a column in one (column, slab) unit
MAX_PROBS = 8        # RCP_QUANTILE_MAX_PROBS
UNITS = 4            # kQUnitsPerGroup: units a workgroup counts before it flushes
MATRIX_GROUPS = 2048  # kQMatrixGroups: whole-matrix scope grows the units per workgroup beyond this many groups
MATRIX, COLS = 0, 1
EPS = 2.0 ** -53
F = np.float64

P5 = [0.0, 0.5, 0.95, 0.999, 1.0]
LADDER = [0.95, 0.96, 0.97, 0.98, 0.99, 0.995, 0.999]
P8 = LADDER + [0.5]
PROB_SETS = [P5, LADDER, P8]


def test_restated_constants_match_the_source(gpu):
    txt = open(os.path.join(ROOT, "recoup_amd", "csrc", "rcp_summary.h")).read()
    assert int(re.search(r"kSumColSlabRows = (\d+)", txt).group(1)) == SLAB
    assert int(re.search(r"kQUnitsPerGroup = (\d+)", txt).group(1)) == UNITS
    assert int(re.search(r"kQMatrixGroups = (\d+)", txt).group(1)) == MATRIX_GROUPS
    hdr = open(os.path.join(ROOT, "include", "recoup_amd.h")).read()
    assert int(re.search(r"RCP_QUANTILE_MAX_PROBS (\d+)", hdr).group(1)) == MAX_PROBS == len(P8)
    assert tuple(LADDER) == ra.HEATMAP_LADDER


# ------------------------------------------------------------------------------ plumbing
def padded(n):
    return (n + 15) // 16 * 16 + 16


def odd_ld(n):
    return n if n % 2 else n + 1  # unpadded (or one element of padding): every other column off 16 bytes


def lds(n_rows, pad):
    return padded(n_rows) if pad else odd_ld(n_rows)


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


def quantiles(ts, n_rows, n_cols, ld, probs, scope, log=False, col0=0):
    """-> [S, n_segments, n_probs]"""
    S, n_seg = len(ts), (n_cols if scope == COLS else 1)
    n = S * n_seg * len(probs)
    q = torch.full((max(n, 1),), 7.0, dtype=torch.float64, device="cuda")
    d = _desc(ts, n_rows, n_cols, ld, log, col0)
    p = (ctypes.c_double * len(probs))(*probs)
    _lib.check(_lib.lib().rcp_summary_quantiles(ctypes.byref(d), scope, p, len(probs), _lib.ptr(q), _stream()))
    return q.cpu().numpy()[:n].reshape(S, n_seg, len(probs))


def median_mad(ts, n_rows, n_cols, ld, log=False, want=(True, True), col0=0):
    """-> (median, mad) [S, n_cols] each (None where not asked for)"""
    S = len(ts)
    out = [torch.full((max(S * n_cols, 1),), 7.0, dtype=torch.float64, device="cuda") if w else None for w in want]
    d = _desc(ts, n_rows, n_cols, ld, log, col0)
    _lib.check(_lib.lib().rcp_summary_median_mad(ctypes.byref(d), _lib.ptr(out[0]), _lib.ptr(out[1]), _stream()))
    return [None if a is None else a.cpu().numpy()[:S * n_cols].reshape(S, n_cols) for a in out]


# ------------------------------------------------------------------------------ the restatement
def restated_quantile(xs, p):
    """Type 7 over xs = np.sort of a segment whose zeros are all +0.0 (NaN sorts last)."""
    n = len(xs)
    if n == 0 or np.isnan(xs[-1]):
        return F("nan")
    index = F(1.0) + F(n - 1) * F(p)
    lo, hi = np.floor(index), np.ceil(index)
    h = index - lo
    a, b = xs[int(lo) - 1], xs[int(hi) - 1]
    if index == lo or a == b:
        return a
    with np.errstate(all="ignore"):
        return (F(1.0) - h) * a + h * b  # three roundings


def fold(x):
    return np.asarray(x, F) + 0.0  # -0.0 + 0.0 is +0.0


def sorted_segments(x, scope):
    """x [n_rows, n_cols] (already transformed) -> its segments, each sorted (once for all probabilities)."""
    if scope == MATRIX:
        return [np.sort(fold(x).reshape(-1))]
    xs = np.sort(fold(x), axis=0)
    return [xs[:, c] for c in range(x.shape[1])]


def expected_of(segs, probs):
    return np.array([[restated_quantile(xs, p) for p in probs] for xs in segs], F).reshape(len(segs), len(probs))


def expected(x, probs, scope):
    """-> [n_segments, n_probs]"""
    return expected_of(sorted_segments(x, scope), probs)


def expected_median_mad(x):
    med, mad = np.empty(x.shape[1], F), np.empty(x.shape[1], F)
    for c in range(x.shape[1]):
        col = fold(x[:, c])
        med[c] = restated_quantile(np.sort(col), 0.5)
        with np.errstate(all="ignore"):
            dev = np.abs(col - med[c])
        mad[c] = F(1.4826) * restated_quantile(np.sort(dev), 0.5)
    return med, mad


def bits(a):
    a = np.ascontiguousarray(a, F)
    return np.where(np.isnan(a), F("nan"), a).view(np.uint64)


def assert_same_bits(got, want, tag):
    assert got.shape == want.shape, tag
    g, w = bits(got), bits(want)
    assert np.array_equal(g, w), (tag, np.argwhere(g != w)[:4].tolist(), got[g != w][:4], want[g != w][:4])


# ------------------------------------------------------------------------------ data classes
def normal(rng, n_rows, n_cols):
    return rng.standard_normal((n_rows, n_cols))


def zeros70(rng, n_rows, n_cols):
    """70 % exact zeros, the rest integers below 4096 over 8: the answer sits in a huge tie or beside one."""
    return np.where(rng.random((n_rows, n_cols)) < 0.7, 0.0, rng.integers(0, 4096, (n_rows, n_cols)) / 8.0)


def all_equal(rng, n_rows, n_cols):
    return np.full((n_rows, n_cols), 3.25)


def last_digit(rng, n_rows, n_cols):
    """1 + k * 2^-52 for small k, shuffled: keys that differ only in the last digit pass."""
    return 1.0 + rng.integers(0, 200, (n_rows, n_cols)) * 2.0 ** -52


SPECIALS = np.array([-0.0, 0.0, np.inf, -np.inf, 5e-324, -5e-324, 1e-310, np.finfo(F).max, -np.finfo(F).max, 1.0, -1.5])


def specials(rng, n_rows, n_cols):
    return SPECIALS[rng.integers(0, len(SPECIALS), (n_rows, n_cols))]


EXACT_CLASSES = [normal, zeros70, all_equal, last_digit, specials]

# per-column scope: n_rows x n_cols, trimmed to what runs in seconds (257 columns at two heights)
N_ROWS = [1, 2, 3, 4095, 4096, 4097, 8193]


def n_cols_of(n_rows):
    return [1, 3, 257] if n_rows in (3, 4097) else [1, 3]


# ------------------------------------------------------------------------------ per column
@pytest.mark.parametrize("pad", [False, True], ids=["ld=odd", "ld=padded"])
@pytest.mark.parametrize("n_rows", N_ROWS)
def test_column_quantiles(gpu, n_rows, pad):
    rng = np.random.default_rng(1000 + n_rows + pad)
    ld = lds(n_rows, pad)
    for n_cols in n_cols_of(n_rows):
        for make in EXACT_CLASSES:
            if n_rows * n_cols > 100000 and make in (all_equal, specials):
                continue
            x = make(rng, n_rows, n_cols)
            t = device_matrix(x, ld)
            segs = sorted_segments(x, COLS)
            for probs in PROB_SETS:
                got = quantiles([t], n_rows, n_cols, ld, probs, COLS)[0]
                assert_same_bits(got, expected_of(segs, probs), (make.__name__, n_rows, n_cols, ld, len(probs)))


def test_column_split_over_two_workgroups(gpu):
    """More slabs than one workgroup counts: the column's histogram is the sum of two flushes."""
    rng = np.random.default_rng(5)
    n_rows, n_cols = UNITS * SLAB + 5, 3
    for pad in (False, True):
        ld = lds(n_rows, pad)
        for make in (normal, zeros70):
            x = make(rng, n_rows, n_cols)
            got = quantiles([device_matrix(x, ld)], n_rows, n_cols, ld, P8, COLS)[0]
            assert_same_bits(got, expected(x, P8, COLS), (make.__name__, ld))


def test_several_samples(gpu):
    rng = np.random.default_rng(6)
    n_rows, n_cols, ld = SLAB + 1, 3, padded(SLAB + 1)
    xs = [normal(rng, n_rows, n_cols), zeros70(rng, n_rows, n_cols), last_digit(rng, n_rows, n_cols)]
    ts = [device_matrix(x, ld) for x in xs]
    for scope in (COLS, MATRIX):
        got = quantiles(ts, n_rows, n_cols, ld, P5, scope)
        for s, x in enumerate(xs):
            assert_same_bits(got[s], expected(x, P5, scope), (scope, s))
    med, mad = median_mad(ts, n_rows, n_cols, ld)
    for s, x in enumerate(xs):
        em, ed = expected_median_mad(x)
        assert_same_bits(med[s], em, s)
        assert_same_bits(mad[s], ed, s)


# ------------------------------------------------------------------------------ whole matrix
@pytest.mark.parametrize("pad", [False, True], ids=["ld=odd", "ld=padded"])
@pytest.mark.parametrize("shape", [(65, 257), (4097, 3), (3, UNITS * MATRIX_GROUPS + 8)], ids=str)
def test_matrix_quantiles(gpu, shape, pad):
    """65 x 257: workgroups of 4 units that cross columns; 3 x 8200: more units than 4 per each of
    2048 groups, so a workgroup takes 5."""
    n_rows, n_cols = shape
    rng = np.random.default_rng(2000 + n_rows + pad)
    ld = lds(n_rows, pad)
    for make in EXACT_CLASSES:
        x = make(rng, n_rows, n_cols)
        t = device_matrix(x, ld)
        segs = sorted_segments(x, MATRIX)
        for probs in PROB_SETS:
            got = quantiles([t], n_rows, n_cols, ld, probs, MATRIX)[0]
            assert_same_bits(got, expected_of(segs, probs), (make.__name__, shape, ld, len(probs)))


# ------------------------------------------------------------------------------ special values
def test_selected_zero_is_positive_and_infinities_tie(gpu):
    z = np.array([-1.0, -0.0, -0.0, 0.0, 1.0])  # the median is a -0.0 element: returned as +0.0
    inf = np.array([1.0, np.inf, np.inf, np.inf])  # 4 elements at 0.5: lo and hi both +Inf
    neg = np.array([-np.inf, -np.inf, -np.inf, 0.0])  # lo and hi both -Inf
    for x, want in ((z, 0.0), (inf, np.inf), (neg, -np.inf)):
        n = len(x)
        t = device_matrix(x[:, None], padded(n))
        for scope in (COLS, MATRIX):
            got = quantiles([t], n, 1, padded(n), [0.5], scope)[0, 0, 0]
            assert F(got).view(np.uint64) == F(want).view(np.uint64), (x, scope, got)
        med, mad = median_mad([t], n, 1, padded(n))
        assert F(med[0, 0]).view(np.uint64) == F(want).view(np.uint64)
    # a tie of zeros of both signs around an interpolation point stays +0.0; mad of it too
    x = np.array([-0.0, 0.0, -0.0, 0.0])
    t = device_matrix(x[:, None], padded(4))
    med, mad = median_mad([t], 4, 1, padded(4))
    assert bits(med).tolist() == [[0]] and bits(mad).tolist() == [[0]]
    # -Inf and +Inf interpolate to NaN, as in R
    x = np.array([-np.inf, np.inf])
    assert np.isnan(quantiles([device_matrix(x[:, None], padded(2))], 2, 1, padded(2), [0.5], COLS)).all()


@pytest.mark.parametrize("pad", [False, True], ids=["ld=odd", "ld=padded"])
def test_one_nan_poisons_its_segment_only(gpu, pad):
    rng = np.random.default_rng(7)
    for n_rows, n_cols, where in ((4097, 3, (4096, 1)), (65, 257, (0, 200)), (3, 3, (1, 2))):
        ld = lds(n_rows, pad)
        x = normal(rng, n_rows, n_cols)
        x[where] = -np.nan if pad else np.nan  # either sign
        t = device_matrix(x, ld)
        want = expected(x, P5, COLS)
        assert np.isnan(want[where[1]]).all() and not np.isnan(np.delete(want, where[1], axis=0)).any()
        assert_same_bits(quantiles([t], n_rows, n_cols, ld, P5, COLS)[0], want, (n_rows, n_cols))
        assert np.isnan(quantiles([t], n_rows, n_cols, ld, LADDER, MATRIX)).all()
        med, mad = median_mad([t], n_rows, n_cols, ld)
        em, ed = expected_median_mad(x)
        assert_same_bits(med[0], em, "median")
        assert_same_bits(mad[0], ed, "mad")
        assert np.isnan(mad[0][where[1]]) and np.isnan(med[0][where[1]])


def test_empty_shapes(gpu):
    t = torch.full((4, 32), float("nan"), dtype=torch.float64, device="cuda")
    assert np.isnan(quantiles([t], 0, 4, 32, P5, COLS)).all()      # no rows: every column is numeric(0)
    assert np.isnan(quantiles([t, t], 0, 4, 32, P5, MATRIX)).all()
    assert np.isnan(quantiles([t], 20, 0, 32, P5, MATRIX)).all()   # no columns: the matrix is numeric(0)
    assert quantiles([t], 20, 0, 32, P5, COLS).size == 0           # nothing is written
    med, mad = median_mad([t], 0, 4, 32)
    assert np.isnan(med).all() and np.isnan(mad).all()
    assert median_mad([t], 20, 0, 32)[0].size == 0


# ------------------------------------------------------------------------------ median and mad
@pytest.mark.parametrize("pad", [False, True], ids=["ld=odd", "ld=padded"])
def test_median_mad(gpu, pad):
    """Even heights give an interpolated median, so the centre of the second selection is not an
    element of the column."""
    rng = np.random.default_rng(3000 + pad)
    for n_rows, n_cols in ((1, 1), (2, 3), (4096, 3), (4097, 3), (2 * SLAB + 1, 1), (UNITS * SLAB + 6, 1), (64, 257)):
        ld = lds(n_rows, pad)
        for make in (normal, zeros70, last_digit):
            x = make(rng, n_rows, n_cols)
            em, ed = expected_median_mad(x)
            if make is normal and n_rows % 2 == 0:
                assert not (x == em[None, :]).any()  # interpolated
            t = device_matrix(x, ld)
            med, mad = median_mad([t], n_rows, n_cols, ld)
            assert_same_bits(med[0], em, ("median", make.__name__, n_rows, n_cols, ld))
            assert_same_bits(mad[0], ed, ("mad", make.__name__, n_rows, n_cols, ld))
            only_med, none = median_mad([t], n_rows, n_cols, ld, want=(True, False))
            assert none is None
            assert_same_bits(only_med[0], em, "median alone")
            none, only_mad = median_mad([t], n_rows, n_cols, ld, want=(False, True))
            assert_same_bits(only_mad[0], ed, "mad alone")
            # the quantile call at 0.5 is the same median
            assert_same_bits(quantiles([t], n_rows, n_cols, ld, [0.5], COLS)[0][:, 0], em, "quantile 0.5")


# ------------------------------------------------------------------------------ log2
def test_log2_scale(gpu):
    """log2(x + 1) first.  Worst error seen over these cases on an MI355X: 0.889 of the allowance
    (the device's and NumPy's log2 a full ulp apart at the largest element, where the allowance is
    two ulps)."""
    rng = np.random.default_rng(8)
    worst = 0.0
    for n_rows, n_cols in ((4097, 3), (65, 257), (8193, 1)):
        for pad in (False, True):
            ld = lds(n_rows, pad)
            for make in (lambda r, a, b: np.abs(normal(r, a, b)) * 50.0, zeros70):
                x = make(rng, n_rows, n_cols)
                xl = np.log2(x + 1.0)
                A = 4 * EPS * np.abs(xl).max()
                t = device_matrix(x, ld)
                for scope in (COLS, MATRIX):
                    for probs in (P5, LADDER):
                        got = quantiles([t], n_rows, n_cols, ld, probs, scope, log=True)[0]
                        err = np.abs(got - expected(xl, probs, scope)).max()
                        worst = max(worst, err / A)
                        assert err <= A, (n_rows, n_cols, ld, scope, err / A)
                med, mad = median_mad([t], n_rows, n_cols, ld, log=True)
                em, ed = expected_median_mad(xl)
                e1, e2 = np.abs(med[0] - em).max(), np.abs(mad[0] - ed).max()
                worst = max(worst, e1 / A, e2 / (3 * A))
                assert e1 <= A and e2 <= 3 * A, (n_rows, n_cols, ld, e1 / A, e2 / (3 * A))
    print(f"log2: worst error / allowance {worst:.3g}")


# ------------------------------------------------------------------------------ column ranges
def test_heatmap_column_range(gpu):
    """A recoupProfiles-style tensor: the heatmap's 3 columns after the profile's 4, selected by
    offsetting the pointer.  The profile's columns hold values that would change every result."""
    rng = np.random.default_rng(9)
    for n_rows, ld in ((65, 65), (65, padded(65)), (SLAB + 1, SLAB + 1)):
        x = zeros70(rng, n_rows, 7)
        x[:, :4] += 1e6
        t = device_matrix(x, ld)
        heat = x[:, 4:]
        for scope in (COLS, MATRIX):
            got = quantiles([t], n_rows, 3, ld, P8, scope, col0=4)[0]
            assert_same_bits(got, expected(heat, P8, scope), (n_rows, ld, scope))
        med, mad = median_mad([t], n_rows, 3, ld, col0=4)
        em, ed = expected_median_mad(heat)
        assert_same_bits(med[0], em, "median")
        assert_same_bits(mad[0], ed, "mad")
        # the Python layer finds the same range from the shapes
        sample = [{"id": "s", "profile": np.zeros((n_rows, 4)), "profile_device": t[:, :n_rows]}]
        q = ra.profileQuantiles(sample, P8, by="column", which="heatmap")[0]
        assert_same_bits(q, expected(heat, P8, COLS), "which=heatmap")
        q = ra.profileQuantiles(sample, P5, by="matrix", which="profile")[0]
        assert_same_bits(q, expected(x[:, :4], P5, MATRIX)[0], "which=profile")


# ------------------------------------------------------------------------------ reproducibility
def test_bit_identical_across_calls_and_streams(gpu):
    rng = np.random.default_rng(11)
    n_rows, n_cols = 2 * SLAB + 77, 257
    ld = padded(n_rows)
    t = device_matrix(zeros70(rng, n_rows, n_cols) + (rng.random((n_rows, n_cols)) < 0.1) * rng.random((n_rows, n_cols)), ld)

    def run():
        out = [quantiles([t], n_rows, n_cols, ld, P8, COLS), quantiles([t], n_rows, n_cols, ld, LADDER, MATRIX),
               quantiles([t], n_rows, n_cols, ld, P5, MATRIX, log=True)]
        out += median_mad([t], n_rows, n_cols, ld, log=True)
        return [np.ascontiguousarray(a).view(np.uint8) for a in out]

    runs = [run(), run()]
    torch.cuda.synchronize()
    for _ in range(2):
        with torch.cuda.stream(torch.cuda.Stream()):
            runs.append(run())
        torch.cuda.synchronize()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert np.array_equal(a, b)


# ------------------------------------------------------------------------------ the Python layer
def _sample(x, name, ld=None):
    ld = ld or padded(x.shape[0])
    return {"id": name, "profile_device": device_matrix(x, ld)[:, :x.shape[0]]}


def test_heatmap_color_limits_each(gpu):
    """100 x 100 with 150 elements that are not 0: the quantiles at 0.95 .. 0.98 are 0, at 0.99 not."""
    rng = np.random.default_rng(12)
    x = np.zeros(10000)
    x[rng.choice(10000, 150, replace=False)] = rng.integers(1, 4096, 150) / 8.0
    x = x.reshape(100, 100)
    y = np.abs(normal(rng, 100, 100))  # the first rung already
    want_x = expected(x, LADDER, MATRIX)[0]
    assert (want_x[:4] == 0).all() and want_x[4] != 0
    opts = {"plotParams": {"heatmapScale": "each", "heatmapFactor": 0.5, "signalScale": "natural"}}
    got = ra.heatmapColorLimits([_sample(x, "x"), _sample(y, "y")], opts)
    sup = np.array([want_x[4], expected(y, [0.95], MATRIX)[0, 0]])
    assert_same_bits(got["sup"], sup, "sup")
    assert got["limits"] == [(0.0, 0.5 * float(v)) for v in sup]
    with pytest.raises(ra.SemanticError, match=r"qs\[8\]"):
        ra.heatmapColorLimits([_sample(np.zeros((100, 3)), "z")], opts)
    opts["plotParams"]["signalScale"] = "log2"
    got = ra.heatmapColorLimits([_sample(x, "x")], opts)
    xl = np.log2(x + 1.0)  # the quantile of the logs, not the log of the quantile: it interpolates
    assert abs(got["sup"][0] - expected(xl, LADDER, MATRIX)[0, 4]) <= 4 * EPS * xl.max()


def test_heatmap_color_limits_common(gpu):
    rng = np.random.default_rng(13)
    x, y = zeros70(rng, 257, 65), zeros70(rng, 257, 65) * 2.0
    opts = {"plotParams": {"heatmapScale": "common", "heatmapFactor": 2.0, "signalScale": "natural"}}
    got = ra.heatmapColorLimits([_sample(x, "x"), _sample(y, "y", ld=257)], opts)
    sup = max(expected(x, [0.95], MATRIX)[0, 0], expected(y, [0.95], MATRIX)[0, 0])
    assert_same_bits(got["sup"], np.array([sup, sup]), "sup")
    assert got["limits"] == [(0.0, 2.0 * float(sup))] * 2


FLANK = (2000, 2000)


def test_calc_median_plot_profiles_end_to_end(gpu):
    """test.input's first sample -> coverageRef -> profileMatrix(keep_on_device=True): 100 TSS windows
    in 125 bins; the curve against the restatement applied to sample["profile"]."""
    d = c1_cases.load_inputs()
    G = c1_cases.genome(d)
    genome = ra.GRanges(G["chrom"], G["start"], G["end"], G["strand"], names=G["names"])
    s = list(c1_cases.samples(d))[0]
    sl = {lv: int(v) for lv, v in zip(s["seqlevels"], s["seqlengths"]) if v >= 0}
    reads = ra.GRanges(np.full(len(s["start"]), "chr12"), s["start"], s["end"], s["strand"],
                       seqlevels=s["seqlevels"], seqlengths=sl)
    inp = ra.coverageRef([{"id": s["id"], "name": s["name"], "ranges": reads}], genome, "tss", FLANK)
    inp = ra.profileMatrix(inp, FLANK, {"flankBinSize": 0, "regionBinSize": 125, "sumStat": "mean"},
                           keep_on_device=True)
    p = np.asarray(inp[0]["profile"])
    assert p.shape == (100, 125)
    em, ed = expected_median_mad(p)
    got = ra.calcMedianPlotProfiles(inp, {"plotParams": {"sumStat": "median", "signalScale": "natural"}})[0]
    assert_same_bits(got["profile"], em, "median")
    assert_same_bits(got["upper"], em + ed, "upper")
    assert_same_bits(got["lower"], em - ed, "lower")
    pl = np.log2(p + 1.0)
    em, ed = expected_median_mad(pl)
    A = 4 * EPS * np.abs(pl).max()
    got = ra.calcMedianPlotProfiles(inp, {"plotParams": {"signalScale": "log2"}})[0]
    assert np.abs(got["profile"] - em).max() <= A
    assert np.abs((got["upper"] - got["profile"]) - ed).max() <= 4 * A  # mad's 3 and the sum's rounding
    q = ra.profileQuantiles(inp, [0.5], by="column")[0]
    assert_same_bits(q[:, 0], expected_median_mad(p)[0], "profileQuantiles")
