"""Exact quantiles of kept profile matrices, the parts that need no GPU: the argument checks of
rcp_summary_quantiles / rcp_summary_median_mad (made before the device is touched), the no-device
behaviour, the rank arithmetic rcp_quantile_ranks, the host walk over the heatmap ladder
(R/plot.R:515-523) and the option checks of profileQuantiles / heatmapColorLimits /
calcMedianPlotProfiles."""
import ctypes
import math

import numpy as np
import pytest
import torch

import recoup_amd as ra
from recoup_amd import _lib

NO_GPU = not torch.cuda.is_available()
EINVAL, EUNSUPPORTED, ENODEVICE = -1, -4, -6
OUT = ctypes.c_void_p(8)  # never dereferenced: every call below fails or launches nothing


def _desc(n_rows, n_cols, ld, n_samples, ptrs=None):
    arr = None
    if ptrs is not None:
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    d = _lib.MatrixDesc(n_rows, n_cols, ld, n_samples, 0, arr)
    d._keep = arr
    return d


def _probs(*p):
    return (ctypes.c_double * len(p))(*p)


def quantiles(d, scope=0, probs=_probs(0.5), n_probs=1, out=OUT):
    return _lib.lib().rcp_summary_quantiles(None if d is None else ctypes.byref(d), scope, probs, n_probs, out, None)


def median_mad(d, med=OUT, mad=OUT):
    return _lib.lib().rcp_summary_median_mad(None if d is None else ctypes.byref(d), med, mad, None)


# ------------------------------------------------------------------------------ argument checks
@pytest.mark.parametrize("d,word", [
    (None, b"NULL"),
    (_desc(10, 4, 9, 1, [16]), b"ld"),
    (_desc(10, 4, 16, 0, [16]), b"n_samples"),
    (_desc(-1, 4, 16, 1, [16]), b"negative"),
    (_desc(10, 4, 16, 1, None), b"d_mat"),
    (_desc(10, 4, 16, 2, [16, 0]), b"d_mat"),
])
def test_descriptor_checks_are_those_of_the_other_summaries(d, word):
    assert quantiles(d) == EINVAL
    assert word in _lib.lib().rcp_last_error()
    assert median_mad(d) == EINVAL
    assert word in _lib.lib().rcp_last_error()


def test_rows_above_2_31_are_unsupported():
    d = _desc(1 << 31, 1, 1 << 31, 1, [16])
    assert quantiles(d) == EUNSUPPORTED and median_mad(d) == EUNSUPPORTED


def test_scope_is_checked():
    d = _desc(0, 0, 0, 1)
    assert quantiles(d, scope=2) == EINVAL
    assert b"scope" in _lib.lib().rcp_last_error()
    assert quantiles(d, scope=-1) == EINVAL


def test_probs_are_checked():
    d = _desc(0, 0, 0, 1)
    assert quantiles(d, probs=None) == EINVAL
    assert b"probs" in _lib.lib().rcp_last_error()
    assert quantiles(d, n_probs=0) == EINVAL
    assert quantiles(d, n_probs=-3) == EINVAL
    nine = _probs(*[0.1 * k for k in range(9)])
    assert quantiles(d, probs=nine, n_probs=9) == EUNSUPPORTED
    assert b"n_probs" in _lib.lib().rcp_last_error()
    for bad in (float("nan"), -1e-9, 1.0000001, float("inf")):
        assert quantiles(d, probs=_probs(0.5, bad), n_probs=2) == EINVAL, bad
        assert b"[0,1]" in _lib.lib().rcp_last_error()


def test_null_outputs_are_einval():
    d = _desc(0, 0, 0, 1)
    assert quantiles(d, out=None) == EINVAL
    assert b"d_q" in _lib.lib().rcp_last_error()
    assert median_mad(d, None, None) == EINVAL
    assert b"both NULL" in _lib.lib().rcp_last_error()


def test_a_segment_of_2_32_elements_is_unsupported():
    """Counters are 32-bit: the whole matrix as one segment is refused from 2^32 elements on, before
    any device is looked for; the same matrix by column is not refused for its size."""
    d = _desc(1 << 16, 1 << 16, 1 << 16, 1, [16])
    assert quantiles(d, scope=0) == EUNSUPPORTED
    assert b"2^32" in _lib.lib().rcp_last_error()
    if NO_GPU:  # below the limit, and the same matrix by column: accepted as far as the device
        assert quantiles(_desc(1 << 16, (1 << 16) - 1, 1 << 16, 1, [16]), scope=0) == ENODEVICE
        assert quantiles(d, scope=1) == ENODEVICE


def test_valid_arguments_need_a_device():
    """An empty matrix is legal: on a GPU machine column scope over no columns writes nothing and
    median_mad launches nothing; without a GPU every entry point reports RCP_ENODEVICE."""
    want = ENODEVICE if NO_GPU else 0
    d = _desc(0, 0, 0, 1)
    assert quantiles(d, scope=1) == want
    assert median_mad(d) == want
    assert median_mad(d, OUT, None) == want and median_mad(d, None, OUT) == want
    if NO_GPU:
        assert quantiles(_desc(10, 4, 16, 1, [16]), probs=_probs(0.0, 1.0), n_probs=2) == ENODEVICE
        assert b"no HIP device" in _lib.lib().rcp_last_error()
        assert median_mad(_desc(10, 4, 16, 1, [16])) == ENODEVICE


# ------------------------------------------------------------------------------ ranks
def ranks(n, p):
    lo, hi, h = ctypes.c_int64(-7), ctypes.c_int64(-7), ctypes.c_double(-7.0)
    _lib.check(_lib.lib().rcp_quantile_ranks(n, p, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(h)))
    return lo.value, hi.value, h.value


def restated_ranks(n, p):
    index = 1.0 + float(n - 1) * p  # two roundings
    lo = math.floor(index)
    return int(lo), int(math.ceil(index)), index - lo


@pytest.mark.parametrize("n", [1, 2, 3, 4, 4097, 2 * 10 ** 8])
@pytest.mark.parametrize("p", [0.0, 0.5, 0.95, 0.999, 1.0, 0.25])
def test_ranks_match_the_restatement(n, p):
    lo, hi, h = ranks(n, p)
    assert (lo, hi) == restated_ranks(n, p)[:2]
    assert np.float64(h).view(np.uint64) == np.float64(restated_ranks(n, p)[2]).view(np.uint64)
    assert 1 <= lo <= hi <= n and hi - lo <= 1 and 0.0 <= h < 1.0
    assert (h == 0.0) == (lo == hi)


def test_ranks_at_an_integer_index():
    """(n - 1) * p an integer: lo == hi and no interpolation -- 4097 elements at 0.25 is element 1025."""
    assert ranks(4097, 0.25) == (1025, 1025, 0.0)
    assert ranks(5, 0.5) == (3, 3, 0.0)
    assert ranks(4, 0.5) == (2, 3, 0.5)
    assert ranks(0, 0.5) == (0, 0, 0.0)  # an empty segment: the calls give NaN


def test_ranks_arguments():
    L = _lib.lib()
    lo, hi, h = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
    assert L.rcp_quantile_ranks(-1, 0.5, lo, hi, h) == EINVAL
    assert L.rcp_quantile_ranks(4, 1.5, lo, hi, h) == EINVAL
    assert L.rcp_quantile_ranks(4, float("nan"), lo, hi, h) == EINVAL
    assert L.rcp_quantile_ranks(4, 0.5, None, hi, h) == EINVAL


# ------------------------------------------------------------------------------ the Python layer
def test_ladder_walk():
    assert ra.HEATMAP_LADDER == (0.95, 0.96, 0.97, 0.98, 0.99, 0.995, 0.999)
    assert ra.walkHeatmapLadder([2.5, 3, 4, 5, 6, 7, 8]) == 2.5                # the first is not 0
    assert ra.walkHeatmapLadder([0, 0, 0, 0, 1.25, 2, 3]) == 1.25              # a later one
    assert ra.walkHeatmapLadder([0.0, -0.0, 0, 0, 0, 0, 1e-300]) == 1e-300     # -0.0 is 0 to R
    with pytest.raises(ra.SemanticError, match=r"qs\[8\]"):
        ra.walkHeatmapLadder([0.0] * 7)


def test_heatmap_scale_is_validated():
    inp = [{"id": "s1"}]  # never reached
    with pytest.raises(ra.SemanticError, match="heatmapScale"):
        ra.heatmapColorLimits(inp, {"plotParams": {"heatmapScale": "all", "heatmapFactor": 1}})
    with pytest.raises(ra.SemanticError, match="neither natural nor log2"):
        ra.heatmapColorLimits(inp, {"plotParams": {"heatmapScale": "each", "signalScale": "ln"}})


def test_missing_device_matrix_names_keep_on_device():
    inp = [{"id": "s1", "profile": np.zeros((4, 3))}]  # a host profile alone is never read
    opts = {"plotParams": {"heatmapScale": "each", "heatmapFactor": 1, "signalScale": "natural"}}
    for call in (lambda: ra.profileQuantiles(inp, [0.5]), lambda: ra.profileQuantiles(inp, [0.5], by="column"),
                 lambda: ra.heatmapColorLimits(inp, opts),
                 lambda: ra.heatmapColorLimits(inp, {"plotParams": {"heatmapScale": "common"}}),
                 lambda: ra.calcMedianPlotProfiles(inp, opts)):
        with pytest.raises(ValueError, match="keep_on_device=True"):
            call()


def test_heatmap_columns_must_be_there():
    """which="heatmap" on a kept tensor that holds the profile's columns only (a question about
    shapes, asked before the tensor's device matters)."""
    inp = [{"id": "s1", "profile": np.zeros((4, 3)), "profile_device": torch.zeros((3, 4), dtype=torch.float64)}]
    with pytest.raises(ValueError, match="no heatmap columns"):
        ra.profileQuantiles(inp, [0.5], which="heatmap")
    with pytest.raises(ValueError, match="no heatmap columns"):
        ra.heatmapColorLimits(inp, {"plotParams": {"heatmapScale": "each"}}, which="heatmap")
    with pytest.raises(ValueError, match="neither 'profile' nor 'heatmap'"):
        ra.profileQuantiles(inp, [0.5], which="both")


def test_by_and_scale_are_validated():
    with pytest.raises(ValueError, match="neither 'matrix' nor 'column'"):
        ra.profileQuantiles([{"id": "s1"}], [0.5], by="row")
    with pytest.raises(ra.SemanticError, match="neither natural nor log2"):
        ra.profileQuantiles([{"id": "s1"}], [0.5], scale="ln")


def test_out_of_scope_options_raise():
    inp = [{"id": "s1"}]
    with pytest.raises(ra.UnsupportedError, match="sdim = 1"):
        ra.calcMedianPlotProfiles(inp, {"plotParams": {}}, sdim=1)
    with pytest.raises(ra.UnsupportedError, match="smooth"):
        ra.calcMedianPlotProfiles(inp, {"plotParams": {"smooth": True}})
    # the mean functions keep refusing the median: routing it is a later change
    with pytest.raises(ra.UnsupportedError, match="median"):
        ra.calcPlotProfiles(inp, {"plotParams": {"sumStat": "median"}})
