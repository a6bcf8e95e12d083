"""Device summaries of kept profile matrices, the parts that need no GPU: the argument checks of
rcp_summary_cols / rcp_summary_rows / rcp_order_rows (made before the device is touched), the
no-device behaviour, the ctypes mirror of rcp_matrix_desc, the orderBy$what parser
(R/plot.R:1044-1066), the host paths (orderBy$custom, "none") and the out-of-scope options."""
import ctypes
import os
import subprocess
import warnings

import numpy as np
import pytest
import torch

import recoup_amd as ra
from recoup_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_GPU = not torch.cuda.is_available()


def _desc(n_rows, n_cols, ld, n_samples, ptrs=None):
    arr = None
    if ptrs is not None:
        arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
    d = _lib.MatrixDesc(n_rows, n_cols, ld, n_samples, 0, arr)
    d._keep = arr
    return d


def _calls(d, n_groups=0, gid=None):
    """The three entry points on one descriptor (outputs NULL where the ABI allows it)."""
    L = _lib.lib()
    p = None if d is None else ctypes.byref(d)
    order = ctypes.c_void_p(8)  # never dereferenced: every call below fails or launches nothing
    return [L.rcp_summary_cols(p, gid, n_groups, None, None, None, None),
            L.rcp_summary_rows(p, None, None, None, None, None),
            L.rcp_order_rows(p, 0, -1, 0, gid, n_groups, order, None, None)]


def test_null_descriptor_is_einval():
    assert _calls(None) == [-1, -1, -1]
    assert b"NULL" in _lib.lib().rcp_last_error()


def test_ld_below_n_rows_is_einval():
    assert _calls(_desc(10, 4, 9, 1, [16])) == [-1, -1, -1]
    assert b"ld" in _lib.lib().rcp_last_error()


def test_no_samples_is_einval():
    assert _calls(_desc(10, 4, 16, 0, [16])) == [-1, -1, -1]
    assert b"n_samples" in _lib.lib().rcp_last_error()


def test_null_matrix_pointer_is_einval():
    assert _calls(_desc(10, 4, 16, 1, None)) == [-1, -1, -1]
    assert _calls(_desc(10, 4, 16, 2, [16, 0])) == [-1, -1, -1]


def test_order_arguments_are_checked():
    L = _lib.lib()
    d = _desc(0, 0, 0, 1)
    order = ctypes.c_void_p(8)
    assert L.rcp_order_rows(ctypes.byref(d), 3, -1, 0, None, 0, order, None, None) == -1   # what
    assert L.rcp_order_rows(ctypes.byref(d), 0, 1, 0, None, 0, order, None, None) == -1    # ref_sample
    assert L.rcp_order_rows(ctypes.byref(d), 0, -2, 0, None, 0, order, None, None) == -1
    assert L.rcp_order_rows(ctypes.byref(d), 0, -1, 0, None, 0, None, None, None) == -1    # d_order


def test_groups_above_the_cap_are_unsupported():
    """More groups than the kernels reduce: RCP_EUNSUPPORTED, before any device is looked for."""
    gid = ctypes.c_void_p(8)
    d = _desc(0, 0, 0, 1)
    rc = _calls(d, n_groups=65, gid=gid)
    assert rc[0] == -4 and rc[2] == -4
    assert _calls(d, n_groups=0, gid=gid)[0] == -1  # ids without groups


def test_valid_arguments_need_a_device():
    """An empty matrix is legal: nothing is launched on a GPU machine; without a GPU every entry
    point reports RCP_ENODEVICE (no CPU path)."""
    want = -6 if NO_GPU else 0
    assert _calls(_desc(0, 0, 0, 1)) == [want] * 3
    if NO_GPU:
        assert _calls(_desc(10, 4, 16, 1, [16])) == [-6, -6, -6]
        assert b"no HIP device" in _lib.lib().rcp_last_error()


def test_matrix_desc_layout_matches_the_header(tmp_path):
    fields = [n for n, _ in _lib.MatrixDesc._fields_]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "recoup_amd.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(rcp_matrix_desc));']
    lines += [f'  printf("{f} %zu\\n", offsetof(rcp_matrix_desc, {f}));' for f in fields]
    lines += ['  printf("cap %d\\n", RCP_SUMMARY_MAX_GROUPS);', "  return 0;", "}"]
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(exe)], capture_output=True, text=True,
                                                   check=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.MatrixDesc) == int(got["size"])
    for f in fields:
        assert getattr(_lib.MatrixDesc, f).offset == int(got[f]), f
    assert int(got["cap"]) >= 64


@pytest.mark.parametrize("what,stat,ref,warns", [
    ("suma", "sum", 0, False),
    ("sum1", "sum", 1, False),
    ("max3", "max", 3, False),
    ("avga", "avg", 0, False),
    ("sumn", "sum", 1, True),
    ("none", None, 1, False),
])
def test_order_what_parser(what, stat, ref, warns):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        assert ra.parseOrderWhat(what) == (stat, ref)
    assert bool([x for x in w if "not recognized" in str(x.message)]) == warns


def test_hc_order_is_unsupported():
    with pytest.raises(ra.UnsupportedError, match="hc"):
        ra.parseOrderWhat("hcn")
    with pytest.raises(ra.UnsupportedError, match="hc"):
        ra.orderProfiles([{"id": "a"}], {"orderBy": {"what": "hcn", "order": "descending"}})


def test_custom_order_runs_on_the_host():
    """orderBy$custom: sort(custom, index.return=TRUE) without any sample matrix (plot.R:1036-1043);
    equal values keep their order in both directions."""
    custom = [3.0, 1.0, 3.0, 2.0, 1.0]
    inp = [{"id": "a"}]  # no profile_device: the device is never asked
    up = ra.orderProfiles(inp, {"orderBy": {"custom": custom, "order": "ascending", "what": "suma"}})
    assert up["ix"].tolist() == [1, 4, 3, 0, 2] and up["x"].tolist() == [1, 1, 2, 3, 3]
    down = ra.orderProfiles(inp, {"orderBy": {"custom": custom, "order": "descending", "what": "suma"}})
    assert down["ix"].tolist() == [0, 2, 3, 1, 4] and down["x"].tolist() == [3, 3, 2, 1, 1]
    by = ra.orderProfilesByDesign(inp, np.array([1, 0, 0, 1, 0]), {"orderBy": {"custom": custom,
                                                                             "order": "ascending"}})
    assert by["ix"].tolist() == [1, 4, 2, 3, 0]


def test_design_groups():
    gid, names = ra.designGroups(np.array(["b", "a", "b", "c"]), 4)
    assert gid.tolist() == [1, 0, 1, 2] and names == ["a", "b", "c"] and gid.dtype == np.int32
    # two factors: existing combinations only, the first varying fastest; None leaves a row out
    gid, names = ra.designGroups([np.array([1, 2, 1, None, 2], object), np.array(["x", "x", "y", "y", "y"])], 5)
    assert gid.tolist() == [0, 1, 2, -1, 3] and names == ["1.x", "2.x", "1.y", "2.y"]
    with pytest.raises(ra.SemanticError):
        ra.designGroups(np.zeros(3), 4)


def test_missing_device_matrix_names_keep_on_device():
    inp = [{"id": "s1", "profile": np.zeros((4, 3))}]  # a host profile alone is never read
    opts = {"plotParams": {"sumStat": "mean", "signalScale": "natural"},
            "orderBy": {"what": "suma", "order": "descending"}}
    for call in (lambda: ra.calcPlotProfiles(inp, opts), lambda: ra.orderProfiles(inp, opts),
                 lambda: ra.calcDesignPlotProfiles(inp, np.zeros(4, int), opts),
                 lambda: ra.orderProfilesByDesign(inp, np.zeros(4, int), opts)):
        with pytest.raises(ValueError, match="keep_on_device=True"):
            call()


def test_out_of_scope_options_raise():
    inp = [{"id": "s1"}]
    with pytest.raises(ra.UnsupportedError, match="median"):
        ra.calcPlotProfiles(inp, {"plotParams": {"sumStat": "median"}})
    with pytest.raises(ra.UnsupportedError, match="smooth"):
        ra.calcPlotProfiles(inp, {"plotParams": {"sumStat": "mean", "smooth": True}})
    with pytest.raises(ra.UnsupportedError, match="median"):
        ra.calcDesignPlotProfiles(inp, np.zeros(1, int), {"plotParams": {"sumStat": "median"}})
