"""Device summaries of a kept profile matrix against the download-and-NumPy route.

At the C4 result shape (200,000 x 1000 doubles, padded column stride, one sample; seeded values
generated on the device) this times

  * rcp_summary_cols (mean + sd + count), rcp_summary_rows (sum, max, mean, sd) and
    rcp_order_rows("sum", all samples, descending) with device events, after a warm-up, over
    enough repetitions to fill --min-time seconds each, and reports achieved bytes per second:
    the matrix bytes each call reads (every one reads the matrix exactly once) over its time;
  * calcPlotProfiles and orderProfiles("suma") through the Python API with a host clock (they end
    in the device-to-host copy of the curve / the order);
  * what a user does without them: ``profile_device.cpu().numpy()`` followed by the NumPy
    reductions (column mean and sd, row sums, a stable argsort);

  * the exact quantiles (quantile_bench below): rcp_summary_quantiles over the whole matrix at the
    heatmap ladder and per column at 0.5, and rcp_summary_median_mad, each on this input and on one
    with 70 % zeros, per matrix pass against rcp_summary_cols and against download-and-NumPy;

and prints one JSON line (also written to --out).  It needs a GPU; ``--dry-run`` only checks the
arguments and prints the byte arithmetic.

    python tools/summary_bench.py [--rows 200000 --cols 1000] [--out profiles/summary/summary_bench.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_SPEC = 8.0e12      # bytes/s, MI355X HBM3E datasheet
HBM_PEAK_MEASURED = 6.29e12  # bytes/s, float4 copy on MI355X
LEAN_PILEUP_C4 = 4.1e12     # bytes/s of real bytes the lean pileup kernel sustains on C4


def padded_ld(n_rows):
    return (n_rows + 15) // 16 * 16


def matrix_bytes(n_rows, n_cols):
    """Bytes of matrix elements a summary reads (padding rows are never loaded)."""
    return 8 * n_rows * n_cols


def plan(args):
    ld = padded_ld(args.rows)
    return {"n_rows": args.rows, "n_cols": args.cols, "ld": ld, "matrix_bytes": matrix_bytes(args.rows, args.cols),
            "allocated_bytes": 8 * ld * args.cols, "reads_of_matrix": {"cols": 1, "rows": 1, "order": 1}}


def timed(fn, min_time, torch):
    """Mean milliseconds of fn() by device events: warm-up, then repetitions filling min_time."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(3, int(min_time / one) + 1)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, reps


LADDER = [0.95, 0.96, 0.97, 0.98, 0.99, 0.995, 0.999]


def host_quantile(x, probs, ranks, np):
    """The restatement of the type-7 quantile along the last axis of x with np.partition (the
    elements a sort would put at lo and hi): (1 - h) * x_(lo) + h * x_(hi), rounded separately."""
    n = x.shape[-1]
    out = []
    for p in probs:
        lo, hi, h = ranks(n, p)
        part = np.partition(x, sorted({lo - 1, hi - 1}), axis=-1)
        a, b = part[..., lo - 1], part[..., hi - 1]
        out.append(np.where(a == b, a, (1.0 - h) * a + h * b))
    return np.stack(out, axis=-1)


def quantile_bench(args, res, buf, torch, np, _lib):
    """rcp_summary_quantiles (whole matrix, the seven-entry ladder; per column, p = 0.5) and
    rcp_summary_median_mad on a continuous input and on one with 70 % zeros: milliseconds by device
    events, the matrix passes each call makes, the time per pass over rcp_summary_cols of the same
    input in the same run, and the route a user has today (download, then NumPy) with its results
    compared bit for bit."""
    n_rows, n_cols, ld = args.rows, args.cols, res["ld"]
    L = _lib.lib()
    dev = buf.device
    st = _lib.stream_handle(dev)

    def ranks(n, p):
        lo, hi, h = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
        _lib.check(L.rcp_quantile_ranks(n, p, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(h)))
        return lo.value, hi.value, h.value

    def passes(n, probs):  # 8 digit passes, one more for x_(hi) when a probability interpolates
        return 8 + int(any(ranks(n, p)[0] != ranks(n, p)[1] for p in probs))

    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed + 1)
    tied = torch.empty_like(buf)
    tied.exponential_(0.02, generator=gen)
    tied.mul_(8.0).floor_().div_(8.0)  # coverage-like repeated values
    tied[torch.rand(tied.shape, device=dev, generator=gen) < 0.7] = 0.0
    tied[:, n_rows:] = float("nan")
    ladder = (ctypes.c_double * len(LADDER))(*LADDER)
    half = (ctypes.c_double * 1)(0.5)
    q_mat = torch.empty(len(LADDER), dtype=torch.float64, device=dev)
    q_col = torch.empty(n_cols, dtype=torch.float64, device=dev)
    med = torch.empty(n_cols, dtype=torch.float64, device=dev)
    mad = torch.empty(n_cols, dtype=torch.float64, device=dev)
    c_mean = torch.empty(n_cols, dtype=torch.float64, device=dev)
    c_sd = torch.empty_like(c_mean)
    out = {}
    for name, full in (("continuous", buf), ("zeros70", tied)):
        t = full[:, :n_rows]
        arr = (ctypes.c_void_p * 1)(t.data_ptr())
        d = _lib.MatrixDesc(n_rows, n_cols, ld, 1, 0, arr)
        calls = {
            "cols": (lambda: _lib.check(L.rcp_summary_cols(ctypes.byref(d), None, 1, _lib.ptr(c_mean), _lib.ptr(c_sd),
                                                           None, st)), 1),
            "matrix_ladder": (lambda: _lib.check(L.rcp_summary_quantiles(ctypes.byref(d), 0, ladder, len(LADDER),
                                                                         _lib.ptr(q_mat), st)),
                              passes(n_rows * n_cols, LADDER)),
            "column_median": (lambda: _lib.check(L.rcp_summary_quantiles(ctypes.byref(d), 1, half, 1, _lib.ptr(q_col),
                                                                         st)), passes(n_rows, [0.5])),
            "median_mad": (lambda: _lib.check(L.rcp_summary_median_mad(ctypes.byref(d), _lib.ptr(med), _lib.ptr(mad),
                                                                       st)), 2 * passes(n_rows, [0.5])),
        }
        r = {}
        for call, (fn, n_pass) in calls.items():
            ms, reps = timed(fn, args.min_time, torch)
            r[call] = {"ms": ms, "reps": reps, "matrix_passes": n_pass, "ms_per_pass": ms / n_pass}
        for call in list(calls)[1:]:
            r[call]["pass_over_cols_pass"] = r[call]["ms_per_pass"] / r["cols"]["ms"]
        # today's route: the whole matrix over PCIe, then NumPy
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = t.cpu().numpy()  # (n_cols, n_rows)
        t1 = time.perf_counter()
        h_mat = host_quantile(host.reshape(-1), LADDER, ranks, np)
        t2 = time.perf_counter()
        h_med = host_quantile(host, [0.5], ranks, np)[:, 0]
        t3 = time.perf_counter()
        h_mad = 1.4826 * host_quantile(np.abs(host - h_med[:, None]), [0.5], ranks, np)[:, 0]
        t4 = time.perf_counter()
        del host
        dl = (t1 - t0) * 1e3
        r["download_numpy"] = {"download_ms": dl, "matrix_ladder_ms": dl + (t2 - t1) * 1e3,
                               "column_median_ms": dl + (t3 - t2) * 1e3, "median_mad_ms": dl + (t4 - t2) * 1e3}
        for call in list(calls)[1:]:
            r[call]["ratio_to_download_numpy"] = r["download_numpy"][call + "_ms"] / r[call]["ms"]

        def same(a, b):
            return bool(np.array_equal(a.cpu().numpy().view(np.uint64), np.ascontiguousarray(b).view(np.uint64)))
        r["bits_equal_to_numpy"] = {"matrix_ladder": same(q_mat, h_mat), "column_median": same(q_col, h_med),
                                    "median": same(med, h_med), "mad": same(mad, h_mad)}
        out[name] = r
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--cols", type=int, default=1000)
    ap.add_argument("--min-time", type=float, default=0.3, help="seconds of repetitions per timed call")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary", "summary_bench.json"))
    ap.add_argument("--dry-run", action="store_true", help="check arguments and print the byte arithmetic only")
    args = ap.parse_args(argv)
    if args.rows < 1 or args.cols < 1:
        ap.error("--rows and --cols must be positive")
    res = plan(args)
    if args.dry_run:
        print(json.dumps(res))
        return 0

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        sys.exit("summary_bench needs a GPU (no timing is taken on the CPU); use --dry-run to check arguments")
    import recoup_amd as ra
    from recoup_amd import _lib

    n_rows, n_cols, ld = args.rows, args.cols, res["ld"]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(args.seed)
    buf = torch.empty((n_cols, ld), dtype=torch.float64, device="cuda")
    buf.exponential_(0.02, generator=gen)  # coverage-like: positive, mean 50
    buf[:, n_rows:] = float("nan")         # padding must not matter
    t = buf[:, :n_rows]
    L = _lib.lib()
    arr = (ctypes.c_void_p * 1)(t.data_ptr())
    d = _lib.MatrixDesc(n_rows, n_cols, ld, 1, 0, arr)
    dev = t.device
    st = _lib.stream_handle(dev)
    c_mean = torch.empty(n_cols, dtype=torch.float64, device=dev)
    c_sd = torch.empty_like(c_mean)
    c_cnt = torch.empty(n_cols, dtype=torch.int64, device=dev)
    r_out = [torch.empty(n_rows, dtype=torch.float64, device=dev) for _ in range(4)]
    o_ix = torch.empty(n_rows, dtype=torch.int32, device=dev)
    o_key = torch.empty(n_rows, dtype=torch.float64, device=dev)
    calls = {
        "cols": lambda: _lib.check(L.rcp_summary_cols(ctypes.byref(d), None, 1, _lib.ptr(c_mean), _lib.ptr(c_sd),
                                                      _lib.ptr(c_cnt), st)),
        "rows": lambda: _lib.check(L.rcp_summary_rows(ctypes.byref(d), *[_lib.ptr(a) for a in r_out], st)),
        "order": lambda: _lib.check(L.rcp_order_rows(ctypes.byref(d), 0, -1, 1, None, 0, _lib.ptr(o_ix),
                                                     _lib.ptr(o_key), st)),
    }
    for name, fn in calls.items():
        ms, reps = timed(fn, args.min_time, torch)
        bps = res["matrix_bytes"] * res["reads_of_matrix"][name] / (ms * 1e-3)
        res[name] = {"ms": ms, "reps": reps, "bytes_per_s": bps, "share_of_hbm_spec": bps / HBM_PEAK_SPEC,
                     "share_of_hbm_measured": bps / HBM_PEAK_MEASURED, "vs_lean_pileup_c4": bps / LEAN_PILEUP_C4}

    # the Python API, as a user calls it (ends with the curve / the order on the host)
    sample = [{"id": "s", "profile_device": t}]
    opts = {"plotParams": {"sumStat": "mean", "signalScale": "natural"},
            "orderBy": {"what": "suma", "order": "descending"}}

    def wall(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, out

    api_curve_ms, curve = wall(lambda: ra.calcPlotProfiles(sample, opts))
    api_order_ms, order = wall(lambda: ra.orderProfiles(sample, opts))
    res["api"] = {"calcPlotProfiles_ms": api_curve_ms, "orderProfiles_suma_ms": api_order_ms}

    # today's route: the whole matrix over PCIe, then NumPy
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host = t.cpu().numpy()  # (n_cols, n_rows): R's matrix transposed
    t1 = time.perf_counter()
    h_mean = host.mean(axis=1)
    h_sd = host.std(axis=1, ddof=1)
    t2 = time.perf_counter()
    h_key = host.sum(axis=0)
    h_ix = np.argsort(-h_key, kind="stable")
    t3 = time.perf_counter()
    res["download_numpy"] = {"download_ms": (t1 - t0) * 1e3, "curve_ms": (t2 - t1) * 1e3, "order_ms": (t3 - t2) * 1e3,
                             "download_bytes_per_s": res["matrix_bytes"] / (t1 - t0)}
    res["ratio_curve"] = ((t1 - t0) + (t2 - t1)) * 1e3 / api_curve_ms
    res["ratio_order"] = ((t1 - t0) + (t3 - t2)) * 1e3 / api_order_ms
    res["ratio_both"] = (t3 - t0) * 1e3 / (api_curve_ms + api_order_ms)
    # the two routes computed the same things (the timing is of equal work)
    res["max_rel_diff_mean"] = float(np.max(np.abs(curve[0]["profile"] - h_mean) / np.abs(h_mean)))
    res["max_rel_diff_sd"] = float(np.max(np.abs((curve[0]["upper"] - curve[0]["profile"]) - h_sd) / h_sd))
    res["order_rows_differing"] = int((order["ix"] != h_ix).sum())  # (sums round differently: near-ties may swap)
    del host
    res["quantiles"] = quantile_bench(args, res, buf, torch, np, _lib)
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
