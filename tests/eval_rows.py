"""tests/golden/eval_rows.npz for the two test files that read it (tests/test_eval_reference_rows_cpu.py,
tests/test_gpu_eval_reference_rows.py): the reference's own per-image eval functions, recorded by
tests/golden/make_golden.py (golden_eval_rows) on float32 tensors and on the same values as float64, renamed here to the
keys of `eval.image_metrics_unc` / `depth_metrics_unc` as get_image_metrics_and_images_unc renames them (that renaming is
itself recorded: the `frame` part of the fixture).

The bounds.  AUSE scalars and curves: 2e-6 absolute, the gate tests/test_golden_cpu.py (test_ause_matches_reference) holds
`metrics.ause` to.  Every other key k: y_k = the largest |reference on float32 - reference on float64| over all recorded cases, per case not
smaller than one float32 ulp of the value, 2^-23 |reference on float64| (for the NLL 2^-23 of the recorded mean |term|:
the terms change sign, their mean may be near 0) -- the distance the reference keeps from itself when its arithmetic is
float32.  The kernels' per-pixel terms are float32 in front of float64 sums, so they get 4 y_k (the factor this project
uses elsewhere) against the float64 recording; the host route runs the reference's float32 operations and gets the same
bound against the float32 recording.  The coverage arrays are counts over n: equal."""
import functools

import numpy as np

from conftest import golden

ULP32 = 2.0 ** -23
FACTOR = 4.0
AUSE_GATE = 2e-6
COVERAGE = ("coverage_values", "coverage_error_values", "abs_coverage_error_values", "neg_coverage_error_values")
WORST = {}                                                  # key -> (worst |difference| / bound, where)


def _renamed(prefix, scalars, curves, coverage, avg_length, names):
    """one record under the project's key names -> (metrics dict, curves dict, mean |NLL term|)"""
    s = dict(zip(names["scalars"], scalars))
    md = {f"{prefix}_ause_{et}": s[f"ause_{et}"] for et in ("mse", "mae", "rmse")}
    md.update({f"{prefix}_mse": s["mse"], f"{prefix}_rmse": s["rmse"], f"{prefix}_nll": s["nll"], f"{prefix}_avg_var": s["avg_var"],
               f"{prefix}_auc_abs_error": s["auc_abs_error_values"], f"{prefix}_auc_length": s["auc_length_values"],
               f"{prefix}_auc_neg_error": s["auc_neg_error_values"]})
    cv = {}
    for name, curve in zip(names["curves"], curves):        # err_mse -> rgb_all_ause_mse, err_var_mse -> rgb_all_var_ause_mse
        cv[f"{prefix}_all_" + name.replace("err_var_", "var_ause_").replace("err_", "ause_")] = curve
    for name, curve in zip(names["coverage"], coverage):
        cv[f"{prefix}_all_auce_{name}"] = curve
    cv[f"{prefix}_all_auce_avg_length_values"] = avg_length
    return md, cv, s["nll_abs_mean"]


@functools.lru_cache(maxsize=None)
def load():
    """-> {"rgb": {case: {...}}, "depth": {case: {...}}, "frame": {...}}; a case holds its float32 inputs and per precision
    ("f32", "f64") the tuple (metrics dict, curves dict, mean |NLL term|)"""
    g = golden("eval_rows.npz")
    names = {"scalars": [str(k) for k in g["eval_scalar_names"]], "curves": [str(k) for k in g["eval_curve_names"]],
             "coverage": [str(k) for k in g["eval_coverage_names"]]}
    out = {"rgb": {}, "depth": {}, "min_std": {"rgb": float(g["rgb_min_std"]), "depth": float(g["depth_min_std"])}}
    for prefix in ("rgb", "depth"):
        for case in (str(c) for c in g[f"{prefix}_cases"]):
            tag = f"{prefix}_{case}"
            if prefix == "rgb":                             # the ground truth sits on the 8-bit grid: float32(k) / float32(255)
                c = {"pred": g[f"{tag}_pred"], "gt": g[f"{tag}_gt_u8"].astype(np.float32) / np.float32(255), "std": g[f"{tag}_std"]}
            else:
                c = {"depth": g[f"{tag}_depth"], "std": g[f"{tag}_std"], "gt": g[f"{tag}_gt"], "scale": float(g[f"{tag}_scale"])}
            # the float32 run's curves are stored as their (float32) difference from the float64 run's
            curves64, length64 = g[f"{tag}_f64_curves"], g[f"{tag}_f64_avg_length"]
            c["f64"] = _renamed(prefix, g[f"{tag}_f64_scalars"], curves64, g[f"{tag}_coverage"], length64, names)
            c["f32"] = _renamed(prefix, g[f"{tag}_f32_scalars"], curves64 + g[f"{tag}_d32_curves"], g[f"{tag}_coverage"],
                                length64 + g[f"{tag}_d32_avg_length"], names)
            out[prefix][case] = c
    f = {"keys": [str(k) for k in g["frame_f32_keys"]], "avg": dict(zip((str(k) for k in g["frame_f32_keys"]), g["frame_f32_avg"])),
         "scale": float(g["frame_scale"]), "min_rgb_std": float(g["frame_min_rgb_std"]), "min_depth_std": float(g["frame_min_depth_std"]),
         "images": [], "plots": {}}
    for n in (100, 99):
        f["plots"].update(zip((str(k) for k in g[f"frame_f32_plot_keys_{n}"]), g[f"frame_f32_plot_{n}"]))
    i = 0
    while f"frame_img{i}_rgb" in g.files:
        im = {k: g[f"frame_img{i}_{k}"] for k in ("rgb", "rgb_std", "depth", "depth_std", "depth_gt", "accumulation")}
        im["image"] = g[f"frame_img{i}_image_u8"].astype(np.float32) / np.float32(255)
        im["metrics"] = dict(zip(f["keys"], g[f"frame_f32_img{i}"]))
        im["curves"] = {}
        for n in (100, 99):
            im["curves"].update(zip((str(k) for k in g[f"frame_f32_curve_keys_{n}"]), g[f"frame_f32_img{i}_curves_{n}"]))
        f["images"].append(im)
        i += 1
    out["frame"] = f
    return out


@functools.lru_cache(maxsize=None)
def yardsticks():
    """key -> y_k: the largest |float32 run - float64 run| of the reference over the recorded cases (NaN entries, equal in
    both runs, left out); scalars and arrays alike give one number per key"""
    y = {}
    rows = load()
    for prefix in ("rgb", "depth"):
        for c in rows[prefix].values():
            for part in (0, 1):
                for k, v64 in c["f64"][part].items():
                    d = np.abs(np.asarray(c["f32"][part][k], dtype=np.float64) - np.asarray(v64, dtype=np.float64))
                    assert np.array_equal(np.isnan(d), np.isnan(np.asarray(v64, dtype=np.float64))), (prefix, k)
                    y[k] = max(y.get(k, 0.0), float(np.nanmax(d)) if not np.all(np.isnan(d)) else 0.0)
    return y


def bound(key, ref64, nll_abs_mean):
    """the module docstring's bound for one key of one case, elementwise for an array"""
    if "_ause_" in key:
        return AUSE_GATE
    if any(key.endswith(c) for c in COVERAGE):
        return 0.0
    floor = ULP32 * (nll_abs_mean if key.endswith("_nll") else np.abs(np.asarray(ref64, dtype=np.float64)))
    return FACTOR * np.maximum(yardsticks()[key], floor)


def check(got_md, got_curves, case, against, what):
    """every key of the recording `against` ("f32" / "f64") of `case`: NaN exactly where the reference has NaN, else inside
    `bound`; the measured share of the bound is printed per key and kept in WORST"""
    md, curves, _ = case[against]
    md64, curves64, nll_abs_mean = case["f64"]
    for want_d, got_d, ref64_d in ((md, got_md, md64), (curves, got_curves, curves64)):
        for k, want in want_d.items():
            assert k in got_d, (what, k, "missing")
            got, want = np.asarray(got_d[k], dtype=np.float64), np.asarray(want, dtype=np.float64)
            assert got.shape == want.shape, (what, k, got.shape, want.shape)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan), (what, k, "NaN where the reference has none, or the other way round", got, want)
            diff = np.where(nan, 0.0, np.abs(got - want))
            b = bound(k, ref64_d[k], nll_abs_mean) * np.ones_like(diff)
            if np.all(b == 0):
                assert np.all(diff == 0), (what, k, "equal", float(diff.max()))
                continue
            share = float(np.max(np.where(nan, 0.0, diff / np.where(nan, 1.0, b))))
            if share > WORST.get(k, (0.0, ""))[0]:
                WORST[k] = (share, what)
            print(f"[{what}] {k}: worst |difference| {float(diff.max()):.3e} = {share:.3f} of its bound")
            assert share <= 1.0, (what, k, float(diff.max()), float(np.max(b)), got, want)


def print_worst(title):
    print(f"[{title}] worst share of the bound per key so far: "
          + ", ".join(f"{k} {v:.3f} ({w})" for k, (v, w) in sorted(WORST.items())))
