#!/usr/bin/env python3
"""The ablation ladder from the archived P2C tracker up (development tool, GPU only).

    python scripts/ablation_p2c.py [--reps 12] [--samples 100] [--out FILE]

Config 2 (dataset 000, srand(0), 100 samples).  The four rungs -- P2C, PH,
PH_CodeOpt and the headline launch (time slicing on, as bench.py runs it) -- are
launched alternately, reps rounds after one warm-up round, each launch timed
with HIP events on its stream: median [min, max] ms per rung, its converged /
real / infinity counts and its mean steps per path, and the ratios of the
medians (improved_over_p2c: P2C / headline).  P2C runs the reference's own
tables (tests/golden/p2c) with the map derived from them.  A measurement: no
threshold applies.  One JSON object, stamped with the library's build id.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    sys.path[:0] = [ROOT]
    import numpy as np
    import torch

    from trifocal_pose_estimation_using_improved_gpuhc_amd import (_abi, count_solutions, load_problem,
                                                                   load_ransac_data, p2c, prepare_target_params)
    from trifocal_pose_estimation_using_improved_gpuhc_amd.tracker import DeviceTracker
    arg = lambda name, default: (type(default)(sys.argv[sys.argv.index(name) + 1])   # noqa: E731
                                 if name in sys.argv else default)
    reps, n, out = arg("--reps", 12), arg("--samples", 100), arg("--out", "")
    dev = torch.device("cuda:0")
    problem = load_problem()
    tgt, dif, _ = prepare_target_params(problem, load_ransac_data(0), 0, n)
    tr = DeviceTracker(problem, dev)
    fx = os.path.join(ROOT, "tests", "golden", "p2c")
    tables = p2c.read_tables(os.path.join(fx, "dHdx_indx_P2C.txt"), os.path.join(fx, "dHdt_indx_P2C.txt"))
    cmap = p2c.derive_coeff_map(problem, *tables)
    chx, cht = (torch.from_numpy(b).to(dev) for b in p2c.coefficients(cmap, problem.start_params, dif))
    dev_tables = tr.p2c_tables(tables)
    ws_p2c = tr.new_workspace()   # its own, so neither format's launches rebuild the workspace tables in the timed span
    t, d = torch.from_numpy(tgt).to(dev), torch.from_numpy(dif).to(dev)
    s = torch.cuda.current_stream(dev)
    launches = {
        "p2c": lambda r: tr.launch_p2c(dev_tables, chx, cht, r, stream=s, workspace=ws_p2c),
        "ph": lambda r: tr.launch(t, d, r, stream=s, truncate=False, explicit_rk=True),
        "ph_codeopt": lambda r: tr.launch(t, d, r, stream=s, truncate=False),
        "headline": lambda r: tr.launch(t, d, r, stream=s),
    }
    results = {k: tr.allocate(n) for k in launches}
    ms = {k: [] for k in launches}
    for i in range(reps + 1):
        for k, go in launches.items():
            r = results[k]
            tr.reset_tracks(r)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(s)
            go(r)
            b.record(s)
            torch.cuda.synchronize(dev)
            tr.workspace_status(ws_p2c if k == "p2c" else None)
            if i:
                ms[k].append(a.elapsed_time(b))
    rec = {"build_id": _abi.build_id(), "config": 2, "dataset": 0, "seed": 0, "samples": n, "reps": reps,
           "device": torch.cuda.get_device_name(dev), "modes": {}}
    for k in launches:
        h = results[k].host()
        conv, real, inf = count_solutions(h["tracks"], h["converge"], h["infinity"])
        rec["modes"][k] = {"ms_median": round(float(np.median(ms[k])), 4), "ms_min": round(min(ms[k]), 4),
                           "ms_max": round(max(ms[k]), 4), "converged": conv, "real": real, "inf": inf,
                           "mean_steps_per_path": round(float(h["stats"]["steps"].mean()), 3)}
    med = {k: rec["modes"][k]["ms_median"] for k in launches}
    rec["improved_over_p2c"] = round(med["p2c"] / med["headline"], 3)
    rec["ratios_to_headline"] = {k: round(med[k] / med["headline"], 3) for k in launches}
    line = json.dumps(rec)
    if out:
        with open(out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
