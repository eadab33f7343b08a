"""Does a W.x launch whose weights are requested with the default cache policy run shorter than the same launch on the nontemporal
stream?  From a rocprofv3 kernel trace of ONE run whose budget splits a family (run on the GPU box):
    GTEN_HIP_RESIDENT_MB=204 rocprofv3 --kernel-trace --output-format csv -d DIR -- python3 bench.py --fill prefill --brief
    python3 tools/resident_trace.py DIR [steps] > resident_trace.json
Groups the k_dec_gemv8 dispatches of the last `steps` decode steps (default 64: the timed ones) by family and by the kernel's last
template argument (WLD: 0 nontemporal, 1 default policy) and prints, per group, count, mean, median, standard deviation and the
10 / 90 % points of the dispatch durations, in ns.  The same kernel, the same run, the same step: only the load policy differs.
A profiled run: every launch is slower than in the graph replay; the DIFFERENCE between the two groups of a family is what this is
for."""
import csv
import glob
import json
import os
import statistics
import sys
from collections import defaultdict

PRO = {0: "embed", 1: "resid", 2: "att", 3: "attw", 4: "actq8"}


def family(args):
    """the step's family of a k_dec_gemv8 instantiation <WT, PRO, NCH, R, EPI, NT, NM, WLD>; None: a staging launch"""
    pro, r, epi, nm = args[1], args[3], args[4], args[6]
    if epi == 1:
        return "gate|up"
    if epi != 0:
        return None
    if pro in (2, 3):
        return "o"
    if pro == 4:
        return "down"
    if nm == 1:
        return "lm_head"
    return "q|k|v"


def main():
    d = sys.argv[1]
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    assert files, "no kernel_trace.csv under " + d
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            name = r["Kernel_Name"]
            if "k_dec_gemv8<" not in name:
                continue
            args = [int(x) for x in name.split("k_dec_gemv8<")[1].split(">")[0].split(",")]
            if len(args) != 8:
                continue
            fam = family(args)
            if fam:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), fam, args[7]))
    rows.sort()
    heads = [i for i, r in enumerate(rows) if r[2] == "lm_head"]
    assert len(heads) > steps, f"only {len(heads)} decode steps in the trace"
    win = rows[heads[-steps - 1] + 1:heads[-1] + 1]          # the last `steps` steps, each ending with its lm_head
    groups = defaultdict(list)
    for s, e, fam, wld in win:
        groups[(fam, wld)].append(e - s)
    out = {"steps": steps, "dispatches": len(win), "groups": []}
    for (fam, wld), v in sorted(groups.items()):
        v.sort()
        out["groups"].append({"family": fam, "policy": "default" if wld else "nontemporal", "n": len(v), "mean_ns": round(statistics.fmean(v), 1),
                              "median_ns": v[len(v) // 2], "stdev_ns": round(statistics.pstdev(v), 1), "p10_ns": v[len(v) // 10], "p90_ns": v[len(v) * 9 // 10]})
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
