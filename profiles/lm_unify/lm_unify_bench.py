"""The chain entries before and after they launch the shared-parameter kernels (DESIGN sections 3.28 / 3.29): the `kernels` and `step`
sections of profiles/lm_chain/lm_chain_bench.py, run twice on a tree, with the min .. max of the 7 blocks kept next to every median.

    python profiles/lm_unify/lm_unify_bench.py --tree . --label this_tree                    # one process per tree: it imports the
    python profiles/lm_unify/lm_unify_bench.py --tree variants/parent --label parent         # tree's own package, harness and library
    python profiles/lm_unify/lm_unify_bench.py --compare [--label this_tree]

The parent's tree is a copy of the parent commit kept out of git with its own library built in it.  --compare adds the verdicts: a
figure of the labelled tree (the mean of its two medians) may exceed the parent's by no more than the parent's spread, the larger of its
two runs' block ranges.  Held to that: crt_hip_lm_step_chain_f64 and crt_hip_lm_chain_covariance_f64 alone, and step() of the chained
plans.  lm_unify_bench.json: the parent and this tree, one session.  lm_unify_bench_template.json: the parent and a copy of this tree
with the `template <bool kBorder>` attempt of DESIGN 3.29 (--label template_attempt), a second session; that attempt is not in the tree.
"""
import argparse
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HELD_KERNELS = ("step_chain_ms", "covariance_ms")
HELD_STEPS = ("chained_step_ms",)


def measure(tree, blocks):
    import statistics

    import torch

    tree = os.path.abspath(tree)
    sys.path[:0] = [tree, os.path.join(tree, "tools")]
    spec = importlib.util.spec_from_file_location("lm_chain_bench", os.path.join(tree, "profiles", "lm_chain", "lm_chain_bench.py"))
    B = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(B)
    assert os.path.dirname(os.path.abspath(B._lib.LIB_PATH)) == os.path.join(tree, "crt1d_amd"), B._lib.LIB_PATH

    class Timed(float):  # the median, with the range of the blocks it is the median of
        lo = hi = None

    def timed(fn, blocks, reps):  # tools/levels_bench.timed, keeping every block
        st = torch.cuda.current_stream()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for _ in range(reps):
                fn()
            e1.record(st)
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) / reps)
        t = Timed(statistics.median(out))
        t.lo, t.hi = min(out), max(out)
        return t

    B.timed = timed

    def ranges(r):
        r.update({k + "_range": [v.lo, v.hi] for k, v in list(r.items()) if isinstance(v, Timed)})
        return r

    runs = []
    for _ in range(2):
        run = dict(kernels=[], steps=[])
        for nd in (12, 36):
            for npar in (5, 10):
                run["kernels"].append(ranges(B.kernels_case(10_000, nd, npar, blocks)))
                print(json.dumps(run["kernels"][-1]), flush=True)
        for scheme in ("2s", "bl"):
            for spectral in (False, True):
                run["steps"].append(ranges(B.step_case(scheme, spectral, 10_000, 12, blocks)))
                print(json.dumps(run["steps"][-1]), flush=True)
        runs.append(run)
    return dict(device=torch.cuda.get_device_name(0), blocks=blocks, runs=runs)


def compare(out, label):
    verdicts = []
    for section, keys in (("kernels", HELD_KERNELS), ("steps", HELD_STEPS)):
        for i, case in enumerate(out["parent"]["runs"][0][section]):
            for k in keys:
                par = [run[section][i] for run in out["parent"]["runs"]]
                new = [run[section][i] for run in out[label]["runs"]]
                spread = max(r[k + "_range"][1] - r[k + "_range"][0] for r in par)
                p, n = sum(r[k] for r in par) / 2, sum(r[k] for r in new) / 2
                name = {j: case[j] for j in ("nd", "npar", "scheme", "plan") if j in case}
                verdicts.append(dict(case=name, figure=k, parent_ms=[r[k] for r in par], **{label + "_ms": [r[k] for r in new]}, parent_spread_ms=spread,
                                     over_parent=n / p, within_spread=bool(n - p <= spread)))
    out["held_to_the_parent"] = verdicts
    return all(v["within_spread"] for v in verdicts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=None)
    ap.add_argument("--label", default="this_tree", help="this_tree, parent, or the name of another build that is held against the parent")
    ap.add_argument("--compare", action="store_true", help="add the verdicts of --label against the parent")
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--json", default=os.path.join(HERE, "lm_unify_bench.json"))
    args = ap.parse_args()
    out = json.load(open(args.json)) if os.path.exists(args.json) else {}
    ok = True
    if args.compare:
        ok = compare(out, args.label)
        for v in out["held_to_the_parent"]:
            print(json.dumps(v))
    else:
        out[args.label] = measure(args.tree, args.blocks)
    with open(args.json, "w") as fh:
        json.dump(out, fh, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
