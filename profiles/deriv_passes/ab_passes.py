"""This tree's library against the parent commit's on the closed-form derivative entries: the fused side of the
project's five benchmarks -- tools/dlai_bench.py run_dlai, tools/dleaf_bench.py run_dleaf, tools/grad_bench.py run_grad,
profiles/sensjac/sensjac_bench.py run_fused, profiles/sensjac_series/sensjac_series_bench.py run_series -- at their own shapes, blocks and
repetitions, schemes 2s, bl, g77, bf.  One child process per run, this tree's package in all of them, the library named by
CRT1D_HIP_LIB: parent, new, parent, new, ... (--rounds of each).  The runs of the parent's library against each other give the noise
band of every case: "slower" / "faster" is a case whose median over the runs of the new library lies outside [min, max] of the parent's runs.

    python profiles/deriv_passes/ab_passes.py --parent-lib <libcrt1d_hip.so of the parent commit> [--rounds 3] [--json ab_passes.json]
        [--new-lib <another build of this tree>] [--benches dlai,dleaf,grad,sensjac,sensjac_series] [--schemes 2s,bl,g77,bf]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "profiles", "sensjac"), os.path.join(ROOT, "profiles", "sensjac_series")]

# (module, function, time key, its main()'s defaults)
BENCHES = [("dlai_bench", "run_dlai", "dlai_ms", dict(shapes="10000x300x60,4000x107x60", blocks=21, reps=10)),
           ("dleaf_bench", "run_dleaf", "dleaf_ms", dict(shapes="10000x300x60,4000x107x60", blocks=21, reps=10)),
           ("grad_bench", "run_grad", "grad_ms", dict(shapes="10000x300x60,4000x107x60", blocks=21, reps=10)),
           ("sensjac_bench", "run_fused", "fused_ms", dict(shapes="10000x300x60,2000x2151x60", blocks=7, reps=10)),
           ("sensjac_series_bench", "run_series", "series_ms", dict(shapes="10000x300x60,2000x2151x60", nt="8,24", blocks=7, reps=5))]


def child(args):
    import importlib

    out = {}
    for mod, fn, key, kw in BENCHES:
        if mod[:-6] not in args.benches.split(","):
            continue
        rows = getattr(importlib.import_module(mod), fn)(argparse.Namespace(schemes=args.schemes, **kw))
        for r in rows:
            name = f"{mod[:-6]} {r['scheme']} {r['columns']} {'x'.join(map(str, r['shape']))}" + (f" nt={r['nt']}" if "nt" in r else "")
            out[name] = r[key]
    json.dump(out, sys.stdout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "crt1d_amd", "libcrt1d_hip.so"))
    ap.add_argument("--benches", default="dlai,dleaf,grad,sensjac,sensjac_series")
    ap.add_argument("--schemes", default="2s,bl,g77,bf")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = {"parent": [], "new": []}
    for i in range(args.rounds):
        for who, lib in (("parent", os.path.abspath(args.parent_lib)), ("new", os.path.abspath(args.new_lib))):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-lib", lib, "--child", "--benches", args.benches, "--schemes", args.schemes],
                               env=dict(os.environ, CRT1D_HIP_LIB=lib),
                               stdout=subprocess.PIPE, check=True, timeout=600)
            runs[who].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
            print(f"round {i} {who} done", flush=True)
    rows, slow = [], 0
    for name in runs["parent"][0]:
        p, n = [r[name] for r in runs["parent"]], [r[name] for r in runs["new"]]
        m = statistics.median(n)
        verdict = "slower" if m > max(p) else "faster" if m < min(p) else "inside"
        slow += verdict == "slower"
        rows.append({"case": name, "parent_ms": p, "new_ms": n, "verdict": verdict})
        print(f"{name:52s} parent {' '.join(f'{v:8.4f}' for v in p)} (spread {100 * (max(p) / min(p) - 1):4.2f} %)  new {' '.join(f'{v:8.4f}' for v in n)}  {verdict}",
              flush=True)
    print(f"{len(rows)} cases, {slow} with the new library's median above every run of the parent's")
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"rounds": args.rounds, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
