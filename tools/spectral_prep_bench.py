"""
Time ``Bands.from_spectra`` (one fused launch, k_spectral_prep) against the best composition the library offered before it for the same
five arrays: ``smear_tuv_batched`` on the concatenated sub-edges of every band, torch for the light weights and the per-band sums, and
``smear_tuv_batched`` x ``dwl`` for the irradiance.

    python tools/spectral_prep_bench.py [--ncol 10000] [--out profiles/spectral_prep/spectral_prep_bench.json]

Shapes: ncol columns of per-column leaf_r / leaf_t / soil_r on the 2101-point 1 nm grid and per-column SI_dr / SI_df on a 122-point grid
(1e4 columns: 524 MB of inputs, twice the 256 MB Infinity Cache), to 107 bands and to 2 bands (PAR / NIR), light = the column's own
SI_dr + SI_df.  Timing: HIP events around each call, 2 warm-up calls, then ``--blocks`` blocks in which the two sides alternate,
``--reps`` calls each; the figure is the median over the blocks of the block mean.  Both sides must give the same arrays to 1e-12
relative (the composition sums in another order); the bench asserts it.  The read rate is the compulsory traffic,
8 (3 nx + 2 nxs) + 40 nb bytes per column, over the fused time.
"""

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crt1d_amd import batched  # noqa: E402
from crt1d_amd import spectra as sp  # noqa: E402

NAMES = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")


def inputs(ncol, nx, nxs, dev, seed=5):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = np.linspace(0.4, 2.5, nx)
    xs = np.concatenate([np.linspace(0.3, 0.4, 5, endpoint=False), np.linspace(0.4, 4.0, nxs - 5)])
    smooth = torch.as_tensor(0.25 + 0.2 * np.sin(7 * x), device=dev)
    opt = [(smooth * (0.2 + 0.8 * torch.rand((ncol, 1), generator=g, device=dev, dtype=torch.float64))
            + 0.02 * torch.rand((ncol, nx), generator=g, device=dev, dtype=torch.float64)).contiguous() for _ in range(3)]
    si = [(50.0 + 900.0 * torch.rand((ncol, nxs), generator=g, device=dev, dtype=torch.float64)).contiguous() for _ in range(2)]
    return x, xs, opt, si


class Composition:
    """What a user of the previous library would write: everything that does not depend on the spectra is prepared once."""

    def __init__(self, x, xs, edges, dev):
        counts = sp.sub_bin_counts(x, edges)
        sub = [np.linspace(b0, b1, n + 1) for b0, b1, n in zip(edges[:-1], edges[1:], counts)]
        self.bins = torch.as_tensor(np.concatenate([s[:-1] for s in sub] + [edges[-1:]]), device=dev)
        lo, hi = self.bins[:-1], self.bins[1:]
        self.width = hi - lo
        mid = (lo + hi) / 2
        self.xs = torch.as_tensor(xs, device=dev)
        self.j = (torch.searchsorted(self.xs, mid, right=True) - 1).clamp(0, len(xs) - 2)
        self.t = ((mid - self.xs[self.j]) / (self.xs[self.j + 1] - self.xs[self.j])).clamp(0.0, 1.0)
        seg = np.repeat(np.arange(len(counts)), counts)
        self.S = torch.zeros((len(seg), len(counts)), dtype=torch.float64, device=dev)
        self.S[torch.arange(len(seg)), torch.as_tensor(seg)] = 1.0
        self.x = torch.as_tensor(x, device=dev)
        self.edges = torch.as_tensor(edges, device=dev)
        self.dwl = self.edges[1:] - self.edges[:-1]

    def __call__(self, opt, si):
        light = si[0] + si[1]
        lw = light[:, self.j] + (light[:, self.j + 1] - light[:, self.j]) * self.t
        w = lw * self.width
        den = w @ self.S
        out = [sp.smear_tuv_batched(self.xs, s, self.edges) * self.dwl for s in si]
        for y in opt:
            out.append(((sp.smear_tuv_batched(self.x, y, self.bins) * w) @ self.S) / den)
        return out


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps  # ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ncol", type=int, default=10000)
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    nx, nxs = 2101, 122
    x, xs, opt, si = inputs(args.ncol, nx, nxs, dev)
    results = dict(ncol=args.ncol, nx=nx, nxs=nxs, input_bytes=8 * args.ncol * (3 * nx + 2 * nxs), blocks=args.blocks, reps=args.reps,
                   device=torch.cuda.get_device_name(0), cases=[])
    edge_sets = {"107 bands": np.concatenate([np.linspace(0.4, 0.9, 76), np.linspace(0.9, 2.5, 33)[1:]]), "2 bands (PAR, NIR)": np.array([0.4, 0.7, 2.5])}
    for label, edges in edge_sets.items():
        nb = edges.size - 1
        comp = Composition(x, xs, edges, dev)
        fused = lambda: batched.Bands.from_spectra(x, *opt, xs, *si, edges, light="table")  # noqa: E731
        composed = lambda: comp(opt, si)  # noqa: E731
        b, c = fused(), composed()
        torch.cuda.synchronize()
        worst = 0.0
        for k, ref in zip(NAMES, c):
            got = getattr(b, k)
            worst = max(worst, float(((got - ref).abs() / ref.abs()).max()))
        assert worst <= 1e-12, (label, worst)
        del b, c
        for _ in range(2):
            fused(), composed()
        torch.cuda.synchronize()
        tf, tc = [], []
        for _ in range(args.blocks):
            tf.append(timed(fused, args.reps))
            tc.append(timed(composed, args.reps))
        tf_ms, tc_ms = float(np.median(tf)), float(np.median(tc))
        compulsory = args.ncol * (8 * (3 * nx + 2 * nxs) + 40 * nb)
        case = dict(case=label, nb=nb, sub_bins=int(sp.sub_bin_counts(x, edges).sum()), fused_ms=tf_ms, composed_ms=tc_ms,
                    fused_ms_blocks=[round(t, 4) for t in tf], composed_ms_blocks=[round(t, 4) for t in tc], speedup=tc_ms / tf_ms,
                    fused_is_faster=bool(tf_ms < tc_ms), compulsory_bytes=compulsory, fused_read_rate_GBps=compulsory / tf_ms / 1e6,
                    worst_rel_diff_fused_vs_composed=worst)
        print(json.dumps(case))
        results["cases"].append(case)
    results["note"] = ("fused_ms includes the host side of Bands.from_spectra (sub-bin counts, five torch.empty, one launch); "
                       "composed_ms the eleven launches of the composition with everything spectrum-independent prepared beforehand")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
