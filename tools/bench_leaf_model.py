#!/usr/bin/env python
"""What the plate leaf model costs, one JSON line per run.

  tools/bench_leaf_model.py --mode model [--tree DIR]    k_plate_leaf alone, and step() of a SpectralRetrievalPlan with leaf_model=
                                                         (nm = 6, one soil direction, ln LAI, the leaf angle)
  tools/bench_leaf_model.py --mode fixed [--tree DIR]    step() of the same plan with six FIXED per-column leaf directions of the same
                                                         ntan instead: what a tree without the leaf model runs (--tree: the tree whose
                                                         crt1d_amd and library are measured, default this one)

Shapes: 1e4 x 300 x 60 and 2e3 x 2151 x 60, 2s and bl (bl has no soil: ntan = 6).  Times are HIP events around blocks of calls on one
stream after a warm-up, the median block; bytes are the (2 + 2 nm) doubles k_plate_leaf writes per (column, band)."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["model", "fixed"], required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch

    from crt1d_amd import batched, synth

    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    NABS, NM, NZ = 5, 6, 60

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize(dev)
        ms = []
        for _ in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(n):
                fn()
            e1.record(stream)
            torch.cuda.synchronize(dev)
            ms.append(e0.elapsed_time(e1) / n)
        ms.sort()
        return {"ms_median": ms[len(ms) // 2], "ms_min": ms[0], "ms_max": ms[-1], "calls_per_block": n, "blocks": a.blocks}

    def spectra(nb):
        wl = np.linspace(0.4, 2.5, nb)
        g = lambda c, w: np.exp(-0.5 * ((wl - c) / w) ** 2)  # noqa: E731
        K = np.stack([0.06 * g(0.45, 0.08) + 0.05 * g(0.67, 0.03), 0.04 * g(0.5, 0.1), 40 * g(1.45, 0.06) + 60 * g(1.94, 0.07) + 0.5 * g(0.97, 0.04),
                      8 + 30 * g(2.2, 0.3), 5 + 10 * g(1.7, 0.2)])
        return K, 1.5 - 0.06 * (wl - 0.4) / 2.1

    def q0(ncol, rng):
        return np.stack([rng.uniform(1.2, 2.2, ncol), rng.uniform(25, 60, ncol), rng.uniform(5, 20, ncol), rng.uniform(0.008, 0.02, ncol),
                         rng.uniform(0.003, 0.01, ncol), rng.uniform(0.001, 0.004, ncol)], axis=1)

    out = {"mode": a.mode, "label": a.label, "tree": os.path.abspath(a.tree), "device": torch.cuda.get_device_name(dev), "kernel": [], "step": []}
    for ncol, nb in ((10000, 300), (2000, 2151)):
        rng = np.random.default_rng(11)
        K, n = spectra(nb)
        q = torch.as_tensor(q0(ncol, rng)).to(dev)
        if a.mode == "model":
            from crt1d_amd.leaf_model import PlateLeafModel

            model = PlateLeafModel(K, n)
            o = {k: torch.empty(s, dtype=torch.float64, device=dev) for k, s in (("leaf_r", (ncol, nb)), ("leaf_t", (ncol, nb)),
                                                                                 ("d_leaf_r", (ncol, NM, nb)), ("d_leaf_t", (ncol, NM, nb)))}
            for partials in (True, False):
                t = timed(lambda: batched.plate_leaf_optics(model, q, partials=partials, out=o), 50)
                nbytes = (2 + 2 * NM * partials) * 8 * ncol * nb
                t.update(ncol=ncol, nb=nb, nm=NM, partials=partials, bytes_written=nbytes, GBs_written=nbytes / (t["ms_median"] * 1e-3) / 1e9)
                out["kernel"].append(t)
        d = synth.make_columns(ncol, nb, NZ, seed=5)
        cols, bands = batched.Columns.from_host(d, dev), batched.Bands.from_host(d, dev)
        for scheme in ("2s", "bl"):
            soil = scheme != "bl"
            b = bands if soil else batched.Bands(bands.I_dr0, bands.I_df0, bands.leaf_r, bands.leaf_t, None)
            ntan = NM + soil
            y = {"I_df_d": torch.full((ncol, 1, nb), 0.5, dtype=torch.float64, device=dev)}
            p0 = np.concatenate([q0(ncol, rng)] + ([np.zeros((ncol, 1))] if soil else []) + [np.zeros((ncol, 1)), d["g_param"][:, None]], axis=1)
            lo = np.array([1.0] + [0.0] * NABS + [-1.0] * soil + [-2.0, 0.2])
            hi = np.array([4.0] + [1e3] * NABS + [1.0] * soil + [2.0, 5.0])
            kw = dict(keys=("I_df_d",), lai=True, leaf=True, lo=lo, hi=hi)
            sd = torch.as_tensor(0.1 * d["soil_r"].mean(axis=0)[None]).to(dev)
            if a.mode == "model":
                if soil:
                    kw["d_soil_r"] = sd
                plan = batched.SpectralRetrievalPlan(scheme, cols, b, (0,), y, leaf_model=model, p0=p0, **kw)
            else:  # six fixed per-column leaf directions in rows 0..5 of ntan rows; the soil direction in the last row
                dl = torch.zeros((2, ncol, ntan, nb), dtype=torch.float64, device=dev)
                dl[:, :, :NM] = 1e-3 * torch.rand((2, ncol, NM, nb), dtype=torch.float64, device=dev)
                kw.update(d_leaf_r=dl[0], d_leaf_t=dl[1])
                if soil:
                    ds = torch.zeros((ncol, ntan, nb), dtype=torch.float64, device=dev)
                    ds[:, NM] = sd
                    kw["d_soil_r"] = ds
                p0f = p0.copy()
                p0f[:, :NM] = 0.0
                lo[:NM], hi[:NM] = -1.0, 1.0
                plan = batched.SpectralRetrievalPlan(scheme, cols, b, (0,), y, p0=p0f, **kw)
            t = timed(lambda: plan.step(), a.steps)
            torch.cuda.synchronize(dev)
            t.update(scheme=scheme, ncol=ncol, nb=nb, nz=NZ, npar=plan.npar, ntan=ntan, params=list(plan.params),
                     direction_bytes=3 * ncol * ntan * nb * 8 if soil else 2 * ncol * ntan * nb * 8,
                     finite_cost=bool(torch.isfinite(plan.cost).all()))
            out["step"].append(t)
            del plan
        del cols, bands
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
