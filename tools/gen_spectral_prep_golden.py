"""
Generate tests/golden/g12_spectral_prep.npz by running the reference's own ``smear_avg_optical_prop`` / ``avg_optical_prop``,
``smear_tuv`` and ``l_wl_planck_integ`` (``crt1d/spectra.py:42-68, 129-300, 366-390``) on its sample spectra:

    python tools/gen_spectral_prep_golden.py --reference <checkout of the reference>

Only the named functions of ``crt1d/spectra.py`` are compiled (``oracle.gen_golden.reference_functions``): the module itself imports
xarray.  Data only goes into the fixture.

cases     names; per case ``<c>`` (optics grid x irradiance grid x edge set):
<c>_x     (nx,)       optics grid, um            <c>_y    (3, nx)   leaf_r, leaf_t, soil_r
<c>_xs    (nxs,)      irradiance grid            <c>_si   (2, nxs)  SI_dr, SI_df
<c>_edges (nb+1,)                                <c>_nsub (nb,)     the reference's default sub-bin counts
<c>_I     (2, nb)     smear_tuv(xs, SI, edges) * diff(edges)
<c>_<light>_<m>       (3, nb)  smear_avg_optical_prop of the three spectra; light in uniform, planck6000, planck3000, table
                      (table: ``lambda x: np.interp(x, xs, SI_dr + SI_df)``); m = d (default x_smear_nb) or 7
<c>_sub_<m>           (2, n)   lower / upper edge of every sub-bin, bands in order (the reference's linspace)
<c>_planck_<m>        (2, n)   l_wl_planck_integ(T, lower, upper) at T = 6000, 3000 (QUADPACK)
nan_cases             the cases whose edge set reaches outside the data on purpose (the only ones that may hold NaN)
"""

import argparse
import math
import os
import sys
import warnings
from pathlib import Path

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

NAMES = ["avg_optical_prop", "smear_avg_optical_prop", "smear_tuv", "_smear_tuv_1", "_x_frac_in_bounds", "l_wl_planck",
         "l_wl_planck_integ", "BAND_DEFNS_UM"]
LIGHTS = ("uniform", "planck6000", "planck3000", "table")
MODES = (("d", None), ("7", 7))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference (the directory that holds crt1d/)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g12_spectral_prep.npz"))
    args = ap.parse_args()
    from scipy.constants import N_A, c, h
    from scipy.constants import k as k_B
    from scipy.integrate import quad

    from oracle import gen_golden as gg

    gg.REF = Path(args.reference)
    ref = gg.reference_functions("crt1d/spectra.py", NAMES, extra=dict(math=math, quad=quad, h=h, c=c, k_B=k_B, N_A=N_A))
    data = Path(args.reference) / "crt1d" / "data"
    wl_nm, r, t = np.loadtxt(data / "PROSPECT_sample.txt", unpack=True)
    soil_dry, _ = np.loadtxt(data / "PROSAIL_sample-soil.txt", unpack=True)
    x_ps5 = wl_nm / 1000.0
    y_ps5 = np.stack([r, t, soil_dry])
    x_sp2, si_dr, si_df = np.loadtxt(data / "SPCTRAL2_xls_default-spectrum.csv", delimiter=",", skiprows=1, unpack=True)
    si_sp2 = np.stack([si_dr, si_df])

    rng = np.random.default_rng(12)
    x9 = np.array([1.0, 1.05, 1.2, 1.25, 1.4, 1.6, 1.65, 1.9, 2.0])
    cases = {
        "parnir": (x_ps5, y_ps5, x_sp2, si_sp2, np.array([0.4, 0.7, 2.5])),
        "sp2": (x_ps5, y_ps5, x_sp2, si_sp2, x_sp2[(x_sp2 >= 0.4) & (x_sp2 <= 2.5)]),
        "odd": (x_ps5, y_ps5, x_sp2, si_sp2, np.array([0.4, 0.4037, 0.55, 0.7000001, 1.3, 2.4999])),
        "outside": (x_ps5, y_ps5, x_sp2, si_sp2, np.array([0.35, 0.45, 1.0, 2.45, 2.7])),
        "nx2": (np.array([0.5, 1.5]), rng.uniform(0.05, 0.6, (3, 2)), np.array([0.4, 1.6]), rng.uniform(10, 900, (2, 2)),
                np.array([0.6, 0.9, 1.4])),
        "nx5": (np.array([0.4, 0.41, 0.5, 0.7, 0.75]), rng.uniform(0.05, 0.6, (3, 5)), np.array([0.3, 0.45, 0.6, 1.0]),
                rng.uniform(10, 900, (2, 4)), np.array([0.405, 0.72])),
        # light table zero below 0.8: the first band has zero total weight under it (NaN in the reference), and reaches below x
        "nx9": (x9, rng.uniform(0.05, 0.6, (3, 9)), np.array([0.5, 0.8, 1.2, 2.5]), np.array([[0.0, 0.0, 300.0, 100.0], [0.0, 0.0, 100.0, 200.0]]),
                np.array([0.55, 0.75, 1.1, 1.9, 2.2])),
    }
    out = dict(cases=np.array(list(cases)), nan_cases=np.array(["outside", "nx9"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # 0 / 0 under the table light of nx9, by design
        for name, (x, y, xs, si, edges) in cases.items():
            edges = np.asarray(edges, dtype=np.float64)
            out.update({f"{name}_x": x, f"{name}_y": y, f"{name}_xs": xs, f"{name}_si": si, f"{name}_edges": edges})
            dx_smear = max(np.diff(x).min(), 5e-3)
            nsub_d = np.array([math.ceil((b1 - b0) / dx_smear) for b0, b1 in zip(edges[:-1], edges[1:])])
            out[f"{name}_nsub"] = nsub_d
            out[f"{name}_I"] = np.stack([ref["smear_tuv"](xs, s, edges) * np.diff(edges) for s in si])
            table = lambda xm, xs=xs, si=si: np.interp(xm, xs, si[0] + si[1])  # noqa: E731
            for m, nbm in MODES:
                kws = dict(uniform=dict(light="uniform"), planck6000=dict(light="planck", T_K=6000), planck3000=dict(light="planck", T_K=3000),
                           table=dict(light=table))
                for light in LIGHTS:
                    out[f"{name}_{light}_{m}"] = np.stack([ref["smear_avg_optical_prop"](x, yy, edges, x_smear_nb=nbm, **kws[light]) for yy in y])
                sub = [np.linspace(b0, b1, (nbm or n) + 1) for b0, b1, n in zip(edges[:-1], edges[1:], nsub_d)]
                lo, hi = np.concatenate([s[:-1] for s in sub]), np.concatenate([s[1:] for s in sub])
                out[f"{name}_sub_{m}"] = np.stack([lo, hi])
                out[f"{name}_planck_{m}"] = np.array([[ref["l_wl_planck_integ"](T, a, b) for a, b in zip(lo, hi)] for T in (6000, 3000)])
            print(f"{name}: nx = {x.size}, nb = {edges.size - 1}, sub-bins = {nsub_d.sum()} (default), NaN in table_d: "
                  f"{int(np.isnan(out[f'{name}_table_d']).sum())}")
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes")


if __name__ == "__main__":
    main()
