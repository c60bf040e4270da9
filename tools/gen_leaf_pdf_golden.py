"""
Generate tests/golden/g11_leaf_pdf.npz by running the reference's own leaf-inclination PDFs and ``mla_from_g``
(``crt1d/leaf_angle.py:31-87``):

    python tools/gen_leaf_pdf_golden.py --reference <checkout of the reference>

theta     (50,)    leaf inclinations in [0, pi/2], both ends included
names     (5,)     the parameter-free PDFs: spherical, uniform, planophile, erectophile, plagiophile
g         (5, 50)  g_<name>(theta)
mla       (5,)     mla_from_g(g_<name>), degrees (scipy.integrate.quad at its default tolerance)
x         (3,)     0.3, 1, 2.5
g_ell     (3, 50)  g_ellipsoidal(theta, x)
mla_ell   (3,)     mla_from_g(lambda t: g_ellipsoidal(t, x))

Only the module ``crt1d/leaf_angle.py`` is loaded (NumPy and SciPy), not the package.
"""

import argparse
import importlib.util
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("spherical", "uniform", "planophile", "erectophile", "plagiophile")
X = (0.3, 1.0, 2.5)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference (the directory that holds crt1d/)")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "g11_leaf_pdf.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_leaf_angle", os.path.join(args.reference, "crt1d", "leaf_angle.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    theta = np.linspace(0.0, np.pi / 2, 50)
    fns = [getattr(ref, "g_" + n) for n in NAMES]
    g = np.stack([np.asarray(f(theta), dtype=np.float64) for f in fns])
    mla = np.array([ref.mla_from_g(f) for f in fns])
    g_ell = np.stack([ref.g_ellipsoidal(theta, x) for x in X])
    mla_ell = np.array([ref.mla_from_g(lambda t, x=x: ref.g_ellipsoidal(t, x)) for x in X])
    np.savez(args.out, theta=theta, names=np.array(NAMES), g=g, mla=mla, x=np.array(X), g_ell=g_ell, mla_ell=mla_ell)
    print(f"wrote {args.out}: mla = {dict(zip(NAMES, mla.round(6)))}, mla_ell = {dict(zip(X, mla_ell.round(6)))}")


if __name__ == "__main__":
    main()
