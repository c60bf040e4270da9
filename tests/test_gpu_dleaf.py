"""GPU: the derivative of the level spectra along a leaf-angle direction (crt_hip_levels_dleaf_f64, batched.LevelsDleafPlan): against the
Richardson-extrapolated central differences of the oracle in g_param (and in mla, and in the `a` of a trigonometric leaf PDF), exact
identities of the schemes, crt_hip_g_dparam_f64 against differences of leaf_angle.eval_G, CRT_G_TABLE columns, bitwise invariants (batch,
levels, keys, flags, shared spectra, graph replay) and the Python surface.

The synthetic columns of tests/test_gpu_jac.py are overridden to each of the three parametric kinds: exact ellipsoidal and
ellipsoidal-approx with the generator's x, Bonan with chi_l drawn in (-0.35, 0.55).

Measured on MI355X (each test prints its figures with -s).  Against the oracle, worst |J - J_ref| / scale per scheme over the three kinds
(bound 1e-6), next to the reference's own h against h / 2 guard (bound 1e-7): 2s 8.7e-9 (guard 1.3e-8), bl 3.9e-10 (3.7e-10), g77 1.2e-10
(2.1e-10), bf 4.2e-10 (5.5e-9), n79 1.1e-9 (1.5e-9), zq 1.6e-9 (3.1e-9); the deep shapes (32- and 16-lane slices) n79 3.0e-9 (1.5e-8), zq
5.6e-9 (2.5e-8); n79 with tau_d_method '9sky' 1.9e-9 (3.0e-9); 2s with dmla alone 1.6e-8 (1.9e-8); wrt="mla" 2.3e-10 (2.7e-10); the
trigonometric PDF along `a` 3.1e-9 (bl) .. 8.3e-9 (2s), each a few percent above its guard (3.0e-9 .. 7.8e-9) -- the differences are the
reference's.  Identities, worst residual / scale (bound 1e-11): I_dr' = -K_b' L I_dr 5.2e-16 relative (bound 1e-13); F' = I_dr' / mu +
2 (dn' + up') 3.4e-16; ground condition 3.3e-16 (2s), 2.6e-16 (bf), 6.3e-17 (n79), 1.0e-16 (zq); I_df_d'[nz-1] 2.1e-15 (2s), 0 (bl, bf,
n79); bl's I_df_u' zero; twice the tangent gives twice every bit, no tangent gives zeros.  crt_hip_g_dparam_f64 against the differences of
eval_G: 3.3e-12 of max |dG| (bound 1e-9); 1 -+ 1e-7 against 1: 2.9e-8 (bound 1e-6).  CRT_G_TABLE columns against their closed forms:
5.1e-15 of scale (2s; bound 1e-12).  tau_d^th on the device against the host rule: 4.3e-16 ('quad'), 3.5e-16 ('9sky') of the sum of
magnitudes (bound 1e-15).  sensor_dleaf against the NumPy contraction: 8.8e-16 of the weighted scale (bound 1e-13)."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_jac import DEEP_SHAPES, SHAPES, _host, _levels

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
TRI = ("n79", "zq")
KINDS = {"ellipsoidal": 3, "approx": 4, "bonan": 5}  # crt_g_kind
H = 3e-3  # relative step in x, absolute step in chi_l
REF_GUARD, BOUND = 1e-7, 1e-6


def _lanes(scheme, nz):
    """Lanes per workgroup of k_dlai_tri (include/crt1d_hip_dlai.h)."""
    whole, half = (292, 536) if scheme == "n79" else (307, 599)
    return 64 if nz <= whole else 32 if nz <= half else 16


@functools.lru_cache(maxsize=None)
def _host_kind(shape, uniform, kind):
    """The generator's columns with every column's leaf-angle class set to ``kind``."""
    d = dict(_host(shape, uniform))
    d["g_kind"] = np.full(shape[0], KINDS[kind], dtype=np.int32)
    if kind == "bonan":
        d["g_param"] = np.random.default_rng(5).uniform(-0.35, 0.55, shape[0])
    return d


@functools.lru_cache(maxsize=None)
def _device_kind(shape, uniform, kind):
    import torch

    from crt1d_amd import batched

    d = _host_kind(shape, uniform, kind)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    torch.cuda.synchronize()
    return cols, bands, tan


def _richardson(f, h):
    """(J, J2): (4 D(h/2) - D(h)) / 3 of the central differences D of ``f(delta) -> {key: array}``, at h and at h / 2."""
    def D(h):
        hi, lo = f(h), f(-h)
        return {k: (hi[k] - lo[k]) / (2 * h) for k in hi}

    d1, d2, d4 = D(h), D(h / 2), D(h / 4)
    return {k: (4 * d2[k] - d1[k]) / 3 for k in d1}, {k: (4 * d4[k] - d2[k]) / 3 for k in d1}


def _scale(J):
    return np.max(np.stack([np.abs(J[k]) for k in KEYS]), axis=(0, 2), keepdims=True)[0]


def _oracle_f(scheme, d, lev, method="quad", **fixed):
    """f(cols_kw) -> the oracle's level spectra {key: (ncol, nsel, nb)} for oracle.Columns(psi, lai, **cols_kw)."""
    from oracle import crt_oracle as O

    names = ("I_dr0", "I_df0", "leaf_r", "leaf_t") + (() if scheme == "bl" else ("soil_r",))
    kw = {k: d[k] for k in names}
    if method != "quad":
        assert scheme == "n79"
        kw["tau_d_method"] = method
    solve = getattr(O, f"solve_{scheme}")

    def f(**cols_kw):
        out = solve(O.Columns(d["psi"], d["lai"], **{**fixed, **cols_kw}), **kw)
        return {k: out[k][:, lev, :] for k in KEYS}

    return f


@functools.lru_cache(maxsize=None)
def _reference(scheme, shape, uniform, kind, method="quad"):
    """(J_ref, J_ref2, scale): the Richardson-extrapolated central difference of the oracle in g_param -- x (1 +- h) divided by x h, or
    chi_l +- h -- at h = H and at H / 2, each {key: (ncol, nsel, nb)}, and scale (ncol, 1, nb) = max |J_ref| over the levels and the four
    quantities.  mla is fixed."""
    d = _host_kind(shape, uniform, kind)
    f = _oracle_f(scheme, d, list(_levels(shape[2])), method, mla=d["mla"], g_kind=d["g_kind"])
    p = d["g_param"]
    unit = np.ones_like(p) if kind == "bonan" else p  # the step of column c is delta * unit[c]
    J, J2 = _richardson(lambda delta: f(g_param=p + delta * unit), H)
    for Jx in (J, J2):
        for k in KEYS:
            Jx[k] = Jx[k] / unit[:, None, None]
    return J, J2, _scale(J)


def _cases():
    """(scheme, shape, uniform, kind, method): six schemes x three kinds x SHAPES, n79 again with '9sky', and n79 / zq ('quad') on
    DEEP_SHAPES: (2, 40, 320) runs the 32-lane slice of k_dlai_tri, (1, 20, 640) the 16-lane slice."""
    for scheme, method in [(s, "quad") for s in SCHEMES] + [("n79", "9sky")]:
        for shape in SHAPES + (DEEP_SHAPES if scheme in TRI and method == "quad" else []):
            for uniform in (True, False):
                for kind in KINDS:
                    name = f"{scheme}-{kind}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}" + ("" if method == "quad" else "-9sky")
                    yield pytest.param(scheme, shape, uniform, kind, method, id=name)


def _dleaf(scheme, cols, bands, tan, nz, **kw):
    import torch

    from crt1d_amd import batched

    plan = batched.LevelsDleafPlan(scheme, cols, bands, kw.pop("levels", _levels(nz)), tan, **kw)
    got = plan()
    torch.cuda.synchronize()
    return plan, got


def _compare(label, got, J, J2, scale):
    """Print the worst figures, then the guard of the reference and the assertion on every element."""
    den = np.where(scale == 0, 1.0, scale)
    g = {k: got[k].cpu().numpy() for k in KEYS}
    for k in KEYS:
        assert g[k].shape == J[k].shape and np.isfinite(g[k]).all(), (label, k)
    worst_ref = max(float(np.max(np.abs(J2[k] - J[k]) / den)) for k in KEYS)
    worst = max(float(np.max(np.abs(g[k] - J[k]) / den)) for k in KEYS)
    print(f"dleaf-vs-oracle {label}: {worst:.3e} of scale (reference guard {worst_ref:.3e})")
    for k in KEYS:
        assert np.all(np.abs(J2[k] - J[k]) <= REF_GUARD * scale), (label, k, "the reference does not meet its own guard", worst_ref)
        assert np.all(np.abs(g[k] - J[k]) <= BOUND * scale), (label, k, worst)


@pytest.mark.parametrize("scheme,shape,uniform,kind,method", _cases())
def test_dleaf_against_the_oracle(scheme, shape, uniform, kind, method):
    """|J - J_ref| <= 1e-6 scale for every element; the reference itself agrees with its h / 2 estimate to 1e-7 scale."""
    J, J2, scale = _reference(scheme, shape, uniform, kind, method)
    cols, bands, tan = _device_kind(shape, uniform, kind)
    plan, got = _dleaf(scheme, cols, bands, tan, shape[2], tau_d_method=method)
    assert plan.last_kernel().startswith("k_dlai_tri<" if scheme in TRI else "k_dleaf<"), plan.last_kernel()
    if scheme in TRI:
        assert plan.last_kernel().endswith(f"slice={_lanes(scheme, shape[2])}"), plan.last_kernel()
    _compare(f"{scheme}{'' if method == 'quad' else ' ' + method} {kind} {shape} {'uniform' if uniform else 'ragged'}", got, J, J2, scale)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_dmla_alone_against_the_oracle(shape, uniform):
    """2s with dmla = 1 and a zero G tangent, against the difference of the oracle in mla at fixed x: cos^2' alone.  Step: 1 degree, where
    the reference's guard is smallest on the CPU (1.9e-8; 1.6e-7 at 0.3 degrees, 7.7e-8 at 1.5): a band with leaf_r close to leaf_t hardly
    knows mla, so its scale is small next to the rounding noise of the difference."""
    import torch

    from crt1d_amd import batched

    d = _host_kind(shape, uniform, "approx")
    f = _oracle_f("2s", d, list(_levels(shape[2])), g_kind=d["g_kind"], g_param=d["g_param"])
    J, J2 = _richardson(lambda delta: f(mla=d["mla"] + delta), 1.0)
    cols, bands, tan = _device_kind(shape, uniform, "approx")
    only = batched.LeafTangent(torch.zeros_like(tan.dg_table), torch.zeros_like(tan.dg_at_psi), torch.ones_like(cols.mla))
    _, got = _dleaf("2s", cols, bands, only, shape[2])
    assert bool((got["I_dr"] == 0).all())  # the beam does not know the mean leaf angle
    _compare(f"2s dmla {shape} {'uniform' if uniform else 'ragged'}", got, J, J2, _scale(J))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_trig_pdf_along_a(scheme):
    """CRT_G_TABLE columns of LeafPDF.trig(a, b) along `a` (leaf_tangent(wrt="a"): G and mla are linear in the PDF) against the oracle
    with G_fn = LeafPDF.trig(a +- h, b) and the PDF's own mla."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.leaf_angle import PDF_TRIG, LeafPDF

    shape, uniform, a, b, h = (3, 70, 60), False, 0.3, -0.2, 0.05
    d = _host(shape, uniform)
    f = _oracle_f(scheme, d, list(_levels(shape[2])))

    def at(delta):
        pdf = LeafPDF.trig(a + delta, b)
        return f(G_fn=pdf, mla=np.full(shape[0], pdf.mla()))

    J, J2 = _richardson(at, h)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda v: torch.as_tensor(v).to(dev)  # noqa: E731
    cols = batched.Columns.from_leaf_pdf(t(d["psi"]), t(d["lai"]), torch.full((shape[0],), PDF_TRIG, dtype=torch.int32), [[a, b]] * shape[0])
    bands = batched.Bands.from_host(d)
    _, got = _dleaf(scheme, cols, bands, batched.leaf_tangent(cols, "a"), shape[2])
    _compare(f"{scheme} trig a {shape}", got, J, J2, _scale(J))


def _identity_cases():
    i = 0
    for scheme in SCHEMES:
        for shape in SHAPES + (DEEP_SHAPES if scheme in TRI else []):
            for uniform in (True, False):
                kind = list(KINDS)[i % 3]  # every scheme meets every kind
                i += 1
                yield pytest.param(scheme, shape, uniform, kind, id=f"{scheme}-{kind}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}")


@pytest.mark.parametrize("scheme,shape,uniform,kind", _identity_cases())
def test_exact_identities(scheme, shape, uniform, kind):
    import torch

    from crt1d_amd import batched

    d = _host_kind(shape, uniform, kind)
    cols, bands, tan = _device_kind(shape, uniform, kind)
    lev = _levels(shape[2])
    _, got = _dleaf(scheme, cols, bands, tan, shape[2])
    got = {k: v.clone() for k, v in got.items()}
    val = batched.solve_levels(scheme, cols, bands, lev)
    torch.cuda.synchronize()
    dI, dn, up, F = (got[k] for k in KEYS)
    dev = dn.device
    scale = torch.stack([v.abs() for v in got.values()]).amax(dim=(0, 2), keepdim=True)[0]  # (ncol, 1, nb)
    worst = {}

    def check(name, resid, sc, factor=1e-11):
        worst[name] = float((resid.abs() / sc.clamp_min(1e-300)).max())
        assert bool((resid.abs() <= factor * sc).all()), (scheme, shape, uniform, name, worst[name])

    # I_dr' = -K_b' L_j I_dr with K_b' = dG(psi_sun) / mu of the tangent and the device's I_dr: 1e-13 relative
    mu = torch.as_tensor(np.cos(d["psi"])).to(dev)
    dKb = tan.dg_at_psi / mu  # (ncol,)
    L = torch.as_tensor(d["lai"][:, list(lev)]).to(dev)  # (ncol, nsel)
    exact = -(dKb[:, None] * L)[:, :, None] * val["I_dr"]
    check("I_dr' = -K_b' L I_dr", dI - exact, exact.abs(), 1e-13)
    check("F' = I_dr'/mu + 2 (dn' + up')", F - (dI / mu[:, None, None] + 2 * (dn + up)), scale)
    assert lev[0] == 0 and lev[-1] == shape[2] - 1
    if scheme in ("2s", "bl", "bf", "n79"):  # the top value is I_df0
        check("top dn' = 0", dn[:, -1], scale[:, 0])
    if scheme in ("2s", "zq", "n79", "bf"):  # I_df_u[0] = soil_r (I_dr[0] + I_df_d[0]), differentiated
        check("ground", up[:, 0] - bands.soil_r * (dI[:, 0] + dn[:, 0]), scale[:, 0])
    if scheme == "bl":
        assert bool((up == 0).all())
    # linear in the tangent: twice the tangent, twice the output (to rounding); no tangent, zeros
    dmla = torch.ones_like(cols.mla)
    one = batched.LeafTangent(tan.dg_table, tan.dg_at_psi, dmla)
    two = batched.LeafTangent(2 * tan.dg_table, 2 * tan.dg_at_psi, 2 * dmla)
    zero = batched.LeafTangent(0 * tan.dg_table, 0 * tan.dg_at_psi, 0 * dmla)
    g1 = {k: v.clone() for k, v in _dleaf(scheme, cols, bands, one, shape[2])[1].items()}
    g2 = {k: v.clone() for k, v in _dleaf(scheme, cols, bands, two, shape[2])[1].items()}
    g0 = _dleaf(scheme, cols, bands, zero, shape[2])[1]
    for k in KEYS:
        check(f"doubling {k}", g2[k] - 2 * g1[k], scale, 1e-15)
        assert bool((g0[k] == 0).all()), (scheme, shape, k, "zero tangent")
    print(f"dleaf-identities {scheme} {kind} {shape} {'uniform' if uniform else 'ragged'}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------
X_GRID = (0.2, 0.5, 1 - 1e-3, 1 - 1e-7, 1.0, 1 + 1e-7, 1 + 1e-3, 2.0, 10.0)
CHI_GRID = (-0.5, -0.3, 0.0, 0.5, 0.7)


def _g_dparam(kind, params, psi):
    import torch

    from crt1d_amd import batched

    n = len(params)
    dev = torch.device("cuda", torch.cuda.current_device())
    cols = batched.Columns(torch.as_tensor(psi).to(dev), torch.zeros((n, 2), dtype=torch.float64, device=dev),
                           torch.full((n,), kind, dtype=torch.int32, device=dev), torch.as_tensor(np.asarray(params, dtype=np.float64)).to(dev))
    dg_table, dg_at_psi = batched.g_dparam(cols)
    torch.cuda.synchronize()
    return dg_table.cpu().numpy(), dg_at_psi.cpu().numpy()


def test_g_dparam():
    """crt_hip_g_dparam_f64 against the Richardson central difference of leaf_angle.eval_G (relative step 1e-3 in x, absolute in chi_l) at
    the nodes and at psi: 1e-9 of max |dG| per column.  G is one analytic function of x through x = 1, where eval_G changes form (and
    returns the limit 1/2 at 1 itself), so a difference may straddle it; the device's derivative is continuous there (1 +- 1e-7 against
    1: 1e-6) and meets the closed limit cos^2 / 2 - 1 / 6 at 1.  Zeros for the parameterless kinds and for Bonan outside the clamp."""
    from crt1d_amd import _lib
    from crt1d_amd.leaf_angle import eval_G

    nodes = _lib.quad_nodes(0.501)
    for name, kind, grid in (("ellipsoidal", 3, X_GRID), ("approx", 4, X_GRID), ("bonan", 5, CHI_GRID)):
        psi = np.linspace(0.05, 1.3, len(grid))
        tab, at = _g_dparam(kind, grid, psi)
        for i, p in enumerate(grid):
            ang = np.concatenate([nodes, psi[i:i + 1]])
            got = np.concatenate([tab[i], at[i:i + 1]])
            h = 1e-3 * (1.0 if name == "bonan" else p)
            D = lambda s: (eval_G(kind, p + s, ang) - eval_G(kind, p - s, ang)) / (2 * s)  # noqa: E731
            want = (4 * D(h / 2) - D(h)) / 3
            if name == "bonan" and not -0.4 < p < 0.6:
                assert np.all(got == 0) and np.all(want == 0), (name, p)
                continue
            err = float(np.max(np.abs(got - want)) / np.max(np.abs(want)))
            print(f"g_dparam {name} {p!r}: {err:.2e} of max |dG|")
            assert err <= 1e-9, (name, p, err)
        if name == "ellipsoidal":
            i1 = grid.index(1.0)
            limit = np.cos(np.concatenate([nodes, psi[i1:i1 + 1]])) ** 2 / 2 - 1.0 / 6
            assert np.max(np.abs(np.concatenate([tab[i1], at[i1:i1 + 1]]) - limit)) <= 1e-15
            for j in (grid.index(1 - 1e-7), grid.index(1 + 1e-7)):
                step = float(max(np.max(np.abs(tab[j] - tab[i1])), abs(np.cos(psi[j]) ** 2 / 2 - 1.0 / 6 - at[j])))
                print(f"g_dparam ellipsoidal {grid[j]!r} against 1: {step:.2e}")
                assert step <= 1e-6, (grid[j], step)
    for kind in (0, 1, 2):  # horizontal, spherical, vertical
        tab, at = _g_dparam(kind, (0.0, 0.7), np.array([0.2, 1.0]))
        assert np.all(tab == 0) and np.all(at == 0)


@pytest.mark.parametrize("scheme,method", [(s, "quad") for s in SCHEMES] + [("n79", "9sky")])
def test_table_columns_match_closed_forms(scheme, method):
    """Every column re-expressed as CRT_G_TABLE -- its closed-form G sampled at the library's nodes by the host path of the drop-in
    solvers (solvers.common._describe) -- with the same tangent gives the closed-form result to 1e-12 of scale: the side precompute reads
    K_b where K0 does."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.solvers import common
    from oracle import crt_oracle as O

    for shape, uniform, kind in (((6, 13, 9), False, "ellipsoidal"), ((3, 70, 60), True, "bonan")):
        d = _host_kind(shape, uniform, kind)
        cols, bands, tan = _device_kind(shape, uniform, kind)
        desc = []
        for c in range(shape[0]):
            G = lambda p, c=c: O._G_closed_form(int(d["g_kind"][c]), float(d["g_param"][c]), np.asarray(p, dtype=np.float64))  # noqa: E731
            desc.append(common._describe(float(d["psi"][c]), lambda p, G=G: G(p) / np.cos(p), G, 0.501))
        assert all(x["g_kind"] == 6 for x in desc)
        dev = cols.device
        tcols = batched.Columns(cols.psi, cols.lai, torch.full((shape[0],), 6, dtype=torch.int32, device=dev), cols.g_param, cols.mla,
                                torch.as_tensor(np.array([x["g_at_psi"] for x in desc], dtype=np.float64)).to(dev),
                                torch.as_tensor(np.stack([x["g_table"] for x in desc])).to(dev))
        a = {k: v.clone() for k, v in _dleaf(scheme, cols, bands, tan, shape[2], tau_d_method=method)[1].items()}
        b = _dleaf(scheme, tcols, bands, tan, shape[2], tau_d_method=method)[1]
        scale = torch.stack([a[k].abs() for k in KEYS]).amax(dim=(0, 2), keepdim=True)[0]
        worst = max(float(((a[k] - b[k]).abs() / scale).max()) for k in KEYS)
        print(f"dleaf table vs closed form {scheme} {method} {kind} {shape}: {worst:.2e} of scale")
        for k in KEYS:
            assert bool(((a[k] - b[k]).abs() <= 1e-12 * scale).all()), (scheme, shape, k, worst)
        # the helper has nothing to say about a table column
        dt, da = batched.g_dparam(tcols)
        assert bool((dt == 0).all()) and bool((da == 0).all())


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bitwise_invariants(scheme, uniform):
    import torch

    from crt1d_amd import _lib, batched

    for i, shape in enumerate(SHAPES + (DEEP_SHAPES if scheme in TRI else [])):
        kind = list(KINDS)[i % 3]
        cols, bands, tan = _device_kind(shape, uniform, kind)
        tan = batched.LeafTangent(tan.dg_table, tan.dg_at_psi, torch.ones_like(cols.mla))
        nz = shape[2]
        lev = _levels(nz)
        plan, full = _dleaf(scheme, cols, bands, tan, nz)
        if scheme in TRI:
            assert plan.last_kernel().endswith(f"slice={_lanes(scheme, nz)}"), plan.last_kernel()
        full = {k: v.clone() for k, v in full.items()}
        # a column alone is its row of the batch
        for c in {0, shape[0] - 1}:
            one = batched.solve_levels_dleaf(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), lev, tan.slice(c, c + 1))
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(one[k][0], full[k][c]), (scheme, shape, c, k)
        # ground and top alone are their rows of the all-levels call
        _, ends = _dleaf(scheme, cols, bands, tan, nz, levels=(0, nz - 1))
        for k in KEYS:
            assert torch.equal(ends[k], full[k][:, [0, len(lev) - 1]]), (scheme, shape, k)
        # a key subset has the bits of the full call, in any order of the keys
        for keys in (("I_df_u",), ("F", "I_dr"), ("I_df_d",)):
            _, sub = _dleaf(scheme, cols, bands, tan, nz, keys=keys)
            assert set(sub) == set(keys)
            for k in keys:
                assert torch.equal(sub[k], full[k]), (scheme, shape, keys, k)
        # PRECOMPUTE_ONLY writes no output; SKIP_PRECOMPUTE on the workspace it filled gives the plain call's bits
        plan = batched.LevelsDleafPlan(scheme, cols, bands, lev, tan)
        for v in plan.out.values():
            v.fill_(7.0)
        plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
        assert plan.last_kernel() == "k_colpre + k_dleaf_side"
        for v in plan.out.values():
            assert bool((v == 7.0).all())
        got = plan(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], full[k]), (scheme, shape, "precompute only + skip precompute", k)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_graph_replay(scheme):
    """One replay of a captured plan equals the direct call (single stream, after a first call outside the capture)."""
    import torch

    shape = (3, 70, 60)
    cols, bands, tan = _device_kind(shape, True, "ellipsoidal")
    plan, got = _dleaf(scheme, cols, bands, tan, shape[2])
    ref = {k: v.clone() for k, v in got.items()}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan()
    for v in plan.out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(plan.out[k], ref[k]), k


def test_shared_spectra_equal_replicated_spectra():
    """col_stride == 0: one set of spectra for all columns gives the bits of a batch that repeats them per column."""
    import torch

    from crt1d_amd import batched, synth

    shape = (5, 70, 20)
    d = synth.make_columns(*shape, seed=11, per_column_optics=False)
    cols, shared = batched.Columns.from_host(d), batched.Bands.from_host(d)
    assert shared.col_stride(shape[0]) == 0
    rep = batched.Bands(*[getattr(shared, k).expand(shape[0], -1).contiguous() for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
    tan = batched.leaf_tangent(cols, "mla")
    for scheme in SCHEMES:
        a = batched.solve_levels_dleaf(scheme, cols, shared, (0, 7, 19), tan)
        b = batched.solve_levels_dleaf(scheme, cols, rep, (0, 7, 19), tan)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (scheme, k)
            assert bool(a[k].isfinite().all())


def test_leaf_tangent_wrt_mla():
    """wrt="mla": the generator ties x to mla by mla_to_x_approx, so the tangent is d/dmla of that family -- against the difference of
    the oracle in mla with x = mla_to_x_approx(mla) (2s: both x and cos^2 move), the bounds of the g_param test."""
    from crt1d_amd import batched
    from crt1d_amd.leaf_angle import mla_to_x_approx

    shape, uniform = (3, 70, 60), False
    d = _host_kind(shape, uniform, "approx")
    f = _oracle_f("2s", d, list(_levels(shape[2])), g_kind=d["g_kind"])
    J, J2 = _richardson(lambda delta: f(mla=d["mla"] + delta, g_param=mla_to_x_approx(d["mla"] + delta)), 0.2)
    cols, bands, _ = _device_kind(shape, uniform, "approx")
    _, got = _dleaf("2s", cols, bands, batched.leaf_tangent(cols, "mla"), shape[2])
    _compare(f"2s wrt mla {shape}", got, J, J2, _scale(J))


def test_sensor_dleaf():
    import torch

    from crt1d_amd import batched, spectra

    shape, uniform = (3, 70, 60), False
    d = _host_kind(shape, uniform, "ellipsoidal")
    cols, bands, tan = _device_kind(shape, uniform, "ellipsoidal")
    lev = _levels(shape[2])
    w = spectra.boxcar_sensor_weights(d["wle"], [(0.4, 0.5), (0.5, 0.7), (0.7, 1.0), (1.0, 1.8), (0.3, 2.6)])
    sensors = batched.SensorSet(w, device=cols.device)
    for scheme in ("2s", "n79"):
        ref = {k: v.clone() for k, v in _dleaf(scheme, cols, bands, tan, shape[2])[1].items()}
        got = batched.sensor_dleaf(scheme, cols, bands, lev, tan, sensors)
        torch.cuda.synchronize()
        for k in KEYS:
            r = ref[k].cpu().numpy()
            want, bound = np.einsum("sb,crb->crs", w, r), 1e-13 * np.einsum("sb,crb->crs", np.abs(w), np.abs(r))
            g = got[k].cpu().numpy()
            assert g.shape == (shape[0], len(lev), 5)
            print(f"sensor_dleaf {scheme} {k}: {float(np.max(np.abs(g - want) / np.where(bound == 0, 1, bound))) * 1e-13:.2e} of the weighted scale")
            assert np.all(np.abs(g - want) <= bound), (scheme, k)


def test_model_run_leaf_angle_sensitivity():
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model
    from crt1d_amd.solvers.common import _describe

    m = Model("2s", nlayers=60)
    J = m.run_leaf_angle_sensitivity()
    assert set(J) == set(KEYS)
    for k in KEYS:
        assert J[k].shape == (2, 107) and J[k].dtype == np.float64
    assert np.abs(J["F"]).max() > 0
    m._check_inputs()
    p = m._p
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
    g = _describe(float(p["psi"]), p.get("K_b_fn"), p.get("G_fn"), 0.501)
    cols = batched.Columns(psi=t(p["psi"]), lai=t(p["lai"])[None, :], g_kind=torch.tensor([g["g_kind"]], dtype=torch.int32, device=dev),
                           g_param=t(g["g_param"]), mla=t(float(p["mla"])), g_at_psi=None if g["g_at_psi"] is None else t(g["g_at_psi"]),
                           g_table=None if g["g_table"] is None else t(g["g_table"])[None, :])
    bands = batched.Bands(t(p["I_dr0_all"]), t(p["I_df0_all"]), t(p["leaf_r"]), t(p["leaf_t"]), t(p["soil_r"]))
    for wrt in ("param", "mla"):
        ref = batched.solve_levels_dleaf("2s", cols, bands, (0, 59), batched.leaf_tangent(cols, wrt))
        torch.cuda.synchronize()
        got = m.run_leaf_angle_sensitivity(wrt=wrt)
        for k in KEYS:
            assert np.array_equal(got[k], ref[k][0].cpu().numpy()), (wrt, k)
    assert np.array_equal(m.run_leaf_angle_sensitivity(levels=(-1,))["F"], J["F"][1:])
    with pytest.raises(ValueError, match="has no leaf-angle-derivative kernel"):
        Model("4s", nlayers=60).run_leaf_angle_sensitivity()
    with pytest.raises(ValueError, match="wrt must be one of"):
        m.run_leaf_angle_sensitivity(wrt="x")


@pytest.mark.parametrize("method", ["quad", "9sky"])
def test_dtau_d_dleaf_on_the_device(method):
    """crt_hip_dtau_d_dleaf_f64 against the host rule of tests/test_dleaf_cpu.py: 1e-15 of sum_q |term_q|, the rule's sum of magnitudes --
    the directions change sign over psi, so the terms cancel in the value itself; where they do not, that is |tau_d^th|."""
    import torch

    from crt1d_amd import _lib
    from domain_cases import CLASSES, G_np, device_rule
    from test_dleaf_cpu import dG_direction, host_dtau_d_dleaf_9sky, host_dtau_d_dleaf_quad
    from test_quadrature_domain_cpu import L_GRID

    lib = _lib.load()
    t, _ = device_rule()
    psi9 = np.radians(5.0 + 10.0 * np.arange(9))
    nodes = _lib.quad_nodes(0.501)
    L = np.asarray(L_GRID)
    worst = 0.0
    for name, kind, x in CLASSES:
        kb, dkb = np.empty(_lib.NQ), np.empty(_lib.NQ)
        for sl, c, s in ((slice(0, 96), np.sin(t), np.cos(t)), (slice(96, 128), np.cos(nodes[96:128]), np.sin(nodes[96:128])),
                         (slice(128, 137), np.cos(psi9), np.sin(psi9))):  # cos psi = sin t keeps its accuracy next to pi/2
            kb[sl], dkb[sl] = G_np(kind, x, c, s) / c, dG_direction(kind, x, c, s) / c
        if method == "quad":
            ref, mag = host_dtau_d_dleaf_quad(kb, dkb, L), -host_dtau_d_dleaf_quad(kb, np.abs(dkb), L)
        else:
            ref, mag = host_dtau_d_dleaf_9sky(kb[128:], dkb[128:], L), -host_dtau_d_dleaf_9sky(kb[128:], np.abs(dkb[128:]), L)
        kb_d, dkb_d, L_d = torch.as_tensor(kb).cuda(), torch.as_tensor(dkb).cuda(), torch.as_tensor(L).cuda()
        out = torch.full_like(L_d, float("nan"))
        st = lib.crt_hip_dtau_d_dleaf_f64(kb_d.data_ptr(), dkb_d.data_ptr(), L_d.data_ptr(), L_d.numel(), _lib.TAU_D_METHODS[method],
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert st == _lib.CRT_OK
        err = float(np.max(np.abs(out.cpu().numpy() - ref) / mag))
        print(f"dtau_d_dleaf device vs host rule, {method} {name:18s} {err:.2e}")
        worst = max(worst, err)
    print(f"dtau_d_dleaf device vs host rule, {method}: worst {worst:.2e}")
    assert worst <= 1e-15, (method, worst)


@pytest.mark.parametrize("scheme", ["n79", "zq"])
def test_depth_limit(scheme):
    """The deepest column the tridiagonal kernel serves (16 lanes per workgroup) passes the F' identity; one level more is
    CRT_ERR_UNSUPPORTED with the outputs and the workspace untouched."""
    import torch

    from crt1d_amd import _lib, batched, synth

    lim = _lib.DLAI_MAX_NZ[scheme]
    d = synth.make_columns(1, 1, lim, seed=11)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    plan = batched.LevelsDleafPlan(scheme, cols, bands, (0, lim // 2, lim - 1), batched.leaf_tangent(cols, "param"))
    got = plan()
    torch.cuda.synchronize()
    assert "slice=16" in plan.last_kernel(), plan.last_kernel()
    dI, dn, up, F = (got[k] for k in KEYS)
    assert bool(torch.isfinite(F).all()) and float(F.abs().max()) > 0
    scale = torch.stack([v.abs() for v in got.values()]).amax(dim=(0, 2), keepdim=True)[0]
    mu = float(np.cos(d["psi"][0]))
    assert bool(((F - (dI / mu + 2 * (dn + up))).abs() <= 1e-11 * scale).all())

    d = synth.make_columns(1, 1, lim + 1, seed=11)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    sentinel = 3.25
    out = {k: torch.full((1, 2, 1), sentinel, dtype=torch.float64, device="cuda") for k in KEYS}
    plan = batched.LevelsDleafPlan(scheme, cols, bands, (0, lim), tan, out=out)
    ws0 = plan.workspace.zero_().clone()
    torch.cuda.synchronize()
    lib = _lib.load()
    c, b, o = cols.c_struct(), bands.c_struct(1), _lib.CrtOptions(0.501, 0, 0)
    jo, tn = _lib.CrtDlaiOut(*[out[k].data_ptr() for k in KEYS]), tan.c_struct()
    lev = (ctypes.c_int32 * 2)(0, lim)
    st = lib.crt_hip_levels_dleaf_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), lev, 2, ctypes.byref(tn),
                                      ctypes.byref(jo), plan.workspace.data_ptr(), plan.workspace.numel() * plan.workspace.element_size(),
                                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == sentinel).all())
    assert torch.equal(plan.workspace, ws0)  # neither K0 nor the side precompute has run
    with pytest.raises(RuntimeError, match="not supported"):
        plan()
