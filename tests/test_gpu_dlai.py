"""GPU: the derivative of the level spectra with respect to the leaf area index (crt_hip_levels_dlai_f64, batched.LevelsDlaiPlan):
against the Richardson-extrapolated central differences of the oracle in the LAI scale s, exact identities of the schemes, bitwise
invariants (batch, levels, keys, flags, shared spectra, graph replay), tau_d' on the device, CRT_G_TABLE columns and the Python surface.

Measured on MI355X (each test prints its figures with -s).  Against the oracle, worst |J - J_ref| / scale per scheme: 2s 1.6e-9, bl 1.0e-11,
g77 1.4e-11, bf 5.2e-11, n79 8.4e-10 ((4, 1, 5) ragged; 1.8e-11 on the other shapes), zq 1.2e-10 -- the deep shapes (32- and 16-lane
slices) 1.2e-10 (n79) and 1.2e-10 (zq); n79 with tau_d_method '9sky' 8.2e-10 ((4, 1, 5) ragged, reference guard 7.7e-10; 1.4e-11 on the
other shapes) -- (bound 1e-7; the reference's own h against h / 2 guard reaches 2.9e-9, bound 1e-8).
Identities, worst residual / scale (bound 1e-11): I_dr' = -K_b L I_dr 4.4e-16 relative on every scheme (bound 1e-13); F' = I_dr' / mu +
2 (dn' + up') 2.4e-16; ground condition 2.8e-16 (2s), 8.9e-17 (bf), 3.7e-17 (n79), 7.3e-17 (zq); I_df_d'[nz-1] 1.9e-15 (2s), 0 (bl, bf,
n79); bl's I_df_u' and the doubling of (I_dr0, I_df0) exact.  tau_d' on the device against the host rule: 5.9e-16 ('quad'), 2.5e-16
('9sky').  CRT_G_TABLE columns against their closed forms: 3.9e-16 (bl), 8.2e-15 (n79; 0 with '9sky'), 5.2e-16 (zq) of scale (bound 1e-12).
sensor_dlai against the NumPy contraction: 9.1e-16 of the weighted scale (bound 1e-13)."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_jac import DEEP_SHAPES, SHAPES, _device, _host, _levels

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
TRI = ("n79", "zq")
H = 3e-3
# DEEP_SHAPES (n79 / zq only): (2, 40, 320) runs the 32-lane slice of k_dlai_tri (n79: 293 .. 536 levels, zq: 308 .. 599), two slices of
# 32 and 8 bands; (1, 20, 640) the 16-lane slice, 16 and 4 bands


def _shapes(scheme):
    return SHAPES + (DEEP_SHAPES if scheme in TRI else [])


def _lanes(scheme, nz):
    """Lanes per workgroup of k_dlai_tri (include/crt1d_hip_dlai.h)."""
    whole, half = (292, 536) if scheme == "n79" else (307, 599)
    return 64 if nz <= whole else 32 if nz <= half else 16


def _oracle_cols(d, lai=None):
    from oracle import crt_oracle as O

    return O.Columns(d["psi"], d["lai"] if lai is None else lai, mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])


@functools.lru_cache(maxsize=None)
def _reference(scheme, shape, uniform, method="quad"):
    """(J_ref, J_ref2, scale): the Richardson-extrapolated central difference (4 D(h/2) - D(h)) / 3 of the oracle in the LAI scale
    s (lai -> lai (1 +- h)) at h = H and at H / 2, each {key: (ncol, nsel, nb)}, and scale (ncol, 1, nb) = max |J_ref| over the levels
    and the four quantities.  ``method``: n79's ``tau_d_method``."""
    from oracle import crt_oracle as O

    d = _host(shape, uniform)
    lev = list(_levels(shape[2]))
    names = ("I_dr0", "I_df0", "leaf_r", "leaf_t") + (() if scheme == "bl" else ("soil_r",))
    kw = {k: d[k] for k in names}
    if method != "quad":
        assert scheme == "n79"
        kw["tau_d_method"] = method
    solve = getattr(O, f"solve_{scheme}")

    def f(s):
        out = solve(_oracle_cols(d, d["lai"] * s), **kw)
        return {k: out[k][:, lev, :] for k in KEYS}

    def D(h):
        hi, lo = f(1 + h), f(1 - h)
        return {k: (hi[k] - lo[k]) / (2 * h) for k in KEYS}

    d1, d2, d4 = D(H), D(H / 2), D(H / 4)
    J = {k: (4 * d2[k] - d1[k]) / 3 for k in KEYS}
    J2 = {k: (4 * d4[k] - d2[k]) / 3 for k in KEYS}
    scale = np.max(np.stack([np.abs(J[k]) for k in KEYS]), axis=(0, 2), keepdims=True)[0]
    return J, J2, scale


def _cases(methods=False):
    """(scheme, shape, uniform); with ``methods`` also the tau_d_method, and n79 once more with '9sky'.  '9sky' runs SHAPES only: what it
    changes is k_dlai_side, which does not know the lane width, and on the deep shapes the REFERENCE misses its own guard with '9sky'
    (h against h / 2 on the CPU: 6.3e-9 at (2, 40, 320) ragged, 6.7e-8 and 3.4e-7 at (1, 20, 640); <= 7.7e-10 on SHAPES)."""
    for scheme, method in [(s, "quad") for s in SCHEMES] + ([("n79", "9sky")] if methods else []):
        for shape in (_shapes(scheme) if method == "quad" else SHAPES):
            for uniform in (True, False):
                name = f"{scheme}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}"
                yield pytest.param(scheme, shape, uniform, method, id=name + "-9sky") if method != "quad" else \
                    pytest.param(*((scheme, shape, uniform) + (("quad",) if methods else ())), id=name)


def _dlai(scheme, shape, uniform, **kw):
    import torch

    from crt1d_amd import batched

    cols, bands = _device(shape, uniform)
    plan = batched.LevelsDlaiPlan(scheme, cols, bands, kw.pop("levels", _levels(shape[2])), **kw)
    got = plan()
    torch.cuda.synchronize()
    return plan, got


@pytest.mark.parametrize("scheme,shape,uniform,method", _cases(methods=True))
def test_dlai_against_the_oracle(scheme, shape, uniform, method):
    """|J - J_ref| <= 1e-7 scale for every element; the reference itself agrees with its h / 2 estimate to 1e-8 scale.  n79 with both
    tau_d_methods: '9sky' takes k_dlai_side through its nine-angle K_b and its own (1 - td_j)', on uniform columns with D = S_DL."""
    J, J2, scale = _reference(scheme, shape, uniform, method)
    plan, got = _dlai(scheme, shape, uniform, tau_d_method=method)
    assert plan.last_kernel().startswith("k_dlai_tri<" if scheme in TRI else "k_dlai<"), plan.last_kernel()
    if scheme in TRI:
        assert plan.last_kernel().endswith(f"slice={_lanes(scheme, shape[2])}"), plan.last_kernel()
    worst_ref = worst = 0.0
    den = np.where(scale == 0, 1.0, scale)
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.shape == J[k].shape
        assert np.isfinite(g).all()
        worst_ref = max(worst_ref, float(np.max(np.abs(J2[k] - J[k]) / den)))
        worst = max(worst, float(np.max(np.abs(g - J[k]) / den)))
    print(f"dlai-vs-oracle {scheme}{'' if method == 'quad' else ' ' + method} {shape} {'uniform' if uniform else 'ragged'}: {worst:.3e} of scale (reference guard {worst_ref:.3e})")
    for k in KEYS:
        assert np.all(np.abs(J2[k] - J[k]) <= 1e-8 * scale), (k, "the reference does not meet its own guard", worst_ref)
        assert np.all(np.abs(got[k].cpu().numpy() - J[k]) <= 1e-7 * scale), (scheme, shape, uniform, k, worst)


@pytest.mark.parametrize("scheme,shape,uniform", _cases())
def test_exact_identities(scheme, shape, uniform):
    import torch

    from crt1d_amd import batched

    d = _host(shape, uniform)
    cols, bands = _device(shape, uniform)
    lev = _levels(shape[2])
    _, got = _dlai(scheme, shape, uniform)
    val = batched.solve_levels(scheme, cols, bands, lev)
    torch.cuda.synchronize()
    dI, dn, up, F = (got[k] for k in KEYS)
    dev = dn.device
    scale = torch.as_tensor(_reference(scheme, shape, uniform)[2]).to(dev)  # (ncol, 1, nb), from J_ref
    worst = {}

    def check(name, resid, sc, factor=1e-11):
        worst[name] = float((resid.abs() / sc.clamp_min(1e-300)).max())
        assert bool((resid.abs() <= factor * sc).all()), (scheme, shape, uniform, name, worst[name])

    # I_dr' = -K_b L_j I_dr, with the oracle's K_b and the device's I_dr: 1e-13 relative
    Kb = torch.as_tensor(_oracle_cols(d).K_b()).to(dev)  # (ncol,)
    L = torch.as_tensor(d["lai"][:, list(lev)]).to(dev)  # (ncol, nsel)
    exact = -(Kb[:, None] * L)[:, :, None] * val["I_dr"]
    check("I_dr' = -K_b L I_dr", dI - exact, exact.abs(), 1e-13)
    mu = torch.as_tensor(np.cos(d["psi"])).to(dev)[:, None, None]
    check("F' = I_dr'/mu + 2 (dn' + up')", F - (dI / mu + 2 * (dn + up)), scale)
    assert lev[0] == 0 and lev[-1] == shape[2] - 1
    if scheme in ("2s", "bl", "bf", "n79"):  # the top value is I_df0
        check("top dn' = 0", dn[:, -1], scale[:, 0])
    if scheme in ("2s", "zq", "n79", "bf"):  # I_df_u[0] = soil_r (I_dr[0] + I_df_d[0]), differentiated with respect to s
        check("ground", up[:, 0] - bands.soil_r * (dI[:, 0] + dn[:, 0]), scale[:, 0])
    if scheme == "bl":
        assert bool((up == 0).all())
    # the outputs are linear in (I_dr0, I_df0): doubling both doubles every bit
    twice = batched.Bands(2 * bands.I_dr0, 2 * bands.I_df0, bands.leaf_r, bands.leaf_t, bands.soil_r)
    got2 = batched.solve_levels_dlai(scheme, cols, twice, lev)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(got2[k], 2 * got[k]), (scheme, shape, k, "doubling")
    print(f"dlai-identities {scheme} {shape} {'uniform' if uniform else 'ragged'}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bitwise_invariants(scheme, uniform):
    import torch

    from crt1d_amd import _lib, batched

    for shape in _shapes(scheme):
        cols, bands = _device(shape, uniform)
        nz = shape[2]
        lev = _levels(nz)
        plan, full = _dlai(scheme, shape, uniform)
        if scheme in TRI:
            assert plan.last_kernel().endswith(f"slice={_lanes(scheme, nz)}"), plan.last_kernel()
        full = {k: v.clone() for k, v in full.items()}
        # a column alone is its row of the batch
        for c in {0, shape[0] - 1}:
            one = batched.solve_levels_dlai(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), lev)
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(one[k][0], full[k][c]), (scheme, shape, c, k)
        # ground and top alone are their rows of the all-levels call
        _, ends = _dlai(scheme, shape, uniform, levels=(0, nz - 1))
        for k in KEYS:
            assert torch.equal(ends[k], full[k][:, [0, len(lev) - 1]]), (scheme, shape, k)
        # a key subset has the bits of the full call, in any order of the keys
        for keys in (("I_df_u",), ("F", "I_dr"), ("I_df_d",)):
            _, sub = _dlai(scheme, shape, uniform, keys=keys)
            assert set(sub) == set(keys)
            for k in keys:
                assert torch.equal(sub[k], full[k]), (scheme, shape, keys, k)
        # PRECOMPUTE_ONLY writes no output; SKIP_PRECOMPUTE on the workspace it filled gives the plain call's bits
        plan = batched.LevelsDlaiPlan(scheme, cols, bands, lev)
        for v in plan.out.values():
            v.fill_(7.0)
        plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
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
    plan, got = _dlai(scheme, shape, True)
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
    for scheme in SCHEMES:
        a = batched.solve_levels_dlai(scheme, cols, shared, (0, 7, 19))
        b = batched.solve_levels_dlai(scheme, cols, rep, (0, 7, 19))
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (scheme, k)


# tau_d' on the device against the host rule of tests/test_dtau_d_quadrature_cpu.py, relative, worst over the ten classes and L in
# {1e-6 .. 12} as measured on MI355X; asserted at 4 x
DTAU_MEASURED = {"quad": 5.9e-16, "9sky": 2.5e-16}


@pytest.mark.parametrize("method", ["quad", "9sky"])
def test_dtau_d_on_the_device(method):
    import torch

    from crt1d_amd import _lib
    from domain_cases import CLASSES, G_np, device_rule
    from test_dtau_d_quadrature_cpu import host_dtau_d_9sky, host_dtau_d_quad
    from test_quadrature_domain_cpu import L_GRID

    lib = _lib.load()
    t, _ = device_rule()
    psi9 = np.radians(5.0 + 10.0 * np.arange(9))
    nodes = _lib.quad_nodes(0.501)
    L = np.asarray(L_GRID)
    worst = 0.0
    for name, kind, x in CLASSES:
        kb = np.empty(_lib.NQ)
        kb[:96] = G_np(kind, x, np.sin(t), np.cos(t)) / np.sin(t)  # cos psi = sin t keeps its accuracy next to pi/2
        kb[96:128] = G_np(kind, x, np.cos(nodes[96:128]), np.sin(nodes[96:128])) / np.cos(nodes[96:128])
        kb[128:] = G_np(kind, x, np.cos(psi9), np.sin(psi9)) / np.cos(psi9)
        ref = host_dtau_d_quad(kb, L) if method == "quad" else host_dtau_d_9sky(kb[128:], L)
        kb_d, L_d = torch.as_tensor(kb).cuda(), torch.as_tensor(L).cuda()
        out = torch.full_like(L_d, float("nan"))
        st = lib.crt_hip_dtau_d_f64(kb_d.data_ptr(), L_d.data_ptr(), L_d.numel(), _lib.TAU_D_METHODS[method], out.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert st == _lib.CRT_OK
        err = float(np.max(np.abs(out.cpu().numpy() - ref) / np.abs(ref)))
        print(f"dtau_d device vs host rule, {method} {name:18s} {err:.2e}")
        worst = max(worst, err)
    print(f"dtau_d device vs host rule, {method}: worst {worst:.2e}")
    assert worst <= 4 * DTAU_MEASURED[method], (method, worst)


@pytest.mark.parametrize("scheme,method", [("bl", "quad"), ("n79", "quad"), ("n79", "9sky"), ("zq", "quad")])
def test_table_columns_match_closed_forms(scheme, method):
    """Every column re-expressed as CRT_G_TABLE -- its closed-form G sampled at the library's nodes by the host path of the drop-in
    solvers (solvers.common._describe) -- gives the closed-form result to 1e-12 of scale: the side precompute reads K_b where K0 does."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.solvers import common
    from oracle import crt_oracle as O

    for shape, uniform in (((6, 13, 9), False), ((3, 70, 60), True)):
        d = _host(shape, uniform)
        cols, bands = _device(shape, uniform)
        desc = []
        for c in range(shape[0]):
            G = lambda p, c=c: O._G_closed_form(int(d["g_kind"][c]), float(d["g_param"][c]), np.asarray(p, dtype=np.float64))  # noqa: E731
            desc.append(common._describe(float(d["psi"][c]), lambda p, G=G: G(p) / np.cos(p), G, 0.501))
        assert all(x["g_kind"] == 6 for x in desc)
        dev = cols.device
        tcols = batched.Columns(cols.psi, cols.lai, torch.full((shape[0],), 6, dtype=torch.int32, device=dev), cols.g_param, cols.mla,
                                torch.as_tensor(np.array([x["g_at_psi"] for x in desc], dtype=np.float64)).to(dev),
                                torch.as_tensor(np.stack([x["g_table"] for x in desc])).to(dev))
        lev = _levels(shape[2])
        a = batched.solve_levels_dlai(scheme, cols, bands, lev, tau_d_method=method)
        b = batched.solve_levels_dlai(scheme, tcols, bands, lev, tau_d_method=method)
        torch.cuda.synchronize()
        scale = torch.stack([a[k].abs() for k in KEYS]).amax(dim=(0, 2), keepdim=True)[0]
        worst = max(float(((a[k] - b[k]).abs() / scale).max()) for k in KEYS)
        print(f"dlai table vs closed form {scheme} {method} {shape}: {worst:.2e} of scale")
        for k in KEYS:
            assert bool(((a[k] - b[k]).abs() <= 1e-12 * scale).all()), (scheme, shape, k, worst)


def test_per_lai_and_sensor_dlai():
    import torch

    from crt1d_amd import batched, spectra

    shape, uniform = (3, 70, 60), False
    d = _host(shape, uniform)
    cols, bands = _device(shape, uniform)
    lev = _levels(shape[2])
    w = spectra.boxcar_sensor_weights(d["wle"], [(0.4, 0.5), (0.5, 0.7), (0.7, 1.0), (1.0, 1.8), (0.3, 2.6)])
    sensors = batched.SensorSet(w, device=cols.device)
    for scheme in ("2s", "n79"):
        log = {k: v.clone() for k, v in _dlai(scheme, shape, uniform)[1].items()}
        _, lai = _dlai(scheme, shape, uniform, per="lai")
        for k in KEYS:
            assert torch.equal(lai[k], log[k] / cols.lai[:, 0][:, None, None]), (scheme, k)
        for per, ref in (("log", log), ("lai", lai)):
            got = batched.sensor_dlai(scheme, cols, bands, lev, sensors, per=per)
            torch.cuda.synchronize()
            for k in KEYS:
                r = ref[k].cpu().numpy()
                want, bound = np.einsum("sb,crb->crs", w, r), 1e-13 * np.einsum("sb,crb->crs", np.abs(w), np.abs(r))
                g = got[k].cpu().numpy()
                assert g.shape == (shape[0], len(lev), 5)
                print(f"sensor_dlai {scheme} {per} {k}: {float(np.max(np.abs(g - want) / np.where(bound == 0, 1, bound))) * 1e-13:.2e} of the weighted scale")
                assert np.all(np.abs(g - want) <= bound), (scheme, per, k)


def test_model_run_lai_sensitivity():
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model
    from crt1d_amd.solvers.common import _describe

    m = Model("2s", nlayers=60)
    J = m.run_lai_sensitivity()
    assert set(J) == set(KEYS)
    for k in KEYS:
        assert J[k].shape == (2, 107) and J[k].dtype == np.float64
    m._check_inputs()
    p = m._p
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
    g = _describe(float(p["psi"]), p.get("K_b_fn"), p.get("G_fn"), 0.501)
    cols = batched.Columns(psi=t(p["psi"]), lai=t(p["lai"])[None, :], g_kind=torch.tensor([g["g_kind"]], dtype=torch.int32, device=dev),
                           g_param=t(g["g_param"]), mla=t(float(p["mla"])), g_at_psi=None if g["g_at_psi"] is None else t(g["g_at_psi"]),
                           g_table=None if g["g_table"] is None else t(g["g_table"])[None, :])
    bands = batched.Bands(t(p["I_dr0_all"]), t(p["I_df0_all"]), t(p["leaf_r"]), t(p["leaf_t"]), t(p["soil_r"]))
    for per in ("log", "lai"):
        ref = batched.solve_levels_dlai("2s", cols, bands, (0, 59), per=per)
        torch.cuda.synchronize()
        got = m.run_lai_sensitivity(per=per)
        for k in KEYS:
            assert np.array_equal(got[k], ref[k][0].cpu().numpy()), (per, k)
    assert np.array_equal(m.run_lai_sensitivity(levels=(-1,))["F"], J["F"][1:])
    with pytest.raises(ValueError, match="has no LAI-derivative kernel"):
        Model("4s", nlayers=60).run_lai_sensitivity()
    with pytest.raises(ValueError, match="per must be"):
        m.run_lai_sensitivity(per="percent")


@pytest.mark.parametrize("scheme", ["n79", "zq"])
def test_depth_limit(scheme):
    """The deepest column the tridiagonal kernel serves (16 lanes per workgroup) passes the F' identity; one level more is
    CRT_ERR_UNSUPPORTED with the outputs and the workspace untouched."""
    import torch

    from crt1d_amd import _lib, batched, synth

    lim = _lib.DLAI_MAX_NZ[scheme]
    d = synth.make_columns(1, 1, lim, seed=11)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    plan = batched.LevelsDlaiPlan(scheme, cols, bands, (0, lim // 2, lim - 1))
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
    sentinel = 3.25
    out = {k: torch.full((1, 2, 1), sentinel, dtype=torch.float64, device="cuda") for k in KEYS}
    plan = batched.LevelsDlaiPlan(scheme, cols, bands, (0, lim), out=out)
    ws0 = plan.workspace.zero_().clone()
    torch.cuda.synchronize()
    lib = _lib.load()
    c, b, o = cols.c_struct(), bands.c_struct(1), _lib.CrtOptions(0.501, 0, 0)
    jo = _lib.CrtDlaiOut(*[out[k].data_ptr() for k in KEYS])
    lev = (ctypes.c_int32 * 2)(0, lim)
    st = lib.crt_hip_levels_dlai_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), lev, 2, ctypes.byref(jo),
                                     plan.workspace.data_ptr(), plan.workspace.numel() * plan.workspace.element_size(),
                                     torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == sentinel).all())
    assert torch.equal(plan.workspace, ws0)  # neither K0 nor the side precompute has run
    with pytest.raises(RuntimeError, match="not supported"):
        plan()
