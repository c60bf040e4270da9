"""GPU: the optical-property Jacobians of the level spectra (crt_hip_levels_jac_f64, batched.LevelsJacPlan): against the
Richardson-extrapolated central differences of the oracle, exact identities of the schemes, bitwise invariants (batch, levels, keys,
flags, graph replay), sensor_jvp, Model.run_jacobian and the depth limit of the tridiagonal kernel.

Measured on MI355X (each test prints its figures with -s).  Against the oracle, worst |J - J_ref| / scale per scheme: 2s 2.7e-9, bl 4.6e-9,
g77 5.7e-9, bf 3.8e-9, n79 6.6e-10, zq 1.9e-10 -- the deep shapes (32- and 16-lane slices) 1.0e-10 (n79) and 1.9e-10 (zq) -- (bound 1e-7; the reference's own h against h / 2 guard reaches 9.4e-9, bound 1e-8).
Identities, worst residual / scale (bound 1e-11): F' = 2 (dn' + up') 0 everywhere; ground condition 3.1e-13 (2s), 2.0e-14 (bf), 5.0e-14
(n79), 1.1e-14 (zq); I_df_d'[nz-1] 1.8e-15 (2s), 0 (n79, bf); bl / g77 leaf_r slab against leaf_t slab 0 (bound 1e-13)."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")
KEYS = ("I_df_d", "I_df_u", "F")
SHAPES = [(6, 13, 9), (3, 70, 60), (2, 130, 100), (4, 1, 5)]  # (ncol, nb, nz)
# n79 / zq only: columns deep enough for the narrowed band slices of k_jac_tri (whole waves up to 304 / 311 levels, 32 lanes up to 584 /
# 619, 16 lanes beyond), with more bands than one slice holds: two slices of 32 and two of 16, the last one partial
DEEP_SHAPES = [(2, 40, 320), (1, 20, 640)]
TRI = ("n79", "zq")
H = 1e-3
PARAMS = ("leaf_r", "leaf_t", "soil_r")


def _levels(nz):
    if nz <= 64:
        return tuple(range(nz))
    step = 7
    while len(range(0, nz, step)) + 1 > 64:  # (one call serves 64 levels)
        step += 4
    return tuple(sorted(set(range(0, nz, step)) | {nz - 1}))


def _shapes(scheme):
    return SHAPES + (DEEP_SHAPES if scheme in TRI else [])


def _lanes(scheme, nz):
    """Lanes per workgroup of k_jac_tri (include/crt1d_hip_jac.h)."""
    whole, half = (304, 584) if scheme == "n79" else (311, 619)
    return 64 if nz <= whole else 32 if nz <= half else 16


@functools.lru_cache(maxsize=None)
def _host(shape, uniform):
    from crt1d_amd import synth

    return synth.make_columns(*shape, seed=11, uniform_dlai=uniform)


@functools.lru_cache(maxsize=None)
def _device(shape, uniform):
    import torch

    from crt1d_amd import batched

    d = _host(shape, uniform)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    torch.cuda.synchronize()
    return cols, bands


@functools.lru_cache(maxsize=None)
def _reference(scheme, shape, uniform):
    """(J_ref, J_ref2, scale): the Richardson-extrapolated central difference of the oracle at h and at h / 2, each
    {key: (ncol, nsel, 3, nb)}, and the scale (ncol, 1, 3, nb) = max |J_ref| over the levels and the three quantities."""
    from oracle import crt_oracle as O

    d = _host(shape, uniform)
    oc = O.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
    lev = list(_levels(shape[2]))
    names = ("I_dr0", "I_df0", "leaf_r", "leaf_t") + (() if scheme == "bl" else ("soil_r",))
    solve = getattr(O, f"solve_{scheme}")

    def f(param, delta):
        kw = {k: d[k] for k in names}
        kw[param] = kw[param] + delta
        out = solve(oc, **kw)
        return {k: out[k][:, lev, :] for k in KEYS}

    def D(param, h):
        hi, lo = f(param, h), f(param, -h)
        return {k: (hi[k] - lo[k]) / (2 * h) for k in KEYS}

    ncol, nb, _ = shape
    J = {k: np.zeros((ncol, len(lev), 3, nb)) for k in KEYS}
    J2 = {k: np.zeros((ncol, len(lev), 3, nb)) for k in KEYS}
    for p, param in enumerate(PARAMS):
        if param not in names:
            continue  # bl has no soil: the slab is zero
        d1, d2, d4 = D(param, H), D(param, H / 2), D(param, H / 4)
        for k in KEYS:
            J[k][:, :, p] = (4 * d2[k] - d1[k]) / 3
            J2[k][:, :, p] = (4 * d4[k] - d2[k]) / 3
    scale = np.max(np.stack([np.abs(J[k]) for k in KEYS]), axis=(0, 2), keepdims=True)[0]
    return J, J2, scale


def _cases():
    for scheme in SCHEMES:
        for shape in _shapes(scheme):
            for uniform in (True, False):
                yield pytest.param(scheme, shape, uniform, id=f"{scheme}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}")


def _jac(scheme, shape, uniform, **kw):
    import torch

    from crt1d_amd import batched

    cols, bands = _device(shape, uniform)
    plan = batched.LevelsJacPlan(scheme, cols, bands, kw.pop("levels", _levels(shape[2])), **kw)
    got = plan()
    torch.cuda.synchronize()
    return plan, got


@pytest.mark.parametrize("scheme,shape,uniform", _cases())
def test_jacobian_against_the_oracle(scheme, shape, uniform):
    """|J - J_ref| <= 1e-7 scale for every element; the reference itself agrees with its h / 2 estimate to 1e-8 scale."""
    J, J2, scale = _reference(scheme, shape, uniform)
    plan, got = _jac(scheme, shape, uniform)
    assert plan.last_kernel().startswith("k_jac_tri<" if scheme in TRI else "k_jac<"), plan.last_kernel()
    if scheme in TRI:
        assert plan.last_kernel().endswith(f"slice={_lanes(scheme, shape[2])}"), plan.last_kernel()
    worst_ref = worst = 0.0
    for k in KEYS:
        g = got[k].cpu().numpy()
        assert g.shape == J[k].shape
        assert np.isfinite(g).all()
        den = np.where(scale == 0, 1.0, scale)
        worst_ref = max(worst_ref, float(np.max(np.abs(J2[k] - J[k]) / den)))
        worst = max(worst, float(np.max(np.abs(g - J[k]) / den)))
        assert np.all(np.abs(J2[k] - J[k]) <= 1e-8 * scale), (k, "the reference does not meet its own guard")
        assert np.all(np.abs(g - J[k]) <= 1e-7 * scale), (scheme, shape, uniform, k, worst)
    print(f"jac-vs-oracle {scheme} {shape} {'uniform' if uniform else 'ragged'}: {worst:.3e} of scale (reference guard {worst_ref:.3e})")


@pytest.mark.parametrize("scheme,shape,uniform", _cases())
def test_exact_identities(scheme, shape, uniform):
    import torch

    from crt1d_amd import batched

    cols, bands = _device(shape, uniform)
    lev = _levels(shape[2])
    _, got = _jac(scheme, shape, uniform)
    val = batched.solve_levels(scheme, cols, bands, lev)
    torch.cuda.synchronize()
    dn, up, F = (got[k] for k in KEYS)
    scale = torch.as_tensor(_reference(scheme, shape, uniform)[2]).to(dn.device)  # (ncol, 1, 3, nb), from J_ref
    worst = {}

    def check(name, resid, sc, factor=1e-11):
        worst[name] = float((resid.abs() / sc.clamp_min(1e-300)).max())
        assert bool((resid.abs() <= factor * sc).all()), (scheme, shape, uniform, name, worst[name])

    check("F' = 2 (dn' + up')", F - 2 * (dn + up), scale)
    assert lev[0] == 0 and lev[-1] == shape[2] - 1
    if scheme in ("2s", "zq", "n79", "bf"):  # I_df_u[0] = soil_r (I_dr[0] + I_df_d[0]), differentiated
        rs = bands.soil_r  # (ncol, nb)
        check("ground, leaf", up[:, 0, :2] - rs[:, None, :] * dn[:, 0, :2], scale[:, 0, :2])
        lit = val["I_dr"][:, 0] + val["I_df_d"][:, 0]
        check("ground, soil", up[:, 0, 2] - (lit + rs * dn[:, 0, 2]), scale[:, 0, 2])
    if scheme in ("2s", "n79", "bf"):
        check("top dn' = 0", dn[:, -1], scale[:, 0])
    if scheme == "bl":
        assert bool((up == 0).all()) and bool((dn[:, :, 2] == 0).all()) and bool((F[:, :, 2] == 0).all())
    if scheme in ("bl", "g77"):  # both depend on leaf_r + leaf_t only
        for x in (dn, up, F):
            check("leaf_r slab = leaf_t slab", x[:, :, 0] - x[:, :, 1], scale[:, :, 0], 1e-13)
    print(f"jac-identities {scheme} {shape} {'uniform' if uniform else 'ragged'}: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bitwise_invariants(scheme, uniform):
    import torch

    from crt1d_amd import _lib, batched

    for shape in _shapes(scheme):
        cols, bands = _device(shape, uniform)
        nz = shape[2]
        lev = _levels(nz)
        plan, full = _jac(scheme, shape, uniform)
        if scheme in TRI:
            assert plan.last_kernel().endswith(f"slice={_lanes(scheme, nz)}"), plan.last_kernel()
        full = {k: v.clone() for k, v in full.items()}
        # a column alone is its row of the batch
        for c in {0, shape[0] - 1}:
            one = batched.solve_levels_jac(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), lev)
            torch.cuda.synchronize()
            for k in KEYS:
                assert torch.equal(one[k][0], full[k][c]), (scheme, shape, c, k)
        # ground and top alone are their rows of the all-levels call
        _, ends = _jac(scheme, shape, uniform, levels=(0, nz - 1))
        for k in KEYS:
            assert torch.equal(ends[k], full[k][:, [0, len(lev) - 1]]), (scheme, shape, k)
        # a key subset has the bits of the full call, in any order of the keys
        for keys in (("I_df_u",), ("F", "I_df_d")):
            _, sub = _jac(scheme, shape, uniform, keys=keys)
            assert set(sub) == set(keys)
            for k in keys:
                assert torch.equal(sub[k], full[k]), (scheme, shape, keys, k)
        # the records of crt_hip_levels_f64 serve the Jacobian
        lp = batched.LevelsPlan(scheme, cols, bands, (0,))
        lp()
        torch.cuda.synchronize()
        plan = batched.LevelsJacPlan(scheme, cols, bands, lev, workspace=lp.workspace)
        got = plan(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], full[k]), (scheme, shape, "skip precompute", k)
        for v in plan.out.values():
            v.fill_(7.0)
        plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
        for v in plan.out.values():
            assert bool((v == 7.0).all())


@pytest.mark.parametrize("scheme", SCHEMES)
def test_graph_replay(scheme):
    """One replay of a captured plan equals the direct call (single stream, after a first call outside the capture)."""
    import torch

    shape = (3, 70, 60)
    plan, got = _jac(scheme, shape, True)
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


def test_broadcast_spectra_give_each_column_its_own_response():
    """col_stride == 0: one set of spectra for all columns; the derivative is the one of a batch that repeats them per column."""
    import torch

    from crt1d_amd import batched, synth

    shape = (5, 70, 20)
    d = synth.make_columns(*shape, seed=11, per_column_optics=False)
    cols, shared = batched.Columns.from_host(d), batched.Bands.from_host(d)
    assert shared.col_stride(shape[0]) == 0
    rep = batched.Bands(*[getattr(shared, k).expand(shape[0], -1).contiguous() for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
    for scheme in ("2s", "zq"):
        a = batched.solve_levels_jac(scheme, cols, shared, (0, 19))
        b = batched.solve_levels_jac(scheme, cols, rep, (0, 19))
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (scheme, k)


# Rows whose exact derivative is identically zero (the identity I_df_d'[nz-1] = 0 of test_exact_identities): there the finite-difference
# reference is its own rounding noise (measured: 5.9e-10 of scale for 2s at (3, 70, 60)), and a bound proportional to |J_ref| is a bound
# proportional to that noise, which nothing meets.  These rows are compared with their exact value, zero, at 1e-11 of the weighted scale
# (tighter than the 1e-7 of the other rows); every other row has the bound 1e-7 sum_b |w| sum_p |J_ref| |d|.
EXACT_ZERO_TOP = {("2s", "I_df_d")}


@pytest.mark.parametrize("scheme", ["2s", "zq"])
def test_sensor_jvp(scheme):
    import torch

    from crt1d_amd import batched, spectra

    shape, uniform, ntan = (3, 70, 60), True, 4
    d = _host(shape, uniform)
    cols, bands = _device(shape, uniform)
    J, _, _ = _reference(scheme, shape, uniform)
    w = spectra.boxcar_sensor_weights(d["wle"], [(0.4, 0.5), (0.5, 0.7), (0.7, 1.0), (1.0, 1.8), (0.3, 2.6)])
    sensors = batched.SensorSet(w, device=cols.device)
    rng = np.random.default_rng(3)
    dirs = [rng.normal(size=(ntan, shape[1])), rng.normal(size=(shape[0], ntan, shape[1])), rng.normal(size=(ntan, shape[1]))]
    got = batched.sensor_jvp(scheme, cols, bands, _levels(shape[2]), sensors, *dirs)
    torch.cuda.synchronize()
    D = np.stack([np.broadcast_to(x, (shape[0], ntan, shape[1])) for x in dirs], axis=1)  # (ncol, 3, ntan, nb)
    scale = _reference(scheme, shape, uniform)[2]
    for k in KEYS:
        ref = np.einsum("sb,crpb,cpkb->crsk", w, J[k], D)
        bound = 1e-7 * np.einsum("sb,crpb,cpkb->crsk", np.abs(w), np.abs(J[k]), np.abs(D))
        g = got[k].cpu().numpy()
        assert g.shape == (shape[0], len(_levels(shape[2])), 5, ntan)
        rows = slice(None)
        if (scheme, k) in EXACT_ZERO_TOP:
            floor = 1e-11 * np.einsum("sb,cpb,cpkb->csk", np.abs(w), scale[:, 0], np.abs(D))
            assert np.all(np.abs(g[:, -1]) <= floor), (scheme, k, "top row")
            rows = slice(0, -1)
        print(f"sensor_jvp {scheme} {k}: {float(np.max(np.abs(g - ref)[:, rows] / bound[:, rows])) * 1e-7:.3e} of the weighted scale")
        assert np.all(np.abs(g - ref)[:, rows] <= bound[:, rows]), (scheme, k)


def test_model_run_jacobian():
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model
    from crt1d_amd.solvers.common import _describe

    m = Model("2s", nlayers=60)
    J = m.run_jacobian()
    assert set(J) == set(KEYS)
    for k in KEYS:
        assert J[k].shape == (2, 3, 107) and J[k].dtype == np.float64
    m._check_inputs()
    p = m._p
    dev = torch.device("cuda", torch.cuda.current_device())
    t = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
    g = _describe(float(p["psi"]), p.get("K_b_fn"), p.get("G_fn"), 0.501)
    cols = batched.Columns(psi=t(p["psi"]), lai=t(p["lai"])[None, :], g_kind=torch.tensor([g["g_kind"]], dtype=torch.int32, device=dev),
                           g_param=t(g["g_param"]), mla=t(float(p["mla"])), g_at_psi=None if g["g_at_psi"] is None else t(g["g_at_psi"]),
                           g_table=None if g["g_table"] is None else t(g["g_table"])[None, :])
    bands = batched.Bands(t(p["I_dr0_all"]), t(p["I_df0_all"]), t(p["leaf_r"]), t(p["leaf_t"]), t(p["soil_r"]))
    ref = batched.solve_levels_jac("2s", cols, bands, (0, 59))
    torch.cuda.synchronize()
    for k in KEYS:
        assert np.array_equal(J[k], ref[k][0].cpu().numpy()), k
    assert np.array_equal(m.run_jacobian(levels=(-1,))["F"], J["F"][1:])
    with pytest.raises(ValueError, match="has no Jacobian kernel"):
        Model("4s", nlayers=60).run_jacobian()


@pytest.mark.parametrize("scheme", ["n79", "zq"])
def test_depth_limit(scheme):
    """The deepest column the tridiagonal kernel serves (16 lanes per workgroup) passes the F' identity; one level more is
    CRT_ERR_UNSUPPORTED with the output untouched."""
    import torch

    from crt1d_amd import _lib, batched, synth

    lim = _lib.JAC_MAX_NZ[scheme]
    d = synth.make_columns(1, 1, lim, seed=11)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    plan = batched.LevelsJacPlan(scheme, cols, bands, (0, lim // 2, lim - 1))
    got = plan()
    torch.cuda.synchronize()
    assert "slice=16" in plan.last_kernel(), plan.last_kernel()
    dn, up, F = (got[k] for k in KEYS)
    assert bool(torch.isfinite(F).all()) and float(F.abs().max()) > 0
    scale = torch.stack([dn.abs(), up.abs(), F.abs()]).amax(dim=(0, 2), keepdim=True)[0]
    assert bool(((F - 2 * (dn + up)).abs() <= 1e-11 * scale).all())

    d = synth.make_columns(1, 1, lim + 1, seed=11)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    sentinel = 3.25
    out = {k: torch.full((1, 2, 3, 1), sentinel, dtype=torch.float64, device="cuda") for k in KEYS}
    plan = batched.LevelsJacPlan(scheme, cols, bands, (0, lim), out=out)
    ws0 = plan.workspace.zero_().clone()
    torch.cuda.synchronize()
    lib = _lib.load()
    c, b, o = cols.c_struct(), bands.c_struct(1), _lib.CrtOptions(0.501, 0, 0)
    jo = _lib.CrtJacOut(*[out[k].data_ptr() for k in KEYS])
    lev = (ctypes.c_int32 * 2)(0, lim)
    st = lib.crt_hip_levels_jac_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), lev, 2, ctypes.byref(jo),
                                    plan.workspace.data_ptr(), plan.workspace.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == sentinel).all())
    assert torch.equal(plan.workspace, ws0)  # K0 has not run either
    with pytest.raises(RuntimeError, match="not supported"):
        plan()
