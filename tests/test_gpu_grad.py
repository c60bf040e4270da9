"""GPU: the gradient of a weighted sum of the level spectra (crt_hip_levels_grad_f64, batched.LevelsGradPlan) and the differentiable
solve_levels_ad on top of it.

1. Against the composition it replaces: the outputs of LevelsJacPlan, LevelsDlaiPlan and LevelsDleafPlan contracted with random weights
   on the host in np.longdouble.  The kernel multiplies and adds the same tangent bits (the same jac_schemes.hpp instantiations,
   -ffp-contract=off); only the products and the order of the sum differ, so the bound is derived, not measured:
   |g - g_ref| <= 2 n u S with n the number of terms of that output, u = 2^-53 and S the sum of their magnitudes (recursive summation in
   any order, plus one rounding per product).  Measured on MI355X: see the docstring of test_against_the_composition.
2. End to end against the oracle: <g, direction> against the Richardson-extrapolated central difference of sum w X of the oracle along
   a random direction in (leaf_r, leaf_t, soil_r, the LAI scale, g_param), conventions and constants of tests/test_gpu_dleaf.py: 1e-6
   of S, asserted after the reference's own h against h / 2 guard (1e-7).  All six schemes (n79, zq: the composed path).
3. Bitwise invariants: batch, subsets of wrt, doubled weights, the precompute flags, shared spectra, graph replay, bl.
4. Refusals on the device: n79, zq, 4s, zq_pa through the C entry.
5. Autograd: forward bits, .grad against the plan, gradcheck, a sensor misfit against sensor_jvp / sensor_dlai / sensor_dleaf."""
import ctypes
import functools

import numpy as np
import pytest

from test_gpu_dleaf import H, KINDS, _host_kind, _richardson
from test_gpu_jac import SHAPES, _levels

pytestmark = pytest.mark.gpu

CLOSED = ("2s", "bl", "g77", "bf")
SCHEMES = CLOSED + ("n79", "zq")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
JAC_KEYS = ("I_df_d", "I_df_u", "F")
PARAMS = ("leaf_r", "leaf_t", "soil_r")
WRT = PARAMS + ("lai", "leaf")
# (ncol, nb, nz): those of the Jacobian tests; two band slices with the last one partial (257 = 129 + 128, 300 = 150 + 150: 106 idle
# lanes in the last wave); one column with 64 levels selected
GRAD_SHAPES = list(SHAPES) + [(2, 257, 4), (2, 300, 5), (1, 5, 70)]
U = 2.0 ** -53
REF_GUARD, BOUND = 1e-7, 1e-6


def _lev(shape):
    nz = shape[2]
    return tuple(range(63)) + (nz - 1,) if shape == (1, 5, 70) else _levels(nz)


def _kind(shape):
    return list(KINDS)[GRAD_SHAPES.index(shape) % 3]  # every parametric leaf-angle kind is met


@functools.lru_cache(maxsize=None)
def _device(shape, uniform):
    """(cols, bands, tangent along g_param, weights): the generator's columns with the shape's parametric leaf-angle kind, random weights
    in (-1, 1) for the four quantities."""
    import torch

    from crt1d_amd import batched

    d = _host_kind(shape, uniform, _kind(shape))
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    rng = np.random.default_rng(17)
    w = {k: torch.as_tensor(rng.uniform(-1.0, 1.0, (shape[0], len(_lev(shape)), shape[1]))).to(cols.device) for k in KEYS}
    torch.cuda.synchronize()
    return cols, bands, tan, w


def _grad(scheme, cols, bands, lev, w, **kw):
    import torch

    from crt1d_amd import batched

    plan = batched.LevelsGradPlan(scheme, cols, bands, lev, w, **kw)
    got = plan()
    torch.cuda.synchronize()
    return plan, {k: v.clone() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def _tangents(scheme, shape, uniform):
    """What the three existing plans write, on the host: (J {key: (ncol, nsel, 3, nb)}, dlai, dleaf {key: (ncol, nsel, nb)})."""
    import torch

    from crt1d_amd import batched

    cols, bands, tan, _ = _device(shape, uniform)
    lev = _lev(shape)
    J = batched.solve_levels_jac(scheme, cols, bands, lev)
    A = batched.solve_levels_dlai(scheme, cols, bands, lev)
    B = batched.solve_levels_dleaf(scheme, cols, bands, lev, tan)
    torch.cuda.synchronize()
    host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}  # noqa: E731
    return host(J), host(A), host(B)


def _contract(scheme, shape, uniform, w):
    """{name: (g_ref, S, n)} in np.longdouble: the contraction of the plans' tangents with the host weights ``w``, the sum of the
    magnitudes of its terms and their number.  bl: w["I_df_u"] takes no part."""
    J, A, B = _tangents(scheme, shape, uniform)
    keys = [k for k in KEYS if k in w and not (scheme == "bl" and k == "I_df_u")]
    ld = np.longdouble
    out = {}
    nsel = len(_lev(shape))
    for p, name in enumerate(PARAMS):
        jk = [k for k in keys if k in JAC_KEYS]
        terms = [w[k].astype(ld) * J[k][:, :, p, :].astype(ld) for k in jk]
        g = sum(t.sum(axis=1) for t in terms) if terms else np.zeros((shape[0], shape[1]), dtype=ld)
        S = sum(np.abs(t).sum(axis=1) for t in terms) if terms else np.zeros((shape[0], shape[1]), dtype=ld)
        out[name] = (g, S, len(jk) * nsel)
    for name, D in (("lai", A), ("leaf", B)):
        terms = [w[k].astype(ld) * D[k].astype(ld) for k in keys]
        out[name] = (sum(t.sum(axis=(1, 2)) for t in terms), sum(np.abs(t).sum(axis=(1, 2)) for t in terms), len(keys) * nsel * shape[1])
    return out


def _cases(schemes, shapes):
    for scheme in schemes:
        for shape in shapes:
            for uniform in (True, False):
                yield pytest.param(scheme, shape, uniform, id=f"{scheme}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}")


@pytest.mark.parametrize("scheme,shape,uniform", _cases(CLOSED, GRAD_SHAPES))
def test_against_the_composition(scheme, shape, uniform):
    """|g - g_ref| <= 2 n u S for every element of every output.  Measured on MI355X, worst |g - g_ref| / (2 n u S) over the shapes:
    2s 0.14, bl 0.15, g77 0.13, bf 0.13 (the optics outputs at 257 and 300 bands, n = 3 nsel = 12); lai and leaf at most 0.033 (one
    band, five levels) and below 1e-4 from 13 bands on."""
    cols, bands, tan, w = _device(shape, uniform)
    plan, got = _grad(scheme, cols, bands, _lev(shape), w, tangent=tan)
    nslice = -(-shape[1] // 256)
    assert plan.last_kernel() == f"k_grad<{scheme}> nsel={len(_lev(shape))} slice={-(-shape[1] // nslice)}" + (" + k_grad_finish" if nslice > 1 else "")
    ref = _contract(scheme, shape, uniform, {k: v.cpu().numpy() for k, v in w.items()})
    worst = {}
    for name in WRT:
        g, (r, S, n) = got[name].cpu().numpy(), ref[name]
        assert g.shape == r.shape and np.isfinite(g).all(), name
        bound = 2 * n * U * S
        err = np.abs(g.astype(np.longdouble) - r)
        worst[name] = float(np.max(err / np.where(bound == 0, 1, bound)))
        if scheme == "bl" and name == "soil_r":
            assert np.all(g == 0)
        else:
            assert float(np.max(S)) > 0, name
    print(f"grad-vs-composition {scheme} {shape} {'uniform' if uniform else 'ragged'}: |g - g_ref| / (2 n u S) " +
          ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    for name in WRT:
        g, (r, S, n) = got[name].cpu().numpy(), ref[name]
        assert np.all(np.abs(g.astype(np.longdouble) - r) <= 2 * n * U * S), (scheme, shape, name, worst[name])


# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _direction(shape, uniform):
    """A random direction: relative steps of the optics, of the LAI scale and of g_param (Bonan's chi_l: absolute)."""
    d = _host_kind(shape, uniform, _kind(shape))
    rng = np.random.default_rng(23)
    dr = {k: rng.uniform(-1.0, 1.0, d[k].shape) * d[k] for k in PARAMS}
    dl = rng.uniform(-1.0, 1.0, shape[0])
    dg = rng.uniform(-1.0, 1.0, shape[0]) * (np.ones(shape[0]) if _kind(shape) == "bonan" else d["g_param"])
    return dr, dl, dg


@functools.lru_cache(maxsize=None)
def _oracle_reference(scheme, shape, uniform):
    """(D, D2): the Richardson-extrapolated central differences at H and H / 2 of the oracle's level spectra {key: (ncol, nsel, nb)} along
    the direction of _direction."""
    from oracle import crt_oracle as O

    d = _host_kind(shape, uniform, _kind(shape))
    dr, dl, dg = _direction(shape, uniform)
    lev = list(_lev(shape))
    solve = getattr(O, f"solve_{scheme}")

    def f(delta):
        kw = {k: d[k] for k in ("I_dr0", "I_df0")}
        for k in ("leaf_r", "leaf_t") + (() if scheme == "bl" else ("soil_r",)):
            kw[k] = d[k] + delta * dr[k]
        oc = O.Columns(d["psi"], d["lai"] * (1 + delta * dl)[:, None], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"] + delta * dg)
        out = solve(oc, **kw)
        return {k: out[k][:, lev, :] for k in KEYS}

    return _richardson(f, H)


@pytest.mark.parametrize("scheme,shape,uniform", _cases(SCHEMES, GRAD_SHAPES[:2]))
def test_against_the_oracle(scheme, shape, uniform):
    """<g, direction> against d/d delta of sum w X of the oracle, per column: 1e-6 of S = sum |w| |dX / d delta|, after the reference
    agrees with its own h / 2 estimate to 1e-7 of S.  Measured on MI355X, worst error (reference guard): 2s 1.4e-11 (1.3e-11), bl 6.4e-10
    (6.0e-10), g77 1.0e-9 (9.3e-10), bf 5.0e-10 (4.6e-10), n79 5.6e-12 (5.3e-12), zq 4.5e-12 (4.1e-12) -- the differences are the
    reference's."""
    cols, bands, tan, w = _device(shape, uniform)
    plan, got = _grad(scheme, cols, bands, _lev(shape), w, tangent=tan)
    if scheme in CLOSED:
        assert plan.last_kernel().startswith("k_grad<"), plan.last_kernel()
    else:
        assert "k_jac_tri<" in plan.last_kernel() and "k_dlai_tri<" in plan.last_kernel(), plan.last_kernel()
    D, D2 = _oracle_reference(scheme, shape, uniform)
    wh = {k: v.cpu().numpy() for k, v in w.items()}
    ref = sum((wh[k] * D[k]).sum(axis=(1, 2)) for k in KEYS)
    ref2 = sum((wh[k] * D2[k]).sum(axis=(1, 2)) for k in KEYS)
    S = sum((np.abs(wh[k]) * np.abs(D[k])).sum(axis=(1, 2)) for k in KEYS)
    dr, dl, dg = _direction(shape, uniform)
    g = {k: v.cpu().numpy() for k, v in got.items()}
    val = sum((g[k] * dr[k]).sum(axis=1) for k in PARAMS) + g["lai"] * dl + g["leaf"] * dg
    guard, err = float(np.max(np.abs(ref2 - ref) / S)), float(np.max(np.abs(val - ref) / S))
    print(f"grad-vs-oracle {scheme} {_kind(shape)} {shape} {'uniform' if uniform else 'ragged'}: {err:.3e} of S (reference guard {guard:.3e})")
    assert np.all(np.abs(ref2 - ref) <= REF_GUARD * S), (scheme, shape, "the reference does not meet its own guard", guard)
    assert np.all(np.abs(val - ref) <= BOUND * S), (scheme, shape, err)


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", CLOSED)
def test_bitwise_invariants(scheme, uniform):
    import torch

    from crt1d_amd import _lib, batched

    for shape in GRAD_SHAPES:
        cols, bands, tan, w = _device(shape, uniform)
        lev = _lev(shape)
        _, full = _grad(scheme, cols, bands, lev, w, tangent=tan)
        # a column alone is its row of the batch
        for c in {0, shape[0] - 1}:
            _, one = _grad(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), lev, {k: v[c:c + 1].contiguous() for k, v in w.items()},
                           tangent=tan.slice(c, c + 1))
            for k in WRT:
                assert torch.equal(one[k][0], full[k][c]), (scheme, shape, c, k)
        # a subset of wrt has the bits of the full call, in any order
        for wrt in (("leaf",), ("lai",), ("soil_r", "leaf_r"), ("leaf_t", "lai"), ("leaf", "leaf_r")):
            _, sub = _grad(scheme, cols, bands, lev, w, wrt=wrt, tangent=tan if "leaf" in wrt else None)
            assert set(sub) == set(wrt)
            for k in wrt:
                assert torch.equal(sub[k], full[k]), (scheme, shape, wrt, k)
        # leaf without a tangent: along leaf_tangent(cols, "param")
        assert torch.equal(_grad(scheme, cols, bands, lev, w, wrt=("leaf",))[1]["leaf"], full["leaf"])
        # twice the weights, twice every bit
        _, twice = _grad(scheme, cols, bands, lev, {k: 2 * v for k, v in w.items()}, tangent=tan)
        for k in WRT:
            assert torch.equal(twice[k], 2 * full[k]), (scheme, shape, "doubling", k)
        # PRECOMPUTE_ONLY writes no output; SKIP_PRECOMPUTE on the workspace it filled gives the plain call's bits
        plan = batched.LevelsGradPlan(scheme, cols, bands, lev, w, tangent=tan)
        for v in plan.out.values():
            v.fill_(7.0)
        plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
        assert plan.last_kernel() == "k_colpre" + (" + k_dlai_side" if scheme == "bl" else "") + " + k_dleaf_side"
        for v in plan.out.values():
            assert bool((v == 7.0).all())
        got = plan(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in WRT:
            assert torch.equal(got[k], full[k]), (scheme, shape, "precompute only + skip precompute", k)
        # per="lai": the lai output divided by the column's total LAI
        _, per = _grad(scheme, cols, bands, lev, w, wrt=("lai",), per="lai")
        assert torch.equal(per["lai"], full["lai"] / cols.lai[:, 0])


def test_bl_has_no_soil_and_no_upward_stream():
    import torch

    shape = (3, 70, 60)
    cols, bands, tan, w = _device(shape, False)
    _, full = _grad("bl", cols, bands, _lev(shape), w, tangent=tan)
    assert bool((full["soil_r"] == 0).all())
    for other in ({k: v for k, v in w.items() if k != "I_df_u"}, {**w, "I_df_u": torch.full_like(w["I_df_u"], float("nan"))}):
        _, got = _grad("bl", cols, bands, _lev(shape), other, tangent=tan)
        for k in WRT:
            assert torch.equal(got[k], full[k]), k


@pytest.mark.parametrize("scheme", SCHEMES)
def test_graph_replay(scheme):
    """One replay of a captured plan equals the direct call (single stream, after a first call outside the capture)."""
    import torch

    from crt1d_amd import batched

    shape = (3, 70, 60)
    cols, bands, tan, w = _device(shape, True)
    plan = batched.LevelsGradPlan(scheme, cols, bands, _lev(shape), w, tangent=tan)
    ref = {k: v.clone() for k, v in plan().items()}
    torch.cuda.synchronize()  # (the side stream below writes the same buffers)
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
    for k in WRT:
        assert torch.equal(plan.out[k], ref[k]), k


def test_shared_spectra_equal_replicated_spectra():
    """col_stride == 0: one set of spectra for all columns gives, row by row, the bits of a batch that repeats them per column."""
    import torch

    from crt1d_amd import batched, synth

    shape = (5, 70, 20)
    d = synth.make_columns(*shape, seed=11, per_column_optics=False)
    cols, shared = batched.Columns.from_host(d), batched.Bands.from_host(d)
    assert shared.col_stride(shape[0]) == 0
    rep = batched.Bands(*[getattr(shared, k).expand(shape[0], -1).contiguous() for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
    rng = np.random.default_rng(3)
    w = {k: torch.as_tensor(rng.uniform(-1, 1, (5, 3, 70))).cuda() for k in KEYS}
    for scheme in SCHEMES:
        a = _grad(scheme, cols, shared, (0, 7, 19), w)[1]
        b = _grad(scheme, cols, rep, (0, 7, 19), w)[1]
        for k in WRT:
            assert a[k].shape == ((5, 70) if k in PARAMS else (5,))
            assert torch.equal(a[k], b[k]), (scheme, k)
            assert bool(a[k].isfinite().all())


@pytest.mark.parametrize("scheme", ["n79", "zq", "4s", "zq_pa"])
def test_refused_on_the_device(scheme):
    """CRT_ERR_UNSUPPORTED through the C entry with a whole set of valid device arguments: outputs and workspace untouched."""
    import torch

    from crt1d_amd import _lib

    shape = (3, 70, 60)
    cols, bands, tan, w = _device(shape, True)
    lev = _lev(shape)
    sentinel = 3.25
    out = {k: torch.full((3, 70) if k in PARAMS else (3,), sentinel, dtype=torch.float64, device="cuda") for k in WRT}
    ws = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    c, b, o = cols.c_struct(), bands.c_struct(3), _lib.CrtOptions(0.501, 0, 0)
    cw, co, tn = _lib.CrtGradWeights(*[w[k].data_ptr() for k in KEYS]), _lib.CrtGradOut(*[out[k].data_ptr() for k in WRT]), tan.c_struct()
    arr = (ctypes.c_int32 * len(lev))(*lev)
    st = lib.crt_hip_levels_grad_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), arr, len(lev), ctypes.byref(cw),
                                     ctypes.byref(tn), ctypes.byref(co), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == sentinel).all())
    assert bool((ws == 0).all())


# ------------------------------------------------------------------------------------------------------------------
def _ad_inputs(shape, uniform, shared=False):
    """Leaves that require grad on top of the generator's columns: the three optics, lai_scale, g_param."""
    import torch

    from crt1d_amd import batched

    d = _host_kind(shape, uniform, _kind(shape))
    t = lambda v: torch.as_tensor(v).cuda()  # noqa: E731
    leaf = {k: (t(d[k][0]) if shared else t(d[k])).requires_grad_() for k in PARAMS}
    scale = t(np.random.default_rng(5).uniform(0.8, 1.25, shape[0])).requires_grad_()
    gp = t(d["g_param"]).requires_grad_()
    cols = batched.Columns(t(d["psi"]), t(d["lai"]), t(d["g_kind"]), gp, t(d["mla"]))
    I0 = (t(d["I_dr0"][0]), t(d["I_df0"][0])) if shared else (t(d["I_dr0"]), t(d["I_df0"]))
    bands = batched.Bands(*I0, leaf["leaf_r"], leaf["leaf_t"], leaf["soil_r"])
    return cols, bands, leaf, scale, gp


@pytest.mark.parametrize("shared", [False, True], ids=["per-column", "shared"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_autograd_forward_and_backward_bits(scheme, shared):
    import torch

    from crt1d_amd import batched

    shape = (3, 70, 60)
    lev = _lev(shape)
    _, _, _, w = _device(shape, False)
    cols, bands, leaf, scale, gp = _ad_inputs(shape, False, shared)
    # forward: bitwise solve_levels
    plain = batched.solve_levels(scheme, cols, bands, lev)
    out = batched.solve_levels_ad(scheme, cols, bands, lev)
    for k in KEYS:
        assert torch.equal(out[k], plain[k]) and out[k].requires_grad, k
    # with lai_scale: solve_levels on the scaled columns
    scaled = batched.Columns(cols.psi, cols.lai.detach() * scale.detach()[:, None], cols.g_kind, gp.detach(), cols.mla)
    plain = batched.solve_levels(scheme, scaled, bands, lev)
    out = batched.solve_levels_ad(scheme, cols, bands, lev, lai_scale=scale)
    for k in KEYS:
        assert torch.equal(out[k], plain[k]), k
    sum((w[k] * out[k]).sum() for k in KEYS).backward()
    ref = batched.solve_levels_grad(scheme, scaled, bands, lev, w)
    torch.cuda.synchronize()
    for k in PARAMS:
        want = ref[k].sum(0) if shared else ref[k]  # shared spectra: the sum over the columns
        assert leaf[k].grad.shape == leaf[k].shape and torch.equal(leaf[k].grad, want), k
    assert torch.equal(scale.grad, ref["lai"] / scale.detach())
    assert torch.equal(gp.grad, ref["leaf"])
    # only what requires grad is formed: a subset gives the same bits, a second backward is refused
    cols2, bands2, leaf2, scale2, _ = _ad_inputs(shape, False, shared)
    leaf2["leaf_t"].requires_grad_(False)
    cols2.g_param.requires_grad_(False)
    out = batched.solve_levels_ad(scheme, cols2, bands2, lev, keys=("F", "I_df_u"), lai_scale=scale2)
    assert set(out) == {"F", "I_df_u"}
    loss = (w["F"] * out["F"]).sum() + (w["I_df_u"] * out["I_df_u"]).sum()
    loss.backward()
    ref = batched.solve_levels_grad(scheme, scaled, bands, lev, {k: w[k] for k in ("I_df_u", "F")}, wrt=("leaf_r", "soil_r", "lai"))
    assert torch.equal(leaf2["leaf_r"].grad, ref["leaf_r"].sum(0) if shared else ref["leaf_r"])
    assert leaf2["leaf_t"].grad is None and cols2.g_param.grad is None
    assert torch.equal(scale2.grad, ref["lai"] / scale2.detach())
    with pytest.raises(ValueError, match="I_dr0 requires grad"):
        batched.solve_levels_ad(scheme, cols, batched.Bands(bands.I_dr0.clone().requires_grad_(), bands.I_df0, bands.leaf_r, bands.leaf_t, bands.soil_r), lev)


@pytest.mark.parametrize("scheme", ["2s", "bl", "g77", "bf"])
def test_gradcheck(scheme):
    """torch.autograd.gradcheck at its default tolerances on (ncol, nb, nz) = (2, 5, 4), with respect to the optics and lai_scale."""
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(2, 5, 4, seed=11, uniform_dlai=False)
    t = lambda v: torch.as_tensor(v).cuda()  # noqa: E731
    cols = batched.Columns(t(d["psi"]), t(d["lai"]), t(d["g_kind"]), t(d["g_param"]), t(d["mla"]))
    I_dr0, I_df0 = t(d["I_dr0"]), t(d["I_df0"])

    def f(leaf_r, leaf_t, soil_r, lai_scale):
        bands = batched.Bands(I_dr0, I_df0, leaf_r, leaf_t, None if scheme == "bl" else soil_r)
        out = batched.solve_levels_ad(scheme, cols, bands, (0, 2, 3), lai_scale=lai_scale)
        return tuple(out[k] for k in KEYS)

    leaves = [t(d[k]).requires_grad_() for k in PARAMS] + [t(np.array([0.9, 1.1])).requires_grad_()]
    if scheme == "bl":
        leaves[2].requires_grad_(False)  # (not an input of the graph)
    assert torch.autograd.gradcheck(f, leaves)


def test_sensor_misfit_backpropagates():
    """A squared sensor misfit built from SensorSet.dense and einsum: .grad against sensor_jvp (a unit direction per band), sensor_dlai and
    sensor_dleaf contracted by hand with the residuals in np.longdouble.  Every term is residual * sensor weight * tangent, T[c, r, s, b]
    per quantity: both sides add them in their own grouping, each with an error chain far shorter than the n terms, so the bound of test 1
    holds with n their number and S their sum of magnitudes.  Measured on MI355X, |grad - by hand| / (2 n u S): optics 0.047, lai 4.3e-4,
    leaf 8.5e-4."""
    import torch

    from crt1d_amd import batched, spectra

    shape, uniform, scheme = (3, 70, 60), False, "2s"
    d = _host_kind(shape, uniform, _kind(shape))
    cols, bands, leaf, scale, gp = _ad_inputs(shape, uniform)
    with torch.no_grad():
        scale.fill_(1.0)
    lev = (0, shape[2] - 1)
    W = spectra.boxcar_sensor_weights(d["wle"], [(0.4, 0.5), (0.5, 0.7), (0.7, 1.0), (1.0, 1.8), (0.3, 2.6)])
    sensors = batched.SensorSet(W, device=cols.device)
    Wd = torch.as_tensor(sensors.dense(shape[1])).to(cols.device)
    qk = ("I_df_u", "F")
    out = batched.solve_levels_ad(scheme, cols, bands, lev, keys=qk, lai_scale=scale)
    sums = {k: torch.einsum("crb,sb->crs", out[k], Wd) for k in qk}
    obs = {k: 0.9 * sums[k].detach() + 0.01 for k in qk}
    sum(((sums[k] - obs[k]) ** 2).sum() for k in qk).backward()
    torch.cuda.synchronize()
    R = {k: (2 * (sums[k].detach() - obs[k])).cpu().numpy().astype(np.longdouble) for k in qk}  # d loss / d sums (ncol, nsel, nsens)
    plain = batched.Bands(bands.I_dr0, bands.I_df0, *[leaf[k].detach() for k in PARAMS])
    pcols = batched.Columns(cols.psi, cols.lai, cols.g_kind, gp.detach(), cols.mla)
    eye = torch.eye(shape[1], dtype=torch.float64)
    n_opt, n_col = len(qk) * len(lev) * W.shape[0], len(qk) * len(lev) * W.shape[0] * shape[1]
    absW = np.abs(sensors.dense(shape[1])).astype(np.longdouble)
    J = {k: v.cpu().numpy() for k, v in batched.solve_levels_jac(scheme, pcols, plain, lev, keys=qk).items()}
    worst = {}
    for p, name in enumerate(PARAMS):
        dirs = [eye if i == p else None for i in range(3)]
        jv = batched.sensor_jvp(scheme, pcols, plain, lev, sensors, *dirs, keys=qk)  # [c, r, s, b] = w_s[b] J_p[c, r, b]
        want = sum(np.einsum("crs,crsb->cb", R[k], jv[k].cpu().numpy().astype(np.longdouble)) for k in qk)
        S = sum(np.einsum("crs,sb,crb->cb", np.abs(R[k]), absW, np.abs(J[k][:, :, p, :]).astype(np.longdouble)) for k in qk)
        err = np.abs(leaf[name].grad.cpu().numpy() - want)
        worst[name] = float(np.max(err / (2 * n_opt * U * S)))
        assert np.all(err <= 2 * n_opt * U * S), (name, worst[name])
    tan = batched.leaf_tangent(pcols, "param")
    for name, got, sd, D in (("lai", scale.grad, batched.sensor_dlai(scheme, pcols, plain, lev, sensors, keys=qk),
                              batched.solve_levels_dlai(scheme, pcols, plain, lev, keys=qk)),
                             ("leaf", gp.grad, batched.sensor_dleaf(scheme, pcols, plain, lev, tan, sensors, keys=qk),
                              batched.solve_levels_dleaf(scheme, pcols, plain, lev, tan, keys=qk))):
        want = sum(np.einsum("crs,crs->c", R[k], sd[k].cpu().numpy().astype(np.longdouble)) for k in qk)
        S = sum(np.einsum("crs,sb,crb->c", np.abs(R[k]), absW, np.abs(D[k].cpu().numpy()).astype(np.longdouble)) for k in qk)
        err = np.abs(got.cpu().numpy() - want)
        worst[name] = float(np.max(err / (2 * n_col * U * S)))
        assert np.all(err <= 2 * n_col * U * S), (name, worst[name])
    print("sensor misfit, |grad - by hand| / (2 n u S): " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_model_run_gradient():
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=60)
    J = m.run_jacobian()
    A = m.run_lai_sensitivity()
    B = m.run_leaf_angle_sensitivity()
    rng = np.random.default_rng(1)
    w = {k: rng.uniform(-1, 1, (2, 107)) for k in KEYS}
    g = m.run_gradient(w)
    assert set(g) == set(WRT) and g["leaf_r"].shape == (107,) and isinstance(g["lai"], float)
    ld = np.longdouble
    for p, name in enumerate(PARAMS):
        terms = [w[k].astype(ld) * J[k][:, p, :].astype(ld) for k in JAC_KEYS]
        assert np.all(np.abs(g[name] - sum(t.sum(0) for t in terms)) <= 2 * 6 * U * sum(np.abs(t).sum(0) for t in terms)), name
    for name, D in (("lai", A), ("leaf", B)):
        terms = [w[k].astype(ld) * D[k].astype(ld) for k in KEYS]
        assert abs(g[name] - sum(t.sum() for t in terms)) <= 2 * 8 * 107 * U * sum(np.abs(t).sum() for t in terms), name
    assert set(m.run_gradient({"F": w["F"][1:]}, levels=(-1,), wrt=("lai", "soil_r"))) == {"lai", "soil_r"}
    with pytest.raises(ValueError, match="has no gradient"):
        Model("4s", nlayers=60).run_gradient(w)
