"""GPU: the Jacobian of the sensor-band sums in one kernel (crt_hip_sensor_jac_f64, batched.SensorJacPlan), gauss_newton_step and
Model.run_sensor_jacobian on top of it.

1. Against the composition it replaces: the arrays of solve_levels_jac, solve_levels_dlai and solve_levels_dleaf folded on the host in
   np.longdouble with the dense sensor weights and the directions.  The kernel multiplies and adds the same tangent bits (the same
   jac_schemes.hpp instantiations, -ffp-contract=off); only the products and the order of the sums differ, so the bounds are derived, not
   measured.  LAI and leaf-angle columns: |g - ref| <= 2 n u S, n the bands of the support, u = 2^-53, S = sum_b |w_s[b]| |X'| (one
   rounding per product, recursive summation of n terms in any order, doubled for the higher-order terms).  Direction columns:
   |g - ref| <= 2 (3 n + 1) u S with S = sum_b |w_s[b]| sum_p |J_p| |d_p|: 3 n terms of two roundings each, summed in any order.
2. End to end against the oracle, one parameter column at a time: the Richardson-extrapolated central difference of the oracle's sensor
   sums along that parameter, constants and reference-guard convention of tests/test_gpu_grad.py: 1e-6 of S, asserted after the
   reference's own h against h / 2 guard (1e-7); S is the column's sum of |w_s[b]| |dX / d delta| over keys, levels, sensor bands and bands,
   every element of the column is held to it.  All six schemes (n79, zq: the composed path).
3. Bitwise invariants: batch, keys, dropped parameter columns, shared directions, doubled weights, the precompute flags, the forward
   sums on the plan's workspace, graph replay, bl, I_dr.
4. Refusals on the device: n79, zq, 4s, zq_pa and a configuration beyond the LDS through the C entry.
5. A noise-free retrieval by damped Gauss-Newton steps, against the same loop on the composed Jacobian; Model.run_sensor_jacobian."""
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
# (ncol, nb, nz): those of the Jacobian tests; two band slices of 256 lanes with the last one partial (257 = 129 + 128, 300 = 150 + 150)
SJ_SHAPES = list(SHAPES) + [(2, 257, 4), (2, 300, 5)]
U = 2.0 ** -53
REF_GUARD, BOUND = 1e-7, 1e-6


def _lev(shape):
    """At most 16 of the levels of the Jacobian tests, the ground and the top among them: with 5 parameters a level takes 15 staging rows,
    so that 5 levels run 256-lane slices, 9 levels 128-lane slices and 16 levels 64-lane slices (70 bands: 35 + 35, 130: 44 + 43 + 43)."""
    lv = _levels(shape[2])
    if len(lv) > 16:
        lv = tuple(sorted(set(lv[::-(-len(lv) // 15)]) | {shape[2] - 1}))
    assert len(lv) <= 16
    return lv


def _slices(nb, nsel, npar):
    """(nslice, per) of k_sens_jac, the launcher's arithmetic: the widest of 256, 128, 64 lanes whose nsel * max(3 npar, 4) staging rows
    of doubles fit 160 KB less 4 KB; balanced slices."""
    w = 256
    while nsel * max(3 * npar, 4) * w * 8 > 160 * 1024 - 4096:
        w //= 2
    assert w >= 64
    nslice = -(-nb // w)
    return nslice, -(-nb // nslice)


def _kind(shape):
    return list(KINDS)[SJ_SHAPES.index(shape) % 3]  # every parametric leaf-angle kind is met


def _ntan(shape):
    return 3 if SJ_SHAPES.index(shape) % 2 == 0 else 1


@functools.lru_cache(maxsize=None)
def _supports(shape, ntan=None, single=False):
    """(first, count) of the 5-band set: all bands | one band | a support straddling the first slice boundary | one wholly in the second
    slice | one overlapping the others (one slice: the same shapes about the middle of the bands).  single: one sensor band."""
    nb = shape[1]
    if single:
        f = nb // 5
        return (f,), (max(nb - nb // 7 - f, 1),)
    nslice, per = _slices(nb, len(_lev(shape)), (_ntan(shape) if ntan is None else ntan) + 2)
    edge = per if nslice > 1 else nb // 2
    spans = [(0, nb), (nb // 3, nb // 3 + 1), (edge - 2, edge + 3), (edge + 1, edge + 5), (nb // 4, nb // 4 + nb // 2)]
    first, count = [], []
    for lo, hi in spans:
        lo = min(max(lo, 0), nb - 1)
        hi = min(max(hi, lo + 1), nb)
        first.append(lo)
        count.append(hi - lo)
    return tuple(first), tuple(count)


@functools.lru_cache(maxsize=None)
def _sensors(shape, single=False):
    from crt1d_amd import batched

    first, count = _supports(shape, single=single)
    w = np.random.default_rng(29).uniform(-1.0, 1.0, int(np.sum(count)))
    return batched.SensorSet.from_supports(np.array(first), np.array(count), w, nb=shape[1])


@functools.lru_cache(maxsize=None)
def _host_dirs(shape, uniform, ntan, shared):
    """Directions in the three spectra, relative to the spectra themselves (a step of 3e-3 keeps them physical)."""
    d = _host_kind(shape, uniform, _kind(shape))
    rng = np.random.default_rng(31)
    out = {}
    for k in PARAMS:
        base = d[k].mean(axis=0, keepdims=True) if shared else d[k]
        out[k] = rng.uniform(-1.0, 1.0, (base.shape[0], ntan, shape[1])) * base[:, None, :]
    return out


@functools.lru_cache(maxsize=None)
def _device(shape, uniform):
    import torch

    from crt1d_amd import batched

    d = _host_kind(shape, uniform, _kind(shape))
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param")
    torch.cuda.synchronize()
    return cols, bands, tan


def _dev_dirs(shape, uniform, ntan, shared):
    import torch

    d = _host_dirs(shape, uniform, ntan, shared)
    return {"d_" + k: torch.as_tensor(v[0] if shared else v).cuda() for k, v in d.items()}


def _jac(scheme, cols, bands, lev, sensors, **kw):
    import torch

    from crt1d_amd import batched

    plan = batched.SensorJacPlan(scheme, cols, bands, lev, sensors, **kw)
    got = plan()
    torch.cuda.synchronize()
    return plan, {k: v.clone() for k, v in got.items()}


@functools.lru_cache(maxsize=None)
def _tangents(scheme, shape, uniform):
    """What the three existing plans write, on the host: (J {key: (ncol, nsel, 3, nb)}, dlai, dleaf {key: (ncol, nsel, nb)})."""
    import torch

    from crt1d_amd import batched

    cols, bands, tan = _device(shape, uniform)
    lev = _lev(shape)
    J = batched.solve_levels_jac(scheme, cols, bands, lev)
    A = batched.solve_levels_dlai(scheme, cols, bands, lev)
    B = batched.solve_levels_dleaf(scheme, cols, bands, lev, tan)
    torch.cuda.synchronize()
    host = lambda d: {k: v.cpu().numpy() for k, v in d.items()}  # noqa: E731
    return host(J), host(A), host(B)


def _fold(scheme, shape, uniform, sensors, dirs):
    """{key: (ref, bound)} in np.longdouble, each (ncol, nsel, nsens, npar): the composition and the derived bound of every element."""
    J, A, B = _tangents(scheme, shape, uniform)
    ld = np.longdouble
    W = sensors.dense(shape[1]).astype(ld)  # (nsens, nb)
    n = np.asarray(sensors.count, dtype=ld)[None, None, :]
    ntan = next(iter(dirs.values())).shape[1]
    out = {}
    for k in KEYS:
        ref, bound = [], []
        if k in JAC_KEYS:
            T = sum(J[k][:, :, p, None, :].astype(ld) * dirs[name][:, None, :, :].astype(ld) for p, name in enumerate(PARAMS))
            Ta = sum(np.abs(J[k][:, :, p, None, :]).astype(ld) * np.abs(dirs[name][:, None, :, :]).astype(ld) for p, name in enumerate(PARAMS))
            ref.append(np.einsum("crkb,sb->crsk", T, W))
            bound.append(2 * (3 * n[..., None] + 1) * U * np.einsum("crkb,sb->crsk", Ta, np.abs(W)))
        else:
            z = np.zeros((shape[0], len(_lev(shape)), sensors.nsens, ntan), dtype=ld)
            ref.append(z)
            bound.append(z)
        for D in (A, B):
            ref.append(np.einsum("crb,sb->crs", D[k].astype(ld), W)[..., None])
            bound.append((2 * n * U * np.einsum("crb,sb->crs", np.abs(D[k]).astype(ld), np.abs(W)))[..., None])
        out[k] = (np.concatenate(ref, axis=-1), np.concatenate(bound, axis=-1))
    return out


def _cases(schemes, shapes):
    for scheme in schemes:
        for shape in shapes:
            for uniform in (True, False):
                yield pytest.param(scheme, shape, uniform, id=f"{scheme}-{'x'.join(map(str, shape))}-{'uniform' if uniform else 'ragged'}")


@pytest.mark.parametrize("scheme,shape,uniform", _cases(CLOSED, SJ_SHAPES))
def test_against_the_composition(scheme, shape, uniform):
    """Every element within its derived bound.  ntan = 3 (shapes 0, 2, 4) or 1; directions per column (uniform) or shared (ragged); the
    5-band set and the 1-band set.  Measured on MI355X, worst |g - ref| / bound over the shapes and both sets: directions 2s 0.29, bl 0.25, g77
    0.31, bf 0.30; LAI and leaf angle 0.49 for every scheme, at the single-band supports (n = 1: the one product rounding, half an ulp, of the
    two roundings the bound allows) -- 0.11 at most for the 1-band set's support of 10 bands, below 0.01 from 46 bands on."""
    cols, bands, tan = _device(shape, uniform)
    lev, ntan, shared = _lev(shape), _ntan(shape), not uniform
    hd = _host_dirs(shape, uniform, ntan, shared)
    for single in (False, True):
        sensors = _sensors(shape, single)
        plan, got = _jac(scheme, cols, bands, lev, sensors, tangent=tan, **_dev_dirs(shape, uniform, ntan, shared))
        assert plan.params == tuple(f"dir{k}" for k in range(ntan)) + ("lai", "leaf")
        npar = ntan + 2
        nslice, per = _slices(shape[1], len(lev), npar)
        assert plan.last_kernel() == (f"k_sens_jac<{scheme}> nsel={len(lev)} nsens={sensors.nsens} npar={npar} slice={per}" +
                                      (" + k_sens_jac_finish" if nslice > 1 else ""))
        ref = _fold(scheme, shape, uniform, sensors, hd)
        worst = {"dir": 0.0, "lai/leaf": 0.0}
        bad = []
        for k in KEYS:
            g, (r, bound) = got[k].cpu().numpy(), ref[k]
            assert g.shape == r.shape == (shape[0], len(lev), sensors.nsens, npar) and np.isfinite(g).all(), k
            err = np.abs(g.astype(np.longdouble) - r)
            ratio = err / np.where(bound == 0, 1, bound)
            worst["dir"] = max(worst["dir"], float(ratio[..., :ntan].max()))
            worst["lai/leaf"] = max(worst["lai/leaf"], float(ratio[..., ntan:].max()))
            if not np.all(err <= bound):
                bad.append(k)
            if k == "I_dr":
                assert np.all(g[..., :ntan] == 0)
            elif scheme == "bl" and k == "I_df_u":
                assert np.all(g == 0)
            else:
                assert float(bound.max()) > 0, k
        print(f"sensjac-vs-composition {scheme} {shape} {'uniform' if uniform else 'ragged'} nsens={sensors.nsens}: |g - ref| / bound " +
              ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
        assert not bad, (scheme, shape, sensors.nsens, bad, worst)


# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _oracle_reference(scheme, shape, uniform, par):
    """(D, D2): the Richardson-extrapolated central differences at H and H / 2 of the oracle's level spectra {key: (ncol, nsel, nb)} along
    parameter column ``par``: 0 .. ntan - 1 a direction, "lai" the LAI scale, "leaf" g_param (relative; Bonan's chi_l: absolute)."""
    from oracle import crt_oracle as O

    d = _host_kind(shape, uniform, _kind(shape))
    dirs = _host_dirs(shape, uniform, _ntan(shape), not uniform)
    lev = list(_lev(shape))
    solve = getattr(O, f"solve_{scheme}")
    dg = np.ones(shape[0]) if _kind(shape) == "bonan" else d["g_param"]

    def f(delta):
        kw = {k: d[k] for k in ("I_dr0", "I_df0")}
        for k in ("leaf_r", "leaf_t") + (() if scheme == "bl" else ("soil_r",)):
            kw[k] = d[k] + (delta * dirs[k][:, par, :] if isinstance(par, int) else 0.0)
        lai = d["lai"] * (1 + delta) if par == "lai" else d["lai"]
        gp = d["g_param"] + delta * dg if par == "leaf" else d["g_param"]
        out = solve(O.Columns(d["psi"], lai, mla=d["mla"], g_kind=d["g_kind"], g_param=gp), **kw)
        return {k: out[k][:, lev, :] for k in KEYS}

    return _richardson(f, H)


@pytest.mark.parametrize("scheme,shape,uniform", _cases(SCHEMES, SJ_SHAPES[:2]))
def test_against_the_oracle(scheme, shape, uniform):
    """Every parameter column against d / d delta of the oracle's sensor sums: 1e-6 of S, after the reference agrees with its own h / 2
    estimate to 1e-7 of S.  Measured on MI355X, worst error (reference guard) over the columns: 2s 4.9e-12 (5.5e-12), bl
    4.6e-10 (4.3e-10), g77 2.4e-10 (2.2e-10), bf 1.6e-10 (1.5e-10), n79 2.3e-12 (2.2e-12), zq 2.6e-12 (2.4e-12) -- the differences are the
    reference's."""
    cols, bands, tan = _device(shape, uniform)
    lev, ntan, shared = _lev(shape), _ntan(shape), not uniform
    sensors = _sensors(shape)
    plan, got = _jac(scheme, cols, bands, lev, sensors, tangent=tan, **_dev_dirs(shape, uniform, ntan, shared))
    if scheme in CLOSED:
        assert plan.last_kernel().startswith(f"k_sens_jac<{scheme}>"), plan.last_kernel()
    else:
        assert "k_jac_tri<" in plan.last_kernel() and plan.last_kernel().count("k_dlai_tri<") == 2, plan.last_kernel()
    W = sensors.dense(shape[1])
    d = _host_kind(shape, uniform, _kind(shape))
    dg = np.ones(shape[0]) if _kind(shape) == "bonan" else d["g_param"]
    worst = [0.0, 0.0]
    for j, par in enumerate(list(range(ntan)) + ["lai", "leaf"]):
        D, D2 = _oracle_reference(scheme, shape, uniform, par)
        S = sum(np.einsum("crb,sb->c", np.abs(D[k]), np.abs(W)) for k in KEYS)[:, None, None]
        for k in KEYS:
            ref, ref2 = np.einsum("crb,sb->crs", D[k], W), np.einsum("crb,sb->crs", D2[k], W)
            val = got[k].cpu().numpy()[..., j] * (dg[:, None, None] if par == "leaf" else 1.0)
            worst = [max(worst[0], float(np.max(np.abs(val - ref) / S))), max(worst[1], float(np.max(np.abs(ref2 - ref) / S)))]
            assert np.all(np.abs(ref2 - ref) <= REF_GUARD * S), (scheme, shape, par, k, "the reference does not meet its own guard", worst[1])
            assert np.all(np.abs(val - ref) <= BOUND * S), (scheme, shape, par, k, worst[0])
    print(f"sensjac-vs-oracle {scheme} {_kind(shape)} {shape} {'uniform' if uniform else 'ragged'}: {worst[0]:.3e} of S (reference guard {worst[1]:.3e})")


# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", CLOSED)
def test_bitwise_invariants(scheme, uniform):
    import torch

    from crt1d_amd import _lib, batched

    for shape in SJ_SHAPES:
        cols, bands, tan = _device(shape, uniform)
        lev, ntan, sensors = _lev(shape), _ntan(shape), _sensors(shape)
        dirs = _dev_dirs(shape, uniform, ntan, False)
        _, full = _jac(scheme, cols, bands, lev, sensors, tangent=tan, **dirs)
        # a column alone is its row of the batch
        for c in {0, shape[0] - 1}:
            _, one = _jac(scheme, cols.slice(c, c + 1), bands.slice(c, c + 1), lev, sensors, tangent=tan.slice(c, c + 1),
                          **{k: v[c:c + 1].contiguous() for k, v in dirs.items()})
            for k in KEYS:
                assert torch.equal(one[k][0], full[k][c]), (scheme, shape, c, k)
        # a subset of keys has the bits of the full call, in any order
        for keys in (("F",), ("I_dr",), ("I_df_u", "I_df_d"), ("F", "I_dr", "I_df_d")):
            _, sub = _jac(scheme, cols, bands, lev, sensors, tangent=tan, keys=keys, **dirs)
            assert set(sub) == set(keys)
            for k in keys:
                assert torch.equal(sub[k], full[k]), (scheme, shape, keys, k)
        # dropping a parameter column leaves the bits of the others (the slices follow npar: compare where they are the same ones)
        for drop in ("leaf", "lai", "dirs", "lai+leaf"):
            kw = dict(tangent=None if "leaf" in drop else tan, lai="lai" not in drop, **({} if drop == "dirs" else dirs))
            plan, sub = _jac(scheme, cols, bands, lev, sensors, **kw)
            if _slices(shape[1], len(lev), len(plan.params)) != _slices(shape[1], len(lev), ntan + 2):
                continue
            idx = [("dir%d" % k if k < ntan else ("lai", "leaf")[k - ntan]) for k in range(ntan + 2)]
            for k in KEYS:
                for j, name in enumerate(plan.params):
                    assert torch.equal(sub[k][..., j], full[k][..., idx.index(name)]), (scheme, shape, drop, k, name)
        # shared directions are the same directions given per column
        sh = _dev_dirs(shape, uniform, ntan, True)
        _, a = _jac(scheme, cols, bands, lev, sensors, tangent=tan, **sh)
        _, b = _jac(scheme, cols, bands, lev, sensors, tangent=tan, **{k: v[None].expand(shape[0], -1, -1).contiguous() for k, v in sh.items()})
        for k in KEYS:
            assert torch.equal(a[k], b[k]), (scheme, shape, "shared directions", k)
        # twice the weights, twice every bit
        twice = batched.SensorSet.from_supports(sensors.first, sensors.count, 2 * sensors.w, nb=shape[1])
        _, two = _jac(scheme, cols, bands, lev, twice, tangent=tan, **dirs)
        for k in KEYS:
            assert torch.equal(two[k], 2 * full[k]), (scheme, shape, "doubling", k)
        # PRECOMPUTE_ONLY writes no output; SKIP_PRECOMPUTE on the workspace it filled gives the plain call's bits
        plan = batched.SensorJacPlan(scheme, cols, bands, lev, sensors, tangent=tan, **dirs)
        for v in plan.out.values():
            v.fill_(7.0)
        plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
        assert plan.last_kernel() == "k_colpre" + (" + k_dlai_side" if scheme == "bl" else "") + " + k_dleaf_side"
        for v in plan.out.values():
            assert bool((v == 7.0).all())
        got = plan(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(got[k], full[k]), (scheme, shape, "precompute only + skip precompute", k)
        # the forward sums on this plan's workspace, without a second column precompute, are those of a stand-alone plan
        alone = {k: v.clone() for k, v in batched.solve_sensor_levels(scheme, cols, bands, lev, sensors).items()}
        fwd = batched.SensorLevelsPlan(scheme, cols, bands, lev, sensors, workspace=plan.workspace)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in KEYS:
            assert torch.equal(fwd[k], alone[k]), (scheme, shape, "forward sums on the Jacobian's workspace", k)


def test_bl_has_no_soil_and_no_upward_stream():
    import torch

    shape = (3, 70, 60)
    cols, bands, tan = _device(shape, False)
    lev, sensors = _lev(shape), _sensors(shape)
    dirs = _dev_dirs(shape, False, 3, False)
    _, full = _jac("bl", cols, bands, lev, sensors, tangent=tan, **dirs)
    assert bool((full["I_df_u"] == 0).all())
    assert bool((full["I_dr"][..., :3] == 0).all()) and bool((full["I_dr"][..., 3:] != 0).any())
    for other in ({k: v for k, v in dirs.items() if k != "d_soil_r"}, {**dirs, "d_soil_r": torch.full_like(dirs["d_soil_r"], float("nan"))}):
        _, got = _jac("bl", cols, bands, lev, sensors, tangent=tan, **other)
        for k in KEYS:
            assert torch.equal(got[k], full[k]), k


@pytest.mark.parametrize("scheme", CLOSED)
def test_graph_replay(scheme):
    """One replay of a captured plan equals the direct call (single stream, after a first call outside the capture); 70 bands in two
    slices: the finish kernel is part of the graph."""
    import torch

    from crt1d_amd import batched

    shape = (3, 70, 60)
    cols, bands, tan = _device(shape, True)
    plan = batched.SensorJacPlan(scheme, cols, bands, _lev(shape), _sensors(shape), tangent=tan, **_dev_dirs(shape, True, 3, False))
    ref = {k: v.clone() for k, v in plan().items()}
    assert plan.last_kernel().endswith(" + k_sens_jac_finish")
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
    for k in KEYS:
        assert torch.equal(plan.out[k], ref[k]), k


def _c_call(scheme, shape, lev, ntan, with_tan=True):
    """The C entry with a whole set of valid device arguments, sentinel outputs and a zeroed workspace -> (status, outputs, workspace)."""
    import torch

    from crt1d_amd import _lib

    cols, bands, tan = _device(shape, True)
    sensors = _sensors(shape)
    npar = ntan + 1 + with_tan
    dirs = {k: torch.ones((ntan, shape[1]), dtype=torch.float64, device="cuda") for k in PARAMS}
    out = {k: torch.full((shape[0], len(lev), sensors.nsens, npar), 3.25, dtype=torch.float64, device="cuda") for k in KEYS}
    ws = torch.zeros(1 << 24, dtype=torch.uint8, device="cuda")
    lib = _lib.load()
    c, b, o = cols.c_struct(), bands.c_struct(shape[0]), _lib.CrtOptions(0.501, 0, 0)
    cs, cd = sensors.c_struct(), _lib.CrtOpticsDirs(ntan, 0, *[dirs[k].data_ptr() for k in PARAMS])
    co, tn = _lib.CrtSensJacOut(*[out[k].data_ptr() for k in KEYS]), tan.c_struct()
    arr = (ctypes.c_int32 * len(lev))(*lev)
    st = lib.crt_hip_sensor_jac_f64(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), arr, len(lev), ctypes.byref(cs),
                                    ctypes.byref(cd), 1, ctypes.byref(tn) if with_tan else None, ctypes.byref(co), ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, out, ws


@pytest.mark.parametrize("scheme", ["n79", "zq", "4s", "zq_pa"])
def test_refused_on_the_device(scheme):
    """CRT_ERR_UNSUPPORTED through the C entry with a whole set of valid device arguments: outputs and workspace untouched."""
    from crt1d_amd import _lib

    st, out, ws = _c_call(scheme, (3, 70, 60), _lev((3, 70, 60)), 3)
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == 3.25).all())
    assert bool((ws == 0).all())


@pytest.mark.parametrize("scheme", CLOSED)
def test_refused_beyond_the_lds(scheme):
    """The launcher's arithmetic: nsel * max(3 npar, 4) staging rows of 64 doubles within 160 KB less 4 KB, 312 rows.  npar = 5: 15 rows per
    level, 20 levels (300 rows) are served, 21 (315) refused before K0 -- nothing is written."""
    from crt1d_amd import _lib

    shape = (3, 70, 60)
    assert 20 * 15 * 64 * 8 <= 160 * 1024 - 4096 < 21 * 15 * 64 * 8
    st, out, ws = _c_call(scheme, shape, tuple(range(21)), 3)
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for v in out.values():
        assert bool((v == 3.25).all())
    assert bool((ws == 0).all())
    st, out, ws = _c_call(scheme, shape, tuple(range(20)), 3)
    assert st == _lib.CRT_OK
    for k, v in out.items():
        assert bool(v.isfinite().all()) and bool((v[..., 3:] != 3.25).all()), k


# ------------------------------------------------------------------------------------------------------------------
NITER = 14


def _retrieval(jacobian):
    """Damped Gauss-Newton on a noise-free problem: 2s, 4 columns, 30 bands, 12 levels, the upwelling sums of 5 sensor bands at the top of
    the canopy; unknowns ln(LAI scale), the ellipsoidal x, one leaf-reflectance coefficient.  A step that raises a column's misfit is rejected and that column's damping raised.  -> (misfit history (niter + 1,
    ncol), parameter error)."""
    import torch

    from crt1d_amd import batched, synth

    ncol, nb, nz = 4, 30, 12
    d = synth.make_columns(ncol, nb, nz, seed=5)
    t = lambda v: torch.as_tensor(v).cuda()  # noqa: E731
    rng = np.random.default_rng(41)
    x_true = t(rng.uniform(0.7, 2.0, ncol))
    dirn = t(0.3 * d["leaf_r"].mean(axis=0) * np.sin(np.linspace(0.0, 3.0, nb)))  # (nb,): one shared direction in leaf_r
    truth = torch.stack((t(rng.uniform(-0.2, 0.2, ncol)), t(rng.uniform(-0.2, 0.2, ncol)), x_true), dim=1)  # a, ln LAI scale, x
    kind = torch.full((ncol,), KINDS["ellipsoidal"], dtype=torch.int32, device="cuda")
    w = np.zeros((5, nb))
    for s in range(5):
        w[s, 6 * s:6 * s + 8] = np.hanning(10)[1:9][: nb - 6 * s]
    sensors = batched.SensorSet(w)
    lev, keys = (nz - 1,), ("I_df_u",)

    def inputs(p):
        cols = batched.Columns(t(d["psi"]), t(d["lai"]) * torch.exp(p[:, 1])[:, None], kind, p[:, 2].contiguous(), t(d["mla"]))
        bands = batched.Bands(t(d["I_dr0"]), t(d["I_df0"]), t(d["leaf_r"]) + p[:, 0, None] * dirn, t(d["leaf_t"]), t(d["soil_r"]))
        return cols, bands

    def forward(p):
        o = batched.solve_sensor_levels("2s", *inputs(p), lev, sensors, keys=keys)
        return o["I_df_u"][:, 0]  # (ncol, 5)

    y = forward(truth).clone()
    p = torch.stack((torch.zeros(ncol, dtype=torch.float64, device="cuda"),) * 2 + (torch.full((ncol,), 1.2, dtype=torch.float64, device="cuda"),), dim=1)
    lam = torch.full((ncol,), 1e-2, dtype=torch.float64, device="cuda")
    r = forward(p) - y
    hist = [(r * r).sum(1)]
    for _ in range(NITER):
        cols, bands = inputs(p)
        Jm = jacobian(cols, bands, lev, sensors, dirn, keys)["I_df_u"][:, 0]  # (ncol, 5, 3)
        trial = p + batched.gauss_newton_step(Jm, r, damping=lam)
        trial[:, 2] = trial[:, 2].clamp(0.2, 5.0)
        rt = forward(trial) - y
        better = (rt * rt).sum(1) < hist[-1]
        p = torch.where(better[:, None], trial, p)
        r = torch.where(better[:, None], rt, r)
        lam = torch.where(better, lam / 10, lam * 10)
        hist.append((r * r).sum(1))
    torch.cuda.synchronize()
    return torch.stack(hist).cpu().numpy(), float((p - truth).abs().max())


def test_retrieval_by_gauss_newton_steps():
    """The misfit never increases, and the loop on the fused Jacobian ends no further than 10 x from the truth than the identical loop on
    the Jacobian composed of sensor_jvp, sensor_dlai and sensor_dleaf: both converge to rounding level, where the last digits
    fluctuate.  Measured on MI355X, largest parameter error after 14 steps: fused 1.4e-13, composed 9.5e-14; largest column
    misfit 5.8e-01 -> 7.0e-29 (composed 2.6e-28)."""
    import torch

    from crt1d_amd import batched

    def fused(cols, bands, lev, sensors, dirn, keys):
        return batched.sensor_jacobian("2s", cols, bands, lev, sensors, d_leaf_r=dirn[None], tangent=batched.leaf_tangent(cols, "param"), keys=keys)

    def composed(cols, bands, lev, sensors, dirn, keys):
        a = batched.sensor_jvp("2s", cols, bands, lev, sensors, dirn[None], None, None, keys=keys)
        b = batched.sensor_dlai("2s", cols, bands, lev, sensors, keys=keys)
        c = batched.sensor_dleaf("2s", cols, bands, lev, batched.leaf_tangent(cols, "param"), sensors, keys=keys)
        return {k: torch.cat([a[k], b[k][..., None], c[k][..., None]], dim=-1) for k in keys}

    hf, ef = _retrieval(fused)
    hc, ec = _retrieval(composed)
    print(f"retrieval: parameter error fused {ef:.3e}, composed {ec:.3e}; misfit {hf[0].max():.3e} -> {hf[-1].max():.3e} (composed {hc[-1].max():.3e})")
    assert np.all(hf[1:] <= hf[:-1]) and np.all(hc[1:] <= hc[:-1])
    assert hf[-1].max() < 1e-12 * hf[0].max()  # (it did converge)
    assert ef <= 10 * ec, (ef, ec)


def test_model_run_sensor_jacobian():
    """Model.run_sensor_jacobian is the batched call on the model's own column: bitwise."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.model import Model

    m = Model("2s", nlayers=60)
    nb = m.nwl
    w = np.zeros((3, nb))
    w[0, : nb // 2], w[1, nb // 3:], w[2, nb // 2] = 1.0, 0.5, 2.0
    d = np.random.default_rng(3).uniform(-0.1, 0.1, (2, nb))
    got = m.run_sensor_jacobian(w, levels=(0, -1), directions={"leaf_r": d, "soil_r": 2 * d}, lai=True, wrt_leaf="param")
    assert got["params"] == ("dir0", "dir1", "lai", "leaf")
    scheme, cols, b, sun = m._series_inputs(np.atleast_1d(float(m._p["psi"])), None, None, "sensor Jacobian")
    cols = batched.Columns(psi=sun.psi[:, 0].contiguous(), lai=cols.lai, g_kind=cols.g_kind, g_param=cols.g_param, mla=cols.mla,
                           g_at_psi=None if sun.g_at_psi is None else sun.g_at_psi[:, 0].contiguous(), g_table=cols.g_table)
    b = batched.Bands(sun.I_dr0[:, 0].contiguous(), sun.I_df0[:, 0].contiguous(), b.leaf_r, b.leaf_t, b.soil_r)
    ref = batched.sensor_jacobian("2s", cols, b, (0, -1), batched.SensorSet(w), d_leaf_r=d, d_soil_r=2 * d, tangent=batched.leaf_tangent(cols, "param"))
    torch.cuda.synchronize()
    for k in KEYS:
        assert got[k].shape == (2, 3, 4) and np.array_equal(got[k], ref[k][0].cpu().numpy()), k
    assert m.run_sensor_jacobian(w, lai=True)["params"] == ("lai",)
    with pytest.raises(ValueError, match="has no sensor Jacobian"):
        Model("4s", nlayers=60).run_sensor_jacobian(w)
