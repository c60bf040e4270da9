"""f32 storage past the solve: the epilogue (``crt_hip_absorb_f32``, ``crt_hip_absorb_bandsum{,2}_f32``) and the fused integrated path
(``crt_hip_integrated{,2}_f32``) read float spectra and profiles and do fp64 arithmetic.  Every check feeds float-representable values to
the f32 entry point and the same values, upcast, to its f64 twin: the band sums must be the same bits (the kernel choice, and with it the
order of every band reduction, depends on the shape only), the per-band absorption the f64 result rounded once."""
import ctypes

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
SPEC = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")
PROF = ("I_dr", "I_df_d", "I_df_u")


def _case(ncol, nb, nz, *, uniform=True, seed=21, per_column_optics=True):
    """Columns (fp64), float32 bands and the same bands upcast to float64."""
    from crt1d_amd import batched, synth

    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform, per_column_optics=per_column_optics)
    cols = batched.Columns.from_host(d)
    b32 = batched.Bands.from_host({k: (d[k].astype(np.float32) if k in SPEC else d[k]) for k in d})
    b64 = batched.Bands(*[t.double() for t in (b32.I_dr0, b32.I_df0, b32.leaf_r, b32.leaf_t, b32.soil_r)])
    return cols, b32, b64


def _weights(torch, ngroup, nb, seed=3):
    rng = np.random.default_rng(seed + ngroup)
    return torch.as_tensor(rng.uniform(0.0, 1.0, (ngroup, nb))).cuda()


def _profiles(scheme, cols, b64):
    """The f64 solve's profiles rounded to float (what the f32 solve writes, tests/test_gpu_dropin.py::test_f32_storage_variant) and the
    same values upcast."""
    from crt1d_amd import batched

    sol = batched.solve(scheme, cols, b64)
    p32 = {k: sol[k].float() for k in PROF}
    return p32, {k: v.double() for k, v in p32.items()}


# (ncol, nb, nz, uniform ΔLAI): the band-sum kernel forms -- one wave per column (300, 107), lanes over layers (40, profiles off), a
# column per half wave (12, 6: profiles off), a workgroup per column with 1024-band launches (1500)
BANDSUM_SHAPES = [(5, 300, 60, True), (5, 107, 61, False), (7, 40, 20, True), (7, 12, 20, True), (5, 6, 20, False), (3, 1500, 30, True)]


@pytest.mark.parametrize("shape", BANDSUM_SHAPES, ids=lambda s: "x".join(map(str, s[1:3])) + ("" if s[3] else "-ragged"))
@pytest.mark.parametrize("scheme", SCHEMES)
def test_bandsum_f32_is_bitwise_f64_of_upcast(scheme, shape):
    import torch

    from crt1d_amd import batched

    ncol, nb, nz, uniform = shape
    cols, b32, b64 = _case(ncol, nb, nz, uniform=uniform)
    p32, p64 = _profiles(scheme, cols, b64)
    for ngroup in (1, 3, 4):
        w = _weights(torch, ngroup, nb)
        for profiles in (False, True):
            r32 = batched.absorb_bandsum(cols, b32, p32, w, profiles=profiles)
            r64 = batched.absorb_bandsum(cols, b64, p64, w, profiles=profiles)
            keys = batched.BANDSUM_KEYS + (batched.PROFILE_KEYS if profiles else ())
            assert set(r32) == set(keys)
            for k in keys:
                assert r32[k].dtype == torch.float64
                assert torch.equal(r32[k], r64[k]), (k, ngroup, profiles)


@pytest.mark.parametrize("shape", [(5, 300, 60), (5, 107, 61), (4, 30, 20), (4, 40, 20), (3, 1500, 30)], ids=lambda s: f"{s[1]}x{s[2]}")
@pytest.mark.parametrize("shared_optics", [False, True])
def test_absorb_f32_is_rounded_f64(shape, shared_optics):
    """Per-band absorption: the seven arrays are the f64 result rounded to float, bit for bit; laim and f_slm are the f64 values.
    nb = 300, 40: the 16-byte (four-float) tile kernel; 107, 30: the per-band kernel for float, the tile kernel for double (no reduction:
    the choice cannot change a value)."""
    import torch

    from crt1d_amd import batched

    ncol, nb, nz = shape
    cols, b32, b64 = _case(ncol, nb, nz, seed=4, per_column_optics=not shared_optics)
    p32, p64 = _profiles("2s", cols, b64)
    a32 = batched.absorb(cols, b32, p32)
    a64 = batched.absorb(cols, b64, p64)
    for k in batched.ABSORPTION_KEYS:
        assert a32[k].dtype == torch.float32 and a32[k].shape == (ncol, nz - 1, nb)
        assert torch.equal(a32[k], a64[k].float()), k
    for k in ("laim", "f_slm"):
        assert a32[k].dtype == torch.float64
        assert torch.equal(a32[k], a64[k]), k


def _family(name):
    """Kernel name without the storage tag and the configuration: 'k_int<2s>', 'k_tri_int<n79>', 'k_zqpa_int<zq_pa>'."""
    return name.split(" ")[0]


INT_SHAPES = [(5, 300, 60), (4, 107, None), (3, 300, 150), (4, 64, 13), (3, 33, 7)]


@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: f"{s[1]}x{s[2] or 'min'}")
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("profiles", [False, True])
def test_integrated_f32_equals_f64_of_upcast(scheme, shape, profiles):
    """The fused path on float spectra == on the upcast spectra: bitwise when both calls ran the same kernel family (they read the same
    values and do the same fp64 arithmetic), else within 1e-14 of the flux scale.  nz = None: the reference's minimum (3 for n79, else 2)."""
    import torch

    from crt1d_amd import batched

    ncol, nb, nz = shape
    if nz is None:
        nz = 3 if scheme == "n79" else 2
    cols, b32, b64 = _case(ncol, nb, nz, uniform=nz % 2 == 0, seed=9)
    w = _weights(torch, 3, nb)
    p32 = batched.IntegratedPlan(scheme, cols, b32, w, profiles=profiles)
    r32 = p32()
    n32 = p32.last_kernel()
    p64 = batched.IntegratedPlan(scheme, cols, b64, w, profiles=profiles)
    r64 = p64()
    n64 = p64.last_kernel()
    assert " f32" in n32 and " f32" not in n64, (n32, n64)
    assert ("level profiles" in n32) == profiles, n32
    flux = float(r64["totals"][..., 0].abs().max())
    same = _family(n32) == _family(n64)
    for k in r64:
        assert r32[k].dtype == torch.float64
        if same:
            assert torch.equal(r32[k], r64[k]), (k, n32, n64)
        else:
            assert float((r32[k] - r64[k]).abs().max()) <= 1e-14 * flux, (k, n32, n64)


def test_mixed_precision_is_a_type_error():
    import torch

    from crt1d_amd import batched

    cols, b32, b64 = _case(3, 40, 10)
    p32, p64 = _profiles("2s", cols, b64)
    w = _weights(torch, 1, 40)
    for bands, sol in ((b32, p64), (b64, p32)):
        with pytest.raises(TypeError):
            batched.absorb_bandsum(cols, bands, sol, w)
        with pytest.raises(TypeError):
            batched.absorb_bandsum(cols, bands, sol, w, profiles=True)
        with pytest.raises(TypeError):
            batched.absorb(cols, bands, sol)
    mixed = dict(p32, I_df_u=p64["I_df_u"])
    with pytest.raises(TypeError):
        batched.absorb_bandsum(cols, b32, mixed, w)


def _bandsum_out(torch, ncol, nz, ng, partial):
    """A crt_bandsum_out with all ten arrays, or (partial) with only three of the six optional ones."""
    from crt1d_amd import _lib, batched

    out = {k: torch.zeros(sh, dtype=torch.float64, device="cuda") for k, sh in batched.bandsum_shapes(ncol, nz, ng, True).items()}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    if partial:
        for k in ("I_df_u", "F", "I_d"):
            ptrs[k] = None
    return out, _lib.CrtBandsumOut(**ptrs)


def test_abi_errors_of_the_f32_entries():
    """nb = 1025 on the integrated path is CRT_ERR_UNSUPPORTED; a partial set of the six optional outputs is CRT_ERR_BAD_ARG (both
    entries), as for the f64 twins; so are null profiles."""
    import torch

    from crt1d_amd import _lib

    lib = _lib.load()
    opts = _lib.CrtOptions(0.501, _lib.TAU_D_METHODS["quad"], 0)
    stream = torch.cuda.current_stream().cuda_stream
    for nb, partial, expect in ((1025, False, _lib.CRT_ERR_UNSUPPORTED), (64, True, _lib.CRT_ERR_BAD_ARG)):
        cols, b32, _ = _case(2, nb, 10)
        w = _weights(torch, 2, nb)
        _, o = _bandsum_out(torch, 2, 10, 2, partial)
        ws = torch.empty(lib.crt_hip_workspace_bytes_nb(_lib.SCHEME_IDS["2s"], 2, 10, nb), dtype=torch.uint8, device="cuda")
        c, b = cols.c_struct(), b32.c_struct(2)
        st = lib.crt_hip_integrated2_f32(_lib.SCHEME_IDS["2s"], ctypes.byref(c), ctypes.byref(b), ctypes.byref(opts), w.data_ptr(), 2,
                                         ctypes.byref(o), ws.data_ptr(), ws.numel(), stream)
        assert st == expect, (nb, partial, st)
        if partial:
            prof = torch.zeros((2, 10, nb), dtype=torch.float32, device="cuda")
            st = lib.crt_hip_absorb_bandsum2_f32(ctypes.byref(c), ctypes.byref(b), prof.data_ptr(), prof.data_ptr(), prof.data_ptr(),
                                                 w.data_ptr(), 2, ctypes.byref(o), stream)
            assert st == _lib.CRT_ERR_BAD_ARG
            _, full = _bandsum_out(torch, 2, 10, 2, False)
            st = lib.crt_hip_absorb_bandsum2_f32(ctypes.byref(c), ctypes.byref(b), None, prof.data_ptr(), prof.data_ptr(), w.data_ptr(), 2,
                                                 ctypes.byref(full), stream)
            assert st == _lib.CRT_ERR_BAD_ARG
            st = lib.crt_hip_absorb_bandsum2_f32(ctypes.byref(c), ctypes.byref(b), prof.data_ptr(), prof.data_ptr(), prof.data_ptr(),
                                                 w.data_ptr(), 5, ctypes.byref(full), stream)
            assert st == _lib.CRT_ERR_BAD_ARG  # ngroup > 4
    torch.cuda.synchronize()


@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_sharded_f32(scheme):
    """crt1d_amd.dist at world size 1 with float32 bands, both partitions, keep_profiles True and False: the f64 run on the upcast bands
    to 1e-14 of the flux scale.  With profiles the f32 pipeline stores them as float, so its f64 counterpart rounds its profiles once
    before the epilogue."""
    import torch

    from crt1d_amd import batched
    from crt1d_amd.dist import solve_sharded

    def solve_rounded(scheme, c, b, **kw):
        return {k: v.float().double() for k, v in batched.solve(scheme, c, b, **kw).items()}

    cols, b32, b64 = _case(23, 300, 60, uniform=False, seed=12)
    w = _weights(torch, 3, 300)
    for partition in ("column", "band"):
        for keep in (True, False):
            r32 = solve_sharded(scheme, cols, b32, w, partition=partition, keep_profiles=keep)
            r64 = solve_sharded(scheme, cols, b64, w, partition=partition, keep_profiles=keep, solve_fn=solve_rounded if keep else None)
            flux = float(r64["totals"][..., 0].abs().max())
            for k in ("aI", "aI_sl", "aI_sh", "totals"):
                assert r32[k].dtype == torch.float64
                assert float((r32[k] - r64[k]).abs().max()) <= 1e-14 * flux, (partition, keep, k)
            if keep:
                assert r32["profiles"]["I_dr"].dtype == torch.float32


def _g10_case(torch, g1):
    """The reference's default case, spectra rounded to float (tests/test_gpu_band.py::_default_case in f32 storage)."""
    from crt1d_amd import batched

    t = lambda a, dt=torch.float64: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to("cuda", dt)  # noqa: E731
    cols = batched.Columns(psi=t(g1["psi"]), lai=t(g1["lai"])[None, :], g_kind=torch.tensor([4], dtype=torch.int32, device="cuda"),
                           g_param=t(g1["x"]), mla=t(g1["mla"]))
    f = lambda k: t(g1[k], torch.float32)  # noqa: E731
    return cols, batched.Bands(f("I_dr0_all"), f("I_df0_all"), f("leaf_r"), f("leaf_t"), f("soil_r"))


@pytest.mark.parametrize("scheme", ["2s", "n79", "zq"])
def test_f32_path_vs_g10(scheme):
    """The f32 pipeline on the reference's default case (inputs rounded to float) against the reference's band sums (g10): the f32 solve
    + the f32 epilogue, and the fused f32 path, within 1e-6 of each variable's scale."""
    import torch

    from crt1d_amd import batched, spectra

    g1, g10 = load_golden("g1_default"), load_golden("g10_band_profiles")
    cols, b32 = _g10_case(torch, g1)
    w = torch.as_tensor(spectra.band_weights(g10["wle"], [str(n) for n in g10["band_names"]])).cuda()
    sol = batched.solve(scheme, cols, b32)
    assert sol["I_dr"].dtype == torch.float32
    for res in (batched.absorb_bandsum(cols, b32, sol, w, profiles=True), batched.solve_integrated(scheme, cols, b32, w, profiles=True)):
        res = {k: v[0].cpu().numpy() for k, v in res.items()}
        for k in ("I_dr", "I_df_d", "I_df_u", "F", "I_d"):
            ref = g10[f"{scheme}__{k}__band"]
            assert np.abs(res[k].T - ref).max() <= 1e-6 * np.abs(ref).max(), k
        ab = batched.absorption_from_bandsums(res)
        scale = np.abs(g10[f"{scheme}__aI__band"]).max()
        for k in ("aI", "aI_dr", "aI_df", "aI_sl", "aI_sh", "aI_df_sl", "aI_df_sh"):
            assert np.abs(ab[k].T - g10[f"{scheme}__{k}__band"]).max() <= 1e-6 * scale, k
