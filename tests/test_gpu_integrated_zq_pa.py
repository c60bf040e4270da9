"""GPU: the fused integrated path of zq_pa (crt_hip_integrated2_f64 -> k_zqpa_int): the solve on the computational grid, the band
sums and the absorption in one kernel, no profile and no computational-grid scratch written.  The kernel interpolates the BAND SUMS
of the grid's interface fluxes to the caller's levels (the interpolation weights do not depend on the band), so it must equal the
profile path followed by the band-sum epilogue up to rounding."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FLUX_KEYS = ("aI", "aI_sl", "aI_sh", "totals", "reflectance")


def _case(ncol, nb, nz, uniform, seed=23):
    import torch

    from crt1d_amd import batched, spectra, synth

    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    w = torch.as_tensor(spectra.band_weights(d["wle"])).cuda()
    return d, cols, bands, w


def _compare(fused, ref, profiles):
    """Every output within 1e-13 of the flux scale of its band group (F: of its own scale, it carries I_dr / mu)."""
    from crt1d_amd import batched

    keys = batched.BANDSUM_KEYS + (batched.PROFILE_KEYS if profiles else ())
    assert sorted(fused) == sorted(keys)
    flux = ref["totals"][:, :, 0].abs().amax(dim=0)  # (ngroup,): incoming flux of each group
    for k in keys:
        assert fused[k].shape == ref[k].shape, k
        g_axis = 1 if k == "totals" else 2
        for g in range(flux.numel()):
            a, b = fused[k].select(g_axis, g), ref[k].select(g_axis, g)
            scale = max(float(flux[g]), float(b.abs().max()))
            err = float((a - b).abs().max()) / scale
            assert err < 1e-13, (k, g, err)


@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("shape", [(19, 300, 60, True), (19, 300, 60, False), (7, 107, 61, False), (5, 64, 13, False), (3, 30, 9, True),
                                   (2, 513, 100, True), (3, 300, 100, False), (3, 300, 150, False), (3, 300, 150, True), (4, 40, 2, True), (2, 1024, 40, False)])
def test_fused_equals_solve_plus_epilogue(shape, profiles):
    """IntegratedPlan("zq_pa") == batched.solve("zq_pa") followed by absorb_bandsum, at the bar of the other schemes' fused kernels.
    nz = 150 > 100: the grid has 100 rows and a grid row spans more than one caller level; nz = 2: the smallest grid.  Without profiles
    300 x 100 takes the separate-sums form at M = 12, the other shapes the net-flux form (launch_zqpa_int)."""
    from crt1d_amd import batched

    ncol, nb, nz, uniform = shape
    _, cols, bands, w = _case(ncol, nb, nz, uniform)
    plan = batched.IntegratedPlan("zq_pa", cols, bands, w, profiles=profiles)
    fused = plan()
    name = plan.lib.crt_hip_last_kernel().decode()
    sol = batched.solve("zq_pa", cols, bands)
    ref = batched.absorb_bandsum(cols, bands, sol, w, profiles=profiles)
    _compare(fused, ref, profiles)
    assert "k_zqpa_int" in name and "zq_pa" in name, name
    assert ("level profiles" in name) == profiles, name


@pytest.mark.parametrize("ngroup", [1, 3, 4])
def test_fused_band_groups(ngroup):
    """One, three and four band groups; the fourth row holds photon-flux weights (PAR / e_wl_umol, diagnostics.py:92-104)."""
    import torch

    from crt1d_amd import batched, spectra

    d, cols, bands, _ = _case(6, 120, 47, False, seed=31)
    wW = spectra.band_weights(d["wle"])
    wP = spectra.band_weights(d["wle"], ("PAR",), pfd=True)
    rows = {1: [2], 3: [0, 1, 2], 4: [0, 1, 2, 3]}[ngroup]  # solar | PAR, NIR, solar | + PAR photon flux
    w = torch.as_tensor(np.vstack([wW, wP])[rows]).contiguous().cuda()
    assert w.shape == (ngroup, 120)
    sol = batched.solve("zq_pa", cols, bands)
    for profiles in (False, True):
        fused = batched.solve_integrated("zq_pa", cols, bands, w, profiles=profiles)
        ref = batched.absorb_bandsum(cols, bands, sol, w, profiles=profiles)
        _compare(fused, ref, profiles)


def test_fused_vs_reference_default_case():
    """The default canopy (60 levels x 107 bands): the reference's own zq_pa profiles (g1), band-summed on the host with the same
    weights and run through the oracle's absorption, against the fused kernel.  Bar: zq_pa's parity with the reference, 1e-6."""
    import torch

    from crt1d_amd import batched, spectra
    from oracle import crt_oracle as O

    g1, g10 = load_golden("g1_default"), load_golden("g10_band_profiles")
    dev = "cuda"
    t = lambda a: torch.as_tensor(np.atleast_1d(np.asarray(a, dtype=np.float64))).to(dev)  # noqa: E731
    cols = batched.Columns(psi=t(g1["psi"]), lai=t(g1["lai"])[None, :], g_kind=torch.tensor([4], dtype=torch.int32, device=dev),
                           g_param=t(g1["x"]), mla=t(g1["mla"]))
    bands = batched.Bands(t(g1["I_dr0_all"]), t(g1["I_df0_all"]), t(g1["leaf_r"]), t(g1["leaf_t"]), t(g1["soil_r"]))
    wn = spectra.band_weights(g10["wle"], [str(n) for n in g10["band_names"]])
    res = {k: v[0].cpu().numpy() for k, v in batched.solve_integrated("zq_pa", cols, bands, torch.as_tensor(wn).cuda(), profiles=True).items()}

    prof = {k: g1[f"zq_pa__{k}"] for k in ("I_dr", "I_df_d", "I_df_u", "F")}  # (nz, nb)
    lev = {k: v @ wn.T for k, v in prof.items()}
    lev["I_d"] = (prof["I_dr"] + prof["I_df_d"]) @ wn.T
    oc = O.Columns(float(g1["psi"]), g1["lai"][None, :], mla=float(g1["mla"]), g_kind=4, g_param=float(g1["x"]))
    ab = O.calc_absorption(oc, {k: v[None] for k, v in prof.items()}, leaf_r=g1["leaf_r"], leaf_t=g1["leaf_t"])
    for k in ("I_dr", "I_df_d", "I_df_u", "F", "I_d"):
        assert np.abs(res[k] - lev[k]).max() <= 1e-6 * np.abs(lev[k]).max(), k
    scale = np.abs(ab["aI"][0] @ wn.T).max()
    for k in ("aI", "aI_sl", "aI_sh", "aI_dr"):
        assert np.abs(res[k] - ab[k][0] @ wn.T).max() <= 1e-6 * scale, k
    tot = np.stack([lev["I_d"][-1], lev["I_df_u"][-1], lev["I_d"][0], lev["I_df_u"][0]], axis=1)  # (ngroup, 4)
    assert np.abs(res["totals"] - tot).max() <= 1e-6 * np.abs(tot).max()


@pytest.mark.parametrize("nz", [37, 130])
def test_fused_vs_oracle_ragged(oracle, nz):
    """Synthetic columns with ragged dLAI against the NumPy oracle's zq_pa + its absorption, band-summed on the host."""
    from crt1d_amd import batched

    d, cols, bands, w = _case(5, 64, nz, False, seed=8)
    res = {k: v.cpu().numpy() for k, v in batched.solve_integrated("zq_pa", cols, bands, w, profiles=True).items()}
    oc = oracle.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
    ref = oracle.SOLVERS["zq_pa"](oc, I_dr0=d["I_dr0"], I_df0=d["I_df0"], leaf_r=d["leaf_r"], leaf_t=d["leaf_t"], soil_r=d["soil_r"])
    ab = oracle.calc_absorption(oc, ref, leaf_r=d["leaf_r"], leaf_t=d["leaf_t"])
    wn = w.cpu().numpy()
    lev = {k: ref[k] @ wn.T for k in ("I_dr", "I_df_d", "I_df_u", "F")}
    lev["I_d"] = (ref["I_dr"] + ref["I_df_d"]) @ wn.T
    flux = np.abs(lev["I_d"][:, -1]).max()
    for k, v in lev.items():
        assert np.abs(res[k] - v).max() <= 1e-6 * max(flux, np.abs(v).max()), k
    for k in ("aI", "aI_sl", "aI_sh", "aI_dr"):
        assert np.abs(res[k] - ab[k] @ wn.T).max() <= 1e-6 * flux, k


def test_band_limit_is_an_error():
    """nb > 1024 is CRT_ERR_UNSUPPORTED, as for the other integrated kernels; no solve kernel is reported as launched."""
    from crt1d_amd import batched

    _, cols, bands, w = _case(2, 64, 10, True)
    plan = batched.IntegratedPlan("zq_pa", cols, bands, w)
    plan()
    before = plan.lib.crt_hip_last_kernel().decode()
    assert "k_zqpa_int" in before
    _, cols, bands, w = _case(2, 1025, 10, True)
    with pytest.raises(RuntimeError, match="crt_hip_integrated2_f64"):
        batched.solve_integrated("zq_pa", cols, bands, w)
    assert plan.lib.crt_hip_last_kernel().decode() == before


def test_dist_keep_profiles_false():
    """crt1d_amd.dist at world size 1: keep_profiles=False (fused kernel) == keep_profiles=True (solve + epilogue), column and band
    partitions."""
    from crt1d_amd.dist import solve_sharded

    _, cols, bands, w = _case(23, 300, 60, False, seed=12)
    for partition in ("column", "band"):
        rp = solve_sharded("zq_pa", cols, bands, w, partition=partition)
        rf = solve_sharded("zq_pa", cols, bands, w, partition=partition, keep_profiles=False)
        assert rf["profiles"] is None
        flux = float(rp["totals"][..., 0].abs().max())
        for k in FLUX_KEYS:
            assert rf[k].shape == rp[k].shape, (partition, k)
            assert float((rf[k] - rp[k]).abs().max()) <= 1e-13 * flux, (partition, k)
