"""GPU: every scheme on the whole supported input domain (tests/domain_cases.py: ten leaf-angle classes x sun zenith 0.05 .. 89 degrees x
total LAI 0.01 .. 12 = 200 columns, classes interleaved) against the NumPy oracle, and the two bitwise contracts on the same batch.

Two comparisons per (scheme, shape, profile), both per (column, band) -- domain_cases.check_scheme, the two assertions of
tests/test_gpu_parity.py::test_hip_vs_oracle_synthetic (profile error <= bar, elementwise error <= 100 x bar):

  A  against the oracle evaluated with the DEVICE's quadrature rules (6 x 16 nodes for tau_d and mu_bar, 2 x 16 for G_int), at the bars
     of test_hip_vs_oracle_synthetic: 1e-11; 3e-10 for n79's aI_ls* on ragged profiles; for the two closed forms with a removable
     singularity the oracle's own conditioning term, 2s 1e-11 + 1e-14 / |sigma| and bf 1e-11 + 1e-14 / |k_d - K_b|
     (test_invariants_full_size) instead of a flat 1e-9, and the same for 4s, 1e-11 + 1e-14 / min |1 - lambda / K_b| over the eigenvalues
     of its matrix (domain_cases.domain_bars: one band of the batch has an eigenvalue within 4e-7 of K_b).  aI_lsh of g77 and bf, (1 - e^{-K_b L}) x ...: plus
     4 ulp(1) / (1 - e^{-K_b LAI}), the rounding of e^{-K_b L} on both sides where K_b LAI << 1.  This is the check of the kernels' arithmetic.
  B  against the plain oracle, whose rules are pinned to mpmath at 2e-15 (tests/test_quadrature_domain_cpu.py), at the same bars plus
     4 x the truncation error of the device's rules propagated through the scheme, |oracle with the device's rules - oracle| per output,
     column and band.  This is the check of the result; what the widening amounts to is tabulated in DESIGN.md 3.2.

No bar comes from a kernel's output.  Measured on MI355X (pytest -s prints every output of every case): worst error as a fraction of
the profile maximum over all shapes and both profiles, in brackets the largest error / bar, then where the worst error is.

  scheme  A: against the oracle with the device's rules      B: against the plain oracle
  2s      3.0e-10 [0.24]  I_df_d  200x70x60 uniform          3.6e-10 [0.20]  I_df_d  200x70x60 uniform   (|sigma| small)
  4s      4.2e-10 [0.23]  I_df_u  200x18x12 uniform          3.8e-10 [0.23]  I_df_u  200x18x12 uniform   (eigenvalue 4e-7 from K_b)
  n79     2.0e-12 [0.20]  I_df_d  200x70x60 ragged           1.9e-08 [0.25]  aI_lsh  200x70x60 ragged    (the rule at dlai = 3.6e-6)
  zq      5.1e-12 [0.51]  I_df_d  200x70x60 ragged           2.4e-11 [0.23]  I_df_d  200x70x60 uniform   (the rule, Bonan chi_l = 0.6)
  bl      1.7e-12 [0.17]  I_df_d  200x70x60 uniform          1.7e-12 [0.17]  I_df_d  200x70x60 uniform
  g77     2.0e-11 [0.22]  aI_lsh  200x6x12 uniform           the same: no quadrature                     (one ulp of e^{-K_b L})
  bf      5.1e-11 [0.25]  I_df_d  200x70x60 uniform          the same: no quadrature                     (k_d close to K_b)
  zq_pa   1.6e-12 [0.16]  I_df_d  200x70x60 ragged           2.4e-11 [0.23]  I_df_d  200x70x60 uniform   (the rule, Bonan chi_l = 0.6)

Where a plain 1e-11 would not hold, the excess is in every case a term derived before the run: the three removable singularities, the
rounding of e^{-K_b L} in aI_lsh, or the rules' truncation error (B only; against the same rules n79 agrees to 2e-12).
"""
import functools

import numpy as np
import pytest

import domain_cases as D

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
TRI = ("n79", "zq")
# (nb, nz).  6 and 18 bands: the kernels that pack 64 / nb columns into one compute wave (k_pipe_pack, the packed k_tri_pipe).  At 6 bands
# a pack is ten columns, one of every class, each class always in the same lanes, and 200 columns are 20 full packs; at 18 bands a pack is
# three columns, so the classes move through the lanes and the 67th pack is partial (two columns).  70 bands: one column per workgroup
# (k_pipe, k_tri_pipe), with layers down to dlai = 3.6e-6 on the ragged profiles.
SHAPES = ((6, 12), (18, 12), (70, 60))
PACKED_MAX_NB = 32
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _case(nb, nz, uniform):
    """The domain batch on the host and on the device, and its bars; built once per (shape, profile) and left unchanged."""
    from crt1d_amd import batched
    from oracle import crt_oracle

    d = D.make_domain_columns(nb, nz, uniform)
    return d, batched.Columns.from_host(d, DEV), batched.Bands.from_host(d, DEV), D.domain_bars(crt_oracle, d, uniform)


def _family(scheme, nb, name):
    """The kernel family the shape is there for, as test_config4_shape_zq asserts it."""
    if scheme == "zq_pa":  # below 16 bands: the grid solve in the packed k_tri_pipe, then k_zqpa_interp; else the fused kernels
        return ("two-kernel path" in name and "packed columns=" in name) if nb < 16 else "k_zqpa_pipe" in name
    if scheme in TRI:
        return "k_tri_pipe<" in name and (("packed columns=" in name) == (nb <= PACKED_MAX_NB))
    return ("k_pipe_pack<" if nb <= PACKED_MAX_NB else "k_pipe<") in name


def _worst(tally):
    return "  ".join(f"{k} {e:.1e} [{r:.2f}]" for k, (e, r) in tally.items())


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "200x%dx%d" % s)
@pytest.mark.parametrize("scheme", SCHEMES)
def test_domain_vs_oracle(oracle, scheme, shape, uniform):
    import torch

    from crt1d_amd import batched

    nb, nz = shape
    d, cols, bands, bars = _case(nb, nz, uniform)
    ref = D.oracle_solve(oracle, d, scheme)
    for k, v in ref.items():  # the reference is finite on the whole domain: no column is dropped or skipped below
        assert np.all(np.isfinite(v)), (k, np.argwhere(~np.isfinite(v))[:3])
    rule_ref = D.oracle_solve_device_rules(oracle, d, scheme, ref)
    plan = batched.Plan(scheme, cols, bands, placement="none")
    got = plan()
    torch.cuda.synchronize()
    assert _family(scheme, nb, plan.last_kernel()), plan.last_kernel()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert all(v.shape[0] == D.NCOL for v in got.values())
    ta, tb = {}, {}
    fa = D.check_scheme(scheme, got, rule_ref, bars, tally=ta)
    fb = D.check_scheme(scheme, got, ref, bars, rule_ref=rule_ref, tally=tb)
    tag = f"{scheme} 200x{nb}x{nz} {'uniform' if uniform else 'ragged'}"
    print(f"\n{tag} A (device rules): {_worst(ta)}\n{tag} B (oracle):       {_worst(tb)}")

    def describe(fails):
        return [(k, D.CLASS_NAMES[d["cls"][c]], D.PSI_DEG[d["ipsi"][c]], D.LAI_TOT[d["ilai"][c]], f"{r:.1f} x bar {t:.1e}") for k, c, r, t in fails[:6]]

    assert not fa, (len(fa), describe(fa))
    assert not fb, (len(fb), describe(fb))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_level_rows_are_the_profile_rows(scheme):
    """batched.solve_levels at the ground, the middle and the top == those rows of the full solve, bit for bit, on the ragged 70-band
    batch (the contract of tests/test_gpu_levels.py, there on sun zenith <= 75 degrees and one leaf-angle class)."""
    import torch

    from crt1d_amd import batched

    nb, nz = SHAPES[2]
    d, cols, bands, _ = _case(nb, nz, False)
    lev = (0, nz // 2, nz - 1)
    full = batched.solve(scheme, cols, bands)
    got = batched.solve_levels(scheme, cols, bands, lev)
    torch.cuda.synchronize()
    idx = torch.tensor(lev, device=cols.device)
    for k in ("I_dr", "I_df_d", "I_df_u", "F"):
        assert got[k].shape == (D.NCOL, len(lev), nb)
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], full[k].index_select(1, idx)), (scheme, k)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_series_slices_are_the_per_step_calls(scheme):
    """IntegratedSeriesPlan over the five sun states of PSI_DEG, on the 40 columns class x LAI of the ragged 70-band batch: every slice
    [:, t] == the per-step crt_hip_integrated2_f64 call (IntegratedPlan), bit for bit, with level profiles and three band groups.  This
    puts k_colsun at 0.05 and 89 degrees for every class (tests/test_gpu_series.py draws 0 .. 75 degrees).  No column here is of kind
    CRT_G_TABLE, so there is no g_at_psi to pass."""
    import torch

    from crt1d_amd import batched, synth

    nb, nz = SHAPES[2]
    full, _, _, _ = _case(nb, nz, False)
    d = D.take_columns(full, np.flatnonzero(full["ipsi"] == 0))
    ncol, nt = d["psi"].shape[0], len(D.PSI_DEG)
    assert ncol == len(D.CLASSES) * len(D.LAI_TOT) == 40
    s = synth.make_sun_series(d, nt, seed=9)
    s["psi"] = np.ascontiguousarray(np.broadcast_to(np.deg2rad(np.asarray(D.PSI_DEG)), (ncol, nt)))
    cols, bands, sun = batched.Columns.from_host(d, DEV), batched.Bands.from_host(d, DEV), batched.SunSeries.from_host(s, DEV)
    band_w = torch.as_tensor(np.random.default_rng(5).uniform(0.0, 1.0, (3, nb)), device=DEV)
    plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, band_w, profiles=True)
    got = plan()
    torch.cuda.synchronize()
    assert "series" in plan.last_kernel() and "k_colsun" in plan.last_kernel(), plan.last_kernel()
    for t in range(nt):
        c = batched.Columns(sun.psi[:, t].contiguous(), cols.lai, cols.g_kind, cols.g_param, cols.mla)
        b = batched.Bands(sun.I_dr0[:, t].contiguous(), sun.I_df0[:, t].contiguous(), bands.leaf_r, bands.leaf_t, bands.soil_r)
        step = batched.IntegratedPlan(scheme, c, b, band_w, profiles=True)()
        torch.cuda.synchronize()
        for k, v in step.items():
            assert got[k].shape[:2] == (ncol, nt)
            assert bool(torch.isfinite(v).all()), (scheme, k, t)
            assert torch.equal(got[k][:, t], v), (scheme, k, t, float((got[k][:, t] - v).abs().max()))
