"""GPU: leaf-inclination PDFs on the device (crt_hip_g_from_pdf_f64, k_g_from_pdf).

Bar: ``|G - G_exact| <= 1e-11`` at every node and every caller angle.  An error d in G moves a flux by about
d LAI / cos(psi) <= d 8 / cos(75 deg) ~ 31 d relative; the tightest parity bar of the project is 3e-10 (n79 ``aI_ls*``),
so d must stay at 1e-11.  End to end a PDF column and the closed-form column of the same distribution may then differ by
3e-10 x 3 ~ 1e-9 of the incoming flux.  G_exact: 0.5 (spherical), Campbell's exact form (ellipsoidal), mpmath's tanh-sinh rule split at
the kink (TRIG; tests/test_leaf_pdf_cpu.py, in machine arithmetic, itself within 1e-13 of the 25-digit values there)."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from test_leaf_pdf_cpu import mp_G

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-11
HALF_PI = np.pi / 2
SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
# (kind, (p0, p1)): the eight PDFs, mixed over the columns of every call
PDFS = [(0, (0.0, 0.0)), (2, (1.0, 0.0)), (1, (0.3, 0.0)), (2, (0.0, 0.0)), (1, (2.5, 0.0)), (2, (-1.0, 0.0)), (1, (1.0, 0.0)), (2, (0.0, -1.0))]
PSI_POOL = np.array([0.0, 1e-3, np.deg2rad(20.0), np.deg2rad(75.0), np.deg2rad(89.99), 0.3, 1.0, 1.4, HALF_PI])


def _mods():
    from crt1d_amd import _lib, batched, leaf_angle, synth

    return _lib, batched, leaf_angle, synth


def g_exact(kind, p, psi):
    _, _, la, _ = _mods()
    psi = np.asarray(psi, dtype=np.float64)
    if kind == 0:
        return np.full(psi.shape, 0.5)
    if kind == 1:
        return la.G_ellipsoidal(psi, p[0])
    return mp_G(kind, p, psi.ravel(), multiprecision=False).reshape(psi.shape)  # (cached per angle: the pool and the nodes repeat)


def _pdf_arrays(ncol):
    kind = np.array([PDFS[c % len(PDFS)][0] for c in range(ncol)], dtype=np.int32)
    param = np.array([PDFS[c % len(PDFS)][1] for c in range(ncol)], dtype=np.float64)
    return kind, param


@pytest.mark.parametrize("mu_s", [0.501, 0.33998])
@pytest.mark.parametrize("npsi", [0, 1, 5])
@pytest.mark.parametrize("ncol", [1, 3, 130])
def test_tables_meet_the_bar(ncol, npsi, mu_s):
    _lib, batched, la, _ = _mods()
    kind, param = _pdf_arrays(ncol)
    psi = PSI_POOL[(np.arange(ncol * npsi) * 7 % len(PSI_POOL))].reshape(ncol, npsi)
    g_table, g_at_psi, mla = batched.leaf_pdf_tables(torch.as_tensor(kind, device=DEV), torch.as_tensor(param, device=DEV), mu_s=mu_s,
                                                     psi=torch.as_tensor(psi, device=DEV) if npsi else None)
    torch.cuda.synchronize()
    assert g_table.shape == (ncol, _lib.NQ) and g_at_psi.shape == (ncol, npsi) and mla.shape == (ncol,)
    g_table, g_at_psi = g_table.cpu().numpy(), g_at_psi.cpu().numpy()
    nodes = _lib.quad_nodes(mu_s)
    worst = 0.0
    for c in range(min(ncol, 2 * len(PDFS))):  # every PDF twice; the rest of 130 columns against these rows below
        k, p = PDFS[c % len(PDFS)]
        worst = max(worst, np.abs(g_table[c] - g_exact(k, p, nodes)).max())
        if npsi:
            worst = max(worst, np.abs(g_at_psi[c] - g_exact(k, p, psi[c])).max())
    print(f"ncol={ncol} npsi={npsi} mu_s={mu_s}: worst |G - G_exact| = {worst:.2e}")
    assert worst <= BAR
    for c in range(len(PDFS), ncol):  # the same PDF gives the same bits in every column
        assert np.array_equal(g_table[c], g_table[c % len(PDFS)]), c
    if npsi and ncol > 2 * len(PDFS):
        for c in range(2 * len(PDFS), ncol):
            k, p = PDFS[c % len(PDFS)]
            assert np.abs(g_at_psi[c] - g_exact(k, p, psi[c])).max() <= BAR, c


def test_hand_limits():
    """Erectophile at psi -> 0: G = (2/pi) int (1 - cos 2t) cos t dt = 4 / (3 pi); planophile: 8 / (3 pi) there and
    (2/pi)^2 (1 - 1/3) at pi/2, where A = (2/pi) sin(theta); spherical 0.5 at both ends."""
    _, batched, la, _ = _mods()
    psi = np.array([[0.0, 1e-9, HALF_PI]] * 3)
    kind = np.array([2, 2, 0], dtype=np.int32)
    param = np.array([[-1.0, 0.0], [1.0, 0.0], [0.0, 0.0]])
    _, g, _ = batched.leaf_pdf_tables(kind, param, psi=psi)
    g = g.cpu().numpy()
    assert np.isfinite(g).all()
    assert np.abs(g[0, :2] - 4 / (3 * np.pi)).max() < 1e-14 and abs(g[0, 2] - (2 / np.pi) ** 2 * 4 / 3) < 1e-14
    assert np.abs(g[1, :2] - 8 / (3 * np.pi)).max() < 1e-14 and abs(g[1, 2] - (2 / np.pi) ** 2 * 2 / 3) < 1e-14
    assert np.abs(g[2] - 0.5).max() < 1e-14


def test_mla():
    _, batched, la, _ = _mods()
    g = load_golden("g11_leaf_pdf")
    pdfs = [getattr(la.LeafPDF, str(n))() for n in g["names"]] + [la.LeafPDF.ellipsoidal(float(x)) for x in g["x"]]
    _, _, mla = batched.leaf_pdf_tables([p.kind for p in pdfs], [p.param for p in pdfs])
    mla = mla.cpu().numpy()
    ref = np.concatenate([g["mla"], g["mla_ell"]])
    print("mla - reference (deg):", mla - ref)
    assert np.abs(mla - ref).max() < 1e-7  # the reference's quad runs at its default tolerance
    assert abs(mla[0] - np.rad2deg(1.0)) < 1e-10 and abs(mla[1] - 45.0) < 1e-10  # spherical: 1 rad; uniform: 45 deg
    assert abs(mla[4] - 45.0) < 1e-10 and abs(mla[2] + mla[3] - 90.0) < 1e-10  # plagiophile by symmetry; planophile + erectophile
    assert abs(la.LeafPDF.uniform().mla() - 45.0) < 1e-10


def test_bad_descriptor_writes_nothing():
    """A bad kind in the LAST column: ValueError, and all three outputs keep what they held."""
    _lib, batched, la, _ = _mods()
    ncol, npsi = 5, 2
    kind, param = _pdf_arrays(ncol)
    fill = -7.25
    outs = [torch.full(s, fill, dtype=torch.float64, device=DEV) for s in ((ncol, _lib.NQ), (ncol, npsi), (ncol,))]
    psi = torch.full((ncol, npsi), 0.4, dtype=torch.float64, device=DEV)
    lib = _lib.load()

    def call(k, p):
        kt, pt = torch.as_tensor(k, device=DEV), torch.as_tensor(p, device=DEV)
        st = lib.crt_hip_g_from_pdf_f64(kt.data_ptr(), pt.data_ptr(), ncol, 0.501, psi.data_ptr(), npsi, outs[0].data_ptr(), outs[1].data_ptr(),
                                        outs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st

    bad = []
    k = kind.copy(); k[-1] = 3; bad.append((k, param))  # noqa: E702
    k = kind.copy(); k[-1] = -1; bad.append((k, param))  # noqa: E702
    p = param.copy(); k = kind.copy(); k[-1] = 1; p[-1] = (0.0, 0.0); bad.append((k, p))  # x = 0  # noqa: E702
    p = param.copy(); k = kind.copy(); k[-1] = 1; p[-1] = (np.nan, 0.0); bad.append((k, p))  # noqa: E702
    p = param.copy(); k = kind.copy(); k[-1] = 1; p[-1] = (0.1, 0.0); bad.append((k, p))  # below CRT_LEAF_X_MIN  # noqa: E702
    p = param.copy(); k = kind.copy(); k[-1] = 1; p[-1] = (20.0, 0.0); bad.append((k, p))  # above CRT_LEAF_X_MAX  # noqa: E702
    p = param.copy(); k = kind.copy(); k[-1] = 2; p[-1] = (1.5, 0.0); bad.append((k, p))  # negative near theta = pi/2  # noqa: E702
    p = param.copy(); k = kind.copy(); k[-1] = 2; p[-1] = (0.0, 1.5); bad.append((k, p))  # negative at theta = pi/4  # noqa: E702
    for k, p in bad:
        assert call(k, p) == _lib.CRT_ERR_BAD_ARG
        for o in outs:
            assert bool((o == fill).all())
    with pytest.raises(ValueError):
        batched.leaf_pdf_tables(bad[0][0], bad[0][1])
    assert call(kind, param) == _lib.CRT_OK  # the good descriptors do write
    for o in outs:
        assert not bool((o == fill).any())


def _closed_and_pdf_columns(d, pdf, g_kind, g_param, mu_s=0.501):
    """The columns of ``d`` twice: every column with the PDF ``pdf`` through the table, and with the closed form of the same
    distribution; both with the kernel's mla."""
    _, batched, la, _ = _mods()
    ncol = d["psi"].shape[0]
    psi, lai = torch.as_tensor(d["psi"], device=DEV), torch.as_tensor(d["lai"], device=DEV)
    tab = batched.Columns.from_leaf_pdf(psi, lai, [pdf.kind] * ncol, [pdf.param] * ncol, mu_s=mu_s)
    assert bool((tab.g_kind == la.G_TABLE).all()) and tab.g_table.shape == (ncol, 137) and tab.g_at_psi.shape == (ncol,)
    closed = batched.Columns(psi, lai, torch.full((ncol,), g_kind, dtype=torch.int32, device=DEV),
                             torch.full((ncol,), g_param, dtype=torch.float64, device=DEV), tab.mla)
    return tab, closed


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("dist", ["spherical", "ellipsoidal2.5"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_end_to_end_solve(scheme, dist, uniform):
    """(ncol, nb, nz) = (5, 12, 9): every output of batched.solve within 1e-9 x the incoming flux of its (column, band)."""
    _, batched, la, synth = _mods()
    d = synth.make_columns(5, 12, 9, seed=23, uniform_dlai=uniform)
    pdf, kind, par = (la.LeafPDF.spherical(), la.G_SPHERICAL, 0.0) if dist == "spherical" else (la.LeafPDF.ellipsoidal(2.5), la.G_ELLIPSOIDAL, 2.5)
    tab, closed = _closed_and_pdf_columns(d, pdf, kind, par)
    bands = batched.Bands.from_host(d, DEV)
    got, ref = batched.solve(scheme, tab, bands), batched.solve(scheme, closed, bands)
    torch.cuda.synchronize()
    incoming = torch.as_tensor(d["I_dr0"] + d["I_df0"], device=DEV)[:, None, :]
    assert set(got) == set(ref)
    for k in ref:
        err = float(((got[k] - ref[k]).abs() / incoming).max())
        assert err <= 1e-9, (scheme, dist, k, err)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("dist", ["spherical", "ellipsoidal2.5"])
@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_end_to_end_series(scheme, dist, uniform):
    """The same through IntegratedSeriesPlan, nt = 3, with SunSeries.g_at_psi from the kernel: every band-integrated output within
    1e-9 x the band-integrated incoming flux of its (column, t, group)."""
    _, batched, la, synth = _mods()
    nt, ng = 3, 2
    d = synth.make_columns(5, 12, 9, seed=29, uniform_dlai=uniform)
    s = synth.make_sun_series(d, nt, seed=31)
    pdf, kind, par = (la.LeafPDF.spherical(), la.G_SPHERICAL, 0.0) if dist == "spherical" else (la.LeafPDF.ellipsoidal(2.5), la.G_ELLIPSOIDAL, 2.5)
    tab, closed = _closed_and_pdf_columns(d, pdf, kind, par)
    bands = batched.Bands.from_host(d, DEV)
    sun = batched.SunSeries.from_host(s, DEV)
    _, g_at, _ = batched.leaf_pdf_tables([pdf.kind] * 5, [pdf.param] * 5, psi=sun.psi)
    assert g_at.shape == sun.psi.shape
    sun_tab = batched.SunSeries(sun.psi, sun.I_dr0, sun.I_df0, g_at)
    w = torch.as_tensor(np.random.default_rng(5).uniform(0.0, 1.0, (ng, 12)), device=DEV)
    got = batched.solve_integrated_series(scheme, tab, bands, sun_tab, w, profiles=True)
    ref = batched.solve_integrated_series(scheme, closed, bands, sun, w, profiles=True)
    torch.cuda.synchronize()
    incoming = torch.einsum("ctb,gb->ctg", sun.I_dr0 + sun.I_df0, w)  # (ncol, nt, ng)
    assert set(got) == set(ref)
    for k in ref:
        scale = incoming[..., None] if k == "totals" else incoming[:, :, None, :]
        err = float(((got[k] - ref[k]).abs() / scale).max())
        assert err <= 1e-9, (scheme, dist, k, err)


def test_planophile_model():
    """Model("2s", G_fn=LeafPDF.planophile()) runs on the device's table -- which is really used: the albedo differs from the spherical
    canopy's by more than 1 % -- and the table call does not touch crt_hip_last_kernel."""
    _lib, batched, la, _ = _mods()
    from crt1d_amd.model import Model

    def albedo(G_fn):
        m = Model("2s", G_fn=G_fn, psi=np.deg2rad(40.0)).run()
        up, down = m.out["I_df_u"][-1], m.out["I_dr"][-1] + m.out["I_df_d"][-1]
        assert np.isfinite(up).all() and (down > 0).all()
        return m, float(up.sum() / down.sum())

    m_sph, a_sph = albedo(la.G_spherical.gfunction)
    before = _lib.load().crt_hip_last_kernel()
    pdf = la.LeafPDF.planophile()
    table, g_at, mla = pdf.tables(np.deg2rad(40.0))
    assert _lib.load().crt_hip_last_kernel() == before and before  # a solve kernel's name, not the table kernel's
    m_pl, a_pl = albedo(pdf)
    print(f"albedo: spherical {a_sph:.5f}, planophile {a_pl:.5f}")
    assert abs(a_pl - a_sph) > 0.01 * a_sph
    # K_b_fn of such a model evaluates through the kernel too, scalar and array
    kb = m_pl.copy_p()["K_b_fn"]
    psi = np.array([0.2, np.deg2rad(40.0), 1.1])
    np.testing.assert_allclose(kb(psi), g_exact(2, (1.0, 0.0), psi) / np.cos(psi), rtol=0, atol=1e-10)
    assert abs(kb(np.deg2rad(40.0)) * np.cos(np.deg2rad(40.0)) - g_at[0]) < 1e-15
    # the series path of the same model (run_series samples G_fn(psi_t) through the kernel)
    res = m_pl.run_series(np.deg2rad([20.0, 40.0, 60.0]), bands=("PAR",))
    assert np.isfinite(res["PAR"]["aI"]).all()
    # a spherical PDF as G_fn against the spherical closed form, through the single-column path
    m_tab, a_tab = albedo(la.LeafPDF.spherical())
    for k in ("I_dr", "I_df_d", "I_df_u", "F"):
        scale = (m_sph._p["I_dr0_all"] + m_sph._p["I_df0_all"])[None, :]
        scale = np.where(scale > 0, scale, 1.0)
        assert np.max(np.abs(m_tab.out[k] - m_sph.out[k]) / scale) <= 1e-9, k


def test_python_floats_keep_their_precision():
    """Parameters and angles given as Python floats (lists, LeafPDF.tables) reach the kernel as the float64 they are: 0.3 is not
    representable in float32, and G moves by ~1e-8 when x does."""
    _, batched, la, _ = _mods()
    psi = [0.3, 1.0, 1.4]
    g = la.LeafPDF.ellipsoidal(0.3)(psi)
    assert np.abs(g - la.G_ellipsoidal(np.array(psi), 0.3)).max() <= BAR
    a = batched.leaf_pdf_tables([1], [(0.3, 0.0)], psi=[psi])
    b = batched.leaf_pdf_tables(np.array([1], dtype=np.int32), np.array([[0.3, 0.0]]), psi=np.array([psi]))
    for u, v in zip(a, b):
        assert torch.equal(u, v)
