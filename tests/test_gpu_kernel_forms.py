"""GPU: every kernel form a launcher can pick gives the same bits, and no solve or epilogue kernel depends on where the caller's arrays
start.

Which kernel a call runs depends on nb, nz, the storage type, the ``crt_options.tune`` overrides and the alignment of the output
pointers.  Part 1 forces each zq_pa form (the scheme with the most of them) and compares it bitwise with the two-kernel path, which is
itself held to the oracle.  Part 2 hands every solve and epilogue entry arrays at element offsets inside a larger allocation filled with a
sentinel: the results must be the bits of the aligned call, and the guard bands around each view must be untouched (a stray write shows
up as changed data, not as a fault)."""
import numpy as np
import pytest

from conftest import rel_profile_err
from crt1d_amd import _lib

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "bl", "g77", "bf", "n79", "zq", "zq_pa")
_IO = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")


def _case(ncol, nb, nz, seed, uniform, dtype="f64"):
    from crt1d_amd import batched, synth

    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform)
    if dtype == "f32":
        d = {k: (v.astype(np.float32) if k in _IO else v) for k, v in d.items()}
    return d, batched.Columns.from_host(d), batched.Bands.from_host(d)


def _upcast(bands):
    from crt1d_amd import batched

    return batched.Bands(*[None if t is None else t.double() for t in (bands.I_dr0, bands.I_df0, bands.leaf_r, bands.leaf_t, bands.soil_r)])


def _bits(t):
    import torch

    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _same_bits(a, b):
    import torch

    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _nan_fill(out):
    for v in out.values():
        v.fill_(float("nan"))


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. zq_pa: every form against the two-kernel path (grid solve into workspace scratch + k_zqpa_interp)

_ZQPA_ANCHOR = {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_TWO_KERNEL}
# the default heuristics; k_zqpa_pipe; k_zqpa_pipe2 double-buffered / register-staged; M = 8 and M = 16, with either staging at M = 8; no
# flat flush / no whole-line flush; one and four store waves; the grid solve of the two-kernel path through k_tri_tile M8 T8 (the grid
# solve reads ZQPA_TWO_KERNEL as NO_PIPELINE, csrc/tri_zqpa.hip)
_ZQPA_SETTINGS = ({}, {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE}, {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE2_DB},
                  {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE2_RS}, {_lib.TUNE_TRI_M: 8},
                  {_lib.TUNE_TRI_M: 8, _lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE2_DB},
                  {_lib.TUNE_TRI_M: 8, _lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE2_RS}, {_lib.TUNE_TRI_M: 16},
                  {_lib.TUNE_FLAT_FLUSH: _lib.FLAT_FLUSH_OFF}, {_lib.TUNE_FLAT_FLUSH: _lib.FLAT_FLUSH_PART_LINE},
                  {_lib.TUNE_TRI_STORE_WAVES: 1}, {_lib.TUNE_TRI_STORE_WAVES: 4},
                  {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_TWO_KERNEL, _lib.TUNE_TRI_M: 8, _lib.TUNE_TRI_T: 8})
# (ncol, nb, nz, uniform dLAI, check the anchor against the oracle): nb across every threshold of launch_zqpa (16, 48 / 49, 64 / 65, 128,
# 256 / 257, one compute wave, odd / even, 1000 = no single-kernel form fits, 1025 = per-wave grid solve); nz below, at and above the
# 100-row computational grid
_ZQPA_SHAPES = [(4, 16, 60, True, True), (5, 17, 13, False, False), (3, 38, 100, False, False), (4, 48, 61, True, False),
                (3, 49, 101, False, True), (4, 63, 3, True, False), (3, 64, 99, False, False), (5, 65, 60, False, False),
                (3, 106, 150, True, False), (4, 107, 61, False, True), (3, 128, 100, True, False), (4, 129, 2, False, True),
                (3, 255, 101, True, False), (2, 256, 250, False, False), (2, 257, 60, True, False), (3, 300, 100, False, True),
                (2, 300, 60, True, False), (2, 301, 150, True, False), (2, 601, 99, False, False), (2, 1000, 61, False, False),
                (2, 1025, 13, True, True), (130, 64, 61, False, False), (131, 107, 100, True, False)]
M15_TOL = 4e-15  # k_zqpa_pipe M = 15 vs the other forms, of the profile maximum (measured up to 7e-16 of the array maximum)
_ZQPA_SEEN = {}  # shape -> kernel names of the f64 matrix
_ZQPA_SEEN32 = {}  # shape -> kernel names of the f32 matrix


def _zqpa_f64_matrix(shape, oracle=None):
    import torch

    from crt1d_amd import batched

    ncol, nb, nz, uniform, _ = shape
    d, cols, bands = _case(ncol, nb, nz, 5 + nb, uniform)
    ref = batched.Plan("zq_pa", cols, bands, tune=_ZQPA_ANCHOR)
    _nan_fill(ref.out)
    ref()
    torch.cuda.synchronize()
    names = [ref.last_kernel()]
    assert "two-kernel" in names[0], names[0]
    if oracle is not None:
        oc = oracle.Columns(d["psi"], d["lai"], mla=d["mla"], g_kind=d["g_kind"], g_param=d["g_param"])
        want = oracle.SOLVERS["zq_pa"](oc, **{k: d[k] for k in _IO})
        for k, v in ref.out.items():
            err = rel_profile_err(v.cpu().numpy(), want[k])
            assert err <= 1e-11, (k, err)
    for tune in _ZQPA_SETTINGS:
        p = batched.Plan("zq_pa", cols, bands, tune=tune)
        _nan_fill(p.out)
        p()
        torch.cuda.synchronize()
        name = p.last_kernel()
        names.append(name)
        if "k_zqpa_pipe" in name:  # the single-kernel forms: odd band counts take a flat store role, even ones the (row, band pair) flush
            assert ("flat" in name) == bool(nb % 2), name
        for k in ref.out:
            assert bool(torch.isfinite(p.out[k]).all()), (tune, name, k)
            if " M=15 " in name:  # the one form whose segments restart off the re-seeding schedule (tri_schemes.hpp RENORM): equal to rounding
                err = rel_profile_err(p.out[k].cpu().numpy(), ref.out[k].cpu().numpy())
                assert err <= M15_TOL, (tune, name, k, err)
            else:
                assert _same_bits(p.out[k], ref.out[k]), (tune, name, k)
    return names


@pytest.mark.parametrize("shape", _ZQPA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}{'u' if s[3] else 'r'}")
def test_zq_pa_every_form_equals_two_kernel_path(oracle, shape):
    """Every zq_pa setting gives the BITWISE output of the two-kernel path (same expressions; the rounds must hand every output level
    exactly the computational rows it needs); the anchor itself is within 1e-11 of the oracle's profile maxima on a subset.  The exception
    is k_zqpa_pipe M = 15, whose checkpoint spacing is off the sweep's re-seeding schedule: equal to rounding (M15_TOL)."""
    _ZQPA_SEEN[shape] = _zqpa_f64_matrix(shape, oracle if shape[4] else None)


_ZQPA_F32_SETTINGS = ({}, {_lib.TUNE_TRI_STORE_WAVES: 1}, {_lib.TUNE_TRI_STORE_WAVES: 4})
_ZQPA_F32_SHAPES = [s for s in _ZQPA_SHAPES if 16 <= s[1] <= 832 and s[0] < 130] + [(3, 832, 13, False, False), (3, 832, 60, False, False)]
_ZQPA_F32_TOO_WIDE = {(3, 832, 60, False, False)}  # no f32 form fits the LDS (include/crt1d_hip.h): refused, nothing launched


def _zqpa_f32_matrix(shape):
    import torch

    from crt1d_amd import batched

    ncol, nb, nz, uniform, _ = shape
    _, cols, b32 = _case(ncol, nb, nz, 7 + nb, uniform, "f32")
    if shape in _ZQPA_F32_TOO_WIDE:
        with pytest.raises(RuntimeError, match="not supported"):
            batched.Plan("zq_pa", cols, b32)()
        return []
    ref = batched.Plan("zq_pa", cols, _upcast(b32), tune=_ZQPA_ANCHOR)  # the f64 two-kernel path on the same (float-representable) values
    ref()
    names = []
    for tune in _ZQPA_F32_SETTINGS:
        p = batched.Plan("zq_pa", cols, b32, tune=tune)
        _nan_fill(p.out)
        p()
        torch.cuda.synchronize()
        names.append(p.last_kernel())
        for k in ref.out:
            if " M=15 " in names[-1]:  # (see M15_TOL) rounding to float may then land one float ulp apart
                err = rel_profile_err(p.out[k].double().cpu().numpy(), ref.out[k].cpu().numpy())
                assert err <= 2.0**-23, (tune, names[-1], k, err)
            else:
                assert _same_bits(p.out[k], ref.out[k].float()), (tune, names[-1], k)
    return names


@pytest.mark.parametrize("shape", _ZQPA_F32_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}x{s[2]}{'u' if s[3] else 'r'}")
def test_zq_pa_f32_forms_equal_rounded_f64(shape):
    """f32 storage: the fp64 result rounded once, bit for bit the f64 two-kernel path's output `.float()`, in every f32 form (but M = 15)."""
    _ZQPA_SEEN32[shape] = _zqpa_f32_matrix(shape)


_ZQPA_FORMS = ("k_zqpa_pipe2<f64> register-staged M=8 ", "k_zqpa_pipe2<f64> register-staged M=16 ", "k_zqpa_pipe2<f64> double-buffered M=8 ",
               "k_zqpa_pipe2<f64> double-buffered M=16 ", "k_zqpa_pipe2<f64> flat-flush", "k_zqpa_pipe2<f64> whole-line flat-flush",
               "k_zqpa_pipe<f64> M=12 ", "k_zqpa_pipe<f64> M=15 ", "k_zqpa_pipe<f64> M=16 ", "k_zqpa_pipe<f64,flat> M=12 ",
               "k_zqpa_pipe<f64,flat> M=15 ", "k_zqpa_pipe<f64,flat> M=16 ", "two-kernel path: grid solve k_tri_tile<zq_pa grid,f64> M=8 T=8",
               "two-kernel path: grid solve k_tri_wave<zq_pa grid,f64>")
_ZQPA_FORMS32 = ("k_zqpa_pipe<f32> M=16 ", "k_zqpa_pipe<f32> M=15 ", "k_zqpa_pipe<f32,flat> M=16 ")


def test_zq_pa_matrix_reaches_every_form():
    """The matrices above really selected every named form (shapes the run did not reach are run here)."""
    names = set()
    for shape in _ZQPA_SHAPES:
        names.update(_ZQPA_SEEN[shape] if shape in _ZQPA_SEEN else _zqpa_f64_matrix(shape))
    missing = [f for f in _ZQPA_FORMS if not any(f in n for n in names)]
    assert not missing, (missing, sorted(names))
    # default heuristics at a width no single-kernel form fits (ncomp = 1024 leaves no store wave): the two-kernel path
    assert "two-kernel" in _ZQPA_SEEN.get((2, 1000, 61, False, False), _zqpa_f64_matrix((2, 1000, 61, False, False)))[1]
    names32 = set()
    for shape in _ZQPA_F32_SHAPES:
        names32.update(_ZQPA_SEEN32[shape] if shape in _ZQPA_SEEN32 else _zqpa_f32_matrix(shape))
    missing = [f for f in _ZQPA_FORMS32 if not any(f in n for n in names32)]
    assert not missing, (missing, sorted(names32))


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. caller-owned arrays at element offsets, inside guard bands

GUARD = 64  # elements before and after every view (256 / 512 B: the view's misalignment is exactly its element offset)
OFFSETS = {"f64": (1, 2, 16), "f32": (1, 2, 3, 32)}  # 8, 16, 128 B and 4, 8, 12, 128 B off a 128-B line
MIXED = {"f64": (1, 2, 16, 3, 5, 7, 9), "f32": (1, 2, 3, 32, 5, 6, 7)}  # a different offset per array


class _Guarded:
    """A contiguous ``shape`` view at element ``off`` of one allocation that holds GUARD sentinel elements on either side."""

    SENTINEL = {8: 0x7FF4DEADBEEF0F0F, 4: 0x7FA50F0F}  # NaN payloads: an element nobody wrote compares unequal to any result

    def __init__(self, shape, dtype, off):
        import torch

        n = int(np.prod(shape))
        self.buf = torch.empty(GUARD + off + n + GUARD, dtype=dtype, device="cuda")
        self.pat = self.SENTINEL[self.buf.element_size()]
        _bits(self.buf).fill_(self.pat)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.view = self.buf[self.lo:self.hi].view(shape)
        assert (self.view.data_ptr() - off * self.buf.element_size()) % 128 == 0

    def intact(self):
        b = _bits(self.buf)
        return bool((b[:self.lo] == self.pat).all()) and bool((b[self.hi:] == self.pat).all())


def _guarded_like(ref, offs):
    return {k: _Guarded(tuple(v.shape), v.dtype, off) for (k, v), off in zip(ref.items(), offs)}


def _offset_cases(dt, nkeys):
    return [(o,) * nkeys for o in OFFSETS[dt]] + [tuple(MIXED[dt][i % len(MIXED[dt])] for i in range(nkeys))]


# one forced family per scheme: k_tri_tile, k_zqpa_pipe, and k_tile for the closed forms
_FORCED = {"n79": {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_NO_PIPELINE}, "zq": {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_NO_PIPELINE},
           "zq_pa": {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE}}
_FORCED_CLOSED = {_lib.TUNE_TILE_FLAGS: _lib.TILE_FLAG_NO_PIPELINE}
_ALIGN_SHAPES = [(3, 20, 33), (3, 37, 33), (3, 64, 13), (3, 107, 61), (2, 300, 33)]  # an even width <= 32 (packed), odd, 64, 107, 300


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_solve_outputs_at_any_offset(scheme, dtype):
    """Plan(out=...) at element offsets: the bits of the aligned call, nothing written outside the arrays."""
    import torch

    from crt1d_amd import batched

    for ncol, nb, nz in _ALIGN_SHAPES:
        _, cols, bands = _case(ncol, nb, nz, 31 + nb, nb % 2 == 0, dtype)
        ref = batched.Plan(scheme, cols, bands)
        ref()
        torch.cuda.synchronize()
        for tune in ({}, _FORCED.get(scheme, _FORCED_CLOSED)):
            for offs in _offset_cases(dtype, len(ref.out)):
                g = _guarded_like(ref.out, offs)
                out = {k: v.view for k, v in g.items()}
                if scheme == "zq_pa" and dtype == "f32" and any(o % 2 for o in offs):
                    with pytest.raises(ValueError, match="8-byte boundary"):  # refused before any launch (tests below)
                        batched.Plan(scheme, cols, bands, out=out, tune=tune)
                    continue
                p = batched.Plan(scheme, cols, bands, out=out, tune=tune)
                p()
                torch.cuda.synchronize()
                name = p.last_kernel()
                for k in ref.out:
                    assert _same_bits(out[k], ref.out[k]), (nb, tune, offs, name, k)
                    assert g[k].intact(), (nb, tune, offs, name, k)
                if scheme == "zq_pa" and dtype == "f64" and any(o % 2 for o in offs):  # no single-kernel form takes 8-B aligned outputs
                    assert "two-kernel" in name, name


def test_zq_pa_f32_outputs_need_8_byte_alignment():
    """f32 zq_pa stores band pairs in every form and has no two-kernel path: the C entry refuses outputs at a 4-byte offset
    (CRT_ERR_UNSUPPORTED, nothing written), and Plan raises a ValueError that names the requirement before it launches anything."""
    import torch

    from crt1d_amd import _lib, batched

    _, cols, b32 = _case(3, 107, 60, 41, False, "f32")
    ref = batched.Plan("zq_pa", cols, b32)
    ref()
    for off in (1, 3):
        g = _guarded_like(ref.out, (off,) * 4)
        out = {k: v.view for k, v in g.items()}
        with pytest.raises(ValueError, match="8-byte boundary"):
            batched.Plan("zq_pa", cols, b32, out=out)
        raw = batched.Plan("zq_pa", cols, b32)  # the C entry on its own, behind the Python check
        raw._point_at(out)
        with pytest.raises(RuntimeError, match=f"status {_lib.CRT_ERR_UNSUPPORTED}"):
            raw()
        torch.cuda.synchronize()
        for k in out:
            assert g[k].intact() and bool((_bits(out[k]) == g[k].pat).all()), k
    g = _guarded_like(ref.out, (2, 4, 6, 34))  # 8-byte aligned, not 16: fine
    p = batched.Plan("zq_pa", cols, b32, out={k: v.view for k, v in g.items()})
    p()
    torch.cuda.synchronize()
    for k in ref.out:
        assert _same_bits(p.out[k], ref.out[k]) and g[k].intact(), k


_EPI_SHAPES = [(5, 20, 33), (4, 37, 13), (6, 40, 33), (3, 64, 60), (3, 107, 61), (2, 300, 33)]  # 40: the lanes-over-layers kernel


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_epilogue_arrays_at_any_offset(dtype):
    """absorb_bandsum / BandSumPlan (profiles read from offset views, outputs written to offset views, with and without the level
    profiles) and absorb (profiles from offset views): the bits of the aligned call; inputs and guards untouched."""
    import torch

    from crt1d_amd import batched, spectra

    for ncol, nb, nz in _EPI_SHAPES:
        d, cols, bands = _case(ncol, nb, nz, 51 + nb, nb % 2 == 1, dtype)
        w = torch.as_tensor(spectra.band_weights(d["wle"])).cuda()
        sol = {k: v for k, v in batched.solve("2s", cols, bands).items() if k in ("I_dr", "I_df_d", "I_df_u")}
        per = batched.absorb(cols, bands, sol)
        for poffs in _offset_cases(dtype, 3):
            gs = _guarded_like(sol, poffs)
            for k, v in gs.items():
                v.view.copy_(sol[k])
            sv = {k: v.view for k, v in gs.items()}
            got = batched.absorb(cols, bands, sv)
            for k in per:
                assert _same_bits(got[k], per[k]), (nb, poffs, k)
            for profiles in (False, True):
                ref = batched.absorb_bandsum(cols, bands, sol, w, profiles=profiles)
                flux = float(ref["totals"][..., 0].abs().max())
                # k_absorb_bandsum_l (32 < nb <= 48, even, no level profiles) moves pieces of two bands: profiles that do not start on one
                # take the lanes-over-bands kernel, whose band sums are added in another order -> equal to rounding there, bitwise elsewhere
                other_kernel = not profiles and 32 < nb <= 48 and nb % 2 == 0 and any(o % 2 for o in poffs)
                for ooffs in _offset_cases("f64", len(ref)):
                    go = _guarded_like(ref, ooffs)
                    res = batched.BandSumPlan(cols, bands, sv, w, out={k: v.view for k, v in go.items()}, profiles=profiles)()
                    torch.cuda.synchronize()
                    for k in ref:
                        if other_kernel:
                            err = float((res[k] - ref[k]).abs().max()) / flux
                            assert err <= 1e-14, (nb, poffs, ooffs, k, err)
                        else:
                            assert _same_bits(res[k], ref[k]), (nb, profiles, poffs, ooffs, k)
                        assert go[k].intact(), (nb, profiles, poffs, ooffs, k)
            for k, v in gs.items():
                assert v.intact() and _same_bits(v.view, sol[k]), k


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_integrated_outputs_at_any_offset(scheme, dtype):
    """IntegratedPlan(out=...) at element offsets, with and without the level profiles: the bits of the aligned call, guards untouched."""
    import torch

    from crt1d_amd import batched, spectra

    for ncol, nb, nz in [(4, 20, 33), (3, 107, 61), (2, 300, 13)]:
        d, cols, bands = _case(ncol, nb, nz, 61 + nb, nz % 2 == 1, dtype)
        w = torch.as_tensor(spectra.band_weights(d["wle"])).cuda()
        for profiles in (False, True):
            ref = batched.IntegratedPlan(scheme, cols, bands, w, profiles=profiles)()
            for offs in _offset_cases("f64", len(ref)):
                g = _guarded_like(ref, offs)
                p = batched.IntegratedPlan(scheme, cols, bands, w, profiles=profiles, out={k: v.view for k, v in g.items()})
                p()
                torch.cuda.synchronize()
                for k in ref:
                    assert _same_bits(p.out[k], ref[k]), (nb, profiles, offs, p.last_kernel(), k)
                    assert g[k].intact(), (nb, profiles, offs, p.last_kernel(), k)
