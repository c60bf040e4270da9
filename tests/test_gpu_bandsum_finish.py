"""``crt_hip_bandsum_finish_f64``: re-forms ``aI = aI_sl + aI_sh``, ``F`` and ``I_d`` of a ``profiles=True`` band-sum result in place from
``aI_sl, aI_sh`` and the level sums ``I_dr, I_df_d, I_df_u`` (the band partition all-reduces only those, crt1d_amd/dist.py).  ``F`` and
``I_d`` must be the bits the epilogue and the fused integrated kernels write for the same sums; ``aI`` differs from the kernels' directly
summed one by rounding only."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
SPEC = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")
DERIVED = ("aI", "F", "I_d")
# (ncol, nb, nz, uniform ΔLAI)
SHAPES = [(6, 40, 20, True), (5, 107, 33, False), (4, 300, 120, False), (300, 20, 100, True)]


def _case(ncol, nb, nz, uniform, f32, seed=5):
    from crt1d_amd import batched, synth

    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform)
    cols = batched.Columns.from_host(d)
    bands = batched.Bands.from_host({k: (d[k].astype(np.float32) if (f32 and k in SPEC) else d[k]) for k in d})
    return cols, bands


def _weights(torch, ngroup, nb, seed=3):
    rng = np.random.default_rng(seed + ngroup)
    return torch.as_tensor(rng.uniform(0.0, 1.0, (ngroup, nb))).cuda()


def _check_finish(cols, ref):
    """Zero aI, F, I_d of a copy of ``ref``, finish it, compare with ``ref``."""
    import torch

    from crt1d_amd import batched

    got = {k: v.clone() for k, v in ref.items()}
    for k in DERIVED:
        got[k].zero_()
    batched.bandsum_finish(cols, got)
    torch.cuda.synchronize()
    for k in ("F", "I_d"):
        assert torch.equal(got[k], ref[k]), (k, float((got[k] - ref[k]).abs().max()))
    # the kernels sum A directly, the finish adds the sunlit and shaded parts: rounding of the absorption scale only
    scale = float(ref["aI"].abs().max())
    assert float((got["aI"] - ref["aI"]).abs().max()) <= 1e-15 * scale, "aI"
    for k in ("aI_sl", "aI_sh", "aI_dr", "I_dr", "I_df_d", "I_df_u", "totals"):
        assert torch.equal(got[k], ref[k]), k  # read (or ignored), never written


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("ngroup", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + ("" if s[3] else "-ragged"))
def test_finish_matches_the_epilogue(shape, ngroup, f32):
    import torch

    from crt1d_amd import batched

    ncol, nb, nz, uniform = shape
    cols, bands = _case(ncol, nb, nz, uniform, f32)
    sol = batched.solve("zq", cols, bands)
    ref = batched.absorb_bandsum(cols, bands, sol, _weights(torch, ngroup, nb), profiles=True)
    torch.cuda.synchronize()
    _check_finish(cols, ref)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_finish_matches_the_integrated_kernels(scheme, f32):
    import torch

    from crt1d_amd import batched

    for ncol, nb, nz, uniform in ((6, 40, 20, True), (5, 107, 33, False)):
        cols, bands = _case(ncol, nb, nz, uniform, f32, seed=9)
        for ngroup in (1, 3):
            ref = batched.IntegratedPlan(scheme, cols, bands, _weights(torch, ngroup, nb), profiles=True)()
            torch.cuda.synchronize()
            _check_finish(cols, ref)


def test_argument_errors_write_nothing():
    import torch

    from crt1d_amd import _lib, batched

    lib = _lib.load()
    ncol, nz, ng = 4, 10, 3
    cols, bands = _case(ncol, 12, nz, True, False)
    out = {k: torch.full(sh, 7.0, dtype=torch.float64, device="cuda") for k, sh in batched.bandsum_shapes(ncol, nz, ng, True).items()}
    keys8 = ("aI", "aI_sl", "aI_sh", "I_dr", "I_df_d", "I_df_u", "F", "I_d")
    s = torch.cuda.current_stream().cuda_stream

    def call(c=None, ngroup=ng, o=None, null=None):
        c = cols.c_struct() if c is None else c
        o = _lib.CrtBandsumOut(**{k: out[k].data_ptr() for k in keys8}) if o is None else o
        if null:
            setattr(o, null, None)
        return lib.crt_hip_bandsum_finish_f64(ctypes.byref(c), ngroup, ctypes.byref(o) if o is not False else None, s)

    for k in keys8:
        assert call(null=k) == _lib.CRT_ERR_BAD_ARG, k
    assert call(o=False) == _lib.CRT_ERR_BAD_ARG
    assert lib.crt_hip_bandsum_finish_f64(None, ng, ctypes.byref(_lib.CrtBandsumOut(**{k: out[k].data_ptr() for k in keys8})), s) == _lib.CRT_ERR_BAD_ARG
    for g in (0, 5, -1):
        assert call(ngroup=g) == _lib.CRT_ERR_BAD_ARG, g
    c = cols.c_struct()
    c.psi = None
    assert call(c=c) == _lib.CRT_ERR_BAD_ARG
    for n_col, n_z in ((0, nz), (-3, nz), (ncol, 1), (ncol, 0)):
        c = cols.c_struct()
        c.ncol, c.nz = n_col, n_z
        assert call(c=c) == _lib.CRT_ERR_BAD_ARG, (n_col, n_z)
    c = cols.c_struct()
    c.nz = 2**30  # a column's (level, group) index past 32 bits: refused before any launch
    assert call(c=c, ngroup=4) == _lib.CRT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v == 7.0).all()), k
    # and the good call after all of them writes
    assert call() == _lib.CRT_OK
    torch.cuda.synchronize()
    assert torch.equal(out["I_d"], torch.full_like(out["I_d"], 14.0))
    assert torch.equal(out["aI"], torch.full_like(out["aI"], 14.0))
