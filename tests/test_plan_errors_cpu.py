"""CPU: what each of the five solve plans raises for an input with exactly one fault, for every fault that is found without a device.
The expectations (exception type and a distinctive fragment of the message) were recorded from the constructors before they were given
one base class."""
import os
import types

import pytest


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


NZ, NB, NCOL, NT = 5, 4, 3, 6


def _stubs(torch, _lib, dtype):
    """Stand-ins for Columns / Bands with everything a constructor reads before it needs device memory (a real Columns asks for CUDA
    tensors); nothing here is a tensor, so a constructor that got past its argument checks fails on the first allocation."""
    dev = torch.device("cpu")
    cols = types.SimpleNamespace(ncol=NCOL, nz=NZ, device=dev, mla=object(), g_table=None, g_at_psi=None, g_kind=torch.zeros(NCOL, dtype=torch.int32),
                                 check_tables=lambda: None, c_struct=lambda: _lib.CrtColumns())
    bands = types.SimpleNamespace(nb=NB, dtype=dtype, I_dr0=None, I_df0=None, leaf_r=None, leaf_t=None, soil_r=None,
                                  c_struct=lambda ncol: _lib.CrtBands())
    return cols, bands


# (plan, overrides of the valid arguments, exception, fragment of the message)
S, M, K, L = "scheme", "tau_d_method", "keys", "levels"
CASES = [
    ("Plan", {S: "nope"}, ValueError, "unknown scheme 'nope'; valid: 2s, 4s, n79, zq, bl, g77, bf, zq_pa"),
    ("Plan", {M: "simpson"}, ValueError, "invalid `method`. Valid options are 'quad' and '9sky'."),
    ("Plan", {"placement": "fast"}, ValueError, "placement must be 'auto' or 'none'"),
    ("Plan", {"placement": None}, ValueError, "placement must be 'auto' or 'none'"),
    ("IntegratedPlan", {S: "nope"}, ValueError, "scheme 'nope' has no integrated kernel"),
    ("IntegratedPlan", {M: "simpson"}, ValueError, "invalid `method`. Valid options are 'quad' and '9sky'."),
    ("IntegratedPlan", {"band_w": "5x4"}, ValueError, "band_w must be (ngroup <= 4, nb)"),
    ("IntegratedPlan", {"band_w": "2x3"}, ValueError, "band_w must be (ngroup <= 4, nb)"),
    ("IntegratedPlan", {"band_w": "f32"}, TypeError, "band_w must be torch.float64"),
    ("IntegratedSeriesPlan", {S: "nope"}, ValueError, "scheme 'nope' has no integrated kernel"),
    ("IntegratedSeriesPlan", {M: "simpson"}, ValueError, "invalid `method`. Valid options are 'quad' and '9sky'."),
    ("IntegratedSeriesPlan", {"sun": "dict"}, TypeError, "sun must be a SunSeries (float64 spectra)"),
    ("IntegratedSeriesPlan", {"sun": "f32"}, TypeError, "sun must be a SunSeries (float64 spectra)"),
    ("IntegratedSeriesPlan", {"bands": "f32"}, TypeError, "the sun-angle series has no f32 storage form: bands must be float64"),
    ("IntegratedSeriesPlan", {"band_w": "5x4"}, ValueError, "band_w must be (ngroup <= 4, nb)"),
    ("LevelsPlan", {S: "nope"}, ValueError, "unknown scheme 'nope'; valid: 2s, 4s, n79, zq, bl, g77, bf, zq_pa"),
    ("LevelsPlan", {M: "simpson"}, ValueError, "invalid `method`. Valid options are 'quad' and '9sky'."),
    ("LevelsPlan", {K: ()}, ValueError, "keys must be distinct names out of ('I_dr', 'I_df_d', 'I_df_u', 'F'), got ()"),
    ("LevelsPlan", {K: ("I_d",)}, ValueError, "keys must be distinct names out of ('I_dr', 'I_df_d', 'I_df_u', 'F'), got ('I_d',)"),
    ("LevelsPlan", {K: ("F", "F")}, ValueError, "keys must be distinct names out of ('I_dr', 'I_df_d', 'I_df_u', 'F'), got ('F', 'F')"),
    ("LevelsPlan", {K: "aI"}, ValueError, "got ('aI',)"),
    ("LevelsPlan", {L: 5}, ValueError, "level 5 is out of range for nz = 5 (valid: -5 .. 4)"),
    ("LevelsPlan", {L: (0, -6)}, ValueError, "level -6 is out of range for nz = 5 (valid: -5 .. 4)"),
    ("LevelsPlan", {L: (1, -4)}, ValueError, "level(s) [1] selected more than once (negative indices count from nz = 5)"),
    ("LevelsPlan", {L: ()}, ValueError, "levels is empty: select at least one level"),
    ("LevelsPlan", {L: (0, 1.5)}, ValueError, "levels must be integers"),
    ("LevelsPlan", {L: "65 of 100"}, ValueError, "65 levels selected; one call serves at most 64"),
    ("LevelsSeriesPlan", {S: "nope"}, ValueError, "unknown scheme 'nope'; valid: 2s, 4s, n79, zq, bl, g77, bf, zq_pa"),
    ("LevelsSeriesPlan", {M: "simpson"}, ValueError, "invalid `method`. Valid options are 'quad' and '9sky'."),
    ("LevelsSeriesPlan", {"sun": "dict"}, TypeError, "sun must be a SunSeries or a SunSeriesF32"),
    ("LevelsSeriesPlan", {K: ()}, ValueError, "keys must be distinct names out of ('I_dr', 'I_df_d', 'I_df_u', 'F'), got ()"),
    ("LevelsSeriesPlan", {K: ("I_d",)}, ValueError, "got ('I_d',)"),
    ("LevelsSeriesPlan", {K: ("F", "F")}, ValueError, "got ('F', 'F')"),
    ("LevelsSeriesPlan", {L: 5}, ValueError, "level 5 is out of range for nz = 5 (valid: -5 .. 4)"),
    ("LevelsSeriesPlan", {L: (1, -4)}, ValueError, "level(s) [1] selected more than once (negative indices count from nz = 5)"),
    ("LevelsSeriesPlan", {L: "65 of 100"}, ValueError, "65 levels selected; one call serves at most 64"),
    ("LevelsSeriesPlan", {"sun": "f32"}, TypeError, "torch.float64 bands need a SunSeries: the spectra of sun are torch.float32"),
    ("LevelsSeriesPlan", {"bands": "f32"}, TypeError, "torch.float32 bands need a SunSeriesF32: the spectra of sun are torch.float64"),
]


@pytest.mark.parametrize("plan,fault,exc,fragment", CASES, ids=[f"{c[0]}-{'-'.join(c[1])}-{i}" for i, c in enumerate(CASES)])
def test_single_fault_raises_what_it_always_did(lib, monkeypatch, plan, fault, exc, fragment):
    import torch

    from crt1d_amd import _lib, batched

    f64, f32 = torch.float64, torch.float32

    def host(dtype):  # the dtype rule of batched._f64 / _f32 without its demand for a CUDA tensor (test_levels_series_cpu.py)
        def f(t, name):
            if t.dtype != dtype:
                raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
            return t.contiguous()
        return f

    monkeypatch.setattr(batched, "_f64", host(f64))
    monkeypatch.setattr(batched, "_f32", host(f32))
    cols, bands = _stubs(torch, _lib, f32 if fault.get("bands") == "f32" else f64)
    bands.soil_r = bands.leaf_r = bands.leaf_t = types.SimpleNamespace(device=cols.device)
    psi = torch.zeros(NCOL, NT, dtype=f64)
    suns = {
        None: lambda: batched.SunSeries(psi, torch.zeros(NCOL, NT, NB, dtype=f64), torch.zeros(NCOL, NT, NB, dtype=f64)),
        "f32": lambda: batched.SunSeriesF32(psi, torch.zeros(NCOL, NT, NB, dtype=f32), torch.zeros(NCOL, NT, NB, dtype=f32)),
        "dict": lambda: {"psi": psi},
    }
    weights = {None: torch.ones(2, NB, dtype=f64), "5x4": torch.ones(5, NB, dtype=f64), "2x3": torch.ones(2, NB - 1, dtype=f64),
               "f32": torch.ones(2, NB, dtype=f32)}
    levels = fault.get(L, (0, -1))
    if levels == "65 of 100":
        cols.nz, levels = 100, range(65)
    sun, band_w = suns[fault.get("sun")](), weights[fault.get("band_w")]
    scheme = fault.get(S, "2s")
    kw = {M: fault[M]} if M in fault else {}
    build = {
        "Plan": lambda: batched.Plan(scheme, cols, bands, **kw, **({"placement": fault["placement"]} if "placement" in fault else {})),
        "IntegratedPlan": lambda: batched.IntegratedPlan(scheme, cols, bands, band_w, **kw),
        "IntegratedSeriesPlan": lambda: batched.IntegratedSeriesPlan(scheme, cols, bands, sun, band_w, **kw),
        "LevelsPlan": lambda: batched.LevelsPlan(scheme, cols, bands, levels, **kw, **({K: fault[K]} if K in fault else {})),
        "LevelsSeriesPlan": lambda: batched.LevelsSeriesPlan(scheme, cols, bands, sun, levels, **kw, **({K: fault[K]} if K in fault else {})),
    }[plan]
    with pytest.raises(exc) as e:
        build()
    assert type(e.value) is exc and fragment in str(e.value), str(e.value)
