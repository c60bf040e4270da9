"""GPU: which kernel the host launchers pick (``crt_hip_last_kernel``), for every scheme and every output form, against the strings
recorded in ``tests/golden/launch_reports.json`` (written by ``tools/gen_launch_reports.py`` from the library of the commit BEFORE the
launchers were folded into one skeleton per output form).  The kernels' code is compared elsewhere (tools/device_code_diff.py); this
pins what that cannot see: slices, launch-bound rung, M, store waves, LDS bytes, record in LDS or HBM, the finish kernel.

Shapes are tiny in columns (3) and levels (12); the band counts reach every rung and branch: 8 (packed forms, 256 rung), 38 and 107
(narrow even / odd flat flush), 300 (512 rung), 600 (1024 rung), 1100 (levels and sensors: two band slices, k_sens_finish).  The deep
cases of the JSON (``"deep"``) add, per family, the smallest nz at which the recorded library reports M=16 for levels, the closed family's
smallest nz with the record in HBM, and the nz just below each."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
JAC_SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")
NCOL, NZ, NT, NSENS = 3, 12, 2, 3
NBS = (8, 38, 107, 300, 600)
NB_SLICED = 1100  # levels and sensors only: the integrated kernels serve nb <= 1024
# form -> (storage types, takes NB_SLICED)
FORMS = {
    "profiles": (("f64", "f32"), False),
    "integrated": (("f64", "f32"), False),
    "integrated+profiles": (("f64", "f32"), False),
    "integrated_series": (("f64",), False),
    "levels": (("f64", "f32"), True),
    "levels_series": (("f64", "f32"), True),
    "sensor": (("f64", "f32"), True),
    "sensor_series": (("f64",), True),
    "jacobian": (("f64",), False),
}
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_reports.json")

_inputs = {}


def _case(nb, nz, dtype):
    """Columns, bands, sun series, band weights and sensor set of one (nb, nz, storage type), built once."""
    key = (nb, nz, dtype)
    if key not in _inputs:
        from crt1d_amd import batched, synth

        d = synth.make_columns(NCOL, nb, nz, seed=5)
        s = synth.make_sun_series(d, NT, seed=6)
        cols = batched.Columns.from_host(d, DEV)
        bands = batched.Bands.from_host(d, DEV)
        if dtype == "f32":
            bands = batched.Bands(*[getattr(bands, k).to(torch.float32) for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
            sun = batched.SunSeriesF32.from_host(s, DEV)
        else:
            sun = batched.SunSeries.from_host(s, DEV)
        band_w = torch.as_tensor(np.random.default_rng(7).uniform(0.1, 1.0, (2, nb))).to(DEV)
        sensors = batched.SensorSet(np.random.default_rng(8).uniform(0.1, 1.0, (NSENS, nb)), device=DEV)
        _inputs[key] = cols, bands, sun, band_w, sensors
    return _inputs[key]


def report(form, scheme, dtype, nb, nz=NZ):
    """The launch report of one call of `form` (or the error of a call that is refused)."""
    from crt1d_amd import batched

    cols, bands, sun, band_w, sensors = _case(nb, nz, dtype)
    levels = (0, nz // 2, nz - 1)
    with torch.cuda.device(DEV):
        if form == "profiles":
            plan = batched.Plan(scheme, cols, bands)
        elif form == "integrated":
            plan = batched.IntegratedPlan(scheme, cols, bands, band_w)
        elif form == "integrated+profiles":
            plan = batched.IntegratedPlan(scheme, cols, bands, band_w, profiles=True)
        elif form == "integrated_series":
            plan = batched.IntegratedSeriesPlan(scheme, cols, bands, sun, band_w)
        elif form == "levels":
            plan = batched.LevelsPlan(scheme, cols, bands, levels)
        elif form == "levels_series":
            plan = batched.LevelsSeriesPlan(scheme, cols, bands, sun, levels)
        elif form == "sensor":
            plan = batched.SensorLevelsPlan(scheme, cols, bands, levels, sensors)
        elif form == "sensor_series":
            plan = batched.SensorLevelsSeriesPlan(scheme, cols, bands, sun, levels, sensors)
        elif form == "jacobian":
            plan = batched.LevelsJacPlan(scheme, cols, bands, levels)
        else:
            raise ValueError(form)
        try:
            plan()
        except RuntimeError as e:  # a shape the entry does not serve (zq_pa with f32 storage below 16 bands): the status is the report
            return f"RuntimeError: {e}"
        torch.cuda.synchronize()
        return plan.last_kernel()


def shallow_cases(scheme):
    """(form, storage type, nb) of every case of `scheme` at NZ levels."""
    for form, (dtypes, sliced) in FORMS.items():
        if form == "jacobian" and scheme not in JAC_SCHEMES:
            continue
        for dtype in dtypes:
            for nb in NBS + ((NB_SLICED,) if sliced else ()):
                yield form, dtype, nb


def case_id(form, scheme, dtype, nb, nz):
    return f"{form}/{scheme}/{dtype}/nb={nb}/nz={nz}"


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_launch_reports(golden, scheme):
    want = golden["reports"]
    bad = []
    n = 0
    for form, dtype, nb in shallow_cases(scheme):
        cid = case_id(form, scheme, dtype, nb, NZ)
        got = report(form, scheme, dtype, nb)
        n += 1
        if got != want[cid]:
            bad.append((cid, got, want[cid]))
    assert n == sum(1 for k in want if k.split("/")[1] == scheme and k.endswith(f"nz={NZ}")), "the JSON has cases this test does not run"
    assert not bad, bad


def test_launch_reports_deep(golden):
    """Per family, the first nz at which levels take M=16 (n79, zq; k_zqpa_lev has M = 8 only) or the record stays in HBM (closed)."""
    deep = golden["deep"]
    assert set(deep) == {"n79", "zq", "2s"}
    for scheme, e in deep.items():
        for nz in (e["nz"] - 1, e["nz"]):
            cid = case_id("levels", scheme, "f64", 8, nz)
            assert report("levels", scheme, "f64", 8, nz) == golden["reports"][cid], cid
        assert e["marker"] in golden["reports"][case_id("levels", scheme, "f64", 8, e["nz"])]
        assert e["marker"] not in golden["reports"][case_id("levels", scheme, "f64", 8, e["nz"] - 1)]
