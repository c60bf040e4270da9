"""GPU: what the four inverse-problem entries with a parameter axis report (``crt_hip_last_kernel``) -- SensorJacPlan, SensorJacSeriesPlan,
SpectralNormalPlan, SpectralNormalSeriesPlan -- for 2s and bl (bl keeps a LAI side record, 2s none), with and without ``lai``, with and
without a leaf-angle tangent, one direction throughout: the report of a ``FLAG_PRECOMPUTE_ONLY`` call (the column precompute and the side
precomputes that ran) and that of a plain call.  The shape is the smallest at which every side record and the series path exist: two
columns, four levels, three bands, one selected level, one sensor band over the three bands, two sun states.  The strings of
``tests/golden/inverse_reports.json`` are what :func:`reports` gave with the library as it was before the host code of these entries was
folded into one parse and one side-precompute object; only the public API is used."""
import itertools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCOL, NZ, NB, NT = 2, 4, 3, 2
DEV = "cuda:0"
PLANS = ("SensorJacPlan", "SensorJacSeriesPlan", "SpectralNormalPlan", "SpectralNormalSeriesPlan")
CASES = list(itertools.product(PLANS, ("2s", "bl"), (False, True), (False, True)))  # plan, scheme, lai, tangent

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inverse_reports.json")

_inputs = {}


def _case():
    if not _inputs:
        from crt1d_amd import batched, synth

        d = synth.make_columns(NCOL, NB, NZ, seed=5)
        cols, bands = batched.Columns.from_host(d, DEV), batched.Bands.from_host(d, DEV)
        sun = batched.SunSeries.from_host(synth.make_sun_series(d, NT, seed=6), DEV)
        sensors = batched.SensorSet.from_supports(np.array([0]), np.array([NB]), np.ones(NB), nb=NB, device=DEV)
        _inputs.update(cols=cols, bands=bands, sun=sun, sensors=sensors, tan=batched.leaf_tangent(cols, "param"),
                       tan_series=batched.leaf_tangent_series(cols, sun, "param"))
    return _inputs


def reports(plan, scheme, lai, tangent):
    """(the report of a FLAG_PRECOMPUTE_ONLY call, the report of a plain call) of one plan."""
    from crt1d_amd import _lib, batched

    c = _case()
    series = plan.endswith("SeriesPlan")
    kw = dict(d_leaf_r=np.full((1, NB), 0.5), lai=lai, tangent=(c["tan_series"] if series else c["tan"]) if tangent else None)
    a = (scheme, c["cols"], c["bands"]) + ((c["sun"],) if series else ())
    if plan.startswith("SensorJac"):
        p = getattr(batched, plan)(*a, (1,), c["sensors"], **kw)
    else:
        y = {"I_df_d": torch.ones((NCOL, *((NT,) if series else ()), 1, NB), dtype=torch.float64, device=DEV)}
        p = getattr(batched, plan)(*a, (1,), y, keys=("I_df_d",), **kw)
    p(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    pre = p.last_kernel()
    p()
    torch.cuda.synchronize()
    return pre, p.last_kernel()


@pytest.mark.parametrize("plan,scheme,lai,tangent", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_reports_are_those_recorded(plan, scheme, lai, tangent):
    expected = {tuple(case): tuple(r) for case, r in json.load(open(GOLDEN))}
    got = reports(plan, scheme, lai, tangent)
    print(got)
    assert got == expected[plan, scheme, lai, tangent]
