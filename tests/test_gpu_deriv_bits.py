"""GPU: the output BITS of the three level-derivative entries (crt_hip_levels_jac_f64, crt_hip_levels_dlai_f64, crt_hip_levels_dleaf_f64
through their plans) against the SHA-256 digests of ``tests/golden/deriv_bits.json``, written by ``tools/gen_deriv_bits.py`` from the
package and library of the commit BEFORE the three entries were given one host path.  The kernels' code is compared elsewhere
(tools/device_code_diff.py); this pins what that cannot see: grids, LDS sizes, the side record's offset and length, argument order, the
flag handling.  Equality only: there is no tolerance to judge.

Cases: the six schemes on the shallow shapes of tests/test_gpu_jac.py that have an odd band count and a single band, n79 / zq also on its
deep shapes (the 32- and 16-lane slices, the last slice partial); uniform and ragged dLAI; n79 with both tau_d methods; the LAI derivative
per log and per LAI; the leaf-angle derivative along ``leaf_tangent(wrt="param")`` of ellipsoidal columns.  Each case records one plain
call, and one ``FLAG_PRECOMPUTE_ONLY`` call followed by a ``FLAG_SKIP_PRECOMPUTE`` call of a new plan on a zeroed workspace.

The three fused entries of the closed forms (crt_hip_levels_grad_f64, crt_hip_sensor_jac_f64, crt_hip_sensor_jac_series_f64 through
LevelsGradPlan, SensorJacPlan, SensorJacSeriesPlan) are pinned the same way, their digests written from the commit BEFORE
csrc/deriv_passes.hpp gave k_grad the pass code of the single-derivative kernels (sens_jac_body has a copy of its own to keep in
step): ellipsoidal columns, every output and every parameter (three directions, the LAI,
the leaf angle along ``leaf_tangent(wrt="param")``), seeded weights and directions; the two shallow shapes, (2, 257, 4) -- two band
slices: k_grad_finish and k_sens_jac_finish run -- and, for the two sensor entries, (2, 130, 20) with 16 levels, whose staging rows force
the 64-lane slices (tests/test_gpu_sensjac_series.py); the series with three sun states."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_jac import DEEP_SHAPES, _host, _levels
from test_gpu_sensjac_series import L16, _dirs, _sensors

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "bl", "g77", "bf", "n79", "zq")
TRI = ("n79", "zq")
SHAPES = [(6, 13, 9), (4, 1, 5)]  # (ncol, nb, nz)
ENTRIES = ("jac", "dlai-log", "dlai-lai", "dleaf")
FUSED = ("grad", "sensjac", "sensjac-series")  # 2s, bl, g77, bf
FUSED_SHAPES = [(6, 13, 9), (4, 1, 5), (2, 257, 4)]
SENSOR_SHAPE = (2, 130, 20)  # levels L16
NT = 3
G_ELLIPSOIDAL = 3  # crt_g_kind
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deriv_bits.json")


def cases():
    """(entry, scheme, shape, uniform, tau_d_method) of every recorded case."""
    for entry in ENTRIES:
        for scheme in SCHEMES:
            for shape in SHAPES + (DEEP_SHAPES if scheme in TRI else []):
                for uniform in (True, False):
                    for method in ("quad", "9sky") if scheme == "n79" else ("quad",):
                        yield entry, scheme, shape, uniform, method
    for entry in FUSED:
        for scheme in SCHEMES[:4]:
            for shape in FUSED_SHAPES + ([] if entry == "grad" else [SENSOR_SHAPE]):
                for uniform in (True, False):
                    yield entry, scheme, shape, uniform, "quad"


def case_id(entry, scheme, shape, uniform, method):
    return f"{entry}/{scheme}/{'x'.join(map(str, shape))}/{'uniform' if uniform else 'ragged'}/{method}"


@functools.lru_cache(maxsize=None)
def _inputs(shape, uniform, ellipsoidal):
    import torch

    from crt1d_amd import batched

    d = dict(_host(shape, uniform))
    if ellipsoidal:
        d["g_kind"] = np.full(shape[0], G_ELLIPSOIDAL, dtype=np.int32)
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    tan = batched.leaf_tangent(cols, "param") if ellipsoidal else None
    torch.cuda.synchronize()
    return cols, bands, tan


@functools.lru_cache(maxsize=None)
def _weights(shape, nsel):
    import torch

    rng = np.random.default_rng(41)
    return {k: torch.as_tensor(rng.uniform(-1.0, 1.0, (shape[0], nsel, shape[1]))).cuda() for k in ("I_dr", "I_df_d", "I_df_u", "F")}


@functools.lru_cache(maxsize=None)
def _sun(shape, uniform):
    from crt1d_amd import batched, synth

    return batched.SunSeries.from_host(synth.make_sun_series(dict(_host(shape, uniform)), NT, seed=77))


def _fused_plan(entry, scheme, shape, uniform):
    from crt1d_amd import batched

    cols, bands, tan = _inputs(shape, uniform, True)
    lev = L16 if shape == SENSOR_SHAPE else _levels(shape[2])
    if entry == "grad":
        return batched.LevelsGradPlan(scheme, cols, bands, lev, _weights(shape, len(lev)), tangent=tan)
    kw = dict(_dirs(shape, uniform, 3, False), lai=True)
    if entry == "sensjac":
        return batched.SensorJacPlan(scheme, cols, bands, lev, _sensors(shape, len(lev)), tangent=tan, **kw)
    sun = _sun(shape, uniform)
    return batched.SensorJacSeriesPlan(scheme, cols, bands, sun, lev, _sensors(shape, len(lev)), tangent=batched.leaf_tangent_series(cols, sun, "param"), **kw)


def _plan(entry, scheme, shape, uniform, method):
    from crt1d_amd import batched

    if entry in FUSED:
        return _fused_plan(entry, scheme, shape, uniform)
    cols, bands, tan = _inputs(shape, uniform, entry == "dleaf")
    lev = _levels(shape[2])
    if entry == "jac":
        return batched.LevelsJacPlan(scheme, cols, bands, lev, tau_d_method=method)
    if entry == "dleaf":
        return batched.LevelsDleafPlan(scheme, cols, bands, lev, tan, tau_d_method=method)
    return batched.LevelsDlaiPlan(scheme, cols, bands, lev, per=entry[5:], tau_d_method=method)


def _digest(out):
    h = hashlib.sha256()
    for k in sorted(out):
        h.update(k.encode())
        h.update(out[k].cpu().numpy().tobytes())
    return h.hexdigest()


def digests(entry, scheme, shape, uniform, method):
    """[plain call, PRECOMPUTE_ONLY + SKIP_PRECOMPUTE pair]: one SHA-256 each over (key, raw bytes) of every output in key order."""
    import torch

    from crt1d_amd import _lib

    plan = _plan(entry, scheme, shape, uniform, method)
    plain = _digest(plan())
    del plan
    plan = _plan(entry, scheme, shape, uniform, method)
    plan.workspace.zero_()  # (the allocator may hand the first plan's block back: the records must come from the call below)
    for v in plan.out.values():
        v.fill_(float("nan"))
    plan(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    pair = _digest(plan(flags=_lib.FLAG_SKIP_PRECOMPUTE))
    torch.cuda.synchronize()
    return [plain, pair]


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_has_these_cases(golden):
    assert set(golden) == {case_id(*c) for c in cases()}


@pytest.mark.parametrize("entry,scheme,shape,uniform,method", [pytest.param(*c, id=case_id(*c)) for c in cases()])
def test_deriv_bits(golden, entry, scheme, shape, uniform, method):
    assert digests(entry, scheme, shape, uniform, method) == golden[case_id(entry, scheme, shape, uniform, method)]
