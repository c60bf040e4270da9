"""CPU: the level-subset entry points (crt_hip_levels_f64 / _f32) exist, and every argument error is CRT_ERR_BAD_ARG before any launch;
the level normalisation of LevelsPlan is host logic."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_levels_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    for name in ("crt_hip_levels_f64", "crt_hip_levels_f32"):
        assert hasattr(lib, name)
        assert name in _lib.EXPORTS
    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    assert "#define CRT_MAX_LEVEL_SELECT 64" in text and _lib.MAX_LEVEL_SELECT == 64


def _args(nz=20, nb=8):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no
    workspace -> CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    fake = 0x1000
    c = _lib.CrtColumns(2, nz, fake, fake, fake, fake, fake, None, None)
    b = _lib.CrtBands(nb, nb, fake, fake, fake, fake, fake)
    o = _lib.CrtOptions(0.501, 0, 0)
    out = _lib.CrtOutputs(fake, fake, fake, fake, None, None, None)
    return c, b, o, out


def _call(lib, suffix, scheme, c, b, o, levels, out, nsel=None):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    fn = getattr(lib, f"crt_hip_levels_{suffix}")
    return fn(_lib.SCHEME_IDS.get(scheme, scheme) if isinstance(scheme, str) else scheme, None if c is None else ctypes.byref(c),
              None if b is None else ctypes.byref(b), ctypes.byref(o), arr, n, None if out is None else ctypes.byref(out), None, 0, None)


@pytest.mark.parametrize("suffix", ["f64", "f32"])
@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_levels_validation_without_gpu(lib, suffix, scheme):
    from crt1d_amd import _lib

    BAD, nz = _lib.CRT_ERR_BAD_ARG, 20
    c, b, o, out = _args(nz)
    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert _call(lib, suffix, scheme, c, b, o, [0, nz - 1], out) == _lib.CRT_ERR_WORKSPACE
    assert _call(lib, suffix, scheme, c, b, o, list(range(nz)), out) == _lib.CRT_ERR_WORKSPACE
    assert _call(lib, suffix, scheme, None, b, o, [0], out) == BAD  # null columns
    assert _call(lib, suffix, scheme, c, None, o, [0], out) == BAD  # null bands
    assert _call(lib, suffix, scheme, c, b, o, None, out, nsel=1) == BAD  # null levels
    assert _call(lib, suffix, scheme, c, b, o, [0], None) == BAD  # null outputs
    assert _call(lib, suffix, scheme, c, b, o, [0], out, nsel=0) == BAD
    c65, _, _, _ = _args(100)
    assert _call(lib, suffix, scheme, c65, b, o, list(range(64)), out) == _lib.CRT_ERR_WORKSPACE
    assert _call(lib, suffix, scheme, c65, b, o, list(range(65)), out) == BAD  # nsel 65
    assert _call(lib, suffix, scheme, c, b, o, [3, 2], out) == BAD  # unsorted
    assert _call(lib, suffix, scheme, c, b, o, [2, 2], out) == BAD  # duplicate
    assert _call(lib, suffix, scheme, c, b, o, [-1], out) == BAD  # negative
    assert _call(lib, suffix, scheme, c, b, o, [nz], out) == BAD  # >= nz
    assert _call(lib, suffix, scheme, c, b, o, [0, nz], out) == BAD
    none = _lib.CrtOutputs(None, None, None, None, None, None, None)
    assert _call(lib, suffix, scheme, c, b, o, [0], none) == BAD  # all four outputs NULL
    one = _lib.CrtOutputs(None, None, 0x1000, None, None, None, None)
    assert _call(lib, suffix, scheme, c, b, o, [0], one) == _lib.CRT_ERR_WORKSPACE  # any single output is enough
    for x in ("x0", "x1", "x2"):
        extra = _lib.CrtOutputs(0x1000, 0x1000, 0x1000, 0x1000, None, None, None)
        setattr(extra, x, 0x1000)
        assert _call(lib, suffix, scheme, c, b, o, [0], extra) == BAD, x
    assert _call(lib, suffix, 42, c, b, o, [0], out) == BAD  # unknown scheme
    assert _call(lib, suffix, -1, c, b, o, [0], out) == BAD
    o_bad = _lib.set_tune(_lib.CrtOptions(0.501, 0, 0), {_lib.TUNE_TRI_M: 10})  # tune is validated as for the solve
    assert _call(lib, suffix, scheme, c, b, o_bad, [0], out) == BAD
    o_bad = _lib.CrtOptions(0.501, 5, 0)  # unknown tau_d method
    assert _call(lib, suffix, scheme, c, b, o_bad, [0], out) == BAD


def test_levels_shape_errors_follow_the_solve(lib):
    from crt1d_amd import _lib

    c, b, o, out = _args(nz=2)
    assert _call(lib, "f64", "n79", c, b, o, [0, 1], out) == _lib.CRT_ERR_SHAPE  # n79 needs nz >= 3, as its solve
    assert _call(lib, "f64", "2s", c, b, o, [0, 1], out) == _lib.CRT_ERR_WORKSPACE


def test_normalize_levels():
    import numpy as np

    from crt1d_amd.batched import normalize_levels

    assert normalize_levels([-1, 0], 60) == (0, 59)
    assert normalize_levels(-1, 60) == (59,)
    assert normalize_levels(np.int64(7), 60) == (7,)
    assert normalize_levels(np.array([5, -2, 0]), 9) == (0, 5, 7)
    assert normalize_levels(range(0, 60, 7), 60) == tuple(range(0, 60, 7))
    assert normalize_levels(range(64), 64) == tuple(range(64))
    for bad, what in (([60], "out of range"), ([-61], "out of range"), ([3, 3], "more than once"), ([-1, 59], "more than once"),
                      ([], "empty"), ([1.5], "integer"), (list(range(65)), "at most")):
        with pytest.raises(ValueError, match=what):
            normalize_levels(bad, 60 if what != "at most" else 100)
