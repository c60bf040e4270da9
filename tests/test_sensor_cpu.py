"""CPU: the sensor-band entry points (include/crt1d_hip_sensor.h) exist, every argument error is CRT_ERR_BAD_ARG before any launch, and
the host logic of SensorSet, the weight helpers and the plans' own checks."""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from crt1d_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_sensor_entry_points_are_exported(lib):
    from crt1d_amd import _lib

    names = ("crt_hip_sensor_workspace_bytes", "crt_hip_sensor_levels_f64", "crt_hip_sensor_levels_f32",
             "crt_hip_sensor_series_workspace_bytes", "crt_hip_sensor_levels_series_f64")
    assert tuple(sorted(_lib.SENSOR_EXPORTS)) == tuple(sorted(names))
    text = open(os.path.join(ROOT, "include", "crt1d_hip_sensor.h")).read()
    for name in names:
        assert hasattr(lib, name)
        assert name not in _lib.EXPORTS  # crt1d_hip.h keeps its symbol set
        assert name + "(" in text
    assert f"#define CRT_MAX_SENSOR_BANDS {_lib.MAX_SENSOR_BANDS}" in text and _lib.MAX_SENSOR_BANDS == 64
    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3


FAKE = 0x1000


def _args(nz=20, nb=8):
    """Structs whose device pointers are never dereferenced on the host: a VALID call gets as far as the workspace check (no
    workspace -> CRT_ERR_WORKSPACE, no launch)."""
    from crt1d_amd import _lib

    c = _lib.CrtColumns(2, nz, FAKE, FAKE, FAKE, FAKE, FAKE, None, None)
    b = _lib.CrtBands(nb, nb, FAKE, FAKE, FAKE, FAKE, FAKE)
    o = _lib.CrtOptions(0.501, 0, 0)
    out = _lib.CrtSensorOut(FAKE, FAKE, FAKE, FAKE)
    sun = _lib.CrtSunSeries(3, FAKE, None, 0, FAKE, FAKE)
    return c, b, o, out, sun


class _Set:
    """A crt_sensor_set over host arrays that this object keeps alive."""

    def __init__(self, first, count, nsens=None, w=FAKE, null_first=False, null_count=False):
        from crt1d_amd import _lib

        P = ctypes.POINTER(ctypes.c_int32)
        self.f = (ctypes.c_int32 * max(len(first), 1))(*first)
        self.n = (ctypes.c_int32 * max(len(count), 1))(*count)
        self.s = _lib.CrtSensorSet(len(first) if nsens is None else nsens, None if null_first else ctypes.cast(self.f, P),
                                   None if null_count else ctypes.cast(self.n, P), w)


def _call(lib, form, scheme, c, b, o, levels, sens, out, sun=None, nsel=None):
    from crt1d_amd import _lib

    arr = None if levels is None else (ctypes.c_int32 * max(len(levels), 1))(*levels)
    n = len(levels) if nsel is None else nsel
    ref = lambda x: None if x is None else ctypes.byref(x)  # noqa: E731
    sid = _lib.SCHEME_IDS[scheme] if isinstance(scheme, str) else scheme
    tail = (ref(o), arr, n, None if sens is None else ctypes.byref(sens.s), ref(out), None, 0, None)
    if form == "series":
        return lib.crt_hip_sensor_levels_series_f64(sid, ref(c), ref(b), ref(sun), *tail)
    return getattr(lib, f"crt_hip_sensor_levels_{form}")(sid, ref(c), ref(b), *tail)


@pytest.mark.parametrize("form", ["f64", "f32", "series"])
@pytest.mark.parametrize("scheme", ["2s", "n79", "zq_pa"])
def test_sensor_validation_without_gpu(lib, form, scheme):
    from crt1d_amd import _lib

    BAD, WS, nz, nb = _lib.CRT_ERR_BAD_ARG, _lib.CRT_ERR_WORKSPACE, 20, 8
    c, b, o, out, sun = _args(nz, nb)
    if form != "series":
        sun = None
    good = _Set([0, 2, 7, 0], [8, 4, 1, 1])  # whole range, overlapping, one band at each end, any order

    def call(c=c, b=b, o=o, levels=(0, nz - 1), sens=good, out=out, sun=sun, scheme=scheme, nsel=None):
        return _call(lib, form, scheme, c, b, o, None if levels is None else list(levels), sens, out, sun, nsel)

    # a valid call stops at the workspace check: nothing below is rejected for any other reason than the one named
    assert call() == WS
    assert call(sens=_Set(list(range(8)) * 8, [1] * 64)) == WS  # 64 sensor bands
    assert call(out=_lib.CrtSensorOut(None, None, FAKE, None)) == WS  # any single output is enough
    # the sensor set
    assert call(sens=None) == BAD
    assert call(sens=_Set([0], [8], null_first=True)) == BAD
    assert call(sens=_Set([0], [8], null_count=True)) == BAD
    assert call(sens=_Set([0], [8], w=None)) == BAD
    assert call(sens=_Set([0], [8], nsens=0)) == BAD
    assert call(sens=_Set([0], [8], nsens=-1)) == BAD
    assert call(sens=_Set(list(range(8)) * 9, [1] * 72, nsens=65)) == BAD
    assert call(sens=_Set([0, 3], [8, 0])) == BAD  # count < 1
    assert call(sens=_Set([0, 3], [8, -2])) == BAD
    assert call(sens=_Set([-1], [4])) == BAD  # first < 0
    assert call(sens=_Set([1], [8])) == BAD  # first + count > nb
    assert call(sens=_Set([8], [1])) == BAD
    assert call(sens=_Set([0, 2 ** 31 - 1], [8, 2 ** 31 - 1])) == BAD  # (no overflow of first + count)
    # the outputs
    assert call(out=None) == BAD
    assert call(out=_lib.CrtSensorOut(None, None, None, None)) == BAD
    # everything the levels entry rejects
    assert call(c=None) == BAD
    assert call(b=None) == BAD
    assert call(levels=None, nsel=1) == BAD
    assert call(nsel=0) == BAD
    c100 = _args(100, nb)[0]
    assert call(c=c100, levels=range(64)) == WS
    assert call(c=c100, levels=range(65)) == BAD
    assert call(levels=(3, 2)) == BAD
    assert call(levels=(2, 2)) == BAD
    assert call(levels=(-1,)) == BAD
    assert call(levels=(nz,)) == BAD
    assert call(scheme=42) == BAD
    assert call(scheme=-1) == BAD
    assert call(o=_lib.set_tune(_lib.CrtOptions(0.501, 0, 0), {_lib.TUNE_TRI_M: 10})) == BAD
    assert call(o=_lib.CrtOptions(0.501, 5, 0)) == BAD
    if form == "series":
        assert call(sun=None) == BAD
        assert call(sun=_lib.CrtSunSeries(0, FAKE, None, 0, FAKE, FAKE)) == BAD
        assert call(sun=_lib.CrtSunSeries(3, None, None, 0, FAKE, FAKE)) == BAD


# Band slices at 2151 bands and nsel = 2, from the LDS layouts (160 KB per workgroup, slices of 1024 lanes halved until
# the per-lane bytes x lanes + the record fit).  Per lane: 2s 32 B (staging row only) -> 1024 lanes, 3 slices of 717 at any depth;
# n79 16 B per checkpoint pair x ((nz - 1) // 8 + 1 pairs) + 32 B: 80 B at 20 levels -> 3 slices, 160 B at 60 levels -> 512 lanes, 5 slices
# of 431; zq_pa at a grid of Mg = min(nz, 100) rows 16 B x (Mg // 8 + 1) + 16 B x min(Mg, 3 nsel) kept rows + 32 B: 176 B at 20 levels,
# 256 B at 60 -> 512 lanes, 5 slices.  The slice bounds are part of the summation-order contract.
NSLICE_2151 = {("2s", 20): 3, ("2s", 60): 3, ("n79", 20): 3, ("n79", 60): 5, ("zq_pa", 20): 5, ("zq_pa", 60): 5}


@pytest.mark.parametrize("case", sorted(NSLICE_2151))
def test_sensor_workspace_sizes(lib, case):
    """The records of the levels entries come first; partial sums follow only where the call runs several band slices."""
    from crt1d_amd import _lib

    scheme, nz = case
    sid = _lib.SCHEME_IDS[scheme]
    rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, 300)
    assert lib.crt_hip_sensor_workspace_bytes(sid, 5, nz, 300, 2, 13) == rec  # one slice
    rec = lib.crt_hip_workspace_bytes_nb(sid, 5, nz, 2151)
    one = 5 * 2 * 4 * 13 * 8  # [ncol][nsel][4][nsens] doubles per slice
    assert lib.crt_hip_sensor_workspace_bytes(sid, 5, nz, 2151, 2, 13) == rec + NSLICE_2151[case] * one
    rec = lib.crt_hip_levels_series_workspace_bytes(sid, 5, nz, 4)
    assert lib.crt_hip_sensor_series_workspace_bytes(sid, 5, nz, 2151, 4, 2, 13) == rec + 4 * NSLICE_2151[case] * one
    assert lib.crt_hip_sensor_workspace_bytes(sid, 0, nz, 300, 2, 13) == 0
    assert lib.crt_hip_sensor_workspace_bytes(42, 5, nz, 300, 2, 13) == 0


def test_sensor_set_from_dense_weights():
    from crt1d_amd.batched import SensorSet

    nb = 12
    w = np.zeros((4, nb))
    w[0, 3] = 2.0  # a one-band support
    w[1, 2:7] = [1.0, 0.0, 0.0, 3.0, 4.0]  # interior zeros are kept
    w[2, 5:12] = np.arange(1, 8)  # overlaps sensor band 1, reaches the last band
    w[3, 0] = -1.0  # first band, a negative weight is a weight
    s = SensorSet(w)
    assert s.nsens == 4 and s.nb == nb
    assert s.first.dtype == np.int32 and s.count.dtype == np.int32
    assert s.first.tolist() == [3, 2, 5, 0] and s.count.tolist() == [1, 5, 7, 1]
    assert s.offsets.tolist() == [0, 1, 6, 13]
    assert s.w.dtype.is_floating_point and s.w.numel() == 14
    assert s.w.cpu().numpy().tolist() == [2.0, 1.0, 0.0, 0.0, 3.0, 4.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, -1.0]
    assert np.array_equal(s.dense(), w)
    assert SensorSet(np.ones(nb)).count.tolist() == [nb]  # one row given as a vector
    c = s.c_struct()
    assert c.nsens == 4 and [c.first[i] for i in range(4)] == [3, 2, 5, 0] and [c.count[i] for i in range(4)] == [1, 5, 7, 1]


def test_sensor_set_refusals():
    from crt1d_amd.batched import SensorSet

    w = np.ones((3, 10))
    w[1] = 0.0
    with pytest.raises(ValueError, match="no nonzero weight"):
        SensorSet(w)
    with pytest.raises(ValueError, match="1 .. 64"):
        SensorSet(np.ones((65, 10)))
    with pytest.raises(ValueError, match="1 .. 64"):
        SensorSet(np.ones((0, 10)))
    with pytest.raises(ValueError, match=r"\(nsens, nb\)"):
        SensorSet(np.ones((2, 3, 4)))
    s = SensorSet(np.ones((2, 10)))
    with pytest.raises(ValueError, match="built for nb = 10"):  # a wrong nb: what a plan checks against its bands
        s.check(11, s.w.device)
    s.check(10, s.w.device)


def test_sensor_set_from_supports():
    from crt1d_amd.batched import SensorSet

    s = SensorSet.from_supports([4, 0], [3, 2], np.array([1.0, 2.0, 3.0, 4.0, 5.0]), nb=8)
    assert s.first.tolist() == [4, 0] and s.count.tolist() == [3, 2] and s.nsens == 2
    d = np.zeros((2, 8))
    d[0, 4:7] = [1.0, 2.0, 3.0]
    d[1, 0:2] = [4.0, 5.0]
    assert np.array_equal(s.dense(), d)
    free = SensorSet.from_supports([4], [3], np.ones(3))  # nb unknown until a plan checks it
    free.check(7, free.w.device)
    with pytest.raises(ValueError, match="beyond nb = 6"):
        free.check(6, free.w.device)
    for first, count, w, what in (([0], [0], [], "count >= 1"), ([-1], [2], [1.0, 1.0], "first >= 0"), ([7], [2], [1.0, 1.0], "beyond nb"),
                                  ([0], [2], [1.0], "sum\\(count\\)"), ([0, 1], [2], [1.0, 1.0], "one shape"), ([0.5], [2], [1.0, 1.0], "integer")):
        with pytest.raises(ValueError, match=what):
            SensorSet.from_supports(first, count, np.asarray(w, dtype=float), nb=8)
    with pytest.raises(ValueError, match="1 .. 64"):
        SensorSet.from_supports(list(range(65)), [1] * 65, np.ones(65))


def test_boxcar_sensor_weights():
    from crt1d_amd.spectra import boxcar_sensor_weights, x_frac_in_bounds

    wle = np.linspace(0.4, 1.0, 13)  # 12 bands of 0.05
    w = boxcar_sensor_weights(wle, [(0.45, 0.525), (0.8, 0.9), (0.4, 1.0)])
    assert w.shape == (3, 12)
    assert np.allclose(w[0], [0, 1, 0.5, 0, 0, 0, 0, 0, 0, 0, 0, 0])
    assert np.array_equal(w[1], x_frac_in_bounds(wle, (0.8, 0.9)))
    assert np.array_equal(w[2], np.ones(12))
    assert boxcar_sensor_weights(wle, (0.45, 0.525)).shape == (1, 12)
    with pytest.raises(ValueError, match=r"\(nsens, 2\)"):
        boxcar_sensor_weights(wle, [(0.4, 0.5, 0.6)])


def test_sensor_weights_argument_errors():
    from crt1d_amd.spectra import sensor_weights

    with pytest.raises(ValueError, match=r"\(nsens, nx\)"):
        sensor_weights(np.linspace(0.4, 1.0, 13), np.linspace(0.3, 1.1, 50), np.ones(50))
    with pytest.raises(ValueError, match="band edges"):
        sensor_weights(np.array([0.4]), np.linspace(0.3, 1.1, 50), np.ones((2, 50)))


def test_sensor_plan_python_errors_need_no_device():
    from crt1d_amd import batched

    w = np.ones((2, 8))
    for cls, args in ((batched.SensorLevelsPlan, (None, None, (0,), w)), (batched.SensorLevelsSeriesPlan, (None, None, None, (0,), w))):
        with pytest.raises(ValueError, match="unknown scheme"):
            cls("nope", *args)
        with pytest.raises(ValueError, match="invalid `method`"):
            cls("2s", *args, tau_d_method="nope")
        with pytest.raises(ValueError, match="keys must be distinct"):
            cls("2s", *args, keys=("I_dr", "x0"))
    with pytest.raises(TypeError, match="must be a SensorSet"):  # dense weights are not taken silently: the set is built once, by the caller
        batched.SensorLevelsPlan("2s", None, None, (0,), w)
    with pytest.raises(TypeError, match="SunSeries"):
        batched.SensorLevelsSeriesPlan("2s", None, None, "sun", (0,), batched.SensorSet(w))
