"""CPU: the C-ABI shared library loads without a GPU and exports every symbol include/crt1d_hip.h declares."""
import ctypes
import os
import re

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


def _declared():
    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(crt_hip_\w+)\s*\(", text)))


def test_every_declared_symbol_is_exported(lib):
    from crt1d_amd import _lib

    names = _declared()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/crt1d_hip.h but not exported"
    assert sorted(_lib.EXPORTS) == names  # the Python binding list tracks the header


def test_struct_layouts_match_header(lib):
    from crt1d_amd import _lib

    assert ctypes.sizeof(_lib.CrtColumns) == 8 + 7 * 8
    assert ctypes.sizeof(_lib.CrtBands) == 8 + 8 + 5 * 8
    assert ctypes.sizeof(_lib.CrtOptions) == 16 + 4 * _lib.NTUNE  # mu_s, tau_d_method, flags, tune[CRT_NTUNE]
    assert ctypes.sizeof(_lib.CrtOutputs) == 7 * 8
    assert ctypes.sizeof(_lib.CrtBandsumOut) == 10 * 8
    # field order of the header's struct
    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    body = text[text.index("typedef struct crt_bandsum_out {"):text.index("} crt_bandsum_out;")]
    assert re.findall(r"double\* (\w+);", body) == [f[0] for f in _lib.CrtBandsumOut._fields_]


def test_host_only_entry_points(lib):
    from crt1d_amd import _lib

    assert lib.crt_hip_abi_version() == _lib.ABI_VERSION == 3
    assert isinstance(lib.crt_hip_last_kernel(), bytes)  # reporting hook; empty before the first solve
    assert _lib.strerror(0) == "ok" and "workspace" in _lib.strerror(_lib.CRT_ERR_WORKSPACE)
    # record = 16-double header + nvec * nz
    assert lib.crt_hip_workspace_bytes(_lib.SCHEME_IDS["2s"], 10, 60) == 10 * (16 + 2 * 60) * 8
    assert lib.crt_hip_workspace_bytes(_lib.SCHEME_IDS["n79"], 10, 60) == 10 * (16 + 7 * 60) * 8
    assert lib.crt_hip_workspace_bytes(99, 10, 60) == 0
    nodes = _lib.quad_nodes(0.501)
    assert nodes.shape == (_lib.NQ,)
    assert np.all((nodes > 0) & (nodes < np.pi / 2))
    # graded rule: 6 panels x 16 nodes, finest panel [0, 1e-4] pi/2 next to pi/2
    assert np.pi / 2 - nodes[:16].min() < (np.pi / 2) * 1e-4
    g4 = nodes[96:128]
    assert np.all(g4[:16] > np.arccos(0.501)) and np.all(g4[16:] < np.arccos(0.501))
    np.testing.assert_allclose(np.rad2deg(nodes[128:]), np.arange(5, 90, 10))
    with pytest.raises(ValueError):
        _lib.quad_nodes(1.5)


def test_quadrature_nodes_integrate_tau_d(lib):
    """The device's fixed tau_d rule, rebuilt on the host from the exported nodes, against a closed form:
    horizontal leaves, K_b = 1  ->  tau_d(L) = exp(-L) exactly; spherical -> 2 E_3(L/2)."""
    from numpy.polynomial.legendre import leggauss
    from scipy.special import expn

    from crt1d_amd import _lib

    psi = _lib.quad_nodes(0.501)[:96]
    x, w = leggauss(16)
    T = np.pi / 2
    edges = [T * f for f in (0.0, 1e-4, 1e-3, 1e-2, 0.1, 0.6, 1.0)]
    wts = np.concatenate([w * (b - a) / 2 for a, b in zip(edges[:-1], edges[1:])])
    for L in (3e-4, 1e-3, 0.0678, 1.0, 8.0):
        td = np.sum(2 * wts * np.exp(-0.5 / np.cos(psi) * L) * np.sin(psi) * np.cos(psi))
        assert abs(td - 2 * expn(3, 0.5 * L)) / (2 * expn(3, 0.5 * L)) < 5e-13
        # ... and 1 - tau_d, the quantity n79 divides by dlai: RELATIVE accuracy down to dlai ~ 3e-4 (the 0.25 grading of rounds 1-2: 6e-9 there)
        om = np.sum(-2 * wts * np.expm1(-0.5 / np.cos(psi) * L) * np.sin(psi) * np.cos(psi))
        import mpmath

        ref = float(1 - 2 * mpmath.expint(3, mpmath.mpf(0.5) * L))
        assert abs(om - ref) / ref < 3e-12, (L, abs(om - ref) / ref)


def test_validation_without_gpu(lib):
    """Argument validation happens before any launch, so it can be exercised on the CPU."""
    from crt1d_amd import _lib

    c, b, o, out = _lib.CrtColumns(), _lib.CrtBands(), _lib.CrtOptions(0.501, 0, 0), _lib.CrtOutputs()
    assert lib.crt_hip_2s_f64(ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), ctypes.byref(out), None, 0, None) == _lib.CRT_ERR_BAD_ARG
    assert lib.crt_hip_solve_f64(42, ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), ctypes.byref(out), None, 0, None) == _lib.CRT_ERR_BAD_ARG
    with pytest.raises(ValueError):
        _lib.check(_lib.CRT_ERR_BAD_ARG, "x")
    with pytest.raises(AssertionError):
        _lib.check(_lib.CRT_ERR_SHAPE, "x")
    with pytest.raises(RuntimeError):
        _lib.check(_lib.CRT_ERR_LAUNCH, "x")


def test_product_does_not_import_the_oracle():
    """The product path must never route through the oracle (or any CPU fallback)."""
    import subprocess
    import sys

    code = "import sys, crt1d_amd, crt1d_amd.batched, crt1d_amd.solvers, crt1d_amd.model, crt1d_amd.dist; " \
           "print(any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules))"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.stdout.strip() == "False", r.stdout + r.stderr
    for dirpath, _, files in os.walk(os.path.join(ROOT, "crt1d_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_tune_values_are_validated_before_any_launch(lib):
    """crt_options.tune is part of the ABI: out-of-range values and non-zero reserved keys are CRT_ERR_BAD_ARG.  The
    pointers below are never dereferenced on the host; a VALID call gets as far as the workspace check (no workspace -> no launch)."""
    from crt1d_amd import _lib

    fake = 0x1000
    c = _lib.CrtColumns(1, 3, fake, fake, fake, fake, fake, None, None)
    b = _lib.CrtBands(4, 4, fake, fake, fake, fake, fake)
    out = _lib.CrtOutputs(fake, fake, fake, fake, fake, fake, fake)

    def call(tune):
        o = _lib.set_tune(_lib.CrtOptions(0.501, 0, 0), tune)
        return lib.crt_hip_zq_f64(ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), ctypes.byref(out), None, 0, None)

    assert call({}) == _lib.CRT_ERR_WORKSPACE
    assert call({_lib.TUNE_TRI_M: 16, _lib.TUNE_TRI_T: 4, _lib.TUNE_TRI_STORE_WAVES: 2, _lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_REG_STAGED,
                 _lib.TUNE_FLAT_FLUSH: _lib.FLAT_FLUSH_OFF}) == _lib.CRT_ERR_WORKSPACE
    for bad in ({_lib.TUNE_CLOSED_STORE_WAVES: 99}, {_lib.TUNE_CLOSED_PIPE_T: -1}, {_lib.TUNE_TRI_M: 10}, {_lib.TUNE_TRI_T: 5},
                {_lib.TUNE_TRI_FAMILY: 8}, {_lib.TUNE_TRI_STORE_WAVES: 13}, {_lib.TUNE_MIN_TILE_NB: 5000}, {_lib.TUNE_FLAT_FLUSH: 4},
                {_lib.TUNE_TILE_LDS: 1 << 20}, {_lib.TUNE_PACK: 3}, {7: 1}, {14: 7}, {_lib.TUNE_TILE_FLAGS: 256}):  # (7, 14: reserved)
        assert call(bad) == _lib.CRT_ERR_BAD_ARG, bad


def test_tune_names_match_header():
    """The _lib names of the crt_options.tune keys and values are the header's enumerators without the CRT_ prefix, with the same values."""
    from crt1d_amd import _lib

    text = open(os.path.join(ROOT, "include", "crt1d_hip.h")).read()
    assert int(re.search(r"#define CRT_NTUNE (\d+)", text).group(1)) == _lib.NTUNE
    prefixes = ("TUNE_", "TILE_FLAG_", "PACK_", "TRI_FAMILY_", "FLAT_FLUSH_")
    header = {}
    for enum in ("crt_tune_key", "crt_tune_tile_flag", "crt_tune_pack", "crt_tune_tri_family", "crt_tune_flat_flush"):
        body = re.sub(r"/\*.*?\*/", "", re.search(r"enum %s \{(.*?)\};" % enum, text, flags=re.S).group(1), flags=re.S)
        for name, value in re.findall(r"\bCRT_(\w+) = (\d+)", body):
            assert name.startswith(prefixes), name
            header[name] = int(value)
    assert len(header) == 14 + 5 + 2 + 8 + 3
    assert {k: v for k, v in vars(_lib).items() if k.startswith(prefixes)} == header
    assert sorted(header[k] for k in header if k.startswith("TUNE_")) == sorted(set(range(_lib.NTUNE)) - {7, 14})  # 7, 14: reserved


def test_set_tune_rejects_unknown_keys():
    """_lib.set_tune writes every key (0 where none is given) and refuses a key that crt_options.tune does not have; values are left to
    the library (test_tune_values_are_validated_before_any_launch)."""
    from crt1d_amd import _lib

    o = _lib.CrtOptions(0.501, 0, 0)
    o.tune[_lib.TUNE_TRI_T] = 8
    _lib.set_tune(o, {_lib.TUNE_TRI_FAMILY: _lib.TRI_FAMILY_ZQPA_PIPE, 7: -3})
    assert list(o.tune) == [_lib.TRI_FAMILY_ZQPA_PIPE if k == _lib.TUNE_TRI_FAMILY else -3 if k == 7 else 0 for k in range(_lib.NTUNE)]
    for bad in (_lib.NTUNE, -1, "TUNE_TRI_M", 8.0, None):
        with pytest.raises(ValueError, match="unknown crt_options.tune key"):
            _lib.set_tune(o, {bad: 1})


# restype and argtypes of every binding, by ctypes type name (``c_size_t`` is ``c_ulong`` and ``c_int64`` ``c_long`` on LP64 Linux, the only
# platform ROCm has; ``LP_X`` = ``POINTER(X)``), recorded from the hand-written ``load()`` this table replaced.  ``None``: argtypes unset.
_SOLVE = "LP_CrtColumns LP_CrtBands LP_CrtOptions LP_CrtOutputs c_void_p c_ulong c_void_p"
_SIGNATURES = {
    "crt_hip_abi_version": ("c_int", None),
    "crt_hip_strerror": ("c_char_p", "c_int"),
    "crt_hip_workspace_bytes": ("c_ulong", "c_int c_int c_int"),
    "crt_hip_workspace_bytes_nb": ("c_ulong", "c_int c_int c_int c_int"),
    "crt_hip_quad_nodes": ("c_int", "c_double LP_c_double"),
    "crt_hip_solve_f64": ("c_int", "c_int " + _SOLVE),
    "crt_hip_2s_f64": ("c_int", _SOLVE),
    "crt_hip_4s_f64": ("c_int", _SOLVE),
    "crt_hip_n79_f64": ("c_int", _SOLVE),
    "crt_hip_zq_f64": ("c_int", _SOLVE),
    "crt_hip_bl_f64": ("c_int", _SOLVE),
    "crt_hip_g77_f64": ("c_int", _SOLVE),
    "crt_hip_bf_f64": ("c_int", _SOLVE),
    "crt_hip_zq_pa_f64": ("c_int", _SOLVE),
    "crt_hip_solve_f32": ("c_int", "c_int " + _SOLVE),
    "crt_hip_2s_f32": ("c_int", _SOLVE),
    "crt_hip_4s_f32": ("c_int", _SOLVE),
    "crt_hip_n79_f32": ("c_int", _SOLVE),
    "crt_hip_zq_f32": ("c_int", _SOLVE),
    "crt_hip_bl_f32": ("c_int", _SOLVE),
    "crt_hip_g77_f32": ("c_int", _SOLVE),
    "crt_hip_bf_f32": ("c_int", _SOLVE),
    "crt_hip_zq_pa_f32": ("c_int", _SOLVE),
    "crt_hip_absorb_bandsum_f64": ("c_int", "LP_CrtColumns LP_CrtBands c_void_p c_void_p c_void_p c_void_p c_int c_void_p c_void_p c_void_p c_void_p c_void_p"),
    "crt_hip_absorb_bandsum2_f64": ("c_int", "LP_CrtColumns LP_CrtBands c_void_p c_void_p c_void_p c_void_p c_int LP_CrtBandsumOut c_void_p"),
    "crt_hip_integrated_f64": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtOptions c_void_p c_int c_void_p c_void_p c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "crt_hip_integrated2_f64": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtOptions c_void_p c_int LP_CrtBandsumOut c_void_p c_ulong c_void_p"),
    "crt_hip_absorb_f64": ("c_int", "LP_CrtColumns LP_CrtBands c_void_p c_void_p c_void_p LP_c_void_p c_void_p c_void_p c_void_p"),
    "crt_hip_absorb_bandsum_f32": ("c_int", "LP_CrtColumns LP_CrtBands c_void_p c_void_p c_void_p c_void_p c_int c_void_p c_void_p c_void_p c_void_p c_void_p"),
    "crt_hip_absorb_bandsum2_f32": ("c_int", "LP_CrtColumns LP_CrtBands c_void_p c_void_p c_void_p c_void_p c_int LP_CrtBandsumOut c_void_p"),
    "crt_hip_integrated_f32": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtOptions c_void_p c_int c_void_p c_void_p c_void_p c_void_p c_void_p c_ulong c_void_p"),
    "crt_hip_integrated2_f32": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtOptions c_void_p c_int LP_CrtBandsumOut c_void_p c_ulong c_void_p"),
    "crt_hip_series_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int c_int"),
    "crt_hip_integrated_series_f64": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtSunSeries LP_CrtOptions c_void_p c_int LP_CrtBandsumOut c_void_p c_ulong c_void_p"),
    "crt_hip_levels_f64": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtOptions LP_c_int c_int LP_CrtOutputs c_void_p c_ulong c_void_p"),
    "crt_hip_levels_f32": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtOptions LP_c_int c_int LP_CrtOutputs c_void_p c_ulong c_void_p"),
    "crt_hip_levels_series_workspace_bytes": ("c_ulong", "c_int c_int c_int c_int"),
    "crt_hip_levels_series_f64": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtSunSeries LP_CrtOptions LP_c_int c_int LP_CrtOutputs c_void_p c_ulong c_void_p"),
    "crt_hip_levels_series_f32": ("c_int", "c_int LP_CrtColumns LP_CrtBands LP_CrtSunSeriesF32 LP_CrtOptions LP_c_int c_int LP_CrtOutputs c_void_p c_ulong c_void_p"),
    "crt_hip_absorb_f32": ("c_int", "LP_CrtColumns LP_CrtBands c_void_p c_void_p c_void_p LP_c_void_p c_void_p c_void_p c_void_p"),
    "crt_hip_bandsum_finish_f64": ("c_int", "LP_CrtColumns c_int LP_CrtBandsumOut c_void_p"),
    "crt_hip_band_reduce_f64": ("c_int", "c_void_p c_long c_int c_void_p c_int c_void_p c_void_p"),
    "crt_hip_tau_d_f64": ("c_int", "c_void_p c_void_p c_long c_int c_void_p c_void_p"),
    "crt_hip_smear_tuv_f64": ("c_int", "c_void_p c_long c_int c_void_p c_int c_void_p c_int c_void_p c_void_p"),
    "crt_hip_lai_beta_f64": ("c_int", "c_void_p c_void_p c_void_p c_int c_int c_void_p c_void_p c_void_p c_void_p"),
    "crt_hip_buffer_alloc_set": ("c_int", "c_int LP_c_ulong LP_c_void_p"),
    "crt_hip_buffer_alloc": ("c_int", "c_ulong LP_c_void_p"),
    "crt_hip_buffer_free": ("c_int", "c_void_p"),
    "crt_hip_buffer_trim": ("c_int", ""),
    "crt_hip_buffer_set_retain": ("c_int", "c_ulong"),
    "crt_hip_buffer_describe": ("c_int", "c_void_p c_char_p c_ulong"),
    "crt_hip_buffer_stats": ("c_int", "LP_c_long"),
    "crt_hip_last_kernel": ("c_char_p", ""),
    "crt_hip_probe_fill_f64": ("c_int", "c_void_p c_ulong c_double c_void_p"),
    "crt_hip_probe_copy_f64": ("c_int", "c_void_p c_void_p c_ulong c_void_p"),
    "crt_hip_probe_store_set_f64": ("c_int", "LP_c_void_p c_int c_long c_long c_int c_double c_void_p"),
    "crt_hip_probe_math_f64": ("c_int", "c_void_p c_ulong c_void_p c_void_p c_void_p c_void_p"),
}


def test_ctypes_signatures_are_pinned(lib):
    from crt1d_amd import _lib

    assert isinstance(_lib.EXPORTS, list) and len(_lib.EXPORTS) == 57 == len(set(_lib.EXPORTS)) == len(_SIGNATURES)
    assert sorted(_lib.EXPORTS) == sorted(_SIGNATURES) == _declared()  # the header, the binding table and this table name the same symbols
    for name, (restype, argtypes) in _SIGNATURES.items():
        f = getattr(lib, name)
        assert f.restype.__name__ == restype, name
        got = None if f.argtypes is None else [t.__name__ for t in f.argtypes]
        assert got == (None if argtypes is None else argtypes.split()), name
    # the pointer types are the binding's own struct classes, not look-alikes
    assert lib.crt_hip_levels_series_f32.argtypes[3] is ctypes.POINTER(_lib.CrtSunSeriesF32)
    assert lib.crt_hip_levels_series_f64.argtypes[3] is ctypes.POINTER(_lib.CrtSunSeries)
    assert lib.crt_hip_integrated2_f64.argtypes[6] is ctypes.POINTER(_lib.CrtBandsumOut)
