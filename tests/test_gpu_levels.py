"""GPU: the level-subset solve (crt_hip_levels_f64 / _f32, batched.LevelsPlan): every row bitwise the row of the full profile solve, for
all eight schemes, uniform and ragged columns, any band count; f32 rows; key subsets; spectral totals against the fused integrated
path; flags, graph capture, kernel selection and the shape limit."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
KEYS = ("I_dr", "I_df_d", "I_df_u", "F")
SHAPES = [(19, 300, 60), (7, 107, 61), (5, 12, 60), (3, 13, 9), (2, 1, 5), (2, 1025, 20), (1, 2151, 60), (3, 300, 100), (3, 300, 150),
          (4, 40, 3)]
FAMILY = {"n79": "k_tri_lev<", "zq": "k_tri_lev<", "zq_pa": "k_zqpa_lev<"}


def _level_sets(nz):
    sets = [(nz - 1,), (0, nz - 1), tuple(range(0, nz, 7))]
    around = sorted({j for m in range(1, nz // 8 + 1) for j in (8 * m - 1, 8 * m, 8 * m + 1) if j < nz})[:64]
    if around:
        sets.append(tuple(around))
    if nz <= 64:
        sets.append(tuple(range(nz)))
    return sets


def _setup(shape, uniform, seed=11, dtype=None):
    import torch

    from crt1d_amd import batched, synth

    d = synth.make_columns(*shape, seed=seed, uniform_dlai=uniform)
    cols = batched.Columns.from_host(d)
    bands = batched.Bands.from_host(d)
    if dtype is not None:
        bands = batched.Bands(*[None if getattr(bands, k) is None else getattr(bands, k).to(dtype)
                                for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])
    torch.cuda.synchronize()
    return d, cols, bands


def _upcast(bands):
    import torch

    from crt1d_amd import batched

    return batched.Bands(*[None if getattr(bands, k) is None else getattr(bands, k).to(torch.float64)
                           for k in ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")])


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_rows_are_bitwise_the_profile_rows(scheme, uniform):
    import torch

    from crt1d_amd import batched

    for shape in SHAPES:
        _, cols, bands = _setup(shape, uniform)
        nz = shape[2]
        full = batched.solve(scheme, cols, bands)
        for lev in _level_sets(nz):
            plan = batched.LevelsPlan(scheme, cols, bands, lev)
            got = plan()
            torch.cuda.synchronize()
            assert plan.last_kernel().startswith(FAMILY.get(scheme, "k_lev<")), plan.last_kernel()
            idx = torch.tensor(lev, device=cols.device)
            for k in KEYS:
                assert got[k].shape == (shape[0], len(lev), shape[1])
                assert torch.equal(got[k], full[k].index_select(1, idx)), (scheme, shape, lev, k)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_f32_rows_are_the_f64_rows_rounded_once(scheme, uniform):
    """float32 spectra in, float32 rows out: the f64 rows of the same (upcast) inputs rounded once -- also for zq_pa at band counts its
    f32 profile path does not serve (nb < 16, nb > 832)."""
    import torch

    from crt1d_amd import batched

    for shape in [(19, 300, 60), (5, 12, 60), (2, 1025, 20), (3, 13, 9)]:
        _, cols, b32 = _setup(shape, uniform, seed=5, dtype=torch.float32)
        b64 = _upcast(b32)
        nz = shape[2]
        for lev in [(0, nz - 1), tuple(range(0, nz, 7))]:
            p32 = batched.LevelsPlan(scheme, cols, b32, lev)
            r32 = p32()
            assert " f32" in p32.last_kernel(), p32.last_kernel()
            r64 = batched.solve_levels(scheme, cols, b64, lev)
            torch.cuda.synchronize()
            for k in KEYS:
                assert r32[k].dtype == torch.float32
                assert torch.equal(r32[k], r64[k].to(torch.float32)), (scheme, shape, lev, k)


def _raw_call(scheme, cols, bands, levels, ptrs, workspace, flags=0):
    import torch

    from crt1d_amd import _lib

    lib = _lib.load()
    c, b = cols.c_struct(), bands.c_struct(cols.ncol)
    o = _lib.CrtOptions(0.501, 0, flags)
    out = _lib.CrtOutputs(*ptrs, None, None, None)
    lev = (ctypes.c_int32 * len(levels))(*levels)
    fn = lib.crt_hip_levels_f32 if bands.dtype == torch.float32 else lib.crt_hip_levels_f64
    return fn(_lib.SCHEME_IDS[scheme], ctypes.byref(c), ctypes.byref(b), ctypes.byref(o), lev, len(levels), ctypes.byref(out),
              workspace.data_ptr(), workspace.numel(), torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("scheme", SCHEMES)
def test_key_subsets_write_only_what_is_asked(scheme):
    import torch

    from crt1d_amd import batched

    shape = (5, 107, 30)
    _, cols, bands = _setup(shape, True, seed=2)
    lev = (0, 9, 29)
    full = batched.solve(scheme, cols, bands)
    got = batched.solve_levels(scheme, cols, bands, lev, keys=("I_df_u",))
    torch.cuda.synchronize()
    assert set(got) == {"I_df_u"}
    assert torch.equal(got["I_df_u"], full["I_df_u"][:, list(lev), :])
    # raw ABI: one array given, between guard zones; the other three sentinel arrays are never handed over
    n, guard, sentinel = shape[0] * len(lev) * shape[1], 4096, -12345.5
    buf = torch.full((n + 2 * guard,), sentinel, dtype=torch.float64, device="cuda")
    others = [torch.full((n,), sentinel, dtype=torch.float64, device="cuda") for _ in range(3)]
    ws = torch.empty(batched.workspace_bytes(scheme, shape[0], shape[2], shape[1]), dtype=torch.uint8, device="cuda")
    st = _raw_call(scheme, cols, bands, lev, [None, None, buf[guard:].data_ptr(), None], ws)
    torch.cuda.synchronize()
    assert st == 0
    assert torch.equal(buf[guard:guard + n].view(shape[0], len(lev), shape[1]), full["I_df_u"][:, list(lev), :])
    assert bool((buf[:guard] == sentinel).all()) and bool((buf[guard + n:] == sentinel).all())
    for t in others:
        assert bool((t == sentinel).all())
    # F alone, then I_dr and F: each matches, the arrays not given are not written
    for keys in (("F",), ("I_dr", "F")):
        arrs = {k: torch.full((shape[0], len(lev), shape[1]), sentinel, dtype=torch.float64, device="cuda") for k in KEYS}
        st = _raw_call(scheme, cols, bands, lev, [arrs[k].data_ptr() if k in keys else None for k in KEYS], ws)
        torch.cuda.synchronize()
        assert st == 0
        for k in KEYS:
            if k in keys:
                assert torch.equal(arrs[k], full[k][:, list(lev), :]), (keys, k)
            else:
                assert bool((arrs[k] == sentinel).all()), (keys, k)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "ragged"])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_spectral_totals_contract_to_the_integrated_totals(scheme, uniform):
    import torch

    from crt1d_amd import batched, spectra

    d, cols, bands = _setup((19, 300, 60), uniform, seed=8)
    w = torch.as_tensor(spectra.band_weights(d["wle"]), dtype=torch.float64, device="cuda")
    t = batched.spectral_totals(scheme, cols, bands)
    ref = batched.IntegratedPlan(scheme, cols, bands, w)()["totals"]
    torch.cuda.synchronize()
    assert t.shape == (19, 300, 4) and t.dtype == torch.float64
    got = torch.einsum("cbq,gb->cgq", t, w)
    scale = ref[..., :1].abs().clamp_min(1e-300)  # each group's incoming flux
    assert float(((got - ref).abs() / scale).max()) < 1e-13
    # the per-band terms themselves are the profile rows
    full = batched.solve(scheme, cols, bands)
    torch.cuda.synchronize()
    assert torch.equal(t[..., 0], full["I_dr"][:, -1] + full["I_df_d"][:, -1])
    assert torch.equal(t[..., 1], full["I_df_u"][:, -1])
    assert torch.equal(t[..., 2], full["I_dr"][:, 0] + full["I_df_d"][:, 0])
    assert torch.equal(t[..., 3], full["I_df_u"][:, 0])


@pytest.mark.parametrize("scheme", SCHEMES)
def test_skip_precompute_and_graph_capture(scheme):
    import torch

    from crt1d_amd import _lib, batched

    shape = (40, 300, 60)
    d, cols, bands = _setup(shape, True, seed=4)
    lev = (0, 17, 59)
    plan = batched.LevelsPlan(scheme, cols, bands, lev)
    plan()
    torch.cuda.synchronize()
    # same geometry, new spectra: the column records in the workspace still hold
    d2, _, bands2 = _setup(shape, True, seed=40)
    plan2 = batched.LevelsPlan(scheme, cols, bands2, lev, workspace=plan.workspace)
    got = {k: v.clone() for k, v in plan2(flags=_lib.FLAG_SKIP_PRECOMPUTE).items()}
    fresh = batched.solve_levels(scheme, cols, bands2, lev)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(got[k], fresh[k]), k
    # PRECOMPUTE_ONLY writes no output
    for v in plan2.out.values():
        v.fill_(7.0)
    plan2(flags=_lib.FLAG_PRECOMPUTE_ONLY)
    torch.cuda.synchronize()
    for v in plan2.out.values():
        assert bool((v == 7.0).all())
    # graph capture after the first call: one stream, K0 + the level kernel, replayed bitwise
    plan()
    torch.cuda.synchronize()
    ref = {k: v.clone() for k, v in plan.out.items()}
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        plan()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan()
    for v in plan.out.values():
        v.zero_()
    g.replay()
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(plan.out[k], ref[k]), k


@pytest.mark.parametrize("scheme", SCHEMES)
def test_deep_columns_and_wide_spectra(scheme):
    """nz = 400 at more than 1024 bands: every scheme serves it (several band slices per column)."""
    import torch

    from crt1d_amd import batched

    _, cols, bands = _setup((2, 1100, 400), True, seed=9)
    lev = (0, 7, 8, 199, 398, 399)
    full = batched.solve(scheme, cols, bands)
    got = batched.solve_levels(scheme, cols, bands, lev)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(got[k], full[k][:, list(lev), :]), k


def test_unsupported_shape_writes_nothing():
    """n79 at nz = 3000: its checkpoints do not fit in LDS even for a 64-band slice -> CRT_ERR_UNSUPPORTED, outputs untouched.  The
    records are taken as given (SKIP_PRECOMPUTE): the launcher refuses before any launch."""
    import torch

    from crt1d_amd import _lib, batched

    shape = (2, 16, 3000)
    _, cols, bands = _setup(shape, True, seed=1)
    lev = (0, 2999)
    sentinel = 3.25
    arrs = [torch.full((shape[0], len(lev), shape[1]), sentinel, dtype=torch.float64, device="cuda") for _ in KEYS]
    ws = torch.zeros(batched.workspace_bytes("n79", shape[0], shape[2], shape[1]), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = _raw_call("n79", cols, bands, lev, [a.data_ptr() for a in arrs], ws, flags=_lib.FLAG_SKIP_PRECOMPUTE)
    torch.cuda.synchronize()
    assert st == _lib.CRT_ERR_UNSUPPORTED
    for a in arrs:
        assert bool((a == sentinel).all())
    with pytest.raises(RuntimeError, match="not supported"):
        batched.LevelsPlan("n79", cols, bands, lev, workspace=ws)(flags=_lib.FLAG_SKIP_PRECOMPUTE)
