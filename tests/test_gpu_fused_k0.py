"""GPU: the 2s k_pipe that forms its column records itself (K0 prologue, one launch per call) against k_colpre.

A default 2s call that picks k_pipe runs no k_colpre: each workgroup forms its column's record and writes it to the workspace as well.
The record must be k_colpre's to the last bit -- every other kernel family, SKIP_PRECOMPUTE calls and PRECOMPUTE_ONLY read what k_colpre
writes -- and so must every output.  ``CRT_TUNE_K0_SEPARATE = 1`` keeps k_colpre in front of the same k_pipe (the A/B setting)."""
import numpy as np
import pytest

from crt1d_amd import _lib

pytestmark = pytest.mark.gpu

_IO = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")
_K0_OFF = {_lib.TUNE_K0_SEPARATE: 1}


def _columns(ncol, nb, nz, seed, uniform, g_kind=None, mla=None):
    from crt1d_amd import _lib, synth

    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=uniform)
    rng = np.random.default_rng(seed + 1)
    if mla is not None:
        d["mla"] = np.full(ncol, float(mla))
    if g_kind is not None:
        d["g_kind"] = np.full(ncol, g_kind, dtype=np.int32)
        if g_kind == 3:  # Campbell ellipsoidal: x < 1, x == 1 (its spherical special case) and x > 1
            d["g_param"] = rng.choice([0.3, 1.0, 2.5], ncol)
        elif g_kind == 5:  # Ross-Goudriaan chi_l, clipped to [-0.4, 0.6] on device
            d["g_param"] = rng.uniform(-0.6, 0.8, ncol)
        elif g_kind == 6:  # a caller-sampled G at the library's nodes
            amp = rng.uniform(0.05, 0.3, ncol)

            def G(p):
                return 0.5 + amp[:, None] * np.cos(2 * np.atleast_2d(p))

            d["g_table"] = np.ascontiguousarray(G(_lib.quad_nodes(0.501)[None, :]))
            d["g_at_psi"] = np.ascontiguousarray(G(d["psi"][:, None])[:, 0])
    return d


def _bits(t):
    import torch

    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _raw(t):
    import torch

    return t.contiguous().view(torch.uint8)


def _same(a, b):
    import torch

    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _plans(d, dtype="f64", **kw):
    """the default (fused) plan and its k_colpre twin on the same columns and bands"""
    from crt1d_amd import batched

    if dtype == "f32":
        d = {k: (v.astype(np.float32) if k in _IO else v) for k, v in d.items()}
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    return batched.Plan("2s", cols, bands, placement="none", **kw), batched.Plan("2s", cols, bands, placement="none", tune=_K0_OFF, **kw)


def _nan(plan):
    for v in plan.out.values():
        v.fill_(float("nan"))
    plan.workspace.zero_()


@pytest.mark.parametrize("g_kind", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("uniform", [True, False])
def test_record_equals_k_colpre(g_kind, uniform):
    """After a fused call the workspace holds k_colpre's records byte for byte (every G kind, uniform and ragged dLAI, nz 2..400, several
    mean leaf angles), and the outputs equal those of the two-kernel call."""
    import torch

    from crt1d_amd import _lib

    for nz, nb, mla in ((2, 64, 20.0), (3, 300, 57.3), (60, 300, None), (61, 107, 80.0), (130, 64, 45.0), (400, 300, None)):
        d = _columns(37, nb, nz, seed=100 + nz + g_kind, uniform=uniform, g_kind=g_kind, mla=mla)
        fused, ref = _plans(d)
        for p in (fused, ref):
            _nan(p)
        fused()
        kf = fused.last_kernel()  # (the name of this thread's most recent launch)
        ref()
        kr = ref.last_kernel()
        torch.cuda.synchronize()
        assert "k0=fused" in kf, (nz, nb, kf)
        assert "k0=fused" not in kr, kr
        assert torch.equal(_raw(fused.workspace), _raw(ref.workspace)), (g_kind, uniform, nz, nb)
        # ... and what k_colpre writes by itself (PRECOMPUTE_ONLY) into a cleared workspace
        ws_fused = fused.workspace.clone()
        fused.workspace.zero_()
        fused(flags=_lib.FLAG_PRECOMPUTE_ONLY)
        torch.cuda.synchronize()
        assert torch.equal(_raw(fused.workspace), _raw(ws_fused)), (g_kind, uniform, nz, nb)
        for k in fused.out:
            assert bool(torch.isfinite(fused.out[k]).all()), (k, nz)
            assert _same(fused.out[k], ref.out[k]), (g_kind, uniform, nz, nb, k)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [300, 107, 64, 16])
def test_fused_outputs_equal_k0_off(dtype, nb):
    """Fused outputs are the bits of the two-kernel call: f64 and f32 storage, aligned and generic-flush k_pipe, the packed kernel (16 bands:
    k_colpre runs in front of it), uniform and ragged columns."""
    import torch

    for ncol, nz, uniform in ((203, 60, True), (150, 37, False)):
        d = _columns(ncol, nb, nz, seed=nb + nz, uniform=uniform)
        fused, ref = _plans(d, dtype)
        for p in (fused, ref):
            _nan(p)
        fused()
        kf = fused.last_kernel()
        ref()
        kr = ref.last_kernel()
        torch.cuda.synchronize()
        if nb >= 64:
            assert "k0=fused" in kf, kf
            assert kf.startswith(f"k_pipe<2s,{dtype}> "), kf
        assert kr == kf.replace(" k0=fused", ""), (kr, kf)
        assert torch.equal(_raw(fused.workspace), _raw(ref.workspace))
        for k in fused.out:
            assert _same(fused.out[k], ref.out[k]), (dtype, nb, ncol, k)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nb", [300, 107])
def test_fused_outputs_at_offsets(dtype, nb):
    """Output arrays at element offsets inside sentinel guard bands: the fused call writes the bits of the aligned two-kernel call and
    leaves the guards alone."""
    import torch

    from crt1d_amd import batched

    ncol, nz = 71, 23
    d = _columns(ncol, nb, nz, seed=5, uniform=True)
    if dtype == "f32":
        d = {k: (v.astype(np.float32) if k in _IO else v) for k, v in d.items()}
    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    ref = batched.Plan("2s", cols, bands, placement="none", tune=_K0_OFF)
    ref()
    tdt = torch.float64 if dtype == "f64" else torch.float32
    n = ncol * nz * nb
    for off in (1, 3, 8):
        bufs, out = {}, {}
        for k in ref.out:
            bufs[k] = torch.full((n + off + 64,), 1234.5, dtype=tdt, device="cuda")
            out[k] = bufs[k][off:off + n].view(ncol, nz, nb)
        p = batched.Plan("2s", cols, bands, out=out)
        p()
        torch.cuda.synchronize()
        assert "k0=fused" in p.last_kernel(), p.last_kernel()
        for k in ref.out:
            assert _same(out[k], ref.out[k]), (off, k)
            assert bool((bufs[k][:off] == 1234.5).all()) and bool((bufs[k][off + n:] == 1234.5).all()), (off, k)


def test_skip_precompute_after_fused_call():
    """A SKIP_PRECOMPUTE call on the workspace a fused call filled gives the same bits (it reads the records the prologue wrote)."""
    import torch

    from crt1d_amd import _lib, batched

    for nz, uniform in ((60, True), (45, False)):
        d = _columns(301, 300, nz, seed=nz, uniform=uniform)
        fused, ref = _plans(d)
        fused()
        torch.cuda.synchronize()
        first = {k: v.clone() for k, v in fused.out.items()}
        _nan(fused)
        fused()  # fills the workspace again, then the outputs are cleared and formed from it alone
        for v in fused.out.values():
            v.fill_(float("nan"))
        fused(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        assert "k0=fused" not in fused.last_kernel(), fused.last_kernel()
        for k in first:
            assert _same(fused.out[k], first[k]), (nz, k)
        # a plan sharing the workspace (the bench's roofline pass does this) sees the same records
        other = batched.Plan("2s", fused.cols, fused.bands, placement="none", workspace=fused.workspace)
        other(flags=_lib.FLAG_SKIP_PRECOMPUTE)
        torch.cuda.synchronize()
        for k in first:
            assert _same(other.out[k], first[k]), (nz, k)


def test_fused_plan_replays_from_a_hip_graph():
    """A fused plan captured into a hipGraph replays to the same bits, also after the columns' LAI changes in place."""
    import torch

    d = _columns(257, 300, 60, seed=9, uniform=True)
    fused, ref = _plans(d)
    fused()  # first call outside the capture: uploads the quadrature tables
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        fused(s)
    assert "k0=fused" in fused.last_kernel(), fused.last_kernel()
    for scale in (1.0, 0.7):
        fused.cols.lai.mul_(scale)
        _nan(fused)
        torch.cuda.synchronize()
        g.replay()
        ref()
        torch.cuda.synchronize()
        assert torch.equal(_raw(fused.workspace), _raw(ref.workspace)), scale
        for k in ref.out:
            assert _same(fused.out[k], ref.out[k]), (scale, k)


def test_tune_key_15_is_validated():
    """CRT_TUNE_K0_SEPARATE (key 15) is 0 or 1; other values are CRT_ERR_BAD_ARG (ValueError from the plan)."""
    d = _columns(8, 64, 10, seed=1, uniform=True)
    from crt1d_amd import batched

    cols, bands = batched.Columns.from_host(d), batched.Bands.from_host(d)
    with pytest.raises(ValueError):
        batched.Plan("2s", cols, bands, placement="none", tune={_lib.TUNE_K0_SEPARATE: 2})()
