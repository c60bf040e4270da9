"""CPU, gloo: the band partition's all-reduce carries the band-integrated LEVEL profiles too (``level_profiles=True``).  Oracle-backed
compute functions and a torch ``finish_fn`` are injected (the HIP kernels need a GPU; the packing / reduction / re-forming logic of
crt1d_amd.dist is the same).  Every rank must end up with all ten integrated outputs of the unsharded problem."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_gloo import HostBands, HostCols, _oracle_fns

TEN = ("aI", "aI_sl", "aI_sh", "totals", "aI_dr", "I_dr", "I_df_d", "I_df_u", "F", "I_d")
PROBLEMS = {"odd": (7, 9, 12, 21, True), "even": (5, 40, 10, 33, False)}  # ncol, nb, nz, seed, uniform dlai


def _problem(name):
    from crt1d_amd import spectra, synth

    ncol, nb, nz, seed, unif = PROBLEMS[name]
    d = synth.make_columns(ncol, nb, nz, seed=seed, uniform_dlai=unif)
    return d, torch.from_numpy(spectra.band_weights(d["wle"]))


def _fns():
    """The oracle solve, an oracle epilogue that also returns the level sums (band sums of the reference's own per-band F and
    I_d = I_dr + I_df_d, not the identities), the composed integrated function, and a torch finish."""
    solve_fn, epi4 = _oracle_fns()

    def epilogue_fn(cols, bands, sol, band_w, profiles=False):
        from oracle import crt_oracle as O

        res = dict(epi4(cols, bands, sol, band_w))
        if profiles:
            w = band_w.numpy().T
            oc = O.Columns(cols.d["psi"], cols.d["lai"], mla=cols.d["mla"], g_kind=cols.d["g_kind"], g_param=cols.d["g_param"])
            prof = {k: sol[k].numpy() for k in ("I_dr", "I_df_d", "I_df_u", "F")}
            ab = O.calc_absorption(oc, prof, leaf_r=bands.d["leaf_r"], leaf_t=bands.d["leaf_t"])
            res["aI_dr"] = torch.from_numpy(ab["aI_dr"] @ w)
            for k in ("I_dr", "I_df_d", "I_df_u", "F"):
                res[k] = torch.from_numpy(prof[k] @ w)
            res["I_d"] = torch.from_numpy((prof["I_dr"] + prof["I_df_d"]) @ w)
        return res

    def integrated_fn(scheme, cols, bands, band_w, profiles=False, **opts):
        return epilogue_fn(cols, bands, solve_fn(scheme, cols, bands, **opts), band_w, profiles=profiles)

    def finish_fn(cols, v):
        invmu = (1.0 / torch.cos(torch.from_numpy(np.asarray(cols.d["psi"], dtype=np.float64))))[:, None, None]
        torch.add(v["aI_sl"], v["aI_sh"], out=v["aI"])
        v["F"].copy_(v["I_dr"] * invmu + 2 * (v["I_df_u"] + v["I_df_d"]))
        v["I_d"].copy_(v["I_dr"] + v["I_df_d"])

    return solve_fn, epilogue_fn, integrated_fn, finish_fn


def _msg_doubles(ncol, nz, ng, profiles):
    return ncol * (3 * (nz - 1) * ng + 4 * ng + 3 * nz * ng) if profiles else ncol * (2 * (nz - 1) * ng + 4 * ng)


def _worker(rank, world, port, scheme, prob, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from crt1d_amd.dist import BandShardPlan, gather_columns, grid_mean, solve_sharded

        d, bw = _problem(prob)
        solve_fn, epi, integ, fin = _fns()
        cols, bands = HostCols(d), HostBands(d)
        out = {"band": {}}
        for keep in (True, False):
            for tiles in (1, 3):
                kw = dict(solve_fn=solve_fn, epilogue_fn=epi) if keep else dict(integrated_fn=integ)
                r = solve_sharded(scheme, cols, bands, bw, partition="band", keep_profiles=keep, column_tiles=tiles, level_profiles=True,
                                  finish_fn=fin, **kw)
                out["band"][keep, tiles] = {k: r[k].numpy().copy() for k in TEN + ("reflectance",)}
        rc = solve_sharded(scheme, cols, bands, bw, partition="column", solve_fn=solve_fn, epilogue_fn=epi, level_profiles=True)
        out["column"] = {k: gather_columns(rc[k], cols.ncol).numpy().copy() for k in TEN}
        out["grid_mean"] = {k: v.numpy().copy() for k, v in grid_mean(rc, cols.ncol).items()}
        # message sizes: with level profiles, and unchanged without
        plan = BandShardPlan(scheme, cols, bands, bw, column_tiles=3, solve_fn=solve_fn, epilogue_fn=epi, level_profiles=True, finish_fn=fin)
        plan0 = BandShardPlan(scheme, cols, bands, bw, column_tiles=3, solve_fn=solve_fn, epilogue_fn=epi)
        r0 = plan0().wait()
        out["bytes"] = (plan.message_bytes, plan0.message_bytes, plan.ng, sorted(k for k in r0 if k in TEN))
        q.put((rank, out))
    except Exception as e:  # report at once instead of leaving the parent waiting on the queue
        q.put((rank, {"error": repr(e)}))
        raise
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, scheme, prob):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, scheme, prob, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in range(world)], key=lambda t: t[0])
    for _, out in got:
        assert "error" not in out, out.get("error")
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return [g[1] for g in got]


def _close(got, ref, what):
    scale = max(float(np.abs(ref).max()), 1e-300)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.max(np.abs(got - ref)) <= 1e-12 * scale, (what, float(np.max(np.abs(got - ref))) / scale)


@pytest.mark.parametrize("world,scheme,prob", [(2, "zq", "odd"), (2, "2s", "odd"), (2, "n79", "odd"), (3, "zq", "even"), (5, "zq", "even"),
                                               (8, "zq", "even")])
def test_band_partition_reduces_the_level_profiles(world, scheme, prob):
    from crt1d_amd.dist import solve_sharded

    got = _run(world, scheme, prob)
    d, bw = _problem(prob)
    _, epi, _, _ = _fns()
    solve_fn = _oracle_fns()[0]
    ref = solve_sharded(scheme, HostCols(d), HostBands(d), bw, partition="column", solve_fn=solve_fn, epilogue_fn=epi, level_profiles=True)
    ncol, nb, nz = PROBLEMS[prob][:3]
    ng = bw.shape[0]
    for out in got:
        for (keep, tiles), res in out["band"].items():
            for k in TEN:
                _close(res[k], out["column"][k], (k, keep, tiles, "vs column partition"))
                _close(res[k], ref[k].numpy(), (k, keep, tiles, "vs unsharded"))
            np.testing.assert_allclose(res["reflectance"], ref["reflectance"].numpy(), rtol=1e-12)
        # the column means of the gathered profiles, in grid_mean's one all-reduce
        for k in TEN:
            np.testing.assert_allclose(out["grid_mean"][k], out["column"][k].mean(axis=0), rtol=1e-12, atol=1e-14 * np.abs(out["column"][k]).max())
        with_prof, without, plan_ng, keys0 = out["bytes"]
        assert plan_ng == ng
        # F, I_d and aI do not travel; without level profiles the message (and the result keys) are what they were
        assert with_prof == 8 * _msg_doubles(ncol, nz, ng, True)
        assert without == 8 * _msg_doubles(ncol, nz, ng, False)
        assert keys0 == sorted(("aI", "aI_sl", "aI_sh", "totals"))
    for out in got[1:]:  # every rank holds the same bits
        for key in got[0]["band"]:
            for k in TEN:
                np.testing.assert_array_equal(out["band"][key][k], got[0]["band"][key][k])


def test_message_size_of_config4():
    """The sizes quoted for BASELINE configs[3] (1e5 columns x 100 levels x 3 groups, 4 tiles): 606 doubles per column today, 1803 with
    the level profiles (2403 if F and I_d travelled too)."""
    assert _msg_doubles(1, 100, 3, False) == 606 and _msg_doubles(1, 100, 3, True) == 1803
    assert 8 * _msg_doubles(25000, 100, 3, True) == 360_600_000 and 8 * _msg_doubles(25000, 100, 3, False) == 121_200_000


def test_world_one_level_profiles_without_reduce():
    """A world of one: nothing is reduced, the kernels' (here: the oracle's) own F / I_d / aI stand and finish_fn is never called."""
    from crt1d_amd.dist import BandShardPlan

    d, bw = _problem("odd")
    solve_fn, epi, integ, _ = _fns()

    def no_finish(cols, v):
        raise AssertionError("finish_fn called without a reduce")

    cols, bands = HostCols(d), HostBands(d)
    ref = epi(cols, bands, solve_fn("zq", cols, bands), bw, profiles=True)
    for keep in (True, False):
        kw = dict(solve_fn=solve_fn, epilogue_fn=epi) if keep else dict(integrated_fn=integ)
        plan = BandShardPlan("zq", cols, bands, bw, column_tiles=2, keep_profiles=keep, level_profiles=True, finish_fn=no_finish, **kw)
        r = plan().wait()
        for k in TEN:
            np.testing.assert_allclose(r[k].numpy(), ref[k].numpy(), rtol=1e-14, atol=0)
        assert plan.message_bytes == 8 * _msg_doubles(cols.ncol, cols.nz, bw.shape[0], True)
