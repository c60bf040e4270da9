"""GPU: the band partition with ``level_profiles=True`` on the HIP kernels.  In a world of one nothing is reduced and the result is the
kernels' own (bitwise the unsharded ``BandSumPlan`` / ``IntegratedPlan`` with ``profiles=True``); with two rank processes sharing the one
GPU (gloo, as tests/test_gpu_dist2.py) the level sums travel in the all-reduce and ``crt_hip_bandsum_finish_f64`` re-forms F, I_d and aI."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SCHEMES = ("2s", "4s", "n79", "zq", "bl", "g77", "bf", "zq_pa")
TEN = ("aI", "aI_sl", "aI_sh", "totals", "aI_dr", "I_dr", "I_df_d", "I_df_u", "F", "I_d")
SPEC = ("I_dr0", "I_df0", "leaf_r", "leaf_t", "soil_r")
NCOL, NB, NZ = 50, 300, 40


def _problem(f32=False, device="cuda"):
    import torch

    from crt1d_amd import batched, spectra, synth

    d = synth.make_columns(NCOL, NB, NZ, seed=3, uniform_dlai=False)
    cols = batched.Columns.from_host(d, device)
    bands = batched.Bands.from_host({k: (d[k].astype(np.float32) if (f32 and k in SPEC) else d[k]) for k in d}, device)
    return cols, bands, torch.as_tensor(spectra.band_weights(d["wle"])).to(device)


@pytest.mark.parametrize("keep_profiles", [True, False])
@pytest.mark.parametrize("scheme", SCHEMES)
def test_world_one_is_the_unsharded_result(scheme, keep_profiles):
    import torch

    from crt1d_amd import batched
    from crt1d_amd.dist import BandShardPlan

    cols, bands, bw = _problem()
    if keep_profiles:
        sol = batched.Plan(scheme, cols, bands, placement="auto")()
        ref = batched.BandSumPlan(cols, bands, sol, bw, profiles=True)()
    else:
        ref = batched.IntegratedPlan(scheme, cols, bands, bw, profiles=True)()
    ref = {k: v.clone() for k, v in ref.items()}
    one = BandShardPlan(scheme, cols, bands, bw, keep_profiles=keep_profiles, level_profiles=True)().wait()
    one = {k: one[k].clone() for k in TEN}
    three = BandShardPlan(scheme, cols, bands, bw, keep_profiles=keep_profiles, level_profiles=True, column_tiles=3)().wait()
    torch.cuda.synchronize()
    scale = float(ref["totals"].abs().max())
    for k in TEN:
        assert torch.equal(one[k], ref[k]), k
        assert three[k].shape == ref[k].shape, k
        assert float((three[k] - ref[k]).abs().max()) <= 1e-13 * scale, k
    # the reference's absorption dict follows from the band-partition result unchanged
    ab = batched.absorption_from_bandsums(one)
    assert torch.equal(ab["aI_df_sh"], ref["aI_sh"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, scheme, keep_profiles, f32, q):
    import torch
    import torch.distributed as dist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from crt1d_amd.dist import BandShardPlan

        cols, bands, bw = _problem(f32, "cuda:0")
        plan = BandShardPlan(scheme, cols, bands, bw, column_tiles=3, share_profiles=True, keep_profiles=keep_profiles, level_profiles=True)
        plan().wait()
        r = plan().wait()  # second step on the same buffers
        torch.cuda.synchronize()
        q.put((rank, plan.band_range, plan.message_bytes, {k: r[k].cpu().numpy() for k in TEN + ("reflectance",)}))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("scheme,keep_profiles,f32", [("zq", True, False), ("n79", False, False), ("zq_pa", True, True)])
def test_two_ranks_reduce_the_level_profiles(scheme, keep_profiles, f32):
    import torch.multiprocessing as mp

    from crt1d_amd.dist import solve_sharded

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, scheme, keep_profiles, f32, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    cols, bands, bw = _problem(f32)
    ref = solve_sharded(scheme, cols, bands, bw, partition="column", keep_profiles=keep_profiles, level_profiles=True)  # world of one
    assert [g[1] for g in got] == [(0, 150), (150, 300)]
    ng = bw.shape[0]
    scale = float(ref["totals"].abs().max())
    for rank, _, nbytes, res in got:
        assert nbytes == 8 * NCOL * (3 * (NZ - 1) * ng + 4 * ng + 3 * NZ * ng)
        for k in TEN:
            assert res[k].shape == tuple(ref[k].shape), k
            assert np.max(np.abs(res[k] - ref[k].cpu().numpy())) <= 1e-12 * scale, (rank, k)
        np.testing.assert_allclose(res["reflectance"], ref["reflectance"].cpu().numpy(), rtol=1e-12)
    for k in got[0][3]:
        np.testing.assert_array_equal(got[0][3][k], got[1][3][k])  # both ranks hold the same reduced result
