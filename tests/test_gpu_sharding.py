"""GPU: the multi-GPU path emulated on one device.  gpurun boxes have ONE GPU (RCCL refuses two
ranks on a device), so the shards run back to back on cuda:0 and the all-gather is a torch.stack;
everything else -- contiguous shard plan, per-shard K1/K3/K4 against the shard's own beta, record
layout, rank-order combine kernel K5 -- is the product code.  The collective itself is
smoke-tested with nccl(=RCCL) at world_size 1."""
import os

import numpy as np
import pytest
import torch

import pytorch_mppi_amd as pm
from pytorch_mppi_amd.dist import ShardPlan, combine_records_host

pytestmark = pytest.mark.gpu


def _mk(K, T, nx, nu, rng, shard, dtype=torch.float32, **kw):
    m = pm.models.Integrator(nx, nu)
    g = torch.Generator().manual_seed(3)
    U0 = torch.randn(T, nu, generator=g, dtype=dtype) * 0.05
    return pm.MPPI(m.dynamics, m.running_cost, nx, torch.eye(nu, dtype=dtype) * 0.5, num_samples=K, horizon=T,
                   device="cuda", lambda_=40.0, U_init=U0, rng=rng, seed=99, shard=shard, **kw)


def _run_sharded(K, T, nx, nu, world, rng, z=None, dtype=torch.float32, **kw):
    ctrls = [_mk(K, T, nx, nu, rng, (r, world), dtype, **kw) for r in range(world)]
    x0 = torch.linspace(-1, 1, nx, dtype=dtype).cuda()
    ps = []
    for c in ctrls:
        if z is not None:
            c.inject_noise(z)                     # global draw; each shard takes its own rows
        ps.append(c._begin(x0, True))
    records = torch.stack([p._keep["record"] for p in ps])      # = all_gather_into_tensor, rank order
    for c, p in zip(ctrls, ps):
        c._combine(p, records)
    acts = [c._end(p) for c, p in zip(ctrls, ps)]
    return ctrls, acts, records, x0


@pytest.mark.parametrize("K,world,dtype", [(4096, 2, torch.float32), (1000, 3, torch.float32), (1536, 8, torch.float64)])
def test_sharded_equals_unsharded_with_injected_noise(K, world, dtype):
    T, nx, nu = 12, 6, 4
    z = torch.randn(K, T, nu, generator=torch.Generator().manual_seed(1), dtype=dtype)
    ctrls, acts, records, x0 = _run_sharded(K, T, nx, nu, world, "torch", z, dtype, sample_null_action=True)
    full = _mk(K, T, nx, nu, "torch", None, dtype, sample_null_action=True)
    full.inject_noise(z)
    a_full = full.command(x0)
    tol = 1e-5 if dtype == torch.float32 else 1e-11
    for c, a in zip(ctrls, acts):
        assert torch.equal(c.U, ctrls[0].U), "ranks must hold bit-identical U"
        assert torch.allclose(a, a_full, rtol=tol, atol=tol)
        assert torch.allclose(c.U, full.U, rtol=tol, atol=tol)
        lo, hi = c._shard.bounds(c._shard.rank)
        assert (c.k_offset, c.K_local) == (lo, hi - lo)
        assert torch.allclose(c.cost_total, full.cost_total[lo:hi], rtol=tol, atol=tol * float(full.cost_total.abs().max()))
        assert torch.allclose(c.omega, full.omega[lo:hi], rtol=10 * tol, atol=tol)
    assert abs(sum(float(c.omega.sum()) for c in ctrls) - 1.0) < 1e-5
    # K5 against its host restatement
    Ush = torch.roll(full._last._keep["U"], -1, 0)
    Ush[-1] = 0
    U_host, beta, eta = combine_records_host(records.double().cpu(), Ush.double().cpu(), 40.0)
    assert torch.allclose(ctrls[0].U.double().cpu(), U_host, rtol=tol, atol=tol)
    assert float(beta) == float(full.cost_total.min())


def test_philox_stream_is_independent_of_the_number_of_shards():
    K, T, nx, nu = 3000, 10, 6, 4
    c2, a2, _, x0 = _run_sharded(K, T, nx, nu, 2, "philox")
    c5, a5, _, _ = _run_sharded(K, T, nx, nu, 5, "philox")
    full = _mk(K, T, nx, nu, "philox", None)
    af = full.command(x0)
    for a in a2 + a5:
        assert torch.allclose(a, af, rtol=1e-5, atol=1e-6)
    # the shards regenerate exactly the rows of the global stream
    lo, hi = c5[3]._shard.bounds(3)
    assert torch.equal(c5[3].noise, full.noise[lo:hi])
    assert torch.equal(c5[3].cost_total, full.cost_total[lo:hi])


def test_sampler_rows_live_on_shard_zero_only():
    """global row bookkeeping (mppi.py:387-400) under sharding"""
    K, T, nx, nu, world = 512, 8, 6, 4, 4
    sa = torch.randn(3, T, nu, generator=torch.Generator().manual_seed(5)) * 0.3

    class S(pm.SpecificActionSampler):
        def sample_trajectories(self, state, info):
            return sa.clone()

    z = torch.randn(K, T, nu, generator=torch.Generator().manual_seed(2))
    ctrls, acts, _, x0 = _run_sharded(K, T, nx, nu, world, "torch", z, sample_null_action=True,
                                      specific_action_sampler=S())
    full = _mk(K, T, nx, nu, "torch", None, sample_null_action=True, specific_action_sampler=S())
    full.inject_noise(z)
    af = full.command(x0)
    assert torch.allclose(acts[0], af, rtol=1e-5, atol=1e-6)
    assert torch.equal(ctrls[0].perturbed_action[0], torch.zeros(T, nu, device="cuda"))
    assert torch.allclose(ctrls[0].perturbed_action[1:4].cpu(), sa, atol=0)
    assert torch.equal(ctrls[1].perturbed_action, full.perturbed_action[128:256])
    assert (ctrls[2].specific_action_sampler.start_idx, ctrls[2].specific_action_sampler.end_idx) == (1, 4)


def test_record_all_gather_over_rccl_world_size_one():
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        rec = torch.arange(2 + 64 * 12, device="cuda", dtype=torch.float32)
        out = ShardPlan(65536, 0, 1).all_gather(rec)
        torch.cuda.synchronize()
        assert out.shape == (1, rec.numel()) and torch.equal(out[0], rec)
    finally:
        dist.destroy_process_group()


def test_sharded_philox_generates_next_rows_behind_the_collective():
    """Sharded + rng="philox" (generator launch): the rows of command n+1 are generated while the
    record all-gather of command n is in flight (RCCL at world_size 1, collective forced) and picked
    up by the next command; the controller is the unsharded one, and a seed change drops the buffer."""
    import torch.distributed as dist
    from pytorch_mppi_amd import MPPI, models
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29535")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        m = models.Integrator(8, 4)
        mk = lambda shard: MPPI(m.dynamics, m.running_cost, 8, 0.5 * torch.eye(4), num_samples=3000, horizon=20, device="cuda",
                                lambda_=4.0, u_max=torch.ones(4), U_init=torch.zeros(20, 4), rng="philox", seed=5, shard=shard)
        a, b = mk(None), mk((0, 1))
        a.philox_fill = b.philox_fill = True
        b._force_collective = True
        b.overlap_collective = True
        x = torch.linspace(-1, 1, 8, device="cuda")
        for i in range(6):
            ua, ub = a.command(x), b.command(x)
            # a: single-launch command (partial sums per workgroup, rescaled); b: K3 against the shard minimum, K5
            torch.testing.assert_close(ua, ub, rtol=3e-5, atol=5e-6)
            torch.testing.assert_close(a.cost_total, b.cost_total, rtol=1e-5, atol=1e-5)
            b.U = a.U.clone()                    # two closed loops with different rounding drift apart: keep them in step
        assert b._pf_hits == 5 and a._pf_hits == 0
        b.seed = a.seed = 6                      # stale buffer: key mismatch -> regenerated
        torch.testing.assert_close(a.command(x), b.command(x), rtol=3e-5, atol=5e-6)
        assert b._pf_hits == 5
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["mppi-fused", "mppi-generic", "kmppi"])
def test_engine_owned_rccl_exchange_world_size_one(kind):
    """The exchange inside the C-ABI (csrc/dist.hip): mppi_dist_unique_id / mppi_dist_init create an RCCL
    communicator bound at run time, mppi_command_sharded = K1 + K3 + K4 + ncclAllGather + K5 on the
    caller's stream in ONE call (fused path), mppi_exchange_combine for the callback path and KMPPI.
    One GPU here: world_size 1, the collective has no peer -- what is checked is the whole code path
    and that the result is the unsharded command.  No torch.distributed involved at all."""
    from pytorch_mppi_amd import MPPI, KMPPI, models
    from pytorch_mppi_amd.dist import NativeComm
    m = models.Integrator(8, 4)
    f, q = (m.dynamics, m.running_cost) if kind != "mppi-generic" else ((lambda s, a: m.dynamics(s, a)), (lambda s, a: m.running_cost(s, a)))
    cls, extra = (KMPPI, dict(num_support_pts=6)) if kind == "kmppi" else (MPPI, {})
    mk = lambda shard: cls(f, q, 8, 0.5 * torch.eye(4), num_samples=3000, horizon=20, device="cuda", lambda_=4.0,
                           u_max=torch.ones(4), U_init=torch.zeros(20, 4), rng="philox", seed=5, shard=shard, **extra)
    a, b = mk(None), mk((0, 1))
    b._force_collective = True
    x = torch.linspace(-1, 1, 8, device="cuda")
    for i in range(4):
        ua, ub = a.command(x), b.command(x)
        # a may run as the single-launch command (other, equally valid summation order): 3e-5 / 5e-6
        torch.testing.assert_close(ua, ub, rtol=3e-5, atol=5e-6)
        torch.testing.assert_close(a.U, b.U, rtol=3e-5, atol=5e-6)
        torch.testing.assert_close(a.cost_total, b.cost_total, rtol=1e-5, atol=1e-5)
        torch.testing.assert_close(a.omega, b.omega, rtol=1e-4, atol=1e-8)
        b.U = a.U.clone()                        # keep the two closed loops in step (their rounding differs)
        if kind == "kmppi":
            b.theta = a.theta.clone()
    assert isinstance(b._shard._native, NativeComm), "the sharded command must have gone through the engine's own RCCL communicator"
    if kind == "mppi-fused":
        assert b._last._combined and b._last._keep["records"].shape == (1, 2 + 20 * 4)
        assert torch.equal(b._last._keep["records"][0], b._last._keep["record"])     # the all-gather of one rank is its record
    b._shard._native.close()


@pytest.mark.parametrize("native", [True, False])
def test_env_sharded_mppi_batched_needs_no_collective(native):
    """MPPI_Batched(shard=(rank, world)): the environment axis split over the ranks (3 shards of 7
    environments, emulated back to back).  Every environment is an independent controller and the one
    shared noise draw is the same Philox stream on every rank, so each shard reproduces exactly its
    slice of the unsharded controller -- without any exchange."""
    N_env, K, T, world = 7, 512, 9, 3
    lin = pm.models.LinearGoal(torch.tensor([[1.0, 0.0], [0.0, -1.0]]), torch.tensor([2.0, 2.0]))
    f, q = (lin.dynamics, lin.running_cost) if native else ((lambda s, a: lin.dynamics(s, a)), (lambda s, a: lin.running_cost(s, a)))
    g = torch.Generator().manual_seed(4)
    U0 = torch.randn(N_env, T, 2, generator=g) * 0.2
    states = torch.randn(N_env, 2, generator=g) * 2
    kw = dict(num_samples=K, horizon=T, device="cuda", lambda_=3.0, u_max=torch.tensor([1.5, 1.0]), rng="philox", seed=21)
    full = pm.MPPI_Batched(f, q, 2, torch.eye(2), N_env, **kw)
    full.U = U0.cuda().clone()
    shards = [pm.MPPI_Batched(f, q, 2, torch.eye(2), N_env, shard=(r, world), **kw) for r in range(world)]
    lo = 0
    for c in shards:
        assert c.N_global == N_env and c.env_offset == lo
        c.U = U0[lo:lo + c.N].cuda().clone()
        lo += c.N
    assert lo == N_env
    for step in range(3):
        a_full = full.command(states)
        for c in shards:
            a = c.command(states)                          # the GLOBAL state array: the shard takes its rows
            sl = slice(c.env_offset, c.env_offset + c.N)
            assert torch.equal(a, a_full[sl]) and torch.equal(c.U, full.U[sl])
            assert torch.equal(c.cost_total, full.cost_total[sl]) and torch.equal(c.omega, full.omega[sl])
    with pytest.raises(ValueError):
        pm.MPPI_Batched(f, q, 2, torch.eye(2), N_env, shard=(0, 2), num_samples=K, horizon=T, device="cuda", rng="torch")


def _torchrun(args, env_extra=None, timeout=300):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.update(env_extra or {})
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547"] + args
    return subprocess.run(cmd, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)


def test_two_processes_sharded_command_matches_unsharded():
    """the real N>1 path end to end: 2 PROCESSES (sharing cuda:0, gloo), record all-gather, K5"""
    r = _torchrun([os.path.join("tests", "dist_worker.py")])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count("OK") == 2


def test_bench_two_ranks_prints_one_valid_json_line():
    """bench.py under torch.distributed.run with 2 ranks (gloo test rig): weak scaling bookkeeping"""
    import json
    r = _torchrun(["bench.py", "--gpus", "2", "--steps", "5", "--warmup", "2", "--workload", "c2", "--full"],
                  env_extra={"MPPI_BENCH_BACKEND": "gloo"})
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["K_global"] == 2 * d["config"]["K_per_gpu"]
    assert d["config"]["ranks_hold_identical_U"] is True and d["value"] > 0 and "cpu_baseline" not in d



def test_bench_gpus_2_starts_its_own_ranks():
    """`python bench.py --gpus 2 --process-model spawn` with no launcher around it: bench.py starts its own two ranks;
    on this 1-GPU box they share cuda:0 and exchange through gloo (labelled a test rig in config.backend)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MPPI_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "4", "--warmup", "2", "--workload", "c2", "--process-model", "spawn", "--full"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["world_size"] == 2 and d["config"]["K_global"] == 2 * d["config"]["K_per_gpu"]
    assert d["config"]["ranks_hold_identical_U"] is True and d["value"] > 0
    ex = d["config"]["collective_per_command"]
    assert ex["us_per_exchange"] > 0 and ex["calls"] > 0
    if torch.cuda.device_count() < 2:
        assert "TEST RIG" in d["config"]["backend"]
    # what the first multi-GPU run has to put on record (VERDICT r03 missing #1): weak scaling against this box's own
    # single-GPU time of the same workload, the collective alone, and BASELINE configs[4] (C5: the MLP at K = 65536 x N)
    for key, kper in (("weak_scaling", d["config"]["K_per_gpu"]), ("c5", 65536)):
        w = d[key]
        assert w["n_gpus"] == 2 and w["K_per_gpu"] == kper and w["K_global"] == 2 * kper
        assert w["sharded_ms_per_step"] > 0 and w["single_gpu_ms_per_step"] > 0 and w["collective_us"] > 0
        assert abs(w["weak_scaling_speedup"] - 2 * w["single_gpu_ms_per_step"] / w["sharded_ms_per_step"]) < 1e-9
    assert "MLP" in d["c5"]["workload"] and abs(d["weak_scaling"]["sharded_ms_per_step"] - d["ms_per_step"]) < 1e-9


def test_sharded_kmppi_with_the_interpolation_inside_k1_rolls_out_its_own_global_rows():
    """KMPPI under `shard=` on the fused-interpolation path with in-kernel Philox: every shard must draw the rows of
    ITS global samples (counter = global k) and see the null-action row on shard 0 only -- its cost_total is the slice
    of the unsharded controller's.  (The exchange itself is stubbed: the costs are final before it.)"""
    nx, nu, K, T, S = 6, 4, 3000, 20, 10
    m = pm.models.Integrator(nx, nu)
    x0 = torch.linspace(-1, 1, nx).cuda()
    kw = dict(num_samples=K, horizon=T, device="cuda", lambda_=5.0, num_support_pts=S, rng="philox", seed=21,
              sample_null_action=True, U_init=torch.zeros(T, nu), u_max=torch.ones(nu))
    full = pm.KMPPI(m.dynamics, m.running_cost, nx, torch.eye(nu) * 0.6, **kw)
    lib = pm._native.lib()
    n0 = lib.mppi_stat_kmppi_fused_rollouts()
    full.command(x0)
    world = 3
    for r in range(world):
        c = pm.KMPPI(m.dynamics, m.running_cost, nx, torch.eye(nu) * 0.6, shard=(r, world), **kw)
        c._shard.native_comm = lambda device: None
        c._shard.all_gather = lambda rec: torch.stack([rec] * world)          # stub: not what is under test
        c.command(x0)
        lo, hi = c._shard.bounds(r)
        ref = full.cost_total[lo:hi]
        assert float((c.cost_total - ref).abs().max()) <= 1e-6 * max(1.0, float(ref.abs().max())), r
    assert lib.mppi_stat_kmppi_fused_rollouts() == n0 + 1 + world


def test_bench_gpus_2_in_one_process_on_a_device_group():
    """`python bench.py --gpus 2` with no launcher around it: ONE process, MPPI(..., devices=[0, 1]) -- on this 1-GPU box
    devices=[0, 0], records staged through device copies (labelled)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MPPI_BENCH_BACKEND")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "4", "--warmup", "2", "--process-model", "devices", "--full"],
                       cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["K_global"] == 2 * d["config"]["K_per_gpu"] and d["value"] > 0
    assert d["config"]["devices_hold_identical_U"] is True and "ONE process" in d["config"]["process_model"]
    assert d["host_issue_us_per_device"] > 0 and "worker thread" in d["config"]["process_model"]
    if torch.cuda.device_count() < 2:
        assert d["config"]["devices"] == [0, 0] and "not a measurement" in d["config"]["process_model"]
    assert d["weak_scaling"]["single_gpu_ms_per_step"] > 0
