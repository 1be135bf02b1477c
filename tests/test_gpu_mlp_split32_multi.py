"""Stochastic MLP dynamics with 16 < nx <= 32 states and rollout_samples M = 2..4 on the matrix cores
(csrc/rollout_mlp_split32_multi.hip: the two-output-tile kernel's arithmetic and LDS-resident layer 1, one wave per rollout copy, two
process-noise blocks per lane group and sample tile, the copies' step costs exchanged through LDS, visited states stored by the kernel).
`command()` against the fp64 oracle fed the consumed action normals and the exported process normals, under the project's rule
(err <= max(1e-5 scale, 2 x the reference's own fp32 error), tests/margins.py) -- and the launch counter says which kernel ran."""
import os

import pytest
import torch

import gpu_util
import margins
import test_gpu_fullsize_parity as F
from test_gpu_mlp_split32 import _well_conditioned_lambda
from pytorch_mppi_amd import _build, _native as N, _resources as R

VAR = dict(rollout_var_cost=0.3, rollout_var_discount=0.9)
SMPPI = dict(w=0.7, dt=0.1, amax=1.2)


def _launches():
    return int(N.lib().mppi_stat_mlp_split32_multi_launches())


def _parity(cfg, M, both=None, rng="torch", noisy=True, smppi=False, dtype=None, served=True, sigma=None):
    """one command with M rollouts per action sequence against the oracle on the same action and process draws; returns
    (controller, fp64 oracle results, fp32 oracle results).  noisy=False: a deterministic model, judged against the oracle's
    single-rollout command (zero variance, the mean of M equal costs).  served: the new kernel takes the command (the launch counter
    moves, no callback loop) | the callback loop does (the counter stands still)"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc, dynamics as dyn
    model, mk, sigma0, kw, x0, U0 = F._setup(cfg)
    sigma = sigma0 if sigma is None else sigma
    nx, nu, K, T = cfg["nx"], cfg["nu"], cfg["K"], cfg["T"]
    sd = torch.linspace(0.02, 0.08, nx)
    if noisy:
        model.with_process_noise(sd)
    kw = dict(kw, **(both or {}))
    amax = torch.full((nu,), SMPPI["amax"])
    csigma = sigma if dtype is None else sigma.to(dtype)             # the controller takes its dtype from noise_sigma

    def make(lam):
        if not smppi:
            return F._controller(cfg, model, csigma, dict(kw, rollout_samples=M, **VAR), U0, lam, rng)
        return pm.SMPPI(model.dynamics, model.running_cost, nx, sigma, num_samples=K, horizon=T, device="cuda", lambda_=lam, rng=rng,
                        seed=4321, U_init=U0.clone(), action_max=amax, w_action_seq_cost=SMPPI["w"], delta_t=SMPPI["dt"],
                        rollout_samples=M, **VAR)
    probe = make(1.0)
    probe.command(x0.cuda())
    lam = _well_conditioned_lambda(probe.cost_total)
    ctrl = make(lam)
    assert ctrl._needs_generic() == (not served)
    A0, Ud0 = (ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone()) if smppi else (None, None)
    torch.manual_seed(31)
    n0 = _launches()
    act = ctrl.command(x0.cuda())
    assert (_launches() - n0 >= 1) == served, "which path took the command"
    z = F._consumed_normals(ctrl)
    w = gpu_util.device_process_normals(ctrl, int(ctrl._last.call)) if noisy else None
    refs = []
    for dt in (torch.float64, torch.float32):
        f, q = mk(dt)
        okw = {k: (v.to(dt) if torch.is_tensor(v) else v) for k, v in kw.items()}
        if noisy:
            p = orc.Problem(dynamics=dyn.with_injected_process_noise(f, w.to(dt), sd.to(dt)), running_cost=lambda s_, a_, t_: q(s_, a_),
                            nx=nx, noise_sigma=sigma.to(dt), K=K, T=T, lambda_=lam, step_dependent_dynamics=True, rollout_samples=M,
                            **VAR, **okw)
        else:
            p = orc.Problem(dynamics=f, running_cost=q, nx=nx, noise_sigma=sigma.to(dt), K=K, T=T, lambda_=lam, **okw)
        if smppi:
            refs.append(orc.smppi_command(p, Ud0.to(dt), A0.to(dt), x0.to(dt), z.to(dt), -amax.to(dt), amax.to(dt), SMPPI["w"],
                                          SMPPI["dt"], True))
        else:
            refs.append(orc.command(p, U0.to(dt), x0.to(dt), z.to(dt), True))
    name, got = f"mlp split32 multi M{M} {cfg} {sorted(kw)} {rng}", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega)
    if dtype == torch.float64:
        for k, v in got.items():
            margins.check(name, k, v.detach().cpu().numpy(), refs[0][k].numpy(), refs[1][k].numpy(), rtol=1e-9)
    else:
        F._check(name, got, *refs)
    return ctrl, refs[0], refs[1]


# every M on every shape; K = 40 (a ragged second half and an idle tile; M = 2: an idle wave pair) and 64 n_cu + 40 (the second trip of
# the persistent loop); T = 1 / 9 (a partial exchange chunk) / 17 (the first reuse of an LDS buffer half); (24, 6, 100): tile 1 with
# lane groups 2 and 3 without a noise block, no second control, hidden width padded to 128
CASES = [(32, 8, 64, 2, 40, 1), (32, 8, 64, 3, 40, 9), (32, 8, 64, 4, "big", 17), (32, 8, 64, 2, "big", 17),
         (32, 8, 256, 2, "big", 9), (32, 8, 256, 3, 40, 17), (32, 8, 256, 4, 40, 1), (32, 8, 256, 3, "big", 9),
         (24, 6, 100, 2, 40, 17), (24, 6, 100, 3, "big", 1), (24, 6, 100, 4, 40, 9), (24, 6, 100, 4, "big", 17)]


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,H,M,K,T", CASES)
def test_command_equals_oracle_on_the_one_wave_per_copy_two_tile_kernel(nx, nu, H, M, K, T):
    K = K if isinstance(K, int) else 64 * torch.cuda.get_device_properties(0).multi_processor_count + 40
    _parity(dict(kind="mlp", K=K, T=T, nx=nx, nu=nu, H=H), M)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,H,M", [(32, 8, 64, 3), (24, 6, 100, 2)])
def test_visited_states_are_the_kernels_own_stores(nx, nu, H, M):
    """there is no per-lane form to rerun: the lane that owns rows 16 o + 4g .. + 3 of copy m wrote them"""
    ctrl, r64, r32 = _parity(dict(kind="mlp", K=200, T=9, nx=nx, nu=nu, H=H), M)
    n0, got = _launches(), ctrl.states
    assert _launches() == n0 + 1 and got.shape == (M, 200, 9, nx)
    margins.check("mlp split32 multi", "states", got.cpu().numpy(), r64["states"].numpy(), r32["states"].numpy())


@pytest.mark.gpu
def test_bounds_and_null_action_row():
    ctrl, _, _ = _parity(dict(kind="mlp", K=200, T=5, nx=24, nu=6, H=64), 2,
                         both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


@pytest.mark.gpu
def test_smppi_lifted_controls():
    _parity(dict(kind="mlp", K=200, T=9, nx=32, nu=8, H=64), 3, rng="philox", smppi=True)


@pytest.mark.gpu
def test_deterministic_copies_cost_what_one_rollout_costs():
    _parity(dict(kind="mlp", K=200, T=9, nx=32, nu=8, H=64), 3, noisy=False)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["MPPI_MLP_MULTI=0", "full Sigma", "fp64"])
def test_what_the_kernel_does_not_serve_keeps_the_callback_loop(what, monkeypatch):
    """(a deterministic model: the callables of the callback loop draw their own process noise, which no oracle can be fed).  A full
    Sigma: the kernel's action cost is one product per element, so the off-diagonal terms of Sigma^-1 need the callback loop"""
    if what == "MPPI_MLP_MULTI=0":
        monkeypatch.setenv("MPPI_MLP_MULTI", "0")
    sigma = torch.eye(6) + 0.3 * torch.diag(torch.ones(5), 1) + 0.3 * torch.diag(torch.ones(5), -1) if what == "full Sigma" else None
    _parity(dict(kind="mlp", K=200, T=5, nx=24, nu=6, H=64), 3, noisy=False, dtype=torch.float64 if what == "fp64" else None,
            served=False, sigma=sigma)


@pytest.mark.parametrize("nx,nu", [(32, 8), (24, 6)])
def test_every_instantiation_runs_out_of_registers_and_lds_alone(nx, nu):
    """H = 256: the M = 1 kernel's 128 + 48 pinned AGPRs beside two draw states and 16 waiting normals -- no scratch, no spilled VGPRs"""
    if not os.path.exists(_build.LIB):
        pytest.skip("library not built")
    hit = {k: v for k, v in R.find(R.kernels(_build.LIB), "rollout_mlp_split32_multi_kernel<").items() if f", {nx}, {nu}>" in k}
    assert len(hit) >= 1, (nx, nu)
    for name, r in hit.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
