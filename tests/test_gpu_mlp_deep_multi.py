"""The two-hidden-layer residual MLP (models.MLPResidual2) with process noise and rollout_samples M = 2..4 on the matrix cores
(csrc/rollout_mlp_deep_multi.hip: the deep kernel's arithmetic and LDS-resident hidden layer, one wave per rollout copy, process noise
drawn in the owning lane, the copies' step costs exchanged through LDS, visited states stored by the kernel).  `command()` against the
fp64 oracle fed the consumed action normals and the exported process normals, under the project's rule (err <= max(1e-5 scale, 2 x the
reference's own fp32 error), tests/margins.py) -- and the launch counter says which kernel ran."""
import os

import pytest
import torch

import gpu_util
import margins
import test_gpu_fullsize_parity as F
from test_gpu_mlp_deep import _setup
from test_gpu_mlp_split32 import _well_conditioned_lambda
from pytorch_mppi_amd import _build, _native as N, _resources as R

VAR = dict(rollout_var_cost=0.3, rollout_var_discount=0.9)
SMPPI = dict(w=0.7, dt=0.1, amax=1.2)


def _launches():
    return int(N.lib().mppi_stat_mlp_deep_multi_launches())


def _parity(cfg, M, both=None, rng="torch", noisy=True, smppi=False, kmppi=0, dtype=None, served=True, sigma=None):
    """one command with M rollouts per action sequence against the oracle on the same action and process draws; returns
    (controller, fp64 oracle results).  noisy=False: a deterministic model, judged against the oracle's single-rollout command (zero
    variance, the mean of M equal costs).  kmppi=S: KMPPI with S support points from U = theta = 0 (its two-launch form: raw actions
    in memory).  served: the new kernel takes the command (the launch counter moves, no callback loop) | the callback loop does
    (the counter stands still)"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc, dynamics as dyn
    model, mk, sigma0, kw, x0, U0 = _setup(cfg)
    sigma = sigma0 if sigma is None else sigma
    nx, nu, K, T = cfg["nx"], cfg["nu"], cfg["K"], cfg["T"]
    U0 = torch.zeros_like(U0) if kmppi else U0
    sd = torch.linspace(0.02, 0.08, nx)
    if noisy:
        model.with_process_noise(sd)
    kw = dict(kw, **(both or {}))
    amax = torch.full((nu,), SMPPI["amax"])
    csigma = sigma if dtype is None else sigma.to(dtype)             # the controller takes its dtype from noise_sigma

    def make(lam):
        if kmppi:
            return pm.KMPPI(model.dynamics, model.running_cost, nx, csigma, num_samples=K, horizon=T, device="cuda", lambda_=lam, rng=rng,
                            seed=4321, U_init=U0.clone(), num_support_pts=kmppi, kernel=pm.RBFKernel(sigma=1.5), rollout_samples=M,
                            **VAR, **kw)
        if not smppi:
            return F._controller(cfg, model, csigma, dict(kw, rollout_samples=M, **VAR), U0, lam, rng)
        return pm.SMPPI(model.dynamics, model.running_cost, nx, sigma, num_samples=K, horizon=T, device="cuda", lambda_=lam, rng=rng,
                        seed=4321, U_init=U0.clone(), action_max=amax, w_action_seq_cost=SMPPI["w"], delta_t=SMPPI["dt"],
                        rollout_samples=M, **VAR)
    probe = make(1.0)
    probe.command(x0.cuda())
    ctrl = make(_well_conditioned_lambda(probe.cost_total))
    lam = float(ctrl.lambda_)
    assert ctrl._needs_generic() == (not served)
    A0, Ud0 = (ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone()) if smppi else (None, None)
    torch.manual_seed(31)
    n0 = _launches()
    act = ctrl.command(x0.cuda())
    assert (_launches() - n0 >= 1) == served, "which path took the command"
    call = int(ctrl._call if kmppi else ctrl._last.call)
    z = gpu_util.device_philox_normals(ctrl, call, Tn=kmppi) if kmppi else F._consumed_normals(ctrl)
    w = gpu_util.device_process_normals(ctrl, call) if noisy else None
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
        if kmppi:
            W, W_shift, _, _ = orc.kmppi_matrices(T, kmppi, dt, kernel=lambda t_, tk: orc.rbf_kernel(t_, tk, sigma=1.5))
            refs.append(orc.kmppi_command(p, torch.zeros(kmppi, nu, dtype=dt), U0.to(dt), x0.to(dt), z.to(dt), W, W_shift, True))
        elif smppi:
            refs.append(orc.smppi_command(p, Ud0.to(dt), A0.to(dt), x0.to(dt), z.to(dt), -amax.to(dt), amax.to(dt), SMPPI["w"],
                                          SMPPI["dt"], True))
        else:
            refs.append(orc.command(p, U0.to(dt), x0.to(dt), z.to(dt), True))
    got = dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega, **(dict(theta=ctrl.theta) if kmppi else {}))
    for k, got in got.items():
        margins.check(f"mlp deep multi M{M} {cfg} {sorted(kw)} {rng}", k, got.detach().cpu().numpy(), refs[0][k].numpy(),
                      refs[1][k].numpy(), rtol=1e-9 if dtype == torch.float64 else 1e-5)
    return ctrl, refs[0], refs[1]


# every M; K = 40 (a ragged second half and an idle tile; M = 2: an idle wave pair) and 64 n_cu + 40 (the second trip of the persistent
# loop); T = 1 / 9 (a partial exchange chunk) / 17 (the first reuse of an LDS buffer half); (12, 6, (48, 40)): unequal widths padded to
# 64, lane group 3 without a noise block, nu > 4; (2, 1, (32, 32)): three idle lane groups
CASES = [(16, 4, (128, 128), 2, 40, 1), (16, 4, (128, 128), 3, 40, 9), (16, 4, (128, 128), 4, "big", 17), (16, 4, (128, 128), 2, "big", 17),
         (16, 4, (128, 128), 3, "big", 9), (12, 6, (48, 40), 2, 40, 17), (12, 6, (48, 40), 3, "big", 1), (12, 6, (48, 40), 4, 40, 9),
         (12, 6, (48, 40), 4, "big", 17), (2, 1, (32, 32), 2, "big", 9), (2, 1, (32, 32), 3, 40, 17), (2, 1, (32, 32), 4, 40, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,H,M,K,T", CASES)
def test_command_equals_oracle_on_the_one_wave_per_copy_deep_kernel(nx, nu, H, M, K, T):
    K = K if isinstance(K, int) else 64 * torch.cuda.get_device_properties(0).multi_processor_count + 40
    _parity(dict(kind="mlp2", K=K, T=T, nx=nx, nu=nu, H=H), M)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,H,M", [(16, 4, (64, 64), 3), (12, 6, (48, 40), 2), (2, 1, (32, 32), 4)])
def test_visited_states_are_the_kernels_own_stores(nx, nu, H, M):
    """there is no per-lane form to rerun: the lane that owns rows 4g..4g+3 of copy m wrote them"""
    ctrl, r64, r32 = _parity(dict(kind="mlp2", K=200, T=9, nx=nx, nu=nu, H=H), M)
    n0, got = _launches(), ctrl.states
    assert _launches() == n0 + 1 and got.shape == (M, 200, 9, nx)
    margins.check("mlp deep multi", "states", got.cpu().numpy(), r64["states"].numpy(), r32["states"].numpy())


@pytest.mark.gpu
def test_bounds_and_null_action_row():
    ctrl, _, _ = _parity(dict(kind="mlp2", K=200, T=5, nx=12, nu=6, H=(48, 40)), 2,
                         both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


@pytest.mark.gpu
def test_smppi_lifted_controls():
    _parity(dict(kind="mlp2", K=200, T=9, nx=16, nu=4, H=(64, 64)), 3, rng="philox", smppi=True)


@pytest.mark.gpu
@pytest.mark.parametrize("nx,nu,H,M", [(16, 4, (64, 64), 3), (12, 6, (48, 40), 2)])
def test_kmppi_raw_actions(nx, nu, H, M):
    """KMPPI's two-launch form: the kernel's raw-action instantiations, under a diagonal Sigma with unequal entries and a bound"""
    _parity(dict(kind="mlp2", K=200, T=9, nx=nx, nu=nu, H=H), M, rng="philox", kmppi=5, sigma=torch.diag(torch.linspace(0.5, 1.2, nu)),
            both=dict(u_max=torch.full((nu,), 1.1)))


@pytest.mark.gpu
def test_deterministic_copies_cost_what_one_rollout_costs():
    _parity(dict(kind="mlp2", K=200, T=9, nx=16, nu=4, H=(64, 64)), 3, noisy=False)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["fp64", "weights beyond fp16", "MPPI_MLP_MULTI=0", "full Sigma", "full Sigma, KMPPI"])
def test_what_the_kernel_does_not_serve_keeps_the_callback_loop(what, monkeypatch):
    """(a deterministic model: the callables of the callback loop draw their own process noise, which no oracle can be fed).  A full
    Sigma: the kernel's action cost is one product per element, so the off-diagonal terms of Sigma^-1 need the callback loop"""
    import pytorch_mppi_amd as pm
    cfg = dict(kind="mlp2", K=200, T=5, nx=12, nu=6, H=(48, 40))
    if what == "weights beyond fp16":
        # one hidden->hidden weight whose folded value -2 (2 log2 e) W2 = 7e4 is no fp16 (it multiplies a saturated tanh: finite)
        m = pm.models.MLPResidual2.random(12, 6, 48, 40, seed=2)
        m.W2[3, 5] = 1.25e4
        assert m.flags() == N.MODEL_FLAG_EXACT_FP32
        cfg["_model"] = m
    if what == "MPPI_MLP_MULTI=0":
        monkeypatch.setenv("MPPI_MLP_MULTI", "0")
    full = what.startswith("full Sigma")
    sigma = torch.eye(6) + 0.3 * torch.diag(torch.ones(5), 1) + 0.3 * torch.diag(torch.ones(5), -1) if full else None
    _parity(cfg, 3, noisy=False, dtype=torch.float64 if what == "fp64" else None, served=False, sigma=sigma,
            rng="philox" if what.endswith("KMPPI") else "torch", kmppi=5 if what.endswith("KMPPI") else 0)


def test_every_instantiation_runs_out_of_registers_and_lds_alone():
    """H = 128: the M = 1 kernel's pinned AGPRs beside the draw's counter, keys and 2 x 4 normals -- no scratch, no spilled VGPRs"""
    if not os.path.exists(_build.LIB):
        pytest.skip("library not built")
    hit = R.find(R.kernels(_build.LIB), "rollout_mlp_deep_multi_kernel<")
    assert len(hit) == 18, sorted(hit)                       # (16,4) (12,6) (2,1) x H 32 / 64 / 128 x (rows | raw actions)
    for name, r in hit.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
