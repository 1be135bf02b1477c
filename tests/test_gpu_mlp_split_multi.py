"""Stochastic MLP dynamics with rollout_samples M = 2..4 on the matrix cores (csrc/rollout_mlp_split_multi.hip: one wave per rollout
copy, process noise drawn in the owning lane, the copies' step costs exchanged through LDS).  `command()` against the fp64 oracle fed
the consumed action normals and the exported process normals, under the project's rule (err <= max(1e-5 scale, 2 x the reference's own
fp32 error), tests/margins.py) -- and the launch counter says which kernel ran."""
import pytest
import torch

import gpu_util
import margins
import test_gpu_fullsize_parity as F
from test_gpu_mlp_split32 import _well_conditioned_lambda
from pytorch_mppi_amd import _native as N

pytestmark = pytest.mark.gpu
VAR = dict(rollout_var_cost=0.3, rollout_var_discount=0.9)
SMPPI = dict(w=0.7, dt=0.1, amax=1.2)


def _parity(cfg, M, both=None, rng="torch", noisy=True, smppi=False, in_k1=False):
    """one command with M rollouts per action sequence against the oracle on the same action and process draws; returns
    (controller, launches of the new kernel by that command, (fp64, fp32) oracle results).  noisy=False: a deterministic model,
    judged against the oracle's single-rollout command (zero variance, the mean of M equal costs); in_k1: K1 generates its rows"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc, dynamics as dyn
    model, mk, sigma, kw, x0, U0 = F._setup(cfg)
    nx, nu, K, T = cfg["nx"], cfg["nu"], cfg["K"], cfg["T"]
    sd = torch.linspace(0.02, 0.08, nx)
    if noisy:
        model.with_process_noise(sd)
    kw = dict(kw, **(both or {}))
    amax = torch.full((nu,), SMPPI["amax"])

    def make(lam):
        if not smppi:
            c = F._controller(cfg, model, sigma, dict(kw, rollout_samples=M, **VAR), U0, lam, rng)
            c.philox_fill = False if in_k1 else None
            return c
        return pm.SMPPI(model.dynamics, model.running_cost, nx, sigma, num_samples=K, horizon=T, device="cuda", lambda_=lam, rng=rng,
                        seed=4321, U_init=U0.clone(), action_max=amax, w_action_seq_cost=SMPPI["w"], delta_t=SMPPI["dt"],
                        rollout_samples=M, **VAR)
    probe = make(1.0)
    probe.command(x0.cuda())
    lam = _well_conditioned_lambda(probe.cost_total)
    ctrl = make(lam)
    assert not ctrl._needs_generic()
    A0, Ud0 = (ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone()) if smppi else (None, None)
    torch.manual_seed(31)
    n0 = int(N.lib().mppi_stat_mlp_split_multi_launches())
    act = ctrl.command(x0.cuda())
    moved = int(N.lib().mppi_stat_mlp_split_multi_launches()) - n0
    z = F._consumed_normals(ctrl)
    w = gpu_util.device_process_normals(ctrl, int(ctrl._last.call))
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
    F._check(f"mlp split multi M{M} {cfg} {sorted(kw)} {rng}", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega), *refs)
    return ctrl, moved, refs


# every M, K = 40 (second half ragged, an idle tile; M = 2: an idle wave pair) and 64 n_cu + 40 (second trip of the persistent loop),
# T = 1 / 9 / 17 (a partial exchange chunk; the first reuse of an LDS buffer half), three shapes ((12, 6, 100): lane group 3 without
# a noise block, component-wise rows, padded hidden width)
CASES = [(16, 4, 64, 2, 40, 1), (16, 4, 64, 3, 40, 9), (16, 4, 64, 4, "big", 17), (16, 4, 64, 2, "big", 17),
         (16, 4, 256, 2, "big", 9), (16, 4, 256, 3, 40, 17), (16, 4, 256, 4, 40, 1), (16, 4, 256, 3, "big", 9),
         (12, 6, 100, 2, 40, 17), (12, 6, 100, 3, "big", 1), (12, 6, 100, 4, 40, 9), (12, 6, 100, 4, "big", 17)]


@pytest.mark.parametrize("nx,nu,H,M,K,T", CASES)
def test_command_equals_oracle_on_the_one_wave_per_copy_kernel(nx, nu, H, M, K, T):
    K = K if isinstance(K, int) else 64 * torch.cuda.get_device_properties(0).multi_processor_count + 40
    _, moved, _ = _parity(dict(kind="mlp", K=K, T=T, nx=nx, nu=nu, H=H), M)
    assert moved >= 1, "the matrix-core kernel must take M > 1 at this shape"


def test_rows_generated_in_the_kernel_and_the_states_of_the_per_lane_rerun():
    """rng="philox" at a short horizon: every copy-wave regenerates the action rows, copy 0 stores what the oracle is fed.  The lazy
    `states` come from a per-lane launch on the same process-noise stream: they tie the new kernel's counters to it"""
    ctrl, moved, (r64, r32) = _parity(dict(kind="mlp", K=200, T=9, nx=16, nu=4, H=64), 3, rng="philox", in_k1=True)
    assert moved >= 1 and ctrl.last_draw == "philox-k1", ctrl.last_draw
    assert ctrl.states.shape == (3, 200, 9, 16)
    margins.check("mlp split multi", "states", ctrl.states.cpu().numpy(), r64["states"].numpy(), r32["states"].numpy())


def test_bounds_and_null_action_row():
    ctrl, moved, _ = _parity(dict(kind="mlp", K=200, T=5, nx=12, nu=6, H=64), 2,
                             both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert moved >= 1 and torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


def test_smppi_lifted_controls():
    _, moved, _ = _parity(dict(kind="mlp", K=200, T=9, nx=16, nu=4, H=128), 3, rng="philox", smppi=True)
    assert moved >= 1


def test_deterministic_copies_cost_what_one_rollout_costs():
    _, moved, _ = _parity(dict(kind="mlp", K=200, T=9, nx=16, nu=4, H=64), 3, noisy=False)
    assert moved >= 1


def test_same_draws_through_the_per_lane_copies_and_the_one_wave_per_copy_kernel(monkeypatch):
    cfg = dict(kind="mlp", K=200, T=9, nx=12, nu=6, H=128)
    monkeypatch.setenv("MPPI_MLP_MULTI", "0")
    per_lane, moved, _ = _parity(cfg, 4)
    assert moved == 0
    monkeypatch.delenv("MPPI_MLP_MULTI")
    multi, moved, (r64, r32) = _parity(cfg, 4)
    assert moved >= 1 and torch.equal(F._consumed_normals(per_lane), F._consumed_normals(multi))
    for c in (per_lane, multi):                              # both within the rule of the same fp64 costs
        margins.check("mlp split multi per-lane | per-copy", "cost_total", c.cost_total.cpu().numpy(), r64["cost_total"].numpy(), r32["cost_total"].numpy())


def test_rows_left_to_k1_are_filled_after_all_where_the_kernel_refuses(monkeypatch):
    """philox_fill = False under MPPI_MLP_MULTI=0: the per-lane copies read rows from memory, so the command fills them and runs"""
    monkeypatch.setenv("MPPI_MLP_MULTI", "0")
    ctrl, moved, _ = _parity(dict(kind="mlp", K=200, T=9, nx=16, nu=4, H=64), 3, rng="philox", in_k1=True)
    assert moved == 0 and ctrl.last_draw == "philox-fill", ctrl.last_draw
