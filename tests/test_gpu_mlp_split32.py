"""Dense-MLP dynamics with 16 < nx <= 32 states on the matrix cores (csrc/rollout_mlp_split32.hip: two layer-2 output tiles, two
layer-1 k-steps, layer-1 weights in LDS).  `command()` against the fp64 oracle on the consumed draw under SURVEY 7.3's rule
(err <= max(1e-5 scale, 2 x the reference's own fp32 error), tests/margins.py), at the smallest shapes at which the kernel can go
wrong -- and the launch counter says which kernel ran: a silent fall-back to the per-lane kernel or to the callback loop fails."""
import os

import pytest
import torch

import margins
import test_gpu_fullsize_parity as F
from pytorch_mppi_amd import _build, _native as N, _resources as R

SHAPES = [(32, 8, 64), (32, 8, 256), (24, 6, 100)]          # hidden 100: zero-padded to 128 by the host


def _launches():
    return int(N.lib().mppi_stat_mlp_split32_launches())


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _well_conditioned_lambda(cost):
    """lambda = max |cost| / 8.  The softmax turns a cost error dc into a weight error d omega / omega = dc / lambda, and any fp32
    rollout -- the reference's own included -- carries dc ~ 2^-22 max |cost|.  With lambda >= max |cost| / 8 that is at most
    2 x 8 x 2^-22 = 4e-6 on omega, U and action: inside the rule's 1e-5 branch, so those three measure the kernel and the update, not
    which of two equally sized rounding errors happened to land on a heavy sample (at a lambda for N_eff = 1000 the ratio err / own
    fp32 floor of the derived outputs has p95 ~ 2-3 for ANY fp32 kernel, tests/test_gpu_fullsize_parity.py -- the full-size case
    below is judged over seeds for that reason).  cost_total, what the kernel itself computes, is judged the same at any lambda."""
    return float(cost.abs().max()) / 8.0


def _parity(cfg, both=None, dtype=None):
    """one command on torch's stream (rows in memory at any horizon) against the oracle; returns (controller, launches of the
    kernel by that command, (fp64, fp32) oracle results).  `both`: further keywords of the controller and of the oracle"""
    model, mk, sigma, kw, x0, U0 = F._setup(cfg)
    kw = dict(kw, **(both or {}))
    csigma = sigma if dtype is None else sigma.to(dtype)             # the controller takes its dtype from noise_sigma
    probe = F._controller(cfg, model, csigma, kw, U0, 1.0, "torch")
    probe.command(x0.cuda())
    lam = _well_conditioned_lambda(probe.cost_total)
    ctrl = F._controller(cfg, model, csigma, kw, U0, lam, "torch")
    assert not ctrl._needs_generic()
    torch.manual_seed(31)
    n0 = _launches()
    act = ctrl.command(x0.cuda())
    moved = _launches() - n0
    refs = F._oracle_pair(cfg, mk, sigma, kw, lam, U0, x0, F._consumed_normals(ctrl))
    F._check(f"mlp split32 {cfg} {sorted(kw)}", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega), *refs)
    return ctrl, moved, refs


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("K", [200, "128*n_cu+72"])
@pytest.mark.parametrize("nx,nu,H", SHAPES)
def test_command_equals_oracle_on_the_two_tile_kernel(nx, nu, H, K, T):
    """K = 200: a ragged second chunk with a half-active sample tile and idle waves; K = 128 n_cu + 72: the second trip of the
    persistent chunk loop"""
    K = K if isinstance(K, int) else 128 * _n_cu() + 72
    _, moved, _ = _parity(dict(kind="mlp", K=K, T=T, nx=nx, nu=nu, H=H))
    assert moved >= 1, "the two-tile matrix-core kernel must take this shape"


@pytest.mark.gpu
def test_bounds_and_null_action_row():
    ctrl, moved, _ = _parity(dict(kind="mlp", K=200, T=5, nx=24, nu=6, H=64),
                             both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert moved >= 1 and torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


@pytest.mark.gpu
def test_smppi_lifted_controls():
    """base sequence, 1/dt rescaling and smoothness cost inside the kernel, against `oracle.smppi_command`"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc
    cfg = dict(kind="mlp", K=200, T=8, nx=32, nu=8, H=64)            # 16 rows per sample: the generator launch, rows in memory
    model, mk, sigma, _, x0, U0 = F._setup(cfg)
    dt_, w_, amax = 0.1, 0.7, torch.full((8,), 1.2)

    def make(lam):
        return pm.SMPPI(model.dynamics, model.running_cost, 32, sigma, num_samples=200, horizon=8, device="cuda", lambda_=lam, rng="philox",
                        seed=4321, U_init=U0.clone(), action_max=amax, w_action_seq_cost=w_, delta_t=dt_)
    probe = make(1.0)
    probe.command(x0.cuda())
    lam = _well_conditioned_lambda(probe.cost_total)
    ctrl = make(lam)
    A0, Ud0, n0 = ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone(), _launches()
    act = ctrl.command(x0.cuda())
    assert _launches() == n0 + 1
    z, outs = F._consumed_normals(ctrl), []
    for dt in (torch.float64, torch.float32):
        f, q = mk(dt)
        p = orc.Problem(dynamics=f, running_cost=q, nx=32, noise_sigma=sigma.to(dt), K=200, T=8, lambda_=lam)
        outs.append(orc.smppi_command(p, Ud0.to(dt), A0.to(dt), x0.to(dt), z.to(dt), -amax.to(dt), amax.to(dt), w_, dt_, True))
    got = dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega)
    F._check("mlp split32 smppi", got, *outs)


@pytest.mark.gpu
def test_batched_two_environments_share_the_draw():
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc
    cfg = dict(kind="mlp", K=200, T=8, nx=32, nu=8, H=64)
    model, mk, sigma, _, _, _ = F._setup(cfg)
    g = torch.Generator().manual_seed(11)
    xs, U0 = torch.randn(2, 32, generator=g), torch.randn(2, 8, 8, generator=g) * 0.02

    def make(lam):
        c = pm.MPPI_Batched(model.dynamics, model.running_cost, 32, sigma, 2, num_samples=200, horizon=8, device="cuda", lambda_=lam,
                            rng="philox", seed=4321)
        c.U = U0.clone().cuda()
        return c
    probe = make(1.0)
    probe.command(xs.cuda())
    lam = _well_conditioned_lambda(probe.cost_total)
    ctrl, n0 = make(lam), _launches()
    act = ctrl.command(xs.cuda())
    assert _launches() == n0 + 1, "one launch, the environments on grid z"
    p = ctrl._last
    rows = p._keep["z"].view(-1, int(p.noise_pitch) or 200, 4)[:, :200]
    z = rows.permute(1, 0, 2).reshape(200, -1)[:, :64].reshape(200, 8, 8).cpu()
    for e in range(2):
        outs = []
        for dt in (torch.float64, torch.float32):
            f, q = mk(dt)
            pr = orc.Problem(dynamics=f, running_cost=q, nx=32, noise_sigma=sigma.to(dt), K=200, T=8, lambda_=lam)
            outs.append(orc.command(pr, U0[e].to(dt), xs[e].to(dt), z.to(dt), True))
        F._check(f"mlp split32 batched env {e}", dict(action=act[e], U=ctrl.U[e], cost_total=ctrl.cost_total[e], omega=ctrl.omega[e]), *outs)


@pytest.mark.gpu
def test_same_draw_through_the_per_lane_kernel_and_the_two_tile_kernel(monkeypatch):
    cfg = dict(kind="mlp", K=200, T=5, nx=32, nu=8, H=128)
    monkeypatch.setenv("MPPI_MLP_VALU", "1")
    per_lane, moved, _ = _parity(cfg)
    assert moved == 0
    monkeypatch.delenv("MPPI_MLP_VALU")
    split, moved, (r64, r32) = _parity(cfg)
    assert moved >= 1 and torch.equal(F._consumed_normals(per_lane), F._consumed_normals(split))
    for c in (per_lane, split):                              # both within the rule of the same fp64 costs
        margins.check("mlp split32 per-lane | two-tile", "cost_total", c.cost_total.cpu().numpy(), r64["cost_total"].numpy(), r32["cost_total"].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["healthy", "peaked"])
def test_c4_style_full_size_nx32_nu8_h256_65536x64(regime):
    n0 = _launches()
    F._run_case_over_seeds(dict(kind="mlp", K=65536, T=64, nx=32, nu=8, H=256), "philox", regime, "philox-fill")
    assert _launches() > n0


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["fp64", "states", "MPPI_MLP_EXACT=1"])
def test_what_the_two_tile_kernel_does_not_serve_runs_per_lane(what, monkeypatch):
    if what == "MPPI_MLP_EXACT=1":
        monkeypatch.setenv("MPPI_MLP_EXACT", "1")
    cfg = dict(kind="mlp", K=200, T=5, nx=24, nu=6, H=64)
    ctrl, moved, _ = _parity(cfg, dtype=torch.float64 if what == "fp64" else None)
    assert moved == (1 if what == "states" else 0)
    if what == "states":
        # the visited states come from a second K1 launch, per lane; against the fp64 dynamics on the command's own bounded actions
        ctrl._want_states = True
        n0, got = _launches(), ctrl.states.cpu()
        assert _launches() == n0 and got.shape == (1, 200, 5, 24)
        model, mk, _, _, x0, _ = F._setup(cfg)
        f, x, u = mk(torch.float64)[0], x0.double().expand(200, -1), ctrl.perturbed_action.double().cpu()
        for t in range(5):
            x = f(x, u[:, t])
            margins.check("mlp split32 states", f"x[{t}]", got[0, :, t].numpy(), x.numpy())


@pytest.mark.parametrize("nx,nu", [(32, 8), (24, 6)])
def test_the_two_tile_kernel_runs_out_of_registers_and_lds_alone(nx, nu):
    """H = 256: 128 AGPRs of layer-2 weights + 48 of the layer-1 B operand beside the pipeline's VGPRs -- no scratch, no spills"""
    if not os.path.exists(_build.LIB):
        pytest.skip("library not built")
    hit = R.find(R.kernels(_build.LIB), f"rollout_mlp_split32_kernel<16, 0, {nx}, {nu}>")
    assert len(hit) == 1, sorted(hit)
    r = next(iter(hit.values()))
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, r
