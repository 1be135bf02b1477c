"""Residual MLP dynamics with a ReLU hidden layer (models.MLPResidual(..., activation="relu")) on the matrix cores
(csrc/rollout_mlp_relu.hip: both layers on three-piece bf16 operands, layer 1 in AGPRs, the layer-2 planes in LDS).  `command()`
against the fp64 oracle on the consumed draw under SURVEY 7.3's rule (err <= max(1e-5 scale, 2 x the reference's own fp32 error),
tests/margins.py) at the smallest shapes at which the kernel can go wrong -- and the launch counter says which path ran.  The
oracle's callables are written out here over the model's weights; `model.dynamics` is not used on that side."""
import os

import pytest
import torch

import margins
import test_gpu_fullsize_parity as F
from pytorch_mppi_amd import _build, _native as N, _resources as R

SHAPES = [(16, 4, 256), (12, 6, 100), (8, 2, 64), (16, 8, 128)]      # 100: zero-padded to 128 by the host


def _launches():
    return int(N.lib().mppi_stat_mlp_relu_launches())


def _model(nx, nu, H, big=False):
    import pytorch_mppi_amd as pm
    m = pm.models.MLPResidual.random(nx, nu, H, seed=2, activation="relu")
    if big:
        # unit 3 reads control 0 with weight 200 and drives state 1 with weight 1e5: from the second step on x[1] ~ 1e6 and every
        # hidden activation that reads it is far beyond fp16's 65504
        m.W1[3, nx] = 200.0
        m.W2[1, 3] = 1.0e5
    return m


def _mk(model):
    def mk(dt):
        def f(x, u):
            W1, b1, W2, b2 = (w.to(x.device, dt) for w in (model.W1, model.b1, model.W2, model.b2))
            return x + model.res_scale * (torch.relu(torch.cat((x, u), dim=1) @ W1.T + b1) @ W2.T + b2)
        return f, lambda x, u: (x ** 2).sum(dim=-1)
    return mk


def _parity(cfg, both=None, dtype=None, fused=True):
    """one command on torch's stream (rows in memory) against the oracle at lambda = max |cost| / 8 from a probe command;
    returns (controller, launches of the kernel)"""
    model = cfg.get("_model") or _model(cfg["nx"], cfg["nu"], cfg["H"])
    g = torch.Generator().manual_seed(0)
    x0, U0, sigma, kw = torch.randn(cfg["nx"], generator=g), torch.randn(cfg["T"], cfg["nu"], generator=g) * 0.02, torch.eye(cfg["nu"]), dict(both or {})
    csigma = sigma if dtype is None else sigma.to(dtype)             # the controller takes its dtype from noise_sigma
    probe = F._controller(cfg, model, csigma, kw, U0, 1.0, "torch")
    probe.command(x0.cuda())
    lam = float(probe.cost_total.abs().max()) / 8.0
    ctrl = F._controller(cfg, model, csigma, kw, U0, lam, "torch")
    assert ctrl._needs_generic() == (not fused)
    torch.manual_seed(31)
    n0 = _launches()
    act = ctrl.command(x0.cuda())
    moved = _launches() - n0
    refs = F._oracle_pair(cfg, _mk(model), sigma, {k: v for k, v in kw.items() if k != "rollout_samples"}, lam, U0, x0,
                          F._consumed_normals(ctrl))
    got = dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega)
    for k in got:
        margins.check(f"mlp relu {cfg['nx'], cfg['nu'], cfg['H']} {sorted(kw)}", k, got[k].detach().cpu().numpy(), refs[0][k].numpy(),
                      refs[1][k].numpy(), rtol=1e-9 if dtype == torch.float64 else 1e-5)
    return ctrl, moved


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("K", [200, "128*n_cu+72"])
@pytest.mark.parametrize("nx,nu,H", SHAPES)
def test_command_equals_oracle_on_the_relu_kernel(nx, nu, H, K, T):
    """K = 200: a ragged second chunk with a half-active sample tile and idle waves; K = 128 n_cu + 72: the second trip of the
    persistent chunk loop"""
    K = K if isinstance(K, int) else 128 * torch.cuda.get_device_properties(0).multi_processor_count + 72
    _, moved = _parity(dict(kind="relu", K=K, T=T, nx=nx, nu=nu, H=H))
    assert moved >= 1, "the matrix-core kernel must take this shape"


@pytest.mark.gpu
def test_bounds_and_null_action_row():
    ctrl, moved = _parity(dict(kind="relu", K=200, T=5, nx=12, nu=6, H=100),
                          both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert moved >= 1 and torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


@pytest.mark.gpu
def test_smppi_lifted_controls():
    """base sequence, 1/dt rescaling and smoothness cost inside the kernel, against `oracle.smppi_command`"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc
    model, g = _model(16, 4, 64), torch.Generator().manual_seed(0)
    x0, U0, sigma = torch.randn(16, generator=g), torch.randn(16, 4, generator=g) * 0.02, torch.eye(4)
    dt_, w_, amax = 0.1, 0.7, torch.full((4,), 1.2)

    def make(lam):
        return pm.SMPPI(model.dynamics, model.running_cost, 16, sigma, num_samples=200, horizon=16, device="cuda", lambda_=lam,
                        rng="philox", seed=4321, U_init=U0.clone(), action_max=amax, w_action_seq_cost=w_, delta_t=dt_)
    probe = make(1.0)
    probe.command(x0.cuda())
    ctrl = make(float(probe.cost_total.abs().max()) / 8.0)
    A0, Ud0, n0 = ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone(), _launches()
    act = ctrl.command(x0.cuda())
    assert _launches() == n0 + 1
    z, outs = F._consumed_normals(ctrl), []
    for dt in (torch.float64, torch.float32):
        f, q = _mk(model)(dt)
        p = orc.Problem(dynamics=f, running_cost=q, nx=16, noise_sigma=sigma.to(dt), K=200, T=16, lambda_=ctrl.lambda_)
        outs.append(orc.smppi_command(p, Ud0.to(dt), A0.to(dt), x0.to(dt), z.to(dt), -amax.to(dt), amax.to(dt), w_, dt_, True))
    F._check("mlp relu smppi", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega), *outs)


@pytest.mark.gpu
def test_weights_and_activations_beyond_fp16_range():
    """what a fp16 operand path would fail: W2 = 1e5, W1 = 200, activations ~ 1e5..1e6 -- same kernel, same rule"""
    m = _model(16, 4, 64, big=True)
    assert m.flags() == 0
    ctrl, moved = _parity(dict(kind="relu", K=200, T=5, nx=16, nu=4, H=64, _model=m))
    assert moved >= 1 and float(ctrl.cost_total.max()) > 1e9 and bool(torch.isfinite(ctrl.cost_total).all())


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["fp64", "rollout_samples=2", "states"])
def test_what_the_relu_kernel_does_not_serve_runs_the_callback_loop(what):
    cfg = dict(kind="relu", K=200, T=5, nx=12, nu=6, H=100)
    if what == "rollout_samples=2":
        # the copies of a deterministic model agree: the oracle's single rollout is the mean, the variance term is zero.  The
        # process noise (std 0: adds exactly nothing) makes the model stochastic as far as the path decision goes
        cfg["_model"] = _model(12, 6, 100).with_process_noise(0.0)
    ctrl, moved = _parity(cfg, both=dict(rollout_samples=2) if what == "rollout_samples=2" else None,
                          dtype=torch.float64 if what == "fp64" else None, fused=what == "states")
    assert moved == (1 if what == "states" else 0)
    if what == "states":
        ctrl._want_states = True
        n0, got = _launches(), ctrl.states.cpu()
        assert _launches() == n0 and got.shape == (1, 200, 5, 12)
        g = torch.Generator().manual_seed(0)
        f, x, u = _mk(_model(12, 6, 100))(torch.float64)[0], torch.randn(12, generator=g).double().expand(200, -1), ctrl.perturbed_action.double().cpu()
        for t in range(5):
            x = f(x, u[:, t])
            margins.check("mlp relu states", f"x[{t}]", got[0, :, t].numpy(), x.numpy())


def test_activation_argument():
    import pytorch_mppi_amd as pm
    a, b = pm.models.MLPResidual.random(12, 6, 100, seed=2), pm.models.MLPResidual.random(12, 6, 100, seed=2, activation="tanh")
    assert (a.model_id, a.hidden, a.flags()) == (b.model_id, b.hidden, b.flags()) == (N.MODEL_MLP, 128, 0)
    assert torch.equal(a.param_blob("cpu", torch.float32), b.param_blob("cpu", torch.float32))
    with pytest.raises(ValueError):
        pm.models.MLPResidual.random(12, 6, 100, activation="gelu")
    m = _model(12, 6, 100)
    assert (m.model_id, m.hidden, m.flags()) == (N.MODEL_MLP_RELU, 128, 0)
    g = torch.Generator().manual_seed(1)
    x, u = torch.randn(7, 12, generator=g, dtype=torch.float64), torch.randn(7, 6, generator=g, dtype=torch.float64)
    assert torch.equal(m.dynamics(x, u), _mk(m)(torch.float64)[0](x, u))


def test_no_relu_kernel_spills():
    if not os.path.exists(_build.LIB):
        pytest.skip("library not built")
    hit = R.find(R.kernels(_build.LIB), "rollout_mlp_relu_kernel<")
    assert len(hit) == 24, sorted(hit)                       # 4 shapes x 3 widths x (rows | raw actions)
    for name, r in hit.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
