"""Residual MLP dynamics with TWO ReLU hidden layers (models.MLPResidual2(..., activation="relu")) on the matrix cores
(csrc/rollout_mlp_deep_relu.hip: all three layers on three-piece bf16 operands, layer 1, the output layer and the first hidden
vector in AGPRs, the hidden->hidden planes in LDS).  `command()` against the fp64 oracle on the consumed draw under SURVEY 7.3's
rule (err <= max(1e-5 scale, 2 x the reference's own fp32 error), tests/margins.py) at the smallest shapes at which the kernel
can go wrong -- and the launch counter says which path ran.  The oracle's callables are written out here over the model's
weights; `model.dynamics` is not used on that side."""
import os

import pytest
import torch

import gpu_util
import margins
import test_gpu_fullsize_parity as F
from pytorch_mppi_amd import _build, _native as N, _resources as R

# (48, 40): unequal widths padded to 64, nu > 4, lane group 3 without a full state block; (32, 32): padded to 64, three idle lane groups
SHAPES = [(16, 4, (128, 128)), (12, 6, (48, 40)), (2, 1, (32, 32)), (16, 4, (64, 64))]


def _launches():
    return int(N.lib().mppi_stat_mlp_deep_relu_launches())


def _model(nx, nu, H, big=False):
    import pytorch_mppi_amd as pm
    m = pm.models.MLPResidual2.random(nx, nu, *H, seed=2, activation="relu")
    if big:
        # layer-1 unit 3 reads control 0 alone, with weight 200; layer-2 unit 5 reads that unit alone, with weight 1e4, and drives
        # state 1 with weight 1e5: h2[5] ~ 7e6 and x[1] ~ 7e10 from the first step on, and from the second step on every layer-1
        # unit that reads x[1] and every layer-2 unit behind those is ~ 1e10 -- all far beyond fp16's 65504.  (No loop through
        # the large weights: costs stay ~ 1e23, finite in fp32 -- test_the_big_weights_stay_finite_in_fp32)
        m.W1[3, :nx], m.W1[3, nx], m.W2[5, :] = 0.0, 200.0, 0.0
        m.W2[5, 3], m.W3[1, 5] = 1.0e4, 1.0e5
    return m


def _mk(model):
    def mk(dt):
        def f(x, u):
            W1, b1, W2, b2, W3, b3 = (w.to(x.device, dt) for w in (model.W1, model.b1, model.W2, model.b2, model.W3, model.b3))
            h = torch.relu(torch.relu(torch.cat((x, u), dim=1) @ W1.T + b1) @ W2.T + b2)
            return x + model.res_scale * (h @ W3.T + b3)
        return f, lambda x, u: (x ** 2).sum(dim=-1)
    return mk


def _check(name, got, refs, rtol=1e-5):
    for k in got:
        margins.check(name, k, got[k].detach().cpu().numpy(), refs[0][k].numpy(), refs[1][k].numpy(), rtol=rtol)


def _parity(cfg, both=None, dtype=None, fused=True, sigma=None):
    """one command on torch's stream (rows in memory) against the oracle at lambda = max |cost| / 8 from a probe command;
    returns (controller, launches of the kernel)"""
    model = cfg.get("_model") or _model(cfg["nx"], cfg["nu"], cfg["H"])
    g = torch.Generator().manual_seed(0)
    x0, U0, kw = torch.randn(cfg["nx"], generator=g), torch.randn(cfg["T"], cfg["nu"], generator=g) * 0.02, dict(both or {})
    sigma = torch.eye(cfg["nu"]) if sigma is None else sigma
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
    _check(f"mlp deep relu {cfg['nx'], cfg['nu'], cfg['H']} {sorted(kw)}", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total,
           omega=ctrl.omega), refs, rtol=1e-9 if dtype == torch.float64 else 1e-5)
    return ctrl, moved


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("K", [200, "128*n_cu+72"])
@pytest.mark.parametrize("nx,nu,H", SHAPES)
def test_command_equals_oracle_on_the_deep_relu_kernel(nx, nu, H, K, T):
    """K = 200: a ragged second chunk with a half-active sample tile and idle waves; K = 128 n_cu + 72: the second trip of the
    persistent chunk loop"""
    K = K if isinstance(K, int) else 128 * torch.cuda.get_device_properties(0).multi_processor_count + 72
    _, moved = _parity(dict(kind="relu2", K=K, T=T, nx=nx, nu=nu, H=H))
    assert moved >= 1, "the matrix-core kernel must take this shape"


@pytest.mark.gpu
def test_bounds_and_null_action_row():
    ctrl, moved = _parity(dict(kind="relu2", K=200, T=5, nx=12, nu=6, H=(48, 40)),
                          both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert moved >= 1 and torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


def _lifted(make, x0):
    """the controller `make` builds, at lambda = max |cost| / 8 of a probe command"""
    probe = make(1.0)
    probe.command(x0.cuda())
    return make(float(probe.cost_total.abs().max()) / 8.0)


@pytest.mark.gpu
def test_smppi_lifted_controls():
    """base sequence, 1/dt rescaling and smoothness cost inside the kernel, against `oracle.smppi_command`"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc
    model, g = _model(16, 4, (64, 64)), torch.Generator().manual_seed(0)
    x0, U0, sigma = torch.randn(16, generator=g), torch.randn(16, 4, generator=g) * 0.02, torch.eye(4)
    dt_, w_, amax = 0.1, 0.7, torch.full((4,), 1.2)
    ctrl = _lifted(lambda lam: pm.SMPPI(model.dynamics, model.running_cost, 16, sigma, num_samples=200, horizon=16, device="cuda",
                                        lambda_=lam, rng="philox", seed=4321, U_init=U0.clone(), action_max=amax,
                                        w_action_seq_cost=w_, delta_t=dt_), x0)
    A0, Ud0, n0 = ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone(), _launches()
    act = ctrl.command(x0.cuda())
    assert _launches() == n0 + 1
    z, outs = F._consumed_normals(ctrl), []
    for dt in (torch.float64, torch.float32):
        f, q = _mk(model)(dt)
        p = orc.Problem(dynamics=f, running_cost=q, nx=16, noise_sigma=sigma.to(dt), K=200, T=16, lambda_=ctrl.lambda_)
        outs.append(orc.smppi_command(p, Ud0.to(dt), A0.to(dt), x0.to(dt), z.to(dt), -amax.to(dt), amax.to(dt), w_, dt_, True))
    _check("mlp deep relu smppi", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega), outs)


@pytest.mark.gpu
def test_kmppi_raw_actions():
    """KMPPI's two-launch form: the kernel's raw-action instantiation, under a diagonal Sigma with unequal entries and a bound"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc
    nx, nu, T, S = 12, 6, 9, 5
    model, x0 = _model(nx, nu, (48, 40)), torch.randn(nx, generator=torch.Generator().manual_seed(0))
    sigma, umax = torch.diag(torch.linspace(0.5, 1.2, nu)), torch.full((nu,), 1.1)
    ctrl = _lifted(lambda lam: pm.KMPPI(model.dynamics, model.running_cost, nx, sigma, num_samples=200, horizon=T, device="cuda",
                                        lambda_=lam, rng="philox", seed=4321, U_init=torch.zeros(T, nu), num_support_pts=S,
                                        kernel=pm.RBFKernel(sigma=1.5), u_max=umax), x0)
    n0 = _launches()
    act = ctrl.command(x0.cuda())
    assert _launches() == n0 + 1 and not ctrl._needs_generic()
    z, outs = gpu_util.device_philox_normals(ctrl, int(ctrl._call), Tn=S), []
    for dt in (torch.float64, torch.float32):
        f, q = _mk(model)(dt)
        p = orc.Problem(dynamics=f, running_cost=q, nx=nx, noise_sigma=sigma.to(dt), K=200, T=T, lambda_=ctrl.lambda_, u_max=umax.to(dt))
        W, W_shift, _, _ = orc.kmppi_matrices(T, S, dt, kernel=lambda t_, tk: orc.rbf_kernel(t_, tk, sigma=1.5))
        outs.append(orc.kmppi_command(p, torch.zeros(S, nu, dtype=dt), torch.zeros(T, nu, dtype=dt), x0.to(dt), z.to(dt), W, W_shift, True))
    _check("mlp deep relu kmppi", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega, theta=ctrl.theta), outs)


def test_the_big_weights_stay_finite_in_fp32():
    """the fp32 oracle alone, on the host: activations of both hidden layers and the state beyond 65504, every cost finite"""
    m, g = _model(16, 4, (64, 64), big=True), torch.Generator().manual_seed(0)
    x, cost = torch.randn(16, generator=g).expand(200, -1), torch.zeros(200)
    f, q = _mk(m)(torch.float32)
    for t in range(5):
        xu = torch.cat((x, torch.randn(200, 4, generator=g)), dim=1)
        h1 = torch.relu(xu @ m.W1.T + m.b1)
        x = f(x, xu[:, 16:])
        cost = cost + q(x, None)
    assert float(h1.max()) > 65504 and float(torch.relu(h1 @ m.W2.T + m.b2).max()) > 65504 and float(x.abs().max()) > 65504
    assert bool(torch.isfinite(cost).all()) and float(cost.max()) < 1e30


@pytest.mark.gpu
def test_weights_and_activations_beyond_fp16_range():
    """what a fp16 operand path would fail: W1 = 200, W2 = 1e4, W3 = 1e5, activations ~ 1e7..1e10 -- same kernel, same rule"""
    m = _model(16, 4, (64, 64), big=True)
    assert m.flags() == 0
    ctrl, moved = _parity(dict(kind="relu2", K=200, T=5, nx=16, nu=4, H=(64, 64), _model=m))
    assert moved >= 1 and float(ctrl.cost_total.max()) > 1e9 and bool(torch.isfinite(ctrl.cost_total).all())


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["fp64", "full Sigma", "rollout_samples=2", "states"])
def test_what_the_deep_relu_kernel_does_not_serve_runs_the_callback_loop(what):
    cfg = dict(kind="relu2", K=200, T=5, nx=12, nu=6, H=(48, 40))
    if what == "rollout_samples=2":
        # the copies of a deterministic model agree: the oracle's single rollout is the mean, the variance term is zero.  The
        # process noise (std 0: adds exactly nothing) makes the model stochastic as far as the path decision goes
        cfg["_model"] = _model(12, 6, (48, 40)).with_process_noise(0.0)
    sigma = torch.eye(6) + 0.3 * torch.diag(torch.ones(5), 1) + 0.3 * torch.diag(torch.ones(5), -1) if what == "full Sigma" else None
    ctrl, moved = _parity(cfg, both=dict(rollout_samples=2) if what == "rollout_samples=2" else None,
                          dtype=torch.float64 if what == "fp64" else None, fused=what == "states", sigma=sigma)
    assert moved == (1 if what == "states" else 0)
    if what == "states":
        ctrl._want_states = True
        n0, got = _launches(), ctrl.states.cpu()
        assert _launches() == n0 and got.shape == (1, 200, 5, 12)
        g = torch.Generator().manual_seed(0)
        f, x, u = _mk(_model(12, 6, (48, 40)))(torch.float64)[0], torch.randn(12, generator=g).double().expand(200, -1), ctrl.perturbed_action.double().cpu()
        for t in range(5):
            x = f(x, u[:, t])
            margins.check("mlp deep relu states", f"x[{t}]", got[0, :, t].numpy(), x.numpy())


def test_activation_argument():
    import pytorch_mppi_amd as pm
    a, b = pm.models.MLPResidual2.random(12, 6, 48, 40, seed=2), pm.models.MLPResidual2.random(12, 6, 48, 40, seed=2, activation="tanh")
    assert (a.model_id, a.hidden, a.flags()) == (b.model_id, b.hidden, b.flags()) == (N.MODEL_MLP2, 64, 0)
    assert torch.equal(a.param_blob("cpu", torch.float32), b.param_blob("cpu", torch.float32))
    with pytest.raises(ValueError):
        pm.models.MLPResidual2.random(12, 6, 48, 40, activation="gelu")
    m = _model(12, 6, (48, 40))
    assert (m.model_id, m.hidden, m.flags()) == (N.MODEL_MLP2_RELU, 64, 0)
    assert (_model(2, 1, (32, 32)).hidden, _model(16, 4, (100, 128)).hidden, _model(7, 5, (48, 40)).hidden) == (64, 128, 48)
    g = torch.Generator().manual_seed(1)
    x, u = torch.randn(7, 12, generator=g, dtype=torch.float64), torch.randn(7, 6, generator=g, dtype=torch.float64)
    assert torch.equal(m.dynamics(x, u), _mk(m)(torch.float64)[0](x, u))


def test_static_promise_and_resources_of_the_deep_relu_kernel():
    if not os.path.exists(_build.LIB):
        pytest.skip("library not built")
    assert N.model_supported(N.MODEL_MLP2_RELU, 16, 4, N.F32, 128) and N.model_supported(N.MODEL_MLP2_RELU, 2, 1, N.F32, 64)
    assert not N.model_supported(N.MODEL_MLP2_RELU, 16, 4, N.F64, 128) and not N.model_supported(N.MODEL_MLP2_RELU, 7, 5, N.F32, 64)
    assert not N.model_supported(N.MODEL_MLP2_RELU, 16, 4, N.F32, 32)
    hit = R.find(R.kernels(_build.LIB), "rollout_mlp_deep_relu_kernel<")
    assert len(hit) == 12, sorted(hit)                       # 3 shapes x 2 widths x (rows | raw actions)
    for name, r in hit.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
