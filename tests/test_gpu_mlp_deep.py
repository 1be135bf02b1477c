"""Residual MLP dynamics with TWO hidden layers (models.MLPResidual2) on the matrix cores (csrc/rollout_mlp_deep.hip: layer 1 and
the output layer in AGPRs, the hidden->hidden layer's planes in LDS, a three-stage software pipeline) and per lane
(csrc/rollout_mlp2.hip).  `command()` against the fp64 oracle on the consumed draw under SURVEY 7.3's rule (err <= max(1e-5 scale,
2 x the reference's own fp32 error), tests/margins.py) at the smallest shapes at which the kernel can go wrong -- and the launch
counter says which kernel ran: a silent fall-back to the per-lane kernel or to the callback loop fails."""
import os

import pytest
import torch

import margins
import test_gpu_fullsize_parity as F
from pytorch_mppi_amd import _build, _native as N, _resources as R

SHAPES = [(16, 4, 128, 128), (12, 6, 48, 40), (2, 1, 32, 32)]      # (48, 40): unequal widths, zero-padded to 64 by the host


def _launches():
    return int(N.lib().mppi_stat_mlp_deep_launches())


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _setup(cfg):
    """`F._setup` for the two-hidden-layer model: (model, oracle callables factory, sigma, ctor kwargs, x0, U0).  The oracle's
    callables close over the model's weights cast to the oracle's dtype (on the device of the states they are given)."""
    import pytorch_mppi_amd as pm
    nx, nu, (h1, h2) = cfg["nx"], cfg["nu"], cfg["H"]
    model = cfg.get("_model") or pm.models.MLPResidual2.random(nx, nu, h1, h2, seed=2)
    g = torch.Generator().manual_seed(0 + margins.seed_offset())

    def mk(dt):
        def f(x, u):
            W1, b1, W2, b2, W3, b3 = (w.to(x.device, dt) for w in (model.W1, model.b1, model.W2, model.b2, model.W3, model.b3))
            return x + model.res_scale * (torch.tanh(torch.tanh(torch.cat((x, u), dim=1) @ W1.T + b1) @ W2.T + b2) @ W3.T + b3)
        return f, lambda x, u: (x ** 2).sum(dim=-1)
    x0 = torch.randn(nx, generator=g)
    return model, mk, torch.eye(nu), {}, x0, torch.randn(cfg["T"], nu, generator=g) * 0.02


def _parity(cfg, both=None, dtype=None):
    """one command on torch's stream (rows in memory at any horizon) against the oracle, at lambda = max |cost| / 8 (the reason:
    tests/test_gpu_mlp_split32.py `_well_conditioned_lambda`); returns (controller, launches of the kernel, oracle results)"""
    model, mk, sigma, kw, x0, U0 = _setup(cfg)
    kw = dict(kw, **(both or {}))
    csigma = sigma if dtype is None else sigma.to(dtype)             # the controller takes its dtype from noise_sigma
    probe = F._controller(cfg, model, csigma, kw, U0, 1.0, "torch")
    probe.command(x0.cuda())
    lam = float(probe.cost_total.abs().max()) / 8.0
    ctrl = F._controller(cfg, model, csigma, kw, U0, lam, "torch")
    assert not ctrl._needs_generic()
    torch.manual_seed(31)
    n0 = _launches()
    act = ctrl.command(x0.cuda())
    moved = _launches() - n0
    refs = F._oracle_pair(cfg, mk, sigma, kw, lam, U0, x0, F._consumed_normals(ctrl))
    got = dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega)
    for k in got:
        margins.check(f"mlp deep {cfg['nx'], cfg['nu'], cfg['H']} {sorted(kw)}", k, got[k].detach().cpu().numpy(), refs[0][k].numpy(),
                      refs[1][k].numpy(), rtol=1e-9 if dtype == torch.float64 else 1e-5)
    return ctrl, moved, refs


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("K", [200, "128*n_cu+72"])
@pytest.mark.parametrize("nx,nu,h1,h2", SHAPES)
def test_command_equals_oracle_on_the_deep_kernel(nx, nu, h1, h2, K, T):
    """K = 200: a ragged second chunk with a half-active sample tile and idle waves; K = 128 n_cu + 72: the second trip of the
    persistent chunk loop"""
    K = K if isinstance(K, int) else 128 * _n_cu() + 72
    _, moved, _ = _parity(dict(kind="mlp2", K=K, T=T, nx=nx, nu=nu, H=(h1, h2)))
    assert moved >= 1, "the matrix-core kernel must take this shape"


@pytest.mark.gpu
def test_bounds_and_null_action_row():
    ctrl, moved, _ = _parity(dict(kind="mlp2", K=200, T=5, nx=12, nu=6, H=(48, 40)),
                             both=dict(u_min=torch.full((6,), -0.4), u_max=torch.full((6,), 0.6), sample_null_action=True))
    assert moved >= 1 and torch.equal(ctrl.perturbed_action[0], torch.zeros(5, 6, device="cuda"))


@pytest.mark.gpu
def test_smppi_lifted_controls():
    """base sequence, 1/dt rescaling and smoothness cost inside the kernel, against `oracle.smppi_command`"""
    import pytorch_mppi_amd as pm
    from oracle import mppi_oracle as orc
    cfg = dict(kind="mlp2", K=200, T=16, nx=16, nu=4, H=(64, 64))     # 16 rows per sample: the generator launch, rows in memory
    model, mk, sigma, _, x0, U0 = _setup(cfg)
    dt_, w_, amax = 0.1, 0.7, torch.full((4,), 1.2)

    def make(lam):
        return pm.SMPPI(model.dynamics, model.running_cost, 16, sigma, num_samples=200, horizon=16, device="cuda", lambda_=lam,
                        rng="philox", seed=4321, U_init=U0.clone(), action_max=amax, w_action_seq_cost=w_, delta_t=dt_)
    probe = make(1.0)
    probe.command(x0.cuda())
    lam = float(probe.cost_total.abs().max()) / 8.0
    ctrl = make(lam)
    A0, Ud0, n0 = ctrl.action_sequence.detach().cpu().clone(), ctrl.U.detach().cpu().clone(), _launches()
    act = ctrl.command(x0.cuda())
    assert _launches() == n0 + 1
    z, outs = F._consumed_normals(ctrl), []
    for dt in (torch.float64, torch.float32):
        f, q = mk(dt)
        p = orc.Problem(dynamics=f, running_cost=q, nx=16, noise_sigma=sigma.to(dt), K=200, T=16, lambda_=lam)
        outs.append(orc.smppi_command(p, Ud0.to(dt), A0.to(dt), x0.to(dt), z.to(dt), -amax.to(dt), amax.to(dt), w_, dt_, True))
    F._check("mlp deep smppi", dict(action=act, U=ctrl.U, cost_total=ctrl.cost_total, omega=ctrl.omega), *outs)


@pytest.mark.gpu
def test_same_draw_through_the_per_lane_kernel_and_the_deep_kernel(monkeypatch):
    cfg = dict(kind="mlp2", K=200, T=5, nx=16, nu=4, H=(128, 128))
    monkeypatch.setenv("MPPI_MLP_VALU", "1")
    per_lane, moved, _ = _parity(cfg)
    assert moved == 0
    monkeypatch.delenv("MPPI_MLP_VALU")
    deep, moved, (r64, r32) = _parity(cfg)
    assert moved >= 1 and torch.equal(F._consumed_normals(per_lane), F._consumed_normals(deep))
    for c in (per_lane, deep):                               # both within the rule of the same fp64 costs
        margins.check("mlp deep per-lane | matrix cores", "cost_total", c.cost_total.cpu().numpy(), r64["cost_total"].numpy(),
                      r32["cost_total"].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["fp64", "states", "weights beyond fp16"])
def test_what_the_deep_kernel_does_not_serve_runs_per_lane(what):
    import pytorch_mppi_amd as pm
    cfg = dict(kind="mlp2", K=200, T=5, nx=12, nu=6, H=(48, 40))
    if what == "weights beyond fp16":
        # one hidden->hidden weight whose folded value -2 (2 log2 e) W2 = 7e4 is no fp16 (it multiplies a saturated tanh: finite)
        m = pm.models.MLPResidual2.random(12, 6, 48, 40, seed=2)
        m.W2[3, 5] = 1.25e4
        assert m.flags() == N.MODEL_FLAG_EXACT_FP32
        cfg["_model"] = m
    ctrl, moved, _ = _parity(cfg, dtype=torch.float64 if what == "fp64" else None)
    assert moved == (1 if what == "states" else 0)
    if what == "states":
        # the visited states come from a second K1 launch, per lane; against the fp64 dynamics on the command's own bounded actions
        ctrl._want_states = True
        n0, got = _launches(), ctrl.states.cpu()
        assert _launches() == n0 and got.shape == (1, 200, 5, 12)
        _, mk, _, _, x0, _ = _setup(cfg)
        f, x, u = mk(torch.float64)[0], x0.double().expand(200, -1), ctrl.perturbed_action.double().cpu()
        for t in range(5):
            x = f(x, u[:, t])
            margins.check("mlp deep states", f"x[{t}]", got[0, :, t].numpy(), x.numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["healthy", "peaked"])
def test_full_size_nx16_nu4_h128_h128_65536x64(regime, monkeypatch):
    """`F._run_case_over_seeds` is written around `F._setup` and, for kind == "mlp", runs the oracle on the GPU.  What this case
    relies on in tests/test_gpu_fullsize_parity.py: `_run_case` calls the module-level `_setup(cfg)` (replaced here by this file's)
    and, because ORACLE_DEVICE != "cpu" and cfg["kind"] == "mlp", puts (model.W1, b1, W2, b2) into cfg["_weights"]; `_oracle_pair`
    then builds its callables with `oracle.dynamics.make_mlp(*those four, on the device, in the oracle's dtype)` instead of `mk` --
    replaced here by the two-hidden-layer closure of the same dtype (its weights follow the states' device)."""
    from oracle import dynamics as dyn
    cfg = dict(kind="mlp", K=65536, T=64, nx=16, nu=4, H=(128, 128))
    monkeypatch.setattr(F, "_setup", _setup)
    monkeypatch.setattr(dyn, "make_mlp", lambda W1, *rest: _setup(cfg)[1](W1.dtype))   # (the weights do not depend on the seed)
    n0 = _launches()
    F._run_case_over_seeds(cfg, "philox", regime, "philox-fill")
    assert _launches() > n0


@pytest.mark.parametrize("nx,nu", [(16, 4), (12, 6), (2, 1)])
def test_the_kernels_of_the_deep_model_run_out_of_registers_and_lds_alone(nx, nu):
    """H = 128: 216 AGPRs of weights, layer-1 inputs and first-hidden-layer activations beside the pipeline's VGPRs; the per-lane
    kernels: every instantiation the model's own launcher builds (csrc/rollout_mlp2.hip) -- no scratch, no spilled VGPRs"""
    if not os.path.exists(_build.LIB):
        pytest.skip("library not built")
    table = R.kernels(_build.LIB)
    hit = R.find(table, f"rollout_mlp_deep_kernel<8, 0, {nx}, {nu}>")
    assert len(hit) == 1, sorted(hit)
    r = next(iter(hit.values()))
    assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, r
    lanes = R.find(table, f"Mlp2Model<float, {nx}, {nu}>") | R.find(table, f"Mlp2Model<double, {nx}, {nu}>")
    assert len(lanes) == 12, sorted(lanes)                   # (rows | Philox | raw actions) x (diagonal | full Sigma) x (fp32 | fp64)
    for name, r in lanes.items():
        assert r.get("scratch", 0) == 0 and r.get("vgpr_spill", 0) == 0, (name, r)
