"""The ReLU residual MLP (models.MLPResidual(..., activation="relu"), csrc/rollout_mlp_relu.hip) at one (nx, nu, hidden), K = 65536,
T = 64, rng = philox (rows in memory), timed beside (b) the same network handed over as plain torch callables with the
controller's defaults -- what a user had before the kernel -- and (c) the tanh model on the split-operand kernel:
    python tools/mlp_relu_run.py 16 4 256 [rounds=3]
--deep: the network with two hidden layers of that width (models.MLPResidual2(..., activation="relu"),
csrc/rollout_mlp_deep_relu.hip) beside its plain callables and the tanh rollout_mlp_deep_kernel:
    python tools/mlp_relu_run.py 16 4 128 3 --deep
Pipelined commands, 5 warm-ups and 20 timed per visit, the three forms visited alternately `rounds` times in one process; one JSON
line: ms per command of every visit, the K1 launch time from the engine's device stamps, which path (b) took."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import pytorch_mppi_amd as pm  # noqa: E402
from pytorch_mppi_amd import _native as N  # noqa: E402

deep = "--deep" in sys.argv
args = [v for v in sys.argv[1:] if v != "--deep"]
nx, nu, H = (int(v) for v in args[:3])
rounds = int(args[3]) if len(args) > 3 else 3
K, T = 65536, 64
torch.manual_seed(0)
if deep:
    relu = pm.models.MLPResidual2.random(nx, nu, H, H, seed=2, activation="relu")
    tanh = pm.models.MLPResidual2.random(nx, nu, H, H, seed=2)
    Ws = [w.cuda() for w in (relu.W1, relu.b1, relu.W2, relu.b2, relu.W3, relu.b3)]
    stat = "mppi_stat_mlp_deep_relu_launches"
else:
    relu = pm.models.MLPResidual.random(nx, nu, H, seed=2, activation="relu")
    tanh = pm.models.MLPResidual.random(nx, nu, H, seed=2)
    Ws = [w.cuda() for w in (relu.W1, relu.b1, relu.W2, relu.b2)]
    stat = "mppi_stat_mlp_relu_launches"


def plain_dynamics(x, u):
    h = torch.relu(torch.cat((x, u), dim=1) @ Ws[0].T + Ws[1])
    for W, b in zip(Ws[2:-2:2], Ws[3:-2:2]):
        h = torch.relu(h @ W.T + b)
    return x + relu.res_scale * (h @ Ws[-2].T + Ws[-1])


def plain_cost(x, u):
    return (x ** 2).sum(dim=-1)


U0, x = torch.randn(T, nu) * 0.02, torch.randn(nx).cuda()
forms = {"relu_kernel": (relu.dynamics, relu.running_cost), "plain_callables": (plain_dynamics, plain_cost),
         "tanh_kernel": (tanh.dynamics, tanh.running_cost)}
ctrls = {}
for name, (f, q) in forms.items():
    c = pm.MPPI(f, q, nx, torch.eye(nu), num_samples=K, horizon=T, device="cuda", lambda_=1.0, U_init=U0.clone(), rng="philox",
                seed=1234)
    c.command(x)
    c.lambda_ = float(c.cost_total.float().std())
    ctrls[name] = c
lib = N.lib()
out = {"shape": [nx, nu, H, H] if deep else [nx, nu, H], "K": K, "T": T, "rounds": rounds,
       "plain_callables_path": "callback loop" if ctrls["plain_callables"]._model is None else "traced kernel",
       "ms_per_command": {k: [] for k in forms}, "k1_device_span_us": {k: [] for k in forms}}
n0 = int(getattr(lib, stat)())
for _ in range(rounds):
    for name, c in ctrls.items():
        for _ in range(5):
            c.command(x)
        lib.mppi_profile_enable(1 << 30)            # device stamps only
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            c.command(x)
        torch.cuda.synchronize()
        out["ms_per_command"][name].append(round((time.perf_counter() - t0) / 20 * 1e3, 4))
        dv, _ = N.profile_read_launches()
        lib.mppi_profile_enable(0)
        out["k1_device_span_us"][name].append(round(sum(dv) / len(dv), 1) if dv else None)
out["relu_launches"] = int(getattr(lib, stat)()) - n0
print(json.dumps(out))
