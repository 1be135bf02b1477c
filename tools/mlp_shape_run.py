"""N commands of the dense-MLP workload at one (nx, nu, hidden) -- K = 65536, T = 64, rng = philox, the split-operand matrix-core K1 --
for a rocprofv3 --pmc / --kernel-trace pass over a shape other than C4's (bench.py --workload c4 is (16, 4, 256)):
    rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE -- python tools/mlp_shape_run.py 12 6 128 [n=12]
matrix-pipe busy share = SQ_VALU_MFMA_BUSY_CYCLES / (GRBM_GUI_ACTIVE / 8 XCDs x 1024 SIMDs), as profiles/pmc_c4_mfma.json computes it.

`--deep H2`: the residual net with two hidden layers (H, H2), models.MLPResidual2 (csrc/rollout_mlp_deep.hip; MPPI_MLP_VALU=1 in the
environment: its per-lane kernel).  `--callables`: the same network handed over as plain torch callables with auto_jit -- the
tracer's dense-layer route (csrc/mlp_wide.hpp).  Only with one of these two (the plain form stays what the committed counter passes
ran): one more warm-up command, the engine's device stamps, and one JSON line: ms per command (wall clock, synchronised) and the K1 launch
time from the engine's device stamps where the launch carries them.

`--rollout-samples M --process-noise SD`: the stochastic model (`with_process_noise(SD)`) with M state rollouts per action sequence
(csrc/rollout_mlp_split_multi.hip; MPPI_MLP_MULTI=0 in the environment: the per-lane copies) timed BESIDE the deterministic M = 1
launch of the same run -- one JSON line with both K1 spans and their ratio (claim ratios within one run only).  With `--deep H2`: the
two-hidden-layer model (csrc/rollout_mlp_deep_multi.hip; MPPI_MLP_MULTI=0: the callback loop, which has no K1 launch).  With nx > 16:
the two-output-tile model (csrc/rollout_mlp_split32_multi.hip; MPPI_MLP_MULTI=0: the callback loop again)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch  # noqa: E402

import pytorch_mppi_amd as pm  # noqa: E402
from pytorch_mppi_amd import _native as N  # noqa: E402

argv, deep = list(sys.argv[1:]), 0
if "--deep" in argv:
    i = argv.index("--deep")
    deep = int(argv[i + 1])
    del argv[i:i + 2]
multi, proc_sd = 0, 0.05
for flag in ("--rollout-samples", "--process-noise"):
    if flag in argv:
        i = argv.index(flag)
        if flag == "--rollout-samples":
            multi = int(argv[i + 1])
        else:
            proc_sd = float(argv[i + 1])
        del argv[i:i + 2]
callables = "--callables" in argv
argv = [v for v in argv if v != "--callables"]
nx, nu, H = (int(v) for v in argv[:3])
n = int(argv[3]) if len(argv) > 3 else 12
K, T = 65536, 64
torch.manual_seed(0)
model = pm.models.MLPResidual2.random(nx, nu, H, deep, seed=2) if deep else pm.models.MLPResidual.random(nx, nu, H, seed=2)
dynamics, cost, jit = model.dynamics, model.running_cost, False
if callables:
    Ws = [w.cuda() for w in ((model.W1, model.b1, model.W2, model.b2, model.W3, model.b3) if deep else (model.W1, model.b1, model.W2,
            model.b2))]

    def dynamics(x, u):
        h = torch.tanh(torch.cat((x, u), dim=1) @ Ws[0].T + Ws[1])
        if deep:
            h = torch.tanh(h @ Ws[2].T + Ws[3])
        return x + model.res_scale * (h @ Ws[-2].T + Ws[-1])

    def cost(x, u):
        return (x ** 2).sum(dim=-1)
    jit = True
c = pm.MPPI(dynamics, cost, nx, torch.eye(nu), num_samples=K, horizon=T, device="cuda", lambda_=1.0,
            U_init=torch.randn(T, nu) * 0.02, rng="philox", seed=1234, auto_jit=jit)
x = torch.randn(nx).cuda()
c.command(x)
c.lambda_ = float(c.cost_total.float().std())
lib = N.lib()
if multi:
    noisy = (pm.models.MLPResidual2.random(nx, nu, H, deep, seed=2) if deep else pm.models.MLPResidual.random(nx, nu, H, seed=2))
    noisy.with_process_noise(torch.full((nx,), proc_sd))
    wide = not deep and nx > 16            # the two-output-tile model: csrc/rollout_mlp_split32_multi.hip, no per-lane copies behind it
    stat = (lib.mppi_stat_mlp_deep_multi_launches if deep else
            lib.mppi_stat_mlp_split32_multi_launches if wide else lib.mppi_stat_mlp_split_multi_launches)
    cm = pm.MPPI(noisy.dynamics, noisy.running_cost, nx, torch.eye(nu), num_samples=K, horizon=T, device="cuda", lambda_=c.lambda_,
                 U_init=torch.randn(T, nu) * 0.02, rng="philox", seed=1234, rollout_samples=multi, rollout_var_cost=0.3,
                 rollout_var_discount=0.9)
    # (--deep under MPPI_MLP_MULTI=0 is the callback loop, with no K1 launch to stamp; everything else must be fused)
    off = os.environ.get("MPPI_MLP_MULTI")
    assert cm._needs_generic() == bool((deep or wide) and off == "0")
    out = {"shape": [nx, nu, H] + ([deep] if deep else []), "M": multi, "callback_loop": bool(cm._needs_generic()),
           "process_noise": proc_sd, "commands": n, "MPPI_MLP_MULTI": off}
    for name, ctrl in (("m1", c), ("multi", cm), ("m1_again", c)):
        for _ in range(2):
            ctrl.command(x)
        m0 = int(stat())
        lib.mppi_profile_enable(1 << 30)            # device stamps only
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            ctrl.command(x)
        torch.cuda.synchronize()
        out[name + "_ms_per_command"] = round((time.perf_counter() - t0) / n * 1e3, 4)
        dv, _ = N.profile_read_launches()
        lib.mppi_profile_enable(0)
        out[name + "_k1_device_span_us"] = round(sum(dv) / len(dv), 1) if dv else None
        out[name + ("_deep_multi_launches" if deep else "_split32_multi_launches" if wide else "_split_multi_launches")] = int(stat()) - m0
    if out["m1_k1_device_span_us"] and out["multi_k1_device_span_us"]:
        out["k1_ratio_multi_over_m1"] = round(out["multi_k1_device_span_us"] / out["m1_k1_device_span_us"], 3)
    print(json.dumps(out))
    sys.exit(0)
if not (deep or callables):
    # the counter / trace passes over the one-hidden-layer shapes: plain launches, nothing but the commands
    n0 = int(lib.mppi_stat_mlp_split_launches())
    for _ in range(n):
        c.command(x)
    torch.cuda.synchronize()
    print(f"({nx},{nu},{H}): {n} commands, split-operand launches {int(lib.mppi_stat_mlp_split_launches()) - n0}")
    sys.exit(0)
c.command(x)
d0 = int(lib.mppi_stat_mlp_deep_launches())
lib.mppi_profile_enable(1 << 30)            # device stamps only
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(n):
    c.command(x)
torch.cuda.synchronize()
ms = (time.perf_counter() - t0) / n * 1e3
dv, _ = N.profile_read_launches()
lib.mppi_profile_enable(0)
print(json.dumps({"shape": [nx, nu, H, deep], "commands": n, "ms_per_command": round(ms, 4),
                  "k1_device_span_us": round(sum(dv) / len(dv), 1) if dv else None,
                  "deep_launches": int(lib.mppi_stat_mlp_deep_launches()) - d0, "callables": callables,
                  "MPPI_MLP_VALU": os.environ.get("MPPI_MLP_VALU"), "jit_note": getattr(c, "jit_note", None)}))
