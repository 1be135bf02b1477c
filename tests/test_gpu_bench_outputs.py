"""GPU: what a plain `bench.py --gpus 1 --steps N --warmup W` run prints and what `--dump-outputs DIR` writes.  bench.main() runs
in this process (no second interpreter start): twice with the same arguments."""
import json
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_plain_line_is_the_headline_alone_and_dumped_outputs_repeat(tmp_path, capsys, monkeypatch):
    import bench
    K, T, nu = bench.WORKLOADS["c3"][4], bench.WORKLOADS["c3"][5], bench.WORKLOADS["c3"][3]
    cpu_rng, gpu_rng = torch.get_rng_state(), torch.cuda.get_rng_state()
    lines, dumps = [], []
    try:
        for run in range(2):
            d = tmp_path / f"run{run}"
            monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--dump-outputs", str(d)])
            bench.main()
            out = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
            assert len(out) == 1
            lines.append(json.loads(out[0]))
            dumps.append({p.name: np.load(p) for p in sorted(d.iterdir())})
    finally:
        torch.set_rng_state(cpu_rng)
        torch.cuda.set_rng_state(gpu_rng)
    for ln in lines:
        assert ln["steps"] == 3 and ln["warmup"] == 2 and ln["n_gpus"] == 1 and ln["dtype"] == "f32"
        assert ln["unit"] == "rollouts/s" and ln["higher_is_better"] is True and ln["ms_per_step"] > 0
        # value = K rollouts per step / the time of one step
        assert abs(ln["value"] - K / (ln["ms_per_step"] * 1e-3)) <= 1e-9 * ln["value"]
        # nothing that takes a run of its own
        assert not {"roofline", "streaming", "onchip", "latency_ms_synced", "other_rng_modes", "other_workloads", "cpu_baseline"} & set(ln)
    shapes = {"action.npy": (nu,), "U.npy": (T, nu), "cost_total.npy": (K,)}
    assert set(dumps[0]) == set(dumps[1]) == set(shapes)
    for name, shape in shapes.items():
        a, b = dumps[0][name], dumps[1][name]
        assert a.dtype == np.float32 and a.shape == shape and np.isfinite(a).all()
        assert np.array_equal(a, b), name            # same arguments, same inputs: the same arrays, bit for bit
    assert np.abs(dumps[0]["U.npy"]).max() > 0 and dumps[0]["cost_total.npy"].std() > 0
