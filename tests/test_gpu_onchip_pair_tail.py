"""The two-wave on-chip kernel's resident last chunk (csrc/rollout_onchip_pair.hpp, MPPI_PAIR_TAIL): a wave that owns a chunk in the
last iteration carries that chunk's bounded noise out of the loop in its registers -- neither stored nor generated a second time --
and reduces it as a tile of its own, scattered to the slots the four-wave combine reads.  Same values, same products, same order of
every sum: every output bit for bit what MPPI_PAIR_TAIL=0 and the one-wave kernel give.

Shapes: integrator 16 x 12 (the model the pair kernel is instantiated for), K = 600 = three workgroups, the last one ragged (88 of
256 lanes); horizons at which the paths differ (P4 = 3 rows per super-step, tiles of SW = 5 super-steps, chunks of CH = 4, or 3 with
the |noise| cost / u_scale terms; registers hold KR = 5 local super-steps per wave):
  16   four chunks, the minimum the launcher accepts: the last chunk (local 4..7) overlaps the register tile -- only 5..7 are resident
  18   five chunks, the last one partial (two of four super-steps real): rows past the horizon contribute zero
  20   five full chunks: the odd wave owns none in the last iteration and carries nothing
  33   nine chunks (odd), 48: twelve, 64: sixteen (C3's geometry), 100: twenty-five -- 0 to 3 regenerated tiles with the tail off
Horizons up to 25 fit the one-wave kernel's registers, so the library sizes no spill array for them and the pair kernel would not
be used: those cases hand the command an array of their own."""
import ctypes as C

import pytest
import torch

import gpu_util
import margins

pytestmark = pytest.mark.gpu

NX, NU, K = 16, 12, 600
HORIZONS = [16, 20, 18, 33, 48, 64, 100]
BOUNDS = dict(sample_null_action=True, u_min=torch.tensor([-0.4] * 12), u_max=torch.tensor([0.6] * 12))
VARIANTS = {
    "plain": {},
    "abs-uscale": dict(noise_abs_cost=True, u_scale=1.5),            # the PLAIN = false instantiation: chunks of three super-steps
    "bounds-null": BOUNDS,
}
CASES = [(T, v, None) for T in HORIZONS for v in VARIANTS] + [(64, "plain", 0.05), (33, "plain", 0.05)]   # peaked: dead waves skip their tiles


def _make(T, kw, lam, seed=99):
    import pytorch_mppi_amd as pm
    model = pm.models.Integrator(NX, NU)
    g = torch.Generator().manual_seed(5 + margins.seed_offset())
    U0 = torch.randn(T, NU, generator=g) * 0.1
    c = pm.MPPI(model.dynamics, model.running_cost, NX, torch.eye(NU) * 0.7, num_samples=K, horizon=T, device="cuda", lambda_=lam,
                U_init=U0.clone(), rng="philox", seed=seed + margins.seed_offset(), **kw)
    c.philox_onchip = True                                             # small K: forced on chip
    if T <= 25:
        # (no array from the library at this horizon: 10 local super-steps x 3 rows x 3 workgroups x 512 threads x 4, more than any
        #  split of the pair kernel uses here)
        c._spill = ((K, T, NU), torch.empty(10 * 3 * 3 * 512 * 4, device="cuda"))
    return c, U0


def _healthy_lambda(T, kw, x0):
    probe, _ = _make(T, kw, 1.0)
    probe.command(x0)
    c = probe.cost_total
    return max(float((c - c.min()).median()), 1e-3)


def _outputs(c, u):
    return dict(action=u, U=c.U, cost_total=c.cost_total, omega=c.omega)


@pytest.mark.parametrize("case", CASES, ids=[f"T{c[0]}-{c[1]}-lam{c[2]}" for c in CASES])
def test_resident_last_chunk_changes_no_bit(case, monkeypatch):
    from pytorch_mppi_amd import _native as N
    T, variant, lam = case
    kw = VARIANTS[variant]
    lib = N.lib()
    x0 = torch.randn(NX, generator=torch.Generator().manual_seed(3)).cuda() * 0.3
    peaked = lam is not None
    if lam is None:
        monkeypatch.setenv("MPPI_ONCHIP_PAIR", "0")
        lam = _healthy_lambda(T, kw, x0)
    ctrl = [_make(T, kw, lam)[0] for _ in range(3)]
    envs = [dict(MPPI_ONCHIP_PAIR="1", MPPI_PAIR_TAIL="1"), dict(MPPI_ONCHIP_PAIR="1", MPPI_PAIR_TAIL="0"), dict(MPPI_ONCHIP_PAIR="0", MPPI_PAIR_TAIL="1")]
    for step, shift in enumerate((True, False, True)):
        got = []
        for c, env in zip(ctrl, envs):
            for k_, v_ in env.items():
                monkeypatch.setenv(k_, v_)
            n0 = int(lib.mppi_stat_onchip_pair_launches())
            u = c.command(x0, shift_nominal_trajectory=shift)
            torch.cuda.synchronize()
            assert c.last_draw == "philox-onchip" and int(lib.mppi_last_command_form()) == N.FORM_ONCHIP
            assert int(lib.mppi_stat_onchip_pair_launches()) - n0 == int(env["MPPI_ONCHIP_PAIR"]), (env, "which kernel ran")
            got.append(_outputs(c, u))
        for other, what in ((got[1], "tail off"), (got[2], "one-wave kernel")):
            for name in got[0]:
                xa, xb = got[0][name], other[name]
                assert torch.equal(xa, xb), (what, name, step, float((xa - xb).abs().max()))
        if step == 0:
            # what the peaked case is for: waves whose 64 weights are all zero (they skip their tiles); the healthy ones have none
            w = got[0]["omega"]
            dead = [bool((w[i:i + 64] == 0).all()) for i in range(0, K, 64)]
            assert any(dead) == peaked, dead


@pytest.mark.parametrize("T,variant", [(64, "plain"), (18, "bounds-null")])
def test_resident_last_chunk_vs_fp64_oracle(T, variant, monkeypatch):
    """the new path against the fp64 oracle on the normals of the device's own stream, under the criterion and the margins of
    test_gpu_onchip.py::test_onchip_random_config_vs_fp64_oracle (SURVEY 7.3 with the floor factor at 8, scale floor 1 except omega)"""
    from oracle import mppi_oracle as orc, dynamics as dyn
    from pytorch_mppi_amd import _native as N
    kw = VARIANTS[variant]
    lib = N.lib()
    monkeypatch.setenv("MPPI_ONCHIP_PAIR", "1")
    monkeypatch.setenv("MPPI_PAIR_TAIL", "1")
    x0 = torch.randn(NX, generator=torch.Generator().manual_seed(3)) * 0.3
    lam = _healthy_lambda(T, kw, x0.cuda())
    c, _ = _make(T, kw, lam)
    sigma = torch.eye(NU) * 0.7
    for step, shift in enumerate((True, False)):
        Ub = c.U.detach().cpu().clone()
        n0 = int(lib.mppi_stat_onchip_pair_launches())
        act = c.command(x0.cuda(), shift_nominal_trajectory=shift)
        torch.cuda.synchronize()
        assert int(lib.mppi_stat_onchip_pair_launches()) == n0 + 1
        z = gpu_util.device_philox_normals(c, c._call)
        outs = []
        for dt in (torch.float64, torch.float32):
            f, q = dyn.make_quadtoy(NX, NU)
            cast = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in kw.items()}
            p = orc.Problem(dynamics=f, running_cost=q, nx=NX, noise_sigma=sigma.to(dt), K=K, T=T, lambda_=lam, **cast)
            outs.append(orc.command(p, Ub.to(dt), x0.to(dt), z.to(dt), shift))
        r64, r32 = outs
        got = _outputs(c, act)
        for key in got:
            margins.check("pair tail vs fp64 oracle", f"T={T} {variant} step {step} {key}", got[key].detach().cpu().numpy(), r64[key].numpy(),
                          r32[key].numpy(), rtol=1e-5, scale_floor=1.0 if key != "omega" else 0.0, floor_factor=8.0)


def _split(T, plain=True):
    from pytorch_mppi_amd import _native as N
    out = (C.c_int32 * 16)()
    assert int(N.lib().mppi_onchip_pair_split(NU, NX, T, int(plain), out)) == 1
    keys = ("P4", "SW", "CH", "KR", "nch", "nls", "ntl", "nsl", "nsm", "nres", "nmem", "nregen")
    return dict(zip(keys, list(out)))


def test_a_wave_without_stored_rows_fetches_nothing(monkeypatch):
    """The memory tiles' prefetch inside the weighting loop had no guard for a wave that stored nothing (only the first fetch had):
    such a wave with a second memory tile ahead of it computed row -1 and read in front of its workgroup's part of the array.

    Derived from onchip_pair_geometry on the CPU (tests/test_onchip_pair_geometry.py enumerates it for T = 16 .. 256): a wave stores
    nothing only when all its real local super-steps fit registers + LDS, KR + nsl.  nsl <= (nch / 2) CH - KR, and the odd wave's
    real super-steps number more than (nch / 2 - 1) CH; so nsl = 0 and at most KR = 5 real super-steps, i.e. nch = 4 with the last
    chunk partial -- and then the wave has two tiles in all, one of them beyond the registers.  With today's constants the two
    conditions never meet, for no MPPI_PAIR_DLS either: the defect was latent.  The nearest shape is run here: T = 13 (chunks of four:
    0..3, 4..7, 8..11, 12), where the odd wave owns five real super-steps, all in registers, nothing stored, while its one memory
    tile exists (MPPI_PAIR_DLS=0: everything beyond the registers waits in memory) -- the guarded fetch, and the loop's."""
    from pytorch_mppi_amd import _native as N
    lib = N.lib()
    T = 13
    monkeypatch.setenv("MPPI_PAIR_DLS", "0")
    monkeypatch.setenv("MPPI_PAIR_TAIL", "0")
    g = _split(T)
    assert (g["nch"], g["KR"], g["nsl"], g["ntl"], g["nmem"]) == (4, 5, 0, 2, 5), g
    x0 =torch.randn(NX, generator=torch.Generator().manual_seed(3)).cuda() * 0.3
    a, b = _make(T, {}, 40.0)[0], _make(T, {}, 40.0)[0]
    for tail in ("1", "0"):
        monkeypatch.setenv("MPPI_PAIR_TAIL", tail)
        for shift in (True, False):
            monkeypatch.setenv("MPPI_ONCHIP_PAIR", "1")
            n0 = int(lib.mppi_stat_onchip_pair_launches())
            ua = a.command(x0, shift_nominal_trajectory=shift)
            torch.cuda.synchronize()
            assert int(lib.mppi_stat_onchip_pair_launches()) == n0 + 1
            monkeypatch.setenv("MPPI_ONCHIP_PAIR", "0")
            ub = b.command(x0, shift_nominal_trajectory=shift)
            torch.cuda.synchronize()
            for name, xa, xb in (("action", ua, ub), ("U", a.U, b.U), ("cost_total", a.cost_total, b.cost_total), ("omega", a.omega, b.omega)):
                assert torch.equal(xa, xb), (name, tail, shift)
