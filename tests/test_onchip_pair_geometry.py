"""Where the rows of the two-waves-per-sample on-chip kernel wait (csrc/common.hpp onchip_pair_geometry, exported as
mppi_onchip_pair_split), restated: per wave, KR local super-steps in registers, nsl in LDS, nmem in the spill array, the last nres of
the wave's real ones resident in the registers of the last iteration (MPPI_PAIR_TAIL, the default), nregen generated a second time
(the padding behind the last chunk counts there).  No GPU needed."""
import ctypes as C

import pytest

from pytorch_mppi_amd import _native as N

NU, NX = 12, 16
KEYS = ("P4", "SW", "CH", "KR", "nch", "nls", "ntl", "nsl", "nsm", "nres", "nmem", "nregen")


def _split(T, plain=True):
    out = (C.c_int32 * 16)()
    ok = int(N.lib().mppi_onchip_pair_split(NU, NX, T, int(plain), out))
    return ok, dict(zip(KEYS, list(out)))


def _restated(T, plain, tail, kt=1, pbrows=12):
    p4, sw = 3, 5                                      # nu = 12: rows of four per super-step, super-steps per weighting tile
    ch = pbrows // p4 - (0 if plain else 1)
    kr = kt * sw
    nss = T
    nch = -(-nss // ch)
    nit = (nch + 1) // 2
    nls = nit * ch
    ntl = -(-nls // sw)
    shn = max((NX + 2 + (0 if plain else NU)) * 256, 8 * ntl * 64)
    fixed = (3 * nss * p4 * 4 + 16 + shn) * 4
    room = (160 * 1024 - fixed) // (p4 * 512 * 16)
    nsl = max(0, min((nch // 2) * ch - kr, room))
    nsl -= nsl % sw
    after = ntl * sw - kr - nsl

    def real(ls):
        return ls < nls and (2 * (ls // ch)) * ch + ls % ch < nss
    areal = sum(1 for ls in range(kr + nsl, ntl * sw) if real(ls))
    best, dls = 1e30, 0
    for c in range(0, 4):                              # the array's size: whole tiles left out, the share closest to a third
        if c * sw > after:
            break
        d = abs(sum(1 for ls in range((ntl - c) * sw, ntl * sw) if real(ls)) - 0.32 * areal)
        if d < best - 1e-9:
            best, dls = d, c * sw
    nsm = after - dls
    if not tail:
        return dict(P4=p4, SW=sw, CH=ch, KR=kr, nch=nch, nls=nls, ntl=ntl, nsl=nsl, nsm=nsm, nres=0, nmem=nsm, nregen=dls)
    nres = min(ch, max(nls - kr - nsl, 0))
    mid, pad = nls - nres - kr - nsl, ntl * sw - nls
    rg = min((mid + 3) // 6, mid)                      # one in six of the rows between LDS and the resident chunk: C3's measured best
    rg = max(rg, mid - nsm)
    return dict(P4=p4, SW=sw, CH=ch, KR=kr, nch=nch, nls=nls, ntl=ntl, nsl=nsl, nsm=nsm, nres=nres, nmem=mid - rg, nregen=rg + pad)


@pytest.mark.parametrize("tail", [1, 0])
@pytest.mark.parametrize("plain", [True, False])
def test_pair_split_is_the_geometry_restated(plain, tail, monkeypatch):
    monkeypatch.delenv("MPPI_PAIR_DLS", raising=False)
    monkeypatch.setenv("MPPI_PAIR_TAIL", str(tail))
    p = N.MppiProblem()
    p.K, p.nx, p.nu, p.dtype, p.sigma_diagonal, p.model_id = 600, NX, NU, N.F32, 1, N.MODEL_INTEGRATOR
    for T in range(16, 257):
        ok, g = _split(T, plain)
        assert ok == 1 and g == _restated(T, plain, tail), (T, g, _restated(T, plain, tail))
        # every local super-step of a wave's tiles is in exactly one place
        assert g["KR"] + g["nsl"] + g["nmem"] + g["nres"] + g["nregen"] == g["ntl"] * g["SW"], (T, g)
        assert min(g["nres"], g["nmem"], g["nregen"]) >= 0 and g["nres"] <= g["CH"]
        # the rows that wait in memory fit the array a caller allocates and, with resident rows, end in front of them
        assert g["nmem"] <= g["nsm"], (T, g)
        if tail:
            assert g["KR"] + g["nsl"] + g["nmem"] + g["nres"] <= g["nls"], (T, g)
        p.T = T
        elems = int(N.lib().mppi_onchip_spill_elems(C.byref(p)))
        if elems:                                       # (0: a horizon the one-wave kernel holds in registers -- no array, no pair kernel)
            assert g["nmem"] * g["P4"] * 3 * 512 * 4 <= elems, (T, g, elems)
    if plain:
        ok, g = _split(64, True)                        # C3
        want = dict(nres=4, nmem=15, nregen=3 + 3) if tail else dict(nres=0, nmem=15, nregen=10)
        assert {k: g[k] for k in want} == want and (g["KR"], g["nsl"], g["nsm"], g["ntl"]) == (5, 5, 15, 7), g


def test_pair_tail_switch_and_override_are_read_at_every_call(monkeypatch):
    monkeypatch.delenv("MPPI_PAIR_DLS", raising=False)
    monkeypatch.delenv("MPPI_PAIR_TAIL", raising=False)
    assert _split(64)[1]["nres"] == 4, "on by default"
    monkeypatch.setenv("MPPI_PAIR_TAIL", "0")
    assert _split(64)[1]["nres"] == 0
    monkeypatch.setenv("MPPI_PAIR_TAIL", "1")
    for d, mem in ((0, 18), (3, 15), (8, 10), (30, 0)):       # regenerated super-steps beside the resident four, of 18 in between
        monkeypatch.setenv("MPPI_PAIR_DLS", str(d))
        g = _split(64)[1]
        assert (g["nres"], g["nmem"]) == (4, mem) and g["nsm"] >= g["nmem"], (d, g)


@pytest.mark.parametrize("tail", [1, 0])
def test_no_wave_without_stored_rows_meets_a_second_memory_tile(tail, monkeypatch):
    """the in-loop prefetch of the next memory tile (csrc/rollout_onchip_pair.hpp `fetch`) now loads nothing for a wave that stored
    nothing; this enumeration shows that the unguarded form was never reached: over every horizon, both instantiations and every
    MPPI_PAIR_DLS, a wave whose real rows all fit registers + LDS never has two tiles that read memory."""
    monkeypatch.setenv("MPPI_PAIR_TAIL", str(tail))
    nearest = []
    for dls in [None] + list(range(0, 31)):
        if dls is None:
            monkeypatch.delenv("MPPI_PAIR_DLS", raising=False)
        else:
            monkeypatch.setenv("MPPI_PAIR_DLS", str(dls))
        for plain in (True, False):
            for T in range(4, 257):
                ok, g = _split(T, plain)
                if not ok or g["nch"] < 4:
                    continue
                ch, sw = g["CH"], g["SW"]
                tb = (g["KR"] + g["nsl"]) // sw
                tm = min(tb + -(-g["nmem"] // sw), g["ntl"])
                for h in (0, 1):
                    nreal = sum(1 for ls in range(g["nls"]) if (2 * (ls // ch) + h) * ch + ls % ch < T)
                    nstored = min(nreal, g["KR"] + g["nsl"] + g["nmem"])
                    if nstored <= tb * sw:
                        assert tm - tb < 2, (T, plain, dls, h, g)
                        if tm - tb == 1:
                            nearest.append((T, plain, h))
    assert (13, True, 1) in nearest or tail == 1      # the shape tests/test_gpu_onchip_pair_tail.py runs (tail off: one memory tile)
