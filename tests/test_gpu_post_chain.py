"""The stages behind the bus mixdown — reverb, master section, master limiter — on ONE handle that changes
its configuration from call to call.  The files of the three stages mostly hold a handle in one configuration; which buffer each
stage reads and writes is decided per call (s2r_post_route, csrc/s2r_post_route.h), and what can go wrong there is the step from one route to
the next.  Handles, events and the one-pole bank are tests/test_gpu_reverb.py's; the models are the host test files'."""
import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import synth2_amd as s2
from synth2_amd import synth as s2s
from test_gpu_buses import ubits
from test_gpu_limiter import Lim
from test_gpu_master import Master
from test_gpu_reverb import SR, V, Model, _events, _handles, _ir
from test_master_host import np_meters

pytestmark = pytest.mark.gpu
F = np.float32
NB = 3
FRAMES = [257, 16, 300, 257, 1, 256, 16, 300, 257, 300]           # the 256-frame blocks of the master and limiter kernels are crossed


def test_every_route_on_one_handle():
    """Handle `a` walks ten configurations, one call each, three buses per call; its twin `b` makes a plain bus fill of the same
    frames every time (a panned one in step 8), so its stems are the dry signal.  The expectation is composed in numpy from them:
    the reverb's history moves in steps 2 to 5 and is fresh in step 9, the applied returns and master fader are carried through,
    the limiter's state goes from step 4 to step 6 untouched by step 5 and is fresh in step 9.  The meters after every master fill
    are the model's over that fill; the limiter's are those of the last fill that ran it (s2r.h), and there are none before step 4.
    Everything the device returns is collected first; the model is asserted to limit and to ramp; then every comparison, on bits."""
    a, b = _handles()
    rv, mm, lim = Model(), Master(), Lim(48, 0)
    ir = _ir(40, 77, True)
    steps = []                                                   # (what, {name: (got, want)})

    def bus_fill(what, n):
        x = b.sample_buses(n, SR, NB)
        steps.append((what, {"buses": (a.sample_buses(n, SR, NB), rv.expect(x))}))

    def master_fill(what, n, stems, limited):
        """-> (the model's master before the limiter, its static form, the model's s' or None)"""
        y = rv.expect(b.sample_buses(n, SR, NB))
        static = mm.static(y)
        m = mm.expect(y)
        want, sp = lim.expect(m) if limited else (m, None)
        got, st = a.sample_master(n, SR, NB, stems=stems)
        assert (st is not None) == stems
        peak, energy = a.meters()
        wp, we = np_meters(y, m)                                 # (the master's entry is over the limiter's input)
        cmp = {"master": (got, want), "peaks": (peak, wp), "energies": (energy, we)}
        if stems:
            cmp["stems"] = (st, y)
        if limited:
            lim_meters[0] = np.array([sp.min(), np.abs(want).max()], dtype=F)
        try:                                                     # of the last fill that ran the limiter; none before the first
            got_meters = np.array(a.limiter_meters(), dtype=F)
        except s2.S2rError as err:
            got_meters = err.status
        cmp["limiter meters"] = (got_meters, s2s.S2R_ERR_INVALID if lim_meters[0] is None else lim_meters[0])
        steps.append((what, cmp))
        return m, static, sp

    lim_meters = [None]
    for k, n in enumerate(FRAMES):
        _events((a, b), V, k)
        if k == 0:
            bus_fill("1: bus fill, plain", n)
        elif k == 1:
            a.set_bus_reverb(1, ir, 0.25, 1.0)
            rv.set(1, ir, 0.25, 1.0)
            bus_fill("2: bus fill, K = 40 reverb on bus 1", n)
        elif k == 2:
            m3, _, _ = master_fill("3: master fill without stems, no limiter", n, False, False)
        elif k == 3:
            lim.set((a,), float(np.abs(m3).max()) / 2.0)
            _, _, sp4 = master_fill("4: master fill with stems and limiter (48, 0)", n, True, True)
        elif k == 4:
            bus_fill("5: bus fill, the limiter set but idle", n)
        elif k == 5:
            a.clear_bus_reverb(1)
            del rv.fx[1]
            _, _, sp6 = master_fill("6: master fill with stems, the reverb removed, the limiter still on", n, True, True)
        elif k == 6:
            a.clear_master_limiter()
            master_fill("7: master fill without stems, the limiter cleared", n, False, False)
        elif k == 7:
            steps.append(("8: panned fill", {"panned": (a.sample_panned(n, SR), b.sample_panned(n, SR))}))
        elif k == 8:
            a.set_bus_reverb(1, ir, 0.25, 1.0)                   # set afresh: the history is +0.0 again, and the limiter's state initial
            rv.set(1, ir, 0.25, 1.0)
            lim = Lim(48, 0, lim.c)
            lim.set((a,), lim.c)
            mm.ret((a,), 0, 0.5)
            mm.fader((a,), 0.7)
            m9, static9, _ = master_fill("9: master fill with stems, reverb and limiter afresh, a return and the master fader on their way", n, True, True)
        else:
            a.clear_bus_reverb(1)
            del rv.fx[1]
            a.clear_master_limiter()
            bus_fill("10: bus fill, plain", n)
    # on the model, before anything is compared: the walk limits, and the ramp of step 9 is visible
    assert (sp4 < 1.0).any() or (sp6 < 1.0).any()
    assert not np.array_equal(ubits(m9), ubits(static9))
    for what, cmp in steps:
        for name, (got, want) in cmp.items():
            if isinstance(want, int):
                assert got == want, "%s: %s" % (what, name)
            else:
                assert_bits_equal_finite(got, want, "%s: %s" % (what, name))
    mm.check_committed(a)
