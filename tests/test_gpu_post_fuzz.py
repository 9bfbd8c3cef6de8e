"""Differential fuzzing of the post-mix chain against the composed host models: the seeded walks of
tests/post_walk.py, played on twin handles.  Handle `a` makes the walk's calls; its twin `b` is fed the same events and makes a plain bus
fill of the same frames and buses every time (a panned one for a panned fill), so its output is the dry signal; the expectation is
post_walk.Chain over it — per bus the EQ's, the dynamics', the drive's, the flanger's, the chorus's, the delay's, the reverb's and the
room's model, eight of them, then the master section's and the limiter's, and behind the limiter the loudness meter's and the spectrum
meter's (test_gpu_loudness.Meter, test_gpu_spectrum.Meter), each the one its tests/test_*_host.py file pins to numpy on bits.  The device
is never compared with itself.  What a walk varies: which effects sit on which of eight buses and in what shape, n_buses and frames from call to call,
max_frames, the kind of fill, kept-state parameter moves, sets in mid-tail, state round trips, timing, and one handover of the whole
chain onto a fresh handle — the flanger's line and phase go through the round trip, the handover and the final comparison as the
chorus's do.  The meters are set, replaced — a spectrum meter at another of its six sizes —, reset and
cleared between the chain's steps, by a second generator that leaves those steps what they were; a master fill feeds each meter that
is on the stems as the chain leaves them and the master as the caller receives it, and its rows, their count and the true peaks are
compared behind every fill, a bus fill and a panned fill having to leave them alone; state, position and rows go through the round
trip and the handover, in the middle of a hop, and state and position are compared there, behind every other bus fill and panned
fill and at the end of the walk — not between two master fills in a row, so that the state's device copies flip unread as well as being
fetched and uploaded again (S2rMirror).  A master fill of max_frames + 1 frames must be refused and move nothing.
The stages of DESIGN.md 4.28 to 4.31 are in the walks too, by a third generator that leaves the steps of the first two what they
were: the multiband compressor between the master fader and the limiter (test_gpu_multiband.Mb; set at 1 to 4 bands, given new
parameters that keep its state, reset, cleared), the limiter under either detector (test_gpu_limiter_tp.LimTp; limiter_detector
switches a present limiter, which resets its state), the converter over nine (L, M, T) (test_gpu_resampler.Res) and the PCM stage
behind it or without it (test_gpu_pcm.Stage; 8, 16 and 24 bits, the three dithers, 0 to 9 taps, t reloaded just below 2^32).  The
multiband's minima, the converter's outputs of all nine programmes and the PCM stage's integers, compared as integers in value,
type and shape, with the clips of the call and the held ones, are read behind every fill, a refused one included; the four states
— the limiter's xh and gh at its detector's sizes, ph and t beside theirs — where the meters' are.  With a meter on, the converter
and the PCM stage never copy the master to the pinned output, so a walk now and then pauses its meters over one master fill
(meters_pause, meters_resume).  The master subset walk goes through the 16 subsets of the four kernels behind the limiter.
tests/test_post_walk_host.py asserts on the CPU that the default seeds cover all of that, and that a flanger runs in
calls of more than 1024 frames, at H = 4096, in calls of 255, 256 and 257 frames, and idles between two fills that run it, and
what the meters meet: its conditions 8 to 16; and what the four newer stages meet: its conditions 17 to 23.

Deterministic: the seeds are fixed and a failure names its seed, step and action and the effects present at that step;
S2R_POST_FUZZ_BASE=<that seed> S2R_POST_FUZZ_SEEDS=1 runs it again.  Every comparison is on bits with no NaN allowance
(helpers.assert_bits_equal_finite).

S2R_POST_FUZZ_SEEDS=N widens the sweep, S2R_POST_FUZZ_BASE moves it.  History: 1200 walks at bases 100000, 200000 and 300000 beside the default 32 at
base 5000 have run equal on bits, before the flanger joined the walks and again with it: no seed has found a fault in the chain yet (a seed that does goes here, as a regression).  What the
first sweeps did find was in the walks: seeds 100022 and 100037 (a walk that ended on a fader move with no master fill behind it; a
limiter whose ceiling, taken from an earlier and louder master, never worked), and on the host seed 300349 (a room under a dry of 1
whose first turn of the lines lies below half an ulp of the bus: post_walk.Chain._excused) and, with the flanger, seeds 5001, 200158,
200335 and 300143 (a flanger under a dry of 1 whose taps of the call are all +0.0 at the far end of its line, or read the first
frame behind a drive, 1e-37: the same place).
With the meters in the walks, 400 walks at base 400000 beside the default 32 have run equal on bits, and the model alone was well behaved
over the same 400 (tests/test_post_walk_host.py): no seed has found a fault in the meters, in their mirrors' transitions or in the
chain in front of them.  What the first run found was in the walk's model: seeds 5001, 5015 and 5020 (a bus fill or a panned fill
directly behind the handover: the fresh handle has made no master fill, so the true peak of its last call reads +0.0, not the old
handle's: post_walk.Chain.handed_over).  Tried once against a library with two defects put in — the walkers' block test turned from >
to >=, and one wrong twiddle in the four-layer pass at s0 = 8 that N = 4096 alone runs —, 31 of the default seeds and the subset
walk failed.
With the multiband compressor, the true-peak detector, the converter and the PCM stage in the walks, 400 walks at base 500000 beside
the default 32 and the two systematic walks have run equal on bits on an MI355X, and the model alone was well behaved over the same
400: no seed has found a fault in the four kernels, in who copies the master out, in their mirrors or in their counters.  The walks
did find a fault in the library's Python binding: Synth.pcm sized its buffer by the converter that is set now, and s2r_get_pcm
refuses a buffer shorter than the samples it holds — so the samples of a fill behind a converter of a ratio above 1, more than
max_frames of them, could not be read once that converter had been cleared or replaced by one of a smaller ratio, though s2r.h
keeps them until the next master fill.  Seeds 500030 (step 33, a panned fill) and 500211 (steps 19 and 63, a bus fill and a panned
fill) read them there, as do others of that sweep and no default seed; Synth.pcm now sizes its buffer by the largest ratio, 4,
the two seeds, which both fail against the getter as it was and pass with the 400 since, stay as
test_the_seeds_that_found_a_fault (post_walk.REGRESSION_SEEDS) and tests/test_gpu_resampler.py holds the
getter to it directly.  What else the first runs found was in the walk and its model, on the host: no master fill of the default seeds ran with both meters off, so the
converter and the PCM stage never copied the master out (hence meters_pause); the master subset walk's fader, alternating from fill
to fill, let the converter's histories carry a loud fill into a quiet one, which then clipped (it alternates from subset to subset);
and seed 500378 (a bus behind a delay with no dry path that sounds only behind the one output of a short call: the converter
rightly makes +0.0 of it, Chain.expect counts a programme as sounding only up to the newest frame an output reads).  Tried once
against three libraries with one defect each in S2rPostChain: the PCM launch behind the resampler given the call's frames for its
count (clamped to the count, so that the defective launch stays inside its buffers: wrong behind a ratio above 1) — 22 of the 32
default seeds fail, neither systematic walk, whose resampler is 147 / 160; t moved by a refused fill — 13 of the default seeds,
neither systematic walk, which make no refused fill; the resampler's kernel copying the master out whenever the loudness meter
alone is off — nothing fails, and nothing can: the spectrum kernel then copies the same frames of the same buffer to the same place,
so the defect is a second, equal write and not a wrong output."""
import os

import numpy as np
import pytest

from helpers import assert_bits_equal_finite
import post_walk as pw
import synth2_amd as s2
from test_gpu_buses import ubits
from test_gpu_reverb import SR, _events, _handles

pytestmark = pytest.mark.gpu
V = 32                                                           # voices of a pool
BASE = int(os.environ.get("S2R_POST_FUZZ_BASE", str(pw.DEFAULT_BASE)))
SEEDS = [BASE + k for k in range(int(os.environ.get("S2R_POST_FUZZ_SEEDS", str(pw.DEFAULT_SEEDS))))]


def play(setup, steps, name):
    """a walk on twin handles: everything the device returns is collected first; then the model's own conditions; then every comparison"""
    a, b = _handles(voices=V, max_frames=setup["max_frames"])
    a.set_timing(setup["timing"])
    chain = pw.Chain((a,))
    got, fill = [], 0                                            # (what, what the device returned, what Chain.expect returned, the twin's output)
    for k, action in enumerate(steps):
        what = "%s, step %d %r [present: %s]" % (name, k, action, chain.present())
        if action["kind"] in ("roundtrip", "handover"):          # what the meters carry into it: these steps read their state anyway
            got.append((what + ", on the way in", pw.meter_states_of(chain, a), chain.meter_states(), None))
        if action["kind"] == "handover":
            # The whole chain onto a fresh handle, and the walk goes on there.  The twin is handed over the same way, voices alone: which
            # voice the next note_on takes is the pool's, not part of an exported state, and only handles made alike choose alike.
            c, d = _handles(voices=V, max_frames=setup["max_frames"])
            c.set_timing(setup["timing"])
            pw.handover(chain, a, c)
            pw.copy_voices(b, d)
            a, b = c, d
        elif action["kind"] != "fill":
            chain.apply(action)
            if action["kind"] == "refused_fill":                 # it moves no reading: rows, outputs, integers and clips as the last master fill left them
                got.append((what, pw.meter_readings_of(chain, a), chain.meter_readings(), None))
        else:
            _events((a, b), V, fill)
            fill += 1
            n, nb = action["frames"], action["n_buses"]
            if action["fill"] == "panned":
                x = b.sample_panned(n, SR)
                want = chain.expect(x, action, what)
                dev = dict(panned=a.sample_panned(n, SR))
            else:
                x = b.sample_buses(n, SR, nb)
                want = chain.expect(x, action, what)             # (the model first: it tunes the drives' pre on the handle)
                if action["fill"] == "bus":
                    dev = dict(buses=a.sample_buses(n, SR, nb))
                else:
                    dev = {}
                    dev["master"], st = a.sample_master(n, SR, nb, stems=action["fill"] == "master_stems")
                    assert (st is not None) == (action["fill"] == "master_stems"), what
                    if st is not None:
                        dev["stems"] = st
                    dev["peaks"], dev["energies"] = a.meters()
                    try:                                         # of the last fill that ran the limiter on this handle; none before the first
                        dev["limiter"] = np.array(a.limiter_meters(), dtype=np.float32)
                    except s2.S2rError as err:
                        dev["limiter"] = err.status
                dev["dyn_meters"] = {bus: a.bus_dynamics_meter(bus) for bus in want["dyn_meters"]}
            # the meters that are on: rows, their count and the true peaks behind every fill — a bus fill and a panned fill must leave
            # them as they were —, through getters that leave the state's copies alone.  State and position, whose getter fetches the
            # device copy for the next master fill to upload again, behind every other bus fill and panned fill only (post_walk.peeks)
            dev.update(pw.meter_readings_of(chain, a))
            if action["fill"] in ("bus", "panned") and pw.peeks(k):
                dev.update(pw.meter_states_of(chain, a))
                want.update(chain.meter_states())
            got.append((what, dev, want, x))
    final = pw.states_of(chain, a)
    # on the model and the twin, before anything is compared: the dry signal is finite and sounds, and a walk that limits does limit
    for what, dev, want, x in got:
        assert x is None or np.isfinite(x).all(), what + ": the twin's output is not finite"
        assert x is None or ubits(x).any() or x.shape[-2] == 1, what + ": the twin is silent"      # (a voice's first frame is +0.0)
    for what, dev, want, x in got:                               # (Chain.expect lowers the ceiling where a master would stay under it)
        assert "gain" not in want or (want["gain"] < 1.0).any() or want["idle"] or want["limiter in"] <= 2.0 ** -19, what + ": the limiter does not work"
    for what, dev, want, x in got:
        for key, g in dev.items():
            w = want[key]
            if key == "dyn_meters":
                for bus in w:
                    assert_bits_equal_finite(g[bus], w[bus], "%s: the meter of the dynamics on bus %d" % (what, bus))
            elif isinstance(w, int) or isinstance(g, int):
                assert isinstance(g, int) and isinstance(w, int) and g == w, "%s: %s: %r, not %r" % (what, key, g, w)
            elif np.issubdtype(w.dtype, np.integer):             # the PCM stage's integers and its clip counts: value, type and shape
                assert g.dtype == w.dtype and g.shape == w.shape, "%s: %s: %s %s, not %s %s" % (what, key, g.dtype, g.shape, w.dtype, w.shape)
                assert np.array_equal(g, w), "%s: %s: %d of %d integers differ, the first at %s" % (
                    what, key, int((g != w).sum()), w.size, tuple(int(i[0]) for i in np.nonzero(g != w)))
            else:
                assert_bits_equal_finite(g, w, "%s: %s" % (what, key))
    model = chain.states()
    assert sorted(final) == sorted(model)
    for key in sorted(model):
        assert_bits_equal_finite(final[key], model[key], "%s, after the last step [present: %s]: the state of %s" % (name, chain.present(), key))
    chain.mm.check_committed(a)
    return chain, got


@pytest.mark.parametrize("seed", SEEDS)
def test_post_fuzz(seed):
    setup, steps = pw.walk(seed)
    play(setup, steps, "seed %d (max_frames %d, timing %s)" % (seed, setup["max_frames"], "on" if setup["timing"] else "off"))


@pytest.mark.parametrize("seed", pw.REGRESSION_SEEDS)
def test_the_seeds_that_found_a_fault(seed):
    """post_walk.REGRESSION_SEEDS, beside the sweep wherever it has been moved.  500030 and 500211: Synth.pcm on samples of more than
    max_frames frames whose converter has been cleared or replaced by one of a smaller ratio since the fill (the history paragraph
    above; tests/test_post_walk_host.py holds the walks to that on the books)"""
    setup, steps = pw.walk(seed)
    play(setup, steps, "seed %d (max_frames %d, timing %s)" % (seed, setup["max_frames"], "on" if setup["timing"] else "off"))


def test_every_insert_subset_on_every_kind_of_call():
    """The systematic complement (post_walk.subset_walk): one pair of handles, three buses, 33 frames a call, 96 calls — the 32 subsets of
    {EQ, dynamics, drive, flanger, room} in Gray-code order, so that each step sets or clears exactly one insert while the others are
    in mid-state, each subset with a bus fill, a master fill with stems and a master fill under the limiter; a chorus on bus 2 and a
    reverb on bus 1 stay on throughout.  An insert that is cleared and set again starts afresh in the model too.  The per-stage files
    run each insert alone, {EQ, dyn}, {EQ, dyn, room}, {EQ, dyn, drive, room} and all five; the seeded walks open on all 32 subsets,
    each on a fresh handle, and this is the one test that goes from subset to subset on one handle, so that the set of a flanger's
    neighbours changes while its line and phase are in mid-state, and every other insert's while a flanger is.  A loudness meter at
    hop 17 and a spectrum meter at N = 1024 are on throughout: what they are fed changes with every insert, and every other master
    fill reaches them through the limiter."""
    setup, steps = pw.subset_walk()
    chain, got = play(setup, steps, "the subset walk")
    assert len(got) == 96 and all("gain" in want and (want["gain"] < 1.0).any() for _, _, want, _ in got[2::3])
    # both meters from the first call to the last: every call compares rows and true peak, and the 64 master fills make 124 hops of 17
    # frames and 16 spectrum rows
    assert all({"loudness rows", "true peak", "true peak held", "spectrum rows"} <= set(dev) for _, dev, _, _ in got)
    assert chain.loud.made == 64 * 33 // 17 and chain.spec.made == 64 * 33 // 128 and len(chain.loud.rows) == 32 and len(chain.spec.rows) == 8


def test_every_subset_of_the_stages_behind_the_limiter():
    """The systematic complement of the third generator (post_walk.master_subset_walk): one pair of handles, three buses, max_frames
    300, an EQ and a room on throughout — the 16 subsets of {loudness, spectrum, resampler, PCM} in Gray-code order, so that each step
    sets or clears exactly one of them while the others are in mid-state, and with it who copies the master to the pinned output.
    Each subset gets three master fills, the limiter off, with the sample-peak detector and with the true-peak detector, alternately
    with and without stems and with and without a three-band multiband compressor, in calls of 127, 128, 129, 1, 9, 257, 64 and 300
    frames — the edges of the 128-frame tiles of the PCM and multiband kernels.  The resampler is (147, 160, 48), the PCM stage 16
    bits with triangular dither and nine taps; the master fader alternates, snapped, between 1 and 0.125.  Outputs, integers, clips
    and the multiband's minima are compared behind every fill, the states at every fourth subset's round trip and at the end."""
    setup, steps = pw.master_subset_walk()
    chain, got = play(setup, steps, "the master subset walk")
    fills = [(dev, want) for _, dev, want, x in got if x is not None]
    assert len(fills) == 48 and all("master" in dev for dev, _ in fills)
    # each of the four stages is on in 24 of the fills, and each reading is compared there
    for key in ("loudness rows", "spectrum rows", "resampled", "pcm"):
        assert sum(key in dev for dev, _ in fills) == 24, key
    assert sum("multiband meters" in dev for dev, _ in fills) == 24 and sum("gain" in want for _, want in fills) == 32
    # the PCM stage behind the resampler makes the resampler's count of frames, a call of one frame included
    both = [(dev, want) for dev, want in fills if "resampled" in dev and "pcm" in dev]
    assert len(both) == 12 and all(dev["pcm"].shape == (9, want["count"], 2) == dev["resampled"].shape for dev, want in both)
